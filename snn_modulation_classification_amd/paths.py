"""The opt-in kernel paths as one table: which per-step path, which learning path, which modifiers, and what excludes what.

A Conv2dDCLLlayer's convolution holds ONE per-step path (`i2h.step_path`: None, 'any', 'wide', 'slab', 'w3') and a slice ONE learning
path (`s.learning_path`: None, 'any', 'wide', 'slab', 'band', 'w3'; `s.learning_bands` goes with 'band', 0 = the library's rule), so two
paths on one axis cannot be on together.  The modifiers are booleans on the slice.  PATHS has one entry per switch of ConvNetwork, in
the order train.py applies its flags; ConvNetwork's properties, its environment variables, train.py's flags and the keywords of
ops.conv_lif_step / ops.conv_lif_backward are all read from here.  A new path is one entry here (and one row in STEP_CALLS or
BACKWARD_CALLS), its predicate in ops, and the help text of its flag in train.py.
"""
from collections import namedtuple
from inspect import cleandoc

# name: the ConvNetwork property; axis: 'step', 'learning', 'both' or 'modifier'; key: the axis' state, for a modifier the slice's
# attribute; entry: the C entry point(s) the path calls; supported: the ConvNetwork / slice method that asks ops' predicate(s) for
# every layer; rides_on: the switch that must be on first; excludes: switches beyond the own axis that cannot be on with it; env: the
# environment variable that sets it at the network's first reset(True); kernel: what train.py's notices call it; doc: the property's
# docstring.  The flag of train.py is '--' + name.
Path = namedtuple('Path', 'name axis key entry supported rides_on excludes env kernel doc')


def _path(name, axis, key, doc, entry=None, supported=None, rides_on=None, excludes=(), env=None, kernel=None):
    return Path(name, axis, key, entry, supported, rides_on, excludes, env, kernel or entry, cleandoc(doc))


PATHS = (
    _path('any_learning_path', 'learning', 'any', entry='dcll_conv_lif_backward_any', supported='backward_any_supported',
          kernel='k_bwd_wgrad_any', doc="""
          True: every slice's learning step takes its weight gradient from k_bwd_wgrad_any (fp32 MFMA, any plain conv layer with
          c_out <= 32 and a kernel up to 16x16 — also layers above 64 taps, which the default path refuses) instead of the
          default dispatch.  The step's structure is unchanged: layer kernels, tails, one dcll_grad_reduce_adam.  Default False;
          setting it on a network that is not fully served raises DCLLUnsupported."""),
    _path('any_step_path', 'step', 'any', entry='dcll_conv_lif_step_any', supported='step_any_supported', env='DCLL_ANY_STEP_PATH',
          kernel='k_lif_step_any', doc="""
          True: every per-step layer call — net.test(x[t]), every learning timestep, Conv2dDCLLlayer.forward, the autograd
          nodes — runs k_lif_step_any (one fp32-MFMA launch with the traces and the pooling fused in; any plain conv layer with
          c_out <= 32 and a kernel up to 16x16) instead of dcll_conv_lif_step's dispatch.  The readout tails and the sequence
          calls (test_sequence, test_sequence_any) are untouched.  Default False; setting it on a network that is not fully
          served (c_out 64, int8 weights) raises DCLLUnsupported.  DCLL_ANY_STEP_PATH=1 in the environment sets it at the network's
          first reset(True), for the entry points without a flag of their own (`DCLL_ANY_STEP_PATH=1 python test_radio_ml.py
          --no_sequence_path` runs its per-step loop on k_lif_step_any); ignored with a notice where a layer is not served."""),
    _path('w3_step_path', 'both', 'w3', entry='dcll_conv_lif_step_w3 / dcll_conv_lif_backward_w3', supported='w3_step_supported',
          excludes=('pool_dv_path',), kernel='k_lif_step_w3 / k_bwd_wgrad_w3', doc="""
          True: every per-step layer call — net.test(x[t]), every learning timestep, Conv2dDCLLlayer.forward — runs
          k_lif_step_w3 (traces, fp32-MFMA chains and the (1,2) pooling in one launch) instead of dcll_conv_lif_step's k_trace +
          k_conv_lif_tiled<1,3> + k_pool, and every learning step takes the weight gradient of its 64 -> 64 layers from
          k_bwd_wgrad_w3 instead of k_bwd_wgrad.  One switch for both halves.  The readout tails and the sequence calls
          (test_sequence, the burn-in of learn_sequence) are untouched.  Default False; setting it on a network with a layer that
          is not served (other geometry, int8 weights, netscale != 1, general-option layers) or together with any other per-step
          or learning path or pool_dv_path raises DCLLUnsupported and leaves it off; switching it off is always allowed, and
          clears w3_first_wgrad and w3_dv_path."""),
    _path('w3_first_wgrad', 'modifier', 'w3_first_wgrad', rides_on='w3_step_path', doc="""
          True: with w3_step_path, the first layer (c_in 1 -> 64) takes its weight gradient from k_bwd_wgrad_w3f (a register-only
          streaming reduction of the dv plane; dcll_conv_lif_backward_w3f[_open]) instead of the generic k_bwd_wgrad; the 64 -> 64
          layers and everything else are w3_step_path's.  That layer's dW / db are then summed in another order (not bit-identical,
          inside the weight-gradient tolerance).  Default False; setting it True while w3_step_path is off raises DCLLUnsupported
          and leaves it off; w3_step_path = False clears it; switching it off is always allowed."""),
    _path('w3_dv_path', 'modifier', 'w3_dv', rides_on='w3_step_path', doc="""
          True: with w3_step_path, every layer's backward takes its dv plane from k_bwd_dv_w3 (a streaming form of k_bwd_dv for
          the (1,2) pooling of these layers; dcll_conv_lif_backward_w3_ex[_open] with DCLL_W3_DV) instead of the generic k_bwd_dv.
          The plane is bit-identical, so spikes, state, every gradient and the parameters after Adam are the bits of the same network
          without it.  Independent of w3_first_wgrad.  Default False; setting it True while w3_step_path is off raises
          DCLLUnsupported and leaves it off; w3_step_path = False clears it; switching it off is always allowed."""),
    _path('wide_step_path', 'step', 'wide', entry='dcll_conv_lif_step_wide', supported='step_wide_supported', env='DCLL_WIDE_STEP_PATH',
          kernel='k_lif_step_wide', doc="""
          True: every per-step layer call — net.test(x[t]), every learning timestep, Conv2dDCLLlayer.forward, the autograd
          nodes — runs dcll_conv_lif_step_wide: k_lif_step_wide (k_lif_step_any's form with two 32-row M tiles) for the layers of
          33 .. 64 output channels that a netscale above 1 makes, k_lif_step_any for the narrower ones, instead of
          dcll_conv_lif_step's dispatch.  The readout tails and the sequence calls are untouched; combines with every learning path
          but w3_step_path's.  Default False; setting it on a network that is not fully served (c_out above 64, int8 weights), or
          together with another per-step path, raises DCLLUnsupported and leaves it off; switching it off is always allowed.
          DCLL_WIDE_STEP_PATH=1 sets it like DCLL_ANY_STEP_PATH=1 does any_step_path; ignored with a notice where a layer is not
          served or another per-step path is already on (DCLL_ANY_STEP_PATH=1 wins where it is served)."""),
    _path('slab_step_path', 'step', 'slab', entry='dcll_conv_lif_step_slab', supported='step_slab_supported', env='DCLL_SLAB_STEP_PATH',
          kernel='k_lif_step_slab', doc="""
          True: every per-step layer call — net.test(x[t]), every learning timestep, Conv2dDCLLlayer.forward, the autograd
          nodes — runs dcll_conv_lif_step_slab: k_lif_step_slab (k_lif_step_wide's chains over B x bands of rows x slabs of 64
          output channels) for the layers of more than 64 output channels that a netscale above 2 makes and for the planes whose
          padded eps1 image exceeds a workgroup's LDS, dcll_conv_lif_step_wide's kernels for the layers that call serves, instead
          of dcll_conv_lif_step's dispatch.  The readout tails and the sequence calls are untouched; combines with every learning
          path but w3_step_path's.  Default False; setting it on a network that is not fully served (int8 weights, general-option
          layers, a plane of which not one pooled row fits), or together with another per-step path, raises DCLLUnsupported and
          leaves it off; switching it off is always allowed.  DCLL_SLAB_STEP_PATH=1 sets it by DCLL_WIDE_STEP_PATH's rule."""),
    _path('wide_learning_path', 'learning', 'wide', entry='dcll_conv_lif_backward_wide', supported='backward_wide_supported', doc="""
          True: every slice's learning step takes its weight gradient from dcll_conv_lif_backward_wide — k_bwd_wgrad_wide (fp32
          MFMA, two 32-row M tiles) for the layers of 33 .. 64 output channels that a netscale above 1 makes, k_bwd_wgrad_any for
          the narrower ones — instead of the default dispatch.  The step's structure is unchanged: layer kernels, tails, one
          dcll_grad_reduce_adam.  Default False; setting it on a network that is not fully served, or together with another
          learning path (w3_step_path is one), raises DCLLUnsupported and leaves it off; switching it off is always allowed."""),
    _path('slab_learning_path', 'learning', 'slab', entry='dcll_conv_lif_backward_slab', supported='backward_slab_supported', doc="""
          True: every slice's learning step takes its weight gradient from dcll_conv_lif_backward_slab — k_bwd_wgrad_slab (fp32
          MFMA, one slab of 64 output channels per workgroup) for the layers of more than 64 output channels that a netscale above
          2 makes, k_bwd_wgrad_wide / k_bwd_wgrad_any for the narrower ones — instead of the default dispatch.  The step's structure
          is unchanged: layer kernels, tails, one dcll_grad_reduce_adam.  Default False; setting it on a network that is not fully
          served, or together with another learning path (w3_step_path is one), raises DCLLUnsupported and leaves it off; switching
          it off is always allowed."""),
    _path('band_learning_path', 'learning', 'band', entry='dcll_conv_lif_backward_bands', supported='backward_bands_supported', doc="""
          False, True or an int N.  True: every slice's learning step takes its weight gradient from dcll_conv_lif_backward_bands —
          k_bwd_wgrad_band (fp32 MFMA, a sample cut into bands of conv-output rows: LDS does not grow with the plane height) for the
          layers whose sample the slab path cannot stage, dcll_conv_lif_backward_slab's kernels for the layers that call serves —
          instead of the default dispatch.  An int N >= 2: exactly N bands per sample in every slice (1: the slab call itself; 0:
          True).  The step's structure is unchanged: layer kernels, tails, one dcll_grad_reduce_adam.  Default False; a negative
          count, a network with a slice that is not served, or another learning path (w3_step_path is one) raises DCLLUnsupported and
          leaves it as it was; switching it off is always allowed.  Combines with any_step_path, wide_step_path and slab_step_path."""),
    _path('pool_dv_path', 'modifier', 'pool_dv', excludes=('w3_step_path',), doc="""
          True: every learning step makes its backward call through dcll_conv_lif_backward_ex[_open] with DCLL_BWD_POOL_DV — the path
          is the one the learning-path switches select — so a layer that pools takes its dv plane from k_bwd_dv_pool (a streaming form
          of k_bwd_dv: a thread owns a pooled window) where ops.bwd_dv_pool_supported holds; a layer without pooling, or an unserved
          one, keeps its kernel.  The plane is bit-identical, so every gradient and the parameters after Adam are the bits of the same
          network without it.  Combines with every learning path and every step path except w3_step_path (which has w3_dv_path):
          setting it True under w3_step_path raises DCLLUnsupported and leaves it off, and so does w3_step_path = True under it.
          Default False; switching it off is always allowed."""),
    _path('native_optim_path', 'modifier', 'native_optimizers', doc="""
          True: the native learning step also serves slices whose optimizer is torch.optim.SGD, Adamax, AdamW, or Adam / AdamW with
          amsgrad (DCLLBase.native_optimizers): their update is applied by k_grad_reduce_optim / k_optim_multi on the state tensors of
          the torch optimizer objects, as torch's _single_tensor_* functions state it, instead of the whole step running under
          autograd.  A network of plain Adam slices keeps its calls and its bits.  Combines with every learning, per-step and dv
          path.  Default False (DCLL_NATIVE_OPTIM=1 sets it at construction); setting it True where a slice's optimizer is none of
          DCLLBase.NATIVE_OPTIMIZERS, or uses maximize / capturable / fused / differentiable / a tensor lr or weight_decay, raises
          DCLLUnsupported and leaves it as it was; switching it off is always allowed."""),
)
BY_NAME = {p.name: p for p in PATHS}
AXIS_NOUN = {'step': 'per-step', 'learning': 'learning', 'both': 'learning'}

# ops.conv_lif_step: path -> (entry point, the query of its w_scratch floats or None, its arguments between `v` and `B`)
STEP_CALLS = {None: ('dcll_conv_lif_step', None, ('scratch', 'opts')),
              'any': ('dcll_conv_lif_step_any', 'dcll_conv_lif_step_any_scratch', ('w_scratch',)),
              'wide': ('dcll_conv_lif_step_wide', 'dcll_conv_lif_step_wide_scratch', ('w_scratch',)),
              'slab': ('dcll_conv_lif_step_slab', 'dcll_conv_lif_step_slab_scratch', ('w_scratch', 'bands')),
              'w3': ('dcll_conv_lif_step_w3', None, ())}
# ops.conv_lif_backward: path -> (entry point, `path` of dcll_conv_lif_backward_ex or None, the rule of its partial-row count:
# ops._BWD_CHUNKS).  w3_first / w3_dv / pool_dv choose among a path's entry points in ops.backward_entry.
BACKWARD_CALLS = {None: ('dcll_conv_lif_backward', 0, 'jobs'), 'any': ('dcll_conv_lif_backward_any', 1, 'batch'),
                  'wide': ('dcll_conv_lif_backward_wide', 2, 'batch'), 'slab': ('dcll_conv_lif_backward_slab', 3, 'batch'),
                  'band': ('dcll_conv_lif_backward_bands', 4, 'plan'), 'w3': ('dcll_conv_lif_backward_w3', None, 'w3')}
# the old boolean keywords of both functions -> the path they stand for
LEGACY_KEYWORDS = {'any_path': 'any', 'wide_path': 'wide', 'slab_path': 'slab', 'band_path': 'band', 'w3_path': 'w3'}


class view:
    """The old per-object attribute of one path (`i2h.any_step_path`, `s.slab_learning_path`, ...) as a view of the axis' one state
    `attr`: reads True where `key` is selected; writing True selects it, writing False clears the axis only if `key` is selected.
    On the class it reads False, the default the attribute had."""

    def __init__(self, attr, key):
        self.attr, self.key = attr, key

    def __get__(self, obj, cls=None):
        return obj is not None and getattr(obj, self.attr) == self.key

    def __set__(self, obj, on):
        if on:
            setattr(obj, self.attr, self.key)
        elif getattr(obj, self.attr) == self.key:
            setattr(obj, self.attr, None)


class band_view(view):
    """DCLLBase.band_learning_path, False | True | N, as a view of (learning_path, learning_bands): True = 0 bands, the library's rule"""

    def __init__(self):
        view.__init__(self, 'learning_path', 'band')

    def __get__(self, obj, cls=None):
        return view.__get__(self, obj) and (obj.learning_bands or True)

    def __set__(self, obj, on):
        view.__set__(self, obj, on is not None and on is not False)
        if obj.learning_path == 'band':
            obj.learning_bands = 0 if on is True else int(on)


# -- the switches of a ConvNetwork `net` ------------------------------------------------------------------------------------------------
def _halves(s, p):
    """Switch `p` in slice `s`: one boolean per axis it is on (w3_step_path: two), a modifier's own one"""
    return (([s.dclllayer.i2h.step_path == p.key] if p.axis in ('step', 'both') else []) +
            ([s.learning_path == p.key] if p.axis in ('learning', 'both') else [])) or [bool(getattr(s, p.key))]


def value(net, p):
    """What `net.<p.name>` reads: True where every slice has it (both halves of w3_step_path); band_learning_path: the slices'
    common True | N."""
    S = net.dcll_slices
    on = all(all(_halves(s, p)) for s in S)
    if on and p.key == 'band':
        return len({s.learning_bands for s in S}) == 1 and S[0].band_learning_path
    return on


def in_the_way(net, p):
    """The switches that are on in some slice and cannot be combined with `p`: the other paths of its axis (w3_step_path is on both)
    and what either names in `excludes`."""
    def clash(q):
        same_axis = 'modifier' not in (p.axis, q.axis) and (p.axis == q.axis or 'both' in (p.axis, q.axis))
        return same_axis or q.name in p.excludes or p.name in q.excludes
    return [q for q in PATHS if q is not p and clash(q) and any(any(_halves(s, q)) for s in net.dcll_slices)]


def refusal(net, p, v):
    """Why `net.<p.name> = v` (v: True, or a band count) is refused -> (kind, detail) or None, in the order the checks have always
    had: 'band count'; 'needs' (the switch it rides on); 'combined' (the switches in the way); 'not served' (what does not serve it)."""
    if p.key == 'band' and v is not True and v < 0:
        return 'band count', None
    if p.rides_on and not value(net, BY_NAME[p.rides_on]):
        return 'needs', BY_NAME[p.rides_on]
    clash = in_the_way(net, p)
    if clash:
        return 'combined', clash
    if p.name == 'native_optim_path':
        bad = net._optimizer_not_served()
        return bad and ('not served', bad)
    if p.supported and not getattr(net, p.supported)(*((0 if v is True else v,) if p.key == 'band' else ())):
        return 'not served', None
    return None


def serves(what):
    return '%s %s not serve every layer of this network' % (what, 'do' if ' / ' in what else 'does')


def refusal_text(p, why):
    """The message of the DCLLUnsupported a refused `net.<p.name> = ...` raises"""
    kind, detail = why
    if kind == 'band count':
        return 'band_learning_path: a band count is >= 0'
    if kind == 'needs':
        return '%s needs %s (set it first)' % (p.name, detail.name)
    if kind == 'combined':
        return '%s cannot be combined with %s' % (p.name, ' / '.join(q.name for q in detail))
    return '%s: %s is not served' % (p.name, detail) if detail else serves(p.entry)


def notice_text(p, why, v=True, given=True, prefix='--'):
    """What follows '<flag or variable> ignored: ' where train.py (prefix '--') or the environment (prefix '') meets that refusal;
    `given`: whether the flag of the switch it rides on was given"""
    kind, detail = why
    if kind == 'band count':
        return 'a band count is >= 0'
    if kind == 'needs':
        return 'it rides on --%s, which is %s' % (detail.name, 'not in effect on this network' if given else 'not given')
    if kind == 'combined':
        names = ' / '.join(prefix + q.name for q in detail)
        if all(q.name in p.excludes for q in detail):
            return '%s is in effect' % names
        return 'another %s path (%s) is %s' % (AXIS_NOUN[p.axis], names, 'in effect' if prefix else 'on')
    return '%s is not served' % detail if detail else serves(p.kernel) + (' with %d bands' % v if p.key == 'band' and v is not True else '')


def assign(net, p, v):
    """`net.<p.name> = v`: normalise, check (refusal), then write every slice; nothing is written if a check fails.  The state is
    part of ConvNetwork._graph_signature / _test_signature: a captured timestep of another path is retaken."""
    from ._lib import DCLLUnsupported
    if p.key == 'band':
        v = False if v is None or v is False else True if v is True or int(v) == 0 else int(v)
    else:
        v = bool(v)
    why = refusal(net, p, v) if v is not False else None
    if why:
        raise DCLLUnsupported(refusal_text(p, why))
    for s in net.dcll_slices:
        if p.axis == 'modifier':
            setattr(s, p.key, v)
            continue
        if p.axis in ('step', 'both'):          # (through the views: False clears an axis only where this path is the one selected)
            setattr(s.dclllayer.i2h, p.key + '_step_path', v)
        if p.axis in ('learning', 'both'):
            setattr(s, p.key + '_learning_path', v)
        if not v:
            for q in PATHS:                     # (what rides on it goes with it)
                if q.rides_on == p.name:
                    setattr(s, q.key, False)


def from_environment(net):
    """The entries with an environment variable, in table order, at the network's first reset(True) that sees the variable set (not
    '' or 0): `net.<name> = True`, or a notice where that would be refused.  Looked at once per network and variable, so a later
    `net.<name> = False` holds."""
    import os
    seen = net.__dict__.setdefault('_path_env_seen', set())
    for p in PATHS:
        if p.env and p.env not in seen and os.environ.get(p.env, '0') not in ('', '0'):
            seen.add(p.env)
            why = refusal(net, p, True)
            if why:
                print('%s ignored: %s' % (p.env, notice_text(p, why, prefix='')))
            else:
                assign(net, p, True)


def network_property(p):
    return property(lambda net: value(net, p), lambda net, v: assign(net, p, v), doc=p.doc)
