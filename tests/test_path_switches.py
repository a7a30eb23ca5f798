"""The opt-in path switches of ConvNetwork as one table of outcomes (host only: the predicates are library queries).

For six networks plus one with int8 weights, every ordered pair of the thirteen switch settings (the twelve
switches with True, and band_learning_path = 2) is applied to a clean network and
the first is then switched off again; the outcome of each assignment (`ok`, or the exception class and the kind of refusal) and the
twelve property values after each stage are compared with tests/path_switch_expected.json.  That file was recorded with this
module's `record()` (`python tests/test_path_switches.py`) at the commit it names, which predates the registry in
snn_modulation_classification_amd/paths.py: the matrix and the environment cases use only names that commit has.  The per-object
views and the old `ops` keywords are checked against what that commit's code did, written out below.
"""
import contextlib
import copy
import io
import itertools
import json
import os
import re
from argparse import Namespace

import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "snn_modulation_classification_amd")
EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "path_switch_expected.json")

NAMES = ["any_learning_path", "wide_learning_path", "slab_learning_path", "band_learning_path", "any_step_path", "wide_step_path",
         "slab_step_path", "w3_step_path", "w3_first_wgrad", "w3_dv_path", "pool_dv_path", "native_optim_path"]
SETTINGS = [(n, True) for n in NAMES] + [("band_learning_path", 2)]
# name -> (yaml, plane, netscale, classes, int8 weights)
NETS = {"radio16_ns1": ("radio_ml_conv.yaml", (16, 16), 1, 24, False), "radio16_ns2": ("radio_ml_conv.yaml", (16, 16), 2, 24, False),
        "radio16_ns3": ("radio_ml_conv.yaml", (16, 16), 3, 24, False), "radio24x40_ns2": ("radio_ml_conv.yaml", (24, 40), 2, 24, False),
        "mnist_ns1": ("mnist_conv.yaml", (28, 28), 1, 10, False), "ref16x128": ("radio_ml_conv_ref.yaml", (16, 128), 1, 24, False),
        "radio16_ns1_int8": ("radio_ml_conv.yaml", (16, 16), 1, 24, True)}
# native_optim_path serves Adamax; the MNIST network gets an optimizer it refuses
OPTIMIZER = {False: dict(opt=torch.optim.Adamax, opt_param={"betas": [0.0, 0.95]}), True: dict(opt=torch.optim.RMSprop, opt_param={})}
ENV = ["DCLL_ANY_STEP_PATH", "DCLL_WIDE_STEP_PATH", "DCLL_SLAB_STEP_PATH"]


def kind(msg):
    for k, pat in (("combined", "combined"), ("needs", " needs "), ("band count", "band count"),
                   ("not served", "does not serve|do not serve|is not served")):
        if re.search(pat, msg):
            return k
    return "other: " + msg


def state(net):
    """the property values as one character each: 0 / 1, or the band count"""
    return "".join(str(int(v)) if v is not True else "1" for v in (getattr(net, n) for n in NAMES))


def assign(net, name, value):
    try:
        setattr(net, name, value)
        return "ok"
    except Exception as e:          # (the class is part of the outcome)
        return "%s: %s" % (type(e).__name__, kind(str(e)))


def all_off(net):
    for n in NAMES:
        setattr(net, n, False)
    assert state(net) == "0" * len(NAMES)


def build(key):
    from snn_modulation_classification_amd import quant
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    yaml, plane, netscale, classes, int8 = NETS[key]
    args = Namespace(netscale=netscale, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    torch.manual_seed(1)
    net = ConvNetwork(args, (1,) + plane, 2, load_network_spec(os.path.join(PKG, "networks", yaml)), classes,
                      act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss, **OPTIMIZER[yaml == "mnist_conv.yaml"],
                      learning_rates=None, burnin=2)
    if int8:
        quant.apply_int8_weights(net)
    return net


def matrix(net):
    out = {}
    for (a, va), (b, vb) in itertools.product(SETTINGS, SETTINGS):
        all_off(net)
        row = []
        for n, v in ((a, va), (b, vb), (a, False)):
            row += [assign(net, n, v), state(net)]
        out["%s=%s, %s=%s" % (a, va, b, vb)] = row
    all_off(net)
    return out


def environment(net, monkeypatch_env, int8=False):
    """the three variables alone and in pairs, each on a network that has not looked yet: the notices of its first reset(True), the
    state behind it, and the state after everything is switched off and reset(True) runs again (looked at once per network)"""
    from snn_modulation_classification_amd import quant
    out = {}
    for combo in [c for r in (1, 2) for c in itertools.combinations(ENV, r)]:
        fresh = copy.deepcopy(net)
        if int8:                            # (the int8 form describes the tensor it was taken from, not its copy)
            quant.apply_int8_weights(fresh)
        with monkeypatch_env(combo), contextlib.redirect_stdout(io.StringIO()) as text:
            fresh.reset(True)
            first = state(fresh)
            all_off(fresh)
            fresh.reset(True)
        notices = ["%s: %s" % (l.split(" ignored")[0], "another path" if "another per-step path" in l else kind(l))
                   for l in text.getvalue().splitlines() if "ignored" in l]
        out[" + ".join(combo)] = [notices, first, state(fresh)]
    return out


@contextlib.contextmanager
def _environ(names):
    old = {n: os.environ.get(n) for n in ENV}
    try:
        for n in ENV:
            os.environ.pop(n, None)
        for n in names:
            os.environ[n] = "1"
        yield
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


def observe(key):
    from snn_modulation_classification_amd.dcll import pytorch_libdcll as L
    old, L.device = L.device, "cpu"
    try:
        with _environ(()):
            net = build(key)
            return dict(matrix=matrix(net), environment=environment(net, _environ, NETS[key][4]))
    finally:
        L.device = old


OUTCOMES = ["ok", "DCLLUnsupported: combined", "DCLLUnsupported: not served", "DCLLUnsupported: needs", "DCLLUnsupported: band count"]
LABELS = ["%s=%s" % s for s in SETTINGS]


def pack(doc):
    """The recording as the text of tests/path_switch_expected.json: per network one line per first setting, holding for each second
    setting the three stages as '<index into OUTCOMES>:<state>', and one line per environment case."""
    out = ['{"recorded_at": %s,' % json.dumps(doc["recorded_at"]), '"names": %s,' % json.dumps(NAMES),
           '"settings": %s,' % json.dumps(LABELS), '"outcomes": %s,' % json.dumps(OUTCOMES), '"networks": {']
    for key, net in sorted(doc["networks"].items()):
        out.append('%s: {"matrix": {' % json.dumps(key))
        for a in LABELS:
            rows = [net["matrix"]["%s, %s" % (a, b)] for b in LABELS]
            cells = [" ".join("%d:%s" % (OUTCOMES.index(o), st) for o, st in zip(r[0::2], r[1::2])) for r in rows]
            out.append('%s: %s,' % (json.dumps(a), json.dumps(cells)))
        out[-1] = out[-1][:-1] + '}, "environment": {'
        out += ['%s: %s,' % (json.dumps(c), json.dumps(v)) for c, v in sorted(net["environment"].items())]
        out[-1] = out[-1][:-1] + '}},'
    out[-1] = out[-1][:-1] + '}}'
    return "\n".join(out) + "\n"


def unpack(text):
    """pack's text -> {network: {"matrix": {"a, b": [outcome, state] x 3}, "environment": ...}}, what observe() returns"""
    doc = json.loads(text)
    assert doc["names"] == NAMES and doc["settings"] == LABELS
    nets = {}
    for key, net in doc["networks"].items():
        m = {}
        for a, cells in net["matrix"].items():
            for b, cell in zip(LABELS, cells):
                m["%s, %s" % (a, b)] = [x for stage in cell.split(" ")
                                         for x in (doc["outcomes"][int(stage.split(":")[0])], stage.split(":")[1])]
        nets[key] = dict(matrix=m, environment=net["environment"])
    return nets


def record():
    import subprocess
    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=PKG).stdout.strip()
    doc = dict(recorded_at="commit %s, by tests/test_path_switches.py record()" % commit, networks={k: observe(k) for k in NETS})
    assert unpack(pack(doc)) == doc["networks"]
    with open(EXPECTED, "w") as f:
        f.write(pack(doc))


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return unpack(f.read())


@pytest.fixture(scope="module")
def observed():
    cache = {}
    return lambda key: cache[key] if key in cache else cache.setdefault(key, observe(key))


@pytest.mark.parametrize("key", list(NETS))
def test_every_ordered_pair_of_settings_ends_as_recorded(key, expected, observed):
    got, want = observed(key)["matrix"], expected[key]["matrix"]
    assert len(got) == len(SETTINGS) ** 2 and set(got) == set(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, "%d of %d pairs differ, e.g. %s" % (len(bad), len(want), list(bad.items())[:3])


@pytest.mark.parametrize("key", list(NETS))
def test_environment_variables_alone_and_in_pairs(key, expected, observed):
    assert observed(key)["environment"] == expected[key]["environment"]


def test_the_recorded_matrix_reaches_every_kind_of_refusal(expected):
    """what the case list is for: every refusal kind, and a `does not serve` from every path's predicate (the slab step's on the
    int8 network only: it serves the six others)"""
    seen = {o for net in expected.values() for row in net["matrix"].values() for o in row[0::2]}
    assert seen == {"ok", "DCLLUnsupported: combined", "DCLLUnsupported: not served", "DCLLUnsupported: needs"}, seen
    for name in NAMES[:8] + ["native_optim_path"]:
        pairs = ["%s=%s, %s=%s" % (n, v, n, v) for n, v in SETTINGS if n == name]      # (the first of a pair meets a clean network)
        assert any(net["matrix"][p][0] == "DCLLUnsupported: not served" for net in expected.values() for p in pairs), name
    assert expected["radio16_ns1_int8"]["matrix"]["slab_step_path=True, slab_step_path=True"][0] == "DCLLUnsupported: not served"
    notices = {n.split(": ", 1)[1] for net in expected.values() for row in net["environment"].values() for n in row[0]}
    assert notices == {"another path", "not served"}


@pytest.fixture
def net16():
    from snn_modulation_classification_amd.dcll import pytorch_libdcll as L
    old, L.device = L.device, "cpu"
    try:
        with _environ(()):
            yield build("radio16_ns1")
    finally:
        L.device = old


def test_a_negative_band_count_is_refused_before_anything_else(net16):
    from snn_modulation_classification_amd._lib import DCLLUnsupported
    net16.any_learning_path = True
    with pytest.raises(DCLLUnsupported, match="band count"):
        net16.band_learning_path = -1
    assert net16.any_learning_path is True and net16.band_learning_path is False
    net16.any_learning_path = False
    net16.band_learning_path = 0            # (0 bands: the library's rule)
    assert net16.band_learning_path is True


def test_per_object_views_are_one_state_per_axis(net16):
    from snn_modulation_classification_amd._lib import DCLLUnsupported
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    assert DCLLBase.pool_dv is False and DCLLBase.w3_dv is False and DCLLBase.native_optimizers is False
    s = net16.dcll_slices[0]
    i2h = s.dclllayer.i2h
    assert (s.learning_path, i2h.step_path) == (None, None)
    s.slab_learning_path = True
    assert s.learning_path == "slab" and s.slab_learning_path is True and net16.slab_learning_path is False
    with pytest.raises(DCLLUnsupported, match="combined"):
        net16.w3_step_path = True
    s.wide_learning_path = True             # (a sibling on the same axis: the slab view reads False from here on)
    assert s.learning_path == "wide" and s.slab_learning_path is False
    s.slab_learning_path = False            # (not the selected path: nothing is cleared)
    assert s.wide_learning_path is True
    s.wide_learning_path = False
    assert s.learning_path is None
    for v, count in ((False, 0), (True, 0), (24, 24)):
        s.band_learning_path = v
        assert s.band_learning_path is v or s.band_learning_path == v and type(s.band_learning_path) is type(v)
        assert s._band_count() == count
    s.w3_learning_path = True
    assert s.band_learning_path is False and s._band_count() == 0 and s.w3_learning_path is True
    s.w3_learning_path = False
    for view, key in (("any_step_path", "any"), ("wide_step_path", "wide"), ("slab_step_path", "slab"), ("w3_step_path", "w3")):
        setattr(i2h, view, True)
        assert i2h.step_path == key and [getattr(i2h, v + "_step_path") for v in ("any", "wide", "slab", "w3")].count(True) == 1
    i2h.any_step_path = False
    assert i2h.step_path == "w3"
    i2h.w3_step_path = False
    assert i2h.step_path is None and state(net16) == "0" * len(NAMES)


# what the code before the registry chose for the old keywords of ops.conv_lif_step / ops.conv_lif_backward
STEP_ENTRY = {(): "dcll_conv_lif_step", ("any_path",): "dcll_conv_lif_step_any", ("wide_path",): "dcll_conv_lif_step_wide",
              ("slab_path",): "dcll_conv_lif_step_slab", ("w3_path",): "dcll_conv_lif_step_w3"}
BWD_ENTRY = {(): "dcll_conv_lif_backward", ("any_path",): "dcll_conv_lif_backward_any", ("wide_path",): "dcll_conv_lif_backward_wide",
             ("slab_path",): "dcll_conv_lif_backward_slab", ("band_path",): "dcll_conv_lif_backward_bands",
             ("w3_path",): "dcll_conv_lif_backward_w3", ("w3_path", "w3_first"): "dcll_conv_lif_backward_w3f",
             ("w3_path", "w3_dv"): "dcll_conv_lif_backward_w3_ex", ("w3_path", "w3_first", "w3_dv"): "dcll_conv_lif_backward_w3_ex"}
BWD_ENTRY.update({k + ("pool_dv",): "dcll_conv_lif_backward_ex" for k in list(BWD_ENTRY) if "w3_path" not in k})


def test_old_ops_keywords_resolve_to_the_entry_points_they_always_chose():
    from snn_modulation_classification_amd import ops, paths
    for kw, fn in STEP_ENTRY.items():
        path, bands = ops.legacy_path("step", None, 0, **{k: True for k in kw})
        assert paths.STEP_CALLS[path][0] == fn and bands == 0
    assert ops.legacy_path("step", None, 3, slab_path=True) == ("slab", 3) == ops.legacy_path("step", "slab", 3)
    for kw, fn in BWD_ENTRY.items():
        mods = {k: k in kw for k in ("w3_first", "w3_dv", "pool_dv")}
        path, bands = ops.legacy_path("backward", None, 0, **{k: True for k in kw})
        assert ops.backward_entry(path, **mods) == fn, kw
    assert ops.legacy_path("backward", None, 5, band_path=True) == ("band", 5) == ops.legacy_path("backward", "band", 5)
    paths_of = ("any_path", "wide_path", "slab_path", "w3_path")
    for where, names in (("step", paths_of), ("backward", paths_of + ("band_path",))):
        for a, b in itertools.combinations(names, 2):           # two paths at once
            with pytest.raises(ValueError):
                ops.legacy_path(where, None, 0, **{a: True, b: True})
        for a in names:                                         # ... one of them given as path=
            with pytest.raises(ValueError):
                ops.legacy_path(where, "w3" if a != "w3_path" else "any", 0, **{a: True})
    for where, kw in (("step", {}), ("step", dict(any_path=True)), ("backward", {}), ("backward", dict(slab_path=True))):
        with pytest.raises(ValueError):                         # a band count without its path
            ops.legacy_path(where, None, 2, **kw)
    for kw in (dict(w3_first=True), dict(w3_dv=True), dict(w3_first=True, any_path=True), dict(w3_dv=True, band_path=True),
               dict(pool_dv=True, w3_path=True)):
        with pytest.raises(ValueError):                         # a rider without w3_path; pool_dv with it
            ops.legacy_path("backward", None, 0, **kw)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(PKG))
    record()
