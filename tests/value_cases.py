"""Value-domain cases for every forward kernel family: subnormal traces, membranes exactly on +-0 / +-2^-149 / saturating values,
real-valued input.  The sibling lists (fuzz_cases, seq_fuzz_cases, step_any_cases, step_w3_cases, seq_any_cases, seq_wide_cases)
cover geometry, dispatch and alignment and draw every value from one narrow region (0/1 input, state in [0, 12), std(v) = 2); this
list takes its GEOMETRY from them — per forward kernel variant the smallest existing case that reaches it, B cut to <= 3 — and
replaces only the DRAW.  Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.
tests/test_value_cases.py proves on the CPU that the list means what it says; tests/test_gpu_values.py runs the HIP kernels.

A case is the source case's dict + kind, src (the sibling module), family (the kernel it is aimed at), alpharp, steps (per-step
entries) and a sub-seed; run(c) draws its tensors IN THE SOURCE MODULE'S FORMAT (so that the source's device runner takes them
as they are) and steps the pinned-order C oracle through them.  Re-run one alone:
    python -c "import value_cases as V; print(V.describe(V.by_id('val-seq-k_lif_seq_w3-decay-R1')))"

Kinds (time constants and alpharp are call inputs: alpha, alphas per input channel from {.5, .75, .9, .97}, tau = 1 / (1 - alpha)):
  decay      silent input (first layers fed by cell indices: every spike into cell 0), eps0 / eps1 log-uniform over
             2^-149 ... 2^-120, arp = -(the same), weights randn * 2^124 (2^100 where cell 0 is fed: its trace is of order 100 and
             v must stay finite), bias +0 / -0 on the even output channels and ~.5 on the odd ones, plain and refractory;
  mixed      ordinary spikes and ordinary weights (std(v) = 2); a drawn half of the state elements is subnormal and silent;
  threshold  membranes exactly on TABLE at the first step (see _threshold), later steps follow the oracle;
  analog     real-valued x (entries whose x is float*): uniform(-2, 3) mixed with -1, .5, 2^-140, -2^-149, 1e10, -0."""
import hashlib
import json

import numpy as np

import fuzz_cases as FZ
import seq_any_cases as A
import seq_fuzz_cases as SF
import seq_wide_cases as WD
import step_any_cases as SA
import step_w3_cases as S3

SEED = 20318
KINDS = ("decay", "mixed", "threshold", "analog")
ALPHAS = np.array([.5, .75, .9, .97], np.float32)
TINY = np.float32(2.0 ** -149)
FLT_MAX = np.float32(np.finfo(np.float32).max)
MAGS = [2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 1, 17, 88, 89, 104, 1e30, 2.0 ** 126, float(FLT_MAX)]
# +0, -0, then +m, -m: index % 4 in (0, 1) lands on the channels with zero weights, (2, 3) on the cancelling pairs (_threshold)
TABLE = np.array([0.0, -0.0] + [s * m for m in MAGS for s in (1, -1)], np.float32)
TABLE_CAPPED = np.clip(TABLE, -np.float32(2.0 ** 126), np.float32(2.0 ** 126))      # 2 V stays finite: what a refractory neuron reaches
ANALOG_TABLE = np.array([-1, .5, 2.0 ** -140, -2.0 ** -149, 1e10, -0.0], np.float32)
W_DECAY, W_DECAY_FED = np.float32(2.0 ** 124), np.float32(2.0 ** 100)
SRC = {"fuzz": FZ, "fuzz-dense": FZ, "step-any": SA, "step-w3": S3, "seq": SF, "seq-any": A, "seq-wide": WD}

# (family = the kernel the case is aimed at, sibling module, source case, overrides of options (never of geometry), kernels the
#  launch log must name where the sibling has no predicted log)
_ROWS = [
    # per-step conv (dcll_conv_lif_step)
    ("k_trace + k_conv_lif", "fuzz", "conv-edge-tile-3x3-7x8", {}, ["k_trace", "k_conv_lif"]),
    ("k_conv_lif_tiled<3,3>", "fuzz", "conv-edge-tile-3x3-8x8", {}, ["k_trace", "k_conv_lif_tiled<3,3>"]),
    ("k_lif_step_c32", "fuzz", "conv-edge-ptr16-plane16", {}, ["k_lif_step_c32"]),
    ("k_lif_step_c32t (8-row tiles)", "fuzz", "conv-edge-k7-plane16", {}, ["k_trace4", "k_lif_step_c32t (8-row tiles)"]),
    ("k_lif_step_c1", "fuzz", "conv-edge-c1-plane16", {}, ["k_lif_step_c1"]),
    ("k_conv_lif_tiled<3,3> + k_pool", "fuzz", "conv-edge-tile-3x3-17x31", {}, ["k_conv_lif_tiled<3,3>", "k_pool"]),
    # per-step dense (one kernel, two grid forms; the wide one starts at B = 16384 and is left to test_gpu_fuzz)
    ("k_dense_lif_mfma (narrow)", "fuzz-dense", "dense-wg128-B127", {}, ["k_trace", "k_dense_lif_mfma (narrow)"]),
    # k_lif_step_any
    ("k_lif_step_any", "step-any", "step-form-R1-fused", {}, None),
    ("k_lif_step_any (pooling)", "step-any", "step-form-R1-pooling", {}, None),
    ("k_lif_step_any (split)", "step-any", "step-form-R1-split", {}, None),
    # k_lif_step_w3: c_in 64 and 1, 4 and 8 tiles per workgroup
    ("k_lif_step_w3 (4 tiles)", "step-w3", "w3-64to64-1x32-B3", {}, None),
    ("k_lif_step_w3 (8 tiles)", "step-w3", "w3-64to64-1x256-B1", {}, None),
    ("k_lif_step_w3 (c_in 1, 4 tiles)", "step-w3", "w3-1to64-1x32-B3", {}, None),
    ("k_lif_step_w3 (c_in 1, 8 tiles)", "step-w3", "w3-switch-1to64-16x128", {}, None),
    # the sequence launchers
    ("k_lif_seq_c32", "seq", "seq-var-c32-R0-O3-N0", {}, None),
    ("k_lif_seq_c32d", "seq", "seq-var-c32d-R1-O3", {}, None),
    ("k_lif_seq_c32rp", "seq", "seq-var-c32rp-R1-O3", {}, None),
    ("k_lif_seq_c32t", "seq", "seq-var-c32t-R1-O3", {}, None),
    ("k_lif_seq_c1 (cells)", "seq", "seq-var-c1-R0-F1-cells", {}, None),
    ("k_lif_seq_c1 (iq)", "seq", "seq-var-c1-R0-F0-iq", {}, None),
    ("k_lif_seq_c1t (cells)", "seq", "seq-var-c1t-R1-F0-cells", {}, None),
    ("k_lif_seq_c1t (iq)", "seq", "seq-var-c1t-R1-F1-iq", {}, None),
    ("k_lif_seq_w3 (full)", "seq", "seq-var-w3-R1-O3-L5-F1", {}, None),
    ("k_lif_seq_w3 (ragged)", "seq", "seq-var-w3-R1-O3-L5-F0", {}, None),
    ("k_lif_seq_w3f", "seq", "seq-var-w3f-R1-O3", {}, None),
    ("k_dense_lif_seq", "seq", "seq-var-dense-seq-R1", {}, None),
    # ... with pv_presigmoid: the buffer holds v
    ("k_lif_seq_c32 presigmoid", "seq", "seq-var-c32-R1-O2-N0", {}, None),
    ("k_lif_seq_c32d presigmoid", "seq", "seq-var-c32d-R0-O2", {}, None),
    ("k_lif_seq_c32rp presigmoid", "seq", "seq-var-c32rp-R0-O2", dict(Ts=[9]), None),
    ("k_lif_seq_c32t presigmoid", "seq", "seq-var-c32t-R0-O2", {}, None),
    ("k_lif_seq_c1 presigmoid", "seq", "seq-var-c1-R0-F2-cells", {}, None),
    ("k_lif_seq_c1t presigmoid", "seq", "seq-var-c1t-R0-F2-cells", {}, None),
    ("k_lif_seq_w3 presigmoid", "seq", "seq-var-w3-R1-O7-L5-F0", {}, None),
    ("k_lif_seq_w3f presigmoid", "seq", "seq-var-w3f-R1-O7", {}, None),
    # k_lif_seq_any / k_lif_seq_wide: weights in LDS, streamed, register form
    ("k_lif_seq_any (LDS)", "seq-any", "any-var-R1-wlds", {}, None),
    ("k_lif_seq_any (streamed)", "seq-any", "any-var-R1-stream", {}, None),
    ("k_lif_seq_any (registers)", "seq-any", "any-var-R1-regs", {}, None),
    ("k_lif_seq_wide (LDS)", "seq-wide", "wide-var-R1-wlds", {}, None),
    ("k_lif_seq_wide (streamed)", "seq-wide", "wide-var-R1-stream", {}, None),
    ("k_lif_seq_wide (registers)", "seq-wide", "wide-var-R1-regs", {}, None),
]
# (kind, refractory, int8 weights on the sequence launchers that take them)
_KIND_ROWS = [("decay", 0, 0), ("decay", 1, 1), ("mixed", 1, 0), ("threshold", 0, 0), ("threshold", 1, 0), ("analog", 0, 0)]
MAX_B, MAX_T, MAX_CALLS, MAX_STEPS = 3, 12, 3, 8


def float_input(c):
    """the entry point takes x as float* (the analog kind applies)"""
    return c["src"] in ("fuzz", "fuzz-dense", "step-any", "step-w3") or (c["src"] == "seq" and c["entry"] == "dense")


def is_dense(c):
    return c["src"] == "fuzz-dense" or (c["src"] == "seq" and c["entry"] == "dense")


def fed_by_cells(c):
    return c["src"] == "seq" and c["entry"] in ("cells", "iq")


def kinds_of(family):
    """the kinds a family has a case of"""
    return sorted({c["kind"] for c in cases() if c["family"] == family})


_BASES = {}


def _base(src, sid):
    if (src, sid) not in _BASES:
        _BASES[(src, sid)] = SRC[src].by_id(sid)
    return _BASES[(src, sid)]


def cases(seed=SEED):
    out = []
    for i, (family, src, sid, over, names) in enumerate(_ROWS):
        base = _base(src, sid)
        for k, (kind, R, q8) in enumerate(_KIND_ROWS):
            c = dict(base)
            c.update(over)
            c.update(src=src, source=sid, family=family, kind=kind, names=names, stratum="values", note="")
            if kind == "analog" and not float_input(c):
                continue
            if "presigmoid" in family and kind in ("mixed", "analog"):
                continue
            c["refractory"] = R
            c["alpharp"] = .5 if (kind == "threshold" and R) else FZ.ALPHARP
            c["B"] = min(c["B"], MAX_B)
            if "B_checked" in c:
                c["B_checked"] = c["B"]
            if "B_run" in c and c["source"] != "w3-switch-1to64-16x128":     # (32 device samples, copies of 3: the 8-tile form)
                c["B_run"] = c["B"]
            if "also_B" in c:
                c["also_B"] = None
            if src in ("fuzz", "fuzz-dense", "step-any", "step-w3"):
                c.update(steps=MAX_STEPS if kind == "decay" else FZ.STEPS, bias=1, state0=1)
                if src != "fuzz-dense":
                    c.update(q8=0, misalign=c["misalign"] if src == "fuzz" else 0)
                if "want_v" in c:
                    c["want_v"] = 1
            elif src == "seq":
                if c["entry"] != "dense":
                    c["q8"] = q8
            else:
                c["bias"] = 1
            c["id"] = "val-%s-%s-%s-R%d" % (src, family.replace(" ", "").replace("(", "-").replace(")", ""), kind, R)
            c["seed"] = seed * 100003 + 10 * i + k
            out.append(c)
    return out


def by_id(cid):
    """the case of that id (a sibling's id: the sibling's case)"""
    for c in cases():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def describe(c):
    return json.dumps(c, sort_keys=True)


def cases_hash(cs):
    return hashlib.sha256("\n".join(describe(c) for c in cs).encode()).hexdigest()


def families():
    return [r[0] for r in _ROWS]


# ---------------------------------------------------------------------------------------------------------------------------
# the launch log (the siblings' predictions, as they are)
# ---------------------------------------------------------------------------------------------------------------------------
def expected_log(c, T=None):
    """the predicted launch log of one call (per-step entries: the kernels in front of the readouts), None where the sibling has
    none — then c['names'] must all be in the log"""
    if c["src"] == "step-any":
        return SA.launch_log(c, c["B_run"])
    if c["src"] == "step-w3":
        return S3.launch_log(c, c["B_run"])
    if c["src"] == "seq":
        return SF.expected_kernels(c, T, None)
    if c["src"] == "seq-any":
        return ["k_seq_any_wprep", A.variant(c)]
    if c["src"] == "seq-wide":
        return WD.launch_log(c)
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------------------
def geometry(c):
    """dict(B, cin, h, w, cout, ch, cw, ph, pw, kh, kw, Ts, tau) of a case; a dense layer is a 1x1 conv on a 1x1 plane.  tau:
    'scalar' (one set of time constants), 'channel' or 'tensor' (c_in, h, w)"""
    if is_dense(c):
        g = dict(cin=c["in_features"], cout=c["out_features"], h=1, w=1, ch=1, cw=1, ph=1, pw=1, kh=1, kw=1,
                 tau="channel" if c["tau_tensor"] else "scalar")
    elif c["src"] == "seq":
        ch, cw, ph, pw = SF.out_shape(c)
        kh, kw = SF.LAYERS[c["layer"]]["k"]
        g = dict(cin=c["c_in"], cout=c["c_out"], h=c["h"], w=c["w"], ch=ch, cw=cw, ph=ph, pw=pw, kh=kh, kw=kw, tau="channel")
    else:
        ch, cw, ph, pw = FZ.conv_shape(c) if c["src"] in ("fuzz", "step-any", "step-w3") else A.out_shape(c)
        tau = "channel" if c["src"] in ("seq-any", "seq-wide") else "tensor"
        g = dict(cin=c["c_in"], cout=c["c_out"], h=c["h"], w=c["w"], ch=ch, cw=cw, ph=ph, pw=pw, kh=c["kh"], kw=c["kw"],
                 tau=tau if c["tau_tensor"] else "scalar")
    g.update(B=c["B"], Ts=list(c["Ts"]) if "Ts" in c else [1] * c["steps"])
    g["pool"] = (c["pool_h"], c["pool_w"]) if "pool_h" in c and not is_dense(c) else (g["ch"] // g["ph"], g["cw"] // g["pw"])
    return g


def subnormal(rng, shape):
    """log-uniform over 2^-149 ... 2^-120 (the bottom octave rounds to 2^-149 or 2^-148)"""
    return (2.0 ** rng.uniform(-149, -120, size=shape)).astype(np.float32)


def subnormal_traces(rng, shape):
    """(eps0, eps1), each log-uniform over 2^-149 ... 2^-120 and within a factor 8 of each other, as the two traces of one input
    are (a pair that sits at 2^-149 together is then no rarity: with alphas = .5 it is eps1 that sticks, once eps0 is 0)"""
    e = rng.uniform(-149, -120, size=shape)
    return (2.0 ** e).astype(np.float32), (2.0 ** np.clip(e + rng.uniform(-3, 3, size=shape), -149, -120)).astype(np.float32)


def _time_constants(c, g, rng):
    """(alpha, tau_m, alphas, tau_s), each (cin, 1, 1) or (cin, h, w): channel j takes alphas = ALPHAS[j % 4] and
    alpha = ALPHAS[(j + 1 + j / 4) % 4] (j = 0: .5 and .75 — eps0 dies out, eps1 sticks), a threshold case gives the channels of a
    pair the same; a (c_in, h, w) tensor draws the pair per element"""
    cin = g["cin"]
    j = np.arange(cin) // 2 if c["kind"] == "threshold" else np.arange(cin)
    if g["tau"] == "scalar":
        j = np.zeros(cin, int)
    ia, im = (j % 4)[:, None, None], ((j + 1 + j // 4) % 4)[:, None, None]
    if g["tau"] == "tensor" and c["kind"] != "threshold":
        ia, im = rng.randint(0, 4, size=(cin, g["h"], g["w"])), rng.randint(0, 4, size=(cin, g["h"], g["w"]))
        ia[0, 0, 0], im[0, 0, 0] = 0, 1
    alphas, alpha = ALPHAS[ia], ALPHAS[im]
    one = np.float32(1)
    return alpha, (one / (one - alpha)).astype(np.float32), alphas, (one / (one - alphas)).astype(np.float32)


def _pair(a):
    """channels 2 cp + 1 := channels 2 cp (axis 1 of a state tensor, axis 2 of a (T, B, cin, h, w) input)"""
    ax = a.ndim - 3
    n = 2 * (a.shape[ax] // 2)
    idx = [slice(None)] * a.ndim
    src, dst = list(idx), list(idx)
    src[ax], dst[ax] = slice(0, n, 2), slice(1, n, 2)
    a[tuple(dst)] = a[tuple(src)]
    return a


def _threshold(c, g, rng):
    """weights, bias and arp that put v EXACTLY on the table at the first step (x = 0 there, the state k * 2^-149 with k < 8):
      output channels co % 4 in (0, 1) (every channel where c_in = 1): W = +-0, the sign drawn per tap — all -0 on co % 4 == 1, so
        that a chain from a bias of -0 stays -0 (one +0 product turns it into +0);
      output channels co % 4 in (2, 3): exactly cancelling input-channel pairs — equal state, time constants and input on channels
        2 cp and 2 cp + 1, weights w = +-2^k (k <= 2) and -w, an odd last channel +-0.  The two links of a pair are neighbours in
        the pinned order and their products p = eps1 w are multiples of 2^-149 below 2^-138: bias + p is exact for every table value
        below 2^-125 and absorbed by every one from 1 up, so every pair returns the chain to the bias (to +0 from +-0).
    plain: b[co] = TABLE[co % n].  refractory: alpharp = .5, b = +-0, arp = 2 TABLE_CAPPED[(co P + pixel + b) % n], so v = the table
    value at every pixel whatever c_out is (where the chain ends at +0, -0 comes out as +0).  A pooling layer counts its windows
    in place of its pixels: a window holds one value — a tie of equal values — and the zeros alternate in sign with the pixel's
    parity, a tie of +0 with -0 (a plain pooling layer holds b[co] in every window anyway)."""
    cout, cin, kh, kw, n = g["cout"], g["cin"], g["kh"], g["kw"], len(TABLE)
    sign = np.where(rng.rand(cout, cin, kh, kw) < .5, np.float32(-1), np.float32(1))
    W = np.zeros((cout, cin, kh, kw), np.float32) * sign
    co = np.arange(cout)
    W[co % 4 == 1] = np.float32(-0.0)
    if cin >= 2:
        pairs = co % 4 >= 2
        w = sign[:, 0::2][:, :cin // 2] * (2.0 ** rng.randint(0, 3, size=(cout, cin // 2, kh, kw))).astype(np.float32)
        W[pairs, 0:2 * (cin // 2):2] = w[pairs]
        W[pairs, 1:2 * (cin // 2):2] = -w[pairs]
    if c["refractory"]:
        b = np.where(co % 4 == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        poh, pow_ = g["pool"]
        wy, wx = (np.arange(g["ch"]) + (poh - 1) // 2) // poh, (np.arange(g["cw"]) + (pow_ - 1) // 2) // pow_
        pos = (wy[:, None] * (wx.max() + 1) + wx[None, :]).ravel()         # (no pooling: the pixel's own index)
        P = int(pos.max()) + 1
        idx = (co[None, :, None] * P + pos[None, None, :] + np.arange(g["B"])[:, None, None]) % n
        if (poh, pow_) != (1, 1):
            parity = ((np.arange(g["ch"])[:, None] + np.arange(g["cw"])[None, :]) % 2).ravel()
            idx = np.where(idx < 2, parity[None, None, :], idx)
        arp = (np.float32(2) * TABLE_CAPPED[idx]).astype(np.float32).reshape(g["B"], cout, g["ch"], g["cw"])
    else:
        b = TABLE[co % n].copy()
        arp = np.zeros((g["B"], cout, g["ch"], g["cw"]), np.float32)
    return W, b, arp


def _cells_input(c, g, rng, extra):
    """per call (cells (T, B), one-hot planes): decay feeds cell 0 alone (the siblings' 'cell_first' window), the other kinds
    uniform cells; an IQ entry gets the window whose values encode them and the cells ops.iq_encode's definition makes of it"""
    B, hw, w = g["B"], g["h"] * g["w"], g["w"]
    n = sum(g["Ts"]) + (c["t0"] + 5 if c["entry"] == "iq" else 0)
    want = np.zeros((n, B), np.int64) if c["kind"] == "decay" else rng.randint(0, hw, size=(n, B))
    if c["entry"] == "iq":
        tab = SF.iq_tables(c, rng)
        iq = np.empty((B, 2, n), np.float32)
        for a, (thr, idx) in enumerate(((tab["thr_i"], want % w), (tab["thr_q"], want // w))):
            lo = np.concatenate([[np.float32(-1.5)], thr])
            iq[:, a] = lo[idx].T                                      # (x == thr[j - 1] -> cell j under the main table)
        extra.update(iq=iq, tab=tab)
    calls, t_off = [], c["t0"] if c["entry"] == "iq" else 0
    for T in g["Ts"]:
        cells = SF.iq_cells(extra["tab"], extra["iq"], t_off, T, w) if c["entry"] == "iq" else want[t_off:t_off + T].astype(np.int32)
        t_off += T
        x = np.zeros((T, B, 1, hw), np.float32)
        x[np.arange(T)[:, None], np.arange(B)[None, :], 0, cells] = 1
        calls.append(dict(x=x.reshape(T, B, 1, g["h"], g["w"]), cells=cells))
    return calls


def draw(c, attempt=0):
    """the value tensors of a case, format-free: dict(tau (4 arrays), calls [dict(x (T, B, cin, h, w)[, cells])], eps0, eps1, arp,
    W0 (cout, cin, kh, kw), b, rescale (std(v) = 2 from a provisional run), silent (mask of the subnormal half)[, iq, tab])"""
    g, kind = geometry(c), c["kind"]
    rng = np.random.RandomState((c["seed"] + 7919 * attempt) % (2 ** 31))
    B, cin, h, w, cout = g["B"], g["cin"], g["h"], g["w"], g["cout"]
    sshape, oshape = (B, cin, h, w), (B, cout, g["ch"], g["cw"])
    D = dict(tau=_time_constants(c, g, rng), silent=None, rescale=kind in ("mixed", "analog"))
    # inputs
    if fed_by_cells(c):
        D["calls"] = _cells_input(c, g, rng, D)
    else:
        D["calls"] = []
        for T in g["Ts"]:
            if kind == "decay":
                x = np.zeros((T,) + sshape, np.float32)
            elif kind == "analog":
                x = rng.uniform(-2, 3, size=(T,) + sshape).astype(np.float32)
                pick = rng.rand(*x.shape)
                for i, val in enumerate(ANALOG_TABLE):
                    x[(pick >= .03 * i) & (pick < .03 * (i + 1))] = val
            else:
                x = (rng.uniform(size=(T,) + sshape) < .3).astype(np.float32)
            D["calls"].append(dict(x=x))
        if kind == "threshold":
            D["calls"][0]["x"][0] = 0
            for call in D["calls"]:
                _pair(call["x"])
    # state
    if kind == "decay":
        (D["eps0"], D["eps1"]), D["arp"] = subnormal_traces(rng, sshape), -subnormal(rng, oshape)
    elif kind == "threshold":
        D["eps0"] = _pair(rng.randint(1, 8, size=sshape).astype(np.float32) * TINY)
        D["eps1"] = _pair(rng.randint(1, 8, size=sshape).astype(np.float32) * TINY)
    else:
        D["eps0"] = rng.uniform(0, 3, size=sshape).astype(np.float32)
        D["eps1"] = rng.uniform(0, 12, size=sshape).astype(np.float32)
        D["arp"] = (-rng.uniform(0, 2, size=oshape)).astype(np.float32)
    if kind == "mixed":
        fed = np.zeros(sshape, bool)
        if fed_by_cells(c):
            for call in D["calls"]:
                fed |= call["x"].any(axis=0)
        silent = (rng.rand(*sshape) < .5) & ~fed
        for call in D["calls"]:
            if "cells" not in call:
                call["x"][:, silent] = 0
        s0, s1 = subnormal_traces(rng, sshape)
        D["eps0"], D["eps1"] = np.where(silent, s0, D["eps0"]), np.where(silent, s1, D["eps1"])
        D["arp"] = np.where(rng.rand(*oshape) < .5, -subnormal(rng, oshape), D["arp"])
        D["silent"] = silent
    # weights and bias
    co = np.arange(cout)
    if kind == "threshold":
        D["W0"], D["b"], D["arp"] = _threshold(c, g, rng)
    elif kind == "decay":
        D["W0"] = (rng.randn(cout, cin, g["kh"], g["kw"]).astype(np.float32) * (W_DECAY_FED if fed_by_cells(c) else W_DECAY)).astype(np.float32)
        b = (rng.randn(cout) * .5).astype(np.float32)
        b[co % 4 == 0], b[co % 4 == 2] = np.float32(0.0), np.float32(-0.0)
        D["b"] = b
    else:
        D["W0"] = rng.randn(cout, cin, g["kh"], g["kw"]).astype(np.float32)
        D["b"] = (rng.randn(cout) * .5).astype(np.float32)
    D["rng"] = rng
    return D


# ---------------------------------------------------------------------------------------------------------------------------
# the siblings' tensor formats and oracle trajectories
# ---------------------------------------------------------------------------------------------------------------------------
def _step_format(c):
    return c["src"] in ("fuzz", "fuzz-dense", "step-any", "step-w3")


def _oracle_case(c):
    return {k: v for k, v in c.items() if k not in SA.EXTRA} if c["src"] in ("step-any", "step-w3") else c


def tensors(c, D, W, b):
    """`D` with weights W and bias b in the format of the case's sibling (fuzz_cases._conv_draw / _dense_draw,
    seq_fuzz_cases._draw, seq_any_cases._draw): what the sibling's device runner and oracle take"""
    g, rng = geometry(c), np.random.RandomState((c["seed"] + 1) % (2 ** 31))
    dense = is_dense(c)
    flat = (lambda a: a.reshape(a.shape[0], -1)) if dense else (lambda a: a)
    T = dict(eps0=flat(D["eps0"]).copy(), eps1=flat(D["eps1"]).copy(), arp=flat(D["arp"]).copy(), b=b, q8=None)
    T["W"] = np.ascontiguousarray(W.reshape(W.shape[0], -1) if dense else W)
    if g["tau"] == "scalar":
        tau = [t.reshape(-1)[:1].copy() for t in D["tau"]]
    elif g["tau"] == "tensor":
        tau = [np.ascontiguousarray(np.broadcast_to(t, (g["cin"], g["h"], g["w"]))) for t in D["tau"]]
    else:
        tau = [np.ascontiguousarray(np.broadcast_to(t, (g["cin"], 1, 1)).reshape(g["cin"])) for t in D["tau"]]
    if not _step_format(c) and g["tau"] == "scalar" and not dense:
        tau = [np.repeat(t, g["cin"]) for t in tau]          # (the sequence entries take (4, c_in): the same values in every channel)
    T["tau"] = tuple(tau)
    K, B, tg = g["cout"] * g["ph"] * g["pw"], g["B"], c.get("target") or 10
    ro = lambda: ((rng.uniform(-1, 1, size=(tg, K)) * (.5 / np.sqrt(K))).astype(np.float32), rng.uniform(-.1, .1, size=(tg,)).astype(np.float32))
    if _step_format(c):
        T["x"] = [flat(call["x"][0]) for call in D["calls"]]
        T["i2o_W"], T["i2o_b"] = ro()
        T["out_W"], T["out_b"] = ro()
        pooled, full = (B, g["cout"]) + ((g["ph"], g["pw"]) if not dense else ()), (B, g["cout"]) + ((g["ch"], g["cw"]) if not dense else ())
        T["g_p"] = rng.randn(B, tg).astype(np.float32) if (dense or c["readout"]) else None
        T["g_o"] = rng.randn(B, tg).astype(np.float32) if c.get("output_layer") else None
        T["g_pv"], T["g_v"] = (rng.randn(*pooled) * .3).astype(np.float32), (rng.randn(*full) * .1).astype(np.float32)
    else:
        T["calls"] = [dict(call, x=call["x"].reshape(call["x"].shape[:2] + (-1,)) if dense else call["x"]) for call in D["calls"]]
        for k in ("iq", "tab"):
            if k in D:
                T[k] = D[k]
        nro = tg if dense else c.get("n_ro", 0)
        T["ro_W"], T["ro_b"] = ro() if nro else (None, None)
    if c.get("q8"):
        q, scale, Wd = FZ.quantize_int8(T["W"])
        T["q8"], T["W"] = (q, scale), np.ascontiguousarray(Wd)
    return T


def trajectory(c, T, before_step=None):
    """the C oracle through every step of every call -> per-step formats: the three... `steps` dicts of fuzz_cases; sequence
    formats: per call dict(v, s, pv (T, B, ...), eps0, eps1, arp after the call).  before_step(state list): a mutant's hook, run
    on the oracle's state in front of every step (the sequence formats step one by one for it)"""
    oc = _oracle_case(c)
    if c["src"] == "fuzz-dense":
        return FZ._dense_oracle(oc, T, before_step)
    if _step_format(c):
        return FZ._conv_oracle(oc, T, before_step)
    if c["src"] == "seq":
        return SF._trajectory(oc, T, before_step)
    return A._trajectory(oc, T, before_step)


def flat_steps(c, traj):
    """[dict(v (B, cout, ...), s, pv)] over all steps of all calls, whatever the format"""
    if _step_format(c):
        return [dict(v=s["v"], s=s["s"], pv=s["pv"]) for s in traj]
    return [dict(v=call["v"][t], s=call["s"][t], pv=call["pv"][t]) for call in traj for t in range(call["v"].shape[0])]


def final_state(c, traj):
    return traj[-1]["eps0"], traj[-1]["eps1"], traj[-1]["arp"]


def is_subnormal(a):
    return (a != 0) & (np.abs(a) < np.float32(2.0 ** -126))


def crossings(c, D, traj):
    """(normal -> subnormal, subnormal -> exactly 0, stuck at 2^-149): element counts over eps0 and eps1 between the initial state
    and the state after the last call.  Stuck: at 2^-149 after the last step, and one more silent step leaves it there —
    alphas * 2^-149 rounds back to 2^-149 for alphas > .5; eps1 = alpha eps1 + eps0 tau_m likewise once eps0 is 0"""
    i0, i1 = D["eps0"], D["eps1"]
    f0, f1 = (a.reshape(i0.shape) for a in final_state(c, traj)[:2])
    normal = lambda a: np.abs(a) >= np.float32(2.0 ** -126)
    down = int((normal(i0) & is_subnormal(f0)).sum() + (normal(i1) & is_subnormal(f1)).sum())
    zero = int((is_subnormal(i0) & (f0 == 0)).sum() + (is_subnormal(i1) & (f1 == 0)).sum())
    alpha, alphas = np.broadcast_to(D["tau"][0], f0.shape[1:]), np.broadcast_to(D["tau"][2], f0.shape[1:])
    stuck = int(((f0 == TINY) & ((alphas * f0).astype(np.float32) == f0)).sum() +
                ((f1 == TINY) & (f0 == 0) & ((alpha * f1).astype(np.float32) == f1)).sum())
    return down, zero, stuck


_RUNS = {}


def run(c, max_attempts=24):
    """(tensors in the sibling's format, the oracle's trajectory, the format-free draw) of a case; computed once per process and
    shared — the callers leave all three unchanged.  mixed / analog: the weights are rescaled so that std(v) = 2 over a
    provisional plain run without bias (v is linear in W there), as the siblings do.  decay / mixed: the first attempt in which
    each of the three crossings occurs (deterministic in the sub-seed; small planes need a second draw now and then)"""
    if c["id"] in _RUNS:
        return _RUNS[c["id"]]
    for attempt in range(max_attempts):
        T, traj, D = _run(c, attempt)
        if c["kind"] not in ("decay", "mixed") or min(crossings(c, D, traj)) > 0:
            D["attempt"] = attempt
            _RUNS[c["id"]] = (T, traj, D)
            return _RUNS[c["id"]]
    raise AssertionError("%s: no draw with all three crossings in %d attempts: %s" % (c["id"], max_attempts, crossings(c, D, traj)))


def _run(c, attempt):
    D = draw(c, attempt)
    W = D["W0"]
    if D["rescale"]:
        c0 = dict(c, refractory=0, q8=0) if "q8" in c else dict(c, refractory=0)
        vs = np.concatenate([s["v"].ravel() for s in flat_steps(c, trajectory(c0, tensors(c0, D, W, None)))])
        std = float(vs.std())
        assert np.isfinite(std) and std > 0, (c["id"], std)
        W = (W * np.float32(2.0 / std)).astype(np.float32)
    T = tensors(c, D, W, D["b"])
    return T, trajectory(c, T), D


def flush(a):
    """flush-to-zero of an fp32 array, in place: what a kernel that drops subnormals would read"""
    a[np.abs(a) < np.float32(2.0 ** -126)] = 0
    return a
