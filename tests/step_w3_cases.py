"""Seeded cases for dcll_conv_lif_step_w3 / dcll_conv_lif_backward_w3[_open] (k_lif_step_w3, k_bwd_wgrad_w3: the opt-in MFMA learning
step of the (1,3)-kernel / 64-channel / (1,2)-pool layers of radio_ml_conv_ref.yaml), built on tests/fuzz_cases.py.

A forward case is one of its conv cases (same keys; FZ.conv_run gives the tensors and the C oracle's trajectory of three steps from
carried state, with its non-vacuity check) plus three keys of this list:
    want_v   0: the call passes out_v = NULL
    B_run    batch on the device; the oracle runs on the first B distinct samples, the device on copies of them
    also_B   a second batch size (the first also_B samples) on the other side of the 8- / 4-tile switch: per-sample results equal
A backward case is a geometry and a batch; bwd_draw() gives its tensors (no oracle run: the backward's inputs are eps1, v and the
gradients), v on a grid of 1/64 so that the pool routing does not hang on the last bit of a sigmoid.
Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_step_w3_cases.py proves the lists on
the CPU; tests/test_gpu_step_w3.py runs the HIP kernels against them.

The launchers are restated ONCE here (csrc/dcll_step_w3.hip: dcll_step_w3_check, step_w3_lds_floats, dcll_step_w3_tiles,
dcll_launch_step_w3, bwd_w3_lds_floats, k_bwd_wgrad_w3's summation order; csrc/dcll_hip.hip: dcll_conv_lif_step_w3)."""
import numpy as np

import fuzz_cases as FZ

SEED = 20271
PST = 65                # floats per position of the forward's pixel-major image
MIN_WGS = 256           # fewer 8-tile workgroups than this: the 4-tile form
MAX_CHUNKS = 256        # partial rows of k_bwd_wgrad_w3, at most
EXTRA = dict(want_v=1, B_run=None, also_B=None)
W3 = dict(c_out=64, kh=1, kw=3, pad_h=0, pad_w=1, pool_h=1, pool_w=2)
GEO64 = [(16, 2), (8, 4), (4, 8), (2, 16), (1, 32), (1, 64), (4, 64), (3, 128), (1, 256), (2, 256), (16, 64)]
GEO1 = [(1, 32), (2, 128), (16, 128)]
FWD_B = (1, 3, 11)
BWD_B = (1, 3, 33, 257, 300)
# the weight gradient against float64 (tests/test_gpu_bwd_any.py's): rtol, atol = GRAD_ATOL * max|ref|.  The fp32 restatement of
# the kernel's summation order stays inside it on every case (tests/test_step_w3_cases.py prints the worst excess), so it stands
GRAD_RTOL, GRAD_ATOL = 2e-3, 5e-5
# share of the forward cases whose oracle trajectory has at least one spike and at least one silent neuron: all of them
# (FZ.conv_run redraws a vacuous trajectory from the next sub-seed; tests/test_step_w3_cases.py asserts the share)
NON_VACUOUS_FLOOR = 1.0


def _case(cid, stratum, seed, **kw):
    extra = {k: kw.pop(k, v) for k, v in EXTRA.items()}
    kw.setdefault("readout", 0)
    c = FZ._case(cid, stratum, seed, **dict(W3, **kw))
    c.update(extra)
    if c["B_run"] is None:
        c["B_run"] = c["B"]
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers, restated
# ---------------------------------------------------------------------------------------------------------------------------
def served(c):
    """dcll_step_w3_check: None = served, else (code, phrase of the message)"""
    if FZ.conv_shape(c) is None or c["c_in"] % c["groups"] or c["c_out"] % c["groups"]:
        return "DCLL_ERR_INVALID", ""
    w = c["w"]
    ok = ((c["stride"], c["dilation"], c["groups"]) == (1, 1, 1) and c["c_in"] in (1, 64) and c["c_out"] == 64 and
          (c["kh"], c["kw"], c["pad_h"], c["pad_w"], c["pool_h"], c["pool_w"]) == (1, 3, 0, 1, 1, 2) and
          2 <= w <= 256 and w & (w - 1) == 0 and (c["h"] * w) % 32 == 0)
    if not ok:
        return "DCLL_ERR_UNSUPPORTED", "serves c_in 1 or 64, c_out 64, kernel (1,3)"
    if c["h"] * w >= 1 << 24:
        return "DCLL_ERR_UNSUPPORTED", "plane larger than 2^24 pixels"
    return None


def positions(w, nt):
    """image positions of a workgroup of nt tiles: its pixels and one shared zero in front of every row and behind the last"""
    return 32 * nt + 32 * nt // w + 1


def lds_bytes(c):
    """dcll_conv_lif_step_w3_lds: LDS bytes of a workgroup of the 8-tile form, 0 = not served"""
    return 0 if served(c) is not None else 4 * (positions(c["w"], 8) * (PST if c["c_in"] == 64 else 1) + 64)


def form_lds_bytes(c, nt):
    return 4 * (positions(c["w"], nt) * (PST if c["c_in"] == 64 else 1) + 64)


def ntiles(c, B):
    return B * (c["h"] * c["w"] // 32)


def tiles(c, B):
    """dcll_step_w3_tiles: tiles per workgroup"""
    return 4 if c["w"] <= 128 and (ntiles(c, B) + 7) // 8 < MIN_WGS else 8


def race_free(c, nt):
    """the race note: a workgroup's pixels are whole rows"""
    return (32 * nt) % c["w"] == 0


def tile_ranges(c, B):
    """[first tile, end tile) of every workgroup of the launch"""
    nt, n = tiles(c, B), ntiles(c, B)
    return [(g, min(g + nt, n)) for g in range(0, n, nt)]


def form(c, B):
    return "k_lif_step_w3<%d> (%s%d tiles)" % (c["refractory"], "c_in 1, " if c["c_in"] == 1 else "", tiles(c, B))


def all_forms():
    return ["k_lif_step_w3<%d> (%s%d tiles)" % (r, ci, nt) for r in (0, 1) for ci in ("", "c_in 1, ") for nt in (8, 4)]


def launch_log(c, B):
    """the kernels of one dcll_conv_lif_step_w3 call in front of its readouts"""
    return [form(c, B)]


def image_reads(c, nt):
    """(lowest, highest) image position any lane of any tile of a workgroup reads as a B operand (taps kx = 0, 1, 2 of every
    pixel), the positions its trace phase writes and the zero positions — the kernel's own index arithmetic"""
    w = c["w"]
    lw = w.bit_length() - 1
    P = 32 * nt
    written = [p + (p >> lw) + 1 for p in range(P)]
    zeros = [k * (w + 1) for k in range(P // w + 1)]
    reads = [p + (p >> lw) + kx for p in range(P) for kx in range(3)]
    return min(reads), max(reads), written, zeros


# ---- the weight gradient
def bwd_positions(w):
    return 130 if w == 256 else 128 + 128 // w + 1


def bwd_cs(w):
    """channel stride of k_bwd_wgrad_w3's image: the positions rounded up to 3 mod 32"""
    return (bwd_positions(w) - 3 + 31) // 32 * 32 + 3


def bwd_lds_bytes(c):
    """dcll_conv_lif_backward_w3_lds; c_in 1: the generic k_bwd_wgrad's row bands"""
    if served(c) is not None:
        return 0
    if c["c_in"] == 64:
        return 4 * (64 * bwd_cs(c["w"]) + 64 * 129 + 16)
    return 4 * (min(FZ.LDS_FLOATS // (c["w"] + 2), c["h"]) * (c["w"] + 2) + 4 * 65)


def bwd_chunks(c, B, room=MAX_CHUNKS):
    """partial rows of a launch with room for `room`: one per 128-pixel block, at most 256"""
    return min(room, MAX_CHUNKS, (ntiles(c, B) + 3) // 4)


def bwd_wgrad_name(c):
    return "k_bwd_wgrad_w3" if c["c_in"] == 64 else "k_bwd_wgrad"


def _fma32(acc, a, b):
    """fmaf on float32 arrays: the product of two floats is exact in float64, the sum is rounded to float64 and then to float32
    (a double rounding in one case of ~2^29: immaterial for an error bound)"""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def wgrad_restated(g, eps1, cols, nchunk):
    """k_bwd_wgrad_w3's summation order in float32 for the weight-gradient columns `cols` (n = 3 ci + kx) of every output channel:
    g (B, 64, h, w) float32, eps1 (B, 64, h, w) float32 -> (dW (64, len(cols)), db (64,)).  Chunk c takes the 128-pixel blocks
    c, c + nchunk, ... of the flattened pixels in order; inside a block the pixel pairs [0, 32) and [32, 64) are two fma chains
    (pixel 2 pp, then 2 pp + 1); first + second at the end; the chunks are then added in order (k_bwd_reduce's plain sum: its
    own grouping differs in the last bit only).  The bias gradient: lane l sums pixels l, l + 64 of every block, then a tree."""
    B, C, h, w = g.shape
    HW = h * w
    gs = np.ascontiguousarray(g.transpose(1, 0, 2, 3)).reshape(C, B * HW)              # the pixel stream of every channel
    ep = np.zeros((eps1.shape[1], B, h, w + 2), np.float32)                            # zero beyond a row's ends
    ep[:, :, :, 1:-1] = eps1.transpose(1, 0, 2, 3)
    # column n at stream pixel p reads eps1[ci, p + kx - 1]
    E = np.stack([ep[n // 3, :, :, n % 3:n % 3 + w].reshape(B * HW) for n in cols])    # (ncol, B HW)
    npx = B * HW
    nblk = (npx + 127) // 128
    pad = nblk * 128 - npx
    gs = np.pad(gs, ((0, 0), (0, pad))).reshape(C, nblk, 2, 64)                        # (co, block, half, pixel of the half)
    E = np.pad(E, ((0, 0), (0, pad))).reshape(len(cols), nblk, 2, 64)
    rounds = (nblk + nchunk - 1) // nchunk
    acc = np.zeros((nchunk, 2, C, len(cols)), np.float32)
    bacc = np.zeros((nchunk, C, 64), np.float32)
    for r in range(rounds):
        blks = np.arange(nchunk) + r * nchunk
        live = blks < nblk
        bi = np.where(live, blks, 0)
        gb = np.where(live[None, :, None, None], gs[:, bi], 0)                         # (co, chunk, half, 64)
        eb = np.where(live[None, :, None, None], E[:, bi], 0)                          # (col, chunk, half, 64)
        for k in range(64):
            a = gb[:, :, :, k].transpose(1, 2, 0)[:, :, :, None]                       # (chunk, half, co, 1)
            b = eb[:, :, :, k].transpose(1, 2, 0)[:, :, None, :]                       # (chunk, half, 1, col)
            acc = _fma32(acc, a, b)
        flat = gb.transpose(1, 0, 2, 3).reshape(nchunk, C, 128)
        bacc = (bacc + flat[:, :, :64]).astype(np.float32)
        bacc = (bacc + flat[:, :, 64:]).astype(np.float32)
    part = (acc[:, 0] + acc[:, 1]).astype(np.float32)
    dW = np.zeros((C, len(cols)), np.float32)
    for ch in range(nchunk):
        dW = (dW + part[ch]).astype(np.float32)
    t = bacc
    while t.shape[-1] > 1:                                                             # (a pairwise tree, as the DPP steps)
        t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    db = np.zeros(C, np.float32)
    for ch in range(nchunk):
        db = (db + t[ch, :, 0]).astype(np.float32)
    return dW, db


# ---------------------------------------------------------------------------------------------------------------------------
# the forward strata
# ---------------------------------------------------------------------------------------------------------------------------
# (refractory, tau_tensor, bias, want_v): every value of every option with every geometry, cycled over the batches
OPTS = [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 0, 0), (0, 0, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0)]


def _geometry_cases(seed):
    out, k = [], 0
    for c_in, geos in ((64, GEO64), (1, GEO1)):
        for h, w in geos:
            for B in FWD_B:
                r, tt, bias, wv = OPTS[k % len(OPTS)]
                out.append(_case("w3-%dto64-%dx%d-B%d" % (c_in, h, w, B), "geometry", seed * 100003 + k, c_in=c_in, h=h, w=w, B=B,
                                 refractory=r, tau_tensor=tt, bias=bias, want_v=wv, rate=.1 if c_in == 64 else .2))
                k += 1
    return out


def _switch_cases(seed):
    """both sides of the 8- / 4-tile switch (2040 tiles: 255 workgroups of eight): the same samples, per-sample results equal;
    B distinct samples, the device runs copies"""
    rows = [(64, 16, 2, 2041, 2040), (64, 8, 4, 2041, 2040), (64, 4, 8, 2041, 2040), (64, 2, 16, 2041, 2040), (64, 1, 32, 2041, 2040),
            (64, 1, 64, 1021, 1020), (64, 3, 128, 171, 170), (64, 16, 64, 64, 63), (1, 1, 32, 2041, 2040), (1, 16, 128, 32, 31)]
    out = []
    for i, (c_in, h, w, B_run, also) in enumerate(rows):
        r, tt, bias, wv = OPTS[(i + 3) % len(OPTS)]
        out.append(_case("w3-switch-%dto64-%dx%d" % (c_in, h, w), "switch", seed * 100003 + 200 + i, c_in=c_in, h=h, w=w, B=3,
                         B_run=B_run, also_B=also, refractory=r, tau_tensor=tt, bias=bias, want_v=1, rate=.1 if c_in == 64 else .2))
    return out


def _grid_cases(seed):
    return [_case("w3-grid", "grid", seed * 100003 + 300, c_in=64, h=4, w=64, B=3, B_run=1100, rate=.1)]


def _readout_cases(seed):
    rows = [("i2o", dict(c_in=64, h=4, w=64, readout=1)), ("i2o-c1", dict(c_in=1, h=2, w=128, readout=1, refractory=0, rate=.2)),
            ("output-layer", dict(c_in=64, h=1, w=32, readout=1, output_layer=1, target=24)),
            ("misalign", dict(c_in=64, h=2, w=16, misalign=1, tau_tensor=1)), ("state0", dict(c_in=64, h=8, w=4, state0=0, rate=.3))]
    return [_case("w3-%s" % n, "readout", seed * 100003 + 400 + i, B=3, **kw) for i, (n, kw) in enumerate(rows)]


def cases(seed=SEED):
    return _geometry_cases(seed) + _switch_cases(seed) + _grid_cases(seed) + _readout_cases(seed)


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    ph = "serves c_in 1 or 64, c_out 64, kernel (1,3)"
    rows = [("cout32", dict(c_out=32), U, ph), ("cin32", dict(c_in=32), U, ph), ("kw5", dict(kw=5, pad_w=2), U, ph),
            ("padw0", dict(pad_w=0), U, ph), ("pool1x1", dict(pool_w=1), U, ph), ("w24", dict(h=4, w=24), U, ph),
            ("w512", dict(h=1, w=512), U, ph), ("hw16", dict(h=1, w=16), U, ph), ("stride2", dict(stride=2), U, ph),
            ("groups2", dict(groups=2), U, ph),
            ("null-x", dict(null="x"), I, "null pointer"), ("null-eps0", dict(null="eps0"), I, "null pointer"),
            ("null-W", dict(null="W"), I, "null pointer"), ("null-s", dict(null="s"), I, "null pointer"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"),
            ("no-out-W", dict(output_layer=1), I, "output layer needs out_W and out_o"),
            ("B-negative", dict(B=-1), I, "negative batch"),
            ("B0", dict(B=0), "DCLL_OK", ""), ("B0-unsupported", dict(B=0, c_out=32), "DCLL_OK", "")]
    base = dict(FZ.CONV_DEFAULT, **W3)
    base.update(c_in=64, h=1, w=32, null=None, B=2, readout=0)
    return [dict(base, id="w3-refuse-%s" % n, code=code, phrase=p, **kw) for n, kw, code, p in rows]


# ---------------------------------------------------------------------------------------------------------------------------
# the backward cases
# ---------------------------------------------------------------------------------------------------------------------------
def bwd_cases(seed=SEED):
    out, k = [], 0
    for c_in, geos in ((64, GEO64), (1, GEO1)):
        for h, w in geos:
            for B in BWD_B:
                # (the readout's gradient g_p on every second case, the output layer's g_o on every fifth)
                out.append(FZ._case("w3-bwd-%dto64-%dx%d-B%d" % (c_in, h, w, B), "backward", seed * 100003 + 1000 + k,
                                    **dict(W3, c_in=c_in, h=h, w=w, B=B, readout=int(k % 2 == 0), output_layer=int(k % 5 == 0 and k % 2 == 0),
                                           target=10)))
                k += 1
    return out


def bwd_draw(c):
    """tensors of a backward case: eps1 as the forward cases carry it, v on a grid of 1/64 in [-4, 4] (distinct values of a pooling
    pair differ by far more than a sigmoid's rounding, equal ones tie: first maximum either way), the gradients as FZ draws them"""
    rng = np.random.RandomState(c["seed"] % (2 ** 31))
    B, cin, cout, h, w = c["B"], c["c_in"], c["c_out"], c["h"], c["w"]
    K = cout * h * (w // 2)
    T = dict(eps1=rng.uniform(0, 12, size=(B, cin, h, w)).astype(np.float32),
             v=(rng.randint(-256, 257, size=(B, cout, h, w)) / 64.0).astype(np.float32),
             i2o_W=(rng.uniform(-1, 1, size=(c["target"], K)) * (.5 / np.sqrt(K))).astype(np.float32),
             g_p=rng.randn(B, c["target"]).astype(np.float32) if c["readout"] else None,
             g_o=rng.randn(B, c["target"]).astype(np.float32) if c["output_layer"] else None,
             g_pv=(rng.randn(B, cout, h, w // 2) * .3).astype(np.float32), g_v=(rng.randn(B, cout, h, w) * .1).astype(np.float32))
    return T


def by_id(cid):
    for c in cases() + refusals() + bwd_cases():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


describe = FZ.describe
cases_hash = FZ.cases_hash


def run(c):
    """(tensors, the oracle's three steps) of a forward case on its c['B'] distinct samples: FZ.conv_run, non-vacuity check included"""
    return FZ.conv_run({k: v for k, v in c.items() if k not in EXTRA})
