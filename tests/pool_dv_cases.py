"""Seeded cases for dcll_conv_lif_backward_ex[_open] with DCLL_BWD_POOL_DV (k_bwd_dv_pool: the opt-in streaming dv kernel of the
layers that pool), built on tests/fuzz_cases.py.

A case is a conv layer (mostly a 1x1 kernel with c_in 1 and padding 0, so that the conv plane is the input plane), a batch, a readout
width and these keys of this list:
    gsel     which of the readout's gradients the call gets: "g_p" (the product's learning step), "g_pv", "both" or "none"
    with_gv  1: g_v is passed as well
    off      bit mask of the pointers placed one float off a 16-byte boundary: OFF_V, OFF_SCRATCH, OFF_GV, OFF_GPV, OFF_W
    draw     "grid" (v on a grid of 1/64: equal membranes give bit-equal sigmoids, exact ties), "neartie" (neighbours nextafter
             apart, 4 <= |v| <= 12: the float32 sigmoids of a window are equal or adjacent), "wide" (|v| up to 40 plus +-inf:
             saturated sigmoids) or "negzero" (grid, with a readout sum that underflows to -0 under a g_pv of -0: the padding terms)
    path     "default", "any", "wide", "slab" or "bands": the entry point dcll_conv_lif_backward_ex names, on a layer it serves
    bands    the band count of path "bands"
Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_pool_dv_cases.py proves the list on the
CPU; tests/test_gpu_pool_dv.py runs the HIP kernel against it.

The served predicate, the launch geometry, the launch-log entry and the kernel's arithmetic are restated ONCE here
(csrc/dcll_bwd_dv_pool.hip: dp_served, dcll_launch_bwd_dv_pool, k_bwd_dv_pool; csrc/dcll_hip.hip: k_bwd_dv)."""
import functools

import numpy as np
import torch

import fuzz_cases as FZ
from dv_w3_cases import DV_ATOL, DV_RTOL        # the formula is the same as there, and so is the tolerance against float64

SEED = 20328
PER_BLOCK = 8           # samples per workgroup (DP_PER_BLOCK)
WINDOWS = 256           # pooled windows per workgroup: one per thread (DP_THREADS)
MAX_TARGET = 32         # more readout rows: the entry point keeps k_bwd_dv
MAX_CHUNKS = 65535      # batch chunks a grid's y takes
INSTANCES = [(ph, pw) for ph in (1, 2, 3) for pw in (1, 2, 3) if (ph, pw) != (1, 1)]
BATCHES = (1, 3, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, 33)          # (around the chunk of 8, of 4 and of 2: 1, 3, 7, 8, 9, 33)
TARGETS = (1, 8, 9, 10, 24, 32, 33)
GSEL = ("g_p", "both", "g_pv", "none")
DRAWS = ("grid", "neartie", "wide")
PATHS = {"default": 0, "any": 1, "wide": 2, "slab": 3, "bands": 4}         # DCLL_BWD_*
POOL_DV = 1                                                                # DCLL_BWD_POOL_DV
OFF_V, OFF_SCRATCH, OFF_GV, OFF_GPV, OFF_W = 1, 2, 4, 8, 16
OFFS = (0, OFF_V, OFF_SCRATCH, OFF_GV, OFF_GPV, OFF_W, 31, 0, OFF_V | OFF_GV, OFF_SCRATCH | OFF_GPV | OFF_W, 0)
ONE = dict(c_in=1, kh=1, kw=1, pad_h=0, pad_w=0)            # the conv plane is the input plane
MNIST = dict(kh=7, kw=7, pad_h=2, pad_w=2)                  # 28x28 -> 26x26 (layer 0), 11x11 -> 9x9 (layer 2)
W3 = dict(kh=1, kw=3, pad_h=0, pad_w=1)                     # radio_ml_conv_ref.yaml's layers

# (pool, plane h x w, c_out): every plane the kernel can go wrong on at its smallest, then the workgroup boundaries in K
_GEOMS = [((2, 2), (2, 2), 1), ((2, 2), (3, 3), 3), ((2, 2), (5, 4), 16), ((2, 2), (9, 9), 3), ((2, 2), (26, 26), 1),
          ((1, 2), (1, 2), 3), ((1, 2), (4, 7), 16), ((1, 2), (2, 16), 33),
          ((2, 1), (7, 1), 16), ((2, 1), (6, 5), 3),
          ((3, 3), (3, 3), 1), ((3, 3), (4, 4), 33), ((3, 3), (6, 9), 3), ((3, 3), (7, 8), 16)]
_GEOMS += [(p, hw, co) for p in ((1, 3), (3, 1), (2, 3), (3, 2)) for hw, co in (((5, 6), 3), ((6, 5), 16))]
_GEOMS += [((2, 2), (10, 34), 3), ((2, 2), (8, 8), 16), ((1, 2), (1, 514), 1),          # K = 255, 256, 257
           ((1, 2), (7, 146), 1), ((2, 2), (8, 16), 16), ((2, 2), (18, 38), 3),         # K = 511, 512, 513
           ((3, 3), (9, 9), 33), ((2, 2), (9, 9), 33), ((3, 3), (6, 6), 16), ((2, 2), (7, 7), 3)]


def cases(seed=SEED):
    out = []

    def add(pool, hw, c_out, B, path="default", bands=0, conv=ONE, c_in=None, **kw):
        k = len(out)
        gsel = kw.pop("gsel", GSEL[k % 4])
        c = FZ._case("dvp-%dx%d-%dx%d-c%d-B%d-%s-%d" % (pool + hw + (c_out, B, path, k)), "backward", seed * 100003 + k,
                     **dict(conv, c_in=conv.get("c_in", 1) if c_in is None else c_in, c_out=c_out, h=hw[0], w=hw[1], pool_h=pool[0],
                            pool_w=pool[1], B=B, readout=int(gsel in ("g_p", "both")), output_layer=int((k // 3) % 2),
                            target=kw.pop("target", TARGETS[k % 7])))
        c.update(gsel=gsel, with_gv=kw.pop("with_gv", int((k // 4) % 2)), off=kw.pop("off", OFFS[k % len(OFFS)]),
                 draw=kw.pop("draw", DRAWS[(k + k // 3) % 3]), path=path, bands=bands)
        assert not kw, kw
        out.append(c)
    for i, (pool, hw, c_out) in enumerate(_GEOMS):
        # (c_out <= 32: the MFMA path of that width too on every other geometry; 33: the wide path)
        kw = dict(target=10) if 22 <= i < 28 and TARGETS[len(out) % 7] > MAX_TARGET else {}       # (the boundaries in K: served)
        add(pool, hw, c_out, BATCHES[i % 6], path=("default", "any")[i % 2] if c_out <= 32 else "wide", **kw)
    # every template instance: pool x readout-width class (8, 16, 24, 32)
    for i, pool in enumerate(INSTANCES):
        for j, target in enumerate((8, 16, 17, 25)):
            add(pool, ((5, 6), (6, 5))[(i + j) % 2], (3, 1)[j % 2], (2, PER_BLOCK + 1)[(i + j) % 2], target=target)
    # the padding terms: a readout sum of -0 under a g_pv of -0, widths with padding terms (9, 10 -> 16; 24 has none: NP = 24)
    add((2, 2), (5, 4), 3, 2, gsel="both", with_gv=0, draw="negzero", target=9)
    add((3, 3), (6, 6), 3, 9, gsel="both", with_gv=0, draw="negzero", target=10, path="any")
    add((1, 2), (4, 7), 3, 2, gsel="both", with_gv=0, draw="negzero", target=1)
    # real kernels: the MNIST layers (16 and 32 channels, pooling 2), every path that serves them
    add((2, 2), (28, 28), 16, 3, conv=MNIST, gsel="g_p", with_gv=0, target=10, draw="grid")
    add((2, 2), (28, 28), 16, 2, path="any", conv=MNIST, gsel="g_p", with_gv=0, target=10, draw="neartie")
    add((2, 2), (11, 11), 32, 3, path="any", conv=MNIST, c_in=24, gsel="g_p", with_gv=0, target=10, draw="grid")
    add((2, 2), (11, 11), 33, 2, path="wide", conv=MNIST, c_in=3, gsel="both", with_gv=1, target=10, draw="wide")
    add((2, 2), (11, 11), 32, 2, path="bands", bands=2, conv=MNIST, c_in=2, gsel="g_p", with_gv=0, target=10, draw="grid")
    # more than 64 channels: the slab path; the bands path forwarding to it (bands 0) and on its own kernel (bands 2)
    add((2, 2), (5, 4), 65, 3, path="slab", target=10)
    add((3, 3), (6, 6), 65, 2, path="bands", bands=0, target=8)
    add((2, 3), (6, 5), 16, 9, path="bands", bands=2, target=24)
    add((3, 2), (6, 5), 33, 3, path="slab", target=32)
    # the (1,2) geometry of radio_ml_conv_ref.yaml at h w = 32: dcll_conv_lif_backward_w3_ex with DCLL_W3_DV serves it too
    add((1, 2), (1, 32), 64, 3, conv=W3, c_in=1, gsel="g_p", with_gv=0, target=24, draw="grid")
    add((1, 2), (2, 16), 64, 9, conv=W3, c_in=64, gsel="both", with_gv=1, target=10, draw="neartie", off=31)
    # the launcher's other path: 512 workgroups and more at PER_BLOCK samples each (K = 65536: 256 x 2 batch chunks) — the only cases
    # of more than a few thousand elements, a fault there cannot show at a smaller size; and one batch chunk less (256 workgroups)
    add((2, 2), (128, 128), 16, PER_BLOCK + 1, gsel="both", with_gv=1, draw="neartie", target=10, off=0)
    add((2, 2), (128, 128), 16, PER_BLOCK, gsel="g_p", with_gv=0, draw="wide", target=10, off=OFF_V)
    add((3, 3), (192, 192), 16, PER_BLOCK + 1, gsel="both", with_gv=1, draw="wide", target=24, off=31)
    # every geometry with uncovered or clipped elements once more on a grid draw with g_v (the elements in no window carry it)
    for pool, hw in sorted({((c["pool_h"], c["pool_w"]), shape(c)[:2]) for c in out if shape(c)[0] < 100}):
        if has_uncovered_or_clipped(dict(ONE, pool_h=pool[0], pool_w=pool[1], h=hw[0], w=hw[1])):
            add(pool, hw, 3, 3, with_gv=1, draw="grid", target=10)
    return out


def by_id(cid):
    for c in cases():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher, restated
# ---------------------------------------------------------------------------------------------------------------------------
def shape(c):
    """(ch, cw, ph, pw), restated (csrc/dcll_internal.h: conv_shape): MaxPool2d(kernel = stride = pool, padding = (pool - 1) // 2)"""
    ch = (c["h"] + 2 * c["pad_h"] - c["dilation"] * (c["kh"] - 1) - 1) // c["stride"] + 1
    cw = (c["w"] + 2 * c["pad_w"] - c["dilation"] * (c["kw"] - 1) - 1) // c["stride"] + 1
    ph = (ch + 2 * ((c["pool_h"] - 1) // 2) - c["pool_h"]) // c["pool_h"] + 1
    pw = (cw + 2 * ((c["pool_w"] - 1) // 2) - c["pool_w"]) // c["pool_w"] + 1
    return ch, cw, ph, pw


def K(c):
    """pooled windows of a sample"""
    _, _, ph, pw = shape(c)
    return c["c_out"] * ph * pw


def served(c, B=None):
    """dcll_launch_bwd_dv_pool takes the call (dcll_bwd_dv_pool_served == 1)"""
    B = c["B"] if B is None else B
    ch, cw, ph, pw = shape(c)
    if not (1 <= c["pool_h"] <= 3 and 1 <= c["pool_w"] <= 3) or (c["pool_h"], c["pool_w"]) == (1, 1):
        return False
    if ch < c["pool_h"] or cw < c["pool_w"] or c["target"] > MAX_TARGET:
        return False
    if c["c_out"] * ph * pw > 2 ** 31 - 1 - WINDOWS or c["c_out"] * ch * cw > 2 ** 31 - 1 - 4 * (cw + 1):
        return False
    return B >= 1 and -(-B // PER_BLOCK) <= MAX_CHUNKS


def NP(c):
    """the template's readout width: target rounded up to 8, at least 8"""
    return max(8, -(-c["target"] // 8) * 8)


MIN_WG = 512            # fewer workgroups than this at PER_BLOCK samples each: one group of samples in flight per workgroup (DP_MIN_WG)


def in_flight(c):
    """samples whose loads are issued before the first is used (dp_group)"""
    return 4 if c["pool_h"] * c["pool_w"] <= 4 else 2


def per_block(c, B=None):
    """samples per workgroup of the launch: PER_BLOCK, or in_flight() where the grid would be small"""
    B = c["B"] if B is None else B
    return in_flight(c) if -(-K(c) // WINDOWS) * -(-B // PER_BLOCK) < MIN_WG else PER_BLOCK


def grid(c, B=None):
    B = c["B"] if B is None else B
    return -(-K(c) // WINDOWS), -(-B // per_block(c, B))


def passed(c):
    """the optional pointers the call passes (non-NULL)"""
    return dict(g_p=c["gsel"] in ("g_p", "both"), g_pv=c["gsel"] in ("g_pv", "both"), g_v=bool(c["with_gv"]),
                i2o_W=c["gsel"] in ("g_p", "both"))


def form_name(c):
    """the launch log's entry for the dv plane with the flag: one form (scalar loads), whatever the alignment"""
    if (c["pool_h"], c["pool_w"]) == (1, 1) and c["target"] <= MAX_TARGET:
        return "k_bwd_dv_nopool<%d>" % NP(c)
    return "k_bwd_dv_pool" if served(c) else "k_bwd_dv"


def all_instances():
    return ["k_bwd_dv_pool<%d,%d,%d>" % (ph, pw, n) for ph, pw in INSTANCES for n in (8, 16, 24, 32)]


def instance_key(c):
    """the template instance a served case runs, as all_instances() spells it"""
    return "k_bwd_dv_pool<%d,%d,%d>" % (c["pool_h"], c["pool_w"], NP(c))


def rowlen(c):
    return (c["c_in"] // c["groups"]) * c["kh"] * c["kw"] + 1


def scratch_floats(c):
    """what the GPU test hands in: the dv plane, min(B, 4) partial rows (every launcher caps its chunks to the room), and the
    output_ gradient's min(B, 16) batch chunks behind them"""
    ch, cw, _, _ = shape(c)
    n = c["B"] * c["c_out"] * ch * cw + min(c["B"], 4) * c["c_out"] * rowlen(c)
    if c["output_layer"]:
        n += min(c["B"], 16) * c["target"] * (K(c) + 1)
    return n


def windows(c):
    """per window element e = (dy, dx) in row-major order: (rows yy (ph,), columns xx (pw,)) — before clipping"""
    ch, cw, ph, pw = shape(c)
    PH, PW = c["pool_h"], c["pool_w"]
    y0, x0 = np.arange(ph) * PH - (PH - 1) // 2, np.arange(pw) * PW - (PW - 1) // 2
    return [(y0 + dy, x0 + dx) for dy in range(PH) for dx in range(PW)]


def coverage(c):
    """(covered (ch, cw) bool: the element is in some window; clipped: some window reaches outside the plane)"""
    ch, cw, ph, pw = shape(c)
    cov, clipped = np.zeros((ch, cw), bool), False
    for yy, xx in windows(c):
        iy, ix = (yy >= 0) & (yy < ch), (xx >= 0) & (xx < cw)
        clipped |= not (iy.all() and ix.all())
        cov[np.ix_(yy[iy], xx[ix])] = True
    return cov, clipped


def has_uncovered_or_clipped(c):
    cov, clipped = coverage(dict(FZ.CONV_DEFAULT, **c))
    return clipped or not cov.all()


# ---------------------------------------------------------------------------------------------------------------------------
# the tensors
# ---------------------------------------------------------------------------------------------------------------------------
def draw(c):
    """the tensors of a case; the gradients it does not pass are None"""
    rng = np.random.RandomState(c["seed"] % (2 ** 31))
    B, cin, cout, N = c["B"], c["c_in"], c["c_out"], c["target"]
    ch, cw, ph, pw = shape(c)
    k = K(c)
    T = dict(eps1=rng.uniform(0, 12, size=(B, cin, c["h"], c["w"])).astype(np.float32),
             v=(rng.randint(-256, 257, size=(B, cout, ch, cw)) / 64.0).astype(np.float32),
             i2o_W=(rng.uniform(-1, 1, size=(N, k)) * (.5 / np.sqrt(k))).astype(np.float32),
             g_p=rng.randn(B, N).astype(np.float32), g_o=rng.randn(B, N).astype(np.float32) if c["output_layer"] else None,
             g_pv=(rng.randn(B, cout, ph, pw) * .3).astype(np.float32), g_v=(rng.randn(B, cout, ch, cw) * .1).astype(np.float32))
    if c["draw"] in ("grid", "negzero"):     # an exact tie for the maximum in every sample and channel: its last window is flat
        y0, x0 = (ph - 1) * c["pool_h"] - (c["pool_h"] - 1) // 2, (pw - 1) * c["pool_w"] - (c["pool_w"] - 1) // 2
        T["v"][:, :, max(y0, 0):y0 + c["pool_h"], max(x0, 0):x0 + c["pool_w"]] = np.float32(1.5)
    if c["draw"] == "neartie":
        u = (rng.uniform(4, 12, size=(B, cout, ph, pw)) * rng.choice([-1.0, 1.0], size=(B, cout, ph, pw))).astype(np.float32)
        py = np.minimum((np.arange(ch) + (c["pool_h"] - 1) // 2) // c["pool_h"], ph - 1)
        px = np.minimum((np.arange(cw) + (c["pool_w"] - 1) // 2) // c["pool_w"], pw - 1)
        base = u[:, :, py][:, :, :, px]
        odd = ((np.arange(ch)[:, None] + np.arange(cw)[None, :]) % 2).astype(bool)
        T["v"] = np.where(odd, np.nextafter(base, np.float32(np.inf)), base).astype(np.float32)
    elif c["draw"] == "wide":
        v = rng.uniform(-40, 40, size=(B, cout, ch, cw)).astype(np.float32)
        r = rng.uniform(size=v.shape)
        v[r < .02], v[r > .98] = -np.inf, np.inf
        T["v"] = v
    elif c["draw"] == "negzero":        # every product g_p W underflows to -0: acc == -0, and g = -0 + -0 == -0
        T["g_p"] = np.full((B, N), -1e-30, np.float32)
        T["i2o_W"] = np.full((N, k), 1e-30, np.float32)
        T["g_pv"] = np.full((B, cout, ph, pw), -0.0, np.float32)
    p = passed(c)
    for key in ("g_p", "g_pv", "g_v", "i2o_W"):
        if not p[key]:
            T[key] = None
    return T


def sigmoid32(v):
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-v.astype(np.float32)))).astype(np.float32)


def _fma32(acc, a, b):
    """fmaf on float32 arrays: the product of two floats is exact in float64, the sum is rounded to float64 and then to float32"""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


UNWRITTEN = np.float32(-3.5)


def winner(c, key, tie_last=False, shift_first=False):
    """per window the flat index y cw + x of its winner: the first maximum of `key` (B, c_out, ch, cw) over the window's in-range
    elements in row-major order, strict > (mutants: tie_last — a tie goes to the LAST maximum; shift_first — clipping is ignored at
    the first pool-3 window: the window that starts at -1 reads the rows / columns 0 .. 2) -> (B, c_out, ph, pw) int64"""
    ch, cw, ph, pw = shape(c)
    win = np.full(key.shape[:2] + (ph, pw), -1, np.int64)
    best = np.zeros(win.shape, key.dtype)
    for yy, xx in windows(c):
        yy, xx = yy.copy(), xx.copy()
        if shift_first and c["pool_h"] == 3:
            yy[0] += 1
        if shift_first and c["pool_w"] == 3:
            xx[0] += 1
        iy, ix = (yy >= 0) & (yy < ch), (xx >= 0) & (xx < cw)
        inr = iy[:, None] & ix[None, :]
        cy, cx = np.clip(yy, 0, ch - 1), np.clip(xx, 0, cw - 1)
        cand = key[:, :, cy][:, :, :, cx]
        take = inr[None, None] & ((win < 0) | ((cand >= best) if tie_last else (cand > best)))
        win = np.where(take, (cy[:, None] * cw + cx[None, :])[None, None], win)
        best = np.where(take, cand, best)
    return win


def dv_restated(c, T, sigmoid=sigmoid32, tie_last=False, over_v=False, skip_uncovered=False, no_clip_first=False, plus0_pad=False):
    """k_bwd_dv's formula in float32, operation by operation, as k_bwd_dv_pool states it: pv = sigmoid(v) of every element; per
    window the first maximum of pv wins; the winner's g = (g_pv or 0) + acc, acc = fmaf(g_p[b][n], i2o_W[n][k], acc) over n in order
    (no sum without g_p); every other element's g is 0; out = g * pv * (1 - pv), + g_v where given -> dv (B, c_out, ch, cw).
    The keyword arguments are the mutants tests/test_pool_dv_cases.py kills."""
    B, cout = c["B"], c["c_out"]
    ch, cw, ph, pw = shape(c)
    k = K(c)
    pv = sigmoid(T["v"])
    g = np.zeros((B, k), np.float32) if T["g_pv"] is None else T["g_pv"].reshape(B, k).astype(np.float32)
    if T["g_p"] is not None:
        acc = np.zeros((B, k), np.float32)
        for n in range(c["target"]):
            acc = _fma32(acc, T["g_p"][:, n:n + 1], T["i2o_W"][n][None, :])
        if plus0_pad:
            for n in range(c["target"], NP(c)):
                acc = _fma32(acc, np.zeros((B, 1), np.float32), np.zeros((1, k), np.float32))
        g = (g + acc).astype(np.float32)
    win = winner(c, T["v"] if over_v else pv, tie_last, no_clip_first)
    gf = np.zeros((B, cout, ch * cw), np.float32)
    np.put_along_axis(gf, win.reshape(B, cout, ph * pw), g.reshape(B, cout, ph * pw), axis=2)
    gf = gf.reshape(B, cout, ch, cw)
    out = ((gf * pv).astype(np.float32) * (np.float32(1) - pv).astype(np.float32)).astype(np.float32)
    if T["g_v"] is not None:
        out = (out + T["g_v"]).astype(np.float32)
    if skip_uncovered:
        out[:, :, ~coverage(c)[0]] = UNWRITTEN
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """float64 dv of a "grid" case from torch autograd through sigmoid / max_pool2d / linear, computed once and shared; read-only.
    The other draws have no float64 reference: the float64 sigmoids route a near tie or a saturated pair differently."""
    c = by_id(cid)
    assert c["draw"] == "grid"
    T = draw(c)
    f64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    v = f64(T["v"]).requires_grad_(True)
    pool = (c["pool_h"], c["pool_w"])
    pvp = torch.nn.functional.max_pool2d(torch.sigmoid(v), pool, pool, ((pool[0] - 1) // 2, (pool[1] - 1) // 2))
    loss = (v * 0).sum()
    if T["g_pv"] is not None:
        loss = loss + (pvp * f64(T["g_pv"])).sum()
    if T["g_p"] is not None:
        loss = loss + (torch.nn.functional.linear(pvp.reshape(c["B"], -1), f64(T["i2o_W"])) * f64(T["g_p"])).sum()
    if T["g_v"] is not None:
        loss = loss + (v * f64(T["g_v"])).sum()
    loss.backward()
    return v.grad.detach()


describe = FZ.describe
cases_hash = FZ.cases_hash
