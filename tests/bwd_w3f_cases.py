"""Seeded cases for dcll_conv_lif_backward_w3f[_open] (k_bwd_wgrad_w3f: the opt-in streaming weight gradient of the FIRST layer,
c_in 1 -> 64, of the (1,3)-kernel / (1,2)-pool geometry of radio_ml_conv_ref.yaml), built on tests/step_w3_cases.py and
tests/fuzz_cases.py.

A case is a plane, a batch and three keys of this list:
    scratch   "ops" (the size ops.conv_lif_backward allocates), "k1" (exactly one partial row), "k3" (three)
    misalign  1: eps1 and scratch one float off a 16-byte boundary (the scalar-load form)
    gsel      which of the readout's gradients the call gets: "g_p", "g_pv" or "both"   (output_layer: g_o as well)
S.bwd_draw() gives the tensors.  Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.
tests/test_bwd_w3f_cases.py proves the list on the CPU; tests/test_gpu_bwd_w3f.py runs the HIP kernel against it.

The launcher and the kernel's summation order are restated ONCE here (csrc/dcll_step_w3.hip: dcll_launch_bwd_wgrad_w3f,
k_bwd_wgrad_w3f; csrc/dcll_hip.hip: conv_lif_backward_impl's reduction dispatch)."""
import functools

import numpy as np

import fuzz_cases as FZ
import step_w3_cases as S

SEED = 20281
PB = 128                # pixels of a job (WF_PB)
MAX_CHUNKS = 256        # partial rows, at most (WF_MAX_CHUNKS)
PLANES = [(16, 128), (16, 2), (1, 32), (2, 16), (4, 64), (1, 256), (2, 256), (2, 128)]
BATCHES = (1, 3, 33, 257)
GRAD_RTOL, GRAD_ATOL = S.GRAD_RTOL, S.GRAD_ATOL
SCRATCH = ("ops", "k1", "k3")
GSEL = ("both", "g_p", "g_pv")


def cases(seed=SEED):
    out, k = [], 0
    for h, w in PLANES:
        for B in BATCHES:
            if (h, w) == (16, 128) and B > 33:
                continue
            c = FZ._case("w3f-%dx%d-B%d" % (h, w, B), "backward", seed * 100003 + k,
                         **dict(S.W3, c_in=1, h=h, w=w, B=B, readout=1, output_layer=int((k // 2) % 2), target=10))
            # (the three scratch rules, both alignments and the three gradient selections cycle with different periods)
            c.update(scratch=SCRATCH[k % 3], misalign=int((k + k // 4) % 2), gsel=GSEL[(k // 3) % 3])
            out.append(c)
            k += 1
    return out


def by_id(cid):
    for c in cases():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def draw(c):
    """S.bwd_draw's tensors with the gradients the case does not pass set to None"""
    T = S.bwd_draw(c)
    if c["gsel"] == "g_p":
        T["g_pv"] = None
    if c["gsel"] == "g_pv":
        T["g_p"] = None
    return T


@functools.lru_cache(maxsize=None)
def reference(cid):
    """float64 gradients of a case (FZ.conv_backward_ref), computed once and shared: dict(dW, db, d_outW, d_outb, dv); read-only"""
    c = by_id(cid)
    T = draw(c)
    Tr = dict(T)
    if Tr["g_pv"] is None:
        Tr["g_pv"] = np.zeros((c["B"], 64, c["h"], c["w"] // 2), np.float32)
    route = FZ.first_max_route(c, FZ._f64(T["v"]))
    return FZ.conv_backward_ref(c, Tr, T["v"], T["eps1"], route)


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher, restated
# ---------------------------------------------------------------------------------------------------------------------------
def npix(c, B=None):
    return (c["B"] if B is None else B) * c["h"] * c["w"]


def jobs(c, B=None):
    """jobs of the flattened (B x h w) pixel stream: ceil(pixels / PB)"""
    return -(-npix(c, B) // PB)


def chunks(c, B=None, room=MAX_CHUNKS):
    """partial rows of a launch with room for `room`: at most 256, at most one per job"""
    return min(room, MAX_CHUNKS, jobs(c, B))


def ops_chunks(c, B=None):
    """the rows ops.conv_lif_backward(w3_first=True) makes room for"""
    return min(jobs(c, B), MAX_CHUNKS)


def room(c):
    """partial rows the case's scratch rule has room for"""
    return dict(ops=ops_chunks(c), k1=1, k3=3)[c["scratch"]]


def scratch_floats(c):
    """the case's scratch: the dv plane, the partial rows of 64 x 4 floats (ops: + nothing, K % 32 == 0 runs k_bwd_outgrad_mfma)"""
    return c["B"] * 64 * c["h"] * c["w"] + room(c) * 64 * 4


def job_lists(c, nchunk, B=None):
    """[chunk][jp] -> the jobs wave parity jp of workgroup `chunk` takes, in its order: the chunk's list chunk, chunk + nchunk, ...
    split into even (jp 0) and odd (jp 1) positions"""
    n = jobs(c, B)
    out = []
    for k in range(nchunk):
        lst = list(range(k, n, nchunk))
        out.append((lst[0::2], lst[1::2]))
    return out


def lane_pixels(c, J, B=None):
    """(first stream pixel of each lane q = 0 .. 31 of job J, live mask): lane q owns 4 pixels from 128 J + 4 q; live = inside the
    stream (the kernel's tile test G < ntot)"""
    p0 = PB * J + 4 * np.arange(32)
    return p0, p0 < npix(c, B)


def neighbour_reads(c, p0):
    """the kernel's own index arithmetic for the two reads outside a lane's 4 pixels at stream pixel p0 (arrays): (left index or
    -1, right index or -1) as stream pixels"""
    w = c["w"]
    x0 = p0 & (w - 1)                               # (h w % 32 == 0 and p0 % 4 == 0: the column of the first pixel)
    left = np.where(x0 != 0, p0 - 1, -1)
    right = np.where(((x0 + 3) & (w - 1)) != w - 1, p0 + 4, -1)
    return left, right


def wgrad_name(c):
    return "k_bwd_wgrad_w3f (unaligned)" if c["misalign"] else "k_bwd_wgrad_w3f"


def reduce_name(nchunk):
    """conv_lif_backward_impl's closed form"""
    return "k_bwd_reduce4<16>" if nchunk >= 64 else "k_bwd_reduce4<4>" if nchunk >= 16 else "k_bwd_reduce"


# ---------------------------------------------------------------------------------------------------------------------------
# the summation order, restated in float32
# ---------------------------------------------------------------------------------------------------------------------------
_fma32 = S._fma32


def _add32(a, b):
    return (a + b).astype(np.float32)


def fma_ld(acc, a, b):
    """fmaf on float32 arrays through long double (64-bit significand on x86: the product is exact, the sum is rounded to 64 bits
    and then to 24 — a double rounding in one case of ~2^40, against ~2^29 through float64): for bit-for-bit comparisons"""
    ld = np.longdouble
    return (acc.astype(ld) + a.astype(ld) * b.astype(ld)).astype(np.float32)


def half_tree(v):
    """half_sum_to_lane31 on the last axis (32 lanes) -> the value of lane 31"""
    q = np.arange(32)
    v = _add32(v, v[..., q ^ 1])
    v = _add32(v, v[..., q ^ 2])
    v = _add32(v, v[..., (q & ~7) | (7 - (q & 7))])
    v = _add32(v, v[..., (q & ~15) | (15 - (q & 15))])
    return _add32(v[..., 31], v[..., 15])


def streams(g, eps1):
    """g (B, 64, h, w), eps1 (B, 1, h, w) -> (gs (64, NP), eL, eC, eR (NP,)): the flattened streams, zero beyond a row's ends"""
    B, C, h, w = g.shape
    gs = np.ascontiguousarray(g.transpose(1, 0, 2, 3)).reshape(C, B * h * w)
    ep = np.zeros((B, h, w + 2), eps1.dtype)
    ep[:, :, 1:-1] = eps1[:, 0]
    return gs, ep[:, :, 0:w].reshape(-1), ep[:, :, 1:w + 1].reshape(-1), ep[:, :, 2:w + 2].reshape(-1)


def wgrad_restated(g, eps1, nchunk, fma=_fma32):
    """k_bwd_wgrad_w3f's summation order in float32: g (B, 64, h, w), eps1 (B, 1, h, w) float32 -> (part (nchunk, 64, 4), dW (64, 3),
    db (64,)).  Chunk k takes the jobs k, k + nchunk, ...; the jobs at even / odd positions of that list are wave parity jp = 0 /
    1; lane q runs the pixels 4 q .. 4 q + 3 of its wave's jobs in order (fma per tap, add for the bias); the 32 lanes by
    half_tree; jp 0 + jp 1.  The chunks are then added in order (k_bwd_reduce's plain sum: k_bwd_reduce4's grouping differs in the
    last bit only).  `fma`: the float32 fused multiply-add (fma_ld: through long double, for a bit-for-bit comparison)."""
    gs, eL, eC, eR = streams(g, eps1)
    C, NP = gs.shape
    n = -(-NP // PB)
    pad = n * PB - NP
    gs = np.pad(gs, ((0, 0), (0, pad))).reshape(C, n, 32, 4)            # (zeros: fma(0, 0, a) = a, a + 0 = a — a skipped lane)
    E = np.stack([np.pad(e, (0, pad)).reshape(n, 32, 4) for e in (eL, eC, eR)])        # (3, job, lane, j)
    acc = np.zeros((2, nchunk, C, 32, 4), np.float32)                   # [jp][chunk][co][lane][kx 0, kx 1, kx 2, bias]
    for i in range(-(-n // nchunk)):
        J = np.arange(nchunk) + i * nchunk
        live = J < n
        Ji = np.where(live, J, 0)
        gb = np.where(live[None, :, None, None], gs[:, Ji], 0).transpose(1, 0, 2, 3)   # (chunk, co, lane, j)
        eb = np.where(live[None, :, None, None], E[:, Ji], 0)                          # (3, chunk, lane, j)
        a = acc[i & 1]
        for j in range(4):
            for kx in range(3):
                a[..., kx] = fma(a[..., kx], gb[..., j], eb[kx][:, None, :, j])
            a[..., 3] = _add32(a[..., 3], gb[..., j])
    tot = half_tree(acc.transpose(0, 1, 2, 4, 3))                       # (jp, chunk, co, 4)
    part = _add32(tot[0], tot[1])
    red = np.zeros((C, 4), np.float32)
    for k in range(nchunk):
        red = _add32(red, part[k])
    return part, red[:, :3], red[:, 3]


def exact_draw(c):
    """small integers: g_v in {-2 .. 2}, eps1 in {0 .. 3}; with g_p = g_pv = NULL k_bwd_dv writes g_v itself, and every product and
    partial sum is an integer of magnitude <= 6 x pixels < 2^24: exact in float32 in ANY summation order"""
    rng = np.random.RandomState((c["seed"] + 77) % (2 ** 31))
    B, h, w = c["B"], c["h"], c["w"]
    assert 6 * B * h * w < 1 << 24
    g_v = rng.randint(-2, 3, size=(B, 64, h, w)).astype(np.float32)
    eps1 = rng.randint(0, 4, size=(B, 1, h, w)).astype(np.float32)
    v = (rng.randint(-256, 257, size=(B, 64, h, w)) / 64.0).astype(np.float32)
    gs, eL, eC, eR = streams(g_v.astype(np.int64), eps1.astype(np.int64))
    dW = np.stack([gs @ e for e in (eL, eC, eR)], axis=1)
    return dict(g_v=g_v, eps1=eps1, v=v, dW=dW, db=gs.sum(axis=1))


describe = FZ.describe
cases_hash = FZ.cases_hash
