"""Seeded cases for dcll_conv_lif_backward_w3_ex[_open] with DCLL_W3_DV (k_bwd_dv_w3: the opt-in streaming dv kernel of the
(1,3)-kernel / (1,2)-pool layers of radio_ml_conv_ref.yaml), built on tests/step_w3_cases.py and tests/fuzz_cases.py.

A case is a plane, a batch, a readout width and these keys of this list:
    gsel     which of the readout's gradients the call gets: "g_p" (the product's learning step), "g_pv", "both" or "none"
    with_gv  1: g_v is passed as well
    off      bit mask of the pointers placed one float off a 16-byte boundary: OFF_V, OFF_SCRATCH, OFF_GV, OFF_GPV, OFF_W
    draw     "grid" (S.bwd_draw: v on a grid of 1/64, exact ties), "neartie" (v[2k + 1] = nextafter(v[2k], +inf), 4 <= |v| <= 12:
             the float32 sigmoids of a pair are equal or adjacent) or "wide" (|v| up to 40: saturated sigmoids, finite values)
    first    1: DCLL_W3_FIRST_WGRAD as well (flags 3), 0: flags 2
    scratch  "ops" (the size ops.conv_lif_backward allocates) or "k1" (exactly one partial row, through the C ABI)
Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_dv_w3_cases.py proves the list on the
CPU; tests/test_gpu_dv_w3.py runs the HIP kernel against it.

The launcher and the kernel's arithmetic are restated ONCE here (csrc/dcll_step_w3.hip: dcll_launch_bwd_dv_w3, k_bwd_dv_w3;
csrc/dcll_hip.hip: k_bwd_dv, conv_lif_backward_impl).  There is no K * B fallback: the kernel serves every batch of a served layer
with target <= 32 (profiles/r15_w3_dv_timing.txt: no layer of the network is slower with it)."""
import functools

import numpy as np

import fuzz_cases as FZ
import step_w3_cases as S

SEED = 20291
PER_BLOCK = 8           # samples per workgroup (DW_PER_BLOCK)
POS = 512               # pooled positions per workgroup: 256 threads x 2 (DW_POS)
MAX_TARGET = 32         # more readout rows: the entry point keeps k_bwd_dv
PLANES = [(16, 2), (1, 32), (2, 16), (1, 256), (4, 64)]
BATCHES = (1, 3, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, 33)
TARGETS = (1, 8, 9, 10, 24, 32, 33)
GSEL = ("g_p", "both", "g_pv", "none")
DRAWS = ("grid", "neartie", "wide")
OFF_V, OFF_SCRATCH, OFF_GV, OFF_GPV, OFF_W = 1, 2, 4, 8, 16
OFFS = (0, OFF_V, OFF_SCRATCH, OFF_GV, OFF_GPV, OFF_W, 31, 0, OFF_V | OFF_GV, OFF_SCRATCH | OFF_GPV | OFF_W, 0)
# dv against float64 on the "grid" draws: rtol, atol = DV_ATOL * max|ref|.  The float32 restatement of the formula stays inside it
# on every such case (tests/test_dv_w3_cases.py prints the worst excess), so it stands as the issue gives it
DV_RTOL, DV_ATOL = 1e-5, 1e-6
NEARTIE_EQUAL_FLOOR = .25


def cases(seed=SEED):
    out, k = [], 0
    rows = [(h, w, B) for h, w in PLANES for B in BATCHES] + [(16, 128, 1), (16, 128, 3), (16, 128, 2)]
    rows += [(4, 64, 3), (1, 32, 17), (2, 16, 33), (16, 2, 16), (1, 256, 15)]
    for h, w, B in rows:
        gsel, with_gv = GSEL[k % 4], int((k // 4) % 2)
        if (h, w) == (16, 128):
            gsel, with_gv = ("g_p", 0) if B != 2 else ("both", 1)            # (the product's call on the product's plane)
        c = FZ._case("dvw3-%dx%d-B%d-%d" % (h, w, B, k), "backward", seed * 100003 + k,
                     **dict(S.W3, c_in=(1, 64)[(k // 2) % 2], h=h, w=w, B=B, readout=int(gsel in ("g_p", "both")),
                            output_layer=int((k // 3) % 2), target=TARGETS[k % 7]))
        c.update(gsel=gsel, with_gv=with_gv, off=OFFS[k % len(OFFS)], draw=DRAWS[(k + k // 3) % 3], first=int((k // 5) % 2),
                 scratch=("ops", "k1")[int(k % 5 == 3)])
        out.append(c)
        k += 1
    return out


def by_id(cid):
    for c in cases():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher, restated
# ---------------------------------------------------------------------------------------------------------------------------
def K(c):
    """pooled positions of a sample: 64 channels x h x w / 2 (a multiple of 1024: h w % 32 == 0)"""
    return 32 * c["h"] * c["w"]


def served(c):
    """dcll_launch_bwd_dv_w3 takes the call: a layer dcll_bwd_w3_check serves, at most 32 readout rows"""
    return S.served(c) is None and c["target"] <= MAX_TARGET


def NP(c):
    """the template's readout width: target rounded up to 8, at least 8"""
    return max(8, -(-c["target"] // 8) * 8)


def grid(c, B=None):
    B = c["B"] if B is None else B
    return K(c) // POS, -(-B // PER_BLOCK)


def passed(c):
    """the optional pointers the call passes (non-NULL)"""
    return dict(g_p=c["gsel"] in ("g_p", "both"), g_pv=c["gsel"] in ("g_pv", "both"), g_v=bool(c["with_gv"]),
                i2o_W=c["gsel"] in ("g_p", "both"))


def vector_form(c, off=None):
    """the 16-byte form: v, scratch and g_v 16-byte aligned and g_pv and i2o_W 8-byte aligned — a NULL pointer is aligned"""
    off = c["off"] if off is None else off
    p = passed(c)
    return not (off & (OFF_V | OFF_SCRATCH) or (off & OFF_GV and p["g_v"]) or (off & OFF_GPV and p["g_pv"]) or
                (off & OFF_W and p["i2o_W"]))


def form_name(c, off=None):
    """the launch log's entry for the dv plane"""
    if not served(c):
        return "k_bwd_dv"
    return "k_bwd_dv_w3" if vector_form(c, off) else "k_bwd_dv_w3 (unaligned)"


def all_forms():
    return ["k_bwd_dv_w3<%d>%s" % (n, a) for n in (8, 16, 24, 32) for a in ("", " (unaligned)")]


def form_key(c, off=None):
    """(template width, alignment) of the kernel a served case runs, as all_forms() spells it"""
    return "k_bwd_dv_w3<%d>%s" % (NP(c), "" if vector_form(c, off) else " (unaligned)")


def ops_room(c):
    """partial rows ops.conv_lif_backward(w3_path=True, w3_first=c['first']) makes room for"""
    B, h, w = c["B"], c["h"], c["w"]
    if c["c_in"] == 64 or c["first"]:
        return min(-(-B * h * w // 128), 256)
    return min(B * max(1, (h // 16) * (w // 16)), 1024)


def room(c):
    return ops_room(c) if c["scratch"] == "ops" else 1


# ---------------------------------------------------------------------------------------------------------------------------
# the tensors
# ---------------------------------------------------------------------------------------------------------------------------
def draw(c):
    """S.bwd_draw's tensors with v redrawn for the "neartie" and "wide" draws, g_o for every output-layer case and the gradients
    the case does not pass set to None"""
    T = S.bwd_draw(dict(c, readout=1))
    rng = np.random.RandomState((c["seed"] + 4711) % (2 ** 31))
    B, h, w = c["B"], c["h"], c["w"]
    if c["draw"] == "neartie":
        left = (rng.uniform(4, 12, size=(B, 64, h, w // 2)) * rng.choice([-1.0, 1.0], size=(B, 64, h, w // 2))).astype(np.float32)
        v = np.empty((B, 64, h, w), np.float32)
        v[..., 0::2] = left
        v[..., 1::2] = np.nextafter(left, np.float32(np.inf))
        T["v"] = v
    elif c["draw"] == "wide":
        T["v"] = rng.uniform(-40, 40, size=(B, 64, h, w)).astype(np.float32)
    p = passed(c)
    for k in ("g_p", "g_pv", "g_v", "i2o_W"):
        if not p[k]:
            T[k] = None
    assert all(np.isfinite(t).all() for t in T.values() if t is not None)
    return T


def sigmoid32(v):
    return (np.float32(1) / (np.float32(1) + np.exp(-v.astype(np.float32)))).astype(np.float32)


def dv_restated(c, T, sigmoid=sigmoid32):
    """k_bwd_dv's formula on a (1,2) pooling in float32, operation by operation: pv = sigmoid(v) of both elements of a pair;
    element 0 wins unless pv1 > pv0; the winner's g = (g_pv or 0) + acc, acc = fmaf(g_p[b][n], i2o_W[n][k], acc) over n in order
    (no sum without g_p); out = g * pv * (1 - pv), + g_v where given -> dv (B, 64, h, w) float32"""
    B, h, w = c["B"], c["h"], c["w"]
    pv = sigmoid(T["v"])
    g = np.zeros((B, K(c)), np.float32) if T["g_pv"] is None else T["g_pv"].reshape(B, K(c)).astype(np.float32)
    if T["g_p"] is not None:
        acc = np.zeros((B, K(c)), np.float32)
        for n in range(c["target"]):
            acc = S._fma32(acc, T["g_p"][:, n:n + 1], T["i2o_W"][n][None, :])
        g = (g + acc).astype(np.float32)
    g = g.reshape(B, 64, h, w // 2)
    right = pv[..., 1::2] > pv[..., 0::2]
    gf = np.zeros((B, 64, h, w), np.float32)
    gf[..., 0::2] = np.where(right, np.float32(0), g)
    gf[..., 1::2] = np.where(right, g, np.float32(0))
    out = ((gf * pv).astype(np.float32) * (np.float32(1) - pv).astype(np.float32)).astype(np.float32)
    if T["g_v"] is not None:
        out = (out + T["g_v"]).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """float64 gradients of a "grid" case (FZ.conv_backward_ref), computed once and shared: dict(dW, db, d_outW, d_outb, dv);
    read-only.  The other draws have no float64 reference: first_max_route on float64 sigmoids routes a near tie differently."""
    c = by_id(cid)
    assert c["draw"] == "grid"
    T = draw(c)
    Tr = dict(T)
    if Tr["g_pv"] is None:
        Tr["g_pv"] = np.zeros((c["B"], 64, c["h"], c["w"] // 2), np.float32)
    if not c["output_layer"]:
        Tr["g_o"] = None
    route = FZ.first_max_route(c, FZ._f64(T["v"]))
    return FZ.conv_backward_ref(c, Tr, T["v"], T["eps1"], route, zero_g_v=T["g_v"] is None)


describe = FZ.describe
cases_hash = FZ.cases_hash
