"""Seeded cases for the opt-in MFMA weight gradient of conv layers with 33 .. 64 output channels
(dcll_conv_lif_backward_wide[_open], k_bwd_wgrad_wide).  Plain module: no GPU, numpy.random.RandomState with fixed seeds only; a
case has the fields of fuzz_cases.CONV_DEFAULT and gets its tensors from fuzz_cases.conv_run (three forward steps with carried
state, the backward after step 3).  tests/test_bwd_wide_cases.py proves the list and the float64 reference on the CPU;
tests/test_gpu_bwd_wide.py runs the HIP kernels against them.

plan() restates the launcher's layout (csrc/dcll_bwd_wide.hip: ww_make_plan; c_out <= 32: bwd_any_cases.plan, the path such a
layer is handed to) so that the list can sit on both sides of each of its thresholds and the GPU test can name the kernel variant
a case must reach:
  strata  named      radio_ml_conv.yaml at netscale 2 and 1.5 on 16x16, mnist_conv.yaml at netscale 2
          shape      c_out / c_in / kernel / plane / padding / pooling / readout edges, one kernel above 64 taps
          edge       LDS, column-split, pixel-split, accumulator-count and batch-chunk thresholds of the launcher
          forwarded  layers of at most 32 output channels (k_bwd_wgrad_any serves them)
          free       uniform draws over the served predicate with c_out in 33 .. 64 under fuzz_cases' work bound
  refusals           descriptors the call refuses before any launch, with code and message
"""
import numpy as np

import bwd_any_cases as BA
import fuzz_cases as FZ

SEED = 20273
LDS_FLOATS = 160 * 1024 // 4
MAX_TPW, MAX_CHUNKS, TARGET_WG, MT = 32, 256, 256, 2
RED_FLOATS = 8 * MT * 16 * 64
MAX_K, MAX_COUT = 16, 64
N_FREE = 40


def plan(c, nchunk=0):
    """The launch layout of dcll_conv_lif_backward_wide for case c with nchunk batch chunks (0: a full launch, what
    dcll_conv_lif_backward_wide_lds reports) -> dict(TPW, nsplit, PS, NQ, lds (bytes), name), or the refusal's message."""
    if not (c["stride"] == 1 and c["dilation"] == 1 and c["groups"] == 1):
        return "plain convolutions only"
    if c["c_out"] > MAX_COUT:
        return "c_out <= 64"
    if c["kh"] > MAX_K or c["kw"] > MAX_K:
        return "kernels up to 16x16"
    if c["c_out"] <= 32:
        return BA.plan(c, nchunk)
    ch, cw, _, _ = FZ.conv_shape(c)
    KK = c["kh"] * c["kw"]
    CF = (c["h"] + 2 * c["pad_h"]) * (c["w"] + 2 * c["pad_w"])
    N = c["c_in"] * KK
    GLD = (ch * (cw + (cw & 1))) | 1
    if CF + 1 + c["c_out"] * GLD > LDS_FLOATS:
        return "exceeds the 160 KiB of LDS"
    NT = (N + 31) // 32

    def floats(tpw):
        channels = max((min((t0 + tpw) * 32, N) - 1) // KK - (t0 * 32) // KK + 1 for t0 in range(0, NT, tpw))
        return ((channels * CF + 1 + 3) & ~3) + c["c_out"] * GLD
    TPW = min(NT, MAX_TPW)
    while True:                 # the full launch: the largest TPW that fits
        if TPW < 1:
            return "exceeds the 160 KiB of LDS"
        lds = floats(TPW)
        if lds <= LDS_FLOATS:
            break
        TPW -= 1
    if 0 < nchunk < TARGET_WG:  # a small batch: fewer tiles per workgroup, never more LDS than the full launch
        want = min(NT, (TARGET_WG + nchunk - 1) // nchunk)
        for tpw in range((NT + want - 1) // want, TPW):
            if floats(tpw) <= max(lds, RED_FLOATS):
                TPW, lds = tpw, floats(tpw)
                break
    lds = max(lds, RED_FLOATS)
    PS = 1 if TPW >= 5 else 2 if TPW >= 3 else 4 if TPW == 2 else 8
    nsplit = (NT + TPW - 1) // TPW
    NQ = 1 if PS > 1 else {1: 1, 2: 2, 3: 4, 4: 4}[(TPW + 7) // 8]
    suffix = [s for s, on in (("column split", nsplit > 1), ("pixel split", PS > 1)) if on]
    name = "k_bwd_wgrad_wide<%d>" % NQ + (" (%s)" % ", ".join(suffix) if suffix else "")
    return dict(TPW=TPW, nsplit=nsplit, PS=PS, NQ=NQ, lds=4 * lds, name=name, NT=NT)


def served(c):
    return FZ.conv_shape(c) is not None and isinstance(plan(c), dict)


def launch_plan(c):
    """The layout of the call ops.conv_lif_backward(wide_path=True) makes for the case: min(B, 256) batch chunks."""
    return plan(c, min(c["B"], MAX_CHUNKS))


VARIANTS = ["k_bwd_wgrad_wide<1>", "k_bwd_wgrad_wide<1> (column split)", "k_bwd_wgrad_wide<1> (pixel split)",
            "k_bwd_wgrad_wide<1> (column split, pixel split)", "k_bwd_wgrad_wide<2>", "k_bwd_wgrad_wide<2> (column split)",
            "k_bwd_wgrad_wide<4>", "k_bwd_wgrad_wide<4> (column split)"]

default_serves = BA.default_serves


def _case(cid, stratum, k, **kw):
    c = FZ._case("bwdwide-%s" % cid, stratum, SEED * 100003 + k, **kw)
    assert served(c), (cid, plan(c))
    assert (c["c_out"] <= 32) == (stratum == "forwarded"), cid
    return c


def _named(out):
    add = lambda name, **kw: out.append(_case(name, "named", len(out), **kw))
    M = dict(kh=7, kw=7, pad_h=2, pad_w=2, target=10, refractory=0)
    R = dict(kh=7, kw=7, pad_h=3, pad_w=3, target=24, tau_tensor=1, h=16, w=16)
    for B in (1, 3, 33):
        for ns, co in (("2", 64), ("1.5", 48)):
            add("radio-ns%s-c1-B%d" % (ns, B), note="radio_ml_conv.yaml at netscale %s: 1 -> %d on 16x16" % (ns, co), c_in=1, c_out=co,
                B=B, **R)
            add("radio-ns%s-c%d-B%d" % (ns, co, B), note="radio_ml_conv.yaml at netscale %s: %d -> %d on 16x16" % (ns, co, co), c_in=co,
                c_out=co, B=B, output_layer=int(B == 3), **R)
        add("mnist-ns2-l2-B%d" % B, note="mnist_conv.yaml at netscale 2: 32 -> 48 on 13x13, pool 1", c_in=32, c_out=48, h=13, w=13, B=B,
            **M)
        add("mnist-ns2-l3-B%d" % B, note="mnist_conv.yaml at netscale 2: 48 -> 64 on 11x11, pool 2, output layer", c_in=48, c_out=64,
            h=11, w=11, pool_h=2, pool_w=2, output_layer=1, B=B, **M)


def _shape(out):
    add = lambda name, **kw: out.append(_case(name, "shape", 200 + len(out), **kw))
    for co in (33, 40, 63, 64):
        add("cout%d" % co, note="c_out %d" % co, c_in=3, c_out=co, h=9, w=8, B=3)
    add("cin1-9cols", note="9 columns (< 32)", c_in=1, c_out=35, B=3)
    add("cin5-45cols", note="odd c_in 5, 45 columns", c_in=5, c_out=37, B=3)
    add("cin33", note="odd c_in 33", c_in=33, c_out=34, h=7, w=7, B=2, tau_tensor=1)
    add("k1x1", note="1x1 kernel", c_in=7, c_out=41, kh=1, kw=1, pad_h=0, pad_w=0, h=6, w=7, B=3)
    add("k2x5", note="2x5 kernel", c_in=3, c_out=50, kh=2, kw=5, pad_h=1, pad_w=2, h=6, w=8, B=3)
    add("cw-odd", note="cw 7, ch cw 35 (odd)", c_in=2, c_out=33, h=5, w=7, B=3)
    add("cw1", note="cw 1", c_in=2, c_out=36, h=6, w=3, pad_w=0, B=3)
    add("chcw1", note="ch cw = 1", c_in=2, c_out=64, h=3, w=3, pad_h=0, pad_w=0, B=5)
    add("pad-0x3", note="padding (0, 3)", c_in=2, c_out=39, kh=3, kw=5, pad_h=0, pad_w=3, h=6, w=6, B=3)
    add("pad-beyond-reach", note="padding 4 around a 2x2 kernel: border outputs see padding only", c_in=2, c_out=44, kh=2, kw=2,
        pad_h=4, pad_w=4, h=5, w=4, B=3)
    add("9x8", note="72 taps (above the default path's 64)", c_in=2, c_out=33, kh=9, kw=8, pad_h=4, pad_w=4, h=10, w=10, B=2)
    k = 0
    for pool in ((1, 1), (2, 2), (3, 2)):
        for readout, outl in ((1, 0), (0, 0), (1, 1)):
            add("pool%dx%d-gp%d-go%d" % (pool + (readout, outl)), note="pooling / readout gradients", c_in=3, c_out=38 + 13 * (k % 3),
                h=9, w=11, pool_h=pool[0], pool_w=pool[1], readout=readout, output_layer=outl, B=4, refractory=k % 2)
            k += 1


def _edge(out):
    add = lambda name, **kw: out.append(_case(name, "edge", 300 + len(out), **kw))
    # the smallest working set at the LDS limit, c_out 64: 628 + 1 + 64 x 629 = 40885 (40888 laid out) floats of 40960
    # (158x4: 632 + 1 + 64 x 633 = 41145, refused)
    add("lds-157x4", note="smallest working set 40885 of 40960 floats", c_in=1, c_out=64, kh=1, kw=1, pad_h=0, pad_w=0, h=157, w=4, B=2,
        target=4)
    # LDS lowers TPW below what the column-tile cap and the batch ask for: 32 channels of 32x32 do not fit beside 33 rows of g
    add("lds-split", note="LDS forces the column split (at most 10 of 32 padded channels fit)", c_in=32, c_out=33, h=30, w=30, B=2,
        target=4)
    # column tiles per workgroup at B = 256 (no split for the batch's sake): pixel split 8 / 4 / 2 / 2 / 1, column tiles per wave
    # 1 / 2 / 4, the 32-tile cap.  4x8 kernel: 32 columns per input channel
    T = dict(kh=4, kw=8, pad_h=1, pad_w=3, h=5, w=9, B=256, target=3, rate=.4)
    for i, nt in enumerate((1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 32, 33)):
        add("tiles%d-B256" % nt, note="%d column tiles, 256 chunks" % nt, c_in=nt, c_out=(33, 36, 64)[i % 3], **T)
    add("tiles5-B255", note="255 chunks: the batch asks for two column splits", c_in=5, c_out=34, **dict(T, B=255))
    add("tiles16-B128", note="<1> column split without pixel split", c_in=16, c_out=35, **dict(T, B=128))
    add("tiles24-B128", note="<2> column split", c_in=24, c_out=64, **dict(T, B=128))
    add("tiles12-B257", note="257 samples on 256 chunks: chunk 0 sums two", c_in=12, c_out=40, **dict(T, B=257))
    add("tiles2-B600", note="600 samples on 256 chunks (2 or 3 each)", c_in=2, c_out=33, **dict(T, B=600))


def _forwarded(out):
    add = lambda name, **kw: out.append(_case(name, "forwarded", 400 + len(out), **kw))
    add("fwd-cout32", note="c_out 32: k_bwd_wgrad_any", c_in=3, c_out=32, h=9, w=8, B=3)
    add("fwd-cout5-pool", note="c_out 5, pool 2, output layer", c_in=5, c_out=5, h=9, w=11, pool_h=2, pool_w=2, output_layer=1, B=4)
    add("fwd-mnist-l1", note="mnist_conv.yaml at netscale 2: 1 -> 32 on 28x28, pool 2", c_in=1, c_out=32, kh=7, kw=7, pad_h=2, pad_w=2,
        h=28, w=28, pool_h=2, pool_w=2, target=10, refractory=0, B=3)


def _free_draw(rng, k):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(33, 65)), kh=int(rng.randint(1, 17)), kw=int(rng.randint(1, 17)),
                 pad_h=int(rng.randint(0, 6)), pad_w=int(rng.randint(0, 6)), pool_h=int(rng.randint(1, 4)),
                 pool_w=int(rng.randint(1, 4)), h=int(rng.randint(1, 31)), w=int(rng.randint(1, 31)),
                 refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5), bias=int(rng.rand() < .75),
                 target=int(rng.randint(1, 41)), readout=int(rng.rand() >= .07), output_layer=int(rng.rand() < 1. / 3),
                 B=int(FZ.B_SET[rng.randint(len(FZ.B_SET))]), rate=float(np.round(rng.uniform(.05, .5), 3)),
                 state0=int(rng.rand() < .5))
        if not c["readout"]:
            c["output_layer"] = 0
        full = dict(FZ.CONV_DEFAULT, **c)
        if FZ.conv_shape(full) is None or not FZ.sees_input(full) or not served(full):
            continue
        ch, cw, _, _ = FZ.conv_shape(full)
        per_sample = c["c_out"] * ch * cw * c["c_in"] * c["kh"] * c["kw"]
        bmax = int(min(FZ.WORK_MAX // per_sample, FZ.ELEMS_MAX // (c["c_in"] * c["h"] * c["w"]), FZ.ELEMS_MAX // (c["c_out"] * ch * cw)))
        if bmax < 1:
            continue
        if c["B"] > bmax:
            ok = [b for b in FZ.B_SET if b <= bmax]
            c["B"] = int(ok[rng.randint(len(ok))])
        return _case("free-%02d" % k, "free", 1000 + k, **c)


def cases(seed=SEED):
    out = []
    _named(out)
    _shape(out)
    _edge(out)
    _forwarded(out)
    rng = np.random.RandomState(seed)
    return out + [_free_draw(rng, k) for k in range(N_FREE)]


def refusals():
    """(case, code name, message part): refused before any launch.  The scratch case is served; its call passes one float too few."""
    r = lambda name, k, **kw: FZ._case("bwdwide-refuse-%s" % name, "refuse", SEED * 100003 + 2000 + k, **kw)
    S = dict(c_in=2, c_out=40, h=10, w=10, B=2)
    return [
        (r("cout65", 0, **dict(S, c_out=65)), "UNSUPPORTED", "c_out <= 64"),
        (r("kh17", 1, **dict(S, kh=17, kw=3, pad_h=8)), "UNSUPPORTED", "kernels up to 16x16"),
        (r("stride2", 2, **dict(S, stride=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("dilation2", 3, **dict(S, dilation=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("groups2", 4, **dict(S, groups=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("lds-158x4", 5, c_in=1, c_out=64, kh=1, kw=1, pad_h=0, pad_w=0, h=158, w=4, B=2, target=4), "UNSUPPORTED",
         "exceeds the 160 KiB of LDS"),
        (r("scratch", 6, **S), "INVALID", "scratch too small"),
    ]


def exact_draw(c):
    """Small integers for the case's geometry: g_v in {-2 .. 2}, eps1 in {0 .. 3}; with g_p = g_pv = NULL k_bwd_dv writes g_v
    itself, and every product and partial sum is an integer of magnitude <= 6 x B x pixels < 2^24: exact in float32 in ANY
    summation order -> g_v, eps1, v (any values: unused without g_p / g_pv) and the integer dW, db."""
    rng = np.random.RandomState((c["seed"] + 77) % (2 ** 31))
    ch, cw, _, _ = FZ.conv_shape(c)
    B, ci, co, h, w = c["B"], c["c_in"], c["c_out"], c["h"], c["w"]
    assert 6 * B * ch * cw < 1 << 24
    g_v = rng.randint(-2, 3, size=(B, co, ch, cw))
    eps1 = rng.randint(0, 4, size=(B, ci, h, w))
    v = (rng.randint(-256, 257, size=(B, co, ch, cw)) / 64.0).astype(np.float32)
    ep = np.pad(eps1, ((0, 0), (0, 0), (c["pad_h"],) * 2, (c["pad_w"],) * 2)).astype(np.int64)
    dW = np.zeros((co, ci, c["kh"], c["kw"]), np.int64)
    g2 = g_v.reshape(B, co, ch * cw).astype(np.int64)
    for ty in range(c["kh"]):
        for tx in range(c["kw"]):
            win = ep[:, :, ty:ty + ch, tx:tx + cw].reshape(B, ci, ch * cw)
            dW[:, :, ty, tx] = np.einsum("bop,bip->oi", g2, win)
    return dict(g_v=g_v.astype(np.float32), eps1=eps1.astype(np.float32), v=v, dW=dW.astype(np.float64),
                db=g2.sum(axis=(0, 2)).astype(np.float64))


def by_id(cid):
    for c in cases() + [r[0] for r in refusals()]:
        if c["id"] == cid:
            return c
    raise KeyError(cid)
