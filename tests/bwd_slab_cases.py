"""Seeded cases for the opt-in MFMA weight gradient of conv layers with MORE than 64 output channels
(dcll_conv_lif_backward_slab[_open], k_bwd_wgrad_slab).  Plain module: no GPU, numpy.random.RandomState with fixed seeds only; a
case has the fields of fuzz_cases.CONV_DEFAULT and gets its tensors from fuzz_cases.conv_run (three forward steps with carried
state, the backward after step 3).  tests/test_bwd_slab_cases.py proves the list and the float64 reference on the CPU;
tests/test_gpu_bwd_slab.py runs the HIP kernels against them.

The slab rule (csrc/dcll_any_shared.h), restated: NS = ceil(c_out / 64); slab s owns the output channels
[64 s, min(64 s + 64, c_out)); rows at or beyond c_out are never stored; NS <= 65 535; c_out <= 64 is handed to
dcll_conv_lif_backward_wide unchanged (bwd_wide_cases.plan).

plan() restates the launcher's layout (csrc/dcll_bwd_slab.hip: ws_make_plan) so that the list can sit on both sides of each of
its thresholds and the GPU test can name the kernel variant a case must reach:
  strata  named      radio_ml_conv.yaml at netscale 3 and 4 on 16x16 (1 -> 96 / 128, 96 -> 96, 128 -> 128), B = 1
          shape      c_out 65 / 96 / 97 / 128 / 129 / 200, c_in 1 / 3 / 64 / 70, kernels 1x1 .. 9x9, odd planes, planes of 9 / 32 /
                     33 conv pixels, poolings 1 / 2 / 3 / (1,2), refractory and plain, B = 1 / 3 / 33 / 257
          edge       LDS, column-split, pixel-split, accumulator-count and small-batch thresholds of the launcher, NS in the rule
          forwarded  layers of 40 and 64 output channels (k_bwd_wgrad_wide serves them)
          free       uniform draws over the served predicate with c_out in 65 .. 200 under fuzz_cases' work bound
  refusals           descriptors the call refuses before any launch, with code and message
"""
import numpy as np

import bwd_wide_cases as BW
import fuzz_cases as FZ

SEED = 20311
LDS_FLOATS = 160 * 1024 // 4
MAX_TPW, MAX_CHUNKS, TARGET_WG, MT = 32, 256, 256, 2
RED_FLOATS = 8 * MT * 16 * 64
MAX_K, SLAB_ROWS, SLAB_MAX = 16, 64, 65535
N_FREE = 30


def slab_count(c_out):
    return (c_out + SLAB_ROWS - 1) // SLAB_ROWS


def slabs(c_out):
    """[(first channel, channels)] of the slabs of a layer."""
    return [(SLAB_ROWS * s, min(SLAB_ROWS, c_out - SLAB_ROWS * s)) for s in range(slab_count(c_out))]


def plan(c, nchunk=0):
    """The launch layout of dcll_conv_lif_backward_slab for case c with nchunk batch chunks (0: a full launch, what
    dcll_conv_lif_backward_slab_lds reports) -> dict(TPW, nsplit, PS, NQ, NS, lds (bytes), name), or the refusal's message."""
    if c["c_out"] <= SLAB_ROWS:
        return BW.plan(c, nchunk)
    if not (c["stride"] == 1 and c["dilation"] == 1 and c["groups"] == 1):
        return "plain convolutions only"
    if c["kh"] > MAX_K or c["kw"] > MAX_K:
        return "kernels up to 16x16"
    NS = slab_count(c["c_out"])
    if NS > SLAB_MAX:
        return "more than 65535 slabs"
    ch, cw, _, _ = FZ.conv_shape(c)
    KK = c["kh"] * c["kw"]
    CF = (c["h"] + 2 * c["pad_h"]) * (c["w"] + 2 * c["pad_w"])
    N = c["c_in"] * KK
    GLD = (ch * (cw + (cw & 1))) | 1
    if CF + 1 + SLAB_ROWS * GLD > LDS_FLOATS:
        return "exceeds the 160 KiB of LDS"
    NT = (N + 31) // 32

    def floats(tpw):
        channels = max((min((t0 + tpw) * 32, N) - 1) // KK - (t0 * 32) // KK + 1 for t0 in range(0, NT, tpw))
        return ((channels * CF + 1 + 3) & ~3) + SLAB_ROWS * GLD
    TPW = min(NT, MAX_TPW)
    while True:                 # the full launch: the largest TPW that fits
        if TPW < 1:
            return "exceeds the 160 KiB of LDS"
        lds = floats(TPW)
        if lds <= LDS_FLOATS:
            break
        TPW -= 1
    wg = nchunk * NS            # workgroups before any column split: the slabs count
    if 0 < nchunk and wg < TARGET_WG:  # a small batch: fewer tiles per workgroup, never more LDS than the full launch
        want = min(NT, (TARGET_WG + wg - 1) // wg)
        for tpw in range((NT + want - 1) // want, TPW):
            if floats(tpw) <= max(lds, RED_FLOATS):
                TPW, lds = tpw, floats(tpw)
                break
    lds = max(lds, RED_FLOATS)
    PS = 1 if TPW >= 5 else 2 if TPW >= 3 else 4 if TPW == 2 else 8
    nsplit = (NT + TPW - 1) // TPW
    NQ = 1 if PS > 1 else {1: 1, 2: 2, 3: 4, 4: 4}[(TPW + 7) // 8]
    suffix = [s for s, on in (("column split", nsplit > 1), ("pixel split", PS > 1)) if on]
    name = "k_bwd_wgrad_slab<%d>" % NQ + (" (%s)" % ", ".join(suffix) if suffix else "")
    return dict(TPW=TPW, nsplit=nsplit, PS=PS, NQ=NQ, NS=NS, lds=4 * lds, name=name, NT=NT)


def served(c):
    return FZ.conv_shape(c) is not None and isinstance(plan(c), dict)


def launch_plan(c):
    """The layout of the call ops.conv_lif_backward(slab_path=True) makes for the case: min(B, 256) batch chunks."""
    return plan(c, min(c["B"], MAX_CHUNKS))


VARIANTS = ["k_bwd_wgrad_slab<1>", "k_bwd_wgrad_slab<1> (column split)", "k_bwd_wgrad_slab<1> (pixel split)",
            "k_bwd_wgrad_slab<1> (column split, pixel split)", "k_bwd_wgrad_slab<2>", "k_bwd_wgrad_slab<2> (column split)",
            "k_bwd_wgrad_slab<4>", "k_bwd_wgrad_slab<4> (column split)"]

default_serves = BW.default_serves


def _case(cid, stratum, k, **kw):
    c = FZ._case("bwdslab-%s" % cid, stratum, SEED * 100003 + k, **kw)
    assert served(c), (cid, plan(c))
    assert (c["c_out"] <= SLAB_ROWS) == (stratum == "forwarded"), cid
    return c


def _named(out):
    add = lambda name, **kw: out.append(_case(name, "named", len(out), **kw))
    R = dict(kh=7, kw=7, pad_h=3, pad_w=3, target=24, tau_tensor=1, h=16, w=16, B=1)
    for ns, co in (("3", 96), ("4", 128)):
        add("radio-ns%s-c1" % ns, note="radio_ml_conv.yaml at netscale %s: 1 -> %d on 16x16" % (ns, co), c_in=1, c_out=co, **R)
        add("radio-ns%s-c%d" % (ns, co), note="radio_ml_conv.yaml at netscale %s: %d -> %d on 16x16" % (ns, co, co), c_in=co, c_out=co,
            output_layer=int(co == 128), **R)


def _shape(out):
    add = lambda name, **kw: out.append(_case(name, "shape", 200 + len(out), **kw))
    for co in (65, 96, 97, 128, 129, 200):
        add("cout%d" % co, note="c_out %d: slabs %s" % (co, slabs(co)), c_in=3, c_out=co, h=9, w=8, B=3, refractory=co & 1)
    add("cin1-9cols", note="9 columns (< 32)", c_in=1, c_out=65, B=3)
    add("cin64", note="c_in 64", c_in=64, c_out=97, h=7, w=7, B=2, tau_tensor=1, refractory=0)
    add("cin70", note="c_in 70", c_in=70, c_out=65, h=6, w=7, B=2)
    add("k1x1", note="1x1 kernel", c_in=7, c_out=96, kh=1, kw=1, pad_h=0, pad_w=0, h=6, w=7, B=3)
    add("k2x5", note="2x5 kernel", c_in=3, c_out=129, kh=2, kw=5, pad_h=1, pad_w=2, h=6, w=8, B=3, refractory=0)
    add("k7x7", note="7x7 kernel", c_in=3, c_out=97, kh=7, kw=7, pad_h=3, pad_w=3, h=8, w=9, B=2)
    add("k9x9", note="81 taps (above the default path's 64)", c_in=2, c_out=65, kh=9, kw=9, pad_h=4, pad_w=4, h=10, w=10, B=2)
    add("cw-odd", note="cw 7, ch cw 35 (odd)", c_in=2, c_out=97, h=5, w=7, B=3)
    add("pix9", note="9 conv pixels", c_in=3, c_out=65, h=3, w=3, B=4, refractory=0)
    add("pix32", note="32 conv pixels", c_in=3, c_out=128, h=4, w=8, B=5)
    add("pix33", note="33 conv pixels", c_in=3, c_out=129, h=3, w=11, B=5)
    add("chcw1", note="ch cw = 1", c_in=2, c_out=200, h=3, w=3, pad_h=0, pad_w=0, B=5)
    for B in (1, 33):
        add("B%d" % B, note="B %d" % B, c_in=3, c_out=96, h=9, w=8, B=B)
    add("B257-4x4", note="257 samples on 256 chunks: chunk 0 sums two", c_in=2, c_out=65, h=4, w=4, B=257, target=3)
    k = 0
    for pool in ((1, 1), (2, 2), (3, 3), (1, 2)):
        for readout, outl in ((1, 0), (0, 0), (1, 1)):
            add("pool%dx%d-gp%d-go%d" % (pool + (readout, outl)), note="pooling / readout gradients", c_in=3,
                c_out=(65, 97, 130)[k % 3], h=9, w=11, pool_h=pool[0], pool_w=pool[1], readout=readout, output_layer=outl, B=4,
                refractory=k % 2)
            k += 1


def _edge(out):
    add = lambda name, **kw: out.append(_case(name, "edge", 300 + len(out), **kw))
    # the smallest working set at the LDS limit: 628 + 1 + 64 x 629 = 40885 (40888 laid out) floats of 40960, whatever c_out
    # (158x4: 632 + 1 + 64 x 633 = 41145, refused)
    add("lds-157x4", note="smallest working set 40885 of 40960 floats", c_in=1, c_out=65, kh=1, kw=1, pad_h=0, pad_w=0, h=157, w=4, B=2,
        target=4)
    # LDS lowers TPW below what the column-tile cap asks for: 64 channels of 22x22 do not fit beside 64 rows of g
    add("lds-split", note="LDS forces the column split (at most 31 of 64 padded channels fit)", c_in=64, c_out=65, h=20, w=20, B=2,
        target=4)
    # column tiles per workgroup where chunks x slabs reach 256 (no split for the batch's sake): pixel split 8 / 4 / 2 / 2 / 1,
    # column tiles per wave 1 / 2 / 4, the 32-tile cap.  4x8 kernel: 32 columns per input channel.  (c_out, B): 2 / 3 / 4 slabs
    T = dict(kh=4, kw=8, pad_h=1, pad_w=3, h=3, w=5, target=3, rate=.4)
    full = ((65, 128), (129, 86), (200, 64))
    for i, nt in enumerate((1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 32, 33)):
        co, B = full[i % 3]
        add("tiles%d-full" % nt, note="%d column tiles, %d chunks x %d slabs" % (nt, B, slab_count(co)), c_in=nt, c_out=co, B=B, **T)
    # one chunk less: chunks x slabs = 254 / 255 / 252 < 256 — the batch asks for two column splits
    add("tiles16-B127", note="2 slabs x 127 chunks: <1> column split without pixel split", c_in=16, c_out=65, B=127, **T)
    add("tiles24-B127", note="2 slabs x 127 chunks: <2> column split", c_in=24, c_out=128, B=127, **T)
    add("tiles16-B85", note="3 slabs x 85 chunks = 255: lowered (86 chunks are not)", c_in=16, c_out=129, B=85, **T)
    add("tiles16-B86", note="3 slabs x 86 chunks = 258: not lowered", c_in=16, c_out=129, B=86, **T)
    add("tiles16-B63", note="4 slabs x 63 chunks = 252: lowered (64 chunks are not)", c_in=16, c_out=200, B=63, **T)


def _forwarded(out):
    add = lambda name, **kw: out.append(_case(name, "forwarded", 400 + len(out), **kw))
    add("fwd-cout40", note="c_out 40: k_bwd_wgrad_wide", c_in=3, c_out=40, h=9, w=8, B=3)
    add("fwd-cout64", note="c_out 64: k_bwd_wgrad_wide, pool 2, output layer", c_in=5, c_out=64, h=9, w=11, pool_h=2, pool_w=2,
        output_layer=1, B=4)


FREE_B = (1, 2, 3, 4, 5)


def _free_draw(rng, k):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(65, 201)), kh=int(rng.randint(1, 17)), kw=int(rng.randint(1, 17)),
                 pad_h=int(rng.randint(0, 6)), pad_w=int(rng.randint(0, 6)), pool_h=int(rng.randint(1, 4)),
                 pool_w=int(rng.randint(1, 4)), h=int(rng.randint(1, 17)), w=int(rng.randint(1, 17)),
                 refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5), bias=int(rng.rand() < .75),
                 target=int(rng.randint(1, 41)), readout=int(rng.rand() >= .07), output_layer=int(rng.rand() < 1. / 3),
                 B=int(FREE_B[rng.randint(len(FREE_B))]), rate=float(np.round(rng.uniform(.05, .5), 3)),
                 state0=int(rng.rand() < .5))
        if not c["readout"]:
            c["output_layer"] = 0
        full = dict(FZ.CONV_DEFAULT, **c)
        if FZ.conv_shape(full) is None or not FZ.sees_input(full) or not served(full):
            continue
        ch, cw, _, _ = FZ.conv_shape(full)
        per_sample = c["c_out"] * ch * cw * c["c_in"] * c["kh"] * c["kw"]
        bmax = int(FZ.WORK_MAX // per_sample)
        if bmax < 1:
            continue
        if c["B"] > bmax:
            ok = [b for b in FREE_B if b <= bmax]
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
    r = lambda name, k, **kw: FZ._case("bwdslab-refuse-%s" % name, "refuse", SEED * 100003 + 2000 + k, **kw)
    S = dict(c_in=2, c_out=96, h=10, w=10, B=2)
    return [
        (r("kh17", 1, **dict(S, kh=17, kw=3, pad_h=8)), "UNSUPPORTED", "kernels up to 16x16"),
        (r("stride2", 2, **dict(S, stride=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("dilation2", 3, **dict(S, dilation=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("groups2", 4, **dict(S, groups=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("lds-158x4", 5, c_in=1, c_out=65, kh=1, kw=1, pad_h=0, pad_w=0, h=158, w=4, B=2, target=4), "UNSUPPORTED",
         "exceeds the 160 KiB of LDS"),
        (r("scratch", 6, **S), "INVALID", "scratch too small"),
    ]


def exact_draw(c):
    """Small integers for the case's geometry: g_v in {-2 .. 2}, eps1 in {0 .. 3}; with g_p = g_pv = NULL k_bwd_dv writes g_v
    itself, and every product and partial sum is an integer of magnitude <= 6 x B x pixels < 2^24: exact in float32 in ANY
    summation order -> g_v, eps1, v (any values: unused without g_p / g_pv) and the integer dW, db (bwd_wide_cases.exact_draw
    asserts the bound).  Each channel's g_v is its own draw, so a row taken from another slab, or from the right row of the wrong
    slab, differs."""
    return BW.exact_draw(c)


def by_id(cid):
    for c in cases() + [r[0] for r in refusals()]:
        if c["id"] == cid:
            return c
    raise KeyError(cid)
