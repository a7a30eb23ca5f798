"""Seeded random-geometry cases for the per-step C ABI (dcll_conv_lif_step / dcll_conv_lif_backward[_open] and their dense twins),
their tensors, and the float64 reference of the backward.  Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed
seeds only.  tests/test_fuzz_cases.py proves the generator and the references on the CPU; tests/test_gpu_fuzz.py runs the HIP
kernels against them.

A case is a small dict (geometry, options, batch, a sub-seed).  Its tensors are drawn from the sub-seed by conv_run / dense_run,
which also run the pinned-order C oracle over the three steps — so a failing case can be re-run alone from its id:
    python -c "import fuzz_cases as F; print(F.describe(F.by_id('conv-free-017')))"

The conv list is stratified (uniform draws never meet the specialised kernels):
  free    uniform draws over everything the descriptor takes;
  edge    the launcher's dispatch conditions (dcll_conv_lif_step, conv_lif_backward_impl), each with its nearest neighbour on
          the other side of the condition;
  refuse  geometries the backward returns DCLL_ERR_UNSUPPORTED for.
"""
import hashlib
import json

import numpy as np
import torch
import torch.nn.functional as F

STEPS = 3
ALPHARP = .65
SEED = 20260
B_SET = list(range(1, 71)) + [255, 256, 257]
# Work bound of a free draw: multiply-adds of one forward step, B * c_out * ch * cw * (c_in / groups) * kh * kw.  The C oracle
# runs 1 ... 3e9 of them per second on 8 cores (the 32 -> 32 7x7 layer at B = 257, 3.3e9 per step: 3 s for its three steps), a
# case costs STEPS steps + a provisional run on <= 4 samples: 168 free cases AT the bound would be ~5 s of oracle, the draws
# average a third of it (measured totals: profiles/r07_fuzz_times.txt).
WORK_MAX = 1.5e7
ELEMS_MAX = 2.0e6           # B * c_in * h * w and B * c_out * ch * cw (wide planes at large batches)
# the launcher's constants, restated once (csrc/dcll_hip.hip: conv_lif_backward_impl)
WG_MAXTAPS = 64
LDS_FLOATS = 48 * 1024 // 4 - 4 * (WG_MAXTAPS + 1)

CONV_DEFAULT = dict(c_in=1, c_out=1, groups=1, kh=3, kw=3, stride=1, dilation=1, pad_h=1, pad_w=1, pool_h=1, pool_w=1, h=8, w=8,
                    refractory=1, tau_tensor=0, bias=1, q8=0, target=10, readout=1, output_layer=0, B=2, rate=.3, state0=1,
                    misalign=0)


def conv_shape(c):
    """(ch, cw, ph, pw) of a case as the library's check_desc / conv_shape compute them, None where the descriptor is refused
    (empty conv or pool output; a pool window larger than the padded map, which torch's MaxPool2d refuses, is not drawn)."""
    eh, ew = c["dilation"] * (c["kh"] - 1) + 1, c["dilation"] * (c["kw"] - 1) + 1
    if c["h"] + 2 * c["pad_h"] < eh or c["w"] + 2 * c["pad_w"] < ew:
        return None
    ch = (c["h"] + 2 * c["pad_h"] - eh) // c["stride"] + 1
    cw = (c["w"] + 2 * c["pad_w"] - ew) // c["stride"] + 1
    pph, ppw = (c["pool_h"] - 1) // 2, (c["pool_w"] - 1) // 2
    if ch + 2 * pph < c["pool_h"] or cw + 2 * ppw < c["pool_w"]:
        return None
    ph = (ch + 2 * pph - c["pool_h"]) // c["pool_h"] + 1
    pw = (cw + 2 * ppw - c["pool_w"]) // c["pool_w"] + 1
    return ch, cw, ph, pw


def sees_input(c):
    """False where every tap of every output falls into the padding (e.g. w 1, pad_w 2, stride 3: outputs at columns -2 and 1):
    v is the bias everywhere and the weight gradient is zero whatever the tensors are — such a draw proves nothing."""
    ch, cw, _, _ = conv_shape(c)
    rows = any(0 <= y * c["stride"] + k * c["dilation"] - c["pad_h"] < c["h"] for y in range(ch) for k in range(c["kh"]))
    cols = any(0 <= x * c["stride"] + k * c["dilation"] - c["pad_w"] < c["w"] for x in range(cw) for k in range(c["kw"]))
    return rows and cols


def conv_work(c):
    ch, cw, _, _ = conv_shape(c)
    return c["B"] * c["c_out"] * ch * cw * (c["c_in"] // c["groups"]) * c["kh"] * c["kw"]


def wgrad_bands(c):
    """(RB, ch) of the generic weight-gradient kernel: RB output rows per LDS band (0: refused), the launcher's formula."""
    ch = conv_shape(c)[0]
    WP = c["w"] + 2 * c["pad_w"]
    rows_fit = LDS_FLOATS // WP
    span = (c["kh"] - 1) * c["dilation"] + 1
    RB = 0 if rows_fit < span else (rows_fit - span) // c["stride"] + 1
    return min(RB, ch), ch


def _case(cid, stratum, seed, **kw):
    c = dict(CONV_DEFAULT)
    unknown = set(kw) - set(c) - {"note"}
    assert not unknown, unknown
    c.update(kw)
    c.update(id=cid, stratum=stratum, seed=int(seed))
    c.setdefault("note", "")
    return c


def _free_draw(rng, k, seed):
    while True:
        gk = ("1", "1", "2", "3", "4", "dw")[rng.randint(6)]
        c_in, c_out = int(rng.randint(1, 71)), int(rng.randint(1, 71))
        if gk == "dw":
            c_in = min(c_in, 35)
            groups, c_out = c_in, c_in * int(rng.randint(1, 3))
        else:
            groups = int(gk)
            c_in, c_out = max(groups, c_in - c_in % groups), max(groups, c_out - c_out % groups)
        h, w = int(rng.randint(1, 41)), int(rng.randint(1, 41))
        if rng.rand() < 0.06:
            w = int(rng.randint(100, 400))                   # a few wide planes
        c = dict(c_in=c_in, c_out=c_out, groups=groups, kh=int(rng.randint(1, 9)), kw=int(rng.randint(1, 9)),
                 stride=int(rng.randint(1, 4)), dilation=int(rng.randint(1, 3)), pad_h=int(rng.randint(0, 5)),
                 pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)), h=h, w=w,
                 refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5), bias=int(rng.rand() < .75),
                 q8=int(rng.rand() < .25), target=int(rng.randint(1, 41)), readout=int(rng.rand() >= .07),
                 output_layer=int(rng.rand() < 1. / 3), B=int(B_SET[rng.randint(len(B_SET))]),
                 rate=float(np.round(rng.uniform(.05, .5), 3)), state0=int(rng.rand() < .5), misalign=0)
        if not c["readout"]:
            c["output_layer"] = 0
        shp = conv_shape(c)
        if shp is None or not sees_input(c):
            continue                                        # (refused descriptor / outputs that see padding only: redrawn)
        ch, cw, _, _ = shp
        per_sample = c["c_out"] * ch * cw * (c_in // groups) * c["kh"] * c["kw"]
        bmax = int(min(WORK_MAX // per_sample, ELEMS_MAX // (c_in * h * w), ELEMS_MAX // (c["c_out"] * ch * cw)))
        if bmax < 1:
            continue
        if c["B"] > bmax:
            ok = [b for b in B_SET if b <= bmax]
            c["B"] = int(ok[rng.randint(len(ok))])
        return _case("conv-free-%03d" % k, "free", seed * 100003 + k, **c)


def _edge_cases(seed):
    """The launcher's conditions, each side.  `note` says which condition and which side."""
    out = []

    def add(name, note, **kw):
        out.append(_case("conv-edge-%s" % name, "edge", seed * 100003 + 1000 + len(out), note=note, **kw))
    L32 = dict(c_in=32, c_out=32, kh=7, kw=7, pad_h=3, pad_w=3, h=16, w=16, target=24, tau_tensor=1)
    # k7 (7x7, pad 3, pool 1, bias, plain conv) on the 16x16 plane against its neighbours
    add("k7-plane16", "k7 && plane16 && split16: k_trace4 + k_lif_step_c32t (8-row tiles); k_bwd_wgrad_c32", B=5, output_layer=1, **L32)
    add("k7-pad2", "k7 false (pad 2): generic path, tiled<7,7>", B=5, **dict(L32, pad_h=2, pad_w=2))
    add("k7-padw2", "k7 false (pad_w 2 only)", B=3, **dict(L32, pad_w=2))
    add("k7-nobias", "k7 false (NULL bias)", B=5, bias=0, **L32)
    add("k7-stride2", "k7 false (stride 2): k_conv_lif", B=5, stride=2, **L32)
    add("k7-pool2", "k7 false (pool 2)", B=3, pool_h=2, pool_w=2, **L32)
    add("k7-q8", "k7 with int8 weights", B=4, q8=1, **L32)
    add("k7-plain", "k7, not refractory, scalar time constants", B=6, refractory=0, **dict(L32, tau_tensor=0))
    # plane16 against 16x17 / 17x16
    add("plane-16x17", "plane16 false (16x17)", B=3, **dict(L32, w=17))
    add("plane-17x16", "plane16 false (17x16)", B=3, **dict(L32, h=17))
    # h % 16, w % 16
    add("plane-32x48", "h % 16 == 0 && w % 16 == 0: k_lif_step_c32t (16-row tiles); k_bwd_wgrad_c32 (tiled)", B=2, **dict(L32, h=32, w=48))
    add("plane-32x40", "w % 16 != 0: generic path", B=2, **dict(L32, h=32, w=40))
    add("plane-32x48-q8", "16-row tiles with int8 weights, not refractory", B=1, q8=1, refractory=0, **dict(L32, h=32, w=48))
    # split16 at DCLL_SPLIT16_MAX_BATCH's default and + 1 (these two are the oracle's most expensive cases)
    add("split16-256", "B == 256: split16, two workgroups per sample", B=256, **L32)
    add("split16-257", "B == 257: k_lif_step_c32", B=257, **L32)
    # ptr16 false: the same layers from buffers one float off 16-byte alignment
    add("ptr16-plane16", "ptr16 false on the k7 16x16 layer: no k_trace4 / tiled MFMA step, falls through to k_lif_step_c32, same bits", B=5, misalign=1, **L32)
    add("ptr16-32x48", "ptr16 false on 32x48: falls through to the generic path, same bits", B=2, misalign=1, **dict(L32, h=32, w=48))
    add("ptr16-c1t", "ptr16 false on the tiled first layer", B=3, misalign=1, **dict(L32, c_in=1, h=32, w=16))
    # c1 / c1t
    C1 = dict(L32, c_in=1)
    add("c1-plane16", "c_in 1, c_out 32, 16x16: k_lif_step_c1; k_bwd_wgrad_c1", B=7, **C1)
    add("c1-plane16-co20", "c_in 1, c_out 20 (<= 32): k_lif_step_c1; generic weight gradient", B=4, **dict(C1, c_out=20))
    add("c1-plane16-co33", "c_in 1, c_out 33: generic", B=4, **dict(C1, c_out=33))
    add("c1t-co32", "c1t at c_out 32 (32x16): k_lif_step_c1 (tiled); k_bwd_wgrad_c1 (tiled)", B=3, **dict(C1, h=32, w=16))
    add("c1t-co33", "c1t false at c_out 33", B=3, **dict(C1, c_out=33, h=32, w=16))
    add("c1t-plain", "c1t, not refractory, scalar time constants, int8", B=2, refractory=0, q8=1, **dict(C1, h=16, w=32, tau_tensor=0))
    # tile_ok at ch, cw = 7 against 8 for each tiled kernel size; ragged tiles (17, 31)
    for (kh, kw, ph_, pw_) in ((7, 7, 3, 3), (5, 5, 2, 2), (3, 3, 1, 1), (1, 3, 0, 1)):
        g = dict(c_in=5, c_out=11, kh=kh, kw=kw, pad_h=ph_, pad_w=pw_, target=12, B=3)
        tag = "%dx%d" % (kh, kw)
        add("tile-%s-8x8" % tag, "tile_ok (ch, cw = 8, 8): k_conv_lif_tiled<%d,%d>" % (kh, kw), **dict(g, h=8, w=8))
        add("tile-%s-7x8" % tag, "tile_ok false (ch 7): k_conv_lif", **dict(g, h=7, w=8))
        add("tile-%s-8x7" % tag, "tile_ok false (cw 7): k_conv_lif", **dict(g, h=8, w=7))
        add("tile-%s-17x31" % tag, "ragged tiles (ch, cw = 17, 31)", pool_h=2, pool_w=3, q8=int(kh == 3), **dict(g, h=17, w=31))
    add("tile-3x3-groups2", "tile_ok false (groups 2) at 3x3", c_in=4, c_out=6, groups=2, h=12, w=12, B=3)
    # the weight gradient's RB < ch multi-band path (stride 2, dilation 2: all three terms of the band formula) against the
    # same layer on a plane that fits one band
    MB = dict(c_in=2, c_out=3, kh=3, kw=3, stride=2, dilation=2, pad_h=1, pad_w=2, w=300, B=2, target=9, tau_tensor=1)
    add("bands-60x300", "k_bwd_wgrad: RB < ch (two bands)", **dict(MB, h=60))
    add("bands-20x300", "k_bwd_wgrad: one band", **dict(MB, h=20))
    add("bands-97x250-k5", "k_bwd_wgrad: RB < ch, 5x4 taps, stride 3, groups 2, last band ragged", c_in=2, c_out=4, groups=2, kh=5,
        kw=4, stride=3, dilation=2, pad_h=0, pad_w=3, h=97, w=250, B=3, target=5)
    # nchunk classes of the closed reduction (generic kernel: nchunk = min(B, 64))
    NC = dict(c_in=3, c_out=4, kh=3, kw=2, pad_h=1, pad_w=0, h=9, w=10, target=7)
    for B in (15, 16, 63, 64):
        add("nchunk-B%d" % B, "closed reduction at %d partial rows" % B, B=B, **NC)
    # the three output_ gradient forms
    OG = dict(c_in=3, kh=3, kw=3, h=8, w=8, output_layer=1, B=9)
    add("outgrad-K256", "output_: K % 32 == 0, target <= 32: k_bwd_outgrad_mfma", c_out=4, target=24, **OG)
    add("outgrad-K320-t32", "output_: K % 32 == 0, target == 32", c_out=5, target=32, **OG)
    add("outgrad-K216", "output_: K % 32 != 0, target <= 32: k_bwd_outgrad_part", c_out=3, target=24, **dict(OG, h=8, w=9))
    add("outgrad-t33", "output_: target 33 (> 32): k_bwd_outgrad; generic k_bwd_dv", c_out=4, target=33, **OG)
    add("outgrad-t40-pool", "output_: target 40 with pooling", c_out=4, target=40, pool_h=2, pool_w=2, **OG)
    # the nopool<NP> classes of k_bwd_dv at their edges, and the generic kernel just beyond
    for t in (8, 9, 16, 17, 24, 25, 32, 33):
        add("dv-target%d" % t, "k_bwd_dv readout-width class at target %d" % t, c_in=2, c_out=6, h=9, w=7, target=t, B=17)
    # exact v ties: padded regions where every output equals the bias, pooled (the first position wins on both sides)
    add("ties-pad4-pool3", "pool windows of equal v (padding 4 around a 2x2 plane)", c_in=2, c_out=3, kh=1, kw=1, pad_h=4, pad_w=4,
        h=2, w=2, pool_h=3, pool_w=3, B=4, refractory=0)
    add("ties-pad4-pool2", "pool windows of equal v, 2x3 pooling, refractory", c_in=1, c_out=4, kh=2, kw=2, pad_h=4, pad_w=4, h=3, w=2,
        pool_h=2, pool_w=3, B=3)
    # readout forms a step call reaches beyond 2048 rows
    add("readout-t16-B2049", "rows > 2048, K % 32 == 0: k_readout_t16", c_in=1, c_out=2, kh=1, kw=1, pad_h=0, pad_w=0, h=4, w=4, B=2049,
        target=11, output_layer=1)
    add("readout-plain-B2049", "rows > 2048, K % 32 != 0: k_readout", c_in=1, c_out=3, kh=1, kw=1, pad_h=0, pad_w=0, h=3, w=3, B=2049,
        target=11)
    return out


def _refuse_cases(seed):
    return [
        _case("conv-refuse-72taps", "refuse", seed * 100003 + 2000, note="kh * kw = 72 > 64", c_in=2, c_out=3, kh=9, kw=8, pad_h=4,
              pad_w=4, h=10, w=10, B=2),
        _case("conv-refuse-65taps", "refuse", seed * 100003 + 2001, note="kh * kw = 65 > 64", c_in=1, c_out=2, kh=5, kw=13, pad_h=2,
              pad_w=6, h=6, w=14, B=1, pool_h=2, pool_w=2),
        _case("conv-refuse-wide-row", "refuse", seed * 100003 + 2002, note="15 input rows of 904 floats exceed the LDS band", c_in=1,
              c_out=2, kh=8, kw=3, dilation=2, pad_h=2, pad_w=2, h=16, w=900, B=1),
    ]


def conv_cases(seed=SEED):
    """[edge..., free...]: the cases that run (refusals: conv_refusals)."""
    rng = np.random.RandomState(seed)
    return _edge_cases(seed) + [_free_draw(rng, k, seed) for k in range(168)]


def conv_refusals(seed=SEED):
    return _refuse_cases(seed)


DENSE_B_SET = B_SET + [127, 128, 129]


def dense_cases(seed=SEED):
    rng = np.random.RandomState(seed + 1)
    out = []

    def add(name, **kw):
        c = dict(in_features=8, out_features=8, target=10, B=4, refractory=1, tau_tensor=0, bias=1, rate=.3, state0=1, note="")
        c.update(kw)
        c.update(id="dense-%s" % name, stratum="dense", seed=(seed + 1) * 100003 + len(out))
        out.append(c)
    for k in range(40):
        nin = int(rng.randint(1, 1101)) if rng.rand() < .6 else int((31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1)[rng.randint(10)])
        nout = int(rng.randint(1, 201)) if rng.rand() < .6 else int((31, 32, 33, 63, 64, 65, 127, 128, 129, 1)[rng.randint(10)])
        B = int(DENSE_B_SET[rng.randint(len(DENSE_B_SET))])
        add("free-%02d" % k, in_features=nin, out_features=nout, target=int(rng.randint(1, 41)), B=B,
            refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5), bias=int(rng.rand() < .75),
            rate=float(np.round(rng.uniform(.05, .5), 3)), state0=int(rng.rand() < .5))
    for B in (127, 128, 129):
        add("wg128-B%d" % B, in_features=40, out_features=70, target=24, B=B, tau_tensor=1, note="the 128-sample workgroup")
    add("wide", in_features=5, out_features=256, target=12, B=16384, refractory=1, bias=1,
        note="ceil(out / 64) * ceil(B / 128) = 512: the wide form of k_dense_lif_mfma")
    add("narrow-neighbour", in_features=5, out_features=256, target=12, B=16256, refractory=1, bias=1,
        note="ceil(out / 64) * ceil(B / 128) = 508: narrow")
    return out


def by_id(cid):
    for c in conv_cases() + conv_refusals() + dense_cases():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def describe(c):
    return json.dumps(c, sort_keys=True)


def cases_hash(cases):
    return hashlib.sha256("\n".join(describe(c) for c in cases).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def _time_constants(rng, shape):
    alpha = rng.uniform(.8, .97, size=shape).astype(np.float32)
    alphas = rng.uniform(.8, .9, size=shape).astype(np.float32)
    tau_m = (np.float32(1) / (np.float32(1) - alpha)).astype(np.float32)
    tau_s = (np.float32(1) / (np.float32(1) - alphas)).astype(np.float32)
    return alpha, tau_m, alphas, tau_s


def quantize_int8(W):
    """snn_modulation_classification_amd.quant's definition (per-output-channel symmetric int8) -> (q, scale, dequantised W): the
    dequantised value is ONE rounded fp32 multiply (float)q * scale[co], what the kernels compute."""
    from snn_modulation_classification_amd import quant
    q, scale = quant.quantize_int8_per_channel(torch.from_numpy(W))
    Wd = quant.dequantize(q, scale).contiguous()
    return q.numpy(), scale.numpy(), Wd.numpy()


def active_share(v):
    return float((np.abs(v) < 4).mean())


def _conv_draw(c, attempt):
    """All tensors of a conv case from (sub-seed, attempt); the weights rescaled from a provisional oracle run (first <= 4
    samples, plain neuron, no bias: v is then linear in W) so that std(v) at the last step is 2 — with unit-scale weights |v|
    reaches several hundred, sigmoid'(v) is exactly 0 in fp32 and the backward would be multiplied by zero."""
    from oracle import c_oracle as C
    rng = np.random.RandomState((c["seed"] + 7919 * attempt) % (2 ** 31))
    ch, cw, ph, pw = conv_shape(c)
    B, cin, cout, cig = c["B"], c["c_in"], c["c_out"], c["c_in"] // c["groups"]
    hw = (c["h"], c["w"])
    K = cout * ph * pw
    T = {}
    W0 = rng.randn(cout, cig, c["kh"], c["kw"]).astype(np.float32)
    T["tau"] = _time_constants(rng, (cin,) + hw if c["tau_tensor"] else (1,))
    T["x"] = [(rng.uniform(size=(B, cin) + hw) < c["rate"]).astype(np.float32) for _ in range(STEPS)]
    if c["state0"]:
        T["eps0"] = rng.uniform(0, 3, size=(B, cin) + hw).astype(np.float32)
        T["eps1"] = rng.uniform(0, 12, size=(B, cin) + hw).astype(np.float32)
        T["arp"] = (-rng.uniform(0, 2, size=(B, cout, ch, cw))).astype(np.float32)
    else:
        T["eps0"], T["eps1"] = np.zeros((B, cin) + hw, np.float32), np.zeros((B, cin) + hw, np.float32)
        T["arp"] = np.zeros((B, cout, ch, cw), np.float32)
    T["i2o_W"] = (rng.uniform(-1, 1, size=(c["target"], K)) * (.5 / np.sqrt(K))).astype(np.float32)
    T["i2o_b"] = rng.uniform(-.1, .1, size=(c["target"],)).astype(np.float32)
    T["out_W"] = (rng.uniform(-1, 1, size=(c["target"], K)) * (.5 / np.sqrt(K))).astype(np.float32)
    T["out_b"] = rng.uniform(-.1, .1, size=(c["target"],)).astype(np.float32)
    T["g_p"] = rng.randn(B, c["target"]).astype(np.float32) if c["readout"] else None
    T["g_o"] = rng.randn(B, c["target"]).astype(np.float32) if c["output_layer"] else None
    T["g_pv"] = (rng.randn(B, cout, ph, pw) * .3).astype(np.float32)
    T["g_v"] = (rng.randn(B, cout, ch, cw) * .1).astype(np.float32)
    # provisional run
    Bp = min(B, 4)
    sd = {"i2h.weight": W0, "i2h.alpha": T["tau"][0], "i2h.tau_m__dt": T["tau"][1], "i2h.alphas": T["tau"][2],
          "i2h.tau_s__dt": T["tau"][3], "i2o.weight": T["i2o_W"], "i2o.bias": T["i2o_b"]}
    pad, pool = (c["pad_h"], c["pad_w"]), (c["pool_h"], c["pool_w"])
    prov = C.OracleConvLayer(sd, hw, pad, pool, 0.0, ALPHARP, False, c["stride"], c["dilation"], c["groups"])
    prov.init_state(Bp)
    prov.state[0][...], prov.state[1][...] = T["eps0"][:Bp], T["eps1"][:Bp]
    for t in range(STEPS):
        v = prov.forward(T["x"][t][:Bp])[3]
    std = float(v.std())
    if std == 0.0:      # (a map of equal values, e.g. one output element: scale by its size instead)
        std = float(np.abs(v).max())
    W = (W0 * np.float32(2.0 / std if std > 0 else 1.0)).astype(np.float32)
    T["b"] = (rng.randn(cout) * .5).astype(np.float32) if c["bias"] else None
    T["q8"] = None
    if c["q8"]:
        q, scale, W = quantize_int8(W)
        T["q8"] = (q, scale)
    T["W"] = np.ascontiguousarray(W)
    return T


def _conv_oracle(c, T, before_step=None):
    """the oracle over the steps of T['x'] (STEPS of them here; tests/value_cases.py runs up to 8, sets c['alpharp'] and hooks a
    mutant in front of every step)"""
    from oracle import c_oracle as C
    sd = {"i2h.weight": T["W"], "i2h.alpha": T["tau"][0], "i2h.tau_m__dt": T["tau"][1], "i2h.alphas": T["tau"][2],
          "i2h.tau_s__dt": T["tau"][3], "i2o.weight": T["i2o_W"], "i2o.bias": T["i2o_b"]}
    if T["b"] is not None:
        sd["i2h.bias"] = T["b"]
    if c["output_layer"]:
        sd["output_.weight"], sd["output_.bias"] = T["out_W"], T["out_b"]
    orc = C.OracleConvLayer(sd, (c["h"], c["w"]), (c["pad_h"], c["pad_w"]), (c["pool_h"], c["pool_w"]),
                            1.0 if c["refractory"] else 0.0, c.get("alpharp", ALPHARP), bool(c["output_layer"]), c["stride"],
                            c["dilation"], c["groups"])
    assert (orc.ch, orc.cw, orc.ph, orc.pw) == conv_shape(c), (c["id"], "the oracle's output shape differs from the generator's")
    orc.init_state(c["B"])
    orc.state[0][...], orc.state[1][...], orc.state[2][...] = T["eps0"], T["eps1"], T["arp"]
    steps = []
    for t in range(len(T["x"])):
        if before_step is not None:
            before_step(orc.state)
        o, p, pv, v, s = orc.forward(T["x"][t])
        steps.append(dict(v=v, s=s, pv=pv, p=p, o=(o if c["output_layer"] else None), eps0=orc.state[0].copy(),
                          eps1=orc.state[1].copy(), arp=orc.state[2].copy()))
    return steps


def vacuous(c, steps):
    """Why a trajectory would prove nothing (None = it is fine): the un-pooled spikes v > 0 of the three steps hold one value
    only, a refractory layer's arp stayed 0, or fewer than 80 % of the last step's |v| are below 4 (sigmoid' ~ 0 beyond)."""
    spk = np.concatenate([(s["v"] > 0).ravel() for s in steps])
    if spk.all() or not spk.any():
        return "spikes hold one value"
    if c["refractory"] and not np.any(steps[-1]["arp"]):
        return "arp is zero"
    if active_share(steps[-1]["v"]) < .8:
        return "active share %.2f" % active_share(steps[-1]["v"])
    return None


def conv_run(c, max_attempts=24):
    """(tensors, oracle steps) of a conv case: the first attempt whose trajectory is not vacuous (deterministic in the sub-seed;
    almost always the first)."""
    why = None
    for attempt in range(max_attempts):
        T = _conv_draw(c, attempt)
        steps = _conv_oracle(c, T)
        why = vacuous(c, steps)
        if why is None:
            T["attempt"] = attempt
            return T, steps
    raise AssertionError("%s: no non-vacuous draw in %d attempts (%s)" % (c["id"], max_attempts, why))


def _dense_draw(c, attempt):
    from oracle import c_oracle as C
    rng = np.random.RandomState((c["seed"] + 7919 * attempt) % (2 ** 31))
    B, nin, nout = c["B"], c["in_features"], c["out_features"]
    T = {}
    W0 = rng.randn(nout, nin).astype(np.float32)
    T["tau"] = _time_constants(rng, (nin,) if c["tau_tensor"] else (1,))
    T["x"] = [(rng.uniform(size=(B, nin)) < c["rate"]).astype(np.float32) for _ in range(STEPS)]
    if c["state0"]:
        T["eps0"] = rng.uniform(0, 3, size=(B, nin)).astype(np.float32)
        T["eps1"] = rng.uniform(0, 12, size=(B, nin)).astype(np.float32)
        T["arp"] = (-rng.uniform(0, 2, size=(B, nout))).astype(np.float32)
    else:
        T["eps0"], T["eps1"], T["arp"] = (np.zeros((B, nin), np.float32), np.zeros((B, nin), np.float32),
                                          np.zeros((B, nout), np.float32))
    T["i2o_W"] = (rng.uniform(-1, 1, size=(c["target"], nout)) * (.5 / np.sqrt(nout))).astype(np.float32)
    T["i2o_b"] = rng.uniform(-.1, .1, size=(c["target"],)).astype(np.float32)
    T["g_p"] = rng.randn(B, c["target"]).astype(np.float32)
    T["g_pv"] = (rng.randn(B, nout) * .3).astype(np.float32)
    T["g_v"] = (rng.randn(B, nout) * .1).astype(np.float32)
    Bp = min(B, 4)
    sd = {"i2h.weight": W0, "i2h.alpha": T["tau"][0], "i2h.tau_m__dt": T["tau"][1], "i2h.alphas": T["tau"][2],
          "i2h.tau_s__dt": T["tau"][3], "i2o.weight": T["i2o_W"], "i2o.bias": T["i2o_b"]}
    prov = C.OracleDenseLayer(sd, 0.0, ALPHARP)
    prov.state = [T["eps0"][:Bp].copy(), T["eps1"][:Bp].copy(), np.zeros((Bp, nout), np.float32)]
    for t in range(STEPS):
        v = prov.forward(T["x"][t][:Bp])[3]
    std = float(v.std())
    if std == 0.0:
        std = float(np.abs(v).max())
    T["W"] = (W0 * np.float32(2.0 / std if std > 0 else 1.0)).astype(np.float32)
    T["b"] = (rng.randn(nout) * .5).astype(np.float32) if c["bias"] else None
    return T


def _dense_oracle(c, T, before_step=None):
    from oracle import c_oracle as C
    sd = {"i2h.weight": T["W"], "i2h.alpha": T["tau"][0], "i2h.tau_m__dt": T["tau"][1], "i2h.alphas": T["tau"][2],
          "i2h.tau_s__dt": T["tau"][3], "i2o.weight": T["i2o_W"], "i2o.bias": T["i2o_b"]}
    if T["b"] is not None:
        sd["i2h.bias"] = T["b"]
    orc = C.OracleDenseLayer(sd, 1.0 if c["refractory"] else 0.0, c.get("alpharp", ALPHARP))
    orc.state = [T["eps0"].copy(), T["eps1"].copy(), T["arp"].copy()]
    steps = []
    for t in range(len(T["x"])):
        if before_step is not None:
            before_step(orc.state)
        s, p, pv, v = orc.forward(T["x"][t])
        steps.append(dict(v=v, s=s, pv=pv, p=p, eps0=orc.state[0].copy(), eps1=orc.state[1].copy(), arp=orc.state[2].copy()))
    return steps


def dense_run(c, max_attempts=24):
    why = None
    for attempt in range(max_attempts):
        T = _dense_draw(c, attempt)
        steps = _dense_oracle(c, T)
        why = vacuous(c, steps)
        if why is None:
            T["attempt"] = attempt
            return T, steps
    raise AssertionError("%s: no non-vacuous draw in %d attempts (%s)" % (c["id"], max_attempts, why))


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references (include/dcll_hip.h: dcll_conv_lif_backward, dcll_dense_lif_backward)
# ---------------------------------------------------------------------------------------------------------------------------
def _f64(a):
    return None if a is None else torch.from_numpy(np.asarray(a)).double()


def identity_route(c):
    """The routing of a layer without pooling: every position is its own window."""
    ch, cw, ph, pw = conv_shape(c)
    assert (ch, cw) == (ph, pw)
    return torch.arange(ch * cw).reshape(1, 1, ch, cw).expand(c["B"], c["c_out"], ch, cw)


def first_max_route(c, pv_full):
    """The routing index map of a pooling layer from an un-pooled pv map (any float dtype): per pooled window the flat index
    (y * cw + x) of its first maximum in row-major order (MaxPool2d's forward: strict >)."""
    if c["pool_h"] == 1 and c["pool_w"] == 1:
        return identity_route(c)
    pool = (c["pool_h"], c["pool_w"])
    _, idx = F.max_pool2d(pv_full, pool, pool, ((pool[0] - 1) // 2, (pool[1] - 1) // 2), return_indices=True)
    return idx


def conv_backward_ref(c, T, v, eps1, route, zero_g_v=False, dtype=torch.float64):
    """dv = route(g_pv + g_p . i2o_W) * pv (1 - pv) + g_v ;  dW = sum dv (x) unfold(eps1) ;  db = sum dv ;
    d_outW = g_o^T . pv_pooled ; d_outb = sum g_o   — in `dtype` (float64: the reference; float32: the same sums in plain fp32, the
    yardstick of an fp32 implementation's error), from the ORACLE's v and eps1 and the routing index map `route` (B, c_out, ph, pw)
    of flat positions y * cw + x.  -> dict(dW, db, d_outW, d_outb, dv)"""
    ch, cw, ph, pw = conv_shape(c)
    B, cin, cout, G = c["B"], c["c_in"], c["c_out"], c["groups"]
    cig, cog, kk = cin // G, cout // G, c["kh"] * c["kw"]
    cv = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
    v = cv(v)
    pv = 1.0 / (1.0 + torch.exp(-v))
    g = cv(T["g_pv"]).clone()
    if T["g_p"] is not None:
        g = g + (cv(T["g_p"]) @ cv(T["i2o_W"])).reshape(B, cout, ph, pw)
    route = route.reshape(B, cout, ph * pw)
    routed = torch.zeros(B, cout, ch * cw, dtype=dtype)
    routed.scatter_(2, route, g.reshape(B, cout, ph * pw))          # (kernel = stride: a position belongs to one window at most)
    dv = routed.reshape(B, cout, ch, cw) * pv * (1.0 - pv)
    if not zero_g_v:
        dv = dv + cv(T["g_v"])
    dW = torch.zeros(G, cog, cig * kk, dtype=dtype)
    e = cv(eps1)
    step = max(1, int(4e6 // max(1, cin * kk * ch * cw)))
    for b0 in range(0, B, step):
        cols = F.unfold(e[b0:b0 + step], (c["kh"], c["kw"]), c["dilation"], (c["pad_h"], c["pad_w"]), c["stride"])
        n = cols.shape[0]
        cols = cols.reshape(n, G, cig * kk, ch * cw)
        dW += torch.einsum("bgol,bgkl->gok", dv[b0:b0 + step].reshape(n, G, cog, ch * cw), cols)
    out = dict(dW=dW.reshape(cout, cig, c["kh"], c["kw"]), db=dv.sum(dim=(0, 2, 3)), dv=dv, d_outW=None, d_outb=None)
    if T["g_o"] is not None:
        pvp = torch.gather(pv.reshape(B, cout, ch * cw), 2, route).reshape(B, cout * ph * pw)
        out["d_outW"] = cv(T["g_o"]).t() @ pvp
        out["d_outb"] = cv(T["g_o"]).sum(0)
    return out


def conv_backward_autograd(c, T, v, eps1):
    """The same gradients from torch autograd in float64 through F.conv2d / F.max_pool2d / F.linear, evaluated AT the oracle's v
    (v enters as conv2d(eps1, W) + a constant, so that both sides differentiate at the same point) -> (grads dict, route)."""
    B, cout = c["B"], c["c_out"]
    _, _, ph, pw = conv_shape(c)
    W = _f64(T["W"]).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    vc = F.conv2d(_f64(eps1), W, b, c["stride"], (c["pad_h"], c["pad_w"]), c["dilation"], c["groups"])
    vv = vc + (_f64(v) - vc).detach()
    pv = torch.sigmoid(vv)
    pool = (c["pool_h"], c["pool_w"])
    pvp, route = F.max_pool2d(pv, pool, pool, ((pool[0] - 1) // 2, (pool[1] - 1) // 2), return_indices=True)
    loss = (pvp * _f64(T["g_pv"])).sum() + (vv * _f64(T["g_v"])).sum()
    if T["g_p"] is not None:
        loss = loss + (F.linear(pvp.reshape(B, -1), _f64(T["i2o_W"]), _f64(T["i2o_b"])) * _f64(T["g_p"])).sum()
    oW = ob = None
    if T["g_o"] is not None:
        oW, ob = _f64(T["out_W"]).requires_grad_(True), _f64(T["out_b"]).requires_grad_(True)
        loss = loss + (F.linear(pvp.detach().reshape(B, -1), oW, ob) * _f64(T["g_o"])).sum()       # (:606: flatten.detach())
    loss.backward()
    return dict(dW=W.grad, db=b.grad, d_outW=None if oW is None else oW.grad, d_outb=None if ob is None else ob.grad), route


def dense_backward_ref(c, T, v, eps1, zero_g_v=False, dtype=torch.float64):
    cv = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    pv = 1.0 / (1.0 + torch.exp(-cv(v)))
    dv = (cv(T["g_p"]) @ cv(T["i2o_W"]) + cv(T["g_pv"])) * pv * (1.0 - pv)
    if not zero_g_v:
        dv = dv + cv(T["g_v"])
    return dict(dW=dv.t() @ cv(eps1), db=dv.sum(0), dv=dv)


def dense_backward_autograd(c, T, v, eps1):
    W = _f64(T["W"]).requires_grad_(True)
    b = torch.zeros(c["out_features"], dtype=torch.float64, requires_grad=True)
    vc = F.linear(_f64(eps1), W, b)
    vv = vc + (_f64(v) - vc).detach()
    pv = torch.sigmoid(vv)
    loss = ((F.linear(pv, _f64(T["i2o_W"]), _f64(T["i2o_b"])) * _f64(T["g_p"])).sum() + (pv * _f64(T["g_pv"])).sum() +
            (vv * _f64(T["g_v"])).sum())
    loss.backward()
    return dict(dW=W.grad, db=b.grad)
