"""Seeded cases for dcll_conv_lif_step_any (ABI 10: k_lif_step_any, the MFMA per-step forward of any plain conv layer), built on
tests/fuzz_cases.py: a case is one of its conv cases (same keys, FZ.conv_run gives the tensors and the C oracle's trajectory of
three steps from carried state, with its non-vacuity check) plus three keys of this list:
    want_v   0: the call passes out_v = NULL
    B_run    batch on the device; the oracle runs on the first B distinct samples, the device on copies of them (grid)
    also_B   a second batch size (the first also_B samples): the other side of an NS threshold; per-sample results must be equal
Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_step_any_cases.py proves the list
on the CPU; tests/test_gpu_step_any.py runs the HIP kernel against it.  Re-run one alone:
    python -c "import step_any_cases as S; print(S.describe(S.by_id('step-mnist-l1')))"

The launcher is restated ONCE here (csrc/dcll_step_any.hip: dcll_step_any_check, step_any_lds_floats, dcll_step_any_split;
csrc/dcll_hip.hip: dcll_conv_lif_step_any): served(), lds_bytes(), ns(), launch_log().

Strata:
  named       the three layers of mnist_conv.yaml; radio_ml_conv.yaml's 1 -> 32 and 32 -> 32 on 16x16, 24x24, 12x32; B = 2
  forms       one small case per template instance and form
  boundaries  c_out, odd c_in, the zero link, kernel sizes, growing / shrinking planes, ragged tiles, pooling windows, bias = 0,
              time constants, out_v = NULL, mis-aligned operands, the LDS limit, both sides of the NS thresholds
  grid        one small layer at B = 1100
  free        uniform draws: c_in 1-40, c_out 1-32, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, planes up to 22x22, B 1-5
  refuse      error returns before any launch (refusals())"""
import numpy as np

import fuzz_cases as FZ

SEED = 20263
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
NW = 8              # waves of a workgroup
CUS = 256
MAX_K, MAX_COUT = 16, 32
EXTRA = dict(want_v=1, B_run=None, also_B=None)


def _case(cid, stratum, seed, **kw):
    extra = {k: kw.pop(k, v) for k, v in EXTRA.items()}
    kw.setdefault("readout", 0)
    kw.setdefault("c_out", 8)
    c = FZ._case(cid, stratum, seed, **kw)
    c.update(extra)
    if c["B_run"] is None:
        c["B_run"] = c["B"]
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher, restated
# ---------------------------------------------------------------------------------------------------------------------------
def pooled(c):
    return (c["pool_h"], c["pool_w"]) != (1, 1)


def served(c):
    """dcll_step_any_check: None = served, else (code, phrase of the message)"""
    if FZ.conv_shape(c) is None or c["c_in"] % c["groups"] or c["c_out"] % c["groups"]:
        return "DCLL_ERR_INVALID", ""
    if (c["stride"], c["dilation"], c["groups"]) != (1, 1, 1):
        return "DCLL_ERR_UNSUPPORTED", "plain convolutions only"
    if c["c_out"] > MAX_COUT:
        return "DCLL_ERR_UNSUPPORTED", "c_out <= 32"
    if max(c["kh"], c["kw"]) > MAX_K:
        return "DCLL_ERR_UNSUPPORTED", "kernels up to 16x16"
    if lds_floats(c) * 4 > LDS_MAX:
        return "DCLL_ERR_UNSUPPORTED", "exceeds the 160 KiB of LDS"
    return None


def lds_floats(c):
    ch, cw, _, _ = FZ.conv_shape(c)
    img = c["c_in"] * (c["h"] + 2 * c["pad_h"]) * (c["w"] + 2 * c["pad_w"])
    return img + (c["c_out"] * ch * cw if pooled(c) else 0) + 32


def lds_bytes(c):
    """dcll_conv_lif_step_any_lds: LDS bytes of a workgroup, 0 = not served"""
    return 0 if served(c) is not None else lds_floats(c) * 4


def steps(c):
    """MFMA steps of one chain = floats / 64 of w_scratch"""
    kk = c["kh"] * c["kw"]
    return (c["c_in"] // 2) * kk + ((kk + 1) // 2 if c["c_in"] % 2 else 0)


def tiles(c):
    ch, cw, _, _ = FZ.conv_shape(c)
    return (ch * cw + 31) // 32


def ns(c, B):
    """dcll_step_any_split: workgroups per sample (1 = the fused form)"""
    if pooled(c) or B < 1:
        return 1
    ntl = tiles(c)
    n = min((ntl + NW - 1) // NW, CUS // B)
    if n <= 1:
        return 1
    tpb = (ntl + n - 1) // n
    return (ntl + tpb - 1) // tpb


def tile_ranges(c, B):
    """[first tile, end tile) of every workgroup of a sample"""
    n, ntl = ns(c, B), tiles(c)
    tpb = (ntl + n - 1) // n
    return [(p * tpb, min((p + 1) * tpb, ntl)) for p in range(n)]


def form(c, B):
    return "k_lif_step_any<%d>%s" % (c["refractory"], " (pooling)" if pooled(c) else " (split)" if ns(c, B) > 1 else "")


def all_forms():
    return ["k_lif_step_any<%d>%s" % (r, s) for r in (0, 1) for s in ("", " (pooling)", " (split)")]


def launch_log(c, B):
    """the kernels of one dcll_conv_lif_step_any call in front of its readouts"""
    return ["k_seq_any_wprep"] + (["k_trace"] if ns(c, B) > 1 else []) + [form(c, B)]


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P2 = dict(kh=7, kw=7, pad_h=2, pad_w=2)
K7P3 = dict(kh=7, kw=7, pad_h=3, pad_w=3)
MNIST = [dict(K7P2, c_in=1, c_out=16, h=28, w=28, pool_h=2, pool_w=2), dict(K7P2, c_in=16, c_out=24, h=13, w=13),
         dict(K7P2, c_in=24, c_out=32, h=11, w=11, pool_h=2, pool_w=2)]
RATES = (.05, .15, .3)


def _named(seed):
    out = []
    for i, g in enumerate(MNIST):           # BASELINE config 1: no refractory trace, tensor time constants
        out.append(_case("step-mnist-l%d" % (i + 1), "named", seed * 100003 + i, refractory=0, tau_tensor=1, B=2, rate=RATES[i],
                         readout=1, output_layer=int(i == 2), **g))
    k = 10
    for h, w in ((16, 16), (24, 24), (12, 32)):
        for c_in in (1, 32):
            out.append(_case("step-radio-%dto32-%dx%d" % (c_in, h, w), "named", seed * 100003 + k, c_in=c_in, c_out=32, h=h, w=w,
                             tau_tensor=1, B=2, rate=.1 if c_in == 32 else .05, readout=1, target=24, **K7P3))
            k += 1
    return out


def _form_cases(seed):
    rows = []
    for r in (0, 1):
        rows += [("R%d-fused" % r, dict(c_in=3, c_out=9, h=9, w=7, refractory=r)),
                 ("R%d-pooling" % r, dict(c_in=4, c_out=32, h=6, w=10, pool_h=2, pool_w=2, refractory=r)),
                 ("R%d-split" % r, dict(c_in=2, c_out=5, h=17, w=16, refractory=r))]
    return [_case("step-form-%s" % n, "forms", seed * 100003 + 100 + i, **kw) for i, (n, kw) in enumerate(rows)]


# c_in at the LDS limit on 16x16, 3x3 pad 1: 324 c_in + 32 floats without pooling, 324 c_in + 8192 + 32 with c_out 32 and pooling 2
LDS_PLAIN = dict(c_out=4, h=16, w=16, refractory=0, rate=.1)
LDS_POOL = dict(c_out=32, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1)
# 17x17, 3x3 pad 1: 289 conv pixels = 10 tiles: two workgroups of five up to B = 128, one from B = 129
NS_B = dict(c_in=2, c_out=4, h=17, w=17)


def _boundary_cases(seed):
    rows = [("cout1", "one output channel", dict(c_in=7, c_out=1, h=9, w=9, refractory=0)),
            ("cout31", "c_out 31", dict(c_in=6, c_out=31, h=7, w=9, kh=2, kw=4)),
            ("cout32", "c_out 32: every MFMA row is a channel", dict(c_in=5, c_out=32, h=7, w=9, pool_h=2, pool_w=1)),
            ("cin1", "c_in 1: the odd-channel part alone, even tap count", dict(c_in=1, c_out=6, h=9, w=8, kh=2, kw=3)),
            ("cin3", "c_in 3: one pair and the odd channel", dict(c_in=3, c_out=6, h=8, w=9, kh=2, kw=2)),
            ("cin31", "c_in 31", dict(c_in=31, c_out=17, h=10, w=10, kh=3, kw=5, pad_h=1, pad_w=2, rate=.1)),
            ("zero-link", "odd c_in with an odd tap count: the chain ends with a zero link", dict(c_in=5, c_out=7, h=8, w=8)),
            ("zero-link-cin1", "c_in 1, 49 taps: 25 steps, the last half empty", dict(K7P3, c_in=1, c_out=12, h=10, w=9)),
            ("k16", "a 16x16 kernel", dict(c_in=2, c_out=5, h=18, w=17, kh=16, kw=16, pad_h=2, pad_w=3)),
            ("k1x1-plane1x1", "one pixel", dict(c_in=3, c_out=4, h=1, w=1, kh=1, kw=1, pad_h=0, pad_w=0, B=5)),
            ("pad-grows", "padding larger than the kernel's half: the conv plane grows",
             dict(c_in=2, c_out=6, h=5, w=6, pad_h=4, pad_w=3, pool_h=3, pool_w=2)),
            ("pad0-shrinks", "no padding: the conv plane shrinks", dict(c_in=3, c_out=7, h=12, w=9, kh=5, kw=4, pad_h=0, pad_w=0)),
            ("cp33", "33 conv pixels: a ragged second tile", dict(c_in=2, c_out=8, h=3, w=11)),
            ("pool3", "pooling 3 with its padding of 1", dict(c_in=4, c_out=12, h=10, w=11, pool_h=3, pool_w=3)),
            ("pool2x3-shrinks", "pooling (2, 3) on a shrinking plane",
             dict(c_in=3, c_out=7, h=12, w=10, kh=5, kw=4, pad_h=0, pad_w=0, pool_h=2, pool_w=3)),
            ("bias0", "bias = 0 (NULL): the chains start at +0", dict(c_in=4, c_out=6, h=8, w=8, bias=0)),
            ("bias0-pool", "bias = 0 with pooling", dict(c_in=3, c_out=6, h=8, w=8, bias=0, pool_h=2, pool_w=2)),
            ("tau-scalar", "scalar time constants", dict(c_in=4, c_out=6, h=9, w=8, tau_tensor=0, refractory=0)),
            ("tau-tensor", "(c_in, h, w) time constants", dict(c_in=4, c_out=6, h=9, w=8, tau_tensor=1, refractory=0)),
            ("tau-tensor-split", "(c_in, h, w) time constants through k_trace", dict(c_in=2, c_out=6, h=16, w=17, tau_tensor=1)),
            ("v-null", "out_v = NULL", dict(c_in=4, c_out=6, h=8, w=8, want_v=0)),
            ("v-null-pool", "out_v = NULL with pooling, no refractory pass at all",
             dict(c_in=4, c_out=6, h=8, w=8, want_v=0, pool_h=2, pool_w=2, refractory=0)),
            ("v-null-pool-R", "out_v = NULL with pooling, refractory", dict(c_in=4, c_out=6, h=8, w=8, want_v=0, pool_h=2, pool_w=2)),
            ("misalign", "operands offset by one float", dict(c_in=4, c_out=6, h=8, w=8, misalign=1, tau_tensor=1)),
            ("misalign-pool", "operands offset by one float, pooling", dict(c_in=3, c_out=6, h=9, w=8, misalign=1, pool_h=2, pool_w=2)),
            ("misalign-split", "operands offset by one float, split form", dict(c_in=2, c_out=6, h=17, w=16, misalign=1)),
            ("lds-cin126", "40856 floats of 40960: the last c_in that fits, no pooling", dict(LDS_PLAIN, c_in=126)),
            ("lds-pool-cin101", "40948 floats of 40960: the last c_in that fits, pooling", dict(LDS_POOL, c_in=101)),
            ("tiles8", "256 conv pixels = 8 tiles: one workgroup's waves, fused", dict(c_in=2, c_out=4, h=16, w=16)),
            ("tiles9", "272 conv pixels = 9 tiles: split 5 + 4", dict(c_in=2, c_out=4, h=16, w=17)),
            ("tiles17", "17 tiles: three workgroups 6 + 6 + 5", dict(c_in=2, c_out=4, h=17, w=32, refractory=0)),
            ("ns-batch", "10 tiles at B = 129 (256 / B = 1: fused) and the same samples at B = 128 (split)",
             dict(NS_B, B=129, also_B=128)),
            ("ns-batch-3to2", "17 tiles at B = 86 (256 / B = 2: 9 + 8) and at B = 85 (three workgroups)",
             dict(c_in=1, c_out=3, h=17, w=32, B=86, also_B=85, refractory=0))]
    return [_case("step-edge-%s" % n, "boundaries", seed * 100003 + 200 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _grid_cases(seed):
    return [_case("step-grid", "grid", seed * 100003 + 300, c_in=3, c_out=8, h=9, w=9, pool_h=2, pool_w=2, B=8, B_run=1100, readout=1)]


N_FREE = 60


def _free_draw(rng, k, seed):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(1, 33)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(1, 23)), w=int(rng.randint(1, 23)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(RATES[rng.randint(3)]), B=int(rng.randint(1, 6)), state0=int(rng.rand() < .8),
                 readout=int(rng.rand() < .5), target=int(rng.randint(1, 25)), want_v=int(rng.rand() < .8))
        c["output_layer"] = int(c["readout"] and rng.rand() < .3)
        cc = _case("step-free-%03d" % k, "free", seed * 100003 + 1000 + k, **c)
        if FZ.conv_shape(cc) is None or not FZ.sees_input(cc) or served(cc) is not None:
            continue
        while FZ.conv_work(cc) > FZ.WORK_MAX and cc["B"] > 1:       # the oracle's work capped: thin the batch
            cc["B"] = cc["B_run"] = cc["B"] // 2
        if FZ.conv_work(cc) > FZ.WORK_MAX:
            continue
        return cc


def cases(seed=SEED):
    """every case that runs (the refusals: refusals())"""
    rng = np.random.RandomState(seed)
    return (_named(seed) + _form_cases(seed) + _boundary_cases(seed) + _grid_cases(seed) +
            [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("stride2", dict(stride=2), U, "plain convolutions only"), ("dilation2", dict(dilation=2), U, "plain convolutions only"),
            ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"), ("cout33", dict(c_out=33), U, "c_out <= 32"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("lds-cin127", dict(LDS_PLAIN, c_in=127), U, "exceeds the 160 KiB of LDS"),
            ("lds-pool-cin102", dict(LDS_POOL, c_in=102), U, "exceeds the 160 KiB of LDS"),
            ("lds-radio-32x32", dict(K7P3, c_in=32, c_out=32, h=32, w=32), U, "exceeds the 160 KiB of LDS"),
            ("lds-radio-24x24-pool2", dict(K7P3, c_in=32, c_out=32, h=24, w=24, pool_h=2, pool_w=2), U, "exceeds the 160 KiB of LDS"),
            ("null-x", dict(null="x"), I, "null pointer"), ("null-eps1", dict(null="eps1"), I, "null pointer"),
            ("null-W", dict(null="W"), I, "null pointer"), ("null-scratch", dict(null="w_scratch"), I, "null pointer"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"), ("B-negative", dict(B=-1), I, "negative batch"),
            ("B0", dict(B=0), "DCLL_OK", ""), ("B0-unsupported", dict(B=0, stride=2), "DCLL_OK", "")]
    base = dict(FZ.CONV_DEFAULT, c_in=2, c_out=6, null=None, B=2, readout=0)
    return [dict(base, id="step-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


def by_id(cid):
    for c in cases() + refusals():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


describe = FZ.describe
cases_hash = FZ.cases_hash


def run(c):
    """(tensors, the oracle's three steps) of a case on its c['B'] distinct samples: FZ.conv_run, non-vacuity check included"""
    return FZ.conv_run({k: v for k, v in c.items() if k not in EXTRA})


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's index arithmetic, restated for the CPU proofs of tests/test_step_any_cases.py
# ---------------------------------------------------------------------------------------------------------------------------
def b_operand_reads(c, B):
    """For every workgroup of a sample: (lowest, highest) float offset into the staged image that any lane of any of its tiles
    forms as a B operand, the padded rows [yp0, yp1] it stages, and the clamped pixels of its lanes — the kernel's own walk
    (off advanced link by link) for the channel-pair part, the tap pairs of an odd last channel behind it."""
    ch, cw, _, _ = FZ.conv_shape(c)
    CP, WP = ch * cw, c["w"] + 2 * c["pad_w"]
    CHS = (c["h"] + 2 * c["pad_h"]) * WP
    kh, kw, KK = c["kh"], c["kw"], c["kh"] * c["kw"]
    npair = (c["c_in"] // 2) * KK
    offs = []                                   # wave-uniform offsets of the pair part
    off = kx = ky = 0
    for _ in range(npair):
        offs.append(off)
        off += 1
        kx += 1
        if kx == kw:
            kx, off = 0, off + WP - kw
            ky += 1
            if ky == kh:
                ky, off = 0, off + 2 * CHS - kh * WP
    assert offs == [(m // KK) * 2 * CHS + ((m % KK) // kw) * WP + (m % KK) % kw for m in range(npair)]
    out = []
    for t0, t1 in tile_ranges(c, B):
        lo, hi, pcs, rows = None, None, [], set()
        for tl in range(t0, t1):
            for j in range(32):
                pix = tl * 32 + j
                pc = min(pix, CP - 1)
                pcs.append((pix, pc))
                base0 = (pc // cw) * WP + pc % cw
                reads = [base0 + hh * CHS + o for o in (offs[0], offs[-1]) for hh in (0, 1)] if offs else []
                if c["c_in"] % 2:
                    for m in range((KK + 1) // 2):
                        for hh in (0, 1):
                            tap = 2 * m + hh
                            if tap < KK:
                                reads.append((c["c_in"] - 1) * CHS + base0 + (tap // kw) * WP + tap % kw)
                lo = min(reads) if lo is None else min(lo, min(reads))
                hi = max(reads) if hi is None else max(hi, max(reads))
                rows |= {pc // cw, pc // cw + kh - 1}
        pl = min(t1 * 32, CP) - 1
        yp0, yp1 = ((t0 * 32) // cw, pl // cw + kh - 1) if ns(c, B) > 1 else (0, c["h"] + 2 * c["pad_h"] - 1)
        out.append(dict(lo=lo, hi=hi, pcs=pcs, rows=(min(rows), max(rows)), staged=(yp0, yp1), image=c["c_in"] * CHS))
    return out
