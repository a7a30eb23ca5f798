"""Seeded cases for dcll_conv_lif_step_wide (k_lif_step_wide, the MFMA per-step forward of plain conv layers with 33 .. 64 output
channels; narrower layers are forwarded to dcll_conv_lif_step_any), built on tests/fuzz_cases.py like tests/step_any_cases.py: a
case is one of its conv cases (FZ.conv_run gives the tensors and the C oracle's three steps from carried state) plus three keys:
    want_v   0: the call passes out_v = NULL
    B_run    batch on the device; the oracle runs on the first B distinct samples, the device on copies of them
    also_B   a second batch size (the first also_B samples): the other side of an NS threshold; per-sample results must be equal
Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_step_wide_cases.py proves the list
on the CPU; tests/test_gpu_step_wide.py runs the HIP kernel against it.  Re-run one alone:
    python -c "import step_wide_cases as S; print(S.describe(S.by_id('wide-radio2-l2')))"

The launcher is restated ONCE here (csrc/dcll_step_wide.hip: dcll_step_wide_check, step_wide_lds_floats, dcll_step_wide_split;
csrc/dcll_hip.hip: dcll_conv_lif_step_wide): served(), lds_bytes(), steps(), units(), ns(), unit_ranges(), form(), launch_log().
A case with c_out <= 32 is a forwarded one: its values are tests/step_any_cases.py's.

Strata:
  named      radio_ml_conv.yaml at netscale 2 (1 -> 64, 64 -> 64) and 1.5 (1 -> 48, 48 -> 48) on 16x16; mnist_conv.yaml at netscale 2
             (1 -> 32 forwarded, 32 -> 48 on 13x13, 48 -> 64 on 11x11 with pooling 2)
  forms      one small case per template instance
  mtile      the second M tile: c_out 33 / 40 / 63 / 64, odd c_in and c_in 1, 1x1 and 2x5 kernels, planes of 9 / 32 / 33 / 64 / 65
             conv pixels, pooling 2, 3 and (3,2), bias = none, scalar and tensor time constants, out_v = NULL, operands 4 bytes off
  split      both sides of units = 4 and of every 256 / B step, an odd upw, the 64 -> 64 layer fused at B_run = 257
  limits     both sides of 160 KiB with and without pooling at c_out 64
  grid       one small c_out 40 layer at B_run = 1100
  forwarded  three c_out <= 32 layers
  free       uniform draws: c_out 33-64, c_in 1-40, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, planes up to 22x22, B 1-5
  refuse     error returns before any launch (refusals())"""
import numpy as np

import fuzz_cases as FZ
import step_any_cases as SA

SEED = 20271
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
NW = 8              # waves of a workgroup
CUS = 256
MAX_K, MAX_COUT, MT = 16, 64, 2
SPLIT_UNITS = 4     # DCLL_STEP_WIDE_UNITS
EXTRA = dict(want_v=1, B_run=None, also_B=None)
# sub-seeds moved (by 50021 k) until the ORACLE's trajectory says something about the second M tile (second_tile_vacuous: a channel
# >= 32 spikes, a pixel of one stays silent, arp non-zero before the last step) — chosen on the CPU, from the oracle alone
RESEED = {"wide-mt-cout33": 1, "wide-free-000": 1}


def _case(cid, stratum, seed, **kw):
    extra = {k: kw.pop(k, v) for k, v in EXTRA.items()}
    kw.setdefault("readout", 0)
    kw.setdefault("c_out", 40)
    c = FZ._case(cid, stratum, seed + 50021 * RESEED.get(cid, 0), **kw)
    c.update(extra)
    if c["B_run"] is None:
        c["B_run"] = c["B"]
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the launcher, restated
# ---------------------------------------------------------------------------------------------------------------------------
def pooled(c):
    return (c["pool_h"], c["pool_w"]) != (1, 1)


def forwarded(c):
    return c["c_out"] <= 32


def served(c):
    """dcll_step_wide_check: None = served, else (code, phrase of the message)"""
    if FZ.conv_shape(c) is None or c["c_in"] % c["groups"] or c["c_out"] % c["groups"]:
        return "DCLL_ERR_INVALID", ""
    if (c["stride"], c["dilation"], c["groups"]) != (1, 1, 1):
        return "DCLL_ERR_UNSUPPORTED", "plain convolutions only"
    if c["c_out"] > MAX_COUT:
        return "DCLL_ERR_UNSUPPORTED", "c_out <= 64"
    if forwarded(c):
        return SA.served(c)
    if max(c["kh"], c["kw"]) > MAX_K:
        return "DCLL_ERR_UNSUPPORTED", "kernels up to 16x16"
    if lds_floats(c) * 4 > LDS_MAX:
        return "DCLL_ERR_UNSUPPORTED", "exceeds the 160 KiB of LDS"
    return None


def lds_floats(c):
    if forwarded(c):
        return SA.lds_floats(c)
    ch, cw, _, _ = FZ.conv_shape(c)
    img = c["c_in"] * (c["h"] + 2 * c["pad_h"]) * (c["w"] + 2 * c["pad_w"])
    return img + (c["c_out"] * ch * cw if pooled(c) else 0) + 32 * MT


def lds_bytes(c):
    """dcll_conv_lif_step_wide_lds: LDS bytes of a workgroup, 0 = not served"""
    return 0 if served(c) is not None else lds_floats(c) * 4


def steps(c):
    """MFMA steps of one chain"""
    return SA.steps(c)


def scratch_floats(c):
    """dcll_conv_lif_step_wide_scratch"""
    return 0 if served(c) is not None else steps(c) * (64 if forwarded(c) else 64 * MT)


def tiles(c):
    return SA.tiles(c)


def units(c):
    """(pixel tile, M tile) units of a sample: u = 2 tile + mt"""
    return MT * tiles(c)


def ns(c, B):
    """dcll_step_wide_split: workgroups per sample (1 = the fused form)"""
    if forwarded(c):
        return SA.ns(c, B)
    if pooled(c) or B < 1:
        return 1
    n = min((units(c) + SPLIT_UNITS - 1) // SPLIT_UNITS, CUS // B)
    if n <= 1:
        return 1
    upw = (units(c) + n - 1) // n
    return (units(c) + upw - 1) // upw


def unit_ranges(c, B):
    """[first unit, end unit) of every workgroup of a sample"""
    n, nu = ns(c, B), units(c)
    upw = (nu + n - 1) // n
    return [(p * upw, min((p + 1) * upw, nu)) for p in range(n)]


def form(c, B):
    if forwarded(c):
        return SA.form(c, B)
    return "k_lif_step_wide<%d>%s" % (c["refractory"], " (pooling)" if pooled(c) else " (split)" if ns(c, B) > 1 else "")


def all_forms():
    return ["k_lif_step_wide<%d>%s" % (r, s) for r in (0, 1) for s in ("", " (pooling)", " (split)")]


def launch_log(c, B):
    """the kernels of one dcll_conv_lif_step_wide call in front of its readouts"""
    if forwarded(c):
        return SA.launch_log(c, B)
    return ["k_step_wide_wprep"] + (["k_trace"] if ns(c, B) > 1 else []) + [form(c, B)]


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P2 = dict(kh=7, kw=7, pad_h=2, pad_w=2)
K7P3 = dict(kh=7, kw=7, pad_h=3, pad_w=3)
RATES = (.05, .15, .3)


def _named(seed):
    out = []
    k = 0
    for tag, co in (("radio2", 64), ("radio15", 48)):       # radio_ml_conv.yaml at netscale 2 / 1.5 on 16x16
        for l, c_in in ((1, 1), (2, co)):
            out.append(_case("wide-%s-l%d" % (tag, l), "named", seed * 100003 + k, c_in=c_in, c_out=co, h=16, w=16, tau_tensor=1, B=2,
                             rate=.05 if c_in == 1 else .1, readout=1, target=24, **K7P3))
            k += 1
    mnist = [dict(K7P2, c_in=1, c_out=32, h=28, w=28, pool_h=2, pool_w=2), dict(K7P2, c_in=32, c_out=48, h=13, w=13),
             dict(K7P2, c_in=48, c_out=64, h=11, w=11, pool_h=2, pool_w=2)]
    for i, g in enumerate(mnist):                           # mnist_conv.yaml at netscale 2: no refractory trace
        out.append(_case("wide-mnist2-l%d" % (i + 1), "named", seed * 100003 + 10 + i, refractory=0, tau_tensor=1, B=2, rate=RATES[i],
                         readout=1, output_layer=int(i == 2), **g))
    return out


def _form_cases(seed):
    rows = []
    for r in (0, 1):
        rows += [("R%d-fused" % r, dict(c_in=3, c_out=40, h=9, w=7, refractory=r)),
                 ("R%d-pooling" % r, dict(c_in=4, c_out=64, h=6, w=10, pool_h=2, pool_w=2, refractory=r)),
                 ("R%d-split" % r, dict(c_in=2, c_out=33, h=8, w=12, refractory=r))]
    return [_case("wide-form-%s" % n, "forms", seed * 100003 + 100 + i, **kw) for i, (n, kw) in enumerate(rows)]


def _mtile_cases(seed):
    rows = [("cout33", "one row of the second M tile", dict(c_in=6, c_out=33, h=7, w=9, kh=2, kw=4)),
            ("cout40", "c_out 40", dict(c_in=4, c_out=40, h=8, w=8)),
            ("cout63", "c_out 63", dict(c_in=5, c_out=63, h=7, w=9, pool_h=2, pool_w=1)),
            ("cout64", "c_out 64: every MFMA row of both tiles is a channel", dict(c_in=4, c_out=64, h=8, w=9)),
            ("cin1", "c_in 1: the odd-channel part alone, even tap count", dict(c_in=1, c_out=40, h=9, w=8, kh=2, kw=3)),
            ("cin5-zero-link", "odd c_in with an odd tap count: the chains end with a zero link", dict(c_in=5, c_out=36, h=8, w=8)),
            ("cin31", "c_in 31", dict(c_in=31, c_out=49, h=10, w=10, kh=3, kw=5, pad_h=1, pad_w=2, rate=.1)),
            ("k1x1", "a 1x1 kernel", dict(c_in=6, c_out=40, h=7, w=7, kh=1, kw=1, pad_h=0, pad_w=0)),
            ("k2x5", "a 2x5 kernel", dict(c_in=3, c_out=40, h=8, w=9, kh=2, kw=5, pad_h=1, pad_w=2)),
            ("cp9", "9 conv pixels", dict(c_in=4, c_out=40, h=3, w=3)),
            ("cp32", "32 conv pixels: one full tile", dict(c_in=4, c_out=40, h=4, w=8)),
            ("cp33", "33 conv pixels: a ragged second tile", dict(c_in=2, c_out=40, h=3, w=11)),
            ("cp64", "64 conv pixels: two full tiles", dict(c_in=2, c_out=40, h=8, w=8)),
            ("cp65", "65 conv pixels: a ragged third tile, split", dict(c_in=2, c_out=40, h=5, w=13)),
            ("pool2", "pooling 2", dict(c_in=4, c_out=40, h=10, w=10, pool_h=2, pool_w=2)),
            ("pool3", "pooling 3 with its padding of 1", dict(c_in=4, c_out=44, h=10, w=11, pool_h=3, pool_w=3)),
            ("pool3x2", "pooling (3, 2)", dict(c_in=3, c_out=39, h=12, w=10, kh=5, kw=4, pad_h=0, pad_w=0, pool_h=3, pool_w=2)),
            ("bias0", "bias = none (NULL): the chains start at +0", dict(c_in=4, c_out=40, h=8, w=8, bias=0)),
            ("bias0-pool", "bias = none with pooling", dict(c_in=3, c_out=40, h=8, w=8, bias=0, pool_h=2, pool_w=2)),
            ("tau-scalar", "scalar time constants", dict(c_in=4, c_out=40, h=9, w=8, tau_tensor=0, refractory=0)),
            ("tau-tensor", "(c_in, h, w) time constants", dict(c_in=4, c_out=40, h=9, w=8, tau_tensor=1, refractory=0)),
            ("tau-tensor-split", "(c_in, h, w) time constants through k_trace", dict(c_in=2, c_out=40, h=8, w=12, tau_tensor=1)),
            ("v-null", "out_v = NULL", dict(c_in=4, c_out=40, h=8, w=8, want_v=0)),
            ("v-null-pool", "out_v = NULL with pooling, no refractory pass at all",
             dict(c_in=4, c_out=40, h=8, w=8, want_v=0, pool_h=2, pool_w=2, refractory=0)),
            ("v-null-pool-R", "out_v = NULL with pooling, refractory", dict(c_in=4, c_out=40, h=8, w=8, want_v=0, pool_h=2, pool_w=2)),
            ("misalign", "operands offset by one float (w_scratch too: its 8-byte loads)", dict(c_in=4, c_out=40, h=8, w=8, misalign=1, tau_tensor=1)),
            ("misalign-pool", "operands offset by one float, pooling", dict(c_in=3, c_out=40, h=9, w=8, misalign=1, pool_h=2, pool_w=2)),
            ("misalign-split", "operands offset by one float, split form", dict(c_in=2, c_out=40, h=8, w=12, misalign=1))]
    return [_case("wide-mt-%s" % n, "mtile", seed * 100003 + 200 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


# 17x16, 3x3 pad 1: 272 conv pixels = 9 tiles = 18 units: ceil(18 / 4) = 5 workgroups while 256 / B allows them
NS_B = dict(c_in=1, c_out=33, h=17, w=16, rate=.15)


def _split_cases(seed):
    rows = [("units4", "64 conv pixels = 4 units: fused", dict(c_in=2, c_out=48, h=8, w=8)),
            ("units6", "96 conv pixels = 6 units: two workgroups of three", dict(c_in=2, c_out=48, h=8, w=12)),
            ("upw-odd", "upw 3: the two M tiles of pixel tile 1 sit in different workgroups", dict(c_in=3, c_out=64, h=8, w=12)),
            ("upw-odd-5", "22 units: four workgroups of 6, 6, 6, 4 at B = 52, five of 5, 5, 5, 5, 2 at B = 51 (upw odd)", dict(c_in=1, c_out=34, h=11, w=32, B=52, also_B=51, rate=.15)),
            ("ns-1to2", "256 / B = 1 (fused) at B = 129, 2 at B = 128", dict(NS_B, B=129, also_B=128)),
            ("ns-2to3", "256 / B = 2 at B = 86, 3 at B = 85", dict(NS_B, B=86, also_B=85, refractory=0)),
            ("ns-3to4", "256 / B = 3 at B = 65, 4 at B = 64", dict(NS_B, B=65, also_B=64)),
            ("ns-4to5", "256 / B = 4 at B = 52, 5 = ceil(units / 4) at B = 51", dict(NS_B, B=52, also_B=51, refractory=0)),
            ("radio2-l2-fused", "the 64 -> 64 layer fused: 257 copies of two samples",
             dict(K7P3, c_in=64, c_out=64, h=16, w=16, tau_tensor=1, B=2, B_run=257, rate=.1))]
    return [_case("wide-split-%s" % n, "split", seed * 100003 + 300 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


# c_in at the LDS limit on 16x16, 3x3 pad 1, c_out 64: 324 c_in + 64 floats without pooling, 324 c_in + 16384 + 64 with pooling 2
LDS_PLAIN = dict(c_out=64, h=16, w=16, refractory=0, rate=.1, B=1)
LDS_POOL = dict(c_out=64, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1, B=1)


def _limit_cases(seed):
    rows = [("lds-cin126", "40888 floats of 40960: the last c_in that fits, no pooling", dict(LDS_PLAIN, c_in=126)),
            ("lds-pool-cin75", "40748 floats of 40960: the last c_in that fits, pooling", dict(LDS_POOL, c_in=75))]
    return [_case("wide-limit-%s" % n, "limits", seed * 100003 + 400 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _grid_cases(seed):
    return [_case("wide-grid", "grid", seed * 100003 + 500, c_in=3, c_out=40, h=9, w=9, pool_h=2, pool_w=2, B=8, B_run=1100, readout=1)]


def _forwarded_cases(seed):
    rows = [("fused", dict(c_in=3, c_out=9, h=9, w=7)), ("pooling", dict(c_in=4, c_out=32, h=6, w=10, pool_h=2, pool_w=2, refractory=0)),
            ("split", dict(c_in=2, c_out=5, h=17, w=16))]
    return [_case("wide-fwd-%s" % n, "forwarded", seed * 100003 + 600 + i, **kw) for i, (n, kw) in enumerate(rows)]


N_FREE = 40


def _free_draw(rng, k, seed):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(33, 65)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(1, 23)), w=int(rng.randint(1, 23)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(RATES[rng.randint(3)]), B=int(rng.randint(1, 6)), state0=int(rng.rand() < .8),
                 readout=int(rng.rand() < .5), target=int(rng.randint(1, 25)), want_v=int(rng.rand() < .8))
        c["output_layer"] = int(c["readout"] and rng.rand() < .3)
        cc = _case("wide-free-%03d" % k, "free", seed * 100003 + 1000 + k, **c)
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
    return (_named(seed) + _form_cases(seed) + _mtile_cases(seed) + _split_cases(seed) + _limit_cases(seed) + _grid_cases(seed) +
            _forwarded_cases(seed) + [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("cout65", dict(c_out=65), U, "c_out <= 64"), ("stride2", dict(stride=2), U, "plain convolutions only"),
            ("dilation2", dict(dilation=2), U, "plain convolutions only"), ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("lds-cin127", dict(LDS_PLAIN, c_in=127), U, "exceeds the 160 KiB of LDS"),
            ("lds-pool-cin76", dict(LDS_POOL, c_in=76), U, "exceeds the 160 KiB of LDS"),
            ("lds-radio2-32x32", dict(K7P3, c_in=64, c_out=64, h=32, w=32), U, "exceeds the 160 KiB of LDS"),
            ("null-x", dict(null="x"), I, "null pointer"), ("null-W", dict(null="W"), I, "null pointer"),
            ("null-scratch", dict(null="w_scratch"), I, "null pointer"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"), ("B-negative", dict(B=-1), I, "negative batch"),
            ("B0", dict(B=0), "DCLL_OK", ""), ("B0-unsupported", dict(B=0, c_out=65), "DCLL_OK", "")]
    base = dict(FZ.CONV_DEFAULT, c_in=2, c_out=40, null=None, B=2, readout=0)
    return [dict(base, id="wide-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


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


def second_tile_vacuous(c, T, osteps):
    """Why a c_out > 32 trajectory would prove nothing about the second M tile (None = it is fine): over the three steps no
    channel >= 32 spikes, or every pixel of those channels spikes at every step; a refractory layer's arp of those channels is
    zero before the last step."""
    if forwarded(c):
        return None
    spk = np.stack([st["s"][:, 32:] for st in osteps])
    if not spk.any():
        return "no channel >= 32 spikes"
    if spk.all():
        return "no pixel of a channel >= 32 stays silent"
    if c["refractory"] and not np.any(osteps[-2]["arp"][:, 32:]):
        return "arp of the channels >= 32 is zero before the last step"
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's index arithmetic, restated for the CPU proofs of tests/test_step_wide_cases.py
# ---------------------------------------------------------------------------------------------------------------------------
def b_operand_reads(c, B):
    """For every workgroup of a sample (c_out > 32): (lowest, highest) float offset into the staged image that any lane of any of
    its units' pixel tiles forms as a B operand, the padded rows [yp0, yp1] it stages, the rows its windows touch and the clamped
    pixels of its lanes — the kernel's walk: the channel-pair part at (cp, ky, kx), the tap pairs of an odd last channel."""
    ch, cw, _, _ = FZ.conv_shape(c)
    CP, WP = ch * cw, c["w"] + 2 * c["pad_w"]
    CHS = (c["h"] + 2 * c["pad_h"]) * WP
    kh, kw, KK = c["kh"], c["kw"], c["kh"] * c["kw"]
    npair = (c["c_in"] // 2) * KK
    first = 0
    last = ((npair - 1) // KK) * 2 * CHS + (kh - 1) * WP + kw - 1 if npair else 0
    out = []
    for u0, u1 in unit_ranges(c, B):
        tl0, tl1 = u0 // 2, (u1 + 1) // 2
        lo, hi, pcs, rows = None, None, [], set()
        for tl in sorted({u // 2 for u in range(u0, u1)}):
            assert tl0 <= tl < tl1
            for j in range(32):
                pix = tl * 32 + j
                pc = min(pix, CP - 1)
                pcs.append((pix, pc))
                base0 = (pc // cw) * WP + pc % cw
                reads = [base0 + hh * CHS + o for o in (first, last) for hh in (0, 1)] if npair else []
                if c["c_in"] % 2:
                    reads += [(c["c_in"] - 1) * CHS + base0 + (tap // kw) * WP + tap % kw for tap in range(KK)]
                lo = min(reads) if lo is None else min(lo, min(reads))
                hi = max(reads) if hi is None else max(hi, max(reads))
                rows |= {pc // cw, pc // cw + kh - 1}
        pl = min(tl1 * 32, CP) - 1
        yp0, yp1 = ((tl0 * 32) // cw, pl // cw + kh - 1) if ns(c, B) > 1 else (0, c["h"] + 2 * c["pad_h"] - 1)
        out.append(dict(lo=lo, hi=hi, pcs=pcs, rows=(min(rows), max(rows)), staged=(yp0, yp1), image=c["c_in"] * CHS))
    return out
