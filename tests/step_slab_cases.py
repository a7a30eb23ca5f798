"""Seeded cases for dcll_conv_lif_step_slab (k_lif_step_slab, the MFMA per-step forward of plain conv layers of any number of output
channels in bands of output rows x slabs of 64 output channels; a layer dcll_conv_lif_step_wide serves, asked for with bands = 0, is
forwarded to it), built on tests/fuzz_cases.py like tests/step_wide_cases.py: a case is one of its conv cases (FZ.conv_run gives the
tensors and the C oracle's three steps from carried state) plus four keys:
    want_v   0: the call passes out_v = NULL
    B_run    batch on the device; the oracle runs on the first B distinct samples, the device on copies of them
    also_B   a second batch size: the other side of a step of the small-batch rule; per-sample results must be equal
    bands    the call's band count (0 = the rule)
Plain module: no GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_step_slab_cases.py proves the list
on the CPU; tests/test_gpu_step_slab.py runs the HIP kernel against it.  Re-run one alone:
    python -c "import step_slab_cases as S; print(S.describe(S.by_id('slab-radio4-l2')))"

The launcher is restated ONCE here (csrc/dcll_step_slab.hip: step_slab_layer_ok, step_slab_lds_floats, dcll_step_slab_plan;
csrc/dcll_any_shared.h: band_plan, slab_first, slab_rows; csrc/dcll_hip.hip: dcll_conv_lif_step_slab): band_plan(), slabs(),
lds_floats(), nb_fit(), plan(), served(), lds_bytes(), scratch_floats(), form(), launch_log(), b_operand_reads().

Strata:
  named      radio_ml_conv.yaml at netscale 4 (1 -> 128, 128 -> 128) and 3 (1 -> 96, 96 -> 96) on 16x16 (the two wide layers need two
             bands); at netscale 2 on 24x40 (64 -> 64: four bands, one slab)
  forms      one small case per template instance
  slabs      c_out 65 / 96 / 97 / 128 / 129 / 200 (last slabs of 1 / 32 / 33 / 64 / 1 / 8 rows); c_out 40 and 64 with bands = 2 (one
             slab through the new kernel)
  cin        c_in 1 / 3 / 64 / 70; 84 and 85 on 16x16 with 7x7 pad 3 (both sides of one band)
  shapes     1x1, 2x5, 3x3, 7x7 and 9x9 kernels; a 4x4 plane, odd planes, bands of 9 / 32 / 33 conv pixels; pooling 2, 3, (1,2),
             (3,2), floor-mode leftovers in the last band; 1, 2, 3 and ph bands
  options    plain and refractory, bias = none, scalar and tensor time constants, out_v = NULL, operands 4 bytes off
  rule       both sides of every 256 / (B NS) step of the small-batch rule at NS 2 and 3
  grid       c_out 65 on 4x4 at B_run = 300
  forwarded  c_out 40 and 64 with bands = 0
  free       uniform draws: c_out 65-200, c_in 1-24, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, planes up to 20x20, B 1-3,
             bands 0-3
  refuse     error returns before any launch (refusals())"""
import functools

import numpy as np

import fuzz_cases as FZ
import step_wide_cases as SW

SEED = 20281
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
NW = 8                  # waves of a workgroup
CUS = 256
MAX_K = 16
SLAB_ROWS, SLAB_MAX = 64, 65535
RULE_UNITS = 4          # DCLL_STEP_SLAB_UNITS
EXTRA = dict(want_v=1, B_run=None, also_B=None, bands=0)
RESEED_CAP = 6          # run(): sub-seeds tried until every (band, slab) of the case says something (asserted, CPU)


def _case(cid, stratum, seed, **kw):
    extra = {k: kw.pop(k, v) for k, v in EXTRA.items()}
    kw.setdefault("readout", 0)
    kw.setdefault("c_out", 65)
    kw.setdefault("B", 2)
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


def slabs(c):
    """[(first channel, rows)] of the layer's slabs: slab s owns [64 s, min(64 s + 64, c_out))"""
    n = (c["c_out"] + SLAB_ROWS - 1) // SLAB_ROWS
    return [(s * SLAB_ROWS, min(SLAB_ROWS, c["c_out"] - s * SLAB_ROWS)) for s in range(n)]


def band_plan(c, k, NB):
    """band k of NB in h (csrc/dcll_any_shared.h band_plan): owned pooled rows [P0, P1), conv rows [C0, C1), held input rows [I0, I1)"""
    ch, cw, ph, pw = FZ.conv_shape(c)
    pool, pph = c["pool_h"], (c["pool_h"] - 1) // 2
    P0, P1 = k * ph // NB, (k + 1) * ph // NB
    C0 = max(P0 * pool - pph, 0)
    C1 = ch if k == NB - 1 else max(P1 * pool - pph, 0)
    clip = lambda y: min(max(y, 0), c["h"])
    return dict(P0=P0, P1=P1, C0=C0, C1=C1, I0=clip(C0 - c["pad_h"]), I1=clip(C1 - c["pad_h"] + c["kh"] - 1))


def lds_floats(c, k, NB):
    """floats of the (band k, any slab) workgroup: the band's padded eps1 rows, the slab's v plane of a pooling layer, the bias"""
    _, cw, _, _ = FZ.conv_shape(c)
    r = band_plan(c, k, NB)
    crows = r["C1"] - r["C0"]
    return c["c_in"] * (crows + c["kh"] - 1) * (c["w"] + 2 * c["pad_w"]) + (SLAB_ROWS * crows * cw if pooled(c) else 0) + SLAB_ROWS


def lds_max(c, NB):
    return max(lds_floats(c, k, NB) for k in range(NB))


def nb_fit(c):
    """the smallest NB <= ph whose largest band fits in 160 KiB, None where not even one pooled row does"""
    ph = FZ.conv_shape(c)[2]
    for NB in range(1, ph + 1):
        if lds_max(c, NB) * 4 <= LDS_MAX:
            return NB
    return None


def layer_ok(c):
    """step_slab_layer_ok: None = a layer of this file, else (code, phrase of the message)"""
    if FZ.conv_shape(c) is None or c["c_in"] % c["groups"] or c["c_out"] % c["groups"]:
        return "DCLL_ERR_INVALID", ""
    if (c["stride"], c["dilation"], c["groups"]) != (1, 1, 1):
        return "DCLL_ERR_UNSUPPORTED", "plain convolutions only"
    if max(c["kh"], c["kw"]) > MAX_K:
        return "DCLL_ERR_UNSUPPORTED", "kernels up to 16x16"
    if len(slabs(c)) > SLAB_MAX:
        return "DCLL_ERR_UNSUPPORTED", "at most 65535 slabs"
    return None


def forwarded(c, bands=None):
    """the call IS dcll_conv_lif_step_wide's: c_out <= 64, the rule asked for, and that entry point serves the layer"""
    bands = c.get("bands", 0) if bands is None else bands
    return bands == 0 and c["c_out"] <= SLAB_ROWS and SW.served(c) is None


def plan(c, B, bands=None):
    """dcll_step_slab_plan: (NB, NS) of a call, or (code, phrase) of its refusal.  A forwarded call has no plan: (0, 0)"""
    bands = c.get("bands", 0) if bands is None else bands
    if bands >= 0 and B >= 1 and forwarded(c, bands):
        return 0, 0
    bad = layer_ok(c)
    if bad is not None:
        return bad
    if bands < 0:
        return "DCLL_ERR_INVALID", "negative band count"
    if B < 1:
        return "DCLL_ERR_INVALID", "batch of at least one"
    ch, cw, ph, pw = FZ.conv_shape(c)
    NS = len(slabs(c))
    if bands > 0:
        if bands > ph:
            return "DCLL_ERR_UNSUPPORTED", "more bands than pooled rows"
        if lds_max(c, bands) * 4 > LDS_MAX:
            return "DCLL_ERR_UNSUPPORTED", "exceeds the 160 KiB of LDS"
        return bands, NS
    fit = nb_fit(c)
    if fit is None:
        return "DCLL_ERR_UNSUPPORTED", "not even one pooled row"
    units = 2 * ((ch * cw + 31) // 32)
    ns0 = min((units + RULE_UNITS - 1) // RULE_UNITS, CUS // (B * NS), ph)
    return max(fit, ns0), NS


def served(c, B=1, bands=None):
    """None = the call is served (or forwarded), else (code, phrase)"""
    p = plan(c, B, bands)
    return None if isinstance(p[0], int) else p


def lds_bytes(c, B, bands=None):
    """dcll_conv_lif_step_slab_lds: bytes of the largest workgroup under the plan, 0 = not served"""
    bands = c.get("bands", 0) if bands is None else bands
    if bands >= 0 and B >= 1 and forwarded(c, bands):
        return SW.lds_bytes(c)
    p = plan(c, B, bands)
    return lds_max(c, p[0]) * 4 if isinstance(p[0], int) else 0


def steps(c):
    """MFMA steps of one chain"""
    return SW.steps(c)


def scratch_floats(c):
    """dcll_conv_lif_step_slab_scratch: 128 per MFMA step of a chain and slab"""
    return 0 if layer_ok(c) is not None else 128 * steps(c) * len(slabs(c))


def form(c, B=None, bands=None):
    if forwarded(c, bands):
        return SW.form(c, B)
    return "k_lif_step_slab<%d>%s" % (c["refractory"], " (pooling)" if pooled(c) else "")


def all_forms():
    return ["k_lif_step_slab<%d>%s" % (r, s) for r in (0, 1) for s in ("", " (pooling)")]


def launch_log(c, B, bands=None):
    """the kernels of one dcll_conv_lif_step_slab call in front of its readouts"""
    if forwarded(c, bands):
        return SW.launch_log(c, B)
    return ["k_step_slab_wprep", "k_trace", form(c, B, bands)]


def paired(c, k, NB, rows):
    """True where the waves of (band k, a slab of `rows` rows) hold both M tiles of their pixel tiles"""
    _, cw, _, _ = FZ.conv_shape(c)
    r = band_plan(c, k, NB)
    ntl = ((r["C1"] - r["C0"]) * cw + 31) // 32
    return rows > 32 and 2 * ((ntl + NW - 1) // NW) <= (2 * ntl + NW - 1) // NW


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P3 = dict(kh=7, kw=7, pad_h=3, pad_w=3)
RATES = (.05, .15, .3)
SMALL = dict(c_in=3, h=8, w=8)


def _named(seed):
    out = []
    k = 0
    for tag, co in (("radio4", 128), ("radio3", 96)):       # radio_ml_conv.yaml at netscale 4 / 3 on 16x16
        for l, c_in in ((1, 1), (2, co)):
            out.append(_case("slab-%s-l%d" % (tag, l), "named", seed * 100003 + k, c_in=c_in, c_out=co, h=16, w=16, tau_tensor=1,
                             B=2 if c_in == 1 else 1, rate=.05 if c_in == 1 else .1, readout=1, target=24, **K7P3))
            k += 1
    out.append(_case("slab-radio2-24x40-l2", "named", seed * 100003 + 9, c_in=64, c_out=64, h=24, w=40, tau_tensor=1, B=1, rate=.1,
                     readout=1, target=24, **K7P3))
    return out


def _form_cases(seed):
    rows = []
    for r in (0, 1):
        rows += [("R%d-plain" % r, dict(c_in=3, c_out=70, h=9, w=7, refractory=r)),
                 ("R%d-pooling" % r, dict(c_in=4, c_out=66, h=6, w=10, pool_h=2, pool_w=2, refractory=r))]
    return [_case("slab-form-%s" % n, "forms", seed * 100003 + 100 + i, **kw) for i, (n, kw) in enumerate(rows)]


def _slab_cases(seed):
    rows = [("cout65", "a last slab of 1 row", dict(SMALL, c_out=65)),
            ("cout96", "a last slab of 32 rows: one M tile, its second weight column never read", dict(SMALL, c_out=96)),
            ("cout97", "a last slab of 33 rows: one row of the second M tile", dict(SMALL, c_out=97, pool_h=2, pool_w=2)),
            ("cout128", "two full slabs", dict(SMALL, c_out=128)),
            ("cout129", "three slabs, the last of 1 row", dict(SMALL, c_out=129, pool_h=2, pool_w=1)),
            ("cout200", "four slabs, the last of 8 rows", dict(SMALL, c_out=200, refractory=0)),
            ("cout40-bands2", "c_out 40 with two bands: one slab through the new kernel", dict(SMALL, c_out=40, bands=2)),
            ("cout64-bands2", "c_out 64 with two bands, pooling", dict(SMALL, c_out=64, bands=2, pool_h=2, pool_w=2))]
    return [_case("slab-co-%s" % n, "slabs", seed * 100003 + 200 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _cin_cases(seed):
    rows = [("cin1", "c_in 1: the odd-channel part alone, even tap count", dict(c_in=1, h=9, w=8, kh=2, kw=3)),
            ("cin3", "c_in 3 with 3x3: the chains end with a zero link", dict(c_in=3, h=8, w=8)),
            ("cin64", "c_in 64", dict(c_in=64, h=8, w=8, rate=.1, B=1)),
            ("cin70", "c_in 70", dict(c_in=70, h=7, w=9, rate=.1, B=1, c_out=66)),
            ("cin84-k7", "c_in 84 on 16x16, 7x7 pad 3: 40720 floats, one band fits", dict(K7P3, c_in=84, h=16, w=16, rate=.1, B=1, B_run=128)),
            ("cin85-k7", "c_in 85 on 16x16, 7x7 pad 3: 41204 floats, two bands", dict(K7P3, c_in=85, h=16, w=16, rate=.1, B=1, B_run=128))]
    return [_case("slab-%s" % n, "cin", seed * 100003 + 300 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _shape_cases(seed):
    rows = [("k1x1", "a 1x1 kernel", dict(c_in=6, h=7, w=7, kh=1, kw=1, pad_h=0, pad_w=0)),
            ("k2x5", "a 2x5 kernel", dict(c_in=3, h=8, w=9, kh=2, kw=5, pad_h=1, pad_w=2)),
            ("k7x7", "a 7x7 kernel, three bands", dict(K7P3, c_in=2, h=9, w=9, bands=3)),
            ("k9x9", "a 9x9 kernel without padding", dict(c_in=2, h=12, w=11, kh=9, kw=9, pad_h=0, pad_w=0)),
            ("p4x4", "a 4x4 plane", dict(c_in=4, h=4, w=4)),
            ("p5x7", "an odd plane, ph bands", dict(c_in=3, h=5, w=7, bands=5)),
            ("p7x5-b1", "an odd plane, one band", dict(c_in=3, h=7, w=5, bands=1)),
            ("band9", "bands of 9 conv pixels", dict(c_in=4, h=6, w=3, bands=2)),
            ("band32", "bands of 32 conv pixels: one full tile each", dict(c_in=4, h=8, w=8, bands=2)),
            ("band33", "bands of 33 conv pixels: a ragged second tile", dict(c_in=2, h=6, w=11, bands=2)),
            ("tiles8", "256 conv pixels in one band: 8 pixel tiles, the waves hold both M tiles", dict(c_in=2, c_out=128, h=16, w=16, bands=1, B=1)),
            ("tiles5", "160 conv pixels in one band: 5 pixel tiles, paired", dict(c_in=2, c_out=70, h=10, w=16, bands=1, B=1)),
            ("pool2", "pooling 2, a leftover row behind the last window", dict(c_in=4, h=9, w=10, pool_h=2, pool_w=2, bands=2)),
            ("pool3", "pooling 3 with its padding of 1, a leftover row, three bands", dict(c_in=4, c_out=70, h=12, w=11, pool_h=3, pool_w=3, bands=3)),
            ("pool1x2", "pooling (1, 2)", dict(c_in=3, h=8, w=10, pool_h=1, pool_w=2)),
            ("pool3x2", "pooling (3, 2), ph bands", dict(c_in=3, c_out=67, h=12, w=10, kh=5, kw=4, pad_h=0, pad_w=0, pool_h=3, pool_w=2, bands=3)),
            ("pool2-rule", "pooling 2 under the rule", dict(c_in=3, h=12, w=12, pool_h=2, pool_w=2))]
    return [_case("slab-sh-%s" % n, "shapes", seed * 100003 + 400 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _option_cases(seed):
    rows = [("plain", "not refractory", dict(SMALL, refractory=0)),
            ("bias0", "bias = none (NULL): the chains start at +0", dict(SMALL, bias=0)),
            ("bias0-pool", "bias = none with pooling", dict(SMALL, bias=0, pool_h=2, pool_w=2)),
            ("tau-scalar", "scalar time constants", dict(SMALL, tau_tensor=0)),
            ("tau-tensor", "(c_in, h, w) time constants", dict(SMALL, tau_tensor=1, h=9)),
            ("v-null", "out_v = NULL", dict(SMALL, want_v=0)),
            ("v-null-pool", "out_v = NULL with pooling, no refractory pass at all", dict(SMALL, want_v=0, pool_h=2, pool_w=2, refractory=0)),
            ("v-null-pool-R", "out_v = NULL with pooling, refractory", dict(SMALL, want_v=0, pool_h=2, pool_w=2)),
            ("misalign", "operands offset by one float (w_scratch too: its 8-byte loads)", dict(SMALL, misalign=1, tau_tensor=1, c_out=97)),
            ("misalign-pool", "operands offset by one float, pooling", dict(SMALL, misalign=1, pool_h=2, pool_w=2, h=9))]
    return [_case("slab-opt-%s" % n, "options", seed * 100003 + 500 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


# 17x16, 3x3 pad 1: 272 conv pixels = 9 tiles = 18 units: ceil(18 / 4) = 5 bands while 256 / (B NS) allows them
RULE_PLANE = dict(c_in=1, h=17, w=16, rate=.15, B=2)
# (B_run, also_B) on both sides of 256 / (B NS) = 1|2, 2|3, 3|4, 4|5
RULE_STEPS = {2: ((65, 64), (43, 42), (33, 32), (26, 25)), 3: ((43, 42), (29, 28), (22, 21), (18, 17))}


def _rule_cases(seed):
    out = []
    for ns_, co in ((2, 70), (3, 129)):
        for i, (B1, B2) in enumerate(RULE_STEPS[ns_]):
            out.append(_case("slab-rule-ns%d-%dto%d" % (ns_, i + 1, i + 2), "rule", seed * 100003 + 600 + 10 * ns_ + i,
                             note="256 / (B NS) = %d at B = %d, %d at B = %d" % (i + 1, B1, i + 2, B2),
                             **dict(RULE_PLANE, c_out=co, B_run=B1, also_B=B2, refractory=i % 2)))
    return out


def _grid_cases(seed):
    return [_case("slab-grid", "grid", seed * 100003 + 700, c_in=3, c_out=65, h=4, w=4, B=3, B_run=300, readout=1)]


def _forwarded_cases(seed):
    rows = [("cout40", dict(c_in=3, c_out=40, h=9, w=7)), ("cout64", dict(c_in=4, c_out=64, h=6, w=10, pool_h=2, pool_w=2, refractory=0))]
    return [_case("slab-fwd-%s" % n, "forwarded", seed * 100003 + 800 + i, **kw) for i, (n, kw) in enumerate(rows)]


N_FREE = 30


def _free_draw(rng, k, seed):
    while True:
        c = dict(c_in=int(rng.randint(1, 25)), c_out=int(rng.randint(65, 201)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(1, 21)), w=int(rng.randint(1, 21)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(RATES[rng.randint(3)]), B=int(rng.randint(1, 4)), state0=int(rng.rand() < .8),
                 readout=int(rng.rand() < .5), target=int(rng.randint(1, 25)), want_v=int(rng.rand() < .8), bands=int(rng.randint(0, 4)))
        c["output_layer"] = int(c["readout"] and rng.rand() < .3)
        cc = _case("slab-free-%03d" % k, "free", seed * 100003 + 1000 + k, **c)
        if FZ.conv_shape(cc) is None or not FZ.sees_input(cc) or served(cc, cc["B"]) is not None:
            continue
        while FZ.conv_work(cc) > FZ.WORK_MAX and cc["B"] > 1:       # the oracle's work capped: thin the batch
            cc["B"] = cc["B_run"] = cc["B"] // 2
        if FZ.conv_work(cc) > FZ.WORK_MAX:
            continue
        return cc


def cases(seed=SEED):
    """every case that runs (the refusals: refusals())"""
    rng = np.random.RandomState(seed)
    return (_named(seed) + _form_cases(seed) + _slab_cases(seed) + _cin_cases(seed) + _shape_cases(seed) + _option_cases(seed) +
            _rule_cases(seed) + _grid_cases(seed) + _forwarded_cases(seed) + [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("stride2", dict(stride=2), U, "plain convolutions only"), ("dilation2", dict(dilation=2), U, "plain convolutions only"),
            ("groups2", dict(c_in=4, c_out=66, groups=2), U, "plain convolutions only"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("bands-above-ph", dict(bands=9), U, "more bands than pooled rows"),
            ("bands1-cin85", dict(K7P3, c_in=85, h=16, w=16, bands=1), U, "exceeds the 160 KiB of LDS"),
            ("bands1-radio4", dict(K7P3, c_in=128, c_out=128, h=16, w=16, bands=1), U, "exceeds the 160 KiB of LDS"),
            ("radio2-128x128", dict(K7P3, c_in=64, c_out=64, h=128, w=128), U, "not even one pooled row"),
            ("bands-negative", dict(bands=-1), I, "negative band count"),
            ("null-x", dict(null="x"), I, "null pointer"), ("null-W", dict(null="W"), I, "null pointer"),
            ("null-scratch", dict(null="w_scratch"), I, "null pointer"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"), ("B-negative", dict(B=-1), I, "negative batch"),
            ("B0", dict(B=0), "DCLL_OK", ""), ("B0-unsupported", dict(B=0, stride=2), "DCLL_OK", "")]
    base = dict(FZ.CONV_DEFAULT, c_in=2, c_out=70, null=None, B=2, readout=0, bands=0)
    return [dict(base, id="slab-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


@functools.lru_cache(maxsize=None)
def _index():
    return {c["id"]: c for c in cases() + refusals()}


def by_id(cid):
    return dict(_index()[cid])


describe = FZ.describe
cases_hash = FZ.cases_hash


# ---------------------------------------------------------------------------------------------------------------------------
# tensors and the oracle's trajectory, computed once per case and shared (callers must not write into them)
# ---------------------------------------------------------------------------------------------------------------------------
def part_vacuous(c, osteps, NB):
    """Why a trajectory would prove nothing about some (band, slab) workgroup of the plan with NB bands (None = it is fine): over
    the three steps the un-pooled spikes v > 0 of that band's conv rows and that slab's channels hold one value only"""
    for k in range(NB):
        r = band_plan(c, k, NB)
        for s, (co0, rows) in enumerate(slabs(c)):
            spk = np.stack([st["v"][:, co0:co0 + rows, r["C0"]:r["C1"]] > 0 for st in osteps])
            if spk.all() or not spk.any():
                return "band %d of %d, slab %d: spikes hold one value" % (k, NB, s)
    return None


def run_nb(c):
    """the band count the non-vacuity rule looks at: the plan of the case's own call (a forwarded call: one band)"""
    return max(plan(c, c["B_run"])[0], 1)


@functools.lru_cache(maxsize=None)
def _run(cid):
    c = by_id(cid)
    why = None
    for k in range(RESEED_CAP):
        cc = {key: v for key, v in c.items() if key not in EXTRA}
        cc["seed"] = c["seed"] + 50021 * k
        T, osteps = FZ.conv_run(cc)
        why = FZ.vacuous(c, osteps) or part_vacuous(c, osteps, run_nb(c))
        if why is None:
            T["reseeds"] = k
            return T, osteps
    raise AssertionError("%s: every one of %d sub-seeds leaves a (band, slab) without spikes or without silence (%s)" % (cid, RESEED_CAP, why))


def run(c):
    """(tensors, the oracle's three steps) of a case on its c['B'] distinct samples: FZ.conv_run on the first sub-seed (of RESEED_CAP,
    50021 apart) whose trajectory has spikes and non-spikes in every (band, slab) of the case's plan — chosen from the oracle alone"""
    return _run(c["id"])


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's index arithmetic and decomposition, restated for the CPU proofs of tests/test_step_slab_cases.py
# ---------------------------------------------------------------------------------------------------------------------------
def b_operand_reads(c, NB):
    """For every band: (lowest, highest) float offset into the staged rows that any lane of any pixel tile forms as a B operand,
    the staged floats, the clamped pixels of the lanes — the kernel's walk: the channel-pair part at (cp, ky, kx), the tap pairs of
    an odd last channel."""
    _, cw, _, _ = FZ.conv_shape(c)
    WP = c["w"] + 2 * c["pad_w"]
    kh, kw, KK = c["kh"], c["kw"], c["kh"] * c["kw"]
    npair = (c["c_in"] // 2) * KK
    out = []
    for k in range(NB):
        r = band_plan(c, k, NB)
        crows = r["C1"] - r["C0"]
        rows = crows + kh - 1
        CHS, NPb = rows * WP, crows * cw
        last = ((npair - 1) // KK) * 2 * CHS + (kh - 1) * WP + kw - 1 if npair else 0
        lo, hi, pcs = None, None, []
        for tl in range((NPb + 31) // 32):
            for j in range(32):
                pix = tl * 32 + j
                pc = min(pix, NPb - 1)
                pcs.append((pix, pc))
                base0 = (pc // cw) * WP + pc % cw
                reads = [base0 + hh * CHS + o for o in (0, last) for hh in (0, 1)] if npair else []
                if c["c_in"] % 2:
                    reads += [(c["c_in"] - 1) * CHS + base0 + (tap // kw) * WP + tap % kw for tap in range(KK)]
                lo = min(reads) if lo is None else min(lo, min(reads))
                hi = max(reads) if hi is None else max(hi, max(reads))
        out.append(dict(lo=lo, hi=hi, pcs=pcs, NPb=NPb, staged=c["c_in"] * CHS, rows=rows))
    return out


MUTANTS = ("halo-short", "slab-off-one-tile", "bias-of-slab0", "traces-twice")


def mutant_touches(c, NB, mutant):
    """can the mutant change anything in this case under NB bands?"""
    ns_ = len(slabs(c))
    if mutant == "halo-short":      # some band's last staged row is a row of the image (a row of zero padding carries nothing)
        return any(0 <= band_plan(c, k, NB)["C1"] - c["pad_h"] + c["kh"] - 2 < c["h"] for k in range(NB))
    if mutant == "slab-off-one-tile":
        return ns_ > 1
    if mutant == "bias-of-slab0":
        return ns_ > 1 and bool(c["bias"])
    return True


def sliced_oracle(c, T, osteps, NB, mutant=None):
    """The layer computed as the kernel decomposes it — band by band and slab by slab, each (band, slab) a run of the C oracle on
    slices: the band's padded eps1 rows [C0 - pad_h, C1 - pad_h + kh - 1) as a plane of its own (the zero padding in h written
    out, pad_h = 0), the slab's rows of W, bias and arp, no pooling; the traces advance ONCE, on the whole plane, in front (the
    oracle's own trace update on the slices is that same update row by row) — then the pooling pass over the band's pooled rows.
    -> per step dict(v, s, arp, eps0, eps1).  mutant: one of MUTANTS, a wrong decomposition the comparison must catch."""
    from oracle import c_oracle as C
    ch, cw, ph, pw = FZ.conv_shape(c)
    B, cin, kh = c["B"], c["c_in"], c["kh"]
    pre = [dict(eps0=T["eps0"], eps1=T["eps1"], arp=T["arp"])] + osteps[:-1]
    out = []
    pph, ppw = (c["pool_h"] - 1) // 2, (c["pool_w"] - 1) // 2
    for t, st in enumerate(osteps):
        x, e0, e1, arp0 = T["x"][t], pre[t]["eps0"], pre[t]["eps1"], pre[t]["arp"]
        if mutant == "traces-twice":    # the state the kernel would stage had k_trace run in front AND the kernel advanced it again
            e0, e1 = st["eps0"], st["eps1"]
        v = np.full((B, c["c_out"], ch, cw), np.nan, np.float32)
        arp = np.full_like(v, np.nan)
        s = np.full((B, c["c_out"], ph, pw), np.nan, np.float32)
        ne0, ne1 = np.full_like(e0, np.nan), np.full_like(e1, np.nan)
        for k in range(NB):
            r = band_plan(c, k, NB)
            y0, rows = r["C0"] - c["pad_h"], r["C1"] - r["C0"] + kh - 1

            def held(a):                # rows [y0, y0 + rows) of a (.., h, w) array, zeros outside the image
                o = np.zeros(a.shape[:-2] + (rows, a.shape[-1]), np.float32)
                lo, hi = max(y0, 0), min(y0 + rows, c["h"])
                if mutant == "halo-short":
                    hi = min(hi, y0 + rows - 1)
                if hi > lo:
                    o[..., lo - y0:hi - y0, :] = a[..., lo:hi, :]
                return o
            tau = [held(a) if c["tau_tensor"] else a for a in T["tau"]]
            for si, (co0, nrow) in enumerate(slabs(c)):
                w0 = co0 - 32 if (mutant == "slab-off-one-tile" and si > 0) else co0
                sd = {"i2h.weight": T["W"][w0:w0 + nrow], "i2h.alpha": tau[0], "i2h.tau_m__dt": tau[1], "i2h.alphas": tau[2],
                      "i2h.tau_s__dt": tau[3], "i2o.weight": np.zeros((1, nrow * (r["C1"] - r["C0"]) * cw), np.float32),
                      "i2o.bias": np.zeros(1, np.float32)}
                if T["b"] is not None:
                    b0 = 0 if (mutant == "bias-of-slab0" and si > 0) else co0
                    sd["i2h.bias"] = T["b"][b0:b0 + nrow]
                orc = C.OracleConvLayer(sd, (rows, c["w"]), (0, c["pad_w"]), (1, 1), 1.0 if c["refractory"] else 0.0,
                                        c.get("alpharp", FZ.ALPHARP), False, 1, 1, 1)
                assert (orc.ch, orc.cw) == (r["C1"] - r["C0"], cw)
                orc.init_state(B)
                orc.state[0][...], orc.state[1][...] = held(e0), held(e1)
                orc.state[2][...] = arp0[:, co0:co0 + nrow, r["C0"]:r["C1"]]
                vv = orc.forward(held(x))[3]
                v[:, co0:co0 + nrow, r["C0"]:r["C1"]] = vv
                arp[:, co0:co0 + nrow, r["C0"]:r["C1"]] = orc.state[2]
                lo, hi = max(y0, 0), min(y0 + rows, c["h"])
                if hi > lo:             # (a band deep in the padding holds no row of the image)
                    ne0[:, :, lo:hi], ne1[:, :, lo:hi] = orc.state[0][:, :, lo - y0:hi - y0], orc.state[1][:, :, lo - y0:hi - y0]
                for py in range(r["P0"], r["P1"]):          # the pooling pass: windows clipped to the band's conv rows and the plane
                    ys = [y for y in range(py * c["pool_h"] - pph, py * c["pool_h"] - pph + c["pool_h"]) if r["C0"] <= y < r["C1"]]
                    assert ys == [y for y in range(py * c["pool_h"] - pph, py * c["pool_h"] - pph + c["pool_h"]) if 0 <= y < ch]
                    for px in range(pw):
                        xs = [q for q in range(px * c["pool_w"] - ppw, px * c["pool_w"] - ppw + c["pool_w"]) if 0 <= q < cw]
                        win = v[:, co0:co0 + nrow, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
                        s[:, co0:co0 + nrow, py, px] = (win.max(axis=(2, 3)) > 0).astype(np.float32)
        out.append(dict(v=v, s=s, arp=arp, eps0=ne0, eps1=ne1))
    return out
