"""Seeded cases for dcll_conv_lif_sequence_bands (k_lif_seq_band: the fused all-T kernel of a plain conv layer with SEVERAL
workgroups per sample, each on a band of output rows), their tensors and the C oracle's trajectories — in the style of
tests/seq_wide_cases.py; the case format, the tensor draws and the oracle stepping are tests/seq_any_cases.py's.  Plain module: no
GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_seq_band_cases.py proves the lists on the CPU;
tests/test_gpu_seq_band.py runs the HIP kernel against them.  Re-run one alone:
    python -c "import seq_band_cases as S; print(S.describe(S.by_id('band-radio2-64to64-b4')))"

A case is seq_any_cases' dict plus `bands` (0: the library's rule, n: exactly n).  Restated ONCE here, from
csrc/dcll_seq_band.hip: the band plan (plan()), the LDS of a band (band_floats(), lds_bytes()), the scratch (scratch_floats()), the
default rule (rule()), the template instance and the launch log (variant(), launch_log()).

Strata:
  named       radio_ml_conv.yaml at netscale 2 on 16x16 (1 -> 64, 64 -> 64 refractory and plain) at 2 / 4 / 8 bands; at netscale 1
              on 48x48 (1 -> 32, 32 -> 32: refused by dcll_conv_lif_sequence_wide, served here); mnist_conv.yaml's three layers at
              netscale 1 and 2 at 2 and 4 bands;
  edges       the smallest shapes at which the banding can go wrong (see the notes of the rows);
  boundaries  both sides of the 160 KiB limit for an explicit band count, of whole-weights-in-LDS, of every threshold of the
              default rule (the far side of the first: refusals());
  grid        B = 300 x 4 bands from 8 distinct samples (1200 workgroups: beyond residency), TWO consecutive calls;
  forwarded   bands = 1, and bands = 0 where the rule picks 1 (one chain per wave; two M tiles at B = 200): the one-workgroup
              kernels' launch log;
  free        uniform draws: c_in 1-40, c_out 1-64, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, h, w 3-40, bands 1 .. ph;
  refuse      error returns before any launch (refusals())."""
import json

import numpy as np

import seq_any_cases as A
import seq_wide_cases as W

ALPHARP = A.ALPHARP
SEED = 20422
WORK_FREE_MAX = A.WORK_FREE_MAX
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
THREADS, NW = 512, 8
MAX_K, MAX_COUT = 16, 64
CUS = 256

DEFAULT = dict(A.DEFAULT, c_in=2, c_out=40, h=8, w=8, bands=2)
out_shape, valid, work, cases_hash = A.out_shape, A.valid, A.work, A.cases_hash
pack_planes, unpack_planes = A.pack_planes, A.unpack_planes
steps = A.steps


def describe(c):
    return json.dumps(c, sort_keys=True)


def _case(cid, stratum, seed, bands=2, **kw):
    c = A._case(cid, stratum, seed, **dict(dict(c_in=DEFAULT["c_in"], c_out=DEFAULT["c_out"], h=DEFAULT["h"], w=DEFAULT["w"]), **kw))
    c["bands"] = int(bands)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the band plan, the LDS, the rule, the dispatch — restated
# ---------------------------------------------------------------------------------------------------------------------------
def mt(c):
    return (c["c_out"] + 31) // 32


def plan(c, nb):
    """the rows of each of nb bands: dicts P (pooled rows), C (conv rows), I (input rows held), O (input rows owned), each a
    half-open (lo, hi)"""
    ch, cw, ph, pw = out_shape(c)
    h, kh, pad, pool = c["h"], c["kh"], c["pad_h"], c["pool_h"]
    pph = (pool - 1) // 2
    clip = lambda y: min(max(y, 0), h)
    first = lambda P: max(P * pool - pph, 0)            # first conv row of pooled row P's window
    out = []
    for k in range(nb):
        P0, P1 = k * ph // nb, (k + 1) * ph // nb
        C0, C1 = first(P0), (ch if k == nb - 1 else first(P1))
        I0, I1 = clip(C0 - pad), clip(C1 - pad + kh - 1)
        O1 = h if k == nb - 1 else clip(C1 - pad)
        out.append(dict(P=(P0, P1), C=(C0, C1), I=(I0, I1), O=(I0, O1)))
    return out


def band_floats(c, band):
    """the working set of one band in floats, without the weights"""
    ch, cw, _, _ = out_shape(c)
    (C0, C1), (I0, I1) = band["C"], band["I"]
    img = c["c_in"] * (C1 - C0 + c["kh"] - 1) * (c["w"] + 2 * c["pad_w"])
    e0 = c["c_in"] * (I1 - I0) * c["w"]
    vpl = c["c_out"] * (C1 - C0) * cw
    return img + e0 + vpl * (2 if c["refractory"] else 1) + 4 * c["c_in"] + 32 * mt(c)


def _layer_ok(c):
    return valid(c) and (c["stride"], c["dilation"], c["groups"]) == (1, 1, 1) and c["c_out"] <= MAX_COUT and max(c["kh"], c["kw"]) <= MAX_K


def fits(c, n):
    """n bands fit: one band = dcll_conv_lif_sequence_wide's own predicate, more = the largest band's set within the LDS"""
    if n == 1:
        return W.lds_bytes(c) > 0
    return max(band_floats(c, b) for b in plan(c, n)) * 4 <= LDS_MAX


def tiles_max(c, n):
    cw = out_shape(c)[1]
    return max(((b["C"][1] - b["C"][0]) * cw + 31) // 32 for b in plan(c, n))


def rule(c, B):
    """the default rule (bands = 0): the smallest count that fits, raised while B n <= 256 (one round of the card) and not beyond
    the count at which more bands stop paying — one band when the one-workgroup kernel already runs ONE chain per wave
    (MT ceil(tiles / 8) == 1), several bands down to one pixel tile per band; 0: none fits"""
    ph = out_shape(c)[2]
    best = 0
    for n in range(1, ph + 1):
        if not fits(c, n):
            continue
        if best and B * n > CUS:
            break
        best = n
        tiles = tiles_max(c, n)
        if (mt(c) * ((tiles + NW - 1) // NW) == 1) if n == 1 else tiles <= 1:
            break
    return best


def band_count(c, B=None, bands=None):
    """dcll_conv_lif_sequence_bands_plan: the band count the call runs, 0 = refused"""
    B = c.get("B", 1) if B is None else B
    bands = c["bands"] if bands is None else bands
    if not _layer_ok(c) or bands < 0 or bands > out_shape(c)[2]:
        return 0
    if bands == 0:
        return rule(c, max(B, 1))
    return bands if fits(c, bands) else 0


def lds_bytes(c, bands=None):
    """dcll_conv_lif_sequence_bands_lds: the largest band's bytes (0 bands: at the rule's count for B = 1;
    one band: dcll_conv_lif_sequence_wide_lds), 0 = refused"""
    n = band_count(c, 1, bands)
    if n == 0:
        return 0
    return W.lds_bytes(c) if n == 1 else 4 * max(band_floats(c, b) for b in plan(c, n))


def scratch_floats(c, B=None):
    """dcll_conv_lif_sequence_bands_scratch: the permuted weights + the snapshot of eps0 / eps1"""
    B = c["B"] if B is None else B
    if band_count(c, B, 0) == 0:
        return 0
    return 64 * mt(c) * steps(c) + 2 * B * c["c_in"] * c["h"] * c["w"]


def whole_weights(c, n):
    base = max(band_floats(c, b) for b in plan(c, n))
    return (base + steps(c) * 64 * mt(c)) * 4 <= LDS_MAX


def variant(c):
    """the template instance a case runs: 'k_lif_seq_band<MT,R,WLDS>', or the one-workgroup kernels' for one band"""
    n = band_count(c)
    assert n > 0, c["id"]
    if n == 1:
        return W.variant(c)
    return "k_lif_seq_band<%d,%d,%d>" % (mt(c), c["refractory"], int(whole_weights(c, n)))


def launch_log(c):
    """the launch log of one call (the weight permutation, the snapshot and the zero fill are not logged; one band: the sibling's)"""
    return W.launch_log(c) if band_count(c) == 1 else [variant(c)]


def all_variants():
    return ["k_lif_seq_band<%d,%d,%d>" % (m, r, l) for m in (1, 2) for r in (0, 1) for l in (1, 0)]


def shared_words(c, n):
    """pooled-pixel positions of the band boundaries that fall inside a spike word: the launcher zero-fills spk_out when any"""
    pw = out_shape(c)[3]
    return [b["P"][0] * pw for b in plan(c, n)[1:] if (b["P"][0] * pw) % 32]


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P2, K7P3, K1 = A.K7P2, A.K7P3, W.K1


def _named(seed):
    rows = []
    radio2 = [("radio2-1to64", dict(K7P3, c_in=1, c_out=64, h=16, w=16, tau_tensor=1, Ts=(2,), B=2, rate=.02)),
              ("radio2-64to64", dict(K7P3, c_in=64, c_out=64, h=16, w=16, tau_tensor=1, Ts=(2,), B=1, rate=.1)),
              ("radio2-64to64-plain", dict(K7P3, c_in=64, c_out=64, h=16, w=16, tau_tensor=1, refractory=0, Ts=(2,), B=1, rate=.1))]
    for i, (n, kw) in enumerate(radio2):           # (one draw per layer shape: the band counts share its oracle trajectory)
        rows += [("%s-b%d" % (n, nb), i, nb, kw) for nb in (2, 4, 8)]
    rows += [("radio1-48x48-1to32", 10, 0, dict(K7P3, c_in=1, c_out=32, h=48, w=48, tau_tensor=1, Ts=(2,), B=2, rate=.02)),
             ("radio1-48x48-32to32", 11, 0, dict(K7P3, c_in=32, c_out=32, h=48, w=48, tau_tensor=1, Ts=(2,), B=1, rate=.1))]
    for s, scale in ((1, 1), (2, 2)):
        for i, g in enumerate(A.MNIST):
            kw = dict(g, c_in=g["c_in"] * (scale if i else 1), c_out=g["c_out"] * scale, refractory=0, tau_tensor=1, Ts=(2,), B=2,
                      rate=A.RATES[i])
            rows += [("mnist%d-l%d-b%d" % (s, i + 1, nb), 20 + 3 * s + i, nb, kw) for nb in (2, 4)]
    out = [_case("band-%s" % n, "named", seed * 100003 + k, bands=nb, **kw) for n, k, nb, kw in rows]
    # (the refractory 64 -> 64 layer at TWO bands is 47680 floats a band: beyond the LDS, the refusal 'radio2-64to64-b2')
    return [c for c in out if band_count(c) > 0]


def _edge_cases(seed):
    rows = [("one-row-per-band", "bands = ph", 8, dict(c_in=3, c_out=40, h=8, w=8)),
            ("one-row-per-band-pool2", "bands = ph under pooling 2", 4, dict(c_in=3, c_out=24, h=8, w=8, pool_h=2, pool_w=2)),
            ("k1x1", "no halo at all", 3, dict(K1, c_in=5, c_out=40, h=6, w=7, rate=.3)),
            ("k2x5", "a halo of ONE row below", 3, dict(c_in=4, c_out=40, h=6, w=9, kh=2, kw=5, pad_h=1, pad_w=2)),
            ("pad0-shrinks", "no padding: the conv plane shrinks", 3, dict(c_in=3, c_out=36, h=12, w=9, kh=5, kw=4, pad_h=0, pad_w=0, rate=.3)),
            ("pad4-grows", "padding beyond the kernel: bands whose conv rows read only padding and hold no input row", 6,
             dict(c_in=2, c_out=40, h=5, w=6, pad_h=4, pad_w=4, rate=.3)),
            ("pool2-odd-ch", "pooling 2 on an odd ch: a trailing unpooled conv row, the last band's", 3,
             dict(c_in=4, c_out=40, h=7, w=8, pool_h=2, pool_w=2)),
            ("pool3", "pooling 3: the pooling's own padding at a band edge", 3, dict(c_in=4, c_out=40, h=10, w=11, pool_h=3, pool_w=3)),
            ("pw5", "pooled width 5: words shared by several bands", 4, dict(c_in=2, c_out=12, h=8, w=5)),
            ("pw11", "pooled width 11 (mnist_conv.yaml)", 3, dict(c_in=3, c_out=40, h=11, w=11)),
            ("pw13", "pooled width 13 (mnist_conv.yaml)", 4, dict(c_in=2, c_out=20, h=26, w=26, pool_h=2, pool_w=2, kh=3, kw=3)),
            ("pw33", "pooled width 33: a boundary word shared by two bands, a last word of one pixel row end", 3,
             dict(c_in=2, c_out=34, h=6, w=33, rate=.1)),
            ("pw5-three-bands-a-word", "one word shared by THREE bands and more", 6, dict(c_in=2, c_out=33, h=6, w=5)),
            ("pw32", "pooled width 32: no shared word, no zero fill — every word is stored over the caller's 0xFFFFFFFF", 3,
             dict(c_in=2, c_out=34, h=6, w=32, rate=.1)),
            ("cin3", "odd c_in: the last channel pairs its taps", 2, dict(c_in=3, c_out=40, h=6, w=7)),
            ("cin5-mt1", "odd c_in, one M tile", 2, dict(c_in=5, c_out=20, h=6, w=7, kh=2, kw=3)),
            ("cout1", "", 2, dict(c_in=4, c_out=1, h=9, w=9, refractory=0)),
            ("cout32", "every MFMA row of the one tile is a channel", 2, dict(c_in=4, c_out=32, h=7, w=9)),
            ("cout33", "one real row in tile 1", 2, dict(c_in=4, c_out=33, h=7, w=9)),
            ("cout64", "every MFMA row of both tiles is a channel", 2, dict(c_in=5, c_out=64, h=7, w=9, pool_h=2, pool_w=1)),
            ("band-below-32px", "a band of fewer than 32 conv pixels", 3, dict(c_in=4, c_out=40, h=6, w=5)),
            ("nobias-carry", "bias = None; two calls on one set of state buffers", 2, dict(c_in=4, c_out=40, h=6, w=6, bias=0, Ts=(3, 2))),
            ("B3-T1", "", 2, dict(c_in=4, c_out=40, h=6, w=6, B=3, Ts=(1,)))]
    # bands with 1, 2, 7, 8, 9 pixel tiles at MT 1 and 2: both sides of the work-split switch (8 tiles); w = 32: a row is a tile
    for m, co in ((1, 24), (2, 40)):
        for nt in (1, 2, 7, 8, 9):
            rows.append(("tiles%d-mt%d" % (nt, m), "%d tiles per band" % nt, 2, dict(c_in=2, c_out=co, h=2 * nt, w=32, rate=.1, Ts=(2,), B=1)))
    return [_case("band-edge-%s" % n, "edges", seed * 100003 + 200 + i, bands=nb, note=note, **kw) for i, (n, note, nb, kw) in enumerate(rows)]


# an explicit band count at the 160 KiB limit: 16x16, 3x3 pad 1, c_out 64, pooling 2, plain, 2 bands: the larger band (the first:
# 8 conv rows, 9 held rows) is 180 c_in + 144 c_in + 64 * 128 + 4 c_in + 64 = 328 c_in + 8256 floats <= 40960: c_in <= 99
LDS_EDGE = dict(c_out=64, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1)
# whole weights in LDS: 6x6, 3x3 pad 1, c_out 40, plain, 2 bands: a band (3 conv rows, 4 held rows) is 40 c_in + 24 c_in + 720 +
# 4 c_in + 64 = 68 c_in + 784 floats in front of 576 c_in of weights: 644 c_in + 784 <= 40960: c_in <= 62
WLDS_EDGE = dict(c_out=40, h=6, w=6, refractory=0, rate=.1)
# beyond dcll_conv_lif_sequence_wide: a pooling layer (no register form), 16x16, 3x3 pad 1, c_out 32: 584 c_in + 8224 > 40960
RULE_EDGE = dict(c_in=60, c_out=32, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1, Ts=(2,), B_checked=2)
# beyond it without pooling: c_in h w > 18432 (no register form), 3x3 pad 1, c_out 8
RULE_TILE = dict(c_in=40, c_out=8, h=32, rate=.1, Ts=(1,), B=2)
# served by the one-workgroup kernels: 3x3 pad 1 on h x 32, a row is a pixel tile
RULE_CPW = dict(c_in=2, c_out=24, w=32, rate=.1, Ts=(2,), B=2)


def _boundary_cases(seed):
    rows = [("lds-cin99", "40728 floats of 40960: the last c_in that fits two bands", 2, dict(LDS_EDGE, c_in=99, Ts=(1,), B=1)),
            ("wlds-cin62", "40712 floats with all the weights", 2, dict(WLDS_EDGE, c_in=62, Ts=(2,))),
            ("wlds-cin64", "one channel pair more: the weights are streamed", 2, dict(WLDS_EDGE, c_in=64, Ts=(2,))),
            ("rule-wide-serves", "bands = 0 on a layer the one-workgroup kernel serves with one chain per wave: one band", 0,
             dict(RULE_EDGE, c_in=56, B=2)),
            ("rule-wide-refuses", "one channel pair beyond it: the rule bands, down to one pixel tile", 0, dict(RULE_EDGE, c_in=58, B=2)),
            ("rule-b64", "B n = 256 at n = 4: still one round of the card", 0, dict(RULE_EDGE, B=64)),
            ("rule-b65", "B n = 260 at n = 4: the rule stays at 3", 0, dict(RULE_EDGE, B=65)),
            ("rule-b256", "a layer of several chains per wave at B = 256: two bands would be a second round", 0, dict(RULE_CPW, h=9, B=256, B_checked=2)),
            ("rule-cpw-t8", "8 pixel tiles, one M tile: one chain per wave in the one-workgroup kernel — one band", 0, dict(RULE_CPW, h=8)),
            ("rule-cpw-t9", "9 pixel tiles: a wave with two chains — the rule bands", 0, dict(RULE_CPW, h=9)),
            ("rule-cpw-mt2", "8 pixel tiles, two M tiles: two chains per wave — the rule bands", 0, dict(RULE_CPW, h=8, c_out=40)),
            ("rule-tile-w16", "two rows of 16 are one pixel tile: the rule stops at ph / 2", 0, dict(RULE_TILE, w=16)),
            ("rule-tile-w17", "two rows of 17 are two tiles: the rule goes on to one row per band", 0, dict(RULE_TILE, w=17))]
    return [_case("band-bound-%s" % n, "boundaries", seed * 100003 + 300 + i, bands=nb, note=note, **kw) for i, (n, note, nb, kw) in enumerate(rows)]


def _grid_cases(seed):
    return [_case("band-grid-b300x4", "grid", seed * 100003 + 400, bands=4, c_in=4, c_out=40, h=8, w=8, Ts=(3, 2), B=300, B_checked=8)]


def _forwarded_cases(seed):
    rows = [("b1-wide", 1, dict(c_in=4, c_out=40, h=6, w=10)), ("b1-any", 1, dict(c_in=3, c_out=9, h=9, w=7, refractory=0)),
            ("b1-regs", 1, dict(c_in=60, c_out=40, h=16, w=16, rate=.1, Ts=(2,), B=1)),
            ("b0-wide", 0, dict(c_in=4, c_out=64, h=6, w=10, B=200, B_checked=2)), ("b0-any-pool", 0, dict(c_in=5, c_out=24, h=7, w=9, pool_h=2, pool_w=3))]
    return [_case("band-fwd-%s" % n, "forwarded", seed * 100003 + 500 + i, bands=nb, **kw) for i, (n, nb, kw) in enumerate(rows)]


N_FREE = 60


def _free_draw(rng, k, seed):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(1, 65)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(3, 41)), w=int(rng.randint(3, 41)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(A.RATES[rng.randint(3)]), B=int(rng.randint(1, 4)), state0=1)
        ncall = (1, 1, 2)[rng.randint(3)]
        c["Ts"] = tuple(int(rng.randint(1, 5)) for _ in range(ncall))
        if ncall == 1 and rng.rand() < .3:
            c["state0"] = 0
        u = rng.rand()
        cc = _case("band-free-%03d" % k, "free", seed * 100003 + 1000 + k, bands=1, **c)
        if not valid(cc):
            continue
        cc["bands"] = 1 + int(u * out_shape(cc)[2])         # uniform over 1 .. ph
        if band_count(cc) == 0:
            continue
        if not cc["bias"] and any(b["I"][0] == b["I"][1] for b in plan(cc, cc["bands"])):
            continue        # (a band that reads only padding, without a bias: v = arp <= 0 for every draw — never sound)
        per = work(dict(cc, B_checked=1, Ts=[1]))
        if per * len(cc["Ts"]) > WORK_FREE_MAX:
            continue
        while work(cc) > WORK_FREE_MAX:             # shorten the calls, then thin the batch
            if max(cc["Ts"]) > 1:
                cc["Ts"] = [max(1, t // 2) for t in cc["Ts"]]
            else:
                cc["B"] = cc["B_checked"] = max(1, cc["B"] // 2)
        return cc


def cases(seed=SEED):
    """every case that runs (the refusals: refusals())"""
    rng = np.random.RandomState(seed)
    return (_named(seed) + _edge_cases(seed) + _boundary_cases(seed) + _grid_cases(seed) + _forwarded_cases(seed) +
            [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("cout65", dict(c_out=65), U, "c_out <= 64"), ("stride2", dict(stride=2), U, "plain convolutions only"),
            ("dilation2", dict(dilation=2), U, "plain convolutions only"), ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("bands-above-ph", dict(bands=9), U, "bands > ph"),
            ("bands-above-ph-pool", dict(pool_h=2, pool_w=2, bands=5), U, "bands > ph"),
            ("lds-cin100", dict(LDS_EDGE, c_in=100, bands=2), U, "exceeds the 160 KiB of LDS at this band count"),
            ("radio2-64to64-b2", dict(K7P3, c_in=64, c_out=64, h=16, w=16, bands=2), U, "exceeds the 160 KiB of LDS at this band count"),
            ("b1-wide-refuses", dict(LDS_EDGE, c_in=100, bands=1), U, "exceeds the 160 KiB of LDS"),
            ("no-count-fits", dict(c_in=40, c_out=64, h=4, w=1000, bands=0), U, "no band count"),
            ("bands-negative", dict(bands=-1), I, "negative band count"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"),
            ("null-spk-in", dict(null="spk_in"), I, "null pointer"), ("null-eps0", dict(null="eps0"), I, "null pointer"),
            ("null-W", dict(null="W"), I, "null pointer"), ("null-tau4", dict(null="tau4"), I, "null pointer"),
            ("null-scratch", dict(null="scratch"), I, "null pointer"),
            ("T-negative", dict(T=-1), I, "negative T or B"), ("B-negative", dict(B=-2), I, "negative T or B"),
            ("T0", dict(T=0), "DCLL_OK", ""), ("B0", dict(B=0), "DCLL_OK", ""), ("T0-unsupported", dict(T=0, c_out=65), "DCLL_OK", "")]
    base = dict(DEFAULT, null=None, T=3, B=2)
    del base["Ts"], base["B_checked"], base["rate"], base["state0"]
    return [dict(base, id="band-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


def by_id(cid):
    for c in cases() + refusals():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def band_rows_of(c):
    """the conv rows of each band the case runs (one band: the whole plane)"""
    n = band_count(c)
    return [b["C"] for b in plan(c, n)] if n > 1 else [(0, out_shape(c)[0])]


def unsound(c, traj):
    """seq_wide_cases.unsound (the share of spikes, arp, both 32-row groups of channels), and for the bands: EVERY band has spikes
    and non-spikes over the case — a kernel that dropped or duplicated a band cannot pass"""
    why = W.unsound(c, traj)
    if why is not None:
        return why
    for k, (C0, C1) in enumerate(band_rows_of(c)):
        s = np.concatenate([call["v"][:, :, :, C0:C1].ravel() for call in traj]) > 0
        if s.all() or not s.any():
            return "band %d (conv rows %d..%d): every v on one side of the threshold" % (k, C0, C1)
    return None


_RUNS = {}


def _draw_key(c):
    return json.dumps({k: v for k, v in c.items() if k not in ("id", "bands", "note", "stratum", "B")}, sort_keys=True)


def run(c, max_attempts=24):
    """(tensors, oracle trajectory) of a case: the first attempt that is sound (deterministic in the sub-seed); computed once per
    process and shared — also among the cases that differ in their band count alone — the callers leave both unchanged"""
    key = (_draw_key(c), tuple(band_rows_of(c)))
    if key in _RUNS:
        return _RUNS[key]
    why = None
    for attempt in range(max_attempts):
        hit = _RUNS.get((_draw_key(c), "attempt", attempt))
        if hit is None:
            T = A._draw(c, attempt)
            T["attempt"] = attempt
            hit = _RUNS[(_draw_key(c), "attempt", attempt)] = (T, A._trajectory(c, T))
        why = unsound(c, hit[1])
        if why is None:
            _RUNS[key] = hit
            return hit
    raise AssertionError("%s: no sound draw in %d attempts (%s)" % (c["id"], max_attempts, why))


# ---------------------------------------------------------------------------------------------------------------------------
# the banded oracle: the C oracle per band on the cropped rows, stitched — the decomposition without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_band(c, v, band):
    """max pooling of the band's conv rows v (..., C1 - C0, cw) -> its pooled rows (..., P1 - P0, pw); every window row lies
    inside the band"""
    ch, cw, ph, pw = out_shape(c)
    (P0, P1), (C0, C1) = band["P"], band["C"]
    pph, ppw = (c["pool_h"] - 1) // 2, (c["pool_w"] - 1) // 2
    out = np.full(v.shape[:-2] + (P1 - P0, pw), -np.inf, np.float32)
    for py in range(P0, P1):
        ys = [y for y in range(py * c["pool_h"] - pph, py * c["pool_h"] - pph + c["pool_h"]) if 0 <= y < ch]
        assert ys and C0 <= ys[0] and ys[-1] < C1, (c["id"], py, ys, band)
        for px in range(pw):
            xs = [x for x in range(px * c["pool_w"] - ppw, px * c["pool_w"] - ppw + c["pool_w"]) if 0 <= x < cw]
            out[..., py - P0, px] = v[..., ys[0] - C0:ys[-1] + 1 - C0, xs[0]:xs[-1] + 1].max(axis=(-2, -1))
    return out


def banded_trajectory(c, T, mutant=None):
    """the trajectory of seq_any_cases._trajectory computed band by band: per band the C oracle on the rows the band holds (its own
    zero rows above and below in place of pad_h, the cropped initial state), v / arp of its conv rows, the final eps0 / eps1 of
    the rows it owns, its pooled spikes packed into the shared words.  -> per call dict(v, s, words, eps0, eps1, arp).
    mutant: 'short-halo' (a band with rows below its own holds one row less), 'live-halo' (the initial state of a band is read
    from the state the bands before it — the later ones run first — have written back), 'store-word' (a boundary word is stored,
    not ORed)."""
    n = max(band_count(c), 1)
    bands = plan(c, n)
    ch, cw, ph, pw = out_shape(c)
    Bc, cin, h, w, kh, pad = c["B_checked"], c["c_in"], c["h"], c["w"], c["kh"], c["pad_h"]
    state = dict(eps0=T["eps0"].copy(), eps1=T["eps1"].copy(), arp=T["arp"].copy())
    out = []
    order = list(range(n))[::-1] if mutant == "live-halo" else list(range(n))
    for call in T["calls"]:
        x = call["x"]
        nt = x.shape[0]
        snap = state if mutant == "live-halo" else {k: a.copy() for k, a in state.items()}
        res = dict(v=np.empty((nt, Bc, c["c_out"], ch, cw), np.float32), s=np.zeros((nt, Bc, c["c_out"], ph, pw), np.float32),
                   words=np.zeros((nt, Bc, c["c_out"], (ph * pw + 31) // 32), np.uint32))
        for k in order:
            b = bands[k]
            (C0, C1), (I0, I1), (O0, O1) = b["C"], b["I"], b["O"]
            if mutant == "short-halo" and I1 > O1:
                I1 -= 1
            RB, top, HB = C1 - C0 + kh - 1, I0 + pad - C0, I1 - I0
            cb = dict(c, h=RB, pad_h=0, pool_h=1, pool_w=1)
            orc = A._oracle(cb, T["W"], T["b"], T["tau"], 1.0 if c["refractory"] else 0.0)
            st = [np.zeros((Bc, cin, RB, w), np.float32), np.zeros((Bc, cin, RB, w), np.float32),
                  np.ascontiguousarray(snap["arp"][:, :, C0:C1])]
            st[0][:, :, top:top + HB] = snap["eps0"][:, :, I0:I1]
            st[1][:, :, top:top + HB] = snap["eps1"][:, :, I0:I1]
            orc.state = st
            for t in range(nt):
                xb = np.zeros((Bc, cin, RB, w), np.float32)
                xb[:, :, top:top + HB] = x[t][:, :, I0:I1]
                v = orc.forward(xb)[3]
                res["v"][t][:, :, C0:C1] = v
                pooled = _pool_band(c, v, b)
                res["s"][t][:, :, b["P"][0]:b["P"][1]] = pooled > 0
                dense = np.zeros((Bc, c["c_out"], ph * pw), np.float32)
                lo, hi = b["P"][0] * pw, b["P"][1] * pw
                dense[:, :, lo:hi] = (pooled > 0).reshape(Bc, c["c_out"], -1)
                mine = pack_planes(dense)
                for wi in range(lo // 32, (hi + 31) // 32):
                    inside = wi * 32 >= lo and min(wi * 32 + 32, ph * pw) <= hi
                    if inside or mutant == "store-word":
                        res["words"][t][:, :, wi] = mine[:, :, wi]
                    else:
                        res["words"][t][:, :, wi] |= mine[:, :, wi]
            assert not orc.state[0][:, :, :top].any() and not orc.state[1][:, :, top + HB:].any()      # the zero rows stay zero
            O1 = min(O1, I1) if mutant == "short-halo" else O1
            state["eps0"][:, :, O0:O1] = orc.state[0][:, :, top + O0 - I0:top + O1 - I0]
            state["eps1"][:, :, O0:O1] = orc.state[1][:, :, top + O0 - I0:top + O1 - I0]
            state["arp"][:, :, C0:C1] = orc.state[2]
        res.update({k: a.copy() for k, a in state.items()})
        out.append(res)
    return out
