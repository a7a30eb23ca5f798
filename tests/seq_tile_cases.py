"""Seeded cases for dcll_conv_lif_sequence_tiles (k_lif_seq_tile: the fused all-T kernel of a plain conv layer with a 2-D grid of
workgroups per sample, each on a tile of the output plane), their tensors and the C oracle's trajectories — in the style of
tests/seq_band_cases.py; the case format, the tensor draws and the oracle stepping are tests/seq_any_cases.py's.  Plain module: no
GPU, no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_seq_tile_cases.py proves the lists on the CPU;
tests/test_gpu_seq_tile.py runs the HIP kernel against them.  Re-run one alone:
    python -c "import seq_tile_cases as S; print(S.describe(S.by_id('tile-radio2-8x64-64to64')))"

A case is seq_any_cases' dict plus `tiles` = [ty, tx] ([0, 0]: the library's rule, [n, 1]: n bands, else exactly that plan).
Restated ONCE here, from csrc/dcll_seq_tile.hip: the tile plan (axis_plan(), tile_plan()), the LDS of a tile (tile_floats(),
lds_bytes()), the scratch (scratch_floats()), the (0, 0) rule (tile_rule()), the template instance and the launch log (variant(),
launch_log()), the shared spike words (shared_words()).

Strata:
  named       radio_ml_conv.yaml at netscale 2 on 8x64 (64 -> 64 refractory and plain: no band count fits, the rule tiles; 1 -> 64:
              the rule returns a band plan); mnist_conv.yaml's three layers at netscale 1 and 2 at (2, 2); a 32 -> 32 7x7 layer on
              12x40 at (2, 2) and (1, 3) — the last nine are served by bands too: the cross-check;
  edges       the smallest shapes at which the tiling can go wrong (see the notes of the rows);
  boundaries  both sides of the 160 KiB limit for an explicit plan, of whole-weights-in-LDS, of every branch of the (0, 0) rule (the
              far side of the first and 'no plan fits': refusals());
  grid        B = 300 x (2, 2) from 8 distinct samples (1200 workgroups: beyond residency), TWO consecutive calls;
  forwarded   tiles_x = 1: dcll_conv_lif_sequence_bands' launch log;
  free        uniform draws: c_in 1-40, c_out 1-64, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, h, w 3-40, plans up to (ph, pw);
  refuse      error returns before any launch (refusals())."""
import json

import numpy as np

import seq_any_cases as A
import seq_band_cases as S
import seq_wide_cases as W

ALPHARP = A.ALPHARP
SEED = 20423
WORK_FREE_MAX = A.WORK_FREE_MAX
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
THREADS, NW = 512, 8
MAX_K, MAX_COUT = 16, 64
CUS = 256
GRID_MAX = 0x7fffffff

DEFAULT = dict(A.DEFAULT, c_in=2, c_out=40, h=8, w=8, tiles=[2, 2])
out_shape, valid, work, cases_hash = A.out_shape, A.valid, A.work, A.cases_hash
pack_planes, unpack_planes = A.pack_planes, A.unpack_planes
steps = A.steps


def describe(c):
    return json.dumps(c, sort_keys=True)


def _case(cid, stratum, seed, tiles=(2, 2), **kw):
    c = A._case(cid, stratum, seed, **dict(dict(c_in=DEFAULT["c_in"], c_out=DEFAULT["c_out"], h=DEFAULT["h"], w=DEFAULT["w"]), **kw))
    c["tiles"] = [int(tiles[0]), int(tiles[1])]
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the tile plan, the LDS, the rule, the dispatch — restated
# ---------------------------------------------------------------------------------------------------------------------------
def mt(c):
    return (c["c_out"] + 31) // 32


def axis_plan(n, size, k, pad, pool, conv, pooled):
    """one direction cut into n parts: dicts P (pooled pixels), C (conv pixels), I (input pixels held), O (input pixels owned), each
    a half-open (lo, hi)"""
    pp = (pool - 1) // 2
    clip = lambda y: min(max(y, 0), size)
    first = lambda P: max(P * pool - pp, 0)             # first conv pixel of pooled pixel P's window
    out = []
    for i in range(n):
        P0, P1 = i * pooled // n, (i + 1) * pooled // n
        C0, C1 = first(P0), (conv if i == n - 1 else first(P1))
        I0, I1 = clip(C0 - pad), clip(C1 - pad + k - 1)
        O1 = size if i == n - 1 else clip(C1 - pad)
        out.append(dict(P=(P0, P1), C=(C0, C1), I=(I0, I1), O=(I0, O1)))
    return out


def tile_plan(c, ny, nx):
    """(the ny row parts, the nx column parts): tile (a, b) is rows[a] x cols[b]"""
    ch, cw, ph, pw = out_shape(c)
    return (axis_plan(ny, c["h"], c["kh"], c["pad_h"], c["pool_h"], ch, ph),
            axis_plan(nx, c["w"], c["kw"], c["pad_w"], c["pool_w"], cw, pw))


def _len(r):
    return r[1] - r[0]


def tile_floats(c, ry, rx):
    """the working set of one tile in floats, without the weights"""
    CR, CC, HR, HC = _len(ry["C"]), _len(rx["C"]), _len(ry["I"]), _len(rx["I"])
    img = c["c_in"] * (CR + c["kh"] - 1) * (CC + c["kw"] - 1)
    e0 = c["c_in"] * HR * HC
    vpl = c["c_out"] * CR * CC
    return img + e0 + vpl * (2 if c["refractory"] else 1) + 4 * c["c_in"] + 32 * mt(c)


def floats_max(c, ny, nx):
    rows, cols = tile_plan(c, ny, nx)
    ys = {(r["C"][1] - r["C"][0], r["I"][1] - r["I"][0]): r for r in rows}.values()
    xs = {(r["C"][1] - r["C"][0], r["I"][1] - r["I"][0]): r for r in cols}.values()
    return max(tile_floats(c, y, x) for y in ys for x in xs)


def held_sum(c, ny, nx):
    rows, cols = tile_plan(c, ny, nx)
    return sum(_len(r["I"]) for r in rows) * sum(_len(r["I"]) for r in cols)


def _layer_ok(c):
    return valid(c) and (c["stride"], c["dilation"], c["groups"]) == (1, 1, 1) and c["c_out"] <= MAX_COUT and max(c["kh"], c["kw"]) <= MAX_K


def fits(c, ny, nx):
    return floats_max(c, ny, nx) * 4 <= LDS_MAX


def tile_rule(c):
    """the (0, 0) rule where no band count serves: the fitting (ny, nx), nx >= 2, with the fewest tiles; ties to the smallest sum
    of held input elements over all tiles, then to the smaller nx (derived from the LDS formula alone); None: no plan fits"""
    ph, pw = out_shape(c)[2:]
    for n in range(2, ph * pw + 1):
        best = None
        for nx in range(2, min(pw, n) + 1):
            if n % nx or n // nx > ph or not fits(c, n // nx, nx):
                continue
            held = held_sum(c, n // nx, nx)
            if best is None or held < best[0]:
                best = (held, n // nx, nx)
        if best:
            return best[1], best[2]
    return None


def tile_count(c, B=None, tiles=None):
    """dcll_conv_lif_sequence_tiles_plan: (NY, NX) the call runs, None = refused.  NX == 1: a band plan, the call is
    dcll_conv_lif_sequence_bands'"""
    B = c.get("B", 1) if B is None else B
    ty, tx = c["tiles"] if tiles is None else tiles
    if not _layer_ok(c) or ty < 0 or tx < 0:
        return None
    ph, pw = out_shape(c)[2:]
    if tx == 1 or (ty, tx) == (0, 0):
        n = S.band_count(c, B, ty)
        if n or tx == 1:
            return (n, 1) if n else None
        return tile_rule(c)
    if ty == 0 or tx == 0 or ty > ph or tx > pw or not fits(c, ty, tx):
        return None
    return ty, tx


def lds_bytes(c, tiles=None):
    """dcll_conv_lif_sequence_tiles_lds: the largest tile's bytes ((0, 0): at the rule's plan for B = 1; a band plan:
    dcll_conv_lif_sequence_bands_lds), 0 = refused"""
    n = tile_count(c, 1, tiles)
    if n is None:
        return 0
    return S.lds_bytes(c, n[0]) if n[1] == 1 else 4 * floats_max(c, *n)


def scratch_floats(c, B=None):
    """dcll_conv_lif_sequence_tiles_scratch: the permuted weights + the snapshot of eps0 / eps1"""
    B = c["B"] if B is None else B
    if B < 0 or tile_count(c, B, (0, 0)) is None:
        return 0
    return 64 * mt(c) * steps(c) + 2 * B * c["c_in"] * c["h"] * c["w"]


def whole_weights(c, ny, nx):
    return (floats_max(c, ny, nx) + steps(c) * 64 * mt(c)) * 4 <= LDS_MAX


def _as_band(c, n):
    return dict(c, bands=n)


def variant(c):
    """the template instance a case runs: 'k_lif_seq_tile<MT,R,WLDS>', or the band path's for one column of tiles"""
    n = tile_count(c)
    assert n is not None, c["id"]
    if n[1] == 1:
        return S.variant(_as_band(c, n[0]))
    return "k_lif_seq_tile<%d,%d,%d>" % (mt(c), c["refractory"], int(whole_weights(c, *n)))


def launch_log(c):
    """the launch log of one call (the weight permutation, the snapshot and the zero fill are not logged; a band plan: the band
    path's)"""
    n = tile_count(c)
    return S.launch_log(_as_band(c, n[0])) if n[1] == 1 else [variant(c)]


def all_variants():
    return ["k_lif_seq_tile<%d,%d,%d>" % (m, r, l) for m in (1, 2) for r in (0, 1) for l in (1, 0)]


def segments(c, ny, nx):
    """per tile (a, b): the half-open ranges of flattened pooled pixels it owns, one per pooled row"""
    pw = out_shape(c)[3]
    rows, cols = tile_plan(c, ny, nx)
    return {(a, b): [(py * pw + rx["P"][0], py * pw + rx["P"][1]) for py in range(*ry["P"])]
            for a, ry in enumerate(rows) for b, rx in enumerate(cols)}


def shared_words(c, ny, nx):
    """the segment starts that fall inside a spike word: the launcher zero-fills spk_out when any"""
    return sorted(s0 for segs in segments(c, ny, nx).values() for s0, _ in segs if s0 % 32)


def tiles_max(c, ny, nx):
    """pixel tiles (32 conv pixels) of the largest tile"""
    rows, cols = tile_plan(c, ny, nx)
    return max((_len(y["C"]) * _len(x["C"]) + 31) // 32 for y in rows for x in cols)


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P2, K7P3, K1 = A.K7P2, A.K7P3, W.K1
RADIO2_8x64 = dict(K7P3, c_in=64, c_out=64, h=8, w=64, tau_tensor=1, Ts=(2,), B=1, rate=.1)
R32_12x40 = dict(K7P3, c_in=32, c_out=32, h=12, w=40, tau_tensor=1, Ts=(2,), B=2, rate=.1)


def _named(seed):
    rows = [("radio2-8x64-64to64", 0, (0, 0), RADIO2_8x64), ("radio2-8x64-64to64-plain", 1, (0, 0), dict(RADIO2_8x64, refractory=0)),
            ("radio2-8x64-1to64", 2, (0, 0), dict(RADIO2_8x64, c_in=1, B=2, rate=.02)),
            ("r32-12x40-t2x2", 3, (2, 2), R32_12x40), ("r32-12x40-t1x3", 3, (1, 3), R32_12x40)]
    for s, scale in ((1, 1), (2, 2)):
        for i, g in enumerate(A.MNIST):
            kw = dict(g, c_in=g["c_in"] * (scale if i else 1), c_out=g["c_out"] * scale, refractory=0, tau_tensor=1, Ts=(2,), B=2,
                      rate=A.RATES[i])
            rows.append(("mnist%d-l%d-t2x2" % (s, i + 1), 20 + 3 * s + i, (2, 2), kw))
    return [_case("tile-%s" % n, "named", seed * 100003 + k, tiles=t, **kw) for n, k, t, kw in rows]


def _edge_cases(seed):
    rows = [("one-pixel-per-tile", "NY = ph, NX = pw", (5, 6), dict(c_in=3, c_out=40, h=5, w=6)),
            ("one-pixel-per-tile-pool2", "NY = ph, NX = pw under pooling 2", (4, 4), dict(c_in=3, c_out=24, h=8, w=8, pool_h=2, pool_w=2)),
            ("k1x1", "no halo at all", (2, 3), dict(K1, c_in=5, c_out=40, h=9, w=11, rate=.3)),
            ("k2x5", "a halo of ONE row, of four columns: a swapped halo reads outside what is held", (3, 2),
             dict(c_in=4, c_out=40, h=9, w=11, kh=2, kw=5, pad_h=1, pad_w=2)),
            ("k5x2", "a halo of four rows, of ONE column", (2, 3), dict(c_in=4, c_out=40, h=9, w=11, kh=5, kw=2, pad_h=2, pad_w=1)),
            ("pad0-shrinks", "no padding: the conv plane shrinks", (2, 2), dict(c_in=3, c_out=36, h=12, w=9, kh=5, kw=4, pad_h=0, pad_w=0, rate=.3)),
            ("pad4-grows", "padding beyond the kernel: tiles that hold no input row or no input column", (6, 6),
             dict(c_in=2, c_out=40, h=5, w=6, pad_h=4, pad_w=4, rate=.3)),
            ("pool2-odd", "pooling 2 on an odd ch and an odd cw: trailing unpooled conv pixels, the last tiles'", (2, 2),
             dict(c_in=4, c_out=40, h=7, w=9, pool_h=2, pool_w=2)),
            ("pool3", "pooling 3: the pooling's own padding at a tile edge", (2, 2), dict(c_in=4, c_out=40, h=10, w=11, pool_h=3, pool_w=3)),
            ("pool1x2", "pooling (1, 2)", (2, 2), dict(c_in=4, c_out=40, h=9, w=11, pool_h=1, pool_w=2)),
            ("pool2x1", "pooling (2, 1)", (2, 2), dict(c_in=4, c_out=40, h=9, w=11, pool_h=2, pool_w=1)),
            ("pw5", "pooled width 5: words shared by many segments", (2, 2), dict(c_in=2, c_out=12, h=8, w=5)),
            ("pw11", "pooled width 11 (mnist_conv.yaml)", (2, 3), dict(c_in=3, c_out=40, h=11, w=11)),
            ("pw13", "pooled width 13 (mnist_conv.yaml)", (2, 3), dict(c_in=2, c_out=20, h=26, w=26, pool_h=2, pool_w=2, kh=3, kw=3)),
            ("pw32", "pooled width 32: every segment of the second column starts inside a word", (2, 2), dict(c_in=2, c_out=34, h=4, w=32, rate=.1)),
            ("pw33", "pooled width 33", (2, 2), dict(c_in=2, c_out=34, h=4, w=33, rate=.1)),
            ("pw64-no-shared-word", "pooled width 64 in two columns: every segment is one whole word — no zero fill, every word "
             "stored over the caller's 0xFFFFFFFF", (3, 2), dict(c_in=2, c_out=34, h=3, w=64, rate=.1)),
            ("cin3", "odd c_in: the last channel pairs its taps", (2, 2), dict(c_in=3, c_out=40, h=6, w=7)),
            ("cin5-mt1", "odd c_in, one M tile", (2, 2), dict(c_in=5, c_out=20, h=6, w=7, kh=2, kw=3)),
            ("cout1", "", (2, 2), dict(c_in=4, c_out=1, h=9, w=9, refractory=0)),
            ("cout32", "every MFMA row of the one tile is a channel", (2, 2), dict(c_in=4, c_out=32, h=7, w=9)),
            ("cout33", "one real row in tile 1", (2, 2), dict(c_in=4, c_out=33, h=7, w=9)),
            ("cout64", "every MFMA row of both tiles is a channel", (2, 2), dict(c_in=5, c_out=64, h=7, w=9, pool_h=2, pool_w=1)),
            ("tile-below-32px", "tiles of fewer than 32 conv pixels", (2, 2), dict(c_in=4, c_out=40, h=6, w=5)),
            ("nobias-carry", "bias = None; two calls on one set of state buffers", (2, 2), dict(c_in=4, c_out=40, h=6, w=6, bias=0, Ts=(3, 2))),
            ("B3-T1", "", (2, 2), dict(c_in=4, c_out=40, h=6, w=6, B=3, Ts=(1,)))]
    # tiles with 1, 2, 7, 8, 9 pixel tiles at MT 1 and 2: both sides of the work-split switch (8 pixel tiles); w = 64 in two
    # columns: a tile's row is a pixel tile
    for m, co in ((1, 24), (2, 40)):
        for nt in (1, 2, 7, 8, 9):
            rows.append(("tiles%d-mt%d" % (nt, m), "%d pixel tiles per tile" % nt, (2, 2),
                         dict(c_in=2, c_out=co, h=2 * nt, w=64, rate=.1, Ts=(2,), B=1)))
    return [_case("tile-edge-%s" % n, "edges", seed * 100003 + 200 + i, tiles=t, note=note, **kw) for i, (n, note, t, kw) in enumerate(rows)]


# an explicit plan at the 160 KiB limit: 16x16, 3x3 pad 1, c_out 64, pooling 2, plain, (2, 2): a tile (8 x 8 conv pixels, 10 x 10
# of img, 9 x 9 held) is 100 c_in + 81 c_in + 64 * 64 + 4 c_in + 64 = 185 c_in + 4160 floats <= 40960: c_in <= 198
LDS_EDGE = dict(c_out=64, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1)
# whole weights in LDS: 6x6, 3x3 pad 1, c_out 40, plain, (2, 2): a tile (3 x 3 conv pixels, 5 x 5 of img, 4 x 4 held) is
# 25 c_in + 16 c_in + 360 + 4 c_in + 64 = 45 c_in + 424 floats in front of 576 c_in of weights: 621 c_in + 424 <= 40960: c_in <= 65
WLDS_EDGE = dict(c_out=40, h=6, w=6, refractory=0, rate=.1)
# the (0, 0) rule.  No band count fits where ONE pooled row is beyond the LDS.  1x1 kernel, c_in 40, c_out 64, plain, w = 300: a row
# is 300 (2 x 40 + 64) = 43200 floats; two tiles of h = 1 fit; at h = 2 two do not (150 x 2 x 144) and three do
RULE_ROW = dict(K1, c_in=40, c_out=64, w=300, refractory=0, rate=.3, Ts=(1,), B=1)
# ties at four tiles on two rows of 600: 1x1 kernel, c_in 20, c_out 64 (104 floats a pixel, 392 pixels a tile): (1, 2) and (1, 3)
# do not fit, (2, 2) and (1, 4) both hold 300 pixels and — no halo — the same 1200 input elements: the smaller NX wins
RULE_TIE_NX = dict(K1, c_in=20, c_out=64, h=2, w=600, refractory=0, rate=.3, Ts=(1,), B=1)
# ... and on two rows of 496 under a 3x1 kernel (pad (1, 0)): (2, 2) is 248 (5 x 20 + 64) + 144 = 40816 floats and holds both rows
# in both of its rows of tiles (1984 elements), (1, 4) holds every element once (992): the larger NX wins on the held sum
RULE_TIE_HELD = dict(c_in=20, c_out=64, h=2, w=496, kh=3, kw=1, pad_h=1, pad_w=0, refractory=0, rate=.3, Ts=(1,), B=1)


def _boundary_cases(seed):
    rows = [("lds-cin198", "40790 floats of 40960: the last c_in that fits (2, 2)", (2, 2), dict(LDS_EDGE, c_in=198, Ts=(1,), B=1)),
            ("wlds-cin64", "40168 floats with all the weights", (2, 2), dict(WLDS_EDGE, c_in=64, Ts=(2,))),
            ("wlds-cin66", "one channel pair more: the weights are streamed", (2, 2), dict(WLDS_EDGE, c_in=66, Ts=(2,))),
            ("rule-band-serves", "(0, 0) on a layer a band count serves: the band rule's plan", (0, 0),
             dict(c_in=60, c_out=32, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1, Ts=(2,), B=2)),
            ("rule-fewest-h1", "no band fits; two tiles fit: (1, 2)", (0, 0), dict(RULE_ROW, h=1)),
            ("rule-fewest-h2", "no band fits; two tiles do not fit, three do: (1, 3)", (0, 0), dict(RULE_ROW, h=2)),
            ("rule-tie-held", "two plans of four tiles fit: the smaller sum of held input elements wins, (1, 4)", (0, 0), RULE_TIE_HELD),
            ("rule-tie-nx", "two plans of four tiles fit with the same held sum: the smaller NX wins, (2, 2)", (0, 0), RULE_TIE_NX)]
    return [_case("tile-bound-%s" % n, "boundaries", seed * 100003 + 300 + i, tiles=t, note=note, **kw) for i, (n, note, t, kw) in enumerate(rows)]


def _grid_cases(seed):
    return [_case("tile-grid-b300-t2x2", "grid", seed * 100003 + 400, tiles=(2, 2), c_in=4, c_out=40, h=8, w=8, Ts=(3, 2), B=300, B_checked=8)]


def _forwarded_cases(seed):
    rows = [("t1x1-wide", (1, 1), dict(c_in=4, c_out=40, h=6, w=10)), ("t1x1-any", (1, 1), dict(c_in=3, c_out=9, h=9, w=7, refractory=0)),
            ("t2x1-band", (2, 1), dict(c_in=4, c_out=40, h=6, w=10)), ("t3x1-band-pool", (3, 1), dict(c_in=5, c_out=24, h=7, w=9, pool_h=2, pool_w=3)),
            ("t0x1-rule", (0, 1), dict(c_in=2, c_out=24, h=9, w=32, rate=.1, Ts=(2,), B=2)),
            ("t0x0-rule", (0, 0), dict(c_in=2, c_out=40, h=8, w=32, rate=.1, Ts=(2,), B=2))]
    return [_case("tile-fwd-%s" % n, "forwarded", seed * 100003 + 500 + i, tiles=t, **kw) for i, (n, t, kw) in enumerate(rows)]


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
        u, v, full = rng.rand(), rng.rand(), rng.rand() < .15
        cc = _case("tile-free-%03d" % k, "free", seed * 100003 + 1000 + k, tiles=(1, 2), **c)
        if not valid(cc):
            continue
        ph, pw = out_shape(cc)[2:]
        if pw < 2:
            continue
        if full and ph * pw <= 64:
            cc["tiles"] = [ph, pw]
        else:                                               # uniform over 1 .. min(ph, 6) x 2 .. min(pw, 8)
            cc["tiles"] = [1 + int(u * min(ph, 6)), 2 + int(v * (min(pw, 8) - 1))]
        if tile_count(cc) is None:
            continue
        rows, cols = tile_plan(cc, *cc["tiles"])
        if not cc["bias"] and any(_len(r["I"]) == 0 for r in rows + cols):
            continue        # (a tile that reads only padding, without a bias: v = arp <= 0 for every draw — never sound)
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
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error().
    B_call: the B handed to the call where it differs from the B the buffers are made for"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("cout65", dict(c_out=65), U, "c_out <= 64"), ("stride2", dict(stride=2), U, "plain convolutions only"),
            ("dilation2", dict(dilation=2), U, "plain convolutions only"), ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("ty-above-ph", dict(tiles=[9, 2]), U, "tiles_y > ph or tiles_x > pw"),
            ("tx-above-pw", dict(tiles=[2, 9]), U, "tiles_y > ph or tiles_x > pw"),
            ("tx-above-pw-pool", dict(pool_h=2, pool_w=2, tiles=[2, 5]), U, "tiles_y > ph or tiles_x > pw"),
            ("lds-cin199", dict(LDS_EDGE, c_in=199, tiles=[2, 2]), U, "exceeds the 160 KiB of LDS at this plan"),
            ("radio2-8x64-t1x4", dict(K7P3, c_in=64, c_out=64, h=8, w=64, tiles=[1, 4]), U, "exceeds the 160 KiB of LDS at this plan"),
            ("no-plan-fits", dict(c_in=100, c_out=8, h=16, w=17, kh=16, kw=16, pad_h=0, pad_w=0, tiles=[0, 0]), U, "no tile plan"),
            ("fwd-bands-above-ph", dict(tiles=[9, 1]), U, "bands > ph"),
            ("fwd-no-count-fits", dict(K7P3, c_in=64, c_out=64, h=8, w=64, tiles=[0, 1]), U, "no band count"),
            ("ty-negative", dict(tiles=[-1, 2]), I, "negative tile count"), ("tx-negative", dict(tiles=[2, -1]), I, "negative tile count"),
            ("ty0-alone", dict(tiles=[0, 2]), I, "0 in one direction only"), ("tx0-alone", dict(tiles=[2, 0]), I, "0 in one direction only"),
            ("grid-beyond", dict(B_call=2 ** 30), I, "beyond the grid"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"),
            ("null-spk-in", dict(null="spk_in"), I, "null pointer"), ("null-eps0", dict(null="eps0"), I, "null pointer"),
            ("null-W", dict(null="W"), I, "null pointer"), ("null-tau4", dict(null="tau4"), I, "null pointer"),
            ("null-scratch", dict(null="scratch"), I, "null pointer"),
            ("T-negative", dict(T=-1), I, "negative T or B"), ("B-negative", dict(B=-2), I, "negative T or B"),
            ("T0", dict(T=0), "DCLL_OK", ""), ("B0", dict(B=0), "DCLL_OK", ""), ("T0-unsupported", dict(T=0, c_out=65), "DCLL_OK", "")]
    base = dict(DEFAULT, null=None, T=3, B=2, B_call=None)
    del base["Ts"], base["B_checked"], base["rate"], base["state0"]
    return [dict(base, id="tile-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


def by_id(cid):
    for c in cases() + refusals():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def tile_boxes(c):
    """the conv pixels ((C0y, C1y), (C0x, C1x)) of each tile the case runs (a band plan: full rows)"""
    ny, nx = tile_count(c)
    rows, cols = tile_plan(c, max(ny, 1), nx)
    return [(y["C"], x["C"]) for y in rows for x in cols]


def unsound(c, traj):
    """seq_wide_cases.unsound (the share of spikes, arp, both 32-row groups of channels), and for the tiles: EVERY tile has spikes
    and non-spikes over the case — a kernel that dropped or duplicated a tile cannot pass"""
    why = W.unsound(c, traj)
    if why is not None:
        return why
    for k, ((y0, y1), (x0, x1)) in enumerate(tile_boxes(c)):
        s = np.concatenate([call["v"][:, :, :, y0:y1, x0:x1].ravel() for call in traj]) > 0
        if s.all() or not s.any():
            return "tile %d (conv rows %d..%d, columns %d..%d): every v on one side of the threshold" % (k, y0, y1, x0, x1)
    return None


_RUNS = {}


def _draw_key(c):
    return json.dumps({k: v for k, v in c.items() if k not in ("id", "tiles", "note", "stratum", "B")}, sort_keys=True)


def run(c, max_attempts=24):
    """(tensors, oracle trajectory) of a case: the first attempt that is sound (deterministic in the sub-seed); computed once per
    process and shared — also among the cases that differ in their plan alone — the callers leave both unchanged"""
    key = (_draw_key(c), tuple(tile_boxes(c)))
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
# the tiled oracle: the C oracle per tile on the cropped region, stitched — the decomposition without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _pool_tile(c, v, ry, rx):
    """max pooling of the tile's conv pixels v (..., CR, CC) -> its pooled pixels (..., P1y - P0y, P1x - P0x); every window pixel
    inside the conv plane lies inside the tile"""
    ch, cw, ph, pw = out_shape(c)
    (P0y, P1y), (C0y, C1y), (P0x, P1x), (C0x, C1x) = ry["P"], ry["C"], rx["P"], rx["C"]
    pph, ppw = (c["pool_h"] - 1) // 2, (c["pool_w"] - 1) // 2
    out = np.full(v.shape[:-2] + (P1y - P0y, P1x - P0x), -np.inf, np.float32)
    for py in range(P0y, P1y):
        ys = [y for y in range(py * c["pool_h"] - pph, py * c["pool_h"] - pph + c["pool_h"]) if 0 <= y < ch]
        assert ys and C0y <= ys[0] and ys[-1] < C1y, (c["id"], py, ys, ry)
        for px in range(P0x, P1x):
            xs = [x for x in range(px * c["pool_w"] - ppw, px * c["pool_w"] - ppw + c["pool_w"]) if 0 <= x < cw]
            assert xs and C0x <= xs[0] and xs[-1] < C1x, (c["id"], px, xs, rx)
            out[..., py - P0y, px - P0x] = v[..., ys[0] - C0y:ys[-1] + 1 - C0y, xs[0] - C0x:xs[-1] + 1 - C0x].max(axis=(-2, -1))
    return out


MUTANTS = ("short-halo-x", "short-halo-y", "live-halo", "store-word")


def tiled_trajectory(c, T, mutant=None):
    """the trajectory of seq_any_cases._trajectory computed tile by tile: per tile the C oracle on the region the tile holds (its own
    zero rows and columns in place of the padding — zero only where the image ends —, the cropped initial state), v / arp of its
    conv pixels, the final eps0 / eps1 of the pixels it owns, its pooled spikes ORed / stored into the shared words segment by
    segment.  -> per call dict(v, s, words, eps0, eps1, arp).
    mutant: 'short-halo-x' / 'short-halo-y' (a tile with columns / rows behind its own holds one column / row less), 'live-halo'
    (the initial state of a tile is read from the state the tiles before it — the later ones run first — have written back),
    'store-word' (a shared word is stored, not ORed)."""
    ny, nx = tile_count(c)
    rows, cols = tile_plan(c, max(ny, 1), nx)
    order = [(a, b) for a in range(len(rows)) for b in range(len(cols))]
    if mutant == "live-halo":
        order = order[::-1]
    ch, cw, ph, pw = out_shape(c)
    PP = ph * pw
    Bc, cin, kh, kw, pad_h, pad_w = c["B_checked"], c["c_in"], c["kh"], c["kw"], c["pad_h"], c["pad_w"]
    state = dict(eps0=T["eps0"].copy(), eps1=T["eps1"].copy(), arp=T["arp"].copy())
    out = []
    for call in T["calls"]:
        x = call["x"]
        nt = x.shape[0]
        snap = state if mutant == "live-halo" else {k: a.copy() for k, a in state.items()}
        res = dict(v=np.empty((nt, Bc, c["c_out"], ch, cw), np.float32), s=np.zeros((nt, Bc, c["c_out"], ph, pw), np.float32),
                   words=np.zeros((nt, Bc, c["c_out"], (PP + 31) // 32), np.uint32))
        for a, b in order:
            ry, rx = rows[a], cols[b]
            (C0y, C1y), (I0y, I1y), (O0y, O1y) = ry["C"], ry["I"], ry["O"]
            (C0x, C1x), (I0x, I1x), (O0x, O1x) = rx["C"], rx["I"], rx["O"]
            if mutant == "short-halo-y" and I1y > O1y:
                I1y -= 1
            if mutant == "short-halo-x" and I1x > O1x:
                I1x -= 1
            RB, top, HR = C1y - C0y + kh - 1, I0y + pad_h - C0y, I1y - I0y
            CB, left, HC = C1x - C0x + kw - 1, I0x + pad_w - C0x, I1x - I0x
            cb = dict(c, h=RB, w=CB, pad_h=0, pad_w=0, pool_h=1, pool_w=1)
            orc = A._oracle(cb, T["W"], T["b"], T["tau"], 1.0 if c["refractory"] else 0.0)
            st = [np.zeros((Bc, cin, RB, CB), np.float32), np.zeros((Bc, cin, RB, CB), np.float32),
                  np.ascontiguousarray(snap["arp"][:, :, C0y:C1y, C0x:C1x])]
            st[0][:, :, top:top + HR, left:left + HC] = snap["eps0"][:, :, I0y:I1y, I0x:I1x]
            st[1][:, :, top:top + HR, left:left + HC] = snap["eps1"][:, :, I0y:I1y, I0x:I1x]
            orc.state = st
            vs = []
            for t in range(nt):
                xb = np.zeros((Bc, cin, RB, CB), np.float32)
                xb[:, :, top:top + HR, left:left + HC] = x[t][:, :, I0y:I1y, I0x:I1x]
                vs.append(orc.forward(xb)[3])
            v = np.stack(vs)
            res["v"][:, :, :, C0y:C1y, C0x:C1x] = v
            spk = _pool_tile(c, v, ry, rx) > 0                          # (nt, Bc, c_out, pooled rows, pooled columns)
            res["s"][:, :, :, ry["P"][0]:ry["P"][1], rx["P"][0]:rx["P"][1]] = spk
            for r, py in enumerate(range(*ry["P"])):
                s0, s1 = py * pw + rx["P"][0], py * pw + rx["P"][1]
                for wi in range(s0 // 32, (s1 + 31) // 32):
                    lo, hi = max(s0, wi * 32), min(s1, wi * 32 + 32)
                    sh = (np.arange(lo, hi) - wi * 32).astype(np.uint32)
                    bits = (spk[:, :, :, r, lo - s0:hi - s0].astype(np.uint32) << sh).sum(axis=-1, dtype=np.uint32)
                    inside = wi * 32 >= s0 and min(wi * 32 + 32, PP) <= s1
                    if inside or mutant == "store-word":
                        res["words"][:, :, :, wi] = bits
                    else:
                        res["words"][:, :, :, wi] |= bits
            # the zero rows and columns stay zero
            assert not orc.state[0][:, :, :top].any() and not orc.state[1][:, :, top + HR:].any()
            assert not orc.state[0][:, :, :, :left].any() and not orc.state[1][:, :, :, left + HC:].any()
            O1y, O1x = min(O1y, I1y), min(O1x, I1x)                     # (the mutants only)
            for k, key in enumerate(("eps0", "eps1")):
                state[key][:, :, O0y:O1y, O0x:O1x] = orc.state[k][:, :, top + O0y - I0y:top + O1y - I0y, left + O0x - I0x:left + O1x - I0x]
            state["arp"][:, :, C0y:C1y, C0x:C1x] = orc.state[2]
        res.update({k: a.copy() for k, a in state.items()})
        out.append(res)
    return out
