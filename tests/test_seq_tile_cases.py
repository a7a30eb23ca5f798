"""CPU self-check of tests/seq_tile_cases.py: the case lists of dcll_conv_lif_sequence_tiles' differential test are proven here
before tests/test_gpu_seq_tile.py lets them judge the kernel.

  - the seed reproduces the lists and the strata hold what they promise, both sides of every boundary included;
  - the tile plan of every case: pooled pixels, conv pixels and owned input pixels are each partitioned exactly once, owned pixels
    are held, every pooling window and every tap of a tile's conv pixels lies inside what the tile holds;
  - the restated plan, LDS bytes, scratch and (0, 0) rule equal dcll_conv_lif_sequence_tiles_plan / _lds / _scratch of the built
    library (host-only calls) on every case and every refusal;
  - the tiled oracle (the C oracle per tile on the cropped region, stitched) equals the whole-image oracle bit for bit on every
    case: the decomposition holds without a GPU;
  - four mutants of it (a halo one column short, a halo one row short, a halo read from the written-back state, a shared word
    stored instead of ORed) are each caught by a case of the stratum that is there for it;
  - the C oracle runs every case with a sound draw: spikes and non-spikes in EVERY tile;
  - the binding declares the four symbols, and the wrappers keep today's calls with tiles=None."""
import collections
import ctypes
import inspect

import numpy as np
import pytest

import seq_band_cases as S
import seq_tile_cases as X
import seq_wide_cases as W

CASES = X.cases()
REFUSE = X.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)
TILED = [c for c in CASES if X.tile_count(c)[1] > 1]


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c.get("tau_tensor", 0), 1.0 if c["refractory"] else 0.0, X.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "05d01d465e83bb8bd38e9c967fb3e41861a19ea1579e0e5fbcb0d216e84a3331"
REFUSE_HASH = "295e60b53bad7e5062838603970f72ea9ff4db3682f10b0992b497e419d38616"


def test_the_seed_reproduces_the_lists():
    assert X.cases_hash(X.cases()) == X.cases_hash(CASES) == CASES_HASH and X.cases_hash(X.refusals()) == X.cases_hash(REFUSE) == REFUSE_HASH
    assert X.cases_hash(X.cases(X.SEED + 1)) != X.cases_hash(CASES)
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(X.by_id(c["id"]) == c for c in CASES[::20] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=11, edges=36, boundaries=8, grid=1, forwarded=6, free=60)
    named = {c["id"][len("tile-"):]: c for c in BY["named"]}
    geo = lambda c: (c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["kw"], c["pad_h"], c["pool_h"], c["refractory"])
    # radio_ml_conv.yaml (7x7, pad 3, no pooling) at netscale 2 on 8x64: no band count fits the 64 -> 64 layers; the fewest tiles
    # are 1x5 (refractory) and 1x4 (plain); the first layer is served by a band plan
    a, b, f = named["radio2-8x64-64to64"], named["radio2-8x64-64to64-plain"], named["radio2-8x64-1to64"]
    assert geo(a) == (64, 64, 8, 64, 7, 7, 3, 1, 1) and geo(b) == (64, 64, 8, 64, 7, 7, 3, 1, 0) and geo(f) == (1, 64, 8, 64, 7, 7, 3, 1, 1)
    assert a["tiles"] == b["tiles"] == f["tiles"] == [0, 0]
    for c in (a, b):
        assert all(S.band_count(c, 1, n) == 0 for n in range(0, 9)) and W.lds_bytes(c) == 0
    assert X.tile_count(a) == (1, 5) and not X.fits(a, 1, 4) and X.tile_count(b) == (1, 4) and not X.fits(b, 1, 3)
    assert all(not X.fits(c, ny, nx) for c in (a, b) for ny in (1, 2) for nx in (1, 2))
    assert X.tile_count(f)[1] == 1 and X.tile_count(f)[0] == S.band_count(f, f["B"], 0) > 0
    # layers that bands also serve: mnist_conv.yaml (16 / 24 / 32 channels, 7x7, pad 2, pooling 2 / 1 / 2 on 28x28 -> 13 -> 11)
    # at netscale 1 and 2 at (2, 2); a 32 -> 32 7x7 layer on 12x40 at (2, 2) and (1, 3)
    for s in (1, 2):
        assert geo(named["mnist%d-l1-t2x2" % s]) == (1, 16 * s, 28, 28, 7, 7, 2, 2, 0)
        assert geo(named["mnist%d-l2-t2x2" % s]) == (16 * s, 24 * s, 13, 13, 7, 7, 2, 1, 0)
        assert geo(named["mnist%d-l3-t2x2" % s]) == (24 * s, 32 * s, 11, 11, 7, 7, 2, 2, 0)
        assert all(named["mnist%d-l%d-t2x2" % (s, i)]["tiles"] == [2, 2] for i in (1, 2, 3))
    assert geo(named["r32-12x40-t2x2"]) == geo(named["r32-12x40-t1x3"]) == (32, 32, 12, 40, 7, 7, 3, 1, 1)
    assert (named["r32-12x40-t2x2"]["tiles"], named["r32-12x40-t1x3"]["tiles"]) == ([2, 2], [1, 3])
    assert sum(S.band_count(c, c["B"], 0) > 0 for c in BY["named"]) == 9
    assert all(max(c["Ts"]) <= 4 and c["B"] <= 3 for c in CASES if c["stratum"] != "grid")
    assert all(X.work(c) <= X.WORK_FREE_MAX for c in CASES if c["stratum"] != "named"), [c["id"] for c in CASES if X.work(c) > X.WORK_FREE_MAX]
    edge = {c["id"][len("tile-edge-"):]: c for c in BY["edges"]}
    ph = lambda c: X.out_shape(c)[2]
    pw = lambda c: X.out_shape(c)[3]
    for k in ("one-pixel-per-tile", "one-pixel-per-tile-pool2"):
        assert edge[k]["tiles"] == [ph(edge[k]), pw(edge[k])], k
    kk = lambda k: (edge[k]["kh"], edge[k]["kw"])
    assert (kk("k1x1"), kk("k2x5"), kk("k5x2")) == ((1, 1), (2, 5), (5, 2))
    assert all(8 <= edge[k]["h"] <= 10 and 10 <= edge[k]["w"] <= 12 for k in ("k1x1", "k2x5", "k5x2", "pool1x2", "pool2x1"))
    p0 = edge["pad0-shrinks"]
    assert p0["pad_h"] == p0["pad_w"] == 0 and X.out_shape(p0)[0] < p0["h"] and X.out_shape(p0)[1] < p0["w"]
    g = edge["pad4-grows"]
    assert (g["pad_h"], g["pad_w"], g["kh"], g["kw"]) == (4, 4, 3, 3) and X.out_shape(g)[0] > g["h"]
    rows, cols = X.tile_plan(g, *g["tiles"])
    for parts in (rows, cols):              # tiles that hold no input row / no input column, at both ends
        held = [p["I"][1] - p["I"][0] for p in parts]
        assert held[0] == 0 and held[-1] == 0 and max(held) > 0
    o = edge["pool2-odd"]
    assert o["pool_h"] == o["pool_w"] == 2 and X.out_shape(o)[0] % 2 == 1 and X.out_shape(o)[1] % 2 == 1
    rows, cols = X.tile_plan(o, *o["tiles"])
    assert rows[-1]["C"][1] == X.out_shape(o)[0] > 2 * ph(o) and cols[-1]["C"][1] == X.out_shape(o)[1] > 2 * pw(o)
    assert edge["pool3"]["pool_h"] == edge["pool3"]["pool_w"] == 3
    assert (edge["pool1x2"]["pool_h"], edge["pool1x2"]["pool_w"], edge["pool2x1"]["pool_h"], edge["pool2x1"]["pool_w"]) == (1, 2, 2, 1)
    assert [pw(edge[k]) for k in ("pw5", "pw11", "pw13", "pw32", "pw33", "pw64-no-shared-word")] == [5, 11, 13, 32, 33, 64]
    for k in ("pw5", "pw11", "pw13", "pw32", "pw33"):
        assert X.shared_words(edge[k], *edge[k]["tiles"]), k
    assert not X.shared_words(edge["pw64-no-shared-word"], *edge["pw64-no-shared-word"]["tiles"])
    assert edge["cin3"]["c_in"] == 3 and edge["cin5-mt1"]["c_in"] == 5 and X.mt(edge["cin5-mt1"]) == 1
    assert [edge[k]["c_out"] for k in ("cout1", "cout32", "cout33", "cout64")] == [1, 32, 33, 64]
    b = edge["tile-below-32px"]
    assert X.tiles_max(b, *b["tiles"]) == 1 and max((y[1] - y[0]) * (x[1] - x[0]) for y, x in X.tile_boxes(b)) < 32
    for m in (1, 2):
        for nt in (1, 2, 7, 8, 9):
            c = edge["tiles%d-mt%d" % (nt, m)]
            assert X.mt(c) == m and {((y[1] - y[0]) * (x[1] - x[0]) + 31) // 32 for y, x in X.tile_boxes(c)} == {nt}
    assert X.NW == 8                # the work split switches at 8 pixel tiles
    g = BY["grid"][0]
    assert (g["B"], g["tiles"], g["B_checked"], len(g["Ts"])) == (300, [2, 2], 8, 2) and max(g["h"], g["w"]) <= 8
    assert all(X.tile_count(c)[1] == 1 for c in BY["forwarded"]) and {c["tiles"][1] for c in BY["forwarded"]} == {0, 1}
    assert {X.variant(c).split("<")[0] for c in BY["forwarded"]} == {"k_lif_seq_any", "k_lif_seq_wide", "k_lif_seq_band"}
    free = BY["free"]
    assert len(free) >= 60 and all(X.tile_count(c)[1] >= 2 for c in free)
    assert min(c["c_out"] for c in free) <= 8 and max(c["c_out"] for c in free) >= 58 and {X.mt(c) for c in free} == {1, 2}
    assert min(c["c_in"] for c in free) <= 3 and max(c["c_in"] for c in free) >= 36 and any(c["c_in"] % 2 and c["c_in"] > 1 for c in free)
    assert {c["kh"] for c in free} | {c["kw"] for c in free} == set(range(1, 10)) and any(c["kh"] != c["kw"] for c in free)
    assert {c["pool_h"] for c in free} == {c["pool_w"] for c in free} == {1, 2, 3}
    assert {c["pad_h"] for c in free} == {c["pad_w"] for c in free} == set(range(5))
    assert any(c["tiles"] == [ph(c), pw(c)] for c in free) and len({tuple(c["tiles"]) for c in free}) > 12
    for key in ("refractory", "tau_tensor", "bias"):
        assert {c[key] for c in free} == {0, 1}, key
    assert any(len(c["Ts"]) == 2 for c in free)


def test_both_sides_of_every_boundary():
    bound = {c["id"][len("tile-bound-"):]: c for c in BY["boundaries"]}
    ref = {c["id"][len("tile-refuse-"):]: c for c in REFUSE}
    # the 160 KiB for an explicit plan
    a, b = bound["lds-cin198"], ref["lds-cin199"]
    assert X.lds_bytes(a) == 4 * 40790 <= X.LDS_MAX < 4 * X.floats_max(b, 2, 2) and X.lds_bytes(b) == 0 and a["tiles"] == b["tiles"] == [2, 2]
    # whole weights in LDS
    a, b = bound["wlds-cin64"], bound["wlds-cin66"]
    assert (X.floats_max(a, 2, 2) + 128 * X.steps(a)) * 4 == 4 * 40168 <= X.LDS_MAX < (X.floats_max(b, 2, 2) + 128 * X.steps(b)) * 4
    assert X.variant(a) == "k_lif_seq_tile<2,0,1>" and X.variant(b) == "k_lif_seq_tile<2,0,0>"
    # the (0, 0) rule: a band plan where a band count serves ...
    a = bound["rule-band-serves"]
    assert a["tiles"] == [0, 0] and X.tile_count(a) == (S.band_count(a, a["B"], 0), 1) and X.tile_count(a)[0] > 1
    # ... else the fewest tiles ...
    a, b = bound["rule-fewest-h1"], bound["rule-fewest-h2"]
    assert all(S.band_count(c, 1, 0) == 0 for c in (a, b))
    assert X.tile_count(a) == (1, 2) and X.tile_count(b) == (1, 3) and not X.fits(b, 1, 2) and not X.fits(b, 2, 1) and X.fits(b, 2, 2)
    # ... ties to the smaller held sum (here against the smaller NX), then to the smaller NX
    a = bound["rule-tie-held"]
    assert S.band_count(a, 1, 0) == 0 and not any(X.fits(a, 1, n) for n in (1, 2, 3)) and not X.fits(a, 2, 1)
    assert X.fits(a, 2, 2) and X.fits(a, 1, 4) and X.held_sum(a, 1, 4) < X.held_sum(a, 2, 2) and X.tile_count(a) == (1, 4)
    a = bound["rule-tie-nx"]
    assert S.band_count(a, 1, 0) == 0 and not any(X.fits(a, 1, n) for n in (1, 2, 3)) and not X.fits(a, 2, 1)
    assert X.fits(a, 2, 2) and X.fits(a, 1, 4) and X.held_sum(a, 1, 4) == X.held_sum(a, 2, 2) and X.tile_count(a) == (2, 2)
    # no plan fits: not even one pooled pixel per tile; a tile owns at least one pooled pixel
    n = ref["no-plan-fits"]
    assert X.tile_count(n, 2) is None and S.band_count(n, 2, 0) == 0 and not X.fits(n, *X.out_shape(n)[2:])
    assert ref["ty-above-ph"]["tiles"][0] == X.out_shape(ref["ty-above-ph"])[2] + 1
    assert ref["tx-above-pw"]["tiles"][1] == X.out_shape(ref["tx-above-pw"])[3] + 1
    assert ref["tx-above-pw-pool"]["tiles"][1] == X.out_shape(ref["tx-above-pw-pool"])[3] + 1
    # the named refractory layer at the plain layer's plan: beyond the LDS
    assert not X.fits(ref["radio2-8x64-t1x4"], 1, 4)
    g = ref["grid-beyond"]
    assert g["B_call"] * g["tiles"][0] * g["tiles"][1] > X.GRID_MAX >= g["B_call"]


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("tile-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported >= {"cout65", "stride2", "dilation2", "groups2", "k17", "ty-above-ph", "tx-above-pw", "lds-cin199", "no-plan-fits"}
    assert invalid >= {"ty-negative", "tx-negative", "ty0-alone", "tx0-alone", "no-arp", "null-spk-in", "null-W", "null-scratch",
                       "T-negative", "B-negative", "grid-beyond"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"T0", "B0", "T0-unsupported"}
    assert all(c["phrase"] for c in REFUSE if c["code"] != "DCLL_OK")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_partitions_every_pixel_exactly_once(case):
    c = case
    ny, nx = X.tile_count(c)
    ch, cw, ph, pw = X.out_shape(c)
    assert 1 <= ny <= ph and 1 <= nx <= pw
    rows, cols = X.tile_plan(c, ny, nx)
    # pooled pixels, conv pixels and owned input pixels: counted tile by tile, every one exactly once
    for key, shape in (("P", (ph, pw)), ("C", (ch, cw)), ("O", (c["h"], c["w"]))):
        count = np.zeros(shape, np.int32)
        for y in rows:
            for x in cols:
                count[y[key][0]:y[key][1], x[key][0]:x[key][1]] += 1
        assert (count == 1).all(), key
    assert all(p["P"][0] < p["P"][1] and p["C"][0] < p["C"][1] for p in rows + cols)
    # the segments of flattened pooled pixels: a partition of [0, ph pw)
    segs = sorted(s for v in X.segments(c, ny, nx).values() for s in v)
    assert segs[0][0] == 0 and segs[-1][1] == ph * pw and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
    for parts, size, k, pad, pool, conv in ((rows, c["h"], c["kh"], c["pad_h"], c["pool_h"], ch), (cols, c["w"], c["kw"], c["pad_w"], c["pool_w"], cw)):
        pp = (pool - 1) // 2
        for p in parts:
            (P0, P1), (C0, C1), (I0, I1), (O0, O1) = p["P"], p["C"], p["I"], p["O"]
            assert I0 <= O0 <= O1 <= I1                                             # owned pixels are held
            win = [y for q in range(P0, P1) for y in range(q * pool - pp, q * pool - pp + pool) if 0 <= y < conv]
            assert min(win) == C0 and max(win) < C1                                 # the pooling windows lie inside the tile
            taps = [y - pad + t for y in range(C0, C1) for t in range(k)]
            assert all(I0 <= y < I1 for y in taps if 0 <= y < size)                 # every in-image tap is held
    if nx > 1:
        assert all(X.tile_floats(c, y, x) * 4 <= X.LDS_MAX for y in rows for x in cols)


def test_the_library_agrees_with_the_restated_plan():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the functions are host-only)
    plan = lambda d, B, t: (lambda nn: (int(lib.dcll_conv_lif_sequence_tiles_plan(ctypes.byref(d), B, t[0], t[1], nn, None, None)),
                                        (nn[0], nn[1])))((ctypes.c_int32 * 2)())
    for c in CASES:
        d = _desc(c)
        ny, nx = X.tile_count(c)
        ph, pw = X.out_shape(c)[2:]
        by, bx, nn = (ctypes.c_int32 * (ph + 2))(), (ctypes.c_int32 * (pw + 2))(), (ctypes.c_int32 * 2)()
        got = int(lib.dcll_conv_lif_sequence_tiles_plan(ctypes.byref(d), c["B"], c["tiles"][0], c["tiles"][1], nn, by, bx))
        assert got == ny * nx > 0 and (nn[0], nn[1]) == (ny, nx), X.describe(c)
        rows, cols = X.tile_plan(c, ny, nx)
        assert list(by)[:ny + 1] == [p["P"][0] for p in rows] + [ph] and list(bx)[:nx + 1] == [p["P"][0] for p in cols] + [pw]
        assert ops.sequence_tiles_plan(d, c["B"], c["tiles"]) == (list(by)[:ny + 1], list(bx)[:nx + 1])
        lds = int(lib.dcll_conv_lif_sequence_tiles_lds(ctypes.byref(d), c["tiles"][0], c["tiles"][1]))
        assert lds == X.lds_bytes(c) > 0 and (lds <= X.LDS_MAX or nx == 1), X.describe(c)
        assert ops.sequence_tiles_lds(d, c["tiles"]) == lds and ops.sequence_tiles_supported(d, c["tiles"])
        assert int(lib.dcll_conv_lif_sequence_tiles_scratch(ctypes.byref(d), c["B"])) == X.scratch_floats(c) > 0, X.describe(c)
        for B in (1, 64, 256, 1000):                # the (0, 0) rule
            n, pair = plan(d, B, (0, 0))
            assert (pair if n else None) == X.tile_count(c, B, (0, 0)) and n > 0, (X.describe(c), B)
        for ty in range(0, min(ph, 5) + 2):         # explicit plans (a column of them: bands): served exactly where they fit
            for tx in sorted({0, 1, 2, 3, pw, pw + 1}):
                n, pair = plan(d, c["B"], (ty, tx))
                assert (pair if n else None) == X.tile_count(c, tiles=(ty, tx)), (X.describe(c), ty, tx)
                assert int(lib.dcll_conv_lif_sequence_tiles_lds(ctypes.byref(d), ty, tx)) == X.lds_bytes(c, (ty, tx))
        if nx == 1:                 # a band plan: the band path's answers, its scratch
            assert lds == int(lib.dcll_conv_lif_sequence_bands_lds(ctypes.byref(d), ny)) > 0
            assert X.scratch_floats(c) == int(lib.dcll_conv_lif_sequence_bands_scratch(ctypes.byref(d), c["B"]))
    for c in REFUSE:
        d = _desc(c)
        n, pair = plan(d, 2, c["tiles"])
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert n == 0 and X.tile_count(c, 2) is None, X.describe(c)
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
            assert int(lib.dcll_conv_lif_sequence_tiles_lds(ctypes.byref(d), *c["tiles"])) == 0 and not ops.sequence_tiles_supported(d, c["tiles"])
            assert ops.sequence_tiles_plan(d, 2, c["tiles"]) is None
        elif min(c["tiles"]) < 0 or (0 in c["tiles"] and c["tiles"] != [0, 0] and c["tiles"][1] != 1):     # an invalid count
            assert n == 0 and X.tile_count(c, 2) is None and c["phrase"] in lib.dcll_last_error().decode(), X.describe(c)
        elif "unsupported" not in c["id"]:
            assert (pair if n else None) == X.tile_count(c, 2) is not None, X.describe(c)


def test_the_cases_reach_every_template_variant():
    var = collections.Counter(X.variant(c) for c in TILED)
    assert set(var) == set(X.all_variants()) and len(var) == 8, var
    print("cases per variant:", dict(var))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_sound_and_the_tiled_oracle_equals_the_whole_image(case):
    """the C oracle tile by tile on the cropped input region, with the tile's own zero rows and columns where the image ends and the
    cropped initial state, stitched == the whole-image oracle, bit for bit: v, pooled spikes, the packed words, eps0 / eps1 / arp
    after every call; every tile has spikes and non-spikes"""
    c = case
    T, traj = X.run(c)                          # (asserts: accepted by the oracle, its shapes, a sound draw within 24 attempts)
    assert X.unsound(c, traj) is None, X.describe(c)
    for (y0, y1), (x0, x1) in X.tile_boxes(c):
        s = np.concatenate([call["v"][:, :, :, y0:y1, x0:x1].ravel() for call in traj]) > 0
        assert s.any() and not s.all(), (c["id"], y0, y1, x0, x1)
    ch, cw, ph, pw = X.out_shape(c)
    for n, call in zip(c["Ts"], traj):
        assert call["v"].shape == (n, c["B_checked"], c["c_out"], ch, cw) and call["s"].shape == (n, c["B_checked"], c["c_out"], ph, pw)
    for k, (got, ref) in enumerate(zip(X.tiled_trajectory(c, T), traj)):
        for key in ("v", "s", "eps0", "eps1", "arp"):
            assert np.array_equal(_bits(got[key]), _bits(ref[key])), (c["id"], k, key)
        assert np.array_equal(got["words"], X.pack_planes(ref["s"].reshape(ref["s"].shape[:3] + (-1,)))), (c["id"], k, "words")


def _differs(c, mutant):
    T, traj = X.run(c)
    for got, ref in zip(X.tiled_trajectory(c, T, mutant), traj):
        if any(not np.array_equal(_bits(got[key]), _bits(ref[key])) for key in ("v", "s", "eps0", "eps1", "arp")):
            return True
        if not np.array_equal(got["words"], X.pack_planes(ref["s"].reshape(ref["s"].shape[:3] + (-1,)))):
            return True
    return False


def test_the_mutants_are_caught():
    """a halo one column short: by every edge case whose kernel is wider than one column — and not by the 1x1 kernel; a halo one row
    short: by every one whose kernel is higher than one row; a halo whose initial state is a neighbour's final state: by the grid
    case (two calls) and the same edges; a shared word stored instead of ORed: by every pooled-width case with a shared word — and
    not by the one without"""
    edge = {c["id"][len("tile-edge-"):]: c for c in BY["edges"]}
    grid = BY["grid"][0]
    assert set(X.MUTANTS) == {"short-halo-x", "short-halo-y", "live-halo", "store-word"}
    for mutant in ("short-halo-x", "short-halo-y", "live-halo"):
        assert _differs(grid, mutant), mutant
        for k in ("one-pixel-per-tile", "k2x5", "k5x2", "pool3", "pw13", "tiles2-mt2"):
            assert _differs(edge[k], mutant), (mutant, k)
        assert not _differs(edge["k1x1"], mutant)       # (no halo: nothing to get wrong)
    for k in ("pw5", "pw11", "pw13", "pw32", "pw33"):
        assert _differs(edge[k], "store-word"), k
    assert not _differs(edge["pw64-no-shared-word"], "store-word")


def test_the_binding_declares_the_four_symbols():
    from snn_modulation_classification_amd import _lib
    S_ = _lib.SIGNATURES
    bands = S_["dcll_conv_lif_sequence_bands"]
    assert S_["dcll_conv_lif_sequence_tiles"] == (bands[0], bands[1][:-1] + [ctypes.c_int32, bands[1][-1]])
    lib = _lib.get()
    assert lib.dcll_version() == _lib.ABI_VERSION == 10
    assert all(hasattr(lib, "dcll_conv_lif_sequence_tiles" + n) for n in ("", "_plan", "_lds", "_scratch"))


def test_the_wrappers_keep_todays_calls_without_tiles():
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import Conv2dDCLLlayer
    from snn_modulation_classification_amd.networks import ConvNetwork
    for fn in (Conv2dDCLLlayer.sequence_any_supported, Conv2dDCLLlayer.forward_sequence_any, ConvNetwork.sequence_any_supported,
               ConvNetwork.test_sequence_any):
        p = inspect.signature(fn).parameters
        assert p["tiles"].default is None and p["bands"].default is None and p["wide"].default is False, fn
    import train
    assert train.parse_args([]).tile_sequence_path is None and train._tile_sequence_arg(train.parse_args([])) is None
    assert train._tile_sequence_arg(train.parse_args(["--tile_sequence_path"])) == (0, 0)
    assert train._tile_sequence_arg(train.parse_args(["--tile_sequence_path", "1", "4"])) == (1, 4)
    with pytest.raises(SystemExit):
        train._tile_sequence_arg(train.parse_args(["--tile_sequence_path", "3"]))
