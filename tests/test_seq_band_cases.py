"""CPU self-check of tests/seq_band_cases.py: the case lists of dcll_conv_lif_sequence_bands' differential test are proven here
before tests/test_gpu_seq_band.py lets them judge the kernel.

  - the seed reproduces the lists and the strata hold what they promise, both sides of every boundary included;
  - the band plan of every case: pooled rows, conv rows, owned input rows and pooled pixel ranges are each an exact partition, owned
    input rows are held, every pooling window and every tap of a band's conv rows lies inside what the band holds;
  - the restated plan, LDS bytes, scratch and default rule equal dcll_conv_lif_sequence_bands_plan / _lds / _scratch of the built
    library (host-only calls) on every case and every refusal;
  - the banded oracle (the C oracle per band on the cropped rows, stitched) equals the whole-image oracle bit for bit on every
    case: the decomposition holds without a GPU;
  - three mutants of it (a halo one row short, a halo read from the written-back state, a boundary word stored instead of ORed) are
    each caught by a case of the stratum that is there for it;
  - the C oracle runs every case with a sound draw: spikes and non-spikes in EVERY band;
  - the binding declares the four symbols, and the wrappers keep today's calls with bands=None."""
import collections
import ctypes
import inspect

import numpy as np
import pytest

import seq_band_cases as S
import seq_wide_cases as W

CASES = S.cases()
REFUSE = S.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)
BANDED = [c for c in CASES if S.band_count(c) > 1]


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c.get("tau_tensor", 0), 1.0 if c["refractory"] else 0.0, S.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "90dcdeb9abad2fab6f3e9498656544d6de71cf2d075127e8554f75ed8d17fe9b"
REFUSE_HASH = "9f7ae984b6d21f6d37dfc38c0d08b064f647a89c9b25f7777a10cdacb7fa704d"


def test_the_seed_reproduces_the_lists():
    assert S.cases_hash(S.cases()) == S.cases_hash(CASES) == CASES_HASH and S.cases_hash(S.refusals()) == S.cases_hash(REFUSE) == REFUSE_HASH
    assert S.cases_hash(S.cases(S.SEED + 1)) != S.cases_hash(CASES)
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(S.by_id(c["id"]) == c for c in CASES[::20] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=22, edges=33, boundaries=13, grid=1, forwarded=5, free=60)
    named = {c["id"][len("band-"):]: c for c in BY["named"]}
    geo = lambda c: (c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["kw"], c["pad_h"], c["pool_h"], c["refractory"])
    # radio_ml_conv.yaml (7x7, pad 3, no pooling) at netscale 2 on 16x16 at 2 / 4 / 8 bands — but the refractory 64 -> 64 layer at
    # two bands, whose band is beyond the LDS: a refusal
    for nb in (2, 4, 8):
        assert geo(named["radio2-1to64-b%d" % nb]) == (1, 64, 16, 16, 7, 7, 3, 1, 1) and named["radio2-1to64-b%d" % nb]["bands"] == nb
        assert geo(named["radio2-64to64-plain-b%d" % nb]) == (64, 64, 16, 16, 7, 7, 3, 1, 0)
    assert "radio2-64to64-b2" not in named and any(r["id"] == "band-refuse-radio2-64to64-b2" for r in REFUSE)
    assert all(geo(named["radio2-64to64-b%d" % nb]) == (64, 64, 16, 16, 7, 7, 3, 1, 1) for nb in (4, 8))
    # netscale 1 on 48x48: refused by the one-workgroup kernels, served here by the rule
    for k in ("radio1-48x48-1to32", "radio1-48x48-32to32"):
        c = named[k]
        assert (c["h"], c["w"], c["c_out"], c["bands"]) == (48, 48, 32, 0) and W.lds_bytes(c) == 0 and S.band_count(c) > 1, k
    # mnist_conv.yaml (16 / 24 / 32 channels, 7x7, pad 2, pooling 2 / 1 / 2 on 28x28 -> 13 -> 11) at netscale 1 and 2
    for s in (1, 2):
        for nb in (2, 4):
            assert geo(named["mnist%d-l1-b%d" % (s, nb)]) == (1, 16 * s, 28, 28, 7, 7, 2, 2, 0)
            assert geo(named["mnist%d-l2-b%d" % (s, nb)]) == (16 * s, 24 * s, 13, 13, 7, 7, 2, 1, 0)
            assert geo(named["mnist%d-l3-b%d" % (s, nb)]) == (24 * s, 32 * s, 11, 11, 7, 7, 2, 2, 0)
    assert all(max(c["Ts"]) <= 4 and c["B"] <= 3 for c in CASES if c["stratum"] not in ("grid", "boundaries", "forwarded"))
    assert all(max(c["Ts"]) <= 4 and c["B_checked"] <= 3 for c in BY["boundaries"] + BY["forwarded"])
    assert all(S.work(c) <= S.WORK_FREE_MAX for c in CASES if c["stratum"] != "named"), [c["id"] for c in CASES if S.work(c) > S.WORK_FREE_MAX]
    edge = {c["id"][len("band-edge-"):]: c for c in BY["edges"]}
    ph = lambda c: S.out_shape(c)[2]
    pw = lambda c: S.out_shape(c)[3]
    assert edge["one-row-per-band"]["bands"] == ph(edge["one-row-per-band"]) == 8
    assert edge["one-row-per-band-pool2"]["bands"] == ph(edge["one-row-per-band-pool2"]) == 4
    assert (edge["k1x1"]["kh"], edge["k1x1"]["kw"], edge["k2x5"]["kh"], edge["k2x5"]["kw"]) == (1, 1, 2, 5)
    assert edge["pad0-shrinks"]["pad_h"] == 0 and S.out_shape(edge["pad0-shrinks"])[0] < edge["pad0-shrinks"]["h"]
    g = edge["pad4-grows"]
    assert g["pad_h"] == 4 and g["kh"] == 3 and S.out_shape(g)[0] > g["h"]
    held = [b["I"][1] - b["I"][0] for b in S.plan(g, g["bands"])]
    assert held[0] == 0 and held[-1] == 0 and max(held) > 0         # bands that read only padding, above and below
    o = edge["pool2-odd-ch"]
    assert o["pool_h"] == 2 and S.out_shape(o)[0] % 2 == 1 and S.plan(o, o["bands"])[-1]["C"][1] == S.out_shape(o)[0] > 2 * ph(o)
    assert edge["pool3"]["pool_h"] == 3
    assert [pw(edge[k]) for k in ("pw5", "pw11", "pw13", "pw33", "pw32")] == [5, 11, 13, 33, 32]
    for k in ("pw5", "pw11", "pw13", "pw33", "pw5-three-bands-a-word"):
        assert S.shared_words(edge[k], edge[k]["bands"]), k
    assert not S.shared_words(edge["pw32"], edge["pw32"]["bands"])
    # a word shared by two bands, and one shared by three and more
    sharers = lambda c: collections.Counter(wi for b in S.plan(c, c["bands"]) for wi in range(b["P"][0] * pw(c) // 32, (b["P"][1] * pw(c) + 31) // 32))
    assert 2 in sharers(edge["pw33"]).values() and max(sharers(edge["pw5-three-bands-a-word"]).values()) >= 3
    assert edge["cin3"]["c_in"] == 3 and edge["cin5-mt1"]["c_in"] == 5
    assert [edge[k]["c_out"] for k in ("cout1", "cout32", "cout33", "cout64")] == [1, 32, 33, 64]
    b = edge["band-below-32px"]
    assert max((p["C"][1] - p["C"][0]) * S.out_shape(b)[1] for p in S.plan(b, b["bands"])) < 32
    for m in (1, 2):
        for nt in (1, 2, 7, 8, 9):
            c = edge["tiles%d-mt%d" % (nt, m)]
            assert S.mt(c) == m and S.tiles_max(c, c["bands"]) == nt == min(((p["C"][1] - p["C"][0]) * 32 + 31) // 32 for p in S.plan(c, 2))
    assert S.NW == 8                # the work split switches at 8 tiles
    g = BY["grid"][0]
    assert (g["B"], g["bands"], g["B_checked"], len(g["Ts"])) == (300, 4, 8, 2) and g["B"] * g["bands"] == 1200
    assert all(S.band_count(c) == 1 for c in BY["forwarded"]) and {c["bands"] for c in BY["forwarded"]} == {0, 1}
    assert {S.variant(c).split("<")[0] for c in BY["forwarded"]} == {"k_lif_seq_any", "k_lif_seq_wide"}
    free = BY["free"]
    assert min(c["c_out"] for c in free) <= 8 and max(c["c_out"] for c in free) >= 58 and {S.mt(c) for c in free} == {1, 2}
    assert min(c["c_in"] for c in free) <= 3 and max(c["c_in"] for c in free) >= 36 and any(c["c_in"] % 2 and c["c_in"] > 1 for c in free)
    assert {c["kh"] for c in free} | {c["kw"] for c in free} == set(range(1, 10)) and any(c["kh"] != c["kw"] for c in free)
    assert {c["pool_h"] for c in free} == {c["pool_w"] for c in free} == {1, 2, 3}
    assert {c["pad_h"] for c in free} == {c["pad_w"] for c in free} == set(range(5))
    assert min(min(c["h"], c["w"]) for c in free) >= 3 and max(max(c["h"], c["w"]) for c in free) >= 36
    assert all(1 <= c["bands"] <= ph(c) for c in free) and any(c["bands"] == ph(c) > 1 for c in free) and len({c["bands"] for c in free}) > 8
    for key in ("refractory", "tau_tensor", "bias"):
        assert {c[key] for c in free} == {0, 1}, key
    assert any(len(c["Ts"]) == 2 for c in free)


def test_both_sides_of_every_boundary():
    bound = {c["id"][len("band-bound-"):]: c for c in BY["boundaries"]}
    ref = {c["id"][len("band-refuse-"):]: c for c in REFUSE}
    # the 160 KiB for an explicit band count
    a, b = bound["lds-cin99"], ref["lds-cin100"]
    assert S.lds_bytes(a) == 4 * 40728 <= S.LDS_MAX < 4 * max(S.band_floats(b, p) for p in S.plan(b, 2)) and S.lds_bytes(b) == 0
    assert a["bands"] == b["bands"] == 2 and W.lds_bytes(a) == 0
    # whole weights in LDS
    a, b = bound["wlds-cin62"], bound["wlds-cin64"]
    base = lambda c: max(S.band_floats(c, p) for p in S.plan(c, 2))
    assert (base(a) + 128 * S.steps(a)) * 4 == 4 * 40712 <= S.LDS_MAX < (base(b) + 128 * S.steps(b)) * 4
    assert S.variant(a) == "k_lif_seq_band<2,0,1>" and S.variant(b) == "k_lif_seq_band<2,0,0>"
    # the default rule: one band where the one-workgroup kernel serves the layer with one chain per wave ...
    a, b = bound["rule-wide-serves"], bound["rule-wide-refuses"]
    assert a["bands"] == b["bands"] == 0 and W.lds_bytes(a) > 0 == W.lds_bytes(b) and b["c_in"] - a["c_in"] == 2
    assert S.band_count(a) == 1 and S.tiles_max(a, 1) == 8 and S.band_count(b) == 8 and S.tiles_max(b, 8) == 1 < S.tiles_max(b, 7)
    a, b, m = bound["rule-cpw-t8"], bound["rule-cpw-t9"], bound["rule-cpw-mt2"]
    assert (S.tiles_max(a, 1), S.mt(a), S.band_count(a)) == (8, 1, 1) and (S.tiles_max(b, 1), S.mt(b), S.band_count(b)) == (9, 1, 9)
    assert (S.tiles_max(m, 1), S.mt(m), S.band_count(m)) == (8, 2, 8) and all(W.lds_bytes(c) > 0 for c in (a, b, m))
    # ... raised while B n <= 256 ...
    a, b = bound["rule-b64"], bound["rule-b65"]
    assert (a["B"], S.band_count(a), b["B"], S.band_count(b)) == (64, 4, 65, 3) and S.fits(a, 4) and S.fits(b, 4) and S.fits(b, 3)
    a = bound["rule-b256"]
    assert a["B"] == 256 and S.band_count(a) == 1 and S.band_count(a, B=128) == 2 and S.band_count(a, B=129) == 1
    # ... and not beyond one pixel tile per band
    a, b = bound["rule-tile-w16"], bound["rule-tile-w17"]
    assert W.lds_bytes(a) == W.lds_bytes(b) == 0
    assert (S.band_count(a), S.tiles_max(a, 16), S.tiles_max(a, 15)) == (16, 1, 2) and (S.band_count(b), S.tiles_max(b, 31)) == (32, 2)
    # no count fits; a band owns at least one pooled row
    assert S.band_count(ref["no-count-fits"]) == 0 and all(not S.fits(ref["no-count-fits"], n) for n in range(1, 5))
    assert ref["bands-above-ph"]["bands"] == S.out_shape(ref["bands-above-ph"])[2] + 1
    assert ref["bands-above-ph-pool"]["bands"] == S.out_shape(ref["bands-above-ph-pool"])[2] + 1


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("band-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported >= {"cout65", "stride2", "dilation2", "groups2", "k17", "bands-above-ph", "lds-cin100", "no-count-fits", "b1-wide-refuses"}
    assert invalid >= {"no-arp", "null-spk-in", "null-W", "null-scratch", "T-negative", "bands-negative"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"T0", "B0", "T0-unsupported"}
    assert all(c["phrase"] for c in REFUSE if c["code"] != "DCLL_OK")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_plan_is_an_exact_partition(case):
    c = case
    n = S.band_count(c)
    assert 1 <= n <= S.out_shape(c)[2]
    ch, cw, ph, pw = S.out_shape(c)
    bands = S.plan(c, n)
    for key, total in (("P", ph), ("C", ch), ("O", c["h"])):
        assert bands[0][key][0] == 0 and bands[-1][key][1] == total, key
        assert all(a[key][1] == b[key][0] for a, b in zip(bands, bands[1:])), key
        assert all(b[key][0] <= b[key][1] for b in bands), key
    assert all(b["P"][0] < b["P"][1] and b["C"][0] < b["C"][1] for b in bands)
    # pooled pixel ranges: a partition of [0, ph pw); every word has a band that stores it or bands that OR into it
    assert [b["P"][0] * pw for b in bands] + [ph * pw] == sorted({b["P"][0] * pw for b in bands} | {ph * pw})
    pph = (c["pool_h"] - 1) // 2
    for b in bands:
        (P0, P1), (C0, C1), (I0, I1), (O0, O1) = b["P"], b["C"], b["I"], b["O"]
        assert I0 <= O0 <= O1 <= I1                                             # owned rows are held
        rows = [y for py in range(P0, P1) for y in range(py * c["pool_h"] - pph, py * c["pool_h"] - pph + c["pool_h"]) if 0 <= y < ch]
        assert min(rows) == C0 and max(rows) < C1                               # the pooling windows lie inside the band
        taps = [y - c["pad_h"] + ky for y in range(C0, C1) for ky in range(c["kh"])]
        assert all(I0 <= y < I1 for y in taps if 0 <= y < c["h"])              # every in-image tap row is held
        assert S.band_floats(c, b) * 4 <= S.LDS_MAX or n == 1


def test_the_library_agrees_with_the_restated_plan():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the functions are host-only)
    for c in CASES:
        d = _desc(c)
        n = S.band_count(c)
        bounds = (ctypes.c_int32 * (S.out_shape(c)[2] + 2))()
        assert int(lib.dcll_conv_lif_sequence_bands_plan(ctypes.byref(d), c["B"], c["bands"], bounds)) == n > 0, S.describe(c)
        assert list(bounds)[:n + 1] == [b["P"][0] for b in S.plan(c, n)] + [S.out_shape(c)[2]] == ops.sequence_bands_plan(d, c["B"], c["bands"])
        got = int(lib.dcll_conv_lif_sequence_bands_lds(ctypes.byref(d), c["bands"]))
        assert got == S.lds_bytes(c) > 0 and got <= S.LDS_MAX, S.describe(c)
        assert ops.sequence_bands_lds(d, c["bands"]) == got and ops.sequence_bands_supported(d, c["bands"])
        assert int(lib.dcll_conv_lif_sequence_bands_scratch(ctypes.byref(d), c["B"])) == S.scratch_floats(c), S.describe(c)
        for B in (1, 64, 255, 256, 1000):          # the default rule
            assert int(lib.dcll_conv_lif_sequence_bands_plan(ctypes.byref(d), B, 0, None)) == S.rule(c, B) > 0, (S.describe(c), B)
        for nb in range(1, S.out_shape(c)[2] + 2):  # every explicit count: served exactly where it fits
            assert int(lib.dcll_conv_lif_sequence_bands_plan(ctypes.byref(d), c["B"], nb, None)) == S.band_count(c, bands=nb)
            assert int(lib.dcll_conv_lif_sequence_bands_lds(ctypes.byref(d), nb)) == S.lds_bytes(c, nb)
        if n == 1:                  # one band: the sibling's answers, its scratch the prefix
            assert int(lib.dcll_conv_lif_sequence_bands_lds(ctypes.byref(d), 1)) == int(lib.dcll_conv_lif_sequence_wide_lds(ctypes.byref(d))) > 0
            assert S.scratch_floats(c) - 2 * c["B"] * c["c_in"] * c["h"] * c["w"] == int(lib.dcll_conv_lif_sequence_wide_scratch(ctypes.byref(d)))
    for c in REFUSE:
        d = _desc(c)
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert int(lib.dcll_conv_lif_sequence_bands_plan(ctypes.byref(d), 2, c["bands"], None)) == 0 == S.band_count(c, 2), S.describe(c)
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
            assert int(lib.dcll_conv_lif_sequence_bands_lds(ctypes.byref(d), c["bands"])) == 0 and not ops.sequence_bands_supported(d, c["bands"])
        elif c["id"] == "band-refuse-bands-negative":
            assert int(lib.dcll_conv_lif_sequence_bands_plan(ctypes.byref(d), 2, c["bands"], None)) == 0 == S.band_count(c, 2)
        elif "unsupported" not in c["id"]:
            assert int(lib.dcll_conv_lif_sequence_bands_plan(ctypes.byref(d), 2, c["bands"], None)) == S.band_count(c, 2) > 0


def test_the_cases_reach_every_template_variant():
    var = collections.Counter(S.variant(c) for c in BANDED)
    assert set(var) == set(S.all_variants()) and len(var) == 8, var
    print("cases per variant:", dict(var))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_sound_and_the_banded_oracle_equals_the_whole_image(case):
    """the C oracle band by band on the cropped input rows, with the band's own zero rows above and below and the cropped initial
    state, stitched == the whole-image oracle, bit for bit: v, pooled spikes, the packed words, eps0 / eps1 / arp after every call"""
    c = case
    T, traj = S.run(c)                          # (asserts: accepted by the oracle, its shapes, a sound draw within 24 attempts)
    assert S.unsound(c, traj) is None, S.describe(c)
    for C0, C1 in S.band_rows_of(c):
        s = np.concatenate([call["v"][:, :, :, C0:C1].ravel() for call in traj]) > 0
        assert s.any() and not s.all(), (c["id"], C0, C1)
    ch, cw, ph, pw = S.out_shape(c)
    for n, call in zip(c["Ts"], traj):
        assert call["v"].shape == (n, c["B_checked"], c["c_out"], ch, cw) and call["s"].shape == (n, c["B_checked"], c["c_out"], ph, pw)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    for k, (got, ref) in enumerate(zip(S.banded_trajectory(c, T), traj)):
        for key in ("v", "s", "eps0", "eps1", "arp"):
            assert np.array_equal(bits(got[key]), bits(ref[key])), (c["id"], k, key)
        assert np.array_equal(got["words"], S.pack_planes(ref["s"].reshape(ref["s"].shape[:3] + (-1,)))), (c["id"], k, "words")


def _differs(c, mutant):
    T, traj = S.run(c)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    for got, ref in zip(S.banded_trajectory(c, T, mutant), traj):
        if any(not np.array_equal(bits(got[key]), bits(ref[key])) for key in ("v", "s", "eps0", "eps1", "arp")):
            return True
        if not np.array_equal(got["words"], S.pack_planes(ref["s"].reshape(ref["s"].shape[:3] + (-1,)))):
            return True
    return False


def test_the_mutants_are_caught():
    """a halo one row short and a halo whose initial state is a neighbour's final state: caught by the grid case (two calls) and by
    EVERY edge case with a kernel of more than one row; a boundary word stored instead of ORed: by every pooled-width case with a
    shared word — and not by the one without"""
    edge = {c["id"][len("band-edge-"):]: c for c in BY["edges"]}
    grid = BY["grid"][0]
    for mutant in ("short-halo", "live-halo"):
        assert _differs(grid, mutant), mutant
        for k in ("one-row-per-band", "k2x5", "pool3", "pw13", "tiles2-mt2"):
            assert _differs(edge[k], mutant), (mutant, k)
        assert not _differs(edge["k1x1"], mutant)       # (no halo: nothing to get wrong)
    for k in ("pw5", "pw11", "pw13", "pw33", "pw5-three-bands-a-word"):
        assert _differs(edge[k], "store-word"), k
    assert not _differs(edge["pw32"], "store-word")


def test_the_binding_declares_the_four_symbols():
    from snn_modulation_classification_amd import _lib
    S_ = _lib.SIGNATURES
    wide = S_["dcll_conv_lif_sequence_wide"]
    assert S_["dcll_conv_lif_sequence_bands"] == (wide[0], wide[1][:-1] + [ctypes.c_int32, wide[1][-1]])
    lib = _lib.get()
    assert lib.dcll_version() == _lib.ABI_VERSION == 10
    assert all(hasattr(lib, "dcll_conv_lif_sequence_bands" + n) for n in ("", "_plan", "_lds", "_scratch"))


def test_the_wrappers_keep_todays_calls_without_bands():
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import Conv2dDCLLlayer
    from snn_modulation_classification_amd.networks import ConvNetwork
    for fn in (Conv2dDCLLlayer.sequence_any_supported, Conv2dDCLLlayer.forward_sequence_any, ConvNetwork.sequence_any_supported,
               ConvNetwork.test_sequence_any):
        p = inspect.signature(fn).parameters
        assert p["bands"].default is None and p["wide"].default is False, fn
    import train
    assert train.parse_args([]).band_sequence_path is None
    assert train.parse_args(["--band_sequence_path"]).band_sequence_path == 0
    assert train.parse_args(["--band_sequence_path", "4"]).band_sequence_path == 4
