"""CPU self-check of tests/step_slab_cases.py: the case list of dcll_conv_lif_step_slab's differential test is proven here before
tests/test_gpu_step_slab.py lets it judge the kernel.

  - the seed reproduces the lists and the strata hold what they promise (the issue's named figures included);
  - the restated plan() / lds_bytes() / scratch_floats() equal dcll_conv_lif_step_slab_plan / _lds / _scratch — the library's own
    (host-only) functions — for every case, band count and refusal, with the refusal's phrase in dcll_last_error();
  - every refusal returns its code and message on the host, before any launch; the older entry points still refuse c_out 65 / 33;
  - the bands partition the conv rows and the pooled rows exactly once, for every case and for ph 1 ... 40; the slabs partition
    [0, c_out); every B-operand offset a lane can form lies inside the band's staged rows; ragged lanes are clamped;
  - the C oracle, run band by band and slab by slab on slices, equals the whole layer bit for bit, and four wrong decompositions
    (a halo one row short, a slab offset by one M tile, the bias of slab 0, traces advanced twice) are each caught in every case
    they can touch;
  - every (band, slab) of every case has spikes and non-spikes at some step, within the asserted cap on re-seeds."""
import collections
import ctypes

import numpy as np
import pytest

import fuzz_cases as FZ
import step_slab_cases as S

CASES = S.cases()
REFUSE = S.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)


# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "3785e0ad8d25904c527e89343efded7f47f82e267994bf6808009f1592dbb3ac"
REFUSE_HASH = "8b945237b85e3ddd6927e720460e4c8260c71252be738f8c1bb6796042eb0fc5"


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c["tau_tensor"], 1.0 if c["refractory"] else 0.0, FZ.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


def band_counts(c):
    """the band counts a case is looked at with: its own call's, 1, 2, 3 and ph wherever each fits"""
    ph = FZ.conv_shape(c)[2]
    own = S.run_nb(c)
    return sorted({own} | {n for n in (1, 2, 3, ph) if n <= ph and S.lds_max(c, n) * 4 <= S.LDS_MAX})


def test_the_seed_reproduces_the_lists_exactly():
    assert S.cases_hash(S.cases()) == S.cases_hash(CASES) == CASES_HASH != S.cases_hash(S.cases(S.SEED + 1))
    assert S.cases_hash(S.refusals()) == S.cases_hash(REFUSE) == REFUSE_HASH
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(S.by_id(c["id"]) == c for c in CASES[::10] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=5, forms=4, slabs=8, cin=6, shapes=17, options=10, rule=8, grid=1,
                                                      forwarded=2, free=30)
    assert all(c["B"] <= 3 for c in CASES)
    named = {c["id"]: c for c in BY["named"]}
    geo = lambda c: (c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["pad_h"], c["pool_h"], c["refractory"])
    assert [geo(named["slab-radio4-l%d" % l]) for l in (1, 2)] == [(1, 128, 16, 16, 7, 3, 1, 1), (128, 128, 16, 16, 7, 3, 1, 1)]
    assert [geo(named["slab-radio3-l%d" % l]) for l in (1, 2)] == [(1, 96, 16, 16, 7, 3, 1, 1), (96, 96, 16, 16, 7, 3, 1, 1)]
    assert geo(named["slab-radio2-24x40-l2"]) == (64, 64, 24, 40, 7, 3, 1, 1)
    # the issue's figures: c_in 128 needs two bands of (128 14 22 + 64) 4 = 157 952 bytes, c_in 96 two, c_in <= 84 one
    l4, l3 = named["slab-radio4-l2"], named["slab-radio3-l2"]
    assert S.nb_fit(l4) == 2 and S.lds_max(l4, 2) * 4 == (128 * 14 * 22 + 64) * 4 == 157952 and S.lds_max(l4, 1) * 4 > S.LDS_MAX
    assert S.nb_fit(l3) == 2 and S.lds_max(l3, 1) * 4 > S.LDS_MAX
    assert S.plan(l4, 512) == (2, 2) and S.plan(l4, 64) == (2, 2) and S.plan(l4, 1) == (4, 2) and S.plan(l3, 512) == (2, 2)
    w24 = named["slab-radio2-24x40-l2"]
    assert S.served(w24) is None and not S.forwarded(w24) and S.plan(w24, 64) == (4, 1) and 64 * 30 * 46 * 4 > S.LDS_MAX
    cin = {c["id"][len("slab-"):]: c for c in BY["cin"]}
    assert (S.nb_fit(cin["cin84-k7"]), S.nb_fit(cin["cin85-k7"])) == (1, 2)
    assert S.plan(cin["cin84-k7"], 128)[0] == 1 and S.plan(cin["cin85-k7"], 128)[0] == 2
    assert sorted(c["c_in"] for c in BY["cin"]) == [1, 3, 64, 70, 84, 85]
    co = {c["id"][len("slab-co-"):]: c for c in BY["slabs"]}
    assert [S.slabs(co["cout%d" % n])[-1][1] for n in (65, 96, 97, 128, 129, 200)] == [1, 32, 33, 64, 1, 8]
    assert [len(S.slabs(co["cout%d" % n])) for n in (65, 96, 97, 128, 129, 200)] == [2, 2, 2, 2, 3, 4]
    for k in ("cout40-bands2", "cout64-bands2"):
        assert co[k]["bands"] == 2 and not S.forwarded(co[k]) and S.plan(co[k], 2) == (2, 1) and S.form(co[k]).startswith("k_lif_step_slab")
    sh = {c["id"][len("slab-sh-"):]: c for c in BY["shapes"]}
    assert {(sh[k]["kh"], sh[k]["kw"]) for k in ("k1x1", "k2x5", "k7x7", "k9x9", "p4x4")} == {(1, 1), (2, 5), (7, 7), (9, 9), (3, 3)}
    assert (sh["p4x4"]["h"], sh["p4x4"]["w"]) == (4, 4)
    for k, n in (("band9", 9), ("band32", 32), ("band33", 33)):
        nb = S.plan(sh[k], sh[k]["B"])[0]
        assert {wg["NPb"] for wg in S.b_operand_reads(sh[k], nb)} == {n}
    assert S.paired(sh["tiles8"], 0, 1, 64) and S.paired(sh["tiles5"], 0, 1, 64) and not S.paired(sh["tiles5"], 0, 1, 6)
    assert not S.paired(sh["band32"], 0, 2, 64)
    assert {(c["pool_h"], c["pool_w"]) for c in BY["shapes"]} >= {(1, 1), (2, 2), (3, 3), (1, 2), (3, 2)}
    for k in ("pool2", "pool3"):        # floor-mode leftovers: the last band owns conv rows behind the last window
        c = sh[k]
        ch, _, ph, _ = FZ.conv_shape(c)
        nb = S.plan(c, c["B"])[0]
        assert ph * c["pool_h"] - (c["pool_h"] - 1) // 2 < ch == S.band_plan(c, nb - 1, nb)["C1"] and nb > 1
    assert {S.plan(c, c["B_run"])[0] for c in BY["shapes"]} >= {1, 2, 3, 5} and sh["p5x7"]["bands"] == FZ.conv_shape(sh["p5x7"])[2]
    assert any(c["bands"] == 0 and S.plan(c, c["B_run"])[0] > 1 for c in CASES)
    op = {c["id"][len("slab-opt-"):]: c for c in BY["options"]}
    assert not op["plain"]["refractory"] and not op["bias0"]["bias"] and not op["v-null"]["want_v"] and op["misalign"]["misalign"]
    assert (op["tau-scalar"]["tau_tensor"], op["tau-tensor"]["tau_tensor"]) == (0, 1)
    for c in BY["rule"]:
        ns_ = len(S.slabs(c))
        a, b = S.CUS // (c["B_run"] * ns_), S.CUS // (c["also_B"] * ns_)
        assert b == a + 1 and c["also_B"] == c["B_run"] - 1 and (S.plan(c, c["B_run"]), S.plan(c, c["also_B"])) == ((a, ns_), (b, ns_))
    assert sorted((len(S.slabs(c)), S.plan(c, c["B_run"])[0]) for c in BY["rule"]) == [(n, k) for n in (2, 3) for k in (1, 2, 3, 4)]
    g = BY["grid"][0]
    assert (g["c_out"], g["h"], g["w"], g["B"], g["B_run"]) == (65, 4, 4, 3, 300)
    assert [c["c_out"] for c in BY["forwarded"]] == [40, 64] and all(S.forwarded(c) and S.plan(c, 2) == (0, 0) for c in BY["forwarded"])
    assert sum(S.forwarded(c) for c in CASES) == 2
    free = BY["free"]
    assert min(c["c_out"] for c in free) >= 65 and max(c["c_out"] for c in free) <= 200 and {len(S.slabs(c)) for c in free} == {2, 3, 4}
    assert {c["bands"] for c in free} == {0, 1, 2, 3} and {c["pool_h"] for c in free} == {1, 2, 3}
    for key in ("refractory", "tau_tensor", "bias", "want_v", "readout", "state0"):
        assert {c[key] for c in free} == {0, 1}, key
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX for c in free)


def test_the_cases_reach_every_form():
    forms = collections.Counter(S.form(c, c["B_run"]) for c in CASES if not S.forwarded(c))
    assert set(forms) == set(S.all_forms()) == {S.form(c, c["B_run"]) for c in BY["forms"]}
    for c in CASES:
        log = S.launch_log(c, c["B_run"])
        if S.forwarded(c):
            assert log[0] == "k_step_wide_wprep" and log[-1].startswith("k_lif_step_wide")
        else:
            assert log == ["k_step_slab_wprep", "k_trace", S.form(c, c["B_run"])]
    print("cases per form:", dict(forms))


def test_the_library_answers_agree_with_the_restated_ones():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the functions are host-only)
    assert lib.dcll_version() == 10
    nb, ns = ctypes.c_int32(-1), ctypes.c_int32(-1)
    codes = {"DCLL_ERR_INVALID": _lib.DCLL_ERR_INVALID, "DCLL_ERR_UNSUPPORTED": _lib.DCLL_ERR_UNSUPPORTED}
    for c in CASES:
        d = _desc(c)
        ph = FZ.conv_shape(c)[2]
        assert int(lib.dcll_conv_lif_step_slab_scratch(ctypes.byref(d))) == S.scratch_floats(c) == ops.step_slab_scratch(d) > 0
        for B in {c["B_run"], c["also_B"] or c["B_run"], 1, 64, 512}:
            for bands in {c["bands"], 0, 1, 2, 3, ph, ph + 1}:
                want = S.plan(c, B, bands)
                rc = lib.dcll_conv_lif_step_slab_plan(ctypes.byref(d), B, bands, ctypes.byref(nb), ctypes.byref(ns))
                got = int(lib.dcll_conv_lif_step_slab_lds(ctypes.byref(d), B, bands))
                assert got == S.lds_bytes(c, B, bands) <= S.LDS_MAX, (S.describe(c), B, bands)
                if isinstance(want[0], int):
                    assert rc == 0 and (nb.value, ns.value) == want and got > 0, (S.describe(c), B, bands, want)
                    assert ops.step_slab_plan(d, B, bands) == want and ops.step_slab_supported(d, B, bands)
                else:
                    assert rc == codes[want[0]] and got == 0 and want[1] in lib.dcll_last_error().decode(), (S.describe(c), B, bands)
        if S.forwarded(c):          # the forwarding rule: dcll_conv_lif_step_wide's value
            assert S.lds_bytes(c, c["B_run"]) == ops.step_wide_lds(d) > 0
    for c in REFUSE:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_slab_lds(ctypes.byref(d), max(c["B"], 1), c["bands"]))
        assert got == S.lds_bytes(c, max(c["B"], 1)), S.describe(c)
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert got == 0 and c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
            assert S.served(c, c["B"]) == (c["code"], c["phrase"])


def test_the_older_entry_points_still_refuse():
    from snn_modulation_classification_amd import _lib
    lib = _lib.get()
    d = _desc(S.by_id("slab-co-cout65"))
    assert int(lib.dcll_conv_lif_step_wide_lds(ctypes.byref(d))) == 0 == int(lib.dcll_conv_lif_step_wide_scratch(ctypes.byref(d)))
    assert "c_out <= 64" in lib.dcll_last_error().decode()
    assert int(lib.dcll_conv_lif_step_any_lds(ctypes.byref(d))) == 0 and "c_out <= 32" in lib.dcll_last_error().decode()
    d = _desc(S.by_id("slab-radio2-24x40-l2"))
    assert int(lib.dcll_conv_lif_step_wide_lds(ctypes.byref(d))) == 0 and "160 KiB" in lib.dcll_last_error().decode()


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("slab-refuse-"):]: c for c in REFUSE}
    assert {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"} == {
        "stride2", "dilation2", "groups2", "k17", "bands-above-ph", "bands1-cin85", "bands1-radio4", "radio2-128x128"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"} == {"bands-negative", "null-x", "null-W", "null-scratch", "no-arp",
                                                                             "B-negative"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"B0", "B0-unsupported"}
    assert S.nb_fit(by["radio2-128x128"]) is None and S.nb_fit(by["bands1-radio4"]) == 2


@pytest.mark.parametrize("ref", REFUSE, ids=[r["id"] for r in REFUSE])
def test_refusals_return_before_anything_is_looked_at(ref):
    """every refusal returns its code and message on the host, before the first launch and before any operand is read: the call
    is made here, without a GPU, on small host buffers that stand in for the operands"""
    from snn_modulation_classification_amd import _lib
    r = ref
    lib = _lib.get()
    d = _desc(r)
    buf = np.zeros(64, np.float32)
    p = lambda k: None if r["null"] == k else ctypes.c_void_p(buf.ctypes.data)
    rc = lib.dcll_conv_lif_step_slab(ctypes.byref(d), p("x"), p("W"), p("b"), p("alpha"), p("tau_m"), p("alphas"), p("tau_s"), p("eps0"),
                                     p("eps1"), p("arp"), None, None, None, None, p("s"), None, None, p("pv"), p("v"), p("w_scratch"),
                                     r["bands"], r["B"], None)
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode() and "dcll_conv_lif_step_slab" in lib.dcll_last_error().decode()
    assert not buf.any()


def _assert_partition(c, NB):
    ch, cw, ph, pw = FZ.conv_shape(c)
    conv, pool = collections.Counter(), collections.Counter()
    for k in range(NB):
        r = S.band_plan(c, k, NB)
        assert r["P0"] < r["P1"] and r["C0"] < r["C1"], (S.describe(c), NB, k)
        conv.update(range(r["C0"], r["C1"]))
        pool.update(range(r["P0"], r["P1"]))
        pph = (c["pool_h"] - 1) // 2
        for py in range(r["P0"], r["P1"]):      # every window of an owned pooled row, clipped to the plane, lies in the band
            ys = [y for y in range(py * c["pool_h"] - pph, (py + 1) * c["pool_h"] - pph) if 0 <= y < ch]
            assert ys and r["C0"] <= ys[0] and ys[-1] < r["C1"]
    assert conv == collections.Counter(range(ch)) and pool == collections.Counter(range(ph)), (S.describe(c), NB)


def test_the_bands_partition_the_rows_for_ph_1_to_40():
    """conv rows and pooled rows exactly once, for every pooling 1 .. 3, every ph 1 .. 40 (with and without floor-mode leftovers) and
    every band count"""
    seen = set()
    for pool in (1, 2, 3):
        for ch in range(1, 40 * pool + pool):
            c = dict(FZ.CONV_DEFAULT, c_in=1, c_out=65, h=ch, w=4, kh=3, kw=3, pad_h=1, pad_w=1, pool_h=pool, pool_w=1)
            shp = FZ.conv_shape(c)
            if shp is None or shp[2] > 40:
                continue
            seen.add(shp[2])
            for NB in range(1, shp[2] + 1):
                _assert_partition(c, NB)
    assert seen == set(range(1, 41))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_indices_stay_in_bounds(case):
    c = case
    _, cw, _, _ = FZ.conv_shape(c)
    sl = S.slabs(c)
    # the slabs partition [0, c_out): consecutive, none empty, at most 64 rows, only the last may be short
    assert sl[0][0] == 0 and sl[-1][0] + sl[-1][1] == c["c_out"] and all(0 < n <= 64 for _, n in sl)
    assert all(sl[i][0] + sl[i][1] == sl[i + 1][0] and sl[i][1] == 64 for i in range(len(sl) - 1))
    for NB in band_counts(c):
        _assert_partition(c, NB)
        for k, wg in enumerate(S.b_operand_reads(c, NB)):
            # every B-operand offset stays inside the band's staged rows, which with the v plane and the bias are the LDS formula
            assert 0 <= wg["lo"] and wg["hi"] < wg["staged"], (S.describe(c), NB, k)
            assert wg["staged"] + (64 * wg["NPb"] if S.pooled(c) else 0) + 64 == S.lds_floats(c, k, NB) <= S.LDS_MAX // 4
            # ragged lanes are clamped to a valid pixel; lanes of the band keep their own
            assert all(0 <= pc < wg["NPb"] and (pc == pix or (pix >= wg["NPb"] and pc == wg["NPb"] - 1)) for pix, pc in wg["pcs"])


def _same(a, b, keys):
    return all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for x, y in zip(a, b) for k in keys)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_not_vacuous_and_the_decomposition_is_the_layer(case):
    c = case
    T, osteps = S.run(c)        # (asserts: a trajectory with spikes and silence in every (band, slab), within RESEED_CAP sub-seeds)
    assert 0 <= T["reseeds"] < S.RESEED_CAP == 6
    own = S.run_nb(c)
    assert FZ.vacuous(c, osteps) is None and S.part_vacuous(c, osteps, own) is None, S.describe(c)
    ch, cw, ph, pw = FZ.conv_shape(c)
    assert len(osteps) == FZ.STEPS == 3
    for st in osteps:
        assert st["v"].shape == (c["B"], c["c_out"], ch, cw) and st["s"].shape == (c["B"], c["c_out"], ph, pw)
    assert (T["b"] is None) == (not c["bias"]) and T["q8"] is None
    whole = [dict(v=st["v"], s=st["s"], arp=st["arp"], eps0=st["eps0"], eps1=st["eps1"]) for st in osteps]
    keys = ("v", "s", "eps0", "eps1") + (("arp",) if c["refractory"] else ())
    for NB in sorted({own, min(2, ph), ph} if FZ.conv_work(c) <= FZ.WORK_MAX else {own}):
        if S.lds_max(c, NB) * 4 > S.LDS_MAX:
            continue
        assert _same(S.sliced_oracle(c, T, osteps, NB), whole, keys), (S.describe(c), NB, "band by band, slab by slab != the layer")
    for m in S.MUTANTS:
        touches = S.mutant_touches(c, own, m)
        if m == "halo-short" and touches:       # ... and the dropped row carries a trace at some step
            rows = [S.band_plan(c, k, own)["C1"] - c["pad_h"] + c["kh"] - 2 for k in range(own)]
            touches = any(st["eps1"][:, :, y].any() for st in osteps for y in rows if 0 <= y < c["h"])
        if touches:
            assert not _same(S.sliced_oracle(c, T, osteps, own, mutant=m), whole, ("v",)), (S.describe(c), m, "not caught")
