"""CPU self-check of tests/step_wide_cases.py: the case list of dcll_conv_lif_step_wide's differential test is proven here before
tests/test_gpu_step_wide.py lets it judge the kernel.

  - the seed reproduces the lists and the strata hold what they promise;
  - the restated lds_bytes(c) / scratch_floats(c) equal dcll_conv_lif_step_wide_lds / _scratch — the library's own (host-only)
    functions — for every case and refusal, with the refusal's phrase in dcll_last_error();
  - every refusal returns its code and message on the host, before any launch; dcll_conv_lif_step_any still refuses c_out 33;
  - the restated dispatch reaches every form of k_lif_step_wide;
  - for every case, from the kernel's restated index arithmetic: the unit ranges partition [0, units) with no empty workgroup,
    every B-operand offset a lane can form stays inside the staged image (split form: inside the rows the workgroup stages),
    ragged lanes are clamped to a valid pixel;
  - the C oracle runs every case with a trajectory that is not vacuous for the SECOND M tile: a channel >= 32 spikes, a pixel of
    such a channel stays silent, a refractory layer's arp is non-zero before the last step."""
import collections
import ctypes

import numpy as np
import pytest

import fuzz_cases as FZ
import step_wide_cases as S

CASES = S.cases()
REFUSE = S.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)

# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "706b66e74e58a825e21653e047a5a7c1fe5c588d4348df924627d5d5e48042eb"
REFUSE_HASH = "e371eb3f181ff18600a8e6a3b2a86015e6319a2fa1b2b53a903531cd7cc24fbd"


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c["tau_tensor"], 1.0 if c["refractory"] else 0.0, FZ.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


def test_the_seed_reproduces_the_lists_exactly():
    assert S.cases_hash(S.cases()) == S.cases_hash(CASES) == CASES_HASH != S.cases_hash(S.cases(S.SEED + 1))
    assert S.cases_hash(S.refusals()) == S.cases_hash(REFUSE) == REFUSE_HASH
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(S.by_id(c["id"]) == c for c in CASES[::25] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=7, forms=6, mtile=28, split=9, limits=2, grid=1, forwarded=3, free=40)
    named = {c["id"]: c for c in BY["named"]}
    geo = lambda c: (c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["pad_h"], c["pool_h"], c["refractory"])
    assert [geo(named["wide-radio2-l%d" % l]) for l in (1, 2)] == [(1, 64, 16, 16, 7, 3, 1, 1), (64, 64, 16, 16, 7, 3, 1, 1)]
    assert [geo(named["wide-radio15-l%d" % l]) for l in (1, 2)] == [(1, 48, 16, 16, 7, 3, 1, 1), (48, 48, 16, 16, 7, 3, 1, 1)]
    assert [geo(named["wide-mnist2-l%d" % l]) for l in (1, 2, 3)] == [(1, 32, 28, 28, 7, 2, 2, 0), (32, 48, 13, 13, 7, 2, 1, 0),
                                                                      (48, 64, 11, 11, 7, 2, 2, 0)]
    assert S.forwarded(named["wide-mnist2-l1"]) and all(c["B"] <= 5 for c in BY["named"])
    # the issue's split counts of the 64 -> 64 layer: B = 64 -> 4, B = 128 -> 2, B >= 256 -> fused
    l2 = named["wide-radio2-l2"]
    assert (S.units(l2), S.ns(l2, 64), S.ns(l2, 128), S.ns(l2, 256), S.ns(l2, 2)) == (16, 4, 2, 1, 4)
    mt = {c["id"][len("wide-mt-"):]: c for c in BY["mtile"]}
    assert all(c["c_out"] > 32 and c["B"] <= 5 for c in BY["mtile"])
    assert [mt[k]["c_out"] for k in ("cout33", "cout40", "cout63", "cout64")] == [33, 40, 63, 64]
    assert (mt["cin1"]["c_in"], mt["cin5-zero-link"]["c_in"], mt["cin31"]["c_in"]) == (1, 5, 31)
    z = mt["cin5-zero-link"]
    assert (z["kh"] * z["kw"]) % 2 and S.steps(z) * 2 == z["c_in"] * z["kh"] * z["kw"] + 1
    assert (mt["k1x1"]["kh"], mt["k1x1"]["kw"], mt["k2x5"]["kh"], mt["k2x5"]["kw"]) == (1, 1, 2, 5)
    for n in (9, 32, 33, 64, 65):
        ch, cw, _, _ = FZ.conv_shape(mt["cp%d" % n])
        assert ch * cw == n
    assert [(mt[k]["pool_h"], mt[k]["pool_w"]) for k in ("pool2", "pool3", "pool3x2")] == [(2, 2), (3, 3), (3, 2)]
    assert not mt["bias0"]["bias"] and not mt["v-null"]["want_v"] and mt["misalign"]["misalign"] and mt["misalign-split"]["misalign"]
    assert (mt["tau-scalar"]["tau_tensor"], mt["tau-tensor"]["tau_tensor"]) == (0, 1)
    sp = {c["id"][len("wide-split-"):]: c for c in BY["split"]}
    assert (S.units(sp["units4"]), S.ns(sp["units4"], 2), S.units(sp["units6"]), S.ns(sp["units6"], 2)) == (4, 1, 6, 2)
    assert S.unit_ranges(sp["upw-odd"], 2) == [(0, 3), (3, 6)] and sp["upw-odd"]["c_out"] == 64
    assert S.unit_ranges(sp["upw-odd-5"], 51) == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 22)]
    assert S.unit_ranges(sp["upw-odd-5"], 52) == [(0, 6), (6, 12), (12, 18), (18, 22)]
    for k, want in (("ns-1to2", (1, 2)), ("ns-2to3", (2, 3)), ("ns-3to4", (3, 4)), ("ns-4to5", (4, 5))):
        c = sp[k]
        assert S.units(c) == 18 and (S.ns(c, c["B"]), S.ns(c, c["also_B"])) == want and c["also_B"] == c["B"] - 1
        assert S.CUS // c["B"] == want[0] and S.CUS // c["also_B"] == want[1]
    f = sp["radio2-l2-fused"]
    assert (f["B"], f["B_run"], S.ns(f, 257), S.form(f, 257)) == (2, 257, 1, "k_lif_step_wide<1>")
    lim = {c["id"][len("wide-limit-"):]: c for c in BY["limits"]}
    ref = {c["id"][len("wide-refuse-"):]: c for c in REFUSE}
    assert S.lds_bytes(lim["lds-cin126"]) == 4 * 40888 <= S.LDS_MAX < 4 * S.lds_floats(ref["lds-cin127"])
    assert S.lds_bytes(lim["lds-pool-cin75"]) == 4 * 40748 <= S.LDS_MAX < 4 * S.lds_floats(ref["lds-pool-cin76"])
    assert all(c["c_out"] == 64 for c in BY["limits"])
    g = BY["grid"][0]
    assert (g["c_out"], g["B"], g["B_run"]) == (40, 8, 1100)
    assert all(S.forwarded(c) for c in BY["forwarded"]) and {S.form(c, c["B_run"]) for c in BY["forwarded"]} == {
        "k_lif_step_any<1>", "k_lif_step_any<0> (pooling)", "k_lif_step_any<1> (split)"}
    free = BY["free"]
    assert min(c["c_out"] for c in free) >= 33 and max(c["c_out"] for c in free) == 64 and min(c["c_out"] for c in free) <= 36
    assert min(c["c_in"] for c in free) <= 2 and max(c["c_in"] for c in free) >= 36 and any(c["c_in"] % 2 and c["c_in"] > 1 for c in free)
    assert {c["kh"] for c in free} | {c["kw"] for c in free} == set(range(1, 10)) and any(c["kh"] != c["kw"] for c in free)
    assert {c["pad_h"] for c in free} == {c["pad_w"] for c in free} == set(range(5))
    assert {c["pool_h"] for c in free} == {c["pool_w"] for c in free} == {1, 2, 3}
    for key in ("refractory", "tau_tensor", "bias", "want_v", "readout", "state0"):
        assert {c[key] for c in free} == {0, 1}, key
    assert max(max(c["h"], c["w"]) for c in free) <= 22 and {c["B"] for c in free} <= {1, 2, 3, 4, 5}
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX for c in free)


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("wide-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported == {"cout65", "stride2", "dilation2", "groups2", "k17", "lds-cin127", "lds-pool-cin76", "lds-radio2-32x32"}
    assert invalid == {"null-x", "null-W", "null-scratch", "no-arp", "B-negative"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"B0", "B0-unsupported"}
    assert by["cout65"]["c_out"] == 65 and by["k17"]["kh"] == 17 and by["no-arp"]["refractory"] == 1 and by["B-negative"]["B"] < 0
    for k in unsupported:
        assert S.served(by[k]) == (by[k]["code"], by[k]["phrase"]), k


def test_the_library_predicate_agrees_with_the_restated_one():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the functions are host-only)
    assert lib.dcll_version() == 10
    for c in CASES:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_wide_lds(ctypes.byref(d)))
        assert got > 0 and got == S.lds_bytes(c) <= S.LDS_MAX, S.describe(c)
        assert ops.step_wide_lds(d) == got and ops.step_wide_supported(d)
        assert ops.step_wide_scratch(d) == int(lib.dcll_conv_lif_step_wide_scratch(ctypes.byref(d))) == S.scratch_floats(c), S.describe(c)
        if S.forwarded(c):          # the forwarding rule: the _any values
            assert got == ops.step_any_lds(d) and S.scratch_floats(c) == ops.step_any_scratch(d) == 64 * S.steps(c)
        else:
            assert S.scratch_floats(c) == 128 * S.steps(c) and not ops.step_any_supported(d)
    for c in REFUSE:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_wide_lds(ctypes.byref(d)))
        assert got == S.lds_bytes(c), S.describe(c)
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert got == 0 and not ops.step_wide_supported(d) and ops.step_wide_scratch(d) == 0 == S.scratch_floats(c)
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
        elif "unsupported" not in c["id"]:
            assert got > 0, S.describe(c)


def test_step_any_still_refuses_33_output_channels():
    from snn_modulation_classification_amd import _lib
    lib = _lib.get()
    d = _desc(S.by_id("wide-mt-cout33"))
    assert int(lib.dcll_conv_lif_step_any_lds(ctypes.byref(d))) == 0 == int(lib.dcll_conv_lif_step_any_scratch(ctypes.byref(d)))
    assert "c_out <= 32" in lib.dcll_last_error().decode()


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
    rc = lib.dcll_conv_lif_step_wide(ctypes.byref(d), p("x"), p("W"), p("b"), p("alpha"), p("tau_m"), p("alphas"), p("tau_s"), p("eps0"),
                                     p("eps1"), p("arp"), None, None, None, None, p("s"), None, None, p("pv"), p("v"), p("w_scratch"),
                                     r["B"], None)
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode() and "dcll_conv_lif_step_wide" in lib.dcll_last_error().decode()
    assert not buf.any()


def test_the_cases_reach_every_form_and_stratum():
    forms = collections.Counter(S.form(c, c["B_run"]) for c in CASES if not S.forwarded(c))
    assert set(forms) == set(S.all_forms()) and len(forms) == 6
    assert {S.form(c, c["B_run"]) for c in BY["forms"]} == set(S.all_forms())
    assert set(BY) == {"named", "forms", "mtile", "split", "limits", "grid", "forwarded", "free"}
    for c in CASES:
        log = S.launch_log(c, c["B_run"])
        assert log[0] == ("k_seq_any_wprep" if S.forwarded(c) else "k_step_wide_wprep") and log[-1] == S.form(c, c["B_run"])
        assert ("k_trace" in log) == log[-1].endswith("(split)")
    print("cases per form:", dict(forms))


WIDE = [c for c in CASES if not S.forwarded(c)]


@pytest.mark.parametrize("case", WIDE, ids=[c["id"] for c in WIDE])
def test_kernel_indices_stay_in_bounds(case):
    c = case
    ch, cw, _, _ = FZ.conv_shape(c)
    CP, WP = ch * cw, c["w"] + 2 * c["pad_w"]
    for B in {c["B_run"], c["also_B"] or c["B_run"]}:
        rng_ = S.unit_ranges(c, B)
        # the unit ranges partition [0, units): consecutive, none empty, first at 0, last at the unit count
        assert rng_[0][0] == 0 and rng_[-1][1] == S.units(c) and len(rng_) == S.ns(c, B)
        assert all(a < b for a, b in rng_) and all(rng_[k][1] == rng_[k + 1][0] for k in range(len(rng_) - 1))
        assert len(rng_) == 1 or (not S.pooled(c) and len(rng_) * B <= S.CUS and S.units(c) > S.SPLIT_UNITS)
        for wg in S.b_operand_reads(c, B):
            # every B-operand offset stays inside the staged image
            assert 0 <= wg["lo"] and wg["hi"] < wg["image"] and wg["image"] * 4 + 256 <= S.lds_bytes(c), S.describe(c)
            # ragged lanes are clamped to a valid pixel; lanes of the plane keep their own
            assert all(0 <= pc < CP and (pc == pix or (pix >= CP and pc == CP - 1)) for pix, pc in wg["pcs"])
            # the padded rows the workgroup's windows touch are rows it stages
            assert wg["staged"][0] <= wg["rows"][0] and wg["rows"][1] <= wg["staged"][1] <= c["h"] + 2 * c["pad_h"] - 1
            assert wg["hi"] < (wg["staged"][1] + 1) * WP + (c["c_in"] - 1) * (c["h"] + 2 * c["pad_h"]) * WP


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_not_vacuous(case):
    c = case
    T, osteps = S.run(c)                        # (asserts: accepted by the oracle, its shapes, a non-vacuous draw in 24 attempts)
    assert FZ.vacuous(c, osteps) is None, S.describe(c)
    assert S.second_tile_vacuous(c, T, osteps) is None, (S.describe(c), S.second_tile_vacuous(c, T, osteps))
    ch, cw, ph, pw = FZ.conv_shape(c)
    assert len(osteps) == FZ.STEPS == 3
    for st in osteps:
        assert st["v"].shape == (c["B"], c["c_out"], ch, cw) and st["s"].shape == (c["B"], c["c_out"], ph, pw)
    assert (T["b"] is None) == (not c["bias"]) and T["q8"] is None
    assert c["state0"] == int(bool(np.any(T["eps1"])))
