"""CPU self-check of tests/step_any_cases.py: the case list of dcll_conv_lif_step_any's differential test is proven here before
tests/test_gpu_step_any.py lets it judge the kernel.

  - the seed reproduces the lists exactly and the strata hold what they promise;
  - the restated lds_bytes(c) equals dcll_conv_lif_step_any_lds — the library's own (host-only) predicate — for every case and
    refusal, with the refusal's phrase in dcll_last_error();
  - every refusal returns its code and message on the host, before any launch;
  - the restated dispatch reaches every form of k_lif_step_any;
  - for every case, from the kernel's restated index arithmetic: the largest B-operand offset a lane can form stays inside the
    staged image (and, in the split form, inside the rows the workgroup stages), ragged lanes are clamped to a valid pixel,
    and the split form's tile ranges partition the tiles;
  - the C oracle (OracleConvLayer) runs every case with a non-vacuous trajectory."""
import collections
import ctypes

import numpy as np
import pytest

import fuzz_cases as FZ
import step_any_cases as S

CASES = S.cases()
REFUSE = S.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)

# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "bd0b325f99865521700b8301a4a0eb6a6f54a65ce14ea770e25d78e2069f926c"
REFUSE_HASH = "79dbce7783d4f6cafb89b1a3718441b9987ca4dc4c4d5650c3c6b3271e38ba54"


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c["tau_tensor"], 1.0 if c["refractory"] else 0.0, FZ.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


def test_the_seed_reproduces_the_lists_exactly():
    assert S.cases_hash(S.cases()) == S.cases_hash(CASES) == CASES_HASH
    assert S.cases_hash(S.refusals()) == S.cases_hash(REFUSE) == REFUSE_HASH
    assert S.cases_hash(S.cases(S.SEED + 1)) != CASES_HASH
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(S.by_id(c["id"]) == c for c in CASES[::25] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=9, forms=6, boundaries=33, grid=1, free=60)
    named = {c["id"]: c for c in BY["named"]}
    geo = [(c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["pad_h"], c["pool_h"], c["refractory"], c["tau_tensor"], c["B"])
           for c in (named["step-mnist-l%d" % i] for i in (1, 2, 3))]
    assert geo == [(1, 16, 28, 28, 7, 2, 2, 0, 1, 2), (16, 24, 13, 13, 7, 2, 1, 0, 1, 2), (24, 32, 11, 11, 7, 2, 2, 0, 1, 2)]
    assert [FZ.conv_shape(named["step-mnist-l%d" % i])[2:] for i in (1, 2, 3)] == [(13, 13), (11, 11), (4, 4)]
    for h, w in ((16, 16), (24, 24), (12, 32)):
        for c_in in (1, 32):
            c = named["step-radio-%dto32-%dx%d" % (c_in, h, w)]
            assert (c["c_out"], c["kh"], c["kw"], c["pad_h"], c["pad_w"], c["pool_h"], c["refractory"], c["B"]) == (32, 7, 7, 3, 3, 1, 1, 2)
    # radio_ml_conv.yaml's 32 -> 32 layer on 24x24: 18 tiles, three workgroups of six
    assert S.tile_ranges(named["step-radio-32to32-24x24"], 2) == [(0, 6), (6, 12), (12, 18)]
    free = BY["free"]
    assert min(c["c_in"] for c in free) == 1 and max(c["c_in"] for c in free) >= 36 and any(c["c_in"] % 2 and c["c_in"] > 1 for c in free)
    assert min(c["c_out"] for c in free) <= 2 and max(c["c_out"] for c in free) >= 31
    assert {c["kh"] for c in free} | {c["kw"] for c in free} == set(range(1, 10)) and any(c["kh"] != c["kw"] for c in free)
    assert {c["pad_h"] for c in free} == {c["pad_w"] for c in free} == set(range(5))
    assert {c["pool_h"] for c in free} == {c["pool_w"] for c in free} == {1, 2, 3}
    for key in ("refractory", "tau_tensor", "bias", "want_v", "readout", "state0"):
        assert {c[key] for c in free} == {0, 1}, key
    assert max(max(c["h"], c["w"]) for c in free) == 22 and {c["B"] for c in free} <= {1, 2, 3, 4, 5}
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX for c in free)
    g = BY["grid"][0]
    assert (g["B"], g["B_run"]) == (8, 1100)
    edge = {c["id"][len("step-edge-"):]: c for c in BY["boundaries"]}
    ref = {c["id"][len("step-refuse-"):]: c for c in REFUSE}
    # both sides of the LDS limit, with and without pooling
    assert S.lds_bytes(edge["lds-cin126"]) == 4 * 40856 <= S.LDS_MAX < 4 * S.lds_floats(ref["lds-cin127"])
    assert S.lds_bytes(edge["lds-pool-cin101"]) == 4 * 40948 <= S.LDS_MAX < 4 * S.lds_floats(ref["lds-pool-cin102"])
    assert (edge["cout1"]["c_out"], edge["cout31"]["c_out"], edge["cout32"]["c_out"], ref["cout33"]["c_out"]) == (1, 31, 32, 33)
    assert (edge["cin1"]["c_in"], edge["cin3"]["c_in"], edge["cin31"]["c_in"]) == (1, 3, 31)
    z = edge["zero-link"]
    assert z["c_in"] % 2 and (z["kh"] * z["kw"]) % 2 and S.steps(z) * 2 == z["c_in"] * z["kh"] * z["kw"] + 1
    assert (edge["k16"]["kh"], edge["k16"]["kw"], ref["k17"]["kh"]) == (16, 16, 17)
    assert FZ.conv_shape(edge["k1x1-plane1x1"]) == (1, 1, 1, 1)
    assert FZ.conv_shape(edge["pad-grows"])[0] > edge["pad-grows"]["h"] and FZ.conv_shape(edge["pad0-shrinks"])[0] < edge["pad0-shrinks"]["h"]
    assert FZ.conv_shape(edge["cp33"])[0] * FZ.conv_shape(edge["cp33"])[1] == 33 and S.tiles(edge["cp33"]) == 2
    assert (edge["pool3"]["pool_h"], edge["pool3"]["pool_w"]) == (3, 3)
    assert (edge["pool2x3-shrinks"]["pool_h"], edge["pool2x3-shrinks"]["pool_w"]) == (2, 3)
    assert not edge["bias0"]["bias"] and not edge["v-null"]["want_v"] and edge["misalign"]["misalign"]
    # both sides of the NS thresholds: tiles against the waves of a workgroup, 256 / B against 2 and 3
    assert (S.tiles(edge["tiles8"]), S.ns(edge["tiles8"], 2)) == (8, 1) and (S.tiles(edge["tiles9"]), S.ns(edge["tiles9"], 2)) == (9, 2)
    assert S.tile_ranges(edge["tiles9"], 2) == [(0, 5), (5, 9)] and S.tile_ranges(edge["tiles17"], 2) == [(0, 6), (6, 12), (12, 17)]
    nb = edge["ns-batch"]
    assert (nb["B"], nb["also_B"], S.ns(nb, 129), S.ns(nb, 128)) == (129, 128, 1, 2)
    nb = edge["ns-batch-3to2"]
    assert (S.ns(nb, nb["B"]), S.ns(nb, nb["also_B"])) == (2, 3)


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("step-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported == {"stride2", "dilation2", "groups2", "cout33", "k17", "lds-cin127", "lds-pool-cin102", "lds-radio-32x32",
                           "lds-radio-24x24-pool2"}
    assert invalid == {"null-x", "null-eps1", "null-W", "null-scratch", "no-arp", "B-negative"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"B0", "B0-unsupported"}
    assert all(c["phrase"] for c in REFUSE if c["code"] != "DCLL_OK")
    assert by["no-arp"]["refractory"] == 1 and by["B-negative"]["B"] < 0
    for k in unsupported:
        assert S.served(by[k]) == (by[k]["code"], by[k]["phrase"]), k


def test_the_library_predicate_agrees_with_the_restated_one():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the function is host-only)
    assert lib.dcll_version() == 10
    for c in CASES:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_any_lds(ctypes.byref(d)))
        assert got > 0 and got == S.lds_bytes(c) <= S.LDS_MAX, S.describe(c)
        assert ops.step_any_lds(d) == got and ops.step_any_supported(d)
        assert ops.step_any_scratch(d) == int(lib.dcll_conv_lif_step_any_scratch(ctypes.byref(d))) == 64 * S.steps(c), S.describe(c)
    for c in REFUSE:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_any_lds(ctypes.byref(d)))
        assert got == S.lds_bytes(c), S.describe(c)
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert got == 0 and not ops.step_any_supported(d)
            assert ops.step_any_scratch(d) == 0
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
        elif "unsupported" not in c["id"]:
            assert got > 0, S.describe(c)


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
    rc = lib.dcll_conv_lif_step_any(ctypes.byref(d), p("x"), p("W"), p("b"), p("alpha"), p("tau_m"), p("alphas"), p("tau_s"), p("eps0"),
                                    p("eps1"), p("arp"), None, None, None, None, p("s"), None, None, p("pv"), p("v"), p("w_scratch"),
                                    r["B"], None)
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode() and "dcll_conv_lif_step_any" in lib.dcll_last_error().decode()
    assert not buf.any()


def test_the_cases_reach_every_form():
    forms = collections.Counter(S.form(c, c["B_run"]) for c in CASES)
    assert set(forms) == set(S.all_forms()) and len(forms) == 6
    assert {S.form(c, c["B_run"]) for c in BY["forms"]} == set(S.all_forms())
    for c in CASES:
        log = S.launch_log(c, c["B_run"])
        assert log[0] == "k_seq_any_wprep" and log[-1] == S.form(c, c["B_run"]) and (("k_trace" in log) == log[-1].endswith("(split)"))
    print("cases per form:", dict(forms))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_indices_stay_in_bounds(case):
    c = case
    ch, cw, _, _ = FZ.conv_shape(c)
    CP, WP = ch * cw, c["w"] + 2 * c["pad_w"]
    for B in {c["B_run"], c["also_B"] or c["B_run"]}:
        rng_ = S.tile_ranges(c, B)
        # the split form's tile ranges partition the tiles: consecutive, none empty, first at 0, last at the tile count
        assert rng_[0][0] == 0 and rng_[-1][1] == S.tiles(c) and len(rng_) == S.ns(c, B)
        assert all(a < b for a, b in rng_) and all(rng_[k][1] == rng_[k + 1][0] for k in range(len(rng_) - 1))
        assert len(rng_) == 1 or (not S.pooled(c) and len(rng_) * B <= S.CUS)
        for wg in S.b_operand_reads(c, B):
            # the largest B-operand offset stays inside the staged image
            assert 0 <= wg["lo"] and wg["hi"] < wg["image"] and wg["image"] * 4 + 128 <= S.lds_bytes(c), S.describe(c)
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
    ch, cw, ph, pw = FZ.conv_shape(c)
    assert len(osteps) == FZ.STEPS == 3
    for st in osteps:
        assert st["v"].shape == (c["B"], c["c_out"], ch, cw) and st["s"].shape == (c["B"], c["c_out"], ph, pw)
    assert (T["b"] is None) == (not c["bias"]) and T["q8"] is None
    assert c["state0"] == int(bool(np.any(T["eps1"])))
