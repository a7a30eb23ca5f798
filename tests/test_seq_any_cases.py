"""CPU self-check of tests/seq_any_cases.py: the case lists of dcll_conv_lif_sequence_any's differential test are proven here
before tests/test_gpu_seq_any.py lets them judge the kernel.

  - the seed reproduces the lists exactly and the strata hold what they promise;
  - every running case satisfies dcll_conv_lif_sequence_any_lds(d) > 0 — the library's own (host-only) predicate — with the byte
    count the module restates, every UNSUPPORTED refusal gives 0, and the weight scratch is the restated size;
  - the restated dispatch reaches every template variant of k_lif_seq_any;
  - the plane packer's word layout is what a plain loop over pixels writes (hw = 169, 81, 256);
  - the C oracle (OracleConvLayer) runs every case with a sound draw: the arbiter accepts all of them."""
import collections
import ctypes

import numpy as np
import pytest

import seq_any_cases as A

CASES = A.cases()
REFUSE = A.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)

# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "c5e79eedd6765f74c2bdc4db79ca1b433c91d27232ad61d4905851611538e1fb"
REFUSE_HASH = "5f57881d30c41286ede66bec3bb3ce4b2b84161033800b8147262e8bad246741"


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c.get("tau_tensor", 0), 1.0 if c["refractory"] else 0.0, A.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


def test_the_seed_reproduces_the_lists_exactly():
    assert A.cases_hash(A.cases()) == A.cases_hash(CASES) == CASES_HASH
    assert A.cases_hash(A.refusals()) == A.cases_hash(REFUSE) == REFUSE_HASH
    assert A.cases_hash(A.cases(A.SEED + 1)) != CASES_HASH
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(A.by_id(c["id"]) == c for c in CASES[::25] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=9, variants=6, boundaries=13, grids=1, free=104)
    named = {c["id"]: c for c in BY["named"]}
    # mnist_conv.yaml on 28x28: 16 / 24 / 32 channels, 7x7, pad 2, pooling 2 / 1 / 2 -> planes 28 -> 13 -> 11 (-> 4)
    geo = [(c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["pad_h"], c["pool_h"]) for c in (named["any-mnist-l%d" % i] for i in (1, 2, 3))]
    assert geo == [(1, 16, 28, 28, 7, 2, 2), (16, 24, 13, 13, 7, 2, 1), (24, 32, 11, 11, 7, 2, 2)]
    assert [A.out_shape(named["any-mnist-l%d" % i])[2:] for i in (1, 2, 3)] == [(13, 13), (11, 11), (4, 4)]
    for h, w in ((16, 16), (24, 24), (12, 32)):
        for c_in in (1, 32):
            c = named["any-radio-%dto32-%dx%d" % (c_in, h, w)]
            assert (c["c_out"], c["kh"], c["kw"], c["pad_h"], c["pad_w"], c["pool_h"], c["refractory"]) == (32, 7, 7, 3, 3, 1, 1)
    free = BY["free"]
    assert len(free) >= 100
    assert min(c["c_in"] for c in free) == 1 and max(c["c_in"] for c in free) >= 38 and any(c["c_in"] % 2 and c["c_in"] > 1 for c in free)
    assert min(c["c_out"] for c in free) <= 2 and max(c["c_out"] for c in free) == 32
    assert {c["kh"] for c in free} | {c["kw"] for c in free} == set(range(1, 10)) and any(c["kh"] != c["kw"] for c in free)
    assert {c["pad_h"] for c in free} == {c["pad_w"] for c in free} == set(range(5))
    shrink = [c for c in free if A.out_shape(c)[0] < c["h"] or A.out_shape(c)[1] < c["w"]]
    grow = [c for c in free if A.out_shape(c)[0] > c["h"] or A.out_shape(c)[1] > c["w"]]
    assert shrink and grow
    assert {c["pool_h"] for c in free} == {c["pool_w"] for c in free} == {1, 2, 3}
    for key in ("refractory", "tau_tensor", "bias"):
        assert {c[key] for c in free} == {0, 1}, key
    assert {t for c in free for t in c["Ts"]} >= set(range(1, 10)) and {c["B"] for c in free} == {1, 2, 3, 4, 5}
    assert any(len(c["Ts"]) == 2 and c["state0"] for c in free) and any(not c["state0"] for c in free)
    assert all(A.work(c) <= A.WORK_FREE_MAX for c in free)
    g = BY["grids"][0]
    assert (g["B"], g["Ts"], g["B_checked"]) == (1100, [6], 8) and (g["c_in"], g["c_out"], g["h"]) == (16, 24, 13)
    edge = {c["id"][len("any-edge-"):]: c for c in BY["boundaries"]}
    ref = {c["id"][len("any-refuse-"):]: c for c in REFUSE}
    # both sides of the LDS limit, of c_out = 32 and of the register form's limits
    assert A.lds_bytes(edge["lds-cin56"]) == 4 * 40928 <= A.LDS_MAX and A._sets(ref["lds-cin57"])[0] * 4 > A.LDS_MAX
    assert edge["cout32"]["c_out"] == 32 and ref["cout33"]["c_out"] == 33
    assert edge["regs-nin18432"]["c_in"] * 24 * 24 == A.KE * A.THREADS < ref["regs-nin19008"]["c_in"] * 24 * 24
    assert 24 * 32 == 32 * A.NW * A.QMAX < 24 * 33 and (edge["regs-cp768"]["w"], ref["regs-cp792"]["w"]) == (32, 33)


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("any-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported >= {"stride2", "dilation2", "groups2", "cout33", "lds-cin57"}
    assert invalid >= {"null-spk-in", "no-arp"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"T0", "B0", "T0-unsupported"}
    assert all(c["phrase"] for c in REFUSE if c["code"] != "DCLL_OK")
    assert by["no-arp"]["refractory"] == 1


def test_the_library_predicate_agrees_with_the_restated_one():
    from snn_modulation_classification_amd import _lib
    lib = _lib.get()                # (loads without a GPU; both functions are host-only)
    for c in CASES:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_sequence_any_lds(ctypes.byref(d)))
        assert got > 0 and got == A.lds_bytes(c) <= A.LDS_MAX, A.describe(c)
        assert int(lib.dcll_conv_lif_sequence_any_scratch(ctypes.byref(d))) == 64 * A.steps(c), A.describe(c)
    for c in REFUSE:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_sequence_any_lds(ctypes.byref(d)))
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert got == 0 == A.lds_bytes(c), A.describe(c)
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
        elif "unsupported" not in c["id"]:
            assert got > 0, A.describe(c)


def test_the_cases_reach_every_template_variant():
    var = collections.Counter(A.variant(c) for c in CASES)
    assert set(var) == set(A.all_variants()) and len(var) == 6
    assert {A.variant(c) for c in BY["variants"]} == set(A.all_variants())
    print("cases per variant:", dict(var))


@pytest.mark.parametrize("hw", [169, 81, 256])
def test_plane_packer_word_layout(hw):
    rng = np.random.RandomState(hw)
    dense = (rng.rand(3, 5, hw) < .4).astype(np.float32)
    got = A.pack_planes(dense)
    words = (hw + 31) // 32
    want = np.zeros((3, 5, words), np.uint32)
    for a in range(3):
        for b in range(5):
            for pix in range(hw):
                if dense[a, b, pix]:
                    want[a, b, pix // 32] |= np.uint32(1) << np.uint32(pix % 32)
    assert got.shape == (3, 5, words) and got.dtype == np.uint32 and np.array_equal(got, want)
    if hw % 32:
        assert not (got[..., -1] >> np.uint32(hw % 32)).any()            # tail bits are zero
    else:
        from conftest import unpack_bits
        assert np.array_equal(unpack_bits(got.view(np.uint8), hw), dense)  # the existing format when hw % 32 == 0
    assert np.array_equal(A.unpack_planes(got, hw), dense)
    assert np.array_equal(A.unpack_planes(got.view(np.int32), hw), dense)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_sound(case):
    c = case
    T, traj = A.run(c)                          # (asserts: accepted by the oracle, its shapes, a sound draw within 24 attempts)
    assert A.unsound(c, traj) is None, A.describe(c)
    assert len(traj) == len(c["Ts"]) == len(T["calls"])
    ch, cw, ph, pw = A.out_shape(c)
    for n, call in zip(c["Ts"], traj):
        assert call["v"].shape == (n, c["B_checked"], c["c_out"], ch, cw) and call["s"].shape == (n, c["B_checked"], c["c_out"], ph, pw)
    assert (T["b"] is None) == (not c["bias"])
    if not c["tau_tensor"]:
        assert all(np.all(t == t[0]) for t in T["tau"])
