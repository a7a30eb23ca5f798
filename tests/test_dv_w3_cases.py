"""CPU self-check of tests/dv_w3_cases.py: the case list of the differential tests of dcll_conv_lif_backward_w3_ex[_open] with
DCLL_W3_DV (k_bwd_dv_w3) is proven here before tests/test_gpu_dv_w3.py lets it judge the kernel.

  - the seed reproduces the list, ids are unique, and the list holds every stratum the issue names: the planes (w = 2 and K = 1024
    among them), both channel counts, the batches around a workgroup's chunk, the readout widths with the fallback at 33, the eight
    gradient selections with the product's call, both alignments of each of the five pointers, the three draws;
  - the restated predicate agrees with step_w3_cases.served, the grid covers every pooled position and sample exactly once;
  - the near-tie draw does what it is for: at least a quarter of its pairs have EQUAL float32 sigmoids with the larger v on the right;
  - a float32 restatement of the dv formula stays within rtol 1e-5 / atol 1e-6 max|ref| of the float64 reference on the grid draws;
  - the refusals of the two entry points on the host, before any launch; the binding declares both symbols."""
import ctypes

import numpy as np
import pytest

import dv_w3_cases as C
import fuzz_cases as FZ
import step_w3_cases as S

CASES = C.cases()
BY = {c["id"]: c for c in CASES}
GRID = [c for c in CASES if c["draw"] == "grid"]


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), c["target"], bool(c["output_layer"]), c["tau_tensor"],
                              1.0 if c["refractory"] else 0.0, FZ.ALPHARP, c["stride"], c["dilation"], c["groups"])


def test_the_seed_reproduces_the_list_and_ids_are_unique():
    assert C.cases_hash(C.cases()) == C.cases_hash(CASES) != C.cases_hash(C.cases(C.SEED + 1))
    assert len(BY) == len(CASES) == 38 and all(C.by_id(c["id"]) == c for c in CASES[::7])
    # the list is pinned: a change of the generator or of a seed shows here
    assert C.cases_hash(CASES) == "3142af9462a5dde7cd783017363af5c126bac33fbef00a8e00b5c76ae19aa0ee"


def test_the_list_holds_every_stratum_the_issue_names():
    assert all(S.served(c) is None and c["c_out"] == 64 for c in CASES)
    assert {(c["h"], c["w"]) for c in CASES} == {(16, 2), (1, 32), (2, 16), (1, 256), (4, 64), (16, 128)}
    assert all(c["B"] <= 3 for c in CASES if (c["h"], c["w"]) == (16, 128))
    assert any(c["w"] == 2 for c in CASES) and any(C.K(c) == 1024 for c in CASES) and all(C.K(c) % 1024 == 0 for c in CASES)
    pb = C.PER_BLOCK
    for hw in C.PLANES:
        assert {c["B"] for c in CASES if (c["h"], c["w"]) == hw} >= {1, 3, pb - 1, pb, pb + 1, 33}, hw
    assert {c["c_in"] for c in CASES} == {1, 64}
    for ci in (1, 64):
        assert {c["B"] for c in CASES if c["c_in"] == ci} >= {1, pb - 1, pb, pb + 1, 33}, ci
    assert {c["target"] for c in CASES} == {1, 8, 9, 10, 24, 32, 33}
    assert {C.NP(c) for c in CASES if C.served(c)} == {8, 16, 24, 32}
    # every gradient selection with and without g_v; the product's call (g_p only) on the product's plane
    assert {(c["gsel"], c["with_gv"]) for c in CASES} == {(g, v) for g in C.GSEL for v in (0, 1)}
    assert any((c["h"], c["w"], c["gsel"], c["with_gv"]) == (16, 128, "g_p", 0) for c in CASES)
    # both alignments of each pointer, while it is passed
    for bit, key in ((C.OFF_V, None), (C.OFF_SCRATCH, None), (C.OFF_GV, "g_v"), (C.OFF_GPV, "g_pv"), (C.OFF_W, "i2o_W")):
        for want in (0, bit):
            assert any(c["off"] & bit == want and (key is None or C.passed(c)[key]) for c in CASES), (bit, want)
        # ... and alone: the only pointer off its boundary selects the scalar form
        assert any(c["off"] == bit and (key is None or C.passed(c)[key]) and C.served(c) and not C.vector_form(c) for c in CASES), bit
    assert {c["draw"] for c in CASES} == set(C.DRAWS)
    for d in C.DRAWS:                                                       # every draw with and without the readout sum
        assert {C.passed(c)["g_p"] for c in CASES if c["draw"] == d} == {False, True}, d
    assert {c["first"] for c in CASES} == {0, 1} and {(c["first"], c["c_in"]) for c in CASES} == {(0, 1), (0, 64), (1, 1), (1, 64)}
    assert {c["scratch"] for c in CASES} == {"ops", "k1"} and {c["output_layer"] for c in CASES} == {0, 1}
    # the fallback: target 33 keeps k_bwd_dv; every kernel form is predicted for some case in one of its two alignments
    assert [C.form_name(c) for c in CASES if c["target"] == 33] == ["k_bwd_dv"] * sum(c["target"] == 33 for c in CASES) != []
    forms = {C.form_key(c, off) for c in CASES if C.served(c) for off in (c["off"], c["off"] ^ 31)}
    assert forms == set(C.all_forms()), set(C.all_forms()) - forms


def test_the_restated_predicate_agrees_with_the_step_predicate():
    base = CASES[0]
    for kw in (dict(), dict(c_out=32), dict(pool_w=1), dict(h=1, w=16), dict(h=1, w=512), dict(kw=5, pad_w=2), dict(c_in=32)):
        for target in (1, 32, 33):
            r = dict(base, target=target, **kw)
            assert C.served(r) == (S.served(r) is None and target <= 32), (kw, target)
    from snn_modulation_classification_amd import ops
    for c in CASES:
        assert ops.backward_w3_supported(_desc(c)) and (C.form_name(c) != "k_bwd_dv") == (c["target"] <= 32)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_the_grid_covers_every_pooled_position_of_every_sample_once(case):
    c = case
    gx, gy = C.grid(c)
    Kc, B = C.K(c), c["B"]
    assert gx * C.POS == Kc and (gy - 1) * C.PER_BLOCK < B <= gy * C.PER_BLOCK and gy <= 65535
    count = np.zeros((B, Kc), np.int32)
    t = np.arange(C.POS // 2)
    for y in range(gy):
        b0, b1 = y * C.PER_BLOCK, min(B, (y + 1) * C.PER_BLOCK)
        for x in range(gx):
            k = x * C.POS + 2 * t                       # a thread's two pooled positions = the un-pooled elements 2k .. 2k + 3
            assert k.max() + 1 < Kc and np.all((2 * k) // c["w"] == (2 * k + 3) // c["w"]) or c["w"] == 2
            count[b0:b1, k] += 1
            count[b0:b1, k + 1] += 1
    assert np.all(count == 1)
    # a pooled position's pair never straddles a row (w is even), so 2k, 2k + 1 are MaxPool2d's window
    assert c["w"] % 2 == 0 and 2 * Kc == 64 * c["h"] * c["w"]


def test_the_near_tie_draw_has_equal_sigmoids_with_the_larger_v_on_the_right():
    near = [c for c in CASES if c["draw"] == "neartie"]
    assert near
    for c in near:
        v = C.draw(c)["v"]
        l, r = v[..., 0::2], v[..., 1::2]
        assert np.all(r > l) and np.all(np.abs(l) >= 4) and np.all(np.abs(l) <= 12)
        assert np.array_equal(r.view(np.int32) - l.view(np.int32), np.where(l > 0, 1, -1))        # adjacent floats
        pl, pr = C.sigmoid32(l), C.sigmoid32(r)
        share = float((pl == pr).mean())
        ulps = np.abs(pl.view(np.int32).astype(np.int64) - pr.view(np.int32))
        print("%s: %.3f of the pairs have equal float32 sigmoids, the rest are %d ulp apart at most" % (c["id"], share, ulps.max()))
        assert share >= C.NEARTIE_EQUAL_FLOOR, (c["id"], share)
    for c in (c for c in CASES if c["draw"] == "wide"):
        v = C.draw(c)["v"]
        pv = C.sigmoid32(v)
        assert np.abs(v).max() > 30 and np.isfinite(pv).all() and (pv == 1).any() and pv.min() < 1e-12
    for c in GRID[:6]:                                                      # the grid draw has exact ties
        v = C.draw(c)["v"]
        assert (v[..., 0::2] == v[..., 1::2]).any() and np.array_equal(v * 64, np.round(v * 64))


WORST = {}


@pytest.mark.parametrize("case", GRID, ids=[c["id"] for c in GRID])
def test_fp32_restatement_of_the_formula_stays_inside_the_tolerance(case):
    c = case
    ref = C.reference(c["id"])["dv"].numpy()
    got = C.dv_restated(c, C.draw(c)).astype(np.float64)
    scale = float(np.abs(ref).max())
    excess = float((np.abs(got - ref) - C.DV_RTOL * np.abs(ref) - C.DV_ATOL * scale).max())
    WORST[c["id"]] = excess / scale if scale else 0.0
    print("%s: max|err| %.3g, max|ref| %.3g, worst excess over the tolerance %.3g" % (c["id"], np.abs(got - ref).max(), scale, excess))
    if c["gsel"] == "none" and not c["with_gv"]:
        assert scale == 0 and not got.any()             # no gradient reaches the plane: zeros, exactly
    else:
        assert scale > 0 and excess <= 0, (c["id"], excess)


def test_the_worst_excess_is_printed():
    if WORST:
        k = max(WORST, key=WORST.get)
        print("worst excess over the tolerance relative to max|ref| (negative = inside): %.3g at %s" % (WORST[k], k))
        assert WORST[k] <= 0


def test_the_restatement_routes_a_tie_to_the_left_and_pads_nothing():
    c = dict(BY[GRID[0]["id"]], B=1, target=3, gsel="both", with_gv=0)
    v = np.zeros((1, 64, c["h"], c["w"]), np.float32)
    v[..., 1::2] = np.where(np.arange(c["w"] // 2) % 2, 1.0, 0.0)           # pairs: tie, right larger, tie, ...
    T = dict(v=v, g_pv=np.ones((1, 64, c["h"], c["w"] // 2), np.float32), g_p=np.zeros((1, 3), np.float32),
             i2o_W=np.zeros((3, C.K(c)), np.float32), g_v=None)
    out = C.dv_restated(c, T)
    assert np.all(out[..., 0::2][..., 0::2] == .25) and np.all(out[..., 1::2][..., 0::2] == 0)     # the tie: left
    assert np.all(out[..., 0::2][..., 1::2] == 0) and np.all(out[..., 1::2][..., 1::2] > 0)        # right larger: right


def test_binding_declares_both_symbols_and_the_wrapper_refuses_w3_dv_alone():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    closed, opened = _lib.SIGNATURES["dcll_conv_lif_backward_w3_ex"], _lib.SIGNATURES["dcll_conv_lif_backward_w3_ex_open"]
    w3, w3o = _lib.SIGNATURES["dcll_conv_lif_backward_w3"], _lib.SIGNATURES["dcll_conv_lif_backward_w3_open"]
    assert closed == (w3[0], w3[1][:-1] + [ctypes.c_uint32] + w3[1][-1:])      # the flag word in front of the stream
    assert opened == (w3o[0], w3o[1][:-1] + [ctypes.c_uint32] + w3o[1][-1:])
    assert getattr(lib, "dcll_conv_lif_backward_w3_ex") and getattr(lib, "dcll_conv_lif_backward_w3_ex_open")
    assert lib.dcll_version() == _lib.ABI_VERSION == 10
    assert (ops.W3_FIRST_WGRAD, ops.W3_DV) == (1, 2)
    import torch
    with pytest.raises(ValueError):
        ops.conv_lif_backward(_desc(CASES[0]), torch.zeros(1, CASES[0]["c_in"], 16, 2), None, None, None, None, None, None, None,
                              want_out=False, w3_dv=True)
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    assert DCLLBase.w3_dv is False


def test_refusals_on_the_host():
    """dcll_conv_lif_backward_w3_ex[_open]: unknown flag bits, geometry refusals, v == NULL, g_p without i2o_W, a scratch one float
    short of one partial row, B < 0, B == 0 — all before any launch (nothing here is device memory)"""
    from snn_modulation_classification_amd import _lib
    lib = _lib.get()
    buf = np.zeros(64, np.float32)
    P = ctypes.c_void_p(buf.ctypes.data)
    part, nchunk = ctypes.c_void_p(), ctypes.c_int32()

    def call(d, v, scratch_floats, B, flags, open_form, g_p=None, i2o_W=None):
        if open_form:
            return lib.dcll_conv_lif_backward_w3_ex_open(ctypes.byref(d), P, v, None, g_p, None, None, P, i2o_W, None, None, P,
                                                         scratch_floats, B, ctypes.byref(part), ctypes.byref(nchunk), flags, None)
        return lib.dcll_conv_lif_backward_w3_ex(ctypes.byref(d), P, v, None, g_p, None, None, P, i2o_W, P, P, None, None, P,
                                                scratch_floats, B, flags, None)
    base = dict(BY[CASES[6]["id"]], h=1, w=32, B=2, target=10)
    for open_form in (False, True):
        for c_in in (1, 64):
            d = _desc(dict(base, c_in=c_in))
            need = 2 * 64 * 32 + 64 * (3 * c_in + 1)
            for flags in (4, 8, 7, 0x80000002, 0xffffffff):
                assert call(d, P, need, 2, flags, open_form) == _lib.DCLL_ERR_INVALID, flags
                assert "unknown flag bits" in lib.dcll_last_error().decode()
                assert call(d, P, need, 0, flags, open_form) == _lib.DCLL_ERR_INVALID           # (also in front of B == 0)
            for flags in (0, 1, 2, 3):
                for kw in (dict(c_out=32), dict(kh=3, kw=3, pad_h=1), dict(h=1, w=512)):
                    r = dict(base, c_in=c_in, **kw)
                    assert S.served(r) is not None
                    assert call(_desc(r), P, 10 ** 7, 2, flags, open_form) == _lib.DCLL_ERR_UNSUPPORTED, kw
                    assert "serves c_in 1 or 64, c_out 64, kernel (1,3)" in lib.dcll_last_error().decode()
                assert call(d, None, need, 2, flags, open_form) == _lib.DCLL_ERR_INVALID
                assert "v may be NULL only" in lib.dcll_last_error().decode()
                assert call(d, P, need, 2, flags, open_form, g_p=P) == _lib.DCLL_ERR_INVALID
                assert "g_p needs i2o_W" in lib.dcll_last_error().decode()
                assert call(d, P, need - 1, 2, flags, open_form) == _lib.DCLL_ERR_INVALID
                assert "scratch too small" in lib.dcll_last_error().decode()
                assert call(d, P, need, -1, flags, open_form) == _lib.DCLL_ERR_INVALID
                assert call(d, P, need, 0, flags, open_form) == _lib.DCLL_OK
                assert call(_desc(dict(base, c_out=32)), P, 0, 0, flags, open_form) == _lib.DCLL_OK     # (B == 0: nothing else is looked at)
    assert not buf.any()
