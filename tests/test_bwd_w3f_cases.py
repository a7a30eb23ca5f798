"""CPU self-check of tests/bwd_w3f_cases.py: the case list of the differential tests of dcll_conv_lif_backward_w3f[_open]
(k_bwd_wgrad_w3f) is proven here before tests/test_gpu_bwd_w3f.py lets it judge the kernel.

  - the seed reproduces the list, and the list holds every item the issue names: the planes, the batches, more jobs than 256
    chunks, a ragged job count against nchunk, a short last job, the three scratch rules, both alignments, the readout selections;
  - the restated job / chunk partition covers every pixel of every case exactly once;
  - every neighbour index the restatement reads lies inside the same row of the same sample;
  - a float32 restatement of the kernel's documented summation order stays inside the weight gradient's tolerance against float64
    on every case — with the case's own chunk count and with nchunk = 1 (one workgroup sums everything);
  - the refusals of the two entry points on the host, before any launch; the binding declares both symbols."""
import ctypes

import numpy as np
import pytest

import bwd_w3f_cases as C
import fuzz_cases as FZ
import step_w3_cases as S

CASES = C.cases()
BY = {c["id"]: c for c in CASES}


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), c["target"], bool(c["output_layer"]), c["tau_tensor"],
                              1.0 if c["refractory"] else 0.0, FZ.ALPHARP, c["stride"], c["dilation"], c["groups"])


def test_the_seed_reproduces_the_list_exactly():
    assert C.cases_hash(C.cases()) == C.cases_hash(CASES) != C.cases_hash(C.cases(C.SEED + 1))
    assert len(BY) == len(CASES) == 31 and all(C.by_id(c["id"]) == c for c in CASES[::7])


def test_the_list_holds_what_the_issue_names():
    assert all(S.served(c) is None and c["c_in"] == 1 and c["c_out"] == 64 for c in CASES)
    assert {(c["h"], c["w"]) for c in CASES} == {(16, 2), (1, 32), (2, 16), (4, 64), (1, 256), (2, 256), (2, 128), (16, 128)}
    for hw in C.PLANES:
        assert {c["B"] for c in CASES if (c["h"], c["w"]) == hw} == ({1, 3, 33} if hw == (16, 128) else {1, 3, 33, 257}), hw
    assert C.PB < 256 and C.PB % 32 == 0                   # rows of 256 pixels are longer than a job
    assert all((c["h"] * c["w"]) % 32 == 0 for c in CASES)
    # more jobs than 256 chunks, with the wrapper's own scratch
    big = BY["w3f-2x128-B257"]
    assert C.jobs(big) == 514 > C.MAX_CHUNKS == C.chunks(big) and big["scratch"] == "ops" and C.room(big) == 256
    # a ragged job count against nchunk (the chunks' lists differ in length), with and without the cap of 256
    ragged = [c for c in CASES if C.jobs(c) % C.chunks(c, room=C.room(c))]
    assert any(c["scratch"] == "ops" for c in ragged) and any(c["scratch"] == "k3" for c in ragged), [c["id"] for c in ragged]
    # a short last job (pixels % 128 != 0), a single-job launch, a launch whose second wave parity has nothing to do
    assert any(C.npix(c) % C.PB for c in CASES) and any(C.jobs(c) == 1 for c in CASES)
    assert any(C.jobs(c) > 1 and C.chunks(c, room=C.room(c)) == C.jobs(c) for c in CASES)
    assert {c["scratch"] for c in CASES} == {"ops", "k1", "k3"} and {c["misalign"] for c in CASES} == {0, 1}
    assert {(c["gsel"], c["output_layer"]) for c in CASES} == {(g, o) for g in ("both", "g_p", "g_pv") for o in (0, 1)}
    for key, vals in (("scratch", C.SCRATCH), ("misalign", (0, 1))):
        for B in C.BATCHES:                                                 # every batch under every rule and alignment
            assert {c[key] for c in CASES if c["B"] == B} == set(vals), (key, B)
    prod = [c for c in CASES if (c["h"], c["w"]) == (16, 128)]
    assert {c["misalign"] for c in prod} == {0, 1}
    # every reduction kernel of the closed form is reached
    assert {C.reduce_name(C.chunks(c, room=C.room(c))) for c in CASES} == {"k_bwd_reduce", "k_bwd_reduce4<4>", "k_bwd_reduce4<16>"}
    # the exact (integer) test's bound holds on every case it runs
    assert all(6 * C.npix(c) < 1 << 24 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_jobs_partition_the_stream_and_neighbours_stay_in_their_row(case):
    c = case
    NP, HW, w = C.npix(c), c["h"] * c["w"], c["w"]
    for nchunk in sorted({C.chunks(c, room=C.room(c)), C.ops_chunks(c), 1}):
        assert 1 <= nchunk <= min(C.MAX_CHUNKS, C.jobs(c))
        lists = C.job_lists(c, nchunk)
        taken = np.array(sorted(J for even, odd in lists for J in even + odd))
        assert np.array_equal(taken, np.arange(C.jobs(c)))                              # every job exactly once
        for k, (even, odd) in enumerate(lists):
            merged = sorted(even + odd)
            assert merged == list(range(k, C.jobs(c), nchunk)) and merged[0::2] == even and merged[1::2] == odd
    count = np.zeros(NP, np.int32)
    for J in range(C.jobs(c)):
        p0, live = C.lane_pixels(c, J)
        p0 = p0[live]
        assert np.all(p0 + 3 < NP) and np.all(p0 // HW == (p0 + 3) // HW)               # a lane's 4 pixels: one sample
        for j in range(4):
            count[p0 + j] += 1
        left, right = C.neighbour_reads(c, p0)
        for nb, own in ((left, p0), (right, p0 + 3)):
            m = nb >= 0
            assert np.all((nb[m] >= 0) & (nb[m] < NP)) and np.all(nb[m] // w == own[m] // w)     # same row (hence sample)
        # and no neighbour inside the row is left out: the mask is exactly "not at the row's end"
        assert np.array_equal(left >= 0, p0 % w != 0) and np.array_equal(right >= 0, (p0 + 3) % w != w - 1)
    assert np.all(count == 1)                                                           # every pixel exactly once


def test_half_tree_is_a_sum_of_32_lanes():
    v = np.arange(32, dtype=np.float32)[None] * np.array([[1.0], [-3.0]], np.float32)
    assert np.array_equal(C.half_tree(v), v.sum(axis=1))
    e = np.eye(32, dtype=np.float32)
    assert np.array_equal(C.half_tree(e), np.ones(32, np.float32))                      # every lane is counted once


WORST = {}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_fp32_restatement_of_the_summation_order_stays_inside_the_tolerance(case):
    c = case
    ref = C.reference(c["id"])
    g = ref["dv"].numpy().astype(np.float32)
    eps1 = C.draw(c)["eps1"]
    for nchunk in sorted({C.chunks(c, room=C.room(c)), 1}):
        part, dW, db = C.wgrad_restated(g, eps1, nchunk)
        assert part.shape == (nchunk, 64, 4)
        for what, got, want in (("dW", dW, ref["dW"].numpy().reshape(64, 3)), ("db", db, ref["db"].numpy())):
            scale = float(np.abs(want).max())
            excess = float((np.abs(got - want) - C.GRAD_RTOL * np.abs(want) - C.GRAD_ATOL * scale).max())
            WORST[(c["id"], nchunk, what)] = excess / scale
            print("%s nchunk %d %s: max|err| %.3g, max|ref| %.3g, worst excess over the tolerance %.3g"
                  % (c["id"], nchunk, what, np.abs(got - want).max(), scale, excess))
            assert scale > 0 and excess <= 0, (c["id"], nchunk, what, excess)


def test_the_worst_excess_is_printed():
    if WORST:
        k = max(WORST, key=WORST.get)
        print("worst excess over the tolerance relative to max|ref| (negative = inside): %.3g at %s" % (WORST[k], k))
        assert WORST[k] <= 0


def test_exact_draw_is_order_independent():
    c = BY["w3f-1x256-B3"]
    X = C.exact_draw(c)
    for nchunk in (1, 2, 6):
        _, dW, db = C.wgrad_restated(X["g_v"], X["eps1"], nchunk)
        assert np.array_equal(dW.astype(np.int64), X["dW"]) and np.array_equal(db.astype(np.int64), X["db"])
    assert np.abs(X["dW"]).max() > 0 and not np.array_equal(X["dW"][:, 0], X["dW"][:, 2])


def test_binding_declares_both_symbols_and_the_wrapper_refuses_w3_first_alone():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    for name in ("dcll_conv_lif_backward_w3f", "dcll_conv_lif_backward_w3f_open"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("w3f", "w3")]
    assert lib.dcll_version() == _lib.ABI_VERSION == 10
    assert ops.BWD_W3F_PB == C.PB
    import torch
    with pytest.raises(ValueError):
        ops.conv_lif_backward(_desc(CASES[0]), torch.zeros(1, 1, 16, 2), None, None, None, None, None, None, None, want_out=False,
                              w3_first=True)


def test_backward_refusals_on_the_host():
    """dcll_conv_lif_backward_w3f[_open]: geometry refusals, v == NULL, a scratch one float short of one partial row, B < 0, B == 0 —
    all before any launch (nothing here is device memory)"""
    from snn_modulation_classification_amd import _lib
    lib = _lib.get()
    buf = np.zeros(64, np.float32)
    P = ctypes.c_void_p(buf.ctypes.data)
    part, nchunk = ctypes.c_void_p(), ctypes.c_int32()

    def call(d, v, scratch_floats, B, open_form):
        if open_form:
            return lib.dcll_conv_lif_backward_w3f_open(ctypes.byref(d), P, v, None, None, None, None, P, None, None, None, P,
                                                       scratch_floats, B, ctypes.byref(part), ctypes.byref(nchunk), None)
        return lib.dcll_conv_lif_backward_w3f(ctypes.byref(d), P, v, None, None, None, None, P, None, P, P, None, None, P,
                                              scratch_floats, B, None)
    base = dict(BY["w3f-1x32-B3"], B=2)
    for open_form in (False, True):
        for kw in (dict(c_out=32), dict(kh=3, kw=3, pad_h=1), dict(h=1, w=512)):
            r = dict(base, **kw)
            assert S.served(r) is not None
            assert call(_desc(r), P, 10 ** 7, 2, open_form) == _lib.DCLL_ERR_UNSUPPORTED, kw
            assert "serves c_in 1 or 64, c_out 64, kernel (1,3)" in lib.dcll_last_error().decode()
        for c_in in (1, 64):
            d = _desc(dict(base, c_in=c_in))
            need = 2 * 64 * 32 + 64 * (3 * c_in + 1)
            assert call(d, None, need, 2, open_form) == _lib.DCLL_ERR_INVALID and "v may be NULL only" in lib.dcll_last_error().decode()
            assert call(d, P, need - 1, 2, open_form) == _lib.DCLL_ERR_INVALID and "scratch too small" in lib.dcll_last_error().decode()
            assert call(d, P, need, -1, open_form) == _lib.DCLL_ERR_INVALID
            assert call(d, P, need, 0, open_form) == _lib.DCLL_OK
        assert call(_desc(dict(base, c_out=32)), P, 0, 0, open_form) == _lib.DCLL_OK      # (B == 0: nothing is looked at)
    assert not buf.any()
