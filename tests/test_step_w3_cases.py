"""CPU self-check of tests/step_w3_cases.py: the case lists of the differential tests of dcll_conv_lif_step_w3 /
dcll_conv_lif_backward_w3 are proven here before tests/test_gpu_step_w3.py lets them judge the kernels.

  - the seed reproduces the lists and the strata hold what the issue names: every served log2 w, one tile per sample, exactly one
    workgroup, a ragged last workgroup, w = 256, the production layer, both sides of the 8- / 4-tile switch, a grid beyond residency;
  - the restated predicate and LDS bytes equal dcll_conv_lif_step_w3_lds / dcll_conv_lif_backward_w3_lds — the library's own
    (host-only) functions — for every case and refusal, with the refusal's phrase in dcll_last_error();
  - every refusal returns its code and message on the host, before any launch;
  - the restated dispatch reaches every form; the 4-tile form is chosen only where the race note allows it;
  - tile ranges partition every plane; every image position a lane reads is a position the workgroup wrote or zeroed;
  - the C oracle runs every forward case with a non-vacuous trajectory (floor: S.NON_VACUOUS_FLOOR of the cases);
  - a float32 restatement of k_bwd_wgrad_w3's summation order stays inside the weight gradient's tolerance against float64 on
    every backward case."""
import collections
import ctypes

import numpy as np
import pytest

import fuzz_cases as FZ
import step_w3_cases as S

CASES = S.cases()
REFUSE = S.refusals()
BWD = S.bwd_cases()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)
# weight-gradient columns n = 3 ci + kx the restatement follows (every output channel of each): both row ends' taps, first / last ci
COLS64 = [0, 1, 2, 94, 96, 98, 189, 191]


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, bool(c["output_layer"]), c["tau_tensor"], 1.0 if c["refractory"] else 0.0,
                              FZ.ALPHARP, c["stride"], c["dilation"], c["groups"])


def test_the_seed_reproduces_the_lists_exactly():
    assert S.cases_hash(S.cases()) == S.cases_hash(CASES) != S.cases_hash(S.cases(S.SEED + 1))
    assert S.cases_hash(S.bwd_cases()) == S.cases_hash(BWD) and S.cases_hash(S.refusals()) == S.cases_hash(REFUSE)
    ids = [c["id"] for c in CASES + REFUSE + BWD]
    assert len(set(ids)) == len(ids)
    assert all(S.by_id(c["id"]) == c for c in CASES[::9] + REFUSE[::5] + BWD[::11])


def test_the_strata_hold_what_the_issue_names():
    assert {k: len(v) for k, v in BY.items()} == dict(geometry=42, switch=10, grid=1, readout=5)
    assert all(S.served(c) is None and c["c_out"] == 64 and (c["kh"], c["kw"], c["pool_w"]) == (1, 3, 2) for c in CASES + BWD)
    geo = BY["geometry"]
    assert {(c["h"], c["w"]) for c in geo if c["c_in"] == 64} == set(S.GEO64) and {(c["h"], c["w"]) for c in geo if c["c_in"] == 1} == set(S.GEO1)
    assert {c["w"] for c in geo if c["c_in"] == 64} == {2, 4, 8, 16, 32, 64, 128, 256}          # every served log2 w
    assert {c["B"] for c in geo} == set(S.FWD_B)
    for key in ("refractory", "tau_tensor", "bias", "want_v"):
        for hw in S.GEO64 + S.GEO1:
            assert {c[key] for c in geo if (c["h"], c["w"]) == hw} == {0, 1}, (key, hw)         # every option both ways per geometry
    by = {c["id"]: c for c in CASES}
    one_tile = by["w3-64to64-16x2-B3"]
    assert one_tile["h"] * one_tile["w"] == 32 and len(S.tile_ranges(one_tile, 3)) == 1          # one tile per sample, one workgroup
    assert S.tile_ranges(by["w3-64to64-16x2-B11"], 11) == [(0, 4), (4, 8), (8, 11)]            # workgroups spanning samples, ragged
    assert S.tile_ranges(by["w3-64to64-3x128-B1"], 1) == [(0, 4), (4, 8), (8, 12)] and S.tiles(by["w3-64to64-3x128-B1"], 171) == 8
    assert S.tile_ranges(by["w3-switch-64to64-3x128"], 171)[-1] == (2048, 2052)                 # ... ragged in the 8-tile form too
    assert all(S.tiles(c, B) == 8 for c in CASES if c["w"] == 256 for B in (1, 3, 11))          # w = 256: the 4-tile form is forbidden
    prod = by["w3-64to64-16x64-B3"]
    assert (prod["c_in"], prod["h"], prod["w"]) == (64, 16, 64)
    for c in BY["switch"]:
        assert (S.tiles(c, c["B_run"]), S.tiles(c, c["also_B"])) == (8, 4) and c["also_B"] == c["B_run"] - 1
        assert (S.ntiles(c, c["B_run"]) + 7) // 8 >= S.MIN_WGS > (S.ntiles(c, c["also_B"]) + 7) // 8
    g = BY["grid"][0]
    assert (g["h"], g["w"], g["B_run"]) == (4, 64, 1100) and len(S.tile_ranges(g, 1100)) == 1100 and S.tiles(g, 1100) == 8
    ro = {c["id"]: c for c in BY["readout"]}
    assert ro["w3-i2o"]["readout"] and ro["w3-output-layer"]["output_layer"] and ro["w3-misalign"]["misalign"] and not ro["w3-state0"]["state0"]
    assert {(c["h"], c["w"]) for c in BWD if c["c_in"] == 64} == set(S.GEO64) and {c["B"] for c in BWD} == set(S.BWD_B)
    assert len(BWD) == 5 * (len(S.GEO64) + len(S.GEO1))
    # both sides of the 256-chunk limit
    assert {S.bwd_chunks(c, c["B"]) == S.MAX_CHUNKS for c in BWD if c["c_in"] == 64} == {False, True}
    assert S.bwd_chunks(S.by_id("w3-bwd-64to64-4x64-B257"), 257) == 256 and S.bwd_chunks(S.by_id("w3-bwd-64to64-16x2-B300"), 300) == 75


def test_refusals_cover_every_field_of_the_predicate():
    by = {c["id"][len("w3-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    assert unsupported == {"cout32", "cin32", "kw5", "padw0", "pool1x1", "w24", "w512", "hw16", "stride2", "groups2"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"} == {"null-x", "null-eps0", "null-W", "null-s", "no-arp",
                                                                             "no-out-W", "B-negative"}
    for k in unsupported:
        assert S.served(by[k]) == (by[k]["code"], by[k]["phrase"]), k
    assert S.served(dict(by["null-x"])) is None


def test_the_library_predicates_agree_with_the_restated_ones():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the functions are host-only)
    assert lib.dcll_version() == 10
    for c in CASES + BWD:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_w3_lds(ctypes.byref(d)))
        assert got > 0 and got == S.lds_bytes(c) <= 160 * 1024, S.describe(c)
        assert ops.step_w3_lds(d) == got and ops.step_w3_supported(d)
        gotb = int(lib.dcll_conv_lif_backward_w3_lds(ctypes.byref(d)))
        assert gotb > 0 and gotb == S.bwd_lds_bytes(c) <= 160 * 1024 and ops.backward_w3_lds(d) == gotb and ops.backward_w3_supported(d)
        for nt in (8, 4):
            assert S.form_lds_bytes(c, nt) <= got
    narrow = dict(CASES[0], w=2, h=16, c_in=64)
    assert S.lds_bytes(narrow) == 4 * (385 * 65 + 64) and S.bwd_lds_bytes(narrow) == 83008          # the largest images
    for c in REFUSE:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_step_w3_lds(ctypes.byref(d)))
        assert got == S.lds_bytes(c), S.describe(c)
        assert int(lib.dcll_conv_lif_backward_w3_lds(ctypes.byref(d))) == S.bwd_lds_bytes(c)
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert got == 0 and not ops.step_w3_supported(d) and not ops.backward_w3_supported(d)
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())


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
    rc = lib.dcll_conv_lif_step_w3(ctypes.byref(d), p("x"), p("W"), p("b"), p("alpha"), p("tau_m"), p("alphas"), p("tau_s"), p("eps0"),
                                   p("eps1"), p("arp"), None, None, None, None, p("s"), None, None, p("pv"), p("v"), r["B"], None)
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode() and "dcll_conv_lif_step_w3" in lib.dcll_last_error().decode()
    assert not buf.any()


def test_backward_refusals_on_the_host():
    """dcll_conv_lif_backward_w3[_open]: geometry refusals, v == NULL, a scratch one float short, B < 0, B == 0 — before any launch"""
    from snn_modulation_classification_amd import _lib
    lib = _lib.get()
    buf = np.zeros(64, np.float32)
    P = ctypes.c_void_p(buf.ctypes.data)
    part, nchunk = ctypes.c_void_p(), ctypes.c_int32()

    def call(d, v, scratch_floats, B, open_form):
        if open_form:
            return lib.dcll_conv_lif_backward_w3_open(ctypes.byref(d), P, v, None, None, None, None, P, None, None, None, P, scratch_floats,
                                                      B, ctypes.byref(part), ctypes.byref(nchunk), None)
        return lib.dcll_conv_lif_backward_w3(ctypes.byref(d), P, v, None, None, None, None, P, None, P, P, None, None, P, scratch_floats,
                                             B, None)
    base = [r for r in REFUSE if r["id"] == "w3-refuse-null-x"][0]
    need = 2 * 64 * 32 + 64 * 193
    for open_form in (False, True):
        for r in REFUSE:
            if r["code"] == "DCLL_ERR_UNSUPPORTED":
                assert call(_desc(r), P, 10 ** 6, 2, open_form) == _lib.DCLL_ERR_UNSUPPORTED, r["id"]
                assert r["phrase"] in lib.dcll_last_error().decode() and "dcll_conv_lif_backward_w3" in lib.dcll_last_error().decode()
        d = _desc(base)
        assert call(d, None, need, 2, open_form) == _lib.DCLL_ERR_INVALID and "v may be NULL only" in lib.dcll_last_error().decode()
        assert call(d, P, need - 1, 2, open_form) == _lib.DCLL_ERR_INVALID and "scratch too small" in lib.dcll_last_error().decode()
        assert call(d, P, need, -1, open_form) == _lib.DCLL_ERR_INVALID
        assert call(d, P, need, 0, open_form) == _lib.DCLL_OK
    assert not buf.any()


def test_the_cases_reach_every_form_and_the_race_note_holds():
    forms = collections.Counter()
    for c in CASES:
        for B in {c["B_run"], c["also_B"] or c["B_run"]}:
            nt = S.tiles(c, B)
            forms[S.form(c, B)] += 1
            assert S.race_free(c, nt), S.describe(c)                       # the form chosen owns whole rows
            assert nt == 8 or (c["w"] <= 128 and 128 % c["w"] == 0)         # 4 tiles only where the race note allows them
            assert S.launch_log(c, B) == [S.form(c, B)]
    assert set(forms) == set(S.all_forms()) and len(forms) == 8, dict(forms)
    # the rule over a sweep of every served width and batch: never four tiles at w = 256, four below 256 workgroups otherwise
    for w in (2, 4, 8, 16, 32, 64, 128, 256):
        for h in (16 if w == 2 else 1, 4, 16):
            if (h * w) % 32:
                continue
            c = dict(CASES[0], h=h, w=w)
            for B in (1, 2, 7, 64, 255, 256, 2040, 2041, 5000):
                nt = S.tiles(c, B)
                assert S.race_free(c, nt) and (nt == 4) == (w <= 128 and (S.ntiles(c, B) + 7) // 8 < 256)
    assert not S.race_free(dict(CASES[0], w=256), 4)
    print("cases per form:", dict(forms))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tile_ranges_partition_the_planes_and_reads_stay_in_the_image(case):
    c = case
    for B in {c["B_run"], c["also_B"] or c["B_run"]}:
        rng_, nt = S.tile_ranges(c, B), S.tiles(c, B)
        assert rng_[0][0] == 0 and rng_[-1][1] == S.ntiles(c, B) == B * c["h"] * c["w"] // 32
        assert all(0 < b - a <= nt for a, b in rng_) and all(rng_[k][1] == rng_[k + 1][0] for k in range(len(rng_) - 1))
        assert all((a * 32) % c["w"] == 0 for a, _ in rng_)                 # every workgroup starts at a row start
        lo, hi, written, zeros = S.image_reads(c, nt)
        npos = S.positions(c["w"], nt)
        assert lo == 0 and hi == npos - 1 and sorted(written + zeros) == list(range(npos))      # every position written exactly once
        assert 4 * (npos * (S.PST if c["c_in"] == 64 else 1) + 64) == S.form_lds_bytes(c, nt) <= S.lds_bytes(c)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_not_vacuous(case):
    c = case
    T, osteps = S.run(c)                        # (asserts: accepted by the oracle, a non-vacuous draw in 24 attempts)
    assert FZ.vacuous(c, osteps) is None, S.describe(c)
    ch, cw, ph, pw = FZ.conv_shape(c)
    assert (ch, cw, ph, pw) == (c["h"], c["w"], c["h"], c["w"] // 2) and len(osteps) == 3
    for st in osteps:
        spikes = st["v"] > 0
        assert spikes.any() and not spikes.all()                            # at least one spike and one silent neuron
        assert st["s"].shape == (c["B"], 64, ph, pw)
    assert (T["b"] is None) == (not c["bias"])


def test_the_non_vacuous_share_meets_its_floor():
    ok = sum(FZ.vacuous(c, S.run(c)[1]) is None for c in CASES[::4])
    assert ok / len(CASES[::4]) >= S.NON_VACUOUS_FLOOR == 1.0


@pytest.mark.parametrize("case", [c for c in BWD if c["c_in"] == 64], ids=[c["id"] for c in BWD if c["c_in"] == 64])
def test_restated_summation_order_stays_inside_the_tolerance(case):
    """float32 in k_bwd_wgrad_w3's order against the float64 reference, on eight weight-gradient columns of every output channel and
    the bias gradient: inside rtol 2e-3, atol 5e-5 max|ref| — the tolerance of tests/test_gpu_step_w3.py stands"""
    c = case
    T = S.bwd_draw(c)
    route = FZ.first_max_route(c, FZ._f64(T["v"]))
    ref = FZ.conv_backward_ref(c, T, T["v"], T["eps1"], route)
    g32 = ref["dv"].numpy().astype(np.float32)
    dW, db = S.wgrad_restated(g32, T["eps1"], COLS64, S.bwd_chunks(c, c["B"]))
    refW = ref["dW"].numpy().reshape(64, 192)
    for got, want, what in ((dW, refW[:, COLS64], "dW"), (db, ref["db"].numpy(), "db")):
        scale = float(np.abs(refW).max()) if what == "dW" else float(np.abs(want).max())
        err = np.abs(got.astype(np.float64) - want)
        excess = float((err - S.GRAD_RTOL * np.abs(want) - S.GRAD_ATOL * scale).max())
        print("%s %s: max|err| %.3g, max|ref| %.3g, worst excess over the tolerance %.3g" % (c["id"], what, err.max(), scale, excess))
        assert excess <= 0, (c["id"], what)
