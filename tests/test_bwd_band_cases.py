"""CPU self-check of tests/bwd_band_cases.py, the cases of the opt-in banded MFMA weight gradient (k_bwd_wgrad_band), before
tests/test_gpu_bwd_band.py lets them judge the kernel:

  - the bands partition [0, ch) exactly once for ch 1 .. 64 and N 1 .. ch, forced and under the rule's rebalancing;
  - the list is well-formed (unique ids, every stratum, the shapes the issue names, every kernel variant of both M-tile counts) and
    the seed reproduces it exactly (hash of the records);
  - the restated plan equals the library's host-side plan (dcll_conv_lif_backward_bands_plan / _bands_lds: no GPU, nothing is
    launched) for every case, no chunk count makes a launch larger than the full launch, and every refusal is refused with its
    message;
  - the binding declares the four symbols and the Python switches exist (ops, DCLLBase, ConvNetwork, train.py);
  - every case is non-vacuous under fuzz_cases.conv_run, and a float32 restatement of the kernel's summation (pixel after pixel, job
    after job, chunk after chunk) is within the weight-gradient tolerance of the float64 reference the GPU test uses;
  - the integer draw of the exact test, assembled band by band with halo rows and per-band zero padding through staging buffers
    that persist from job to job, equals the whole-plane reference bit for bit, and three mutants of that assembly — a halo short by
    one row, padding rows left as the previous job wrote them, a short last band summed over RB rows — are caught by it in every
    multi-band case they apply to (and are the identity where they do not)."""
import os

import numpy as np
import pytest
import torch

import bwd_band_cases as BB
import bwd_slab_cases as BS
import fuzz_cases as FZ
from conftest import ROOT

CASES = BB.cases()
REFUSALS = BB.refusals()
GRAD_RTOL, GRAD_ATOL = 2e-3, 5e-5       # the project's weight-gradient tolerance (tests/test_gpu_bwd_any.py): atol = 5e-5 max|ref|

# sha256 over the JSON records (fuzz_cases.cases_hash)
CASES_HASH = "c499c26a849ead69f1dacbc0245f58e07142c906f3901313dd549e0762236a96"
REFUSALS_HASH = "0abc0cf3000e59c416e27d3ddf91b6df5b7dfd2985a5961a921e4507503e3041"


def test_the_bands_partition_the_rows_exactly_once():
    for ch in range(1, 65):
        for n in range(1, ch + 1):
            rb = -(-ch // n)
            for RB, NB in ((rb, n), (-(-ch // (-(-ch // rb))), -(-ch // rb))):      # forced; the rule's NB = ceil(ch / RB), rebalanced
                owner = np.zeros(ch, np.int64)
                ranges = BB.band_ranges(ch, RB, NB)
                assert len(ranges) == NB
                for r0, rows in ranges:
                    assert 0 <= rows <= RB and 0 <= r0 <= ch
                    owner[r0:r0 + rows] += 1
                assert (owner == 1).all(), (ch, n)
                assert [r0 for r0, _ in ranges] == [min(ch, k * RB) for k in range(NB)]
            assert all(rows >= 1 for _, rows in BB.band_ranges(ch, -(-ch // (-(-ch // rb))), -(-ch // rb)))    # the rule leaves no empty band
    assert BB.band_ranges(9, 3, 4) == [(0, 3), (3, 3), (6, 3), (9, 0)] and BB.band_ranges(10, 3, 4) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert BB.chunk_jobs(3, 3, 2)[0] == [(0, 0), (0, 2), (1, 1), (2, 0), (2, 2)]        # bands 0, 2, 1, 0, 2


def test_the_list_is_well_formed():
    ids = [c["id"] for c in CASES] + [r[0]["id"] for r in REFUSALS]
    assert len(set(ids)) == len(ids)
    strata = {s: [c for c in CASES if c["stratum"] == s] for s in ("forced", "edge", "rule", "free")}
    assert sum(len(v) for v in strata.values()) == len(CASES) and len(strata["free"]) == BB.N_FREE == 30
    for c in CASES:
        assert c["stride"] == c["dilation"] == c["groups"] == 1 and not c["q8"] and not c["misalign"], c["id"]
        p0, p = BB.plan(c, nchunk=0), BB.plan(c)
        assert isinstance(p0, dict) and isinstance(p, dict) and p["lds"] <= p0["lds"] <= 160 * 1024, c["id"]
        if not p["forwarded"]:
            assert p["TPW"] <= p0["TPW"] <= BB.MAX_TPW and (p["NB"], p["RB"]) == (p0["NB"], p0["RB"]), c["id"]
            assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), c["id"]
            assert p["nchunk"] == min(c["B"] * p["NB"], 256) and p["MT"] == (1 if c["c_out"] <= 32 else 2), c["id"]
            assert c["bands"] == 0 or p["NB"] == c["bands"], c["id"]
        assert c["B"] <= 3 or c["stratum"] == "edge" or c["id"] == "bwdband-B257-4x4", c["id"]
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX for c in strata["free"])
    fo = strata["forced"]
    shp = {c["id"]: FZ.conv_shape(c) for c in fo}
    for ch in range(2, 10):
        for n in {2, 3, ch}:
            if n <= ch:
                assert any(shp[c["id"]][0] == ch and c["bands"] == n for c in fo), (ch, n)
    assert any(c["bands"] == shp[c["id"]][0] for c in fo)                                                   # one row per band
    assert any(c["kh"] - 1 > -(-shp[c["id"]][0] // c["bands"]) for c in fo)                                 # halo larger than the band
    assert any(c["pad_h"] >= c["kh"] for c in fo) and any(c["pad_h"] == 0 for c in fo)
    assert any(shp[c["id"]][1] % 2 == 1 and shp[c["id"]][1] > 1 for c in fo) and any(shp[c["id"]][1] == 1 for c in fo)
    assert {(1, 1), (2, 5), (9, 9)} <= {(c["kh"], c["kw"]) for c in fo} and {1, 3, 70} <= {c["c_in"] for c in fo}
    assert {1, 32, 33, 64, 65, 96, 129} <= {c["c_out"] for c in fo}
    assert {(c["pool_h"], c["pool_w"], c["readout"], c["output_layer"]) for c in fo} >= {
        (p[0], p[1], r, o) for p in ((1, 1), (2, 2), (1, 2)) for (r, o) in ((1, 0), (0, 0), (1, 1))}
    assert {c["refractory"] for c in fo} == {0, 1}
    assert any(any(0 < rows < p["RB"] for _, rows in BB.band_ranges(shp[c["id"]][0], p["RB"], p["NB"]))
               for c in fo for p in [BB.plan(c)])                                                           # a short last band
    assert any(any(rows == 0 for _, rows in BB.band_ranges(shp[c["id"]][0], p["RB"], p["NB"])) for c in fo for p in [BB.plan(c)])
    o = BB.by_id("bwdband-order-B3-N3")
    assert (o["B"], o["bands"]) == (3, 3) and [k for _, k in BB.chunk_jobs(3, 3, 2)[0]] == [0, 2, 1, 0, 2]
    b257 = BB.by_id("bwdband-B257-4x4")
    assert (b257["h"], b257["w"], b257["bands"]) == (4, 4, 2) and BB.plan(b257)["nchunk"] == 256 < b257["B"] * 2
    # every kernel variant, from the restated launcher formula
    names = {BB.plan(c)["name"] for c in CASES if not BB.plan(c)["forwarded"]}
    assert names == set(BB.VARIANTS), sorted(set(BB.VARIANTS) ^ names)
    for co in (32, 65):
        tiles = {c["c_in"]: BB.plan(c) for c in strata["edge"] if c["id"].startswith("bwdband-c%d-" % co) and c["id"].endswith("-full")}
        assert [tiles[n]["PS"] for n in (1, 2, 3, 4, 5)] == [8, 4, 2, 2, 1] and all(tiles[n]["nsplit"] == 1 for n in tiles if n <= 32)
        assert [tiles[n]["NQ"] for n in (8, 9, 16, 17, 32)] == [1, 2, 2, 4, 4] and tiles[33]["nsplit"] == 2
        assert all(p["nchunk"] * p["NS"] == 256 for p in tiles.values())
        half = BB.plan(BB.by_id("bwdband-c%d-tiles16-half" % co))
        assert half["nchunk"] * half["NS"] == 128 and half["TPW"] == 8 and half["nsplit"] == 2
    # the rule where the whole plane does not fit, and either side of the slab path's limit
    ru = {c["id"]: c for c in strata["rule"]}
    assert all(c["B"] == 1 and c["bands"] == 0 for c in ru.values())
    for cid in ("radio-ns2-24x40-c1", "radio-ns2-24x40-c64", "radio-ns1-48x48-c32", "c96-24x40", "slab-refuses-158x4"):
        c = ru["bwdband-" + cid]
        assert not isinstance(BS.plan(c), dict) and BB.plan(c)["NB"] >= 2 and not BB.plan(c)["forwarded"], cid
    assert [(c["c_in"], c["c_out"], c["h"], c["w"], c["kh"]) for c in strata["rule"][:3]] == [(1, 64, 24, 40, 7), (64, 64, 24, 40, 7), (32, 32, 48, 48, 7)]
    fits = ru["bwdband-slab-fits-157x4"]
    assert BB.plan(fits)["forwarded"] and BB.plan(fits)["name"] == BS.launch_plan(fits)["name"] and BB.plan(fits)["lds"] == BS.plan(fits)["lds"]
    assert BB.plan(fits, bands=1) == BB.plan(fits, bands=0)
    # refusals: the launcher's message, from the restated predicate
    for c, code, msg in REFUSALS:
        if code == "UNSUPPORTED":
            assert BB.plan(c, nchunk=0) == msg, c["id"]
        else:
            assert BB.served(c)
    small = dict(FZ.CONV_DEFAULT, c_in=1, c_out=64 * 65535, h=2, w=2, bands=2)
    assert isinstance(BB.plan(small, nchunk=0), dict) and BB.plan(dict(small, c_out=64 * 65535 + 1), nchunk=0) == "more than 65535 slabs"


def test_the_seed_reproduces_the_list_exactly():
    assert FZ.cases_hash(BB.cases()) == FZ.cases_hash(CASES) == CASES_HASH
    assert FZ.cases_hash([r[0] for r in BB.refusals()]) == REFUSALS_HASH
    assert FZ.cases_hash(BB.cases(BB.SEED + 1)) != CASES_HASH


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), c["target"], c["output_layer"], c["tau_tensor"],
                              1.0 if c["refractory"] else 0.0, FZ.ALPHARP, c["stride"], c["dilation"], c["groups"])


PLAN_KEYS = ("NB", "RB", "TPW", "PS", "NQ", "NS", "nsplit", "nchunk")


def test_the_binding_and_the_switches():
    import inspect
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    from snn_modulation_classification_amd.networks import ConvNetwork
    header = open(os.path.join(ROOT, "include", "dcll_hip.h")).read()
    for sym in ("dcll_conv_lif_backward_bands_lds", "dcll_conv_lif_backward_bands_plan", "dcll_conv_lif_backward_bands",
                "dcll_conv_lif_backward_bands_open"):
        assert sym + "(" in header and sym in _lib.SIGNATURES and hasattr(_lib.get(), sym), sym
    slab, band = _lib.SIGNATURES["dcll_conv_lif_backward_slab"], _lib.SIGNATURES["dcll_conv_lif_backward_bands"]
    assert band[0] == slab[0] and band[1] == slab[1][:-1] + [_lib._I32, slab[1][-1]]           # the _slab arguments + int32_t bands
    slab, band = _lib.SIGNATURES["dcll_conv_lif_backward_slab_open"], _lib.SIGNATURES["dcll_conv_lif_backward_bands_open"]
    assert band[1] == slab[1][:-3] + [_lib._I32] + slab[1][-3:]
    assert "#define DCLL_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    sig = inspect.signature(ops.conv_lif_backward).parameters
    assert sig["band_path"].default is False and sig["bands"].default == 0
    assert callable(ops.backward_bands_lds) and callable(ops.backward_bands_supported) and callable(ops.backward_bands_plan)
    assert DCLLBase.band_learning_path is False and callable(DCLLBase.backward_bands_supported)
    assert isinstance(ConvNetwork.band_learning_path, property) and callable(ConvNetwork.backward_bands_supported)
    for bad in (dict(any_path=True), dict(w3_path=True), dict(wide_path=True), dict(slab_path=True)):
        with pytest.raises(ValueError):
            ops.conv_lif_backward(None, None, None, None, None, None, None, None, None, False, band_path=True, **bad)
    with pytest.raises(ValueError):
        ops.conv_lif_backward(None, None, None, None, None, None, None, None, None, False, bands=2)
    import train
    assert train.parse_args([]).band_learning_path is None and train.parse_args(["--band_learning_path"]).band_learning_path == 0
    assert train.parse_args(["--band_learning_path", "3"]).band_learning_path == 3


def test_the_host_side_plan_equals_the_restated_plan():
    """dcll_conv_lif_backward_bands_plan and _bands_lds — host code, nothing is launched — against bwd_band_cases.plan."""
    from snn_modulation_classification_amd import _lib, ops
    for c in CASES:
        d = _desc(c)
        p0, p = BB.plan(c, nchunk=0), BB.plan(c)
        assert ops.backward_bands_lds(d, c["bands"]) == p0["lds"] > 0 and ops.backward_bands_supported(d, c["bands"]), c["id"]
        assert ops.backward_bands_plan(d, c["B"], c["bands"]) == {k: p[k] for k in PLAN_KEYS}, c["id"]
        for B in (1, 2, 5, 64, 300):
            assert ops.backward_bands_plan(d, B, c["bands"]) == {k: BB.plan(c, B=B)[k] for k in PLAN_KEYS}, (c["id"], B)
        if p["forwarded"]:
            assert ops.backward_bands_lds(d, c["bands"]) == ops.backward_slab_lds(d) == ops.backward_bands_lds(d, 1), c["id"]
        else:
            assert c["bands"] != 0 or not ops.backward_slab_supported(d), c["id"]
    # forced band counts 1 .. ch on a few geometries: NB, RB and refusals alike
    for c in (BB.by_id("bwdband-ch9-N3"), BB.by_id("bwdband-k9x9"), BB.by_id("bwdband-radio-ns1-48x48-c32"), BB.by_id("bwdband-c96-24x40")):
        d = _desc(c)
        for n in range(0, FZ.conv_shape(c)[0] + 2):
            p = BB.plan(c, bands=n)
            if isinstance(p, dict):
                assert ops.backward_bands_plan(d, c["B"], n) == {k: p[k] for k in PLAN_KEYS}, (c["id"], n)
                assert ops.backward_bands_lds(d, n) == BB.plan(c, bands=n, nchunk=0)["lds"]
            else:
                assert ops.backward_bands_lds(d, n) == 0 and p in _lib.get().dcll_last_error().decode(), (c["id"], n, p)
                with pytest.raises(_lib.DCLLUnsupported):
                    ops.backward_bands_plan(d, c["B"], n)


def test_no_chunk_count_needs_more_lds_than_the_full_launch():
    geoms = [(c, c["bands"]) for c in CASES if c["stratum"] == "rule"]
    for cin in (3, 20, 37):
        for (kh, kw) in ((16, 16), (8, 16), (7, 7)):
            for co in (20, 65, 200):
                for n in (0, 2, 5):
                    geoms.append((dict(FZ.CONV_DEFAULT, c_in=cin, c_out=co, kh=kh, kw=kw, pad_h=kh // 2, pad_w=kw // 2, h=40, w=24), n))
    for g, n in geoms:
        full = BB.plan(g, bands=n, nchunk=0)
        assert isinstance(full, dict), g
        if full["forwarded"]:
            continue
        for nc in range(1, 257):
            p = BB.plan(g, bands=n, nchunk=nc)
            assert p["lds"] <= full["lds"] and BB.red_floats(p["MT"]) * 4 <= p["lds"] <= 160 * 1024, (g, nc)
            assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), (g, nc)
            assert p["o_g"] + p["rows"] * p["GLD"] <= p["lds"] // 4 and (p["NB"], p["RB"]) == (full["NB"], full["RB"]), (g, nc)


def test_the_host_side_refusals():
    from snn_modulation_classification_amd import _lib, ops
    for c, code, msg in REFUSALS:
        d = _desc(c)
        assert ops.backward_bands_supported(d, c["bands"]) == (code == "INVALID"), c["id"]
        if code == "UNSUPPORTED":
            err = _lib.get().dcll_last_error().decode()
            assert msg in err and ("dcll_conv_lif_backward_bands_lds" in err or c["bands"] == 1), (c["id"], err)
            out = (np.zeros(8, np.int32) + 7)
            rc = _lib.get().dcll_conv_lif_backward_bands_plan(__import__("ctypes").byref(d), c["B"], c["bands"],
                                                              out.ctypes.data_as(_lib._IP))
            assert rc == _lib.DCLL_ERR_UNSUPPORTED and not out.any() and msg in _lib.get().dcll_last_error().decode(), c["id"]
    d = _desc(dict(FZ.CONV_DEFAULT, c_in=1, c_out=64 * 65535 + 1, h=2, w=2))
    assert ops.backward_bands_lds(d, 2) == 0 and "more than 65535 slabs" in _lib.get().dcll_last_error().decode()
    assert _lib.get().dcll_conv_lif_backward_bands_lds(None, 0) == 0


def _ref_inputs(c):
    T, steps = FZ.conv_run(c)
    assert FZ.vacuous(c, steps) is None, FZ.describe(c)
    v, eps1 = steps[-1]["v"], steps[-1]["eps1"]
    pv_full = torch.sigmoid(torch.from_numpy(np.asarray(v)))
    route = FZ.first_max_route(c, pv_full)
    return T, v, eps1, route


STRATA = ("forced", "edge", "rule", "free")


@pytest.mark.parametrize("stratum", STRATA)
def test_cases_are_sound_and_float32_in_kernel_order_is_within_the_tolerance(stratum):
    """Every case of the stratum (one test per stratum, a loop inside: the case's id is in every message)."""
    cases = [c for c in CASES if c["stratum"] == stratum]
    assert cases
    for c in cases:
        _case_is_sound_and_float32_in_kernel_order_is_within_the_tolerance(c)


def _case_is_sound_and_float32_in_kernel_order_is_within_the_tolerance(case):
    """The float64 reference of the GPU test, and beside it the same gradient summed in float32 the way a workgroup sums it — job
    after job of its chunk, pixel after pixel of each job's own rows, then the chunks in order (a pixel split only shortens the
    pieces): the sums of a band kernel are as long as the plane is large, and must stay inside rtol 2e-3, atol 5e-5 max|ref|."""
    c = case
    T, v, eps1, route = _ref_inputs(c)
    ref = FZ.conv_backward_ref(c, T, v, eps1, route)
    assert float(ref["dW"].abs().max()) > 0 and float(ref["db"].abs().max()) > 0, c["id"]
    assert float(FZ.conv_backward_ref(c, T, v, eps1, route, zero_g_v=True)["dW"].abs().max()) > 0, (c["id"], "dW behind g_p / g_pv is zero")
    p = BB.plan(c)
    dv32 = FZ.conv_backward_ref(c, T, v, eps1, route, dtype=torch.float32)["dv"].numpy()
    dW, db = BB.band_assemble(c, dv32, np.asarray(eps1, np.float32), p["NB"], p["RB"], p["nchunk"], dtype=np.float32)
    for got, want, what in ((dW, ref["dW"].numpy(), "dW"), (db, ref["db"].numpy(), "db")):
        scale = float(np.abs(want).max())
        err = np.abs(got.astype(np.float64) - want)
        print("%s %s: max|err| %.3g, max|ref| %.3g, atol %.3g" % (c["id"], what, err.max(), scale, GRAD_ATOL * scale))
        np.testing.assert_allclose(got.astype(np.float64), want, rtol=GRAD_RTOL, atol=GRAD_ATOL * scale, err_msg="%s %s" % (c["id"], what))


def exact_cases():
    """Every banded case of at most three samples, and the first case of each kernel variant."""
    out = [c for c in CASES if c["B"] <= 3 and not BB.plan(c)["forwarded"]]
    first = {}
    for c in CASES:
        if not BB.plan(c)["forwarded"]:
            first.setdefault(BB.plan(c)["name"], c)
    return out + [first[v] for v in BB.VARIANTS if first[v] not in out]


@pytest.mark.parametrize("stratum", STRATA)
def test_the_band_assembly_is_the_whole_plane_bit_for_bit_and_catches_the_mutants(stratum):
    """Every exact case of the stratum (one test per stratum, a loop inside: the case's id is in every message)."""
    cases = [c for c in exact_cases() if c["stratum"] == stratum]
    assert cases
    for c in cases:
        _the_band_assembly_is_the_whole_plane_bit_for_bit_and_catches_the_mutants(c)


def _the_band_assembly_is_the_whole_plane_bit_for_bit_and_catches_the_mutants(case):
    c = case
    X = BB.exact_draw(c)
    ch, cw, _, _ = FZ.conv_shape(c)
    assert np.abs(X["g_v"]).max() <= 2 and 0 <= X["eps1"].min() and X["eps1"].max() <= 3 and 6 * c["B"] * ch * cw < 2 ** 24, c["id"]
    assert 0 < np.abs(X["dW"]).max() < 2 ** 24 and np.abs(X["db"]).max() > 0, c["id"]
    p = BB.plan(c)
    ranges = BB.band_ranges(ch, p["RB"], p["NB"])
    for nchunk in sorted({p["nchunk"], 2, 1}):
        dW, db = BB.band_assemble(c, X["g_v"], X["eps1"], p["NB"], p["RB"], nchunk)
        assert np.array_equal(dW, X["dW"]) and np.array_equal(db, X["db"]), (c["id"], nchunk)
    if p["NB"] < 2 or c["B"] > 3:
        return
    # one workgroup runs every job (a scratch for one partial row): stale rows are the previous job's
    # (halo: where some band's last staged row is a row of the image; toppad: where some band stages a padding row behind a job
    # that left data there; lastband: where a band is short)
    real = lambda r0, yy: 0 <= r0 - c["pad_h"] + yy < c["h"]
    live = [(r0, rows) for r0, rows in ranges if rows > 0]
    applies = dict(halo=any(real(r0, rows + c["kh"] - 2) for r0, rows in live),
                   toppad=any(not real(r0, yy) for r0, rows in live for yy in range(rows + c["kh"] - 1)) and (c["B"] > 1 or any(
                       not real(r0, yy) and any(real(q0, yy) for q0, qr in live[:i] if yy < qr + c["kh"] - 1)
                       for i, (r0, rows) in enumerate(live) for yy in range(rows + c["kh"] - 1))),
                   lastband=any(0 < rows < p["RB"] for _, rows in ranges))
    for mutant, on in applies.items():
        mW, mb = BB.band_assemble(c, X["g_v"], X["eps1"], p["NB"], p["RB"], 1, mutant)
        same = np.array_equal(mW, X["dW"]) and np.array_equal(mb, X["db"])
        assert same != on, (c["id"], mutant, "caught" if not same else "not caught", "applies" if on else "does not apply")
