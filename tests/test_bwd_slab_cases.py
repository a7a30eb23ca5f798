"""CPU self-check of tests/bwd_slab_cases.py, the cases of the opt-in MFMA weight gradient of conv layers with more than 64 output
channels (k_bwd_wgrad_slab), before tests/test_gpu_bwd_slab.py lets them judge the kernel:

  - the slabs partition [0, c_out) exactly once for c_out 1 .. 300, and the rule's constants are the header's;
  - the list is well-formed (unique ids, plain convs inside the served predicate, the named layers, every stratum, the shapes where
    slabs can go wrong, every kernel variant and both sides of each launcher threshold — with NS in the small-batch rule) and the
    seed reproduces it exactly (hash of the records);
  - no chunk count 1 .. 256 makes a launch larger than the full launch the predicate reports, and the library's host-side predicate
    (no GPU needed: it launches nothing) returns the restated plan's LDS bytes for every case and 0 for every refusal;
  - the binding declares the three symbols and the Python switches exist (ops, DCLLBase, ConvNetwork, train.py);
  - every case is non-vacuous under fuzz_cases.conv_run and the float64 reference equals torch autograd in float64;
  - the integer draw of the exact test is what float64 autograd gives, its exactness condition holds, the reference computed slab by
    slab on 64-channel slices equals the whole layer's, and two mutants of the slab assembly — a slab offset by one M tile, the bias
    gradient taken from slab 0 — are caught by it in every multi-slab exact case."""
import os

import numpy as np
import pytest
import torch

import bwd_slab_cases as BS
import bwd_wide_cases as BW
import fuzz_cases as FZ
from conftest import ROOT

CASES = BS.cases()
REFUSALS = BS.refusals()

# sha256 over the JSON records (fuzz_cases.cases_hash)
CASES_HASH = "3023e7a3e6fe382d2054918c1c0b8ff9f27431d1bfb919255b3174d19fa0d6e1"
REFUSALS_HASH = "9a891241269b67ab3dfb72c69f169d1d1f8ce41350e4dd85aee174afa744a8d0"


def test_the_slabs_partition_the_channels_exactly_once():
    for c_out in range(1, 301):
        sl = BS.slabs(c_out)
        assert len(sl) == BS.slab_count(c_out) == -(-c_out // 64)
        owner = np.zeros(c_out, np.int64)
        for first, n in sl:
            assert first % 64 == 0 and 1 <= n <= 64
            owner[first:first + n] += 1
        assert (owner == 1).all(), c_out
        assert all(n == 64 for _, n in sl[:-1]) and sl[-1][1] == c_out - 64 * (len(sl) - 1)
    assert [BS.slabs(n)[-1][1] for n in (65, 96, 97, 128, 129, 200)] == [1, 32, 33, 64, 1, 8]
    shared = open(os.path.join(ROOT, "snn_modulation_classification_amd", "csrc", "dcll_any_shared.h")).read()
    assert "constexpr int SLAB_ROWS = %d;" % BS.SLAB_ROWS in shared and "constexpr int SLAB_MAX = %d;" % BS.SLAB_MAX in shared


def _count(it):
    out = {}
    for k in it:
        out[k] = out.get(k, 0) + 1
    return out


def test_the_list_is_well_formed():
    ids = [c["id"] for c in CASES] + [r[0]["id"] for r in REFUSALS]
    assert len(set(ids)) == len(ids)
    strata = {s: [c for c in CASES if c["stratum"] == s] for s in ("named", "shape", "edge", "forwarded", "free")}
    assert sum(len(v) for v in strata.values()) == len(CASES) and len(strata["free"]) == BS.N_FREE == 30
    for c in CASES:
        assert c["stride"] == c["dilation"] == c["groups"] == 1 and not c["q8"] and not c["misalign"], c["id"]
        assert BS.served(c) and isinstance(BS.launch_plan(c), dict), c["id"]
        assert (c["c_out"] <= 64) == (c["stratum"] == "forwarded"), c["id"]
        p0, p = BS.plan(c), BS.launch_plan(c)
        assert p["lds"] <= p0["lds"] <= 160 * 1024 and p["TPW"] <= p0["TPW"] <= BS.MAX_TPW, c["id"]
        assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), c["id"]
        assert p["name"].startswith("k_bwd_wgrad_slab<" if c["c_out"] > 64 else "k_bwd_wgrad_wide<"), c["id"]
        if c["c_out"] > 64:
            assert p["NS"] == BS.slab_count(c["c_out"]) >= 2, c["id"]
    # planes at most 16x16 and B at most 5 but for the stated cases: the batch cases, the launcher's thresholds, the LDS limit
    for c in CASES:
        if c["stratum"] != "edge":
            assert c["h"] <= 16 and c["w"] <= 16, c["id"]
            assert c["B"] <= 5 or c["id"] in ("bwdslab-B33", "bwdslab-B257-4x4"), c["id"]
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX and 65 <= c["c_out"] <= 200 for c in strata["free"])
    # the named layers: radio_ml_conv.yaml at netscale 3 and 4 on 16x16, B = 1 (the forward runs three steps)
    named = _count((c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["kw"], c["pad_h"], c["B"]) for c in strata["named"])
    assert named == {(1, 96, 16, 16, 7, 7, 3, 1): 1, (96, 96, 16, 16, 7, 7, 3, 1): 1, (1, 128, 16, 16, 7, 7, 3, 1): 1,
                     (128, 128, 16, 16, 7, 7, 3, 1): 1} and FZ.STEPS == 3
    # the shapes where slabs can go wrong
    sh = strata["shape"]
    assert {65, 96, 97, 128, 129, 200} <= {c["c_out"] for c in sh} and {1, 3, 64, 70} <= {c["c_in"] for c in sh}
    assert {(1, 1), (2, 5), (3, 3), (7, 7), (9, 9)} <= {(c["kh"], c["kw"]) for c in sh}
    assert any(c["kh"] * c["kw"] > FZ.WG_MAXTAPS for c in sh)
    cshape = [FZ.conv_shape(c) for c in sh]
    assert any(s[1] % 2 == 1 and (s[0] * s[1]) % 2 == 1 and s[1] > 1 for s in cshape)
    assert {9, 32, 33} <= {s[0] * s[1] for s in cshape} and any(s[0] * s[1] == 1 for s in cshape)
    assert {(c["pool_h"], c["pool_w"], c["readout"], c["output_layer"]) for c in sh} >= {
        (p[0], p[1], r, o) for p in ((1, 1), (2, 2), (3, 3), (1, 2)) for (r, o) in ((1, 0), (0, 0), (1, 1))}
    assert {c["refractory"] for c in sh} == {0, 1} and {c["B"] for c in sh} >= {1, 3, 33, 257}
    b257 = BS.by_id("bwdslab-B257-4x4")
    assert (b257["h"], b257["w"]) == (4, 4) and b257["B"] > BS.MAX_CHUNKS
    assert sorted(c["c_out"] for c in strata["forwarded"]) == [40, 64]
    for c in strata["forwarded"]:
        assert BS.plan(c) == BW.plan(c) and BS.launch_plan(c) == BW.launch_plan(c)
    # every kernel variant at c_out > 64, from the restated launcher formula; both sides of its thresholds
    names = {BS.launch_plan(c)["name"] for c in CASES if c["c_out"] > 64}
    assert names == set(BS.VARIANTS), sorted(set(BS.VARIANTS) ^ names)
    tiles = {c["c_in"]: BS.launch_plan(c) for c in strata["edge"] if c["id"].endswith("-full")}
    assert [tiles[n]["PS"] for n in (1, 2, 3, 4, 5)] == [8, 4, 2, 2, 1] and all(tiles[n]["nsplit"] == 1 for n in tiles if n <= 32)
    assert [tiles[n]["NQ"] for n in (8, 9, 16, 17, 24, 32)] == [1, 2, 2, 4, 4, 4] and tiles[33]["nsplit"] == 2
    assert {c["c_out"] for c in strata["edge"] if c["id"].endswith("-full")} == {65, 129, 200}
    for c in strata["edge"]:
        if c["id"].endswith("-full"):       # chunks x slabs reach the CU count: the full launch's layout
            assert c["B"] * BS.slab_count(c["c_out"]) >= BS.TARGET_WG > (c["B"] - 1) * BS.slab_count(c["c_out"]), c["id"]
            assert BS.launch_plan(c)["TPW"] == BS.plan(c)["TPW"], c["id"]
    # the small-batch rule counts the slabs: one chunk less halves TPW at 2, 3 and 4 slabs; with the wide path's rule (chunks alone)
    # 85 / 86 and 63 / 64 chunks would be treated alike
    for lo, hi, ns in (("bwdslab-tiles16-B127", None, 2), ("bwdslab-tiles16-B85", "bwdslab-tiles16-B86", 3),
                       ("bwdslab-tiles16-B63", "bwdslab-tiles17-full", 4)):
        c = BS.by_id(lo)
        assert BS.slab_count(c["c_out"]) == ns and c["B"] * ns < BS.TARGET_WG <= (c["B"] + 1) * ns
        assert BS.launch_plan(c)["TPW"] == 8 and BS.launch_plan(c)["nsplit"] == 2 and BS.plan(c)["TPW"] == 16
        assert BS.plan(c, c["B"] + 1)["TPW"] == 16
        if hi:
            assert BS.launch_plan(BS.by_id(hi))["nsplit"] == 1
    assert BS.launch_plan(BS.by_id("bwdslab-tiles24-B127"))["name"] == "k_bwd_wgrad_slab<2> (column split)"
    p0, p = BS.plan(BS.by_id("bwdslab-lds-split")), BS.launch_plan(BS.by_id("bwdslab-lds-split"))
    assert p0["NT"] == 18 and p0["TPW"] == 8 and p0["nsplit"] == 3 and p["TPW"] == 1      # (LDS, not the 32-tile cap, splits a full launch)
    # both sides of the smallest-working-set limit: 628 + 1 + 64 x 629 = 40885 floats (40888 laid out) of 40960, whatever c_out
    assert BS.plan(BS.by_id("bwdslab-lds-157x4"))["lds"] == 4 * 40888
    assert BS.plan(dict(BS.by_id("bwdslab-lds-157x4"), c_out=6400))["lds"] == 4 * 40888
    assert BS.plan(BS.by_id("bwdslab-refuse-lds-158x4")) == "exceeds the 160 KiB of LDS"
    # the grid's bound, the only new one
    small = dict(FZ.CONV_DEFAULT, c_in=1, c_out=64 * 65535, h=2, w=2)
    assert isinstance(BS.plan(small), dict) and BS.plan(dict(small, c_out=64 * 65535 + 1)) == "more than 65535 slabs"
    # refusals: the launcher's message, from the restated predicate
    for c, code, msg in REFUSALS:
        if code == "UNSUPPORTED":
            assert BS.plan(c) == msg, c["id"]
        else:
            assert BS.served(c)
    assert {r[0]["id"].split("-")[-1] for r in REFUSALS} >= {"kh17", "stride2", "dilation2", "groups2", "158x4", "scratch"}


def test_no_chunk_count_needs_more_lds_than_the_full_launch():
    """The small-batch lowering takes only layouts within the full launch's LDS (16x16 / 8x16 taps: a shorter tile range can
    straddle one input channel more than any range of the full layout) — over the named layers and a grid of geometries."""
    geoms = [c for c in CASES if c["stratum"] == "named"]
    for cin in (3, 11, 20, 37):
        for (kh, kw) in ((16, 16), (8, 16), (7, 7)):
            for co in (65, 128, 200):
                geoms.append(dict(FZ.CONV_DEFAULT, c_in=cin, c_out=co, kh=kh, kw=kw, pad_h=kh // 2, pad_w=kw // 2, h=16, w=16))
    for g in geoms:
        full = BS.plan(g)
        assert isinstance(full, dict), g
        for n in range(1, 257):
            p = BS.plan(g, n)
            assert p["lds"] <= full["lds"] and BS.RED_FLOATS * 4 <= p["lds"] <= 160 * 1024, (g, n)
            assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), (g, n)


def test_the_seed_reproduces_the_list_exactly():
    assert FZ.cases_hash(BS.cases()) == FZ.cases_hash(CASES) == CASES_HASH
    assert FZ.cases_hash([r[0] for r in BS.refusals()]) == REFUSALS_HASH
    assert FZ.cases_hash(BS.cases(BS.SEED + 1)) != CASES_HASH


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), c["target"], c["output_layer"], c["tau_tensor"],
                              1.0 if c["refractory"] else 0.0, FZ.ALPHARP, c["stride"], c["dilation"], c["groups"])


def test_the_binding_the_switches_and_the_host_side_predicate():
    """Header, table and Python layers name the path; the library's predicate — host code, nothing is launched — returns the
    restated plan's LDS bytes for every case, 0 for every refusal, and keeps the older paths' answers."""
    import inspect
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    from snn_modulation_classification_amd.networks import ConvNetwork
    header = open(os.path.join(ROOT, "include", "dcll_hip.h")).read()
    for sym, like in (("dcll_conv_lif_backward_slab_lds", "dcll_conv_lif_backward_wide_lds"), ("dcll_conv_lif_backward_slab", "dcll_conv_lif_backward_wide"),
                      ("dcll_conv_lif_backward_slab_open", "dcll_conv_lif_backward_wide_open")):
        assert sym + "(" in header and _lib.SIGNATURES[sym] == _lib.SIGNATURES[like], sym
    assert "#define DCLL_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    assert "slab_path" in inspect.signature(ops.conv_lif_backward).parameters
    assert callable(ops.backward_slab_lds) and callable(ops.backward_slab_supported)
    assert DCLLBase.slab_learning_path is False and callable(DCLLBase.backward_slab_supported)
    assert isinstance(ConvNetwork.slab_learning_path, property) and callable(ConvNetwork.backward_slab_supported)
    for bad in (dict(any_path=True), dict(w3_path=True), dict(wide_path=True)):
        with pytest.raises(ValueError):
            ops.conv_lif_backward(None, None, None, None, None, None, None, None, None, False, slab_path=True, **bad)
    import train
    assert train.parse_args(["--slab_learning_path"]).slab_learning_path is True and train.parse_args([]).slab_learning_path is False
    for c in CASES:
        d = _desc(c)
        assert ops.backward_slab_lds(d) == BS.plan(c)["lds"] > 0, c["id"]
        assert ops.backward_wide_supported(d) == (c["c_out"] <= 64) and not ops.backward_any_supported(d), c["id"]
        if c["c_out"] <= 64:
            assert ops.backward_slab_lds(d) == ops.backward_wide_lds(d)
    for c, code, msg in REFUSALS:
        assert ops.backward_slab_supported(_desc(c)) == (code == "INVALID"), c["id"]
        if code == "UNSUPPORTED":
            assert msg in _lib.get().dcll_last_error().decode() and "dcll_conv_lif_backward_slab_lds" in _lib.get().dcll_last_error().decode()


def _close(a, b, what, cid):
    scale = float(b.abs().max())
    assert scale > 0, (cid, what, "the autograd gradient is zero")
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-9, atol=1e-12 * scale, err_msg="%s %s" % (cid, what))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_sound(case):
    c = case
    T, steps = FZ.conv_run(c)                       # (asserts: accepted by the oracle, shapes, a non-vacuous draw exists)
    assert FZ.vacuous(c, steps) is None, FZ.describe(c)
    v, eps1 = steps[-1]["v"], steps[-1]["eps1"]
    ag, route = FZ.conv_backward_autograd(c, T, v, eps1)
    ref = FZ.conv_backward_ref(c, T, v, eps1, route)
    for k in ("dW", "db", "d_outW", "d_outb"):
        assert (ref[k] is None) == (ag[k] is None), k
        if ref[k] is not None:
            _close(ref[k], ag[k], k, c["id"])
    assert float(FZ.conv_backward_ref(c, T, v, eps1, route, zero_g_v=True)["dW"].abs().max()) > 0, "dW behind g_p / g_pv is zero"


def exact_cases():
    """The first case of each kernel variant, and the first case of each slab count 2, 3, 4 where that is another one."""
    first = {}
    for c in CASES:
        if c["c_out"] > 64:
            first.setdefault(BS.launch_plan(c)["name"], c)
    out = [first[v] for v in BS.VARIANTS]
    for ns in (2, 3, 4):
        if not any(BS.slab_count(c["c_out"]) == ns for c in out):
            out.append(next(c for c in CASES if BS.slab_count(c["c_out"]) == ns))
    return out


def slab_assemble(X, c, mutant=None):
    """dW, db of the exact draw put together slab by slab as the kernel does — each slab from ITS 64-channel slice of g_v and the
    whole eps1 — with one of the mutants the exact test must catch: 'mtile' (slabs from the second on read their dv rows one M tile
    = 32 channels further down), 'bias0' (every slab's bias gradient is slab 0's)."""
    co = c["c_out"]
    dW, db = np.zeros_like(X["dW"]), np.zeros_like(X["db"])
    for s, (first, n) in enumerate(BS.slabs(co)):
        src = first
        if mutant == "mtile" and s > 0:
            src = first - 32
        rows = np.arange(src, src + n)
        sl = np.ascontiguousarray(X["g_v"][:, rows])
        part = _int_grads(c, sl, X["eps1"])
        dW[first:first + n], db[first:first + n] = part
        if mutant == "bias0" and s > 0:
            db[first:first + n] = db[:n]
    return dW, db


def _int_grads(c, g_v, eps1):
    B, n = g_v.shape[0], g_v.shape[1]
    ch, cw, _, _ = FZ.conv_shape(c)
    ep = np.pad(eps1, ((0, 0), (0, 0), (c["pad_h"],) * 2, (c["pad_w"],) * 2)).astype(np.int64)
    g2 = g_v.reshape(B, n, ch * cw).astype(np.int64)
    dW = np.zeros((n, c["c_in"], c["kh"], c["kw"]), np.int64)
    for ty in range(c["kh"]):
        for tx in range(c["kw"]):
            win = ep[:, :, ty:ty + ch, tx:tx + cw].reshape(B, c["c_in"], ch * cw)
            dW[:, :, ty, tx] = np.einsum("bop,bip->oi", g2, win)
    return dW.astype(np.float64), g2.sum(axis=(0, 2)).astype(np.float64)


@pytest.mark.parametrize("case", exact_cases(), ids=[c["id"] for c in exact_cases()])
def test_the_integer_draw_is_what_autograd_gives_and_catches_the_mutants(case):
    c = case
    X = BS.exact_draw(c)
    ch, cw, _, _ = FZ.conv_shape(c)
    # the exactness condition: every product and partial sum an integer below 2^24
    assert np.array_equal(X["g_v"], np.round(X["g_v"])) and np.array_equal(X["eps1"], np.round(X["eps1"]))
    assert np.abs(X["g_v"]).max() <= 2 and 0 <= X["eps1"].min() and X["eps1"].max() <= 3 and 6 * c["B"] * ch * cw < 2 ** 24
    assert np.abs(X["dW"]).max() > 0 and np.abs(X["dW"]).max() < 2 ** 24 and np.abs(X["db"]).max() > 0
    W = torch.zeros((c["c_out"], c["c_in"], c["kh"], c["kw"]), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c["c_out"], dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.from_numpy(X["eps1"]).double(), W, b, padding=(c["pad_h"], c["pad_w"]))
    (y * torch.from_numpy(X["g_v"]).double()).sum().backward()
    assert np.array_equal(W.grad.numpy(), X["dW"]) and np.array_equal(b.grad.numpy(), X["db"])
    # slab by slab on 64-channel slices == the whole layer, bit for bit
    dW, db = slab_assemble(X, c)
    assert np.array_equal(dW, X["dW"]) and np.array_equal(db, X["db"])
    # the mutants differ from the reference in every slab behind the first
    assert BS.slab_count(c["c_out"]) >= 2
    mW, mb = slab_assemble(X, c, "mtile")
    _, bb = slab_assemble(X, c, "bias0")
    for first, n in BS.slabs(c["c_out"])[1:]:
        assert not np.array_equal(mW[first:first + n], X["dW"][first:first + n]), (c["id"], "mtile", first)
        assert not np.array_equal(mb[first:first + n], X["db"][first:first + n]), (c["id"], "mtile db", first)
        assert not np.array_equal(bb[first:first + n], X["db"][first:first + n]), (c["id"], "bias0", first)
