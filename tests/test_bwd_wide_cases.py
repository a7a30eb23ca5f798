"""CPU self-check of tests/bwd_wide_cases.py, the cases of the opt-in MFMA weight gradient of conv layers with 33 .. 64 output
channels (k_bwd_wgrad_wide), before tests/test_gpu_bwd_wide.py lets them judge the kernel:

  - the list is well-formed (unique ids, plain convs inside the served predicate, the named layers, every stratum, every kernel
    variant and both sides of each launcher threshold reached at c_out > 32) and the seed reproduces it exactly (hash of the records);
  - no chunk count 1 .. 256 makes a launch larger than the full launch the predicate reports;
  - the binding declares the three symbols and the Python switches exist (ops, DCLLBase, ConvNetwork, train.py);
  - every case is non-vacuous under fuzz_cases.conv_run (spikes hold both values, arp non-zero, sigmoid' not 0, dW non-zero);
  - the float64 reference conv_backward_ref equals torch autograd in float64 on all of them;
  - the integer draw of the exact test is what float64 autograd gives."""
import numpy as np
import pytest
import torch

import bwd_any_cases as BA
import bwd_wide_cases as BW
import fuzz_cases as FZ

CASES = BW.cases()
REFUSALS = BW.refusals()

# sha256 over the JSON records (fuzz_cases.cases_hash)
CASES_HASH = "fa6066eebd118ed38ba8a83eb3fcb82956d7ad1965d4780357fc13afc7bdeb8d"
REFUSALS_HASH = "fec7dc68c2b5644891b0582fb9a371104afdc047688c201c1de8fc77fa87c9a4"


def test_the_list_is_well_formed():
    ids = [c["id"] for c in CASES] + [r[0]["id"] for r in REFUSALS]
    assert len(set(ids)) == len(ids)
    strata = {s: [c for c in CASES if c["stratum"] == s] for s in ("named", "shape", "edge", "forwarded", "free")}
    assert sum(len(v) for v in strata.values()) == len(CASES) and len(strata["free"]) == BW.N_FREE
    for c in CASES:
        assert c["stride"] == c["dilation"] == c["groups"] == 1 and not c["q8"] and not c["misalign"], c["id"]
        assert BW.served(c) and isinstance(BW.launch_plan(c), dict), c["id"]
        assert (c["c_out"] <= 32) == (c["stratum"] == "forwarded") and c["c_out"] <= 64, c["id"]
        p0, p = BW.plan(c), BW.launch_plan(c)
        assert p["lds"] <= p0["lds"] <= 160 * 1024 and p["TPW"] <= p0["TPW"] <= BW.MAX_TPW, c["id"]
        assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), c["id"]
        assert p["name"].startswith("k_bwd_wgrad_wide<" if c["c_out"] > 32 else "k_bwd_wgrad_any<"), c["id"]
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX and 33 <= c["c_out"] <= 64 for c in strata["free"])
    # the named layers: radio_ml_conv.yaml at netscale 2 and 1.5 on 16x16, mnist_conv.yaml's second and third layer at netscale 2,
    # each at B 1, 3 and 33
    named = collections_count((c["c_in"], c["c_out"], c["h"], c["w"], c["pad_h"], c["pool_h"], c["target"]) for c in strata["named"])
    assert named == {(1, 64, 16, 16, 3, 1, 24): 3, (64, 64, 16, 16, 3, 1, 24): 3, (1, 48, 16, 16, 3, 1, 24): 3, (48, 48, 16, 16, 3, 1, 24): 3,
                     (32, 48, 13, 13, 2, 1, 10): 3, (48, 64, 11, 11, 2, 2, 10): 3}
    for c in strata["named"]:
        assert c["kh"] == c["kw"] == 7 and c["B"] in (1, 3, 33)
        assert c["output_layer"] == 1 or not (c["h"] == 11)
    # shape edges
    sh = strata["shape"]
    assert {33, 40, 63, 64} <= {c["c_out"] for c in sh} and {1, 5, 33} <= {c["c_in"] for c in sh}
    assert {(1, 1), (2, 5)} <= {(c["kh"], c["kw"]) for c in sh}
    assert any(c["kh"] * c["kw"] > FZ.WG_MAXTAPS for c in sh) and any(c["kh"] * c["kw"] > FZ.WG_MAXTAPS for c in strata["free"])
    cshape = [FZ.conv_shape(c) for c in sh]
    assert any(s[1] % 2 == 1 and s[1] > 1 for s in cshape) and any(s[1] == 1 and s[0] > 1 for s in cshape) and any(s[0] * s[1] == 1 for s in cshape)
    assert any(c["pad_h"] == 0 and c["pad_w"] > 0 for c in sh) and any(c["pad_h"] >= c["kh"] for c in sh)
    assert {(c["pool_h"], c["pool_w"], c["readout"], c["output_layer"]) for c in sh} >= {
        (p[0], p[1], r, o) for p in ((1, 1), (2, 2), (3, 2)) for (r, o) in ((1, 0), (0, 0), (1, 1))}
    # every kernel variant at c_out > 32, from the restated launcher formula; both sides of its thresholds
    names = {BW.launch_plan(c)["name"] for c in CASES if c["c_out"] > 32}
    assert names == set(BW.VARIANTS), sorted(set(BW.VARIANTS) ^ names)
    tiles = {c["c_in"]: BW.launch_plan(c) for c in strata["edge"] if c["id"].startswith("bwdwide-tiles") and c["B"] == 256}
    assert [tiles[n]["PS"] for n in (1, 2, 3, 4, 5)] == [8, 4, 2, 2, 1] and all(tiles[n]["nsplit"] == 1 for n in range(1, 33) if n in tiles)
    assert [tiles[n]["NQ"] for n in (8, 9, 16, 17, 24, 32)] == [1, 2, 2, 4, 4, 4] and tiles[33]["nsplit"] == 2
    assert {c["c_out"] for c in strata["edge"] if c["id"].startswith("bwdwide-tiles")} >= {33, 36, 64}
    assert BW.launch_plan(BW.by_id("bwdwide-tiles5-B255"))["nsplit"] == 2
    p0, p = BW.plan(BW.by_id("bwdwide-lds-split")), BW.launch_plan(BW.by_id("bwdwide-lds-split"))
    assert p0["NT"] == 9 and p0["TPW"] == 2 and p0["nsplit"] == 5 and p["TPW"] == 1      # (LDS, not the 32-tile cap, splits a full launch)
    # both sides of the smallest-working-set limit at c_out 64: 628 + 1 + 64 x 629 = 40885 floats (40888 laid out) of 40960
    assert BW.plan(BW.by_id("bwdwide-lds-157x4"))["lds"] == 4 * 40888
    assert BW.plan(BW.by_id("bwdwide-refuse-lds-158x4")) == "exceeds the 160 KiB of LDS"
    assert {c["B"] for c in strata["edge"]} >= {255, 256, 257} and any(c["B"] > BW.MAX_CHUNKS and c["B"] % BW.MAX_CHUNKS for c in CASES)
    # forwarded layers: the plan IS k_bwd_wgrad_any's
    for c in strata["forwarded"]:
        assert BW.plan(c) == BA.plan(c) and BW.launch_plan(c) == BA.launch_plan(c)
    # refusals: the launcher's message, from the restated predicate
    for c, code, msg in REFUSALS:
        if code == "UNSUPPORTED":
            assert BW.plan(c) == msg, c["id"]
        else:
            assert BW.served(c)
    assert {r[0]["id"].split("-")[-1] for r in REFUSALS} >= {"cout65", "kh17", "stride2", "dilation2", "groups2", "158x4", "scratch"}


def collections_count(it):
    out = {}
    for k in it:
        out[k] = out.get(k, 0) + 1
    return out


def test_no_chunk_count_needs_more_lds_than_the_full_launch():
    """The small-batch lowering takes only layouts within the full launch's LDS (16x16 / 8x16 taps: a shorter tile range can
    straddle one input channel more than any range of the full layout) — over the named layers and a grid of geometries."""
    geoms = [c for c in CASES if c["stratum"] == "named" and c["B"] == 1]
    for cin in (3, 11, 20, 37):
        for (kh, kw) in ((16, 16), (8, 16), (7, 7)):
            for co in (33, 64):
                geoms.append(dict(FZ.CONV_DEFAULT, c_in=cin, c_out=co, kh=kh, kw=kw, pad_h=kh // 2, pad_w=kw // 2, h=16, w=16))
    for g in geoms:
        full = BW.plan(g)
        assert isinstance(full, dict), g
        for n in range(1, 257):
            p = BW.plan(g, n)
            assert p["lds"] <= full["lds"] and BW.RED_FLOATS * 4 <= p["lds"] <= 160 * 1024, (g, n)
            assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), (g, n)


def test_the_seed_reproduces_the_list_exactly():
    assert FZ.cases_hash(BW.cases()) == FZ.cases_hash(CASES) == CASES_HASH
    assert FZ.cases_hash([r[0] for r in BW.refusals()]) == REFUSALS_HASH
    assert FZ.cases_hash(BW.cases(BW.SEED + 1)) != CASES_HASH


def test_the_binding_and_the_switches_exist():
    """Header, table and Python layers name the path (no GPU: nothing is called)."""
    import inspect
    import os
    from conftest import ROOT
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    from snn_modulation_classification_amd.networks import ConvNetwork
    header = open(os.path.join(ROOT, "include", "dcll_hip.h")).read()
    for sym, like in (("dcll_conv_lif_backward_wide_lds", "dcll_conv_lif_backward_any_lds"), ("dcll_conv_lif_backward_wide", "dcll_conv_lif_backward_any"),
                      ("dcll_conv_lif_backward_wide_open", "dcll_conv_lif_backward_any_open")):
        assert sym + "(" in header and _lib.SIGNATURES[sym] == _lib.SIGNATURES[like], sym
    assert "#define DCLL_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    assert "wide_path" in inspect.signature(ops.conv_lif_backward).parameters
    assert callable(ops.backward_wide_lds) and callable(ops.backward_wide_supported)
    assert DCLLBase.wide_learning_path is False and callable(DCLLBase.backward_wide_supported)
    assert isinstance(ConvNetwork.wide_learning_path, property) and callable(ConvNetwork.backward_wide_supported)
    for bad in (dict(any_path=True), dict(w3_path=True)):
        with pytest.raises(ValueError):
            ops.conv_lif_backward(None, None, None, None, None, None, None, None, None, False, wide_path=True, **bad)
    import train
    assert train.parse_args(["--wide_learning_path"]).wide_learning_path is True and train.parse_args([]).wide_learning_path is False


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
    """The first case of each kernel variant whose integer draw stays below 2^24 (all of them do), c_out > 32."""
    first = {}
    for c in CASES:
        if c["c_out"] > 32:
            first.setdefault(BW.launch_plan(c)["name"], c)
    return [first[v] for v in BW.VARIANTS]


@pytest.mark.parametrize("case", exact_cases(), ids=[c["id"] for c in exact_cases()])
def test_the_integer_draw_is_what_autograd_gives(case):
    c = case
    X = BW.exact_draw(c)
    assert np.abs(X["dW"]).max() > 0 and np.abs(X["dW"]).max() < 2 ** 24 and np.abs(X["db"]).max() > 0
    W = torch.zeros((c["c_out"], c["c_in"], c["kh"], c["kw"]), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c["c_out"], dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.from_numpy(X["eps1"]).double(), W, b, padding=(c["pad_h"], c["pad_w"]))
    (y * torch.from_numpy(X["g_v"]).double()).sum().backward()
    assert np.array_equal(W.grad.numpy(), X["dW"]) and np.array_equal(b.grad.numpy(), X["db"])
