"""CPU self-check of tests/bwd_any_cases.py, the cases of the opt-in MFMA weight gradient (k_bwd_wgrad_any, ABI 9), before
tests/test_gpu_bwd_any.py lets them judge the kernel:

  - the list is well-formed (unique ids, plain convs inside the served predicate, the named layers, every stratum, every kernel
    variant and both sides of each launcher threshold reached) and the seed reproduces it exactly (hash of the records);
  - every case is non-vacuous under fuzz_cases.conv_run (spikes hold both values, arp non-zero, sigmoid' not 0, dW non-zero);
  - the float64 reference conv_backward_ref equals torch autograd in float64 on all of them — including the cases above 64 taps,
    which fuzz_cases never draws."""
import numpy as np
import pytest
import torch

import bwd_any_cases as BA
import fuzz_cases as FZ

CASES = BA.cases()
REFUSALS = BA.refusals()

# sha256 over the JSON records (fuzz_cases.cases_hash)
CASES_HASH = "5b42bc238d50f89399bb3d7355c1ebf4a93b10b81fa12dfd6ce947d2429df871"
REFUSALS_HASH = "9b39f655f6c703eb2e7fa2da4f39262d5d11f6642c4779ed1026fb233d592dce"


def test_the_list_is_well_formed():
    ids = [c["id"] for c in CASES] + [r[0]["id"] for r in REFUSALS]
    assert len(set(ids)) == len(ids)
    strata = {s: [c for c in CASES if c["stratum"] == s] for s in ("named", "taps", "shape", "edge", "free")}
    assert sum(len(v) for v in strata.values()) == len(CASES) and len(strata["free"]) == BA.N_FREE
    for c in CASES:
        assert c["stride"] == c["dilation"] == c["groups"] == 1 and not c["q8"] and not c["misalign"], c["id"]
        assert BA.served(c) and isinstance(BA.launch_plan(c), dict), c["id"]
        p0, p = BA.plan(c), BA.launch_plan(c)
        assert p["lds"] <= p0["lds"] <= 160 * 1024 and p["TPW"] <= p0["TPW"] <= BA.MAX_TPW, c["id"]
        assert p["TPW"] <= 8 * p["NQ"] and (p["PS"] == 1 or (p["NQ"] == 1 and p["TPW"] * p["PS"] <= 8)), c["id"]
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX for c in strata["free"])
    # the named layers: three of mnist_conv.yaml, four of radio_ml_conv.yaml on 24x24 / 12x32, each at B 1, 3 and 33
    named = {(c["c_in"], c["c_out"], c["h"], c["w"], c["pad_h"], c["pool_h"], c["output_layer"] if c["c_out"] == 32 and c["h"] == 11 else 0)
             for c in strata["named"]}
    assert {(1, 16, 28, 28, 2, 2, 0), (16, 24, 13, 13, 2, 1, 0), (24, 32, 11, 11, 2, 2, 1), (1, 32, 24, 24, 3, 1, 0),
            (32, 32, 24, 24, 3, 1, 0), (1, 32, 12, 32, 3, 1, 0), (32, 32, 12, 32, 3, 1, 0)} <= named
    for c in strata["named"]:
        assert c["kh"] == c["kw"] == 7 and c["B"] in (1, 3, 33)
    # above the default path's limits
    taps = {(c["kh"], c["kw"]) for c in strata["taps"]}
    assert {(9, 9), (5, 13), (16, 16), (1, 16), (16, 1)} <= taps
    assert all(c["kh"] * c["kw"] > FZ.WG_MAXTAPS or 16 in (c["kh"], c["kw"]) for c in strata["taps"])
    assert any(c["kh"] * c["kw"] > FZ.WG_MAXTAPS for c in strata["free"])
    assert FZ.wgrad_bands(BA.by_id("bwdany-wide-row"))[0] == 0 and not BA.default_serves(BA.by_id("bwdany-wide-row"))
    # shape edges
    sh = strata["shape"]
    assert {1, 31, 32} <= {c["c_out"] for c in sh} and {1, 2, 33} <= {c["c_in"] for c in sh + strata["taps"]}
    cols = {c["c_in"] * c["kh"] * c["kw"] for c in sh}
    assert min(cols) < 32 and 32 in cols and any(n > 32 and n % 32 for n in cols)
    cshape = [FZ.conv_shape(c) for c in sh]
    assert any(s[1] % 2 == 1 and s[1] > 1 for s in cshape) and any(s[1] == 1 and s[0] > 1 for s in cshape) and any(s[0] * s[1] == 1 for s in cshape)
    assert any(c["pad_h"] == 0 and c["pad_w"] > 0 for c in sh) and any(c["pad_h"] >= c["kh"] for c in sh)
    assert {(c["pool_h"], c["pool_w"], c["readout"], c["output_layer"]) for c in sh} >= {
        (p[0], p[1], r, o) for p in ((1, 1), (2, 2), (3, 2)) for (r, o) in ((1, 0), (0, 0), (1, 1))}
    # every kernel variant, from the restated launcher formula; both sides of its thresholds
    names = {BA.launch_plan(c)["name"] for c in CASES}
    assert names == set(BA.VARIANTS), sorted(set(BA.VARIANTS) ^ names)
    tiles = {c["c_in"]: BA.launch_plan(c) for c in strata["edge"] if c["id"].startswith("bwdany-tiles") and c["B"] == 256}
    assert [tiles[n]["PS"] for n in (1, 2, 3, 4, 5)] == [8, 4, 2, 2, 1] and all(tiles[n]["nsplit"] == 1 for n in range(1, 33) if n in tiles)
    assert [tiles[n]["NQ"] for n in (8, 9, 16, 17, 24, 32)] == [1, 2, 2, 4, 4, 4] and tiles[33]["nsplit"] == 2
    assert BA.launch_plan(BA.by_id("bwdany-tiles5-B255"))["nsplit"] == 2
    p0, p = BA.plan(BA.by_id("bwdany-lds-split")), BA.launch_plan(BA.by_id("bwdany-lds-split"))
    assert p0["NT"] == 9 and p0["TPW"] == 5 and p0["nsplit"] == 2 and p["TPW"] == 1      # (LDS, not the 32-tile cap, splits a full launch)
    # a batch that asks for a tile range straddling one channel more than the full layout holds is given the next TPW that
    # needs no more LDS; and NO chunk count makes a launch larger than the predicate reports (16x16 / 8x16 taps straddle)
    c = BA.by_id("bwdany-straddle-B86")
    want = -(-BA.plan(c)["NT"] // -(-BA.TARGET_WG // 86))
    assert want == 30 and BA.launch_plan(c)["TPW"] == BA.plan(c)["TPW"] == 32 and BA.launch_plan(c)["lds"] == BA.plan(c)["lds"]
    for cin in (3, 11, 20, 37):
        for (kh, kw) in ((16, 16), (8, 16), (7, 7)):
            for co in (2, 16):
                g = dict(FZ.CONV_DEFAULT, c_in=cin, c_out=co, kh=kh, kw=kw, pad_h=kh // 2, pad_w=kw // 2, h=24, w=24)
                full = BA.plan(g)["lds"]
                assert all(BA.plan(g, n)["lds"] <= full for n in range(1, 257)), (cin, kh, kw, co)
    assert BA.plan(BA.by_id("bwdany-lds-31x40"))["lds"] == 4 * 40956       # (1240 + 1 floats of image, rounded up to 4, + 32 x 1241 of g; limit 40960)
    assert any(c["B"] > BA.MAX_CHUNKS and c["B"] % BA.MAX_CHUNKS for c in CASES)
    # refusals: the launcher's message, from the restated predicate
    for c, code, msg in REFUSALS:
        if code == "UNSUPPORTED":
            assert BA.plan(c) == msg, c["id"]
        else:
            assert BA.served(c)
    assert {r[0]["id"].split("-")[-1] for r in REFUSALS} >= {"cout33", "kh17", "stride2", "dilation2", "groups2", "32x40", "scratch"}


def test_the_seed_reproduces_the_list_exactly():
    assert FZ.cases_hash(BA.cases()) == FZ.cases_hash(CASES) == CASES_HASH
    assert FZ.cases_hash([r[0] for r in BA.refusals()]) == REFUSALS_HASH
    assert FZ.cases_hash(BA.cases(BA.SEED + 1)) != CASES_HASH


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
