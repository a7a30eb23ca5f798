"""CPU self-check of tests/fuzz_cases.py: the case generator and the float64 references are proven here before
tests/test_gpu_fuzz.py lets them judge a kernel.

  - the lists have the promised sizes and strata, and the seed reproduces them exactly (hash of the records);
  - every case is accepted by the C oracle with the shapes the generator computed;
  - no case is vacuous: the un-pooled spikes of the three steps hold both values, refractory layers have a non-zero arp, at
    least 80 % of the last step's |v| are below 4 (sigmoid' is not 0 there), and the reference dW with g_v = 0 is non-zero;
  - the float64 backward reference (written from the header's formula, routing as an input) equals torch autograd in float64
    through F.conv2d / F.max_pool2d / F.linear, with the routing from float64 return_indices (rtol 1e-9)."""
import numpy as np
import pytest
import torch

import fuzz_cases as FZ

CONV = FZ.conv_cases()
DENSE = FZ.dense_cases()
REFUSE = FZ.conv_refusals()

# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CONV_HASH = "b9724621f94be30e5ce86d0093d3a8a4a9795b5bbce921f81ea681ff724af063"
DENSE_HASH = "242cfb8ad1ba583abd0e3bedd4e507a5217fa8fa5a86c4df60777cf69d08b260"
REFUSE_HASH = "43de072a968fc16ad58828fdfb51ae94a544522f474caad91682f82517378399"


def test_lists_have_the_promised_sizes_and_strata():
    free = [c for c in CONV if c["stratum"] == "free"]
    edge = [c for c in CONV if c["stratum"] == "edge"]
    assert len(free) >= 160 and len(edge) >= 40 and len(free) + len(edge) == len(CONV)
    assert len(DENSE) >= 40 and len(REFUSE) >= 2
    ids = [c["id"] for c in CONV + DENSE + REFUSE]
    assert len(set(ids)) == len(ids)
    # the free draws reach what the issue lists
    f = lambda key: {c[key] for c in free}
    assert {1, 2, 3, 4} <= f("groups") and any(c["groups"] == c["c_in"] > 4 for c in free)           # incl. depthwise
    assert any(c["c_in"] % 2 == 1 and c["c_in"] > 1 for c in free) and any(c["c_out"] % 2 == 1 for c in free)
    assert f("kh") == set(range(1, 9)) and f("kw") == set(range(1, 9))
    assert f("stride") == {1, 2, 3} and f("dilation") == {1, 2}
    assert f("pad_h") == set(range(5)) and f("pad_w") == set(range(5))
    assert f("pool_h") == {1, 2, 3} and f("pool_w") == {1, 2, 3}
    assert any(c["w"] >= 100 for c in free)
    for key in ("refractory", "tau_tensor", "bias", "q8", "readout", "output_layer", "state0"):
        assert f(key) == {0, 1}, key
    assert .15 <= np.mean([c["q8"] for c in free]) <= .35 and .2 <= np.mean([c["output_layer"] for c in free]) <= .45
    t = f("target")
    assert min(t) <= 8 and any(8 < x <= 16 for x in t) and any(16 < x <= 24 for x in t) and any(24 < x <= 32 for x in t) and max(t) > 32
    assert all(c["B"] in FZ.B_SET for c in free) and {255, 256, 257} & f("B") and min(f("B")) < 16 <= max(b for b in f("B") if b < 64)
    assert all(FZ.conv_work(c) <= FZ.WORK_MAX for c in free)
    # the variants a kernel name cannot show, from the launcher's formula
    RB, ch = FZ.wgrad_bands(FZ.by_id("conv-edge-bands-60x300"))
    assert 1 <= RB < ch
    RB, ch = FZ.wgrad_bands(FZ.by_id("conv-edge-bands-20x300"))
    assert RB == ch
    for c in REFUSE:
        assert c["kh"] * c["kw"] > FZ.WG_MAXTAPS or FZ.wgrad_bands(c)[0] == 0, c["id"]
    # the dense list crosses the K chunks, 1024, the neuron tiles and the 128-sample workgroup
    nin, nout, nb = {c["in_features"] for c in DENSE}, {c["out_features"] for c in DENSE}, {c["B"] for c in DENSE}
    assert min(nin) < 32 and max(nin) > 1024 and min(nout) < 32 and any(64 < x <= 128 for x in nout) and max(nout) > 128
    assert {127, 128, 129} <= nb
    wide = FZ.by_id("dense-wide")
    assert -(-wide["out_features"] // 64) * -(-wide["B"] // 128) >= 512                  # dcll_launch_dense_mfma: not `narrow`
    assert all(-(-c["out_features"] // 64) * -(-c["B"] // 128) < 512 for c in DENSE if c["id"] != "dense-wide")


def test_the_seed_reproduces_the_lists_exactly():
    assert FZ.cases_hash(FZ.conv_cases()) == FZ.cases_hash(CONV) == CONV_HASH
    assert FZ.cases_hash(FZ.dense_cases()) == DENSE_HASH
    assert FZ.cases_hash(FZ.conv_refusals()) == REFUSE_HASH
    assert FZ.cases_hash(FZ.conv_cases(FZ.SEED + 1)) != CONV_HASH


def _close(a, b, what, cid):
    scale = float(b.abs().max())
    assert scale > 0, (cid, what, "the autograd gradient is zero")
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-9, atol=1e-12 * scale, err_msg="%s %s" % (cid, what))


@pytest.mark.parametrize("case", CONV, ids=[c["id"] for c in CONV])
def test_conv_case_is_sound(case):
    c = case
    T, steps = FZ.conv_run(c)                       # (asserts: accepted by the oracle, shapes, a non-vacuous draw exists)
    assert FZ.vacuous(c, steps) is None, FZ.describe(c)
    spk = np.concatenate([(s["v"] > 0).ravel() for s in steps])
    assert spk.any() and not spk.all()
    assert FZ.active_share(steps[-1]["v"]) >= .8
    if c["refractory"]:
        assert np.any(steps[-1]["arp"])
    if c["q8"]:
        q, scale = T["q8"]
        assert q.dtype == np.int8 and np.array_equal(T["W"], q.astype(np.float32) * scale.reshape(-1, 1, 1, 1))
    v, eps1 = steps[-1]["v"], steps[-1]["eps1"]
    ag, route = FZ.conv_backward_autograd(c, T, v, eps1)
    if c["pool_h"] == 1 and c["pool_w"] == 1:
        assert torch.equal(route, FZ.identity_route(c))
    ref = FZ.conv_backward_ref(c, T, v, eps1, route)
    for k in ("dW", "db", "d_outW", "d_outb"):
        assert (ref[k] is None) == (ag[k] is None), k
        if ref[k] is not None:
            _close(ref[k], ag[k], k, c["id"])
    assert float(FZ.conv_backward_ref(c, T, v, eps1, route, zero_g_v=True)["dW"].abs().max()) > 0, "dW behind g_p / g_pv is zero"
    # the pooled pv the oracle returns is the maximum the routing points at (fp32 sigmoid is monotone in v up to ties)
    pv64 = torch.sigmoid(torch.from_numpy(v).double())
    B, co = c["B"], c["c_out"]
    got = torch.gather(pv64.reshape(B, co, -1), 2, route.reshape(B, co, -1)).reshape(steps[-1]["pv"].shape)
    np.testing.assert_allclose(got.numpy(), steps[-1]["pv"], atol=2e-6, rtol=0)


@pytest.mark.parametrize("case", DENSE, ids=[c["id"] for c in DENSE])
def test_dense_case_is_sound(case):
    c = case
    T, steps = FZ.dense_run(c)
    assert FZ.vacuous(c, steps) is None, FZ.describe(c)
    v, eps1 = steps[-1]["v"], steps[-1]["eps1"]
    ag = FZ.dense_backward_autograd(c, T, v, eps1)
    ref = FZ.dense_backward_ref(c, T, v, eps1)
    for k in ("dW", "db"):
        _close(ref[k], ag[k], k, c["id"])
    assert float(FZ.dense_backward_ref(c, T, v, eps1, zero_g_v=True)["dW"].abs().max()) > 0


def test_first_maximum_routing_on_exact_ties():
    """first_max_route (the GPU test feeds it the fp32 pv map of the forward) picks the FIRST maximum of a window in row-major
    order, in float32 and float64 alike — the rule of k_bwd_dv."""
    c = dict(FZ.CONV_DEFAULT, c_in=1, c_out=1, h=4, w=6, kh=1, kw=1, pad_h=0, pad_w=0, pool_h=2, pool_w=3, B=1)
    assert FZ.conv_shape(c) == (4, 6, 2, 2)
    for dt in (torch.float32, torch.float64):
        pv = torch.full((1, 1, 4, 6), .25, dtype=dt)
        pv[0, 0, 1, 3] = .5                        # window (0, 1): rows 0-1, columns 2-4 (pool_w 3 pads one column)
        pv[0, 0, 1, 4] = .5
        r = FZ.first_max_route(c, pv)
        assert r.reshape(-1).tolist() == [0, 1 * 6 + 3, 2 * 6 + 0, 2 * 6 + 2]
