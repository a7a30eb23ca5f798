"""Value-domain differential tests of every forward kernel family on the GPU: subnormal traces (decay, mixed), membranes exactly
on +-0 / +-2^-149 / saturating values (threshold), real-valued input (analog) — the cases of tests/value_cases.py (proven on the CPU
by tests/test_value_cases.py), through snn_modulation_classification_amd.ops and the device runners of the sibling files, whose
geometry the cases borrow: test_gpu_fuzz (dcll_conv_lif_step), test_gpu_step_any, test_gpu_step_w3, test_gpu_seq_fuzz (the sequence
launchers), test_gpu_seq_any, test_gpu_seq_wide.  Nothing those runners assert is relaxed.

Every call of every case against the pinned-order C oracle: eps0, eps1, arp, the (pooled) spikes bit for bit after every call; v
bit for bit — up to a zero's sign only where the family's own file grants it (k_lif_step_any, k_lif_step_w3, k_lif_seq_any,
k_lif_seq_wide: DESIGN 2, the zero link; a pooled presigmoid buffer: the larger of +0 and -0 has no sign); pv finite, inside
[0, 1] and within the family's own tolerance of sigmoid64(oracle v); the launch log the sibling predicts; a second run
bit-identical; int8 weights == the dequantised twin.  A kernel that flushes a subnormal operand anywhere, takes the spike from a
wrong comparison or one packed clamp, reads x as a flag, or evaluates the sigmoid where exp overflows, fails here
(test_value_cases.py runs each of these mutants through the oracle).  Found by the threshold cases when this file was written:
k_conv_lif_tiled, k_lif_step_c1, k_lif_seq_c1, k_lif_seq_c1t, k_dense_lif_mfma and k_dense_lif_seq returned v = +0 for a membrane
of -0 (a pad link with a weight of +0; DCLL_PAD_W in csrc/dcll_internal.h).

pv_presigmoid cases: dcll_readout_act(ACT_SIGMOID) on the v plane within the header's 1e-4 of a float64 matmul of sigmoid64(v);
dcll_pv_lowhigh_act / dcll_pv_lowhigh on the first threshold plane == numpy's counts exactly (no table value is within 1e-3 of a
counted edge).  Backward from the last threshold step (saturated membranes: sigmoid' is exactly 0 in fp32): dcll_conv_lif_backward,
dcll_conv_lif_backward_any and dcll_dense_lif_backward finite and within GRAD_RTOL / GRAD_ATOL of the float64 reference."""
import collections
import os

import numpy as np
import pytest
import torch

import fuzz_cases as FZ
import seq_fuzz_cases as SF
import test_gpu_fuzz as GF
import test_gpu_seq_any as GA
import test_gpu_seq_fuzz as GS
import test_gpu_seq_wide as GW
import test_gpu_step_any as GSA
import test_gpu_step_w3 as GS3
import value_cases as V

pytestmark = pytest.mark.gpu

CASES = V.cases()
LOGIT_TOL = 1e-4                        # the header's readout contract
SERVED = collections.Counter()          # (family, kind) -> cases that ran to the end with the launch log they predict
RAN = set()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def sigmoid64(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def pooled(c, v):
    """max-pooled oracle v (..., ch, cw) -> (..., ph, pw)"""
    g = V.geometry(c)
    if g["pool"] == (1, 1):
        return v
    lead = v.shape[:-3]
    pool = g["pool"]
    out = torch.nn.functional.max_pool2d(torch.from_numpy(np.ascontiguousarray(v)).reshape((-1,) + v.shape[-3:]), pool, pool,
                                         ((pool[0] - 1) // 2, (pool[1] - 1) // 2)).numpy()
    return out.reshape(lead + out.shape[-3:])


def check_pv(c, got, v, tol, tag):
    """pv finite, in [0, 1], within `tol` of sigmoid64 of the (pooled) oracle v"""
    got = np.asarray(got, np.float64)
    ref = sigmoid64(pooled(c, v)).reshape(got.shape)
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1, tag
    err = float(np.abs(got - ref).max())
    print("%s: max |pv - sigmoid64(oracle v)| %.3g (tolerance %.3g)" % (tag, err, tol))
    assert err <= tol, (tag, err)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def up_to_zero_sign(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))


# ---------------------------------------------------------------------------------------------------------------------------
# the per-step entries
# ---------------------------------------------------------------------------------------------------------------------------
def run_step_conv(c, T, traj, dev):
    """dcll_conv_lif_step through test_gpu_fuzz's runner; the last threshold step feeds dcll_conv_lif_backward"""
    off16 = bool(c["misalign"])
    steps, last, names = GF.conv_forward(c, T, dev, off16=off16)
    assert set(c["names"]) <= set(names), (c["id"], names)
    GF.check_conv_forward(c, T, traj, steps)
    for t, (g, o) in enumerate(zip(steps, traj)):
        check_pv(c, g["pv"], o["v"], GF.PV_TOL, (c["id"], "step %d" % t))
    again, _, names2 = GF.conv_forward(c, T, dev, off16=off16)
    assert names2 == names
    GF.assert_same_run(steps, again, "a second run", c["id"])
    if c["kind"] == "threshold":
        GF.conv_backward(c, T, traj, steps, last, dev)


def run_step_dense(c, T, traj, dev):
    """dcll_dense_lif_step as test_gpu_fuzz.test_dense_cases drives it; the last threshold step feeds dcll_dense_lif_backward"""
    from snn_modulation_classification_amd import ops
    d = ops.DenseDesc(c["in_features"], c["out_features"], c["target"], c["tau_tensor"], c["refractory"], c["alpharp"],
                      1.0 if c["refractory"] else 0.0)
    cu = GF.cu
    W, b, tau = cu(T["W"], dev), cu(T["b"], dev), [cu(t, dev) for t in T["tau"]]
    i2o_W, i2o_b = cu(T["i2o_W"], dev), cu(T["i2o_b"], dev)
    runs = []
    for _ in range(2):
        eps0, eps1 = cu(T["eps0"], dev), cu(T["eps1"], dev)
        arp = cu(T["arp"], dev) if c["refractory"] else None
        outs = []
        with ops.kernel_trace() as tr:
            for t, o in enumerate(traj):
                s, p, pv, v = ops.dense_lif_step(d, cu(T["x"][t], dev), W, b, *tau, eps0, eps1, arp, i2o_W, i2o_b)
                tag = (c["id"], "step %d" % t)
                assert GF.bits_equal(eps0, o["eps0"]) and GF.bits_equal(eps1, o["eps1"]), tag + ("traces",)
                assert GF.bits_equal(v, o["v"]), tag + ("v",)
                assert GF.bits_equal(s, o["s"]), tag + ("spikes",)
                if c["refractory"]:
                    assert GF.bits_equal(arp, o["arp"]), tag + ("arp",)
                check_pv(c, pv.cpu().numpy(), o["v"], GF.PV_TOL, tag)
                p64 = o["pv"].astype(np.float64) @ T["i2o_W"].astype(np.float64).T + T["i2o_b"].astype(np.float64)
                np.testing.assert_allclose(p.cpu().numpy(), p64, atol=LOGIT_TOL, rtol=0, err_msg=str(tag + ("p",)))
                outs.append([a.cpu().numpy().copy() for a in (s, pv, v, eps0, eps1)])
        assert set(c["names"]) <= set(tr.names), (c["id"], tr.names)
        runs.append(outs)
    assert all(same_bits(x, y) for a, b_ in zip(*runs) for x, y in zip(a, b_)), (c["id"], "a second run")
    if c["kind"] == "threshold":
        g = [cu(T[k], dev) for k in ("g_p", "g_pv", "g_v")]
        dW, db = ops.dense_lif_backward(d, eps1, pv, *g, i2o_W, out={})
        ref = FZ.dense_backward_ref(c, T, traj[-1]["v"], traj[-1]["eps1"])
        GF.assert_grad(dW, ref["dW"], "dW", c["id"])
        GF.assert_grad(db, ref["db"], "db", c["id"])


def run_step_path(c, T, traj, dev, G):
    """k_lif_step_any / k_lif_step_w3 through their files' runners (v up to a zero's sign, as there); the last threshold step of a
    layer without pooling feeds dcll_conv_lif_backward_any"""
    from snn_modulation_classification_amd import ops
    B = c["B_run"]
    steps, logs = G.forward(c, T, dev, B, True)
    G.check_log(c, logs, B)
    G.check_against_oracle(c, T, traj, steps, B)
    idx = np.arange(B) % c["B"]
    for t, (g, o) in enumerate(zip(steps, traj)):
        check_pv(c, g["pv"], o["v"][idx], G.PV_TOL, (c["id"], "step %d" % t))
    again, logs2 = G.forward(c, T, dev, B, True)
    assert logs2 == logs
    G.assert_same(steps, again, ("v", "s", "pv", "eps0", "eps1", "arp"), "a second run", c["id"])
    if G is GSA and c["kind"] == "threshold" and V.geometry(c)["pool"] == (1, 1):
        last = steps[-1]
        d = G.conv_desc(c)
        assert ops.backward_any_supported(d)
        cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with ops.kernel_trace() as tr:
            dW, db, _, _ = ops.conv_lif_backward(d, cu(last["eps1"]), cu(last["v"]), cu(last["pv"]), cu(T["g_p"]), None, cu(T["g_pv"]),
                                                 cu(T["g_v"]), cu(T["i2o_W"]) if c["readout"] else None, want_out=False, out={}, any_path=True)
            torch.cuda.synchronize()
        assert any(n.startswith("k_bwd_wgrad_any") for n in tr.names), tr.names
        ref = FZ.conv_backward_ref(V._oracle_case(c), T, traj[-1]["v"], traj[-1]["eps1"], FZ.identity_route(c))
        GF.assert_grad(dW, ref["dW"], "dW (backward_any)", c["id"])
        GF.assert_grad(db, ref["db"], "db (backward_any)", c["id"])


# ---------------------------------------------------------------------------------------------------------------------------
# the sequence entries
# ---------------------------------------------------------------------------------------------------------------------------
def check_seq_conv(c, T, traj, res):
    """test_gpu_seq_fuzz.check_conv, with the one difference the issue grants: the POOLED presigmoid buffer up to a zero's sign"""
    pooled_presig = c["want_pv"] and c["presigmoid"] and c["layer"] != "k7"
    GS.check_conv(dict(c, want_pv=0) if pooled_presig else c, T, traj, res)
    for k, (T_, o, g) in enumerate(zip(c["Ts"], traj, res)):
        tag = (c["id"], "call %d" % k)
        if pooled_presig:
            assert up_to_zero_sign(g["pv"], pooled(c, o["v"])), tag + ("presigmoid buffer",)
        elif c["want_pv"] and not c["presigmoid"]:
            check_pv(c, g["pv"], o["v"], GS.PV_TOL, tag)


def presigmoid_tail(c, T, traj, res, dev):
    """what reads a presigmoid buffer: dcll_readout_act(ACT_SIGMOID) on every call's plane, the pv statistics on the first plane of
    a threshold case (the table's values: exact counts)"""
    from snn_modulation_classification_amd import ops
    rng = np.random.RandomState(c["seed"] % (2 ** 31))
    g_ = V.geometry(c)
    K = g_["cout"] * g_["ph"] * g_["pw"]
    Wt = (rng.uniform(-1, 1, size=(24, K)) * (.5 / np.sqrt(K))).astype(np.float32)
    bias = rng.uniform(-.1, .1, size=(24,)).astype(np.float32)
    for k, (o, g) in enumerate(zip(traj, res)):
        plane = torch.from_numpy(g["pv"]).to(dev).reshape(-1, K)
        assert ops.readout_act_supported(plane, torch.from_numpy(Wt).to(dev))
        got = ops.readout_act(plane, torch.from_numpy(Wt).to(dev), torch.from_numpy(bias).to(dev), presigmoid=True).cpu().numpy()
        ref = sigmoid64(pooled(c, o["v"])).reshape(-1, K) @ Wt.astype(np.float64).T + bias.astype(np.float64)
        err = float(np.abs(got - ref).max())
        print("%s call %d: dcll_readout_act(sigmoid) max |err| %.3g" % (c["id"], k, err))
        assert np.isfinite(got).all() and err <= LOGIT_TOL, (c["id"], k, err)
    if c["kind"] == "threshold":
        first_v = torch.from_numpy(res[0]["pv"][:1]).to(dev)              # iteration 20 = the call's first step: a histogram step
        ref = sigmoid64(pooled(c, traj[0]["v"][:1]))
        edges = np.linspace(0, 1, 20)
        want = [int((ref < edges[1]).sum()), int((ref >= edges[18]).sum())]
        assert min(want) > 0
        act = ops.pv_lowhigh(first_v, 1, 19, presigmoid=True).cpu().numpy()
        assert act.tolist() == [want], (c["id"], "dcll_pv_lowhigh_act", act.tolist(), want)
        plain = ops.pv_lowhigh(torch.from_numpy(ref.astype(np.float32)).to(dev), 1, 19).cpu().numpy()
        assert plain.tolist() == [want], (c["id"], "dcll_pv_lowhigh", plain.tolist(), want)


def run_seq(c, T, traj, dev):
    if c["entry"] == "dense":
        res = GS.dense_calls(c, T, dev)
        GS.check_dense(c, T, traj, res)
        for k, (o, g) in enumerate(zip(traj, res)):
            check_pv(c, g["pv"], o["v"], GS.PV_TOL, (c["id"], "call %d" % k))
        again = GS.dense_calls(c, T, dev)
        for a, b in zip(res, again):
            assert a["names"] == b["names"] and all(same_bits(a[k], b[k]) for k in ("s", "pv", "v", "p", "eps0", "eps1")), c["id"]
        return
    res = GS.conv_calls(c, T, dev)
    check_seq_conv(c, T, traj, res)
    GS.assert_same_calls(res, GS.conv_calls(c, T, dev), "a second run", c["id"])
    if c["q8"]:
        GS.assert_same_calls(res, GS.conv_calls(c, T, dev, dequantised=True), "int8 weights vs the dequantised fp32 tensor", c["id"])
    if c["presigmoid"]:
        presigmoid_tail(c, T, traj, res, dev)


def run_seq_any(c, T, traj, dev, G):
    """k_lif_seq_any / k_lif_seq_wide through their files' runners (v up to a zero's sign, pv within their 1e-4 of the oracle's)"""
    outs = G.run_case(c, dev, run=(T, traj), count=False)
    for k, (o, g) in enumerate(zip(traj, outs)):
        check_pv(c, g[1], o["v"], GA.PV_TOL, (c["id"], "call %d" % k))
    again = G.run_case(c, dev, run=(T, traj), count=False)
    assert all(same_bits(x, y) for a, b in zip(outs, again) for x, y in zip(a, b)), (c["id"], "a second run")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle(dev, case):
    c = case
    print(V.describe(c))
    T, traj, _ = V.run(c)
    src = c["src"]
    if src == "fuzz":
        run_step_conv(c, T, traj, dev)
    elif src == "fuzz-dense":
        run_step_dense(c, T, traj, dev)
    elif src in ("step-any", "step-w3"):
        run_step_path(c, T, traj, dev, GSA if src == "step-any" else GS3)
    elif src == "seq":
        run_seq(c, T, traj, dev)
    else:
        run_seq_any(c, T, traj, dev, GA if src == "seq-any" else GW)
    SERVED[(c["family"], c["kind"])] += 1
    RAN.add(c["id"])


def test_every_family_served_every_kind_that_applies():
    """every family of the list served a case of every kind that applies to it, to the end and with the launch log it predicts
    (runs behind the cases above).  The counts go to $DCLL_PROFILE_DIR/r18_value_case_counts.txt when that is set (profiles/ holds
    a copy of a whole-file run)."""
    assert RAN == {c["id"] for c in CASES}, sorted({c["id"] for c in CASES} - RAN)
    lines = ["%-36s %s" % ("family", " ".join("%9s" % k for k in V.KINDS))]
    for fam in V.families():
        kinds = V.kinds_of(fam)
        assert all(SERVED[(fam, k)] > 0 for k in kinds), (fam, kinds, dict(SERVED))
        lines.append("%-36s %s" % (fam, " ".join("%9s" % (SERVED[(fam, k)] if k in kinds else "-") for k in V.KINDS)))
    print("\n".join(lines))
    out = os.environ.get("DCLL_PROFILE_DIR")
    if out:
        with open(os.path.join(out, "r18_value_case_counts.txt"), "w") as f:
            f.write("value-domain cases served per kernel family and kind (tests/test_gpu_values.py, %d cases; - = the kind does not "
                    "apply: analog needs a float* input, pv_presigmoid cases are decay and threshold)\n" % len(CASES))
            f.write("\n".join(lines) + "\n")
