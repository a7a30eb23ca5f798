"""The opt-in MFMA weight gradient of any plain conv layer on the device: dcll_conv_lif_backward_any[_open] (k_bwd_wgrad_any,
ABI 9) through ops.conv_lif_backward(any_path=True), on the cases of tests/bwd_any_cases.py (proven on the CPU by
tests/test_bwd_any_cases.py), and through ConvNetwork.any_learning_path / train.py --any_learning_path.

Per case: three forward steps with ops.conv_lif_step as tests/test_gpu_fuzz.py runs them, then the backward.
  - dW, db, d_outW, d_outb against fuzz_cases.conv_backward_ref in float64, from the ORACLE's v and eps1, within the project's
    tolerance for this comparison (rtol 2e-3, atol 5e-5 max|ref|); the pool routing from the forward's un-pooled fp32 pv;
  - the open form + ops.grad_reduce_adam, the v = None form where it applies, and a second run: the closed form's bits;
  - where the default dispatch also serves the layer, the two agree within the same tolerance;
  - the launch log holds the k_bwd_wgrad_any variant bwd_any_cases.plan() predicts and no k_bwd_wgrad; the predicate's LDS bytes
    are the plan's.
The last case test asserts that every variant served a case."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import bwd_any_cases as BA
import fuzz_cases as FZ
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")

CASES = BA.cases()
REFUSALS = BA.refusals()
GRAD_RTOL, GRAD_ATOL = 2e-3, 5e-5       # tests/test_gpu_fuzz.py: rtol, atol = 5e-5 * max|ref|
SERVED = collections.Counter()          # k_bwd_wgrad_any variant -> cases it served
RAN = set()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits_equal(a, b):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_grad(got, ref, what, cid):
    ref = ref.numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    got = got.detach().cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    err = np.abs(got - ref)
    print("%s %s: max|err| %.3g, max|ref| %.3g, worst excess over rtol %.3g (atol %.3g)"
          % (cid, what, err.max(), scale, float((err - GRAD_RTOL * np.abs(ref)).max()), GRAD_ATOL * scale))
    np.testing.assert_allclose(got, ref, rtol=GRAD_RTOL, atol=GRAD_ATOL * scale + 1e-30, err_msg="%s %s" % (cid, what))


def conv_desc(c):
    from snn_modulation_classification_amd import ops
    d = ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                           (c["pool_h"], c["pool_w"]), c["target"], c["output_layer"], c["tau_tensor"],
                           1.0 if c["refractory"] else 0.0, FZ.ALPHARP, c["stride"], c["dilation"], c["groups"])
    assert ops.conv_out_shape(d) == FZ.conv_shape(c)
    return d


def conv_forward(c, T, osteps, dev):
    """The three steps on the device (v checked against the oracle, bit for bit) -> the last step's device tensors + the
    un-pooled fp32 pv of a pooling layer."""
    from snn_modulation_classification_amd import ops
    d = conv_desc(c)
    pooled = not (c["pool_h"] == 1 and c["pool_w"] == 1)
    W, b = cu(T["W"], dev), cu(T["b"], dev)
    tau = [cu(t, dev) for t in T["tau"]]
    eps0, eps1 = cu(T["eps0"], dev), cu(T["eps1"], dev)
    arp = cu(T["arp"], dev) if c["refractory"] else None
    ro = dict(i2o_W=cu(T["i2o_W"], dev), i2o_b=cu(T["i2o_b"], dev)) if c["readout"] else {}
    if c["output_layer"]:
        ro.update(out_W=cu(T["out_W"], dev), out_b=cu(T["out_b"], dev))
    out = {}
    for t in range(FZ.STEPS):
        s, p, o, pv, v = ops.conv_lif_step(d, cu(T["x"][t], dev), W, b, *tau, eps0, eps1, arp, out=out, **ro)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), osteps[-1]["v"].view(np.uint32)), (c["id"], "v of step 3")
    assert np.array_equal(eps1.cpu().numpy().view(np.uint32), osteps[-1]["eps1"].view(np.uint32)), (c["id"], "eps1 of step 3")
    pv_full = out["scratch"][1].detach().cpu().clone() if pooled else None
    return dict(d=d, eps1=eps1, v=v, pv=pv, i2o_W=ro.get("i2o_W")), pv_full


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_any_path_vs_float64_reference(dev, case):
    from snn_modulation_classification_amd import ops
    c, cid = case, case["id"]
    print(FZ.describe(c))
    T, osteps = FZ.conv_run(c)
    last, pv_full = conv_forward(c, T, osteps, dev)
    d, want_out = last["d"], bool(c["output_layer"])
    plan = BA.launch_plan(c)
    assert ops.backward_any_supported(d) and ops.backward_any_lds(d) == BA.plan(c)["lds"] >= plan["lds"]
    g = {k: cu(T[k], dev) for k in ("g_p", "g_o", "g_pv", "g_v")}
    args = (g["g_p"], g["g_o"], g["g_pv"], g["g_v"], last["i2o_W"])
    keys = ("dW", "db") + (("d_outW", "d_outb") if want_out else ())
    with ops.kernel_trace() as tr:
        res = dict(zip(("dW", "db", "d_outW", "d_outb"),
                       ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out={}, any_path=True)))
        out2 = {}
        ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out=out2, open_reduce=True,
                              any_path=True)
        out2["dW"].fill_(float("nan"))
        out2["db"].fill_(float("nan"))
        ops.grad_reduce_adam([dict(out2["parts"])], [])
        out3 = None
        if c["pool_h"] == 1 and c["pool_w"] == 1 and c["target"] <= 32:
            out3 = {}
            ops.conv_lif_backward(d, last["eps1"], None, last["pv"], *args, want_out=want_out, out=out3, any_path=True)
        out4 = {}
        ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out=out4, any_path=True)
        torch.cuda.synchronize()
    names = tr.names
    print("kernels:", names)
    wg = [n for n in names if n.startswith("k_bwd_wgrad")]
    assert wg == [plan["name"]] * len(wg) and len(wg) == (4 if out3 is not None else 3), (cid, wg, plan)
    for k in keys:
        assert bits_equal(out2[k], res[k]), (cid, "open form + dcll_grad_reduce_adam", k)
        assert bits_equal(out4[k], res[k]), (cid, "second run", k)
        if out3 is not None:
            assert bits_equal(out3[k], res[k]), (cid, "v == NULL form", k)
    route = FZ.identity_route(c) if pv_full is None else FZ.first_max_route(c, pv_full)
    ref = FZ.conv_backward_ref(c, T, osteps[-1]["v"], osteps[-1]["eps1"], route)
    for k in keys:
        assert_grad(res[k], ref[k], k, cid)
    if BA.default_serves(c):
        with ops.kernel_trace() as tr:
            dflt = dict(zip(("dW", "db", "d_outW", "d_outb"),
                            ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out={})))
            torch.cuda.synchronize()
        assert not any(n.startswith("k_bwd_wgrad_any") for n in tr.names), tr.names
        for k in keys:
            assert_grad(res[k], dflt[k].detach().cpu().double(), k + " (any path vs default path)", cid)
    SERVED[plan["name"]] += 1
    RAN.add(cid)


def test_every_variant_served_a_case():
    assert RAN == {c["id"] for c in CASES}, "run the whole module: this test sums up the cases above"
    print(dict(SERVED))
    assert set(SERVED) == set(BA.VARIANTS) and all(SERVED[v] >= 1 for v in BA.VARIANTS), dict(SERVED)


def _raw_backward(lib, d, c, dev, scratch_floats, rng, open_form=False):
    """dcll_conv_lif_backward_any[_open] straight through the C ABI with a scratch of the caller's size
    -> (rc, dW, db, scratch, inputs)."""
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    ch, cw, _, _ = FZ.conv_shape(c)
    B = c["B"]
    eps1 = cu(rng.uniform(0, 3, size=(B, c["c_in"], c["h"], c["w"])).astype(np.float32), dev)
    v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    g_v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    dW = torch.full((c["c_out"], c["c_in"] // c["groups"], c["kh"], c["kw"]), -7.25, device=dev)
    db = torch.full((c["c_out"],), -7.25, device=dev)
    scratch = torch.full((scratch_floats + 64,), -3.5, device=dev)
    if open_form:
        part, nchunk = ctypes.c_void_p(), ctypes.c_int32()
        rc = lib.dcll_conv_lif_backward_any_open(ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(g_v), None, None, None,
                                                 ptr(scratch), scratch_floats, B, ctypes.byref(part), ctypes.byref(nchunk), stream_ptr())
    else:
        rc = lib.dcll_conv_lif_backward_any(ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(g_v), None, ptr(dW),
                                            ptr(db), None, None, ptr(scratch), scratch_floats, B, stream_ptr())
    torch.cuda.synchronize()
    return rc, dW, db, scratch, (eps1, v, g_v)


def test_scratch_for_exactly_one_chunk(dev):
    """k = 1: B c_out ch cw + c_out (c_in kh kw + 1) floats — one workgroup row sums all five samples; nothing behind the scratch is
    written; one float less is DCLL_ERR_INVALID with an empty launch log."""
    from snn_modulation_classification_amd import _lib, ops
    c = dict(FZ.CONV_DEFAULT, c_in=3, c_out=5, kh=5, kw=4, pad_h=2, pad_w=1, h=9, w=7, B=5, target=4)
    ch, cw, _, _ = FZ.conv_shape(c)
    d = conv_desc(c)
    need = c["B"] * c["c_out"] * ch * cw + c["c_out"] * (c["c_in"] * 20 + 1)
    with ops.kernel_trace() as tr:
        rc, dW, db, scratch, (eps1, v, g_v) = _raw_backward(_lib.get(), d, c, dev, need, np.random.RandomState(5))
    assert rc == 0, _lib.get().dcll_last_error()
    assert [n for n in tr.names if n.startswith("k_bwd_wgrad")] == [BA.plan(c, 1)["name"]] and "k_bwd_reduce" in tr.names, tr.names
    assert bool((scratch[need:] == -3.5).all())
    e, gv = eps1.cpu().double(), g_v.cpu().double()                       # (no g_p / g_pv: dv = g_v)
    cols = torch.nn.functional.unfold(e, (5, 4), 1, (2, 1), 1)
    ref = torch.einsum("bol,bkl->ok", gv.reshape(5, 5, -1), cols).reshape(dW.shape)
    assert_grad(dW, ref, "dW", "k = 1")
    assert_grad(db, gv.sum(dim=(0, 2, 3)), "db", "k = 1")
    with ops.kernel_trace() as tr:
        rc, dW, db, scratch, _ = _raw_backward(_lib.get(), d, c, dev, need - 1, np.random.RandomState(5))
    assert rc == _lib.DCLL_ERR_INVALID and "scratch too small" in _lib.get().dcll_last_error().decode() and tr.names == []
    assert bool((dW == -7.25).all()) and bool((scratch == -3.5).all())


@pytest.mark.parametrize("open_form", [False, True], ids=["closed", "open"])
@pytest.mark.parametrize("ref", REFUSALS, ids=[r[0]["id"] for r in REFUSALS])
def test_refusals_come_before_any_launch(dev, ref, open_form):
    from snn_modulation_classification_amd import _lib, ops
    c, code, msg = ref
    print(FZ.describe(c))
    d = conv_desc(c)
    assert ops.backward_any_supported(d) == (code == "INVALID")
    ch, cw, _, _ = FZ.conv_shape(c)
    rng = np.random.RandomState(c["seed"] % (2 ** 31))
    if code == "INVALID":
        need = c["B"] * c["c_out"] * ch * cw + c["c_out"] * (c["c_in"] * c["kh"] * c["kw"] + 1)
        with ops.kernel_trace() as tr:
            rc, dW, db, scratch, _ = _raw_backward(_lib.get(), d, c, dev, need - 1, rng, open_form)
        assert rc == _lib.DCLL_ERR_INVALID and msg in _lib.get().dcll_last_error().decode() and tr.names == []
        assert bool((dW == -7.25).all()) and bool((scratch == -3.5).all())
        return
    B = c["B"]
    eps1 = cu(rng.uniform(0, 3, size=(B, c["c_in"], c["h"], c["w"])).astype(np.float32), dev)
    v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    g_v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    out = dict(dW=torch.full((c["c_out"], c["c_in"] // c["groups"], c["kh"], c["kw"]), -7.25, device=dev),
               db=torch.full((c["c_out"],), -7.25, device=dev))
    with ops.kernel_trace() as tr:
        with pytest.raises(_lib.DCLLUnsupported) as e:
            ops.conv_lif_backward(d, eps1, v, None, None, None, None, g_v, None, want_out=False, out=out, open_reduce=open_form,
                                  any_path=True)
    assert msg in str(e.value) and msg in _lib.get().dcll_last_error().decode() and tr.names == [], (str(e.value), tr.names)
    torch.cuda.synchronize()
    assert bool((out["dW"] == -7.25).all()) and bool((out["db"] == -7.25).all()) and "parts" not in out


def test_the_default_path_still_refuses_a_9x9_layer(dev):
    """any_path is opt-in: without it a kernel above 64 taps is refused as before."""
    from snn_modulation_classification_amd import _lib, ops
    c = BA.by_id("bwdany-9x9")
    d = conv_desc(c)
    ch, cw, _, _ = FZ.conv_shape(c)
    eps1 = torch.rand(c["B"], c["c_in"], c["h"], c["w"], device=dev)
    v = torch.randn(c["B"], c["c_out"], ch, cw, device=dev)
    for open_form in (False, True):
        with ops.kernel_trace() as tr:
            with pytest.raises(_lib.DCLLUnsupported) as e:
                ops.conv_lif_backward(d, eps1, v, None, None, None, None, torch.randn_like(v), None, want_out=False, out={},
                                      open_reduce=open_form)
        assert "64 taps" in str(e.value) and tr.names == []


# ------------------------------------------------------------------------------------------------------------------------------
# network level
# ------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from argparse import Namespace
    a = dict(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    a.update(kw)
    return Namespace(**a)


def _net(convs, hw, B, target, burnin, arp, graph):
    from snn_modulation_classification_amd.networks import ConvNetwork
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(_args(arp=arp), (1,) + hw, B, convs, target, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss,
                      opt=torch.optim.Adam, opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6],
                      burnin=burnin)
    net.graph_learn = graph
    net.reset(True)
    net.train()
    return net


def _copy_everything(a, b):
    """b <- a: parameters and buffers, Adam's state, the neuron state (in place: b keeps its addresses)."""
    with torch.no_grad():
        for (ka, ta), (kb, tb) in zip(list(a.named_parameters()) + list(a.named_buffers()),
                                      list(b.named_parameters()) + list(b.named_buffers())):
            assert ka == kb
            tb.copy_(ta)
        for sa, sb_ in zip(a.dcll_slices, b.dcll_slices):
            for ta, tb in zip(sa.dclllayer.i2h.state, sb_.dclllayer.i2h.state):
                tb.copy_(ta)
            assert sa.iter == sb_.iter
            for name in ("optimizer", "optimizer2"):
                oa, ob = getattr(sa, name, None), getattr(sb_, name, None)
                if oa is None:
                    continue
                for pa, pb in zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"]):
                    if pa in oa.state:
                        assert pb in ob.state and set(oa.state[pa]) == set(ob.state[pb])
                        for key, val in oa.state[pa].items():
                            if torch.is_tensor(val):
                                ob.state[pb][key].copy_(val)
                            else:
                                ob.state[pb][key] = val


@pytest.mark.parametrize("spec, hw, B, target, arp", [("mnist_conv.yaml", (28, 28), 4, 10, 0.0), ("radio_ml_conv.yaml", (24, 24), 3, 24, 1.0)],
                         ids=["mnist_conv-B4", "radio_ml_conv-24x24-B3"])
def test_network_learning_steps_any_path_vs_default_path(dev, spec, hw, B, target, arp):
    """Two identically seeded networks, A on the default dispatch and B with any_learning_path: before each of six learning steps
    B takes A's parameters, optimizer state and neuron state; then both learn.  Same forward bits, gradients within the
    tolerance, k_bwd_wgrad_any once per slice in B's log and never in A's."""
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.networks import load_network_spec
    burnin, steps = 3, 6
    convs = lambda: load_network_spec(os.path.join(PKG, "networks", spec))
    A, Bn = _net(convs(), hw, B, target, burnin, arp, False), _net(convs(), hw, B, target, burnin, arp, False)
    assert A.any_learning_path is False and Bn.backward_any_supported() and all(s.backward_any_supported() for s in Bn.dcll_slices)
    Bn.any_learning_path = True
    assert Bn.any_learning_path is True and all(s.any_learning_path for s in Bn.dcll_slices) and not any(s.any_learning_path for s in A.dcll_slices)
    assert all(s._native_learning() is not None for s in A.dcll_slices)
    rng = np.random.RandomState(11)
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    y = y.to(dev)
    learned = 0
    for t in range(burnin - 1 + steps):
        x = torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .15).astype(np.float32)).to(dev)
        _copy_everything(A, Bn)
        logs = []
        for net in (A, Bn):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(tr.names)
        for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):
            for key in ("s", "p", "pv"):
                if torch.is_tensor(sa._learn_bufs.get(key)):
                    assert torch.equal(sa._learn_bufs[key], sb._learn_bufs[key]), (t, key)
        if t < burnin - 1:
            assert not any(n.startswith("k_bwd_wgrad") for n in logs[0] + logs[1])
            continue
        learned += 1
        assert sum(n.startswith("k_bwd_wgrad_any") for n in logs[1]) == len(Bn.dcll_slices), logs[1]
        assert sum(n.startswith("k_bwd_wgrad") for n in logs[1]) == len(Bn.dcll_slices), logs[1]
        assert not any(n.startswith("k_bwd_wgrad_any") for n in logs[0]) and sum(n.startswith("k_bwd_wgrad") for n in logs[0]) == len(A.dcll_slices)
        assert logs[0].count("k_grad_reduce_adam") == logs[1].count("k_grad_reduce_adam") == 1
        for i, (sa, sb) in enumerate(zip(A.dcll_slices, Bn.dcll_slices)):
            for (name, pa), (_, pb) in zip(sa.dclllayer.named_parameters(), sb.dclllayer.named_parameters()):
                assert (pa.grad is None) == (pb.grad is None), name
                if pa.grad is not None:
                    assert_grad(pb.grad, pa.grad.detach().cpu().double(), "slice %d %s.grad" % (i, name), "%s step %d" % (spec, t))
    assert learned == steps


def test_graph_captured_steps_equal_eager_steps_on_the_any_path(dev):
    """With any_learning_path the learning timestep replayed from its captured graph == the step launched eagerly, bit for bit, at
    B = 8 (ConvNetwork.graph_learn, the switch of test_graph_captured_learning_steps_equal_eager_steps)."""
    from snn_modulation_classification_amd.networks import load_network_spec
    B, T, burnin, hw = 8, 16, 4, (28, 28)
    rng = np.random.RandomState(4)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .15).astype(np.float32)).to(dev) for _ in range(T)]
    y = torch.zeros(B, 10)
    y[np.arange(B), rng.randint(0, 10, size=B)] = 1
    y = y.to(dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(load_network_spec(os.path.join(PKG, "networks", "mnist_conv.yaml")), hw, B, 10, burnin, 0.0, graph)
        net.any_learning_path = True
        for t in range(T):
            net.learn(xs[t], y)
        torch.cuda.synchronize()
    a, b = nets[True], nets[False]
    g = a._learn_graphs[((B, 1) + hw, (B, 10))]
    assert g["n"] >= 6 and not b._learn_graphs, (g["n"],)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T
        for (qa, sta), (qb, stb) in zip(sl_a.optimizer.state.items(), sl_b.optimizer.state.items()):
            assert float(sta["step"]) == float(stb["step"]) == T - burnin + 1
            assert torch.equal(sta["exp_avg_sq"], stb["exp_avg_sq"]) and torch.equal(sta["exp_avg"], stb["exp_avg"])
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)


def _radio24(B, burnin, graph=False):
    from snn_modulation_classification_amd.networks import load_network_spec
    net = _net(load_network_spec(os.path.join(PKG, "networks", "radio_ml_conv.yaml")), (24, 24), B, 24, burnin, 1.0, graph)
    net.any_learning_path = True
    return net


def test_learn_sequence_equals_per_step_learning_on_the_any_path(dev):
    """ConvNetwork.learn_sequence with any_learning_path (radio_ml_conv.yaml on 24x24, cells on the device) == the loop
    `for t: net.learn(x[t], y)` on the same planes with the flag: weights, Adam state and clout bit for bit; the weight gradient
    ran on k_bwd_wgrad_any."""
    from snn_modulation_classification_amd import ops
    B, T, burnin, R_ = 4, 11, 6, 24
    rng = np.random.RandomState(3)
    cells = rng.randint(0, R_ * R_, size=(T, B)).astype(np.int32)
    y = torch.zeros(B, 24)
    y[np.arange(B), rng.randint(0, 24, size=B)] = 1
    y = y.to(dev)
    a, b = _radio24(B, burnin), _radio24(B, burnin)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    n_learn = T - burnin + 1
    assert sum(n.startswith("k_bwd_wgrad_any") for n in tr.names) == 3 * n_learn == sum(n.startswith("k_bwd_wgrad") for n in tr.names), tr.names
    x = np.zeros((T, B, R_ * R_), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape(T, B, 1, R_, R_)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        st_a, st_b = sl_a.optimizer.state[sl_a.dclllayer.i2h.weight], sl_b.optimizer.state[sl_b.dclllayer.i2h.weight]
        assert float(st_a["step"]) == float(st_b["step"]) == n_learn and torch.equal(st_a["exp_avg_sq"], st_b["exp_avg_sq"])


def test_the_rank_sharded_step_runs_on_the_any_path(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks — gradients in per-slice slabs, the CLOSED backward per slice
    (dcll_conv_lif_backward_any + k_bwd_reduce), then ops.adam_step — with the collective of a one-rank world (the identity)
    == the single-process step (open form + dcll_grad_reduce_adam) with the flag, bit for bit."""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 7, 3
    rng = np.random.RandomState(8)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1, 24, 24)) < .15).astype(np.float32)).to(dev) for _ in range(T)]
    y = torch.zeros(B, 24)
    y[np.arange(B), rng.randint(0, 24, size=B)] = 1
    y = y.to(dev)
    a, b = _radio24(B, burnin), _radio24(B, burnin)
    for t in range(T):
        a.learn(xs[t], y)
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    monkeypatch.setattr(parallel, "allreduce_slab_begin", lambda slab, local_n, global_n=None: None)
    with ops.kernel_trace() as tr:
        for t in range(T):
            b.learn(xs[t], y)
        torch.cuda.synchronize()
    monkeypatch.undo()
    n_learn = T - burnin + 1
    assert sum(n.startswith("k_bwd_wgrad_any") for n in tr.names) == 3 * n_learn == sum(n.startswith("k_bwd_wgrad") for n in tr.names), tr.names
    assert sum(n.startswith("k_bwd_reduce") for n in tr.names) == 3 * n_learn and tr.count("k_grad_reduce_adam") == 0, tr.names
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))


def test_a_9x9_layer_learns_with_the_flag_and_raises_without(dev):
    from snn_modulation_classification_amd import _lib, ops
    convs = lambda: [dict(out_channels=8, kernel_size=9, padding=4, pooling=2), dict(out_channels=12, kernel_size=5, padding=2, pooling=1)]
    B, hw, burnin = 3, (12, 12), 2
    rng = np.random.RandomState(2)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .2).astype(np.float32)).to(dev) for _ in range(4)]
    y = torch.zeros(B, 10)
    y[np.arange(B), rng.randint(0, 10, size=B)] = 1
    y = y.to(dev)
    net = _net(convs(), hw, B, 10, burnin, 1.0, False)
    assert net.backward_any_supported()
    net.learn(xs[0], y)                                     # burn-in: no backward yet
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.learn(xs[1], y)
    assert "64 taps" in str(e.value)
    net = _net(convs(), hw, B, 10, burnin, 1.0, False)
    net.any_learning_path = True
    w0 = net.dcll_slices[0].dclllayer.i2h.weight.detach().clone()
    with ops.kernel_trace() as tr:
        for x in xs:
            net.learn(x, y)
        torch.cuda.synchronize()
    assert sum(n.startswith("k_bwd_wgrad_any") for n in tr.names) == 2 * 3 and tr.count("k_grad_reduce_adam") == 3, tr.names
    w1 = net.dcll_slices[0].dclllayer.i2h.weight.detach()
    assert w1.shape == (8, 1, 9, 9) and bool(torch.isfinite(w1).all()) and not torch.equal(w0, w1)
    g = net.dcll_slices[0].dclllayer.i2h.weight.grad
    assert g is not None and float(g.abs().max()) > 0


def test_a_network_that_is_not_served_refuses_the_attribute(dev):
    from snn_modulation_classification_amd import _lib
    net = _net([dict(out_channels=40, kernel_size=3, padding=1, pooling=1)], (8, 8), 2, 10, 2, 1.0, False)
    assert not net.backward_any_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.any_learning_path = True
    assert net.any_learning_path is False
    net.any_learning_path = False                           # (switching it off is always allowed)


def test_entry_point_train_mnist_with_any_learning_path(tmp_path, capsys, monkeypatch):
    """train.py --data MNIST --any_learning_path on synthetic images, the sizes of test_entry_point_train_mnist_config1: exits
    normally with finite accuracies and every backward call of its learning steps takes the any path; without the flag the same
    command makes the same calls on the default path and prints no notice."""
    import train
    from snn_modulation_classification_amd import ops
    calls = []
    real = ops.conv_lif_backward

    def counted(*a, **kw):
        calls.append(bool(kw.get("any_path", False)) or kw.get("path") == "any")           # (the old keyword, or path=)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "conv_lif_backward", counted)
    common = ['--data', 'MNIST', '--network_spec', os.path.join(PKG, 'networks', 'mnist_conv.yaml'), '--synthetic', '16',
              '--batch_size', '8', '--batch_size_test', '8', '--n_test_samples', '8', '--n_steps', '2', '--n_iters', '10',
              '--n_iters_test', '10', '--burnin', '4', '--n_test_interval', '1', '--learning_rates', '1e-7']
    runs = {}
    for flag in (False, True):
        del calls[:]
        out_dir = train.main(common + ['--output', str(tmp_path / ('any' if flag else 'default'))] +
                             (['--any_learning_path'] if flag else []))
        text = capsys.readouterr().out
        acc = np.load(os.path.join(out_dir, 'acc_test.npy'))
        assert acc.shape == (2, 1, 3) and np.isfinite(acc).all()
        runs[flag] = (list(calls), text, torch.load(os.path.join(out_dir, 'parameters_1.pth')))
    assert not any(runs[False][0]) and "any_learning_path" not in runs[False][1]
    assert all(runs[True][0]) and len(runs[True][0]) == len(runs[False][0]) > 0
    assert "ignored" not in runs[True][1]
    for k, v in runs[True][2].items():
        assert bool(torch.isfinite(v).all()), k
