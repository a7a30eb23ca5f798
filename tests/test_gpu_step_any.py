"""GPU tests of dcll_conv_lif_step_any (ABI 10: k_lif_step_any, the opt-in MFMA per-step forward of any plain conv layer) on the
cases of tests/step_any_cases.py (proven on the CPU by tests/test_step_any_cases.py), through
snn_modulation_classification_amd.ops.conv_lif_step(any_path=True) — the binding the product uses.

Every case, three consecutive calls on one set of state buffers, against the pinned-order C oracle: v equal bit for bit up to the
sign of a zero, pooled spikes, eps0, eps1 and arp bit for bit, pv within 1e-4, p / o within 1e-4 of a float64 matmul of the
oracle's pv; the launch log equals the restated prediction; a second run gives the same bits; spikes and state equal
dcll_conv_lif_step's bit for bit; the other side of an NS threshold gives the same per-sample results.  Then the refusals, and
the network level: the per-step test loop, learning steps, graph capture, learn_sequence and train.py with any_step_path against
the default path."""
import collections
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import fuzz_cases as FZ
import step_any_cases as S
from conftest import ROOT, unpack_bits

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")

CASES = S.cases()
REFUSALS = S.refusals()
PV_TOL = 1e-4           # the sigmoid's contract (include/dcll_hip.h)
LOGIT_TOL = 1e-4        # the header's readout contract
GRAD_RTOL, GRAD_ATOL = 2e-3, 5e-5       # tests/test_gpu_bwd_any.py's network-level comparison: rtol, atol = 5e-5 * max|ref|
LAYER_KERNELS = ("k_lif_step", "k_trace", "k_conv_lif", "k_pool", "k_seq_any_wprep")

SERVED = collections.Counter()          # form -> cases it served
RAN = set()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a, dev, off16=False):
    """numpy -> device tensor; off16: placed one float into a larger buffer, so its address is 4 (mod 16)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off16:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, device=dev, dtype=t.dtype)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def bits_equal(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.astype(np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32))


def equal_up_to_zero_sign(a, b):
    """every value bit for bit, except that -0.0 and +0.0 count as equal (the zero link turns -0.0 into +0.0)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = a.view(np.uint32) == b.view(np.uint32)
    return a.shape == b.shape and bool(np.all(same | ((a == 0) & (b == 0))))


def conv_desc(c):
    from snn_modulation_classification_amd import ops
    d = ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                           (c["pool_h"], c["pool_w"]), c["target"], c["output_layer"], c["tau_tensor"],
                           1.0 if c["refractory"] else 0.0, c.get("alpharp", FZ.ALPHARP), c["stride"], c["dilation"], c["groups"])
    assert ops.conv_out_shape(d) == FZ.conv_shape(c)
    return d


def forward(c, T, dev, B, any_path, want_v=True):
    """The three steps of a case on the device at batch B (sample b = the case's sample b % c['B']) -> (per-step host copies,
    per-step kernel names).  misalign: every operand and every output of the layer call one float off a 16-byte boundary."""
    from snn_modulation_classification_amd import ops
    d = conv_desc(c)
    off = bool(c["misalign"]) and any_path
    idx = np.arange(B) % c["B"]
    ch, cw, ph, pw = FZ.conv_shape(c)
    W, b = cu(T["W"], dev, off), cu(T["b"], dev, off)
    tau = [cu(t, dev, off) for t in T["tau"]]
    eps0, eps1 = cu(T["eps0"][idx], dev, off), cu(T["eps1"][idx], dev, off)
    arp = cu(T["arp"][idx], dev, off) if c["refractory"] else None
    ro = dict(i2o_W=cu(T["i2o_W"], dev), i2o_b=cu(T["i2o_b"], dev)) if c["readout"] else {}
    if c["output_layer"]:
        ro.update(out_W=cu(T["out_W"], dev), out_b=cu(T["out_b"], dev))
    out = {}
    if off:
        out = dict(s=cu(np.zeros((B, c["c_out"], ph, pw), np.float32), dev, True), pv=cu(np.zeros((B, c["c_out"], ph, pw), np.float32), dev, True),
                   v=cu(np.zeros((B, c["c_out"], ch, cw), np.float32), dev, True),
                   w_scratch=cu(np.zeros(64 * S.steps(c), np.float32), dev, True))
    steps, logs = [], []
    h = lambda a: None if a is None else a.detach().cpu().numpy().copy()
    for t in range(len(T["x"])):          # (FZ.STEPS; tests/value_cases.py draws up to eight)
        with ops.kernel_trace() as tr:
            s, p, o, pv, v = ops.conv_lif_step(d, cu(T["x"][t][idx], dev, off), W, b, *tau, eps0, eps1, arp, out=out, want_v=want_v,
                                               any_path=any_path, **ro)
            torch.cuda.synchronize()
        logs.append(list(tr.names))
        steps.append(dict(s=h(s), p=h(p), o=h(o), pv=h(pv), v=h(v), eps0=h(eps0), eps1=h(eps1), arp=h(arp)))
    if any_path:
        assert "scratch" not in out and out["w_scratch"].numel() == 64 * S.steps(c)
    return steps, logs


def check_against_oracle(c, T, osteps, steps, B):
    idx = np.arange(B) % c["B"]
    for t, (g, o) in enumerate(zip(steps, osteps)):
        tag = (c["id"], "step %d" % t)
        assert bits_equal(g["eps0"], o["eps0"][idx]) and bits_equal(g["eps1"], o["eps1"][idx]), tag + ("traces",)
        if g["v"] is not None:
            assert equal_up_to_zero_sign(g["v"], o["v"][idx]), tag + ("v", float(np.abs(g["v"] - o["v"][idx]).max()))
        assert bits_equal(g["s"], o["s"][idx]), tag + ("pooled spikes",)
        if c["refractory"]:
            assert bits_equal(g["arp"], o["arp"][idx]), tag + ("arp",)
        print("%s step %d: max |pv - oracle| %.3g" % (c["id"], t, float(np.abs(g["pv"] - o["pv"][idx]).max())))
        np.testing.assert_allclose(g["pv"], o["pv"][idx], atol=PV_TOL, rtol=0, err_msg=str(tag))
        flat = o["pv"][idx].astype(np.float64).reshape(B, -1)
        if c["readout"]:
            p64 = flat @ T["i2o_W"].astype(np.float64).T + T["i2o_b"].astype(np.float64)
            np.testing.assert_allclose(g["p"], p64, atol=LOGIT_TOL, rtol=0, err_msg=str(tag + ("p",)))
        else:
            assert g["p"] is None
        if c["output_layer"]:
            o64 = flat @ T["out_W"].astype(np.float64).T + T["out_b"].astype(np.float64)
            np.testing.assert_allclose(g["o"], o64, atol=LOGIT_TOL, rtol=0, err_msg=str(tag + ("o",)))
        else:
            assert g["o"] is None


def check_log(c, logs, B):
    want = S.launch_log(c, B)
    for t, names in enumerate(logs):
        assert names[:len(want)] == want, (c["id"], "step %d" % t, names, want)
        assert not any(n.startswith(LAYER_KERNELS) for n in names[len(want):]), (c["id"], names)       # behind them: readouts only
        assert bool(names[len(want):]) == bool(c["readout"]), (c["id"], names)


def assert_same(a, b, keys, what, cid, rows=None):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            if x[k] is not None and y[k] is not None:
                assert bits_equal(x[k] if rows is None else x[k][:rows], y[k]), (cid, what, "step %d" % t, k)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle(dev, case):
    c = case
    print(S.describe(c))
    T, osteps = S.run(c)
    B = c["B_run"]
    form = S.form(c, B)
    steps, logs = forward(c, T, dev, B, True, want_v=bool(c["want_v"]))
    assert (steps[0]["v"] is None) == (not c["want_v"])
    check_log(c, logs, B)
    check_against_oracle(c, T, osteps, steps, B)
    again, logs2 = forward(c, T, dev, B, True, want_v=bool(c["want_v"]))
    assert logs2 == logs
    assert_same(steps, again, ("v", "s", "pv", "p", "o", "eps0", "eps1", "arp"), "a second run", c["id"])
    # dcll_conv_lif_step serves every plain conv layer: spikes and state bit for bit, v up to a zero's sign
    default, dlogs = forward(c, T, dev, B, False)
    assert not any(n.startswith(("k_lif_step_any", "k_seq_any_wprep")) for names in dlogs for n in names)
    assert_same(steps, default, ("s", "eps0", "eps1", "arp"), "dcll_conv_lif_step", c["id"])
    for t in range(FZ.STEPS):
        if steps[t]["v"] is not None:
            assert equal_up_to_zero_sign(steps[t]["v"], default[t]["v"]), (c["id"], "v of dcll_conv_lif_step", t)
        np.testing.assert_allclose(steps[t]["pv"], default[t]["pv"], atol=PV_TOL, rtol=0)
    if c["also_B"]:                     # the other side of an NS threshold: the same samples, per-sample results equal
        B2 = c["also_B"]
        assert S.ns(c, B2) != S.ns(c, B) and B2 <= c["B"]
        other, logs3 = forward(c, T, dev, B2, True)
        check_log(c, logs3, B2)
        assert_same(steps, other, ("v", "s", "pv", "eps0", "eps1", "arp"), "B = %d" % B2, c["id"], rows=B2)
        SERVED[S.form(c, B2)] += 1
    SERVED[form] += 1
    RAN.add(c["id"])


def test_every_form_served_a_case():
    """a parity test is only worth its name if it ran the kernel it claims to cover (runs behind the cases above)"""
    assert RAN == {c["id"] for c in CASES}, sorted({c["id"] for c in CASES} - RAN)
    assert set(SERVED) == set(S.all_forms()), dict(SERVED)
    forms = {S.form(c, c["B_run"]) for c in CASES if c["stratum"] == "forms" and c["id"] in RAN}
    assert forms == set(S.all_forms())
    print("cases per form:", dict(SERVED))


@pytest.mark.parametrize("ref", REFUSALS, ids=[r["id"] for r in REFUSALS])
def test_refusals_come_before_any_launch(dev, ref):
    """each with its code, a phrase of dcll_last_error(), an empty launch log and untouched buffers"""
    from snn_modulation_classification_amd import _lib, ops
    r = ref
    lib = _lib.get()
    d = ops.make_conv_desc(r["c_in"], r["c_out"], (r["h"], r["w"]), (r["kh"], r["kw"]), (r["pad_h"], r["pad_w"]),
                           (r["pool_h"], r["pool_w"]), 0, False, r["tau_tensor"], 1.0 if r["refractory"] else 0.0, FZ.ALPHARP,
                           r["stride"], r["dilation"], r["groups"])
    shp = FZ.conv_shape(r) or (1, 1, 1, 1)
    ch, cw, ph, pw = shp
    B, Bn = r["B"], max(r["B"], 1)
    SENT = 7.0
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(x=f(Bn, r["c_in"], r["h"], r["w"]), W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]),
             alpha=f(1), tau_m=f(1), alphas=f(1), tau_s=f(1), eps0=f(Bn, r["c_in"], r["h"], r["w"]), eps1=f(Bn, r["c_in"], r["h"], r["w"]),
             arp=f(Bn, r["c_out"], ch, cw), s=f(Bn, r["c_out"], ph, pw), pv=f(Bn, r["c_out"], ph, pw), v=f(Bn, r["c_out"], ch, cw),
             w_scratch=f(max(64 * S.steps(r), 64)))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_step_any(ctypes.byref(d), p["x"], p["W"], p["b"], p["alpha"], p["tau_m"], p["alphas"], p["tau_s"],
                                        p["eps0"], p["eps1"], p["arp"], None, None, None, None, p["s"], None, None, p["pv"], p["v"],
                                        p["w_scratch"], B, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode(), (r["id"], lib.dcll_last_error())
    assert tr.names == [], (r["id"], tr.names)
    for k, x in t.items():
        assert bool((x == SENT).all()), (r["id"], k, "was written")
    if r["code"] == "DCLL_ERR_UNSUPPORTED":
        assert not ops.step_any_supported(d) and ops.step_any_lds(d) == 0


def test_any_path_with_int8_weights_raises(dev):
    from snn_modulation_classification_amd import ops
    c = S.by_id("step-form-R1-fused")
    T, _ = S.run(c)
    d = conv_desc(c)
    q, scale, _ = FZ.quantize_int8(T["W"])
    with ops.kernel_trace() as tr, pytest.raises(ValueError):
        ops.conv_lif_step(d, cu(T["x"][0], dev), cu(T["W"], dev), cu(T["b"], dev), *[cu(a, dev) for a in T["tau"]], cu(T["eps0"], dev),
                          cu(T["eps1"], dev), cu(T["arp"], dev), q8=(torch.from_numpy(q).to(dev), torch.from_numpy(scale).to(dev)),
                          any_path=True)
    assert tr.names == []


# ------------------------------------------------------------------------------------------------------------------------------
# network level
# ------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = dict(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    a.update(kw)
    return Namespace(**a)


def _spec(name):
    from snn_modulation_classification_amd.networks import load_network_spec
    return load_network_spec(os.path.join(PKG, "networks", name))


def _net(convs, hw, B, target, arp, burnin=20, learn=False, graph=False, any_step=False, any_learn=False):
    from snn_modulation_classification_amd.networks import ConvNetwork
    torch.manual_seed(1)
    np.random.seed(1)
    kw = dict(loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam, opt_param={"betas": [0.0, .95], "weight_decay": 10.0},
              learning_rates=[1e-6]) if learn else dict(loss=None, opt=None, opt_param={}, learning_rates=None)
    net = ConvNetwork(_args(arp=arp), (1,) + tuple(hw), B, convs, target, act=torch.nn.Sigmoid(), burnin=burnin, **kw)
    net.graph_learn = graph
    net.reset(True)
    if learn:
        net.train()
    if any_step:
        assert net.step_any_supported() and all(s.step_any_supported() for s in net.dcll_slices) and net.any_step_path is False
        net.any_step_path = True
        assert net.any_step_path is True and all(s.dclllayer.i2h.any_step_path for s in net.dcll_slices)
    if any_learn:
        net.any_learning_path = True
    return net


def _per_layer_spikes(net, x_steps):
    """a network stepped layer by layer through Conv2dDCLLlayer's own step call -> per layer the pooled spikes (T, B, C, ph, pw)"""
    out = [[] for _ in net.dcll_slices]
    net.reset()
    with torch.no_grad():
        for t in range(len(x_steps)):
            cur = x_steps[t]
            for i, sl in enumerate(net.dcll_slices):
                L = sl.dclllayer
                cur = L.i2h._step(cur, L.pooling, L.i2o, L.output_ if L.output_layer else None,
                                  stacked=L.stacked_readout() if L.output_layer else None)[0]
                out[i].append(cur.cpu().numpy().copy())
    return [np.stack(o) for o in out]


def _one_hot(labels, T, n):
    y = torch.zeros(T, len(labels), n)
    y[:, np.arange(len(labels)), labels] = 1
    return y


def _test_loop_equal(a, b, x, n_classes, any_forms):
    """nets a (default) and b (any_step_path) through `for t: net.test(x[t])`: clout, votes, accuracy and final state equal; b's
    first step names k_lif_step_any for every layer and none of the generic kernels"""
    from snn_modulation_classification_amd import ops
    T, B = x.shape[:2]
    a.reset()
    b.reset()
    for t in range(T):
        a.test(x[t])
        with ops.kernel_trace() as tr:
            b.test(x[t])
        if t == 0:
            assert [n for n in tr.names if n.startswith("k_lif_step_any")] == any_forms, tr.names
            assert tr.names.count("k_seq_any_wprep") == 3 and not any(n.startswith(("k_conv_lif", "k_pool", "k_lif_step_c")) for n in tr.names)
    y = _one_hot(np.arange(B) % n_classes, T, n_classes)
    for sa, sb in zip(a.dcll_slices, b.dcll_slices):
        assert np.array_equal(np.array(sa.clout), np.array(sb.clout)) and np.array(sa.clout).shape == (T, B)
        assert np.array_equal(sa._predictions(y)[0], sb._predictions(y)[0])
        for u, v in zip(sa.dclllayer.i2h.state, sb.dclllayer.i2h.state):
            assert torch.equal(u, v)
    assert a.accuracy(y) == b.accuracy(y)


def test_network_mnist_config1_test_loop(dev, golden):
    """mnist_conv.yaml (BASELINE config 1), B = 4, fixture g2_mnist_t50_b4: the per-step test loop with any_step_path against the
    default path — every layer's spikes bit for bit, votes / clout equal, the launch log of a step."""
    g = golden("g2_mnist_t50_b4.npz")
    xs = unpack_bits(g["x"], 28 * 28)
    T, B = xs.shape[:2]
    x = torch.from_numpy(xs.reshape(T, B, 1, 28, 28)).to(dev)
    a = _net(_spec("mnist_conv.yaml"), (28, 28), B, 10, 0.0)
    b = _net(_spec("mnist_conv.yaml"), (28, 28), B, 10, 0.0, any_step=True)
    sa, sb = _per_layer_spikes(a, x), _per_layer_spikes(b, x)
    for i in range(3):
        assert sa[i].shape == sb[i].shape and np.array_equal(sa[i], sb[i]) and 0 < sa[i].mean() < 1, ("spikes", i)
    _test_loop_equal(a, b, x, 10, ["k_lif_step_any<0> (pooling)", "k_lif_step_any<0>", "k_lif_step_any<0> (pooling)"])
    agree = np.mean([np.mean(np.array(s.clout) == g["clout/%d" % i]) for i, s in enumerate(b.dcll_slices)])
    assert agree > 0.99


def test_network_radio_ml_24x24_test_loop(dev):
    """radio_ml_conv.yaml on 24x24, B = 3, refractory: the same comparison, and every layer's spikes equal the C oracle network's;
    the 32 -> 32 layers run the split form (18 tiles, three workgroups per sample)"""
    from oracle import c_oracle as C
    R, T, B = 24, 24, 3
    convs = _spec("radio_ml_conv.yaml")
    a = _net(_spec("radio_ml_conv.yaml"), (R, R), B, 24, 1.0)
    b = _net(convs, (R, R), B, 24, 1.0, any_step=True)
    cells = np.random.RandomState(0).randint(0, R * R, size=(T, B))
    xs = np.zeros((T, B, R * R), np.float32)
    xs[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    xs = xs.reshape(T, B, 1, R, R)
    x = torch.from_numpy(xs).to(dev)
    sds = [{k: v.detach().cpu().numpy() for k, v in s.dclllayer.state_dict().items()} for s in b.dcll_slices]
    orc = C.OracleConvNetwork(sds, convs, (R, R), 1.0)
    outs = [orc.step(xs[t]) for t in range(T)]
    sa, sb = _per_layer_spikes(a, x), _per_layer_spikes(b, x)
    for i in range(3):
        assert np.array_equal(sa[i], sb[i]) and 0 < sa[i].mean() < 1, ("spikes", i)
        assert np.array_equal(sb[i], np.stack([o[i]["s"] for o in outs])), ("oracle spikes", i)
    _test_loop_equal(a, b, x, 24, ["k_lif_step_any<1> (split)"] * 3)


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
            oa, ob = sa.optimizer, sb_.optimizer
            for pa, pb in zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"]):
                if pa in oa.state:
                    for key, val in oa.state[pa].items():
                        if torch.is_tensor(val):
                            ob.state[pb][key].copy_(val)
                        else:
                            ob.state[pb][key] = val


@pytest.mark.parametrize("any_learn", [False, True], ids=["step", "step+learning"])
@pytest.mark.parametrize("spec, hw, B, target, arp", [("mnist_conv.yaml", (28, 28), 4, 10, 0.0), ("radio_ml_conv.yaml", (24, 24), 3, 24, 1.0)],
                         ids=["mnist_conv-B4", "radio_ml_conv-24x24-B3"])
def test_network_learning_steps_vs_default_path(dev, spec, hw, B, target, arp, any_learn):
    """Two identically seeded networks, A on the default dispatch and B with any_step_path (alone, and with any_learning_path):
    before each of six learning steps B takes A's parameters, optimizer state and neuron state; then both learn.  Same spikes and
    readouts.  With any_learning_path the gradients are within the tolerance of tests/test_gpu_bwd_any.py's network-level
    comparison (another summation order).  With any_step_path alone they are EQUAL: observed on the MI355X for all 48 gradient
    tensors of the six steps of either network, as the forward hands the backward the default path's bits."""
    from snn_modulation_classification_amd import ops
    burnin, steps = 3, 6
    A = _net(_spec(spec), hw, B, target, arp, burnin=burnin, learn=True)
    Bn = _net(_spec(spec), hw, B, target, arp, burnin=burnin, learn=True, any_step=True, any_learn=any_learn)
    rng = np.random.RandomState(11)
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    y = y.to(dev)
    for t in range(burnin - 1 + steps):
        x = torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .15).astype(np.float32)).to(dev)
        _copy_everything(A, Bn)
        logs = []
        for net in (A, Bn):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(tr.names)
        assert not any(n.startswith(("k_lif_step_any", "k_seq_any_wprep")) for n in logs[0])
        assert sum(n.startswith("k_lif_step_any") for n in logs[1]) == 3 == logs[1].count("k_seq_any_wprep"), logs[1]
        assert not any(n.startswith(("k_conv_lif", "k_pool", "k_lif_step_c")) for n in logs[1]), logs[1]
        assert any(n.startswith("k_bwd_wgrad_any") for n in logs[1]) == (any_learn and t >= burnin - 1)
        for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):
            for key in ("s", "p"):
                if torch.is_tensor(sa._learn_bufs.get(key)):
                    assert torch.equal(sa._learn_bufs[key], sb._learn_bufs[key]), (t, key)
            if torch.is_tensor(sa._learn_bufs.get("pv")):
                assert float((sa._learn_bufs["pv"] - sb._learn_bufs["pv"]).abs().max()) <= PV_TOL
        if t < burnin - 1:
            continue
        for i, (sa, sb) in enumerate(zip(A.dcll_slices, Bn.dcll_slices)):
            for (name, pa), (_, pb) in zip(sa.dclllayer.named_parameters(), sb.dclllayer.named_parameters()):
                assert (pa.grad is None) == (pb.grad is None), name
                if pa.grad is None:
                    continue
                ref, got = pa.grad.detach().cpu().double().numpy(), pb.grad.detach().cpu().double().numpy()
                scale = float(np.abs(ref).max())
                print("%s step %d slice %d %s.grad: max|diff| %.3g, max|ref| %.3g, equal %s" % (spec, t, i, name, np.abs(got - ref).max(), scale,
                                                                                           np.array_equal(got, ref)))
                if any_learn:
                    np.testing.assert_allclose(got, ref, rtol=GRAD_RTOL, atol=GRAD_ATOL * scale + 1e-30, err_msg="%s %d %s" % (spec, t, name))
                else:
                    assert np.array_equal(got, ref), (spec, t, i, name)


def _drive(net, xs, y, learn):
    for x in xs:
        if learn:
            net.learn(x, y)
        else:
            net.test(x)
    torch.cuda.synchronize()


@pytest.mark.parametrize("learn", [False, True], ids=["test", "learn"])
def test_graph_captured_steps_equal_eager_steps(dev, learn):
    """With any_step_path the timestep replayed from its captured graph == the step launched eagerly, bit for bit, at B = 8
    (mnist_conv.yaml; ConvNetwork.graph_learn switches both captures); toggling the flag retakes the capture."""
    B, T, burnin, hw = 8, 16, 4, (28, 28)
    rng = np.random.RandomState(4)
    xs = [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .15).astype(np.float32)).to(dev) for _ in range(T)]
    y = torch.zeros(B, 10)
    y[np.arange(B), rng.randint(0, 10, size=B)] = 1
    y = y.to(dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(_spec("mnist_conv.yaml"), hw, B, 10, 0.0, burnin=burnin, learn=learn, graph=graph, any_step=True)
        _drive(net, xs, y, learn)
    a, b = nets[True], nets[False]
    graphs = lambda n: n._learn_graphs if learn else n._test_graphs
    key = ((B, 1) + hw, (B, 10)) if learn else (B, 1) + hw
    g = graphs(a)[key]
    assert g["n"] >= 6 and not graphs(b), (g["n"],)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)
    # the flag is part of the capture's signature: switched off, the capture on record is dropped and, after eager steps of the
    # default path, a new one is taken; both networks stay equal
    sig = a._graph_signature() if learn else a._test_signature()
    a.any_step_path = b.any_step_path = False
    assert (a._graph_signature() if learn else a._test_signature()) != sig
    from snn_modulation_classification_amd import ops
    with ops.kernel_trace() as tr:
        _drive(a, xs[:1], y, learn)
    assert graphs(a).get(key) is not g and not any(n.startswith("k_lif_step_any") for n in tr.names) and any(n.startswith("k_conv_lif") for n in tr.names)
    _drive(a, xs[1:8], y, learn)
    _drive(b, xs[:8], y, learn)
    g2 = graphs(a).get(key)
    assert g2 is not None and g2 is not g and g2["n"] >= 1
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)


def test_learn_sequence_equals_per_step_learning(dev):
    """ConvNetwork.learn_sequence with any_step_path (radio_ml_conv.yaml on 24x24, cells on the device) == the loop
    `for t: net.learn(x[t], y)` on the same planes with the flag: weights, Adam state and clout bit for bit"""
    from snn_modulation_classification_amd import ops
    B, T, burnin, R = 4, 11, 6, 24
    rng = np.random.RandomState(3)
    cells = rng.randint(0, R * R, size=(T, B)).astype(np.int32)
    y = torch.zeros(B, 24)
    y[np.arange(B), rng.randint(0, 24, size=B)] = 1
    y = y.to(dev)
    a = _net(_spec("radio_ml_conv.yaml"), (R, R), B, 24, 1.0, burnin=burnin, learn=True, any_step=True)
    b = _net(_spec("radio_ml_conv.yaml"), (R, R), B, 24, 1.0, burnin=burnin, learn=True, any_step=True)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    assert sum(n.startswith("k_lif_step_any") for n in tr.names) == 3 * T and not any(n.startswith("k_conv_lif") for n in tr.names), tr.names
    x = np.zeros((T, B, R * R), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape(T, B, 1, R, R)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        st_a, st_b = sl_a.optimizer.state[sl_a.dclllayer.i2h.weight], sl_b.optimizer.state[sl_b.dclllayer.i2h.weight]
        assert float(st_a["step"]) == float(st_b["step"]) == T - burnin + 1 and torch.equal(st_a["exp_avg_sq"], st_b["exp_avg_sq"])


def test_networks_that_are_not_served_refuse_the_attribute(dev):
    """radio_ml_conv_ref.yaml (c_out 64) and a network with int8 weights: the setter raises DCLLUnsupported, the flag stays off"""
    from snn_modulation_classification_amd import _lib, quant
    net = _net(_spec("radio_ml_conv_ref.yaml"), (16, 128), 2, 24, 1.0)       # (the 128-wide plane its seven (1,2) poolings need)
    assert not net.step_any_supported() and max(s.dclllayer.out_channels for s in net.dcll_slices) == 64
    with pytest.raises(_lib.DCLLUnsupported):
        net.any_step_path = True
    assert net.any_step_path is False
    net.any_step_path = False                               # (switching it off is always allowed)
    net = _net(_spec("radio_ml_conv.yaml"), (24, 24), 2, 24, 1.0).to(dev)
    assert net.step_any_supported()
    quant.apply_int8_weights(net)
    assert all(s.dclllayer.i2h.int8_weights() is not None for s in net.dcll_slices) and not net.step_any_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.any_step_path = True
    assert net.any_step_path is False


class _trace:
    """ops.kernel_trace, imported late (the package loads the library on import of ops)"""

    def __enter__(self):
        from snn_modulation_classification_amd import ops
        self._tr = ops.kernel_trace()
        return self._tr.__enter__()

    def __exit__(self, *exc):
        return self._tr.__exit__(*exc)


@pytest.mark.parametrize("which", ["mnist", "radio24"])
def test_entry_point_train_any_step_path(tmp_path, capsys, which):
    """train.py (MNIST config 1; RadioML on a 24x24 plane) with --any_step_path prints and stores the metrics of the same command
    without the flag and runs every per-step layer call on k_lif_step_any; on RadioML together with --any_learning_path"""
    import train
    if which == "mnist":
        common = ['--data', 'MNIST', '--network_spec', os.path.join(PKG, 'networks', 'mnist_conv.yaml'), '--synthetic', '16',
                  '--batch_size', '8', '--batch_size_test', '8', '--n_test_samples', '8', '--n_steps', '1', '--n_iters', '10',
                  '--n_iters_test', '10', '--burnin', '4', '--n_test_interval', '1', '--learning_rates', '1e-7']
    else:
        common = ['--I_resolution', '24', '--Q_resolution', '24', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
                  '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '12',
                  '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    runs = {}
    flagged = ("step", ['--any_step_path']) if which == "mnist" else ("both", ['--any_step_path', '--any_learning_path'])
    for name, flags in (("default", []), flagged):
        with _trace() as tr:
            out = train.main(common + ['--output', str(tmp_path / name)] + flags)
        text = capsys.readouterr().out
        runs[name] = (np.load(os.path.join(out, 'acc_test.npy')), list(tr.names), text)
        assert "ignored" not in text
    a, names, _ = runs["default"]
    assert a.shape == (1, 1, 3) and np.isfinite(a).all() and not any(n.startswith("k_lif_step_any") for n in names)
    for name in (flagged[0],):
        b, names, _ = runs[name]
        assert np.array_equal(a, b), (name, a, b)
        assert any(n.startswith("k_lif_step_any") for n in names) and not any(n.startswith(("k_conv_lif", "k_pool")) for n in names)
        assert any(n.startswith("k_bwd_wgrad_any") for n in names) == (name == "both")


def test_entry_point_test_radio_ml_on_the_any_step_path(tmp_path, capsys, monkeypatch):
    """test_radio_ml.py --no_sequence_path on a 24x24 plane with DCLL_ANY_STEP_PATH=1 (the script has no flag of its own) prints
    the per-SNR accuracies of the same command without it, and its per-step loop runs k_lif_step_any; on radio_ml_conv_ref.yaml
    the switch is ignored with a notice"""
    import test_radio_ml as cli
    common = ["--I_resolution", "24", "--Q_resolution", "24", "--arp", "1.0", "--burnin", "4", "--batch_size_test", "8",
              "--n_test_samples", "8", "--synthetic", "8", "--n_iters_test", "12", "--min_snr", "10", "--max_snr", "10", "--no_sequence_path"]
    runs = {}
    for name in ("default", "any"):
        if name == "any":
            monkeypatch.setenv("DCLL_ANY_STEP_PATH", "1")
        with _trace() as tr:
            cli.main(common + ["--out_dir", str(tmp_path / name)])
        text = capsys.readouterr().out
        runs[name] = (np.load(tmp_path / name / "snr_evaluation_accs.npy"), [l for l in text.splitlines() if l.startswith("SNR")], list(tr.names))
        assert "ignored" not in text
    assert np.array_equal(runs["default"][0], runs["any"][0]) and runs["default"][1] == runs["any"][1] and runs["any"][1]
    assert not any(n.startswith("k_lif_step_any") for n in runs["default"][2]) and any(n.startswith("k_conv_lif") for n in runs["default"][2])
    assert any(n.startswith("k_lif_step_any") for n in runs["any"][2]) and not any(n.startswith(("k_conv_lif", "k_pool")) for n in runs["any"][2])
    cli.main(["--I_resolution", "128", "--Q_resolution", "16", "--arp", "1.0", "--burnin", "4", "--batch_size_test", "2", "--n_test_samples", "2",
              "--synthetic", "2", "--n_iters_test", "4", "--min_snr", "10", "--max_snr", "10", "--no_sequence_path",
              "--network_spec", os.path.join(PKG, "networks", "radio_ml_conv_ref.yaml"), "--out_dir", str(tmp_path / "ref")])
    assert "DCLL_ANY_STEP_PATH ignored" in capsys.readouterr().out
    monkeypatch.delenv("DCLL_ANY_STEP_PATH")
    net = _net(_spec("radio_ml_conv.yaml"), (24, 24), 2, 24, 1.0)
    assert net.any_step_path is False                       # (unset: nothing changes)
