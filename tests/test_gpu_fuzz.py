"""Seeded random-geometry differential tests of the per-step C ABI: dcll_conv_lif_step, dcll_conv_lif_backward[_open],
dcll_dense_lif_step, dcll_dense_lif_backward[_open] through snn_modulation_classification_amd.ops (the binding the product
uses), on the cases of tests/fuzz_cases.py (proven on the CPU by tests/test_fuzz_cases.py).

Forward, each of 3 steps, against the pinned-order C oracle: v, pooled spikes, eps0, eps1, arp bit for bit (the header's
arithmetic contract); pv within 2e-6; p and o within 1e-4 of a float64 matmul of the oracle's pv.  int8 cases also equal the call
on the dequantised fp32 tensor, the mis-aligned twins their aligned run, bit for bit.

Backward after step 3 against the float64 reference of fuzz_cases.conv_backward_ref / dense_backward_ref, evaluated from the
ORACLE's v and state; the one input taken from the device is the pool-routing index map — the first maximum of the un-pooled fp32 pv
the FORWARD left in its scratch, itself checked against sigmoid(oracle v) — because which of two nearly equal sigmoids wins is
defined by the device's sigmoid alone.  Closed form within rtol 2e-3, atol 5e-5 max|ref| (the project's tolerance for this
comparison, test_backward_on_large_planes); open form + dcll_grad_reduce_adam and the v == NULL form: the closed form's bits.

The last test asserts which kernels served the cases (dcll_kernel_trace): a parity test is only worth its name if it ran the
kernel it claims to cover."""
import collections
import time

import numpy as np
import pytest
import torch

import fuzz_cases as FZ

pytestmark = pytest.mark.gpu

CONV = FZ.conv_cases()
DENSE = FZ.dense_cases()
REFUSE = FZ.conv_refusals()
FREE = [c for c in CONV if c["stratum"] == "free"]
EDGE = [c for c in CONV if c["stratum"] == "edge"]

PV_TOL = 2e-6           # test_options_through_the_c_abi_vs_oracle
LOGIT_TOL = 1e-4        # the header's readout contract
GRAD_RTOL, GRAD_ATOL = 2e-3, 5e-5       # test_backward_on_large_planes: rtol, atol = 5e-5 * max|ref|

SERVED = collections.Counter()          # kernel name -> number of cases at least one of whose calls launched it
RAN = set()                             # ids of the cases that ran to the end
TIMES = collections.Counter()           # seconds: oracle (tensors + C oracle), ref (float64 reference), gpu (calls + copies)


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


def assert_grad(got, ref, what, cid):
    ref = ref.numpy()
    got = got.detach().cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    err = np.abs(got - ref)
    worst = float((err - GRAD_RTOL * np.abs(ref)).max())
    print("%s %s: max|err| %.3g, max|ref| %.3g, worst excess over rtol %.3g (atol %.3g)" % (cid, what, err.max(), scale, worst,
                                                                                             GRAD_ATOL * scale))
    np.testing.assert_allclose(got, ref, rtol=GRAD_RTOL, atol=GRAD_ATOL * scale + 1e-30, err_msg="%s %s" % (cid, what))


def conv_desc(c):
    from snn_modulation_classification_amd import ops
    d = ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                           (c["pool_h"], c["pool_w"]), c["target"], c["output_layer"], c["tau_tensor"],
                           1.0 if c["refractory"] else 0.0, c.get("alpharp", FZ.ALPHARP), c["stride"], c["dilation"], c["groups"])
    assert ops.conv_out_shape(d) == FZ.conv_shape(c)
    return d


def conv_forward(c, T, dev, off16=False, dequantised=False):
    """The steps of a case on the device (three; tests/value_cases.py draws up to eight) -> (per-step dict of host copies, the last
    step's device tensors, kernel names)."""
    from snn_modulation_classification_amd import ops
    d = conv_desc(c)
    pooled = not (c["pool_h"] == 1 and c["pool_w"] == 1)
    W, b = cu(T["W"], dev), cu(T["b"], dev)
    q8 = None
    if T["q8"] is not None and not dequantised:
        q8 = (torch.from_numpy(T["q8"][0]).to(dev), torch.from_numpy(T["q8"][1]).to(dev))
    tau = [cu(t, dev, off16 and c["tau_tensor"]) for t in T["tau"]]
    eps0, eps1 = cu(T["eps0"], dev, off16), cu(T["eps1"], dev, off16)
    arp = cu(T["arp"], dev) if c["refractory"] else None
    ro = dict(i2o_W=cu(T["i2o_W"], dev), i2o_b=cu(T["i2o_b"], dev)) if c["readout"] else {}
    if c["output_layer"]:
        ro.update(out_W=cu(T["out_W"], dev), out_b=cu(T["out_b"], dev))
    steps, out = [], {}
    with ops.kernel_trace() as tr:
        for t in range(len(T["x"])):
            s, p, o, pv, v = ops.conv_lif_step(d, cu(T["x"][t], dev, off16), W, b, *tau, eps0, eps1, arp, out=out, q8=q8, **ro)
            h = lambda a: None if a is None else a.detach().cpu().numpy().copy()
            steps.append(dict(s=h(s), p=h(p), o=h(o), pv=h(pv), v=h(v), eps0=h(eps0), eps1=h(eps1), arp=h(arp),
                              pv_full=h(out["scratch"][1]) if pooled else None))
    last = dict(d=d, eps1=eps1, v=v, pv=pv, i2o_W=ro.get("i2o_W"))
    return steps, last, tr.names


def check_conv_forward(c, T, osteps, steps):
    for t, (g, o) in enumerate(zip(steps, osteps)):
        tag = (c["id"], "step %d" % t)
        assert bits_equal(g["eps0"], o["eps0"]) and bits_equal(g["eps1"], o["eps1"]), tag + ("traces",)
        assert bits_equal(g["v"], o["v"]), tag + ("v", float(np.abs(g["v"] - o["v"]).max()))
        assert bits_equal(g["s"], o["s"]), tag + ("pooled spikes",)
        if c["refractory"]:
            assert bits_equal(g["arp"], o["arp"]), tag + ("arp",)
        np.testing.assert_allclose(g["pv"], o["pv"], atol=PV_TOL, rtol=0, err_msg=str(tag))
        if g["pv_full"] is not None:      # the un-pooled fp32 pv of the forward: the routing of the backward reference
            ref = 1.0 / (1.0 + np.exp(-o["v"].astype(np.float64)))
            np.testing.assert_allclose(g["pv_full"], ref, atol=PV_TOL, rtol=0, err_msg=str(tag + ("un-pooled pv",)))
        flat = o["pv"].astype(np.float64).reshape(c["B"], -1)
        if c["readout"]:
            p64 = flat @ T["i2o_W"].astype(np.float64).T + T["i2o_b"].astype(np.float64)
            np.testing.assert_allclose(g["p"], p64, atol=LOGIT_TOL, rtol=0, err_msg=str(tag + ("p",)))
        else:
            assert g["p"] is None
        if c["output_layer"]:
            o64 = flat @ T["out_W"].astype(np.float64).T + T["out_b"].astype(np.float64)
            np.testing.assert_allclose(g["o"], o64, atol=LOGIT_TOL, rtol=0, err_msg=str(tag + ("o",)))


def assert_same_run(a, b, what, cid):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("v", "s", "eps0", "eps1", "arp"):
            if x[k] is not None:
                assert bits_equal(x[k], y[k]), (cid, what, "step %d" % t, k)


def conv_backward(c, T, osteps, steps, last, dev):
    from snn_modulation_classification_amd import ops
    d = last["d"]
    want_out = bool(c["output_layer"])
    g = {k: cu(T[k], dev) for k in ("g_p", "g_o", "g_pv", "g_v")}
    args = (g["g_p"], g["g_o"], g["g_pv"], g["g_v"], last["i2o_W"])
    with ops.kernel_trace() as tr:
        dW, db, doW, dob = ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out={})
        out2 = {}
        ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out=out2, open_reduce=True)
        out2["dW"].fill_(float("nan"))
        out2["db"].fill_(float("nan"))
        ops.grad_reduce_adam([dict(out2["parts"])], [])
        out3 = None
        if c["pool_h"] == 1 and c["pool_w"] == 1 and c["target"] <= 32:
            out3 = {}
            ops.conv_lif_backward(d, last["eps1"], None, last["pv"], *args, want_out=want_out, out=out3)
        torch.cuda.synchronize()
    cid = c["id"]
    for k, a in (("dW", dW), ("db", db)) + ((("d_outW", doW), ("d_outb", dob)) if want_out else ()):
        assert bits_equal(out2[k], a), (cid, "open form + dcll_grad_reduce_adam", k)
        if out3 is not None:
            assert bits_equal(out3[k], a), (cid, "v == NULL form", k)
    t0 = time.time()
    pv_full = steps[-1]["pv_full"]
    route = FZ.identity_route(c) if pv_full is None else FZ.first_max_route(c, torch.from_numpy(pv_full))
    ref = FZ.conv_backward_ref(c, T, osteps[-1]["v"], osteps[-1]["eps1"], route)
    TIMES["ref"] += time.time() - t0
    assert_grad(dW, ref["dW"], "dW", cid)
    assert_grad(db, ref["db"], "db", cid)
    if want_out:
        assert_grad(doW, ref["d_outW"], "d_outW", cid)
        assert_grad(dob, ref["d_outb"], "d_outb", cid)
    return tr.names


def run_conv_case(c, dev):
    print(FZ.describe(c))
    t0 = time.time()
    T, osteps = FZ.conv_run(c)
    TIMES["oracle"] += time.time() - t0
    names = set()
    try:
        t0 = time.time()
        steps, last, n = conv_forward(c, T, dev)
        names |= set(n)
        check_conv_forward(c, T, osteps, steps)
        if c["q8"]:
            twin, _, n2 = conv_forward(c, T, dev, dequantised=True)
            names |= set(n2)
            assert_same_run(steps, twin, "int8 weights vs the dequantised fp32 tensor", c["id"])
        if c["misalign"]:
            twin, _, n2 = conv_forward(c, T, dev, off16=True)
            names |= set(n2)
            # (aligned: the vector trace pass + the tiled MFMA step; one float off: neither — k_lif_step_c32 on the 16x16 plane, the
            #  generic k_trace + k_conv_lif_tiled path elsewhere)
            assert "k_trace4" in n and not any(k == "k_trace4" or k.startswith(("k_lif_step_c32t", "k_lif_step_c1 (tiled)")) for k in n2), \
                (c["id"], n, n2)
            assert_same_run(steps, twin, "ptr16 false vs the aligned run", c["id"])
        names |= set(conv_backward(c, T, osteps, steps, last, dev))
        TIMES["gpu"] += time.time() - t0
        RAN.add(c["id"])
    finally:
        print("kernels:", sorted(names))
        SERVED.update(names)


@pytest.mark.parametrize("case", EDGE, ids=[c["id"] for c in EDGE])
def test_conv_dispatch_boundaries(dev, case):
    run_conv_case(case, dev)


@pytest.mark.parametrize("case", FREE, ids=[c["id"] for c in FREE])
def test_conv_free_draws(dev, case):
    run_conv_case(case, dev)


@pytest.mark.parametrize("case", DENSE, ids=[c["id"] for c in DENSE])
def test_dense_cases(dev, case):
    from snn_modulation_classification_amd import ops
    c = case
    print(FZ.describe(c))
    t0 = time.time()
    T, osteps = FZ.dense_run(c)
    TIMES["oracle"] += time.time() - t0
    t0 = time.time()
    d = ops.DenseDesc(c["in_features"], c["out_features"], c["target"], c["tau_tensor"], c["refractory"], FZ.ALPHARP,
                      1.0 if c["refractory"] else 0.0)
    W, b, tau = cu(T["W"], dev), cu(T["b"], dev), [cu(t, dev) for t in T["tau"]]
    eps0, eps1 = cu(T["eps0"], dev), cu(T["eps1"], dev)
    arp = cu(T["arp"], dev) if c["refractory"] else None
    i2o_W, i2o_b = cu(T["i2o_W"], dev), cu(T["i2o_b"], dev)
    names = set()
    try:
        with ops.kernel_trace() as tr:
            for t in range(FZ.STEPS):
                s, p, pv, v = ops.dense_lif_step(d, cu(T["x"][t], dev), W, b, *tau, eps0, eps1, arp, i2o_W, i2o_b)
                o = osteps[t]
                tag = (c["id"], "step %d" % t)
                assert bits_equal(eps0, o["eps0"]) and bits_equal(eps1, o["eps1"]), tag + ("traces",)
                assert bits_equal(v, o["v"]), tag + ("v",)
                assert bits_equal(s, o["s"]), tag + ("spikes",)
                if c["refractory"]:
                    assert bits_equal(arp, o["arp"]), tag + ("arp",)
                np.testing.assert_allclose(pv.cpu().numpy(), o["pv"], atol=PV_TOL, rtol=0, err_msg=str(tag))
                p64 = o["pv"].astype(np.float64) @ T["i2o_W"].astype(np.float64).T + T["i2o_b"].astype(np.float64)
                np.testing.assert_allclose(p.cpu().numpy(), p64, atol=LOGIT_TOL, rtol=0, err_msg=str(tag + ("p",)))
            g = [cu(T[k], dev) for k in ("g_p", "g_pv", "g_v")]
            dW, db = ops.dense_lif_backward(d, eps1, pv, *g, i2o_W, out={})
            out2 = {}
            ops.dense_lif_backward(d, eps1, pv, *g, i2o_W, out=out2, open_reduce=True)
            out2["dW"].fill_(float("nan"))
            out2["db"].fill_(float("nan"))
            ops.grad_reduce_adam([dict(out2["parts"])], [])
            torch.cuda.synchronize()
        names = set(tr.names)
        assert bits_equal(out2["dW"], dW) and bits_equal(out2["db"], db), (c["id"], "open form + dcll_grad_reduce_adam")
        t1 = time.time()
        ref = FZ.dense_backward_ref(c, T, osteps[-1]["v"], osteps[-1]["eps1"])
        TIMES["ref"] += time.time() - t1
        assert_grad(dW, ref["dW"], "dW", c["id"])
        assert_grad(db, ref["db"], "db", c["id"])
        TIMES["gpu"] += time.time() - t0
        RAN.add(c["id"])
    finally:
        print("kernels:", sorted(names))
        SERVED.update(names)


@pytest.mark.parametrize("open_form", [False, True], ids=["closed", "open"])
@pytest.mark.parametrize("case", REFUSE, ids=[c["id"] for c in REFUSE])
def test_backward_refusals(dev, case, open_form):
    """Geometries the backward does not serve: DCLL_ERR_UNSUPPORTED from both entry points, dcll_last_error() names the reason,
    dW / db untouched.  (Ordinary error returns: the launcher refuses before the weight-gradient kernel would be launched.)"""
    from snn_modulation_classification_amd import _lib, ops
    c = case
    print(FZ.describe(c))
    rng = np.random.RandomState(c["seed"] % (2 ** 31))
    d = conv_desc(c)
    ch, cw, ph, pw = FZ.conv_shape(c)
    B = c["B"]
    eps1 = cu(rng.uniform(0, 3, size=(B, c["c_in"], c["h"], c["w"])).astype(np.float32), dev)
    v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    g_v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    out = dict(dW=torch.full((c["c_out"], c["c_in"] // c["groups"], c["kh"], c["kw"]), -7.25, device=dev),
               db=torch.full((c["c_out"],), -7.25, device=dev))
    with pytest.raises(_lib.DCLLUnsupported) as e:         # (= the call returned DCLL_ERR_UNSUPPORTED: _lib.check)
        ops.conv_lif_backward(d, eps1, v, None, None, None, None, g_v, None, want_out=False, out=out, open_reduce=open_form)
    msg = _lib.get().dcll_last_error().decode()
    reason = "64 taps" if c["kh"] * c["kw"] > FZ.WG_MAXTAPS else "too wide"
    assert reason in msg and reason in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    assert bool((out["dW"] == -7.25).all()) and bool((out["db"] == -7.25).all())
    assert "parts" not in out


def test_open_multi_on_grouped_layers_equals_the_closed_calls(dev):
    """dcll_conv_lif_backward_open_multi through ops.conv_lif_backward(defer=...) on layers with groups > 1: the partial rows
    are (c_in / groups) * kh * kw + 1 long (ops described them with c_in * kh * kw + 1 and grad_reduce_adam refused them)."""
    from snn_modulation_classification_amd import ops
    grouped = [c for c in EDGE + FREE if c["groups"] > 1][:3]
    assert len(grouped) == 3
    closed, deferred, outs = [], [], []
    for c in grouped:
        T, _ = FZ.conv_run(c)
        _, last, _ = conv_forward(c, T, dev)
        g = [cu(T[k], dev) for k in ("g_p", "g_o", "g_pv", "g_v")]
        args = (last["d"], last["eps1"], last["v"], last["pv"], *g, last["i2o_W"])
        closed.append(ops.conv_lif_backward(*args, want_out=bool(c["output_layer"]), out={}))
        outs.append({})
        ops.conv_lif_backward(*args, want_out=bool(c["output_layer"]), out=outs[-1], open_reduce=True, defer=deferred)
    ops.conv_lif_backward_open_multi(deferred)
    for c, want, out in zip(grouped, closed, outs):
        assert out["parts"]["rowlen"] == (c["c_in"] // c["groups"]) * c["kh"] * c["kw"] + 1
        ops.grad_reduce_adam([dict(out["parts"])], [])
        assert bits_equal(out["dW"], want[0]) and bits_equal(out["db"], want[1]), c["id"]
        if c["output_layer"]:
            assert bits_equal(out["d_outW"], want[2]) and bits_equal(out["d_outb"], want[3]), c["id"]


@pytest.mark.parametrize("open_form", [False, True], ids=["closed", "open"])
def test_expanded_gradients_equal_their_contiguous_copies(dev, open_form):
    """g_p and g_pv (and g_v) as stride-0 expanded tensors in ONE call — what a .sum() / .mean() loss hands to backward — against
    the call on their .contiguous() copies, conv and dense.  The copies ops makes must all be alive when the call is enqueued:
    the three have the same size here, so a copy freed early would hand its block to the next one."""
    from snn_modulation_classification_amd import ops
    rng = np.random.RandomState(77)
    B, N = 6, 32
    e = lambda val, shape: torch.full((1,) * len(shape), val, device=dev).expand(*shape)
    # conv: c_out * ph * pw == target == c_out * ch * cw (no pooling): g_p, g_pv, g_v are 6 x 32 floats each
    d = ops.make_conv_desc(3, 2, (4, 4), 3, 1, 1, N, False, False, 1.0, FZ.ALPHARP)
    eps1 = cu(rng.uniform(0, 3, size=(B, 3, 4, 4)).astype(np.float32), dev)
    v = cu(rng.randn(B, 2, 4, 4).astype(np.float32), dev)
    pv = torch.sigmoid(v)
    i2o_W = cu(rng.uniform(-.3, .3, size=(N, 32)).astype(np.float32), dev)
    g = (e(.3, (B, N)), None, e(-.7, (B, 2, 4, 4)), e(.05, (B, 2, 4, 4)))
    assert not any(t.is_contiguous() for t in g if t is not None)

    def conv(grads):
        out = {}
        ops.conv_lif_backward(d, eps1, v, pv, *grads, i2o_W, want_out=False, out=out, open_reduce=open_form)
        if open_form:
            ops.grad_reduce_adam([dict(out["parts"])], [])
        return out["dW"].clone(), out["db"].clone()
    want = conv(tuple(None if t is None else t.contiguous() for t in g))
    got = conv(g)
    assert float(want[0].abs().max()) > 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "conv: expanded gradients"
    # dense: out_features == target
    dd = ops.DenseDesc(20, N, N, 0, 1, FZ.ALPHARP, 1.0)
    eps1 = cu(rng.uniform(0, 3, size=(B, 20)).astype(np.float32), dev)
    pv = torch.sigmoid(cu(rng.randn(B, N).astype(np.float32), dev))
    i2o_W = cu(rng.uniform(-.3, .3, size=(N, N)).astype(np.float32), dev)
    g = (e(.3, (B, N)), e(-.7, (B, N)), e(.05, (B, N)))

    def dense(grads, pv_):
        out = {}
        ops.dense_lif_backward(dd, eps1, pv_, *grads, i2o_W, out=out, open_reduce=open_form)
        if open_form:
            ops.grad_reduce_adam([dict(out["parts"])], [])
        return out["dW"].clone(), out["db"].clone()
    want = dense(tuple(t.contiguous() for t in g), pv)
    got = dense(g, pv.t().contiguous().t())         # (pv non-contiguous as well: a fourth copy)
    assert float(want[0].abs().max()) > 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "dense: expanded gradients"


# the kernel families the strata aim at (names of the launch log, csrc/*.hip HIP_CHECK_LAUNCH)
FAMILIES = [
    "k_trace", "k_trace4", "k_conv_lif", "k_conv_lif_tiled<7,7>", "k_conv_lif_tiled<5,5>", "k_conv_lif_tiled<3,3>",
    "k_conv_lif_tiled<1,3>", "k_pool", "k_lif_step_c32", "k_lif_step_c32t (8-row tiles)", "k_lif_step_c32t", "k_lif_step_c1",
    "k_lif_step_c1 (tiled)", "k_readout_rows", "k_readout_t16", "k_readout", "k_dense_lif_mfma (narrow)", "k_dense_lif_mfma (wide)",
    "k_bwd_dv"] + ["k_bwd_dv_nopool<%d>%s" % (n, f) for n in (8, 16, 24, 32) for f in ("", " (from pv)")] + [
    "k_bwd_wgrad", "k_bwd_wgrad (row bands)", "k_bwd_wgrad_c32", "k_bwd_wgrad_c1", "k_bwd_wgrad_c1 (tiled)", "k_bwd_wgrad_c32 (tiled)",
    "k_bwd_reduce", "k_bwd_reduce4<4>", "k_bwd_reduce4<16>", "k_bwd_outgrad_mfma", "k_bwd_outgrad_part", "k_bwd_outgrad_reduce",
    "k_bwd_outgrad", "k_dense_bwd_dv", "k_dense_bwd_wgrad", "k_grad_reduce_adam"]


def test_every_kernel_family_served_a_case():
    """Coverage is asserted, not hoped for: every family above launched for at least one case that ran to the end, and the
    variants a name cannot show (the weight gradient's row bands: RB < ch) are in the list that ran, by the launcher's formula."""
    every = {c["id"] for c in CONV + DENSE}
    if RAN != every:
        pytest.skip("depends on the case tests of this file having run (and passed) in the same process: %d of %d cases did"
                    % (len(RAN & every), len(every)))
    print("kernel name: cases served (of %d conv + %d dense)" % (len(CONV), len(DENSE)))
    for name, n in sorted(SERVED.items()):
        print("  %-34s %4d" % (name, n))
    print("seconds: tensors + C oracle %.1f, float64 reference %.1f, device calls + comparisons %.1f"
          % (TIMES["oracle"], TIMES["ref"], TIMES["gpu"] - TIMES["ref"]))
    missing = [f for f in FAMILIES if SERVED[f] == 0]
    assert not missing, missing
    banded = [c["id"] for c in CONV if c["stratum"] == "edge" and "k_bwd_wgrad" in c["note"] and FZ.wgrad_bands(c)[0] < FZ.wgrad_bands(c)[1]]
    assert len(banded) >= 2 and set(banded) <= RAN, banded
