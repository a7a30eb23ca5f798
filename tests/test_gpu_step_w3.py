"""GPU tests of the opt-in MFMA learning step of the (1,3)-kernel / 64-channel / (1,2)-pool layers of radio_ml_conv_ref.yaml:
dcll_conv_lif_step_w3 (k_lif_step_w3) and dcll_conv_lif_backward_w3[_open] (k_bwd_wgrad_w3), on the cases of
tests/step_w3_cases.py (proven on the CPU by tests/test_step_w3_cases.py), through ops.conv_lif_step(w3_path=True) /
ops.conv_lif_backward(w3_path=True) — the bindings the product uses — and through ConvNetwork.w3_step_path / train.py.

Forward, every case: three consecutive calls on one set of state buffers against the pinned-order C oracle — v equal bit for bit up
to the sign of a zero, pooled spikes, eps0, eps1 and arp bit for bit, pv within 1e-4, p / o within 1e-4 of a float64 matmul of the
oracle's pv; the launch log equals the restated prediction; a second run gives the same bits; spikes and state equal
dcll_conv_lif_step's; the other side of the 8- / 4-tile switch gives the same per-sample results.  Then the refusals.
Backward, every case: dW, db, d_outW, d_outb against fuzz_cases.conv_backward_ref in float64 (rtol 2e-3, atol 5e-5 max|ref|; the
fp32 restatement of the kernel's summation order stays inside it: tests/test_step_w3_cases.py); the open form +
ops.grad_reduce_adam and a second run give the closed form's bits; both scratch rules.
Network level: radio_ml_conv_ref.yaml on the (16,128) plane with w3_step_path against the default path."""
import collections
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import fuzz_cases as FZ
import step_w3_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")

CASES = S.cases()
REFUSALS = S.refusals()
BWD = S.bwd_cases()
PV_TOL = 1e-4           # the sigmoid's contract (include/dcll_hip.h)
LOGIT_TOL = 1e-4        # the header's readout contract
GRAD_RTOL, GRAD_ATOL = S.GRAD_RTOL, S.GRAD_ATOL
LAYER_KERNELS = ("k_lif_step", "k_trace", "k_conv_lif", "k_pool")

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


def forward(c, T, dev, B, w3_path, want_v=True):
    """The three steps of a case on the device at batch B (sample b = the case's sample b % c['B']) -> (per-step host copies,
    per-step kernel names).  misalign: every operand and every output of the layer call one float off a 16-byte boundary."""
    from snn_modulation_classification_amd import ops
    d = conv_desc(c)
    off = bool(c["misalign"]) and w3_path
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
        z = lambda *shape: cu(np.zeros(shape, np.float32), dev, True)
        out = dict(s=z(B, c["c_out"], ph, pw), pv=z(B, c["c_out"], ph, pw), v=z(B, c["c_out"], ch, cw))
    steps, logs = [], []
    h = lambda a: None if a is None else a.detach().cpu().numpy().copy()
    for t in range(len(T["x"])):          # (FZ.STEPS; tests/value_cases.py draws up to eight)
        with ops.kernel_trace() as tr:
            s, p, o, pv, v = ops.conv_lif_step(d, cu(T["x"][t][idx], dev, off), W, b, *tau, eps0, eps1, arp, out=out, want_v=want_v,
                                               w3_path=w3_path, **ro)
            torch.cuda.synchronize()
        logs.append(list(tr.names))
        steps.append(dict(s=h(s), p=h(p), o=h(o), pv=h(pv), v=h(v), eps0=h(eps0), eps1=h(eps1), arp=h(arp)))
    if w3_path:
        assert "scratch" not in out and "w_scratch" not in out          # no un-pooled round trip, no weight copy
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
    steps, logs = forward(c, T, dev, B, True, want_v=bool(c["want_v"]))
    assert (steps[0]["v"] is None) == (not c["want_v"])
    check_log(c, logs, B)
    check_against_oracle(c, T, osteps, steps, B)
    again, logs2 = forward(c, T, dev, B, True, want_v=bool(c["want_v"]))
    assert logs2 == logs
    assert_same(steps, again, ("v", "s", "pv", "p", "o", "eps0", "eps1", "arp"), "a second run", c["id"])
    # dcll_conv_lif_step on the same inputs: spikes and state bit for bit, v up to a zero's sign
    default, dlogs = forward(c, T, dev, B, False)
    assert not any(n.startswith("k_lif_step_w3") for names in dlogs for n in names)
    assert any(n.startswith("k_conv_lif") for n in dlogs[0]) and "k_pool" in dlogs[0]
    assert_same(steps, default, ("s", "eps0", "eps1", "arp"), "dcll_conv_lif_step", c["id"])
    for t in range(FZ.STEPS):
        if steps[t]["v"] is not None:
            assert equal_up_to_zero_sign(steps[t]["v"], default[t]["v"]), (c["id"], "v of dcll_conv_lif_step", t)
        np.testing.assert_allclose(steps[t]["pv"], default[t]["pv"], atol=PV_TOL, rtol=0)
    if c["also_B"]:                     # the other tile form: the same samples, per-sample results equal
        B2 = c["also_B"]
        assert S.tiles(c, B2) != S.tiles(c, B) and B2 <= B
        other, logs3 = forward(c, T, dev, B2, True)
        check_log(c, logs3, B2)
        assert_same(steps, other, ("v", "s", "pv", "eps0", "eps1", "arp"), "B = %d" % B2, c["id"], rows=B2)
        SERVED[S.form(c, B2)] += 1
    SERVED[S.form(c, B)] += 1
    RAN.add(c["id"])


def test_every_form_served_a_case():
    """a parity test is only worth its name if it ran the kernel it claims to cover (runs behind the cases above)"""
    assert RAN == {c["id"] for c in CASES}, sorted({c["id"] for c in CASES} - RAN)
    assert set(SERVED) == set(S.all_forms()), dict(SERVED)
    print("cases per form:", dict(SERVED))


@pytest.mark.parametrize("ref", REFUSALS, ids=[r["id"] for r in REFUSALS])
def test_refusals_come_before_any_launch(dev, ref):
    """each with its code, a phrase of dcll_last_error(), an empty launch log and untouched buffers"""
    from snn_modulation_classification_amd import _lib, ops
    r = ref
    lib = _lib.get()
    d = ops.make_conv_desc(r["c_in"], r["c_out"], (r["h"], r["w"]), (r["kh"], r["kw"]), (r["pad_h"], r["pad_w"]),
                           (r["pool_h"], r["pool_w"]), 0, bool(r["output_layer"]), r["tau_tensor"], 1.0 if r["refractory"] else 0.0,
                           FZ.ALPHARP, r["stride"], r["dilation"], r["groups"])
    ch, cw, ph, pw = FZ.conv_shape(r) or (1, 1, 1, 1)
    B, Bn = r["B"], max(r["B"], 1)
    SENT = 7.0
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(x=f(Bn, r["c_in"], r["h"], r["w"]), W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]),
             alpha=f(1), tau_m=f(1), alphas=f(1), tau_s=f(1), eps0=f(Bn, r["c_in"], r["h"], r["w"]), eps1=f(Bn, r["c_in"], r["h"], r["w"]),
             arp=f(Bn, r["c_out"], ch, cw), s=f(Bn, r["c_out"], ph, pw), pv=f(Bn, r["c_out"], ph, pw), v=f(Bn, r["c_out"], ch, cw))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_step_w3(ctypes.byref(d), p["x"], p["W"], p["b"], p["alpha"], p["tau_m"], p["alphas"], p["tau_s"],
                                       p["eps0"], p["eps1"], p["arp"], None, None, None, None, p["s"], None, None, p["pv"], p["v"],
                                       B, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode(), (r["id"], lib.dcll_last_error())
    assert tr.names == [], (r["id"], tr.names)
    for k, x in t.items():
        assert bool((x == SENT).all()), (r["id"], k, "was written")
    if r["code"] == "DCLL_ERR_UNSUPPORTED":
        assert not ops.step_w3_supported(d) and ops.step_w3_lds(d) == 0 and not ops.backward_w3_supported(d)


def test_w3_path_with_any_path_or_int8_weights_raises(dev):
    from snn_modulation_classification_amd import ops
    c = S.by_id("w3-64to64-1x32-B3")
    T, _ = S.run(c)
    d = conv_desc(c)
    q, scale, _ = FZ.quantize_int8(T["W"])
    args = lambda: (d, cu(T["x"][0], dev), cu(T["W"], dev), cu(T["b"], dev), *[cu(a, dev) for a in T["tau"]], cu(T["eps0"], dev),
                    cu(T["eps1"], dev), cu(T["arp"], dev))
    with ops.kernel_trace() as tr:
        with pytest.raises(ValueError):
            ops.conv_lif_step(*args(), q8=(torch.from_numpy(q).to(dev), torch.from_numpy(scale).to(dev)), w3_path=True)
        with pytest.raises(ValueError):
            ops.conv_lif_step(*args(), any_path=True, w3_path=True)
        v = torch.zeros(3, 64, 1, 32, device=dev)
        with pytest.raises(ValueError):
            ops.conv_lif_backward(d, cu(T["eps1"], dev), v, None, None, None, None, v, None, want_out=False, any_path=True, w3_path=True)
    assert tr.names == []


# ------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------
def assert_grad(got, ref, what, cid):
    ref = ref.numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    got = got.detach().cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    err = np.abs(got - ref)
    print("%s %s: max|err| %.3g, max|ref| %.3g, worst excess over rtol %.3g (atol %.3g)"
          % (cid, what, err.max(), scale, float((err - GRAD_RTOL * np.abs(ref)).max()), GRAD_ATOL * scale))
    np.testing.assert_allclose(got, ref, rtol=GRAD_RTOL, atol=GRAD_ATOL * scale + 1e-30, err_msg="%s %s" % (cid, what))


@pytest.mark.parametrize("case", BWD, ids=[c["id"] for c in BWD])
def test_backward_vs_float64_reference(dev, case):
    from snn_modulation_classification_amd import ops
    c, cid = case, case["id"]
    print(FZ.describe(c))
    T = S.bwd_draw(c)
    d = conv_desc(c)
    want_out = bool(c["output_layer"])
    assert ops.backward_w3_supported(d) and ops.backward_w3_lds(d) == S.bwd_lds_bytes(c)
    eps1, v = cu(T["eps1"], dev), cu(T["v"], dev)
    pv = torch.sigmoid(torch.nn.functional.max_pool2d(v, (1, 2)))
    g = {k: cu(T[k], dev) for k in ("g_p", "g_o", "g_pv", "g_v")}
    args = (g["g_p"], g["g_o"], g["g_pv"], g["g_v"], cu(T["i2o_W"], dev) if c["readout"] else None)
    keys = ("dW", "db") + (("d_outW", "d_outb") if want_out else ())
    run = lambda out, **kw: ops.conv_lif_backward(d, eps1, v, pv, *args, want_out=want_out, out=out, w3_path=True, **kw)
    with ops.kernel_trace() as tr:
        res = dict(zip(("dW", "db", "d_outW", "d_outb"), run({})))
        out2 = {}
        run(out2, open_reduce=True)
        out2["dW"].fill_(float("nan"))
        out2["db"].fill_(float("nan"))
        ops.grad_reduce_adam([dict(out2["parts"])], [])
        out4 = {}
        run(out4)
        torch.cuda.synchronize()
    names = tr.names
    print("kernels:", names)
    wg = [n for n in names if n.startswith("k_bwd_wgrad")]
    assert wg == [S.bwd_wgrad_name(c)] * 3 and names.count("k_bwd_dv") == 3, (cid, names)
    if c["c_in"] == 64:
        assert out2["parts"]["nchunk"] == S.bwd_chunks(c, c["B"]) and out2["parts"]["rowlen"] == 193
    for k in keys:
        assert bits_equal(out2[k], res[k]), (cid, "open form + dcll_grad_reduce_adam", k)
        assert bits_equal(out4[k], res[k]), (cid, "second run", k)
    route = FZ.first_max_route(c, FZ._f64(T["v"]))
    ref = FZ.conv_backward_ref(c, T, T["v"], T["eps1"], route)
    for k in keys:
        assert_grad(res[k], ref[k], k, cid)


def _raw_backward(lib, d, c, dev, scratch_floats, rng, open_form):
    """dcll_conv_lif_backward_w3[_open] straight through the C ABI with a scratch of the caller's size"""
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    B = c["B"]
    eps1 = cu(rng.uniform(0, 3, size=(B, c["c_in"], c["h"], c["w"])).astype(np.float32), dev)
    v = cu(rng.randn(B, 64, c["h"], c["w"]).astype(np.float32), dev)
    g_v = cu(rng.randn(B, 64, c["h"], c["w"]).astype(np.float32), dev)
    dW = torch.full((64, c["c_in"], 1, 3), -7.25, device=dev)
    db = torch.full((64,), -7.25, device=dev)
    scratch = torch.full((scratch_floats + 64,), -3.5, device=dev)
    part, nchunk = ctypes.c_void_p(), ctypes.c_int32(-1)
    if open_form:
        rc = lib.dcll_conv_lif_backward_w3_open(ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(g_v), None, None, None,
                                                ptr(scratch), scratch_floats, B, ctypes.byref(part), ctypes.byref(nchunk), stream_ptr())
    else:
        rc = lib.dcll_conv_lif_backward_w3(ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(g_v), None, ptr(dW),
                                           ptr(db), None, None, ptr(scratch), scratch_floats, B, stream_ptr())
    torch.cuda.synchronize()
    return rc, dW, db, scratch, (eps1, v, g_v), (part.value, nchunk.value)


@pytest.mark.parametrize("open_form", [False, True], ids=["closed", "open"])
def test_scratch_for_exactly_one_chunk(dev, open_form):
    """k = 1: B 64 h w + 64 x 193 floats — one workgroup sums every block; nothing behind the scratch is written; the open form
    leaves the one partial row (= dW | db of the closed form); one float less is DCLL_ERR_INVALID with an empty launch log."""
    from snn_modulation_classification_amd import _lib, ops
    c = dict(FZ.CONV_DEFAULT, **S.W3)
    c.update(c_in=64, h=4, w=64, B=5, target=4)
    d = conv_desc(c)
    need = c["B"] * 64 * 256 + 64 * 193
    with ops.kernel_trace() as tr:
        rc, dW, db, scratch, (eps1, v, g_v), (part, nchunk) = _raw_backward(_lib.get(), d, c, dev, need, np.random.RandomState(5), open_form)
    assert rc == 0, _lib.get().dcll_last_error()
    assert [n for n in tr.names if n.startswith("k_bwd_wgrad")] == ["k_bwd_wgrad_w3"] and ("k_bwd_reduce" in tr.names) == (not open_form), tr.names
    assert bool((scratch[need:] == -3.5).all())
    e, gv = eps1.cpu().double(), g_v.cpu().double()                       # (no g_p / g_pv: dv = g_v)
    cols = torch.nn.functional.unfold(e, (1, 3), 1, (0, 1), 1)
    refW = torch.einsum("bol,bkl->ok", gv.reshape(5, 64, -1), cols)
    if open_form:
        row = scratch[c["B"] * 64 * 256:need].reshape(64, 193)
        assert nchunk == 1 and part == scratch.data_ptr() + 4 * c["B"] * 64 * 256
        dW, db = row[:, :192], row[:, 192]
    assert_grad(dW.reshape(64, 192), refW, "dW", "k = 1")
    assert_grad(db, gv.sum(dim=(0, 2, 3)), "db", "k = 1")
    with ops.kernel_trace() as tr:
        rc, dW, db, scratch, _, _ = _raw_backward(_lib.get(), d, c, dev, need - 1, np.random.RandomState(5), open_form)
    assert rc == _lib.DCLL_ERR_INVALID and "scratch too small" in _lib.get().dcll_last_error().decode() and tr.names == []
    assert bool((dW == -7.25).all()) and bool((scratch == -3.5).all())


def test_backward_refusals_come_before_any_launch(dev):
    from snn_modulation_classification_amd import _lib, ops
    for r in REFUSALS:
        if r["code"] != "DCLL_ERR_UNSUPPORTED":
            continue
        d = conv_desc(dict(r, B=2))
        ch, cw, _, _ = FZ.conv_shape(r)
        eps1 = torch.rand(2, r["c_in"], r["h"], r["w"], device=dev)
        v = torch.randn(2, r["c_out"], ch, cw, device=dev)
        for open_form in (False, True):
            out = dict(dW=torch.full((r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), -7.25, device=dev),
                       db=torch.full((r["c_out"],), -7.25, device=dev))
            with ops.kernel_trace() as tr:
                with pytest.raises(_lib.DCLLUnsupported) as e:
                    ops.conv_lif_backward(d, eps1, v, None, None, None, None, torch.randn_like(v), None, want_out=False, out=out,
                                          open_reduce=open_form, w3_path=True)
            assert r["phrase"] in str(e.value) and tr.names == [], (r["id"], str(e.value), tr.names)
            torch.cuda.synchronize()
            assert bool((out["dW"] == -7.25).all()) and "parts" not in out


# ------------------------------------------------------------------------------------------------------------------------------
# network level: radio_ml_conv_ref.yaml on the (16,128) plane
# ------------------------------------------------------------------------------------------------------------------------------
HW = (16, 128)
N_LAYERS = 7
N_TILED = 5         # the default path tiles a plane from 8 columns up: widths 128 ... 8; the (16,4) and (16,2) layers run the plain k_conv_lif


def _args(**kw):
    a = dict(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    a.update(kw)
    return Namespace(**a)


def _spec(name):
    from snn_modulation_classification_amd.networks import load_network_spec
    return load_network_spec(os.path.join(PKG, "networks", name))


def _net(B, burnin=20, learn=False, graph=False, w3=False, spec="radio_ml_conv_ref.yaml", hw=HW, **akw):
    from snn_modulation_classification_amd.networks import ConvNetwork
    torch.manual_seed(1)
    np.random.seed(1)
    kw = dict(loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam, opt_param={"betas": [0.0, .95], "weight_decay": 10.0},
              learning_rates=[1e-6]) if learn else dict(loss=None, opt=None, opt_param={}, learning_rates=None)
    net = ConvNetwork(_args(**akw), (1,) + tuple(hw), B, _spec(spec), 24, act=torch.nn.Sigmoid(), burnin=burnin, **kw)
    net.graph_learn = graph
    net.reset(True)
    if learn:
        net.train()
    if w3:
        assert net.w3_step_supported() and all(s.w3_step_supported() for s in net.dcll_slices) and net.w3_step_path is False
        net.w3_step_path = True
        assert net.w3_step_path is True and all(s.dclllayer.i2h.w3_step_path and s.w3_learning_path for s in net.dcll_slices)
    return net


def _inputs(rng, B, n, dev, rate=.05):
    return [torch.from_numpy((rng.uniform(size=(B, 1) + HW) < rate).astype(np.float32)).to(dev) for _ in range(n)]


def _label(rng, B, dev):
    y = torch.zeros(B, 24)
    y[np.arange(B), rng.randint(0, 24, size=B)] = 1
    return y.to(dev)


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


def test_network_learning_steps_vs_default_path(dev):
    """Two identically seeded networks, A on the default dispatch and B with w3_step_path: before each of six learning steps B takes
    A's parameters, optimizer state and neuron state; then both learn.  Same spikes and readouts, gradients within the tolerance of
    tests/test_gpu_bwd_any.py's network-level comparison (another summation order).  A's log still names k_conv_lif_tiled<1,3> and
    k_bwd_wgrad; B's names neither."""
    from snn_modulation_classification_amd import ops
    B, burnin, steps = 3, 3, 6
    A, Bn = _net(B, burnin, learn=True), _net(B, burnin, learn=True, w3=True)
    rng = np.random.RandomState(11)
    y = _label(rng, B, dev)
    for t in range(burnin - 1 + steps):
        x = _inputs(rng, B, 1, dev)[0]
        _copy_everything(A, Bn)
        logs = []
        for net in (A, Bn):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(tr.names)
        learning = t >= burnin - 1
        # the default path is unchanged
        assert logs[0].count("k_conv_lif_tiled<1,3>") == N_TILED and logs[0].count("k_conv_lif") == N_LAYERS - N_TILED, logs[0]
        assert logs[0].count("k_trace") == N_LAYERS and logs[0].count("k_pool") == N_LAYERS, logs[0]
        assert not any(n.startswith(("k_lif_step_w3", "k_bwd_wgrad_w3")) for n in logs[0]), logs[0]
        assert logs[0].count("k_bwd_wgrad") == (N_LAYERS if learning else 0), logs[0]
        # the flag: one layer launch per slice, no generic conv / pool / trace kernel, the weight gradient of the 64 -> 64 layers
        assert sum(n.startswith("k_lif_step_w3") for n in logs[1]) == N_LAYERS, logs[1]
        assert not any(n.startswith(("k_conv_lif", "k_pool", "k_trace")) for n in logs[1]), logs[1]
        assert logs[1].count("k_bwd_wgrad_w3") == (N_LAYERS - 1 if learning else 0), logs[1]
        assert logs[1].count("k_bwd_wgrad") == (1 if learning else 0)                  # (the first layer, c_in 1: the generic kernel)
        for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):
            for key in ("s", "p"):
                if torch.is_tensor(sa._learn_bufs.get(key)):
                    assert torch.equal(sa._learn_bufs[key], sb._learn_bufs[key]), (t, key)
            if torch.is_tensor(sa._learn_bufs.get("pv")):
                assert float((sa._learn_bufs["pv"] - sb._learn_bufs["pv"]).abs().max()) <= PV_TOL
        if not learning:
            continue
        for i, (sa, sb) in enumerate(zip(A.dcll_slices, Bn.dcll_slices)):
            for (name, pa), (_, pb) in zip(sa.dclllayer.named_parameters(), sb.dclllayer.named_parameters()):
                assert (pa.grad is None) == (pb.grad is None), name
                if pa.grad is not None:
                    assert_grad(pb.grad, pa.grad.detach().cpu().double(), "slice %d %s.grad" % (i, name), "step %d" % t)


def test_per_step_test_loop_equals_the_default_path(dev):
    """`for t: net.test(x[t])` with the flag: clout, votes, accuracy and the final state of the default path; every layer of a step on
    k_lif_step_w3"""
    from snn_modulation_classification_amd import ops
    B, T = 3, 10
    rng = np.random.RandomState(2)
    xs = _inputs(rng, B, T, dev)
    a, b = _net(B), _net(B, w3=True)
    for t in range(T):
        with ops.kernel_trace() as ta:
            a.test(xs[t])
        with ops.kernel_trace() as tb:
            b.test(xs[t])
        if t == 0:
            assert ta.names.count("k_conv_lif_tiled<1,3>") == N_TILED and ta.names.count("k_conv_lif") == N_LAYERS - N_TILED, ta.names
            assert not any(n.startswith("k_lif_step_w3") for n in ta.names), ta.names
            assert [n for n in tb.names if n.startswith("k_lif_step_w3")] == ["k_lif_step_w3<1> (c_in 1, 4 tiles)"] + ["k_lif_step_w3<1> (4 tiles)"] * 6
            assert not any(n.startswith(("k_conv_lif", "k_pool", "k_trace")) for n in tb.names), tb.names
    y = torch.zeros(T, B, 24)
    y[:, np.arange(B), np.arange(B) % 24] = 1
    for sa, sb in zip(a.dcll_slices, b.dcll_slices):
        assert np.array_equal(np.array(sa.clout), np.array(sb.clout)) and np.array(sa.clout).shape == (T, B)
        assert np.array_equal(sa._predictions(y)[0], sb._predictions(y)[0])
        for u, v in zip(sa.dclllayer.i2h.state, sb.dclllayer.i2h.state):
            assert torch.equal(u, v)
    assert a.accuracy(y) == b.accuracy(y)
    assert float(a.dcll_slices[-1].dclllayer.i2h.state.eps1.abs().max()) > 0          # (spikes reached the last layer)


def _drive(net, xs, y, learn):
    for x in xs:
        if learn:
            net.learn(x, y)
        else:
            net.test(x)
    torch.cuda.synchronize()


@pytest.mark.parametrize("learn", [False, True], ids=["test", "learn"])
def test_graph_captured_steps_equal_eager_steps(dev, learn):
    """With w3_step_path the timestep replayed from its captured graph == the step launched eagerly, bit for bit, at B = 8; toggling
    the flag retakes the capture."""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 8, 16, 4
    rng = np.random.RandomState(4)
    xs = _inputs(rng, B, T, dev)
    y = _label(rng, B, dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(B, burnin, learn=learn, graph=graph, w3=True)
        _drive(net, xs, y, learn)
    a, b = nets[True], nets[False]
    graphs = lambda n: n._learn_graphs if learn else n._test_graphs
    key = ((B, 1) + HW, (B, 24)) if learn else (B, 1) + HW
    g = graphs(a)[key]
    assert g["n"] >= 6 and not graphs(b), (g["n"],)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)
    sig = a._graph_signature() if learn else a._test_signature()
    a.w3_step_path = b.w3_step_path = False
    assert (a._graph_signature() if learn else a._test_signature()) != sig
    with ops.kernel_trace() as tr:
        _drive(a, xs[:1], y, learn)
    assert graphs(a).get(key) is not g and not any(n.startswith("k_lif_step_w3") for n in tr.names) and any(n.startswith("k_conv_lif") for n in tr.names)


def test_learn_sequence_equals_per_step_learning(dev):
    """ConvNetwork.learn_sequence with w3_step_path (cells on the device) == the loop `for t: net.learn(x[t], y)` on the same planes
    with the flag: weights, Adam state and clout bit for bit"""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 4, 9, 5
    rng = np.random.RandomState(3)
    cells = rng.randint(0, HW[0] * HW[1], size=(T, B)).astype(np.int32)
    y = _label(rng, B, dev)
    a, b = _net(B, burnin, learn=True, w3=True), _net(B, burnin, learn=True, w3=True)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    n_learn = T - burnin + 1
    assert tr.names.count("k_bwd_wgrad_w3") == (N_LAYERS - 1) * n_learn and not any(n.startswith("k_conv_lif") for n in tr.names), tr.names
    x = np.zeros((T, B, HW[0] * HW[1]), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape(T, B, 1, *HW)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        st_a, st_b = sl_a.optimizer.state[sl_a.dclllayer.i2h.weight], sl_b.optimizer.state[sl_b.dclllayer.i2h.weight]
        assert float(st_a["step"]) == float(st_b["step"]) == n_learn and torch.equal(st_a["exp_avg_sq"], st_b["exp_avg_sq"])


def test_the_rank_sharded_step_runs_on_the_w3_path(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks — gradients in per-slice slabs, the CLOSED backward per slice
    (dcll_conv_lif_backward_w3 + k_bwd_reduce), then ops.adam_step — with the collective of a one-rank world (the identity) == the
    single-process step (open form + dcll_grad_reduce_adam) with the flag, bit for bit (modelled on
    tests/test_gpu_bwd_any.py::test_the_rank_sharded_step_runs_on_the_any_path)."""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 5, 3
    rng = np.random.RandomState(8)
    xs = _inputs(rng, B, T, dev)
    y = _label(rng, B, dev)
    a, b = _net(B, burnin, learn=True, w3=True), _net(B, burnin, learn=True, w3=True)
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
    assert tr.names.count("k_bwd_wgrad_w3") == (N_LAYERS - 1) * n_learn and tr.names.count("k_bwd_wgrad") == n_learn, tr.names
    assert sum(n.startswith("k_bwd_reduce") for n in tr.names) == N_LAYERS * n_learn and tr.count("k_grad_reduce_adam") == 0, tr.names
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))


def test_networks_that_are_not_served_refuse_the_attribute(dev):
    """radio_ml_conv.yaml, int8 weights, netscale 0.25 and the combination with the any paths: the setter raises DCLLUnsupported,
    the flag stays off; switching it off is always allowed"""
    from snn_modulation_classification_amd import _lib, quant
    net = _net(2, spec="radio_ml_conv.yaml", hw=(24, 24))
    assert not net.w3_step_supported() and net.step_any_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_step_path = True
    assert net.w3_step_path is False
    net.w3_step_path = False
    net = _net(2, netscale=.25)
    assert max(s.dclllayer.out_channels for s in net.dcll_slices) == 16 and not net.w3_step_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_step_path = True
    assert net.w3_step_path is False
    net = _net(2).to(dev)
    assert net.w3_step_supported()
    quant.apply_int8_weights(net)
    assert all(s.dclllayer.i2h.int8_weights() is not None for s in net.dcll_slices) and not net.w3_step_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_step_path = True
    assert net.w3_step_path is False and not any(s.w3_learning_path or s.dclllayer.i2h.w3_step_path for s in net.dcll_slices)
    # mutually exclusive with the any paths, in either order
    net = _net(2, w3=True)
    for attr in ("any_step_path", "any_learning_path"):
        with pytest.raises(_lib.DCLLUnsupported):
            setattr(net, attr, True)
        assert getattr(net, attr) is False
    net = _net(2)
    for s in net.dcll_slices:
        s.any_learning_path = True              # (the network's setter refuses it here; set on the slices, as a caller could)
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.w3_step_path = True
    assert "cannot be combined" in str(e.value) and net.w3_step_path is False


class _trace:
    """ops.kernel_trace, imported late (the package loads the library on import of ops)"""

    def __enter__(self):
        from snn_modulation_classification_amd import ops
        self._tr = ops.kernel_trace()
        return self._tr.__enter__()

    def __exit__(self, *exc):
        return self._tr.__exit__(*exc)


def test_entry_point_train_w3_step_path(tmp_path, capsys):
    """train.py on radio_ml_conv_ref.yaml (synthetic windows, the (16,128) plane) with --w3_step_path prints and stores the metrics of
    the same command without the flag and runs its per-step layer calls and weight gradients on the new kernels; on
    radio_ml_conv.yaml the flag is ignored with a notice"""
    import train
    common = ['--I_resolution', '128', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '8',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7',
              '--network_spec', os.path.join(PKG, 'networks', 'radio_ml_conv_ref.yaml')]
    runs = {}
    for name, flags in (("default", []), ("w3", ['--w3_step_path'])):
        with _trace() as tr:
            out = train.main(common + ['--output', str(tmp_path / name)] + flags)
        text = capsys.readouterr().out
        runs[name] = (np.load(os.path.join(out, 'acc_test.npy')), list(tr.names), text)
        assert "ignored" not in text
    a, names, _ = runs["default"]
    assert np.isfinite(a).all() and not any(n.startswith(("k_lif_step_w3", "k_bwd_wgrad_w3")) for n in names)
    b, names, _ = runs["w3"]
    assert np.array_equal(a, b), (a, b)
    assert any(n.startswith("k_lif_step_w3") for n in names) and "k_bwd_wgrad_w3" in names
    assert not any(n.startswith(("k_conv_lif", "k_pool")) for n in names)
    train.main(['--I_resolution', '24', '--Q_resolution', '24', '--arp', '1.0', '--burnin', '4', '--batch_size', '8', '--batch_size_test', '8',
                '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '6', '--n_iters_test', '6', '--n_steps', '1', '--n_test_interval', '1',
                '--learning_rates', '1e-7', '--output', str(tmp_path / 'radio'), '--w3_step_path'])
    assert "--w3_step_path ignored" in capsys.readouterr().out
