"""The opt-in banded MFMA weight gradient on the device: dcll_conv_lif_backward_bands[_open] (k_bwd_wgrad_band: a sample cut into bands
of conv-output rows, so the plane height no longer limits the layer) through ops.conv_lif_backward(band_path=True, bands=...), on the
cases of tests/bwd_band_cases.py (proven on the CPU by tests/test_bwd_band_cases.py), and through ConvNetwork.band_learning_path /
train.py --band_learning_path.

Per case: three forward steps with ops.conv_lif_step as tests/test_gpu_fuzz.py runs them, then the backward.
  - dW, db, d_outW, d_outb against fuzz_cases.conv_backward_ref in float64, from the ORACLE's v and eps1, within the project's
    tolerance for this comparison (rtol 2e-3, atol 5e-5 max|ref|; tests/test_bwd_band_cases.py shows that float32 in the kernel's
    summation order stays inside it on every case);
  - the open form + ops.grad_reduce_adam, the v = None form where it applies, and a second run: the closed form's bits;
  - where the default dispatch also serves the layer: dv, d_outW and d_outb are its bits, dW and db agree within the tolerance;
  - the launch log holds the k_bwd_wgrad_band variant bwd_band_cases.plan() predicts and no other weight-gradient kernel; a
    forwarded case (the slab call serves it) is dcll_conv_lif_backward_slab bit for bit, log for log;
  - every output sits in front of a sentinel tail that must stay untouched.
An integer-valued draw on every variant and band count must come out EXACT, through ops (the plan's chunks) and straight through
the C ABI with room for one and for two partial rows (one workgroup then runs band after band, sample after sample).  The last
case test asserts that every variant served a case."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import bwd_band_cases as BB
import fuzz_cases as FZ
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")

CASES = BB.cases()
REFUSALS = BB.refusals()
GRAD_RTOL, GRAD_ATOL = 2e-3, 5e-5       # tests/test_gpu_bwd_any.py, from tests/test_gpu_fuzz.py: rtol, atol = 5e-5 * max|ref|
SERVED = collections.Counter()          # k_bwd_wgrad_band variant -> cases it served
RAN = set()
TAIL, SENTINEL = 64, -7.25


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


def tailed_out(c, d, dev, want_out):
    """Output tensors as views of buffers with TAIL sentinel floats behind them -> (out dict, [(name, whole buffer, used floats)])."""
    from snn_modulation_classification_amd import ops
    _, _, ph, pw = ops.conv_out_shape(d)
    shapes = dict(dW=(c["c_out"], c["c_in"], c["kh"], c["kw"]), db=(c["c_out"],))
    if want_out:
        shapes.update(d_outW=(c["target"], c["c_out"] * ph * pw), d_outb=(c["target"],))
    out, bufs = {}, []
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        whole = torch.full((n + TAIL,), SENTINEL, device=dev)
        out[k] = whole[:n].view(shp)
        bufs.append((k, whole, n))
    return out, bufs


def tails_intact(bufs):
    return all(bool((whole[n:] == SENTINEL).all()) for _, whole, n in bufs)


def dv_plane(out, c):
    ch, cw, _, _ = FZ.conv_shape(c)
    return out["bwd_scratch"][:c["B"] * c["c_out"] * ch * cw].clone()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_band_path_vs_float64_reference(dev, case):
    from snn_modulation_classification_amd import ops
    c, cid, nb = case, case["id"], case["bands"]
    print(FZ.describe(c))
    T, osteps = FZ.conv_run(c)
    last, pv_full = conv_forward(c, T, osteps, dev)
    d, want_out = last["d"], bool(c["output_layer"])
    plan = BB.plan(c)
    assert ops.backward_bands_supported(d, nb) and ops.backward_bands_lds(d, nb) == BB.plan(c, nchunk=0)["lds"] >= plan["lds"]
    assert ops.backward_bands_plan(d, c["B"], nb) == {k: plan[k] for k in ("NB", "RB", "TPW", "PS", "NQ", "NS", "nsplit", "nchunk")}
    g = {k: cu(T[k], dev) for k in ("g_p", "g_o", "g_pv", "g_v")}
    args = (g["g_p"], g["g_o"], g["g_pv"], g["g_v"], last["i2o_W"])
    keys = ("dW", "db") + (("d_outW", "d_outb") if want_out else ())
    kw = dict(want_out=want_out, band_path=True, bands=nb)
    out1, bufs = tailed_out(c, d, dev, want_out)
    with ops.kernel_trace() as tr:
        res = dict(zip(("dW", "db", "d_outW", "d_outb"), ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, out=out1, **kw)))
        torch.cuda.synchronize()
    first_log = list(tr.names)
    assert tails_intact(bufs), (cid, "a write behind an output")
    with ops.kernel_trace() as tr:
        out2 = {}
        ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, out=out2, open_reduce=True, **kw)
        out2["dW"].fill_(float("nan"))
        out2["db"].fill_(float("nan"))
        assert out2["parts"]["nchunk"] == plan["nchunk"], (cid, out2["parts"]["nchunk"], plan["nchunk"])
        ops.grad_reduce_adam([dict(out2["parts"])], [])
        out3 = None
        if c["pool_h"] == 1 and c["pool_w"] == 1 and c["target"] <= 32:
            out3 = {}
            ops.conv_lif_backward(d, last["eps1"], None, last["pv"], *args, out=out3, **kw)
        out4 = {}
        ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, out=out4, **kw)
        torch.cuda.synchronize()
    names = first_log + tr.names
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
    if BB.default_serves(c):
        with ops.kernel_trace() as tr:
            outd = {}
            dflt = dict(zip(("dW", "db", "d_outW", "d_outb"),
                            ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out=outd)))
            torch.cuda.synchronize()
        assert not any(n.startswith(("k_bwd_wgrad_band", "k_bwd_wgrad_slab", "k_bwd_wgrad_wide", "k_bwd_wgrad_any")) for n in tr.names), tr.names
        assert bits_equal(dv_plane(outd, c), dv_plane(out4, c)), (cid, "dv == the default path's")
        for k in keys:
            if k in ("d_outW", "d_outb"):
                assert bits_equal(dflt[k], res[k]), (cid, "== the default path's", k)
            else:
                assert_grad(res[k], dflt[k].detach().cpu().double(), k + " (band path vs default path)", cid)
    if plan["forwarded"]:
        # dcll_conv_lif_backward_slab itself — bits and launch log
        with ops.kernel_trace() as tr:
            slab = dict(zip(("dW", "db", "d_outW", "d_outb"),
                            ops.conv_lif_backward(d, last["eps1"], last["v"], last["pv"], *args, want_out=want_out, out={}, slab_path=True)))
            torch.cuda.synchronize()
        assert tr.names == first_log and ops.backward_bands_lds(d, nb) == ops.backward_slab_lds(d), (cid, tr.names, first_log)
        assert not plan["name"].startswith("k_bwd_wgrad_band")
        for k in keys:
            assert bits_equal(slab[k], res[k]), (cid, "forwarded == dcll_conv_lif_backward_slab", k)
    else:
        SERVED[plan["name"]] += 1
    RAN.add(cid)


def test_every_variant_served_a_case():
    assert RAN == {c["id"] for c in CASES}, "run the whole module: this test sums up the cases above"
    print(dict(SERVED))
    assert set(SERVED) == set(BB.VARIANTS) and all(SERVED[v] >= 1 for v in BB.VARIANTS), dict(SERVED)


def _raw_backward(lib, d, c, dev, scratch_floats, eps1, v, g_v, open_form=False, bands=None):
    """dcll_conv_lif_backward_bands[_open] straight through the C ABI with a scratch of the caller's size and sentinels behind every
    buffer -> (rc, dW, db, scratch, nchunk or None)."""
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    bands = c["bands"] if bands is None else bands
    B = c["B"]
    nW = c["c_out"] * (c["c_in"] // c["groups"]) * c["kh"] * c["kw"]
    dW = torch.full((nW + TAIL,), SENTINEL, device=dev)
    db = torch.full((c["c_out"] + TAIL,), SENTINEL, device=dev)
    scratch = torch.full((scratch_floats + TAIL,), -3.5, device=dev)
    nchunk = None
    if open_form:
        part, nch = ctypes.c_void_p(), ctypes.c_int32()
        rc = lib.dcll_conv_lif_backward_bands_open(ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(g_v), None, None, None,
                                                   ptr(scratch), scratch_floats, B, bands, ctypes.byref(part), ctypes.byref(nch), stream_ptr())
        nchunk = nch.value
    else:
        rc = lib.dcll_conv_lif_backward_bands(ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(g_v), None, ptr(dW),
                                              ptr(db), None, None, ptr(scratch), scratch_floats, B, bands, stream_ptr())
    torch.cuda.synchronize()
    return rc, dW, db, scratch, nchunk


def exact_cases():
    """Every banded case of at most three samples (every forced band count, the rule's layers) and the first case of each variant."""
    out = [c for c in CASES if c["B"] <= 3 and not BB.plan(c)["forwarded"]]
    first = {}
    for c in CASES:
        if not BB.plan(c)["forwarded"]:
            first.setdefault(BB.plan(c)["name"], c)
    return out + [first[v] for v in BB.VARIANTS if first[v] not in out]


@pytest.mark.parametrize("case", exact_cases(), ids=[c["id"] for c in exact_cases()])
def test_integer_draw_is_exact(dev, case):
    """g_p = g_pv = NULL: k_bwd_dv writes g_v itself; g_v in {-2 .. 2}, eps1 in {0 .. 3}: every product and partial sum is an integer
    below 2^24, so dW and db equal the integer reference EXACTLY in any summation order — a product added twice, dropped, read from a
    stale row of the previous job, from a padding row that was not zeroed, or from the wrong band shows without a tolerance.  Through
    ops (the plan's chunks), then through the C ABI with room for ONE partial row (one workgroup per column split and slab runs every
    job in order) and for TWO (B = 3, N = 3: bands 0, 2, 1, 0, 2)."""
    from snn_modulation_classification_amd import _lib, ops
    c = case
    X = BB.exact_draw(c)
    d = conv_desc(c)
    plan = BB.plan(c)
    assert np.abs(X["dW"]).max() > 0
    eps1, v, g_v = cu(X["eps1"].astype(np.float32), dev), cu(X["v"], dev), cu(X["g_v"].astype(np.float32), dev)
    with ops.kernel_trace() as tr:
        dW, db, _, _ = ops.conv_lif_backward(d, eps1, v, None, None, None, None, g_v, None, want_out=False, out={}, band_path=True,
                                             bands=c["bands"])
        torch.cuda.synchronize()
    assert [n for n in tr.names if n.startswith("k_bwd_wgrad")] == [plan["name"]], tr.names

    def exact(dW, db, how):
        got_W, got_b = dW.cpu().numpy().astype(np.float64).reshape(X["dW"].shape), db.cpu().numpy().astype(np.float64)
        bad = np.argwhere(got_W != X["dW"])
        assert bad.size == 0, (c["id"], how, "dW differs at (co, ci, ky, kx)", bad[:8].tolist(), len(bad))
        assert np.array_equal(got_b, X["db"]), (c["id"], how, "db", np.argwhere(got_b != X["db"])[:8].tolist())
    exact(dW, db, "ops")
    ch, cw, _, _ = FZ.conv_shape(c)
    nconv, per = c["B"] * c["c_out"] * ch * cw, c["c_out"] * (c["c_in"] * c["kh"] * c["kw"] + 1)
    for k in (1, 2):
        if k > c["B"] * plan["NB"]:
            continue
        need = nconv + k * per
        with ops.kernel_trace() as tr:
            rc, rW, rb, scratch, _ = _raw_backward(_lib.get(), d, c, dev, need, eps1, v, g_v)
        assert rc == 0, _lib.get().dcll_last_error()
        assert [n for n in tr.names if n.startswith("k_bwd_wgrad")] == [BB.plan(c, nchunk=k)["name"]], (tr.names, k)
        nW = X["dW"].size
        assert bool((scratch[need:] == -3.5).all()) and bool((rW[nW:] == SENTINEL).all()) and bool((rb[c["c_out"]:] == SENTINEL).all())
        exact(rW[:nW], rb[:c["c_out"]], "room for %d partial rows" % k)
        rc, _, _, _, nchunk = _raw_backward(_lib.get(), d, c, dev, need, eps1, v, g_v, open_form=True)
        assert rc == 0 and nchunk == k, (rc, nchunk, k)


@pytest.mark.parametrize("open_form", [False, True], ids=["closed", "open"])
@pytest.mark.parametrize("ref", REFUSALS, ids=[r[0]["id"] for r in REFUSALS])
def test_refusals_come_before_any_launch(dev, ref, open_form):
    from snn_modulation_classification_amd import _lib, ops
    c, code, msg = ref
    print(FZ.describe(c))
    d = conv_desc(c)
    assert ops.backward_bands_supported(d, c["bands"]) == (code == "INVALID")
    ch, cw, _, _ = FZ.conv_shape(c)
    rng = np.random.RandomState(c["seed"] % (2 ** 31))
    B = c["B"]
    eps1 = cu(rng.uniform(0, 3, size=(B, c["c_in"], c["h"], c["w"])).astype(np.float32), dev)
    v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    g_v = cu(rng.randn(B, c["c_out"], ch, cw).astype(np.float32), dev)
    if code == "INVALID":
        need = B * c["c_out"] * ch * cw + c["c_out"] * (c["c_in"] * c["kh"] * c["kw"] + 1)
        with ops.kernel_trace() as tr:
            rc, dW, db, scratch, _ = _raw_backward(_lib.get(), d, c, dev, need - 1, eps1, v, g_v, open_form)
        err = _lib.get().dcll_last_error().decode()
        assert rc == _lib.DCLL_ERR_INVALID and msg in err and "dcll_conv_lif_backward_bands" in err and tr.names == []
        assert bool((dW == SENTINEL).all()) and bool((scratch == -3.5).all())
        return
    out = dict(dW=torch.full((c["c_out"], c["c_in"] // c["groups"], c["kh"], c["kw"]), SENTINEL, device=dev),
               db=torch.full((c["c_out"],), SENTINEL, device=dev))
    with ops.kernel_trace() as tr:
        with pytest.raises(_lib.DCLLUnsupported) as e:
            ops.conv_lif_backward(d, eps1, v, None, None, None, None, g_v, None, want_out=False, out=out, open_reduce=open_form,
                                  band_path=True, bands=c["bands"])
    assert msg in str(e.value) and msg in _lib.get().dcll_last_error().decode() and tr.names == [], (str(e.value), tr.names)
    assert ("dcll_conv_lif_backward_slab" if c["bands"] == 1 else "dcll_conv_lif_backward_bands") in str(e.value)
    torch.cuda.synchronize()
    assert bool((out["dW"] == SENTINEL).all()) and bool((out["db"] == SENTINEL).all()) and "parts" not in out


def test_the_older_paths_keep_their_refusals(dev):
    """band_path is opt-in and additive: on the 64 -> 64 layer of netscale 2 on 24x40 dcll_conv_lif_backward_slab, _wide and _any keep
    their refusals, and the default path keeps its 64-tap limit (a 9x9 kernel) — all before any launch."""
    from snn_modulation_classification_amd import _lib, ops
    c = BB.by_id("bwdband-radio-ns2-24x40-c64")
    d = conv_desc(c)
    assert not ops.backward_slab_supported(d) and not ops.backward_wide_supported(d) and ops.backward_bands_supported(d)
    ch, cw, _, _ = FZ.conv_shape(c)
    eps1 = torch.rand(c["B"], c["c_in"], c["h"], c["w"], device=dev)
    v = torch.randn(c["B"], c["c_out"], ch, cw, device=dev)
    for path, msg in ((dict(slab_path=True), "exceeds the 160 KiB of LDS"), (dict(wide_path=True), "exceeds the 160 KiB of LDS"),
                      (dict(any_path=True), "c_out <= 32")):
        for open_form in (False, True):
            with ops.kernel_trace() as tr:
                with pytest.raises(_lib.DCLLUnsupported) as e:
                    ops.conv_lif_backward(d, eps1, v, None, None, None, None, torch.randn_like(v), None, want_out=False, out={},
                                          open_reduce=open_form, **path)
            assert msg in str(e.value) and tr.names == [], (path, str(e.value), tr.names)
    c9 = BB.by_id("bwdband-k9x9")
    d9 = conv_desc(c9)
    ch, cw, _, _ = FZ.conv_shape(c9)
    eps1 = torch.rand(c9["B"], c9["c_in"], c9["h"], c9["w"], device=dev)
    v = torch.randn(c9["B"], c9["c_out"], ch, cw, device=dev)
    for open_form in (False, True):
        with ops.kernel_trace() as tr:
            with pytest.raises(_lib.DCLLUnsupported) as e:
                ops.conv_lif_backward(d9, eps1, v, None, None, None, None, torch.randn_like(v), None, want_out=False, out={},
                                      open_reduce=open_form)
        assert "kernels up to 64 taps" in str(e.value) and tr.names == []


# ------------------------------------------------------------------------------------------------------------------------------
# network level: radio_ml_conv.yaml at netscale 2 on 24x40 (1 -> 64, 64 -> 64, 64 -> 64: no MFMA weight gradient served it), B = 3
# ------------------------------------------------------------------------------------------------------------------------------
HW = (24, 40)


def _args(**kw):
    from argparse import Namespace
    a = dict(netscale=2.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    a.update(kw)
    return Namespace(**a)


def _net(convs, hw, B, target, burnin, arp, graph, netscale=2.0):
    from snn_modulation_classification_amd.networks import ConvNetwork
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(_args(arp=arp, netscale=netscale), (1,) + hw, B, convs, target, act=torch.nn.Sigmoid(), loss=torch.nn.SmoothL1Loss,
                      opt=torch.optim.Adam, opt_param={"betas": [0.0, .95], "weight_decay": 10.0}, learning_rates=[1e-6],
                      burnin=burnin)
    net.graph_learn = graph
    net.reset(True)
    net.train()
    return net


def _spec(name):
    from snn_modulation_classification_amd.networks import load_network_spec
    return load_network_spec(os.path.join(PKG, "networks", name))


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


def _radio(B, burnin, graph=False, flag=True):
    net = _net(_spec("radio_ml_conv.yaml"), HW, B, 24, burnin, 1.0, graph)
    assert [s.dclllayer.out_channels for s in net.dcll_slices] == [64, 64, 64]
    if flag is not False:
        net.band_learning_path = flag
    return net


def _labels(B, rng, dev):
    y = torch.zeros(B, 24)
    y[np.arange(B), rng.randint(0, 24, size=B)] = 1
    return y.to(dev)


def _planes(rng, n, B, dev):
    return [torch.from_numpy((rng.uniform(size=(B, 1) + HW) < .15).astype(np.float32)).to(dev) for _ in range(n)]


def test_network_learning_steps_band_path_vs_default_path(dev):
    """Two identically seeded netscale-2 networks on 24x40, A on the default dispatch and B with band_learning_path: before each of
    six learning steps B takes A's parameters, optimizer state and neuron state; then both learn.  Same forward bits (spikes, logits,
    votes), gradients within the weight-gradient tolerance, one k_bwd_wgrad_band per slice in B's log and none in A's."""
    from snn_modulation_classification_amd import _lib, ops
    B, burnin, steps = 3, 3, 6
    A, Bn = _radio(B, burnin, flag=False), _radio(B, burnin, flag=False)
    assert A.band_learning_path is False and Bn.backward_bands_supported() and all(s.backward_bands_supported() for s in Bn.dcll_slices)
    assert not Bn.backward_slab_supported()
    with pytest.raises(_lib.DCLLUnsupported):                  # (pinned: the slab path raises on this plane)
        Bn.slab_learning_path = True
    Bn.band_learning_path = True
    assert Bn.band_learning_path is True and all(s.band_learning_path is True for s in Bn.dcll_slices)
    assert not any(s.band_learning_path for s in A.dcll_slices)
    rng = np.random.RandomState(11)
    y = _labels(B, rng, dev)
    learned = 0
    for t, x in enumerate(_planes(rng, burnin - 1 + steps, B, dev)):
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
        assert sum(n.startswith("k_bwd_wgrad_band") for n in logs[1]) == 3 == sum(n.startswith("k_bwd_wgrad") for n in logs[1]), logs[1]
        assert not any(n.startswith("k_bwd_wgrad_band") for n in logs[0]) and sum(n.startswith("k_bwd_wgrad") for n in logs[0]) == 3
        assert logs[0].count("k_grad_reduce_adam") == logs[1].count("k_grad_reduce_adam") == 1
        for i, (sa, sb) in enumerate(zip(A.dcll_slices, Bn.dcll_slices)):
            for (name, pa), (_, pb) in zip(sa.dclllayer.named_parameters(), sb.dclllayer.named_parameters()):
                assert (pa.grad is None) == (pb.grad is None), name
                if pa.grad is not None:
                    assert_grad(pb.grad, pa.grad.detach().cpu().double(), "slice %d %s.grad" % (i, name), "netscale 2, 24x40, step %d" % t)
    assert learned == steps
    for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):          # the per-step votes of the whole run
        assert np.array_equal(np.asarray(sa.clout), np.asarray(sb.clout)) and len(sa.clout) == steps


def test_graph_captured_steps_equal_eager_steps_on_the_band_path(dev):
    """With band_learning_path the learning timestep replayed from its captured graph == the step launched eagerly, bit for bit, at
    B = 8 (ConvNetwork.graph_learn); the flag and its band count are part of the capture's signature."""
    B, T, burnin = 8, 14, 4
    rng = np.random.RandomState(4)
    xs = _planes(rng, T, B, dev)
    y = _labels(B, rng, dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _radio(B, burnin, graph)
        for t in range(T):
            net.learn(xs[t], y)
        torch.cuda.synchronize()
    a, b = nets[True], nets[False]
    g = a._learn_graphs[((B, 1) + HW, (B, 24))]
    assert g["n"] >= 4 and not b._learn_graphs, (g["n"],)
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
    sig_on = a._graph_signature()
    a.band_learning_path = 4
    sig_4 = a._graph_signature()
    a.band_learning_path = False
    assert len({sig_on, sig_4, a._graph_signature()}) == 3


def test_learn_sequence_equals_per_step_learning_on_the_band_path(dev):
    """ConvNetwork.learn_sequence with band_learning_path (cells on the device) == the loop `for t: net.learn(x[t], y)` on the same
    planes with the flag: weights, Adam state and clout bit for bit; the weight gradient ran on k_bwd_wgrad_band."""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 3, 7, 4
    rng = np.random.RandomState(3)
    cells = rng.randint(0, HW[0] * HW[1], size=(T, B)).astype(np.int32)
    y = _labels(B, rng, dev)
    a, b = _radio(B, burnin), _radio(B, burnin)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    n_learn = T - burnin + 1
    assert sum(n.startswith("k_bwd_wgrad_band") for n in tr.names) == 3 * n_learn == sum(n.startswith("k_bwd_wgrad") for n in tr.names), tr.names
    x = np.zeros((T, B, HW[0] * HW[1]), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape((T, B, 1) + HW)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        st_a, st_b = sl_a.optimizer.state[sl_a.dclllayer.i2h.weight], sl_b.optimizer.state[sl_b.dclllayer.i2h.weight]
        assert float(st_a["step"]) == float(st_b["step"]) == n_learn and torch.equal(st_a["exp_avg_sq"], st_b["exp_avg_sq"])


def test_the_rank_sharded_step_runs_on_the_band_path(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks — gradients in per-slice flat buffers, the CLOSED backward per slice
    (dcll_conv_lif_backward_bands + k_bwd_reduce), then ops.adam_step — with the collective of a one-rank world (the identity)
    == the single-process step (open form + dcll_grad_reduce_adam) with the flag, bit for bit."""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 6, 3
    rng = np.random.RandomState(8)
    xs = _planes(rng, T, B, dev)
    y = _labels(B, rng, dev)
    a, b = _radio(B, burnin), _radio(B, burnin)
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
    assert sum(n.startswith("k_bwd_wgrad_band") for n in tr.names) == 3 * n_learn == sum(n.startswith("k_bwd_wgrad") for n in tr.names), tr.names
    assert sum(n.startswith("k_bwd_reduce") for n in tr.names) == 3 * n_learn and tr.count("k_grad_reduce_adam") == 0, tr.names
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))


def test_the_setter_refuses_what_is_not_served_and_other_learning_paths(dev):
    from snn_modulation_classification_amd import _lib
    # a 17x17 kernel: not served
    net = _net([dict(out_channels=40, kernel_size=17, padding=8, pooling=1)], (8, 8), 2, 10, 2, 1.0, False)
    assert not net.backward_bands_supported()
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.band_learning_path = True
    assert "does not serve" in str(e.value) and net.band_learning_path is False
    net.band_learning_path = False                          # (switching it off is always allowed)
    # a forced band count beyond a slice's rows, and a negative one
    net = _radio(2, 2, flag=False)
    for bad in (25, -1):
        with pytest.raises(_lib.DCLLUnsupported):
            net.band_learning_path = bad
        assert net.band_learning_path is False
    net.band_learning_path = 24
    assert net.band_learning_path == 24 and all(s.band_learning_path == 24 and s._band_count() == 24 for s in net.dcll_slices)
    net.band_learning_path = 0                              # (0 bands: the rule)
    assert net.band_learning_path is True and all(s._band_count() == 0 for s in net.dcll_slices)
    # with the forward paths: combines
    net.slab_step_path = True
    assert net.slab_step_path is True and net.band_learning_path is True
    net.slab_step_path = False
    # with any_learning_path / wide_learning_path / slab_learning_path, in either order (a netscale-1 network all serve)
    for other in ("any_learning_path", "wide_learning_path", "slab_learning_path"):
        net = _net(_spec("mnist_conv.yaml"), (28, 28), 2, 10, 2, 0.0, False, netscale=1.0)
        assert net.backward_bands_supported() and net.backward_slab_supported() and net.backward_any_supported()
        setattr(net, other, True)
        with pytest.raises(_lib.DCLLUnsupported) as e:
            net.band_learning_path = True
        assert "combined" in str(e.value) and net.band_learning_path is False and getattr(net, other) is True
        setattr(net, other, False)
        net.band_learning_path = True
        with pytest.raises(_lib.DCLLUnsupported) as e:
            setattr(net, other, True)
        assert "combined" in str(e.value) and getattr(net, other) is False and net.band_learning_path is True
    # with w3_step_path, in either order (radio_ml_conv_ref.yaml on the (16,128) plane)
    net = _net(_spec("radio_ml_conv_ref.yaml"), (16, 128), 2, 24, 2, 1.0, False, netscale=1.0)
    assert net.w3_step_supported()
    net.w3_step_path = True
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.band_learning_path = True
    assert "combined" in str(e.value) and net.band_learning_path is False and net.w3_step_path is True
    net.w3_step_path = False
    net.band_learning_path = True
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.w3_step_path = True
    assert "combined" in str(e.value) and net.w3_step_path is False


def test_a_9x9_spec_on_24x40_learns(dev):
    """81 taps on 24x40 at netscale 2: the default path refuses the taps, the slab path the plane; with band_learning_path the network
    learns — finite gradients that move the weights, every weight gradient on k_bwd_wgrad_band."""
    from snn_modulation_classification_amd import _lib, ops
    B, burnin = 3, 2
    spec = [dict(out_channels=32, kernel_size=9, padding=4, pooling=1), dict(out_channels=32, kernel_size=9, padding=4, pooling=2)]
    net = _net(spec, HW, B, 24, burnin, 1.0, False)
    assert not net.backward_slab_supported() and net.backward_bands_supported()
    rng = np.random.RandomState(5)
    xs, y = _planes(rng, 4, B, dev), _labels(B, rng, dev)
    net.learn(xs[0], y)
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.learn(xs[1], y)
    assert "kernels up to 64 taps" in str(e.value)
    net = _net(spec, HW, B, 24, burnin, 1.0, False)
    net.band_learning_path = True
    w0 = [s.dclllayer.i2h.weight.detach().clone() for s in net.dcll_slices]
    with ops.kernel_trace() as tr:
        for x in xs:
            net.learn(x, y)
        torch.cuda.synchronize()
    wg = [n for n in tr.names if n.startswith("k_bwd_wgrad")]
    assert len(wg) == 2 * 3 and any(n.startswith("k_bwd_wgrad_band") for n in wg), wg
    assert all(n.startswith(("k_bwd_wgrad_band", "k_bwd_wgrad_wide", "k_bwd_wgrad_any")) for n in wg), wg
    for s, w in zip(net.dcll_slices, w0):
        g = s.dclllayer.i2h.weight.grad
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and not torch.equal(s.dclllayer.i2h.weight, w)


def test_entry_point_train_with_band_learning_path(tmp_path, capsys, monkeypatch):
    """train.py --netscale 2 --band_learning_path on a synthetic RadioML set on the 24x40 plane (no other MFMA weight gradient serves
    it): exits normally with finite accuracies, every backward call of its learning steps takes the band path and its weight
    gradients run on k_bwd_wgrad_band; with a band count the count reaches the calls; together with --slab_learning_path on a network
    that path serves the flag prints the "ignored" notice and the slab path stays in effect."""
    import train
    from snn_modulation_classification_amd import ops
    calls = []
    real = ops.conv_lif_backward

    def counted(*a, **kw):
        calls.append((bool(kw.get("band_path", False)) or kw.get("path") == "band", int(kw.get("bands", 0)),
                      bool(kw.get("slab_path", False)) or kw.get("path") == "slab"))          # (the old keywords, or path=)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "conv_lif_backward", counted)
    common = ['--arp', '1.0', '--burnin', '4', '--batch_size', '4', '--batch_size_test', '4', '--n_test_samples', '4', '--synthetic', '8',
              '--n_iters', '8', '--n_iters_test', '8', '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    plane = ['--I_resolution', str(HW[0]), '--Q_resolution', str(HW[1]), '--netscale', '2']
    for name, flag, bands in (("rule", ['--band_learning_path'], 0), ("forced", ['--band_learning_path', '6'], 6)):
        del calls[:]
        with ops.kernel_trace() as tr:
            out_dir = train.main(common + plane + ['--output', str(tmp_path / name)] + flag)
        text = capsys.readouterr().out
        acc = np.load(os.path.join(out_dir, 'acc_test.npy'))
        assert np.isfinite(acc).all() and "ignored" not in text, text
        assert len(calls) > 0 and all(c == (True, bands, False) for c in calls), calls[:4]
        wg = [n for n in tr.names if n.startswith("k_bwd_wgrad")]
        assert len(wg) == len(calls) and all(n.startswith("k_bwd_wgrad_band") for n in wg), wg[:6]
        for k, v in torch.load(os.path.join(out_dir, 'parameters_0.pth')).items():
            assert bool(torch.isfinite(v).all()), k
    del calls[:]
    train.main(common + ['--I_resolution', '16', '--Q_resolution', '16', '--netscale', '3', '--output', str(tmp_path / "both"),
                         '--slab_learning_path', '--band_learning_path', '2'])
    text = capsys.readouterr().out
    assert "--band_learning_path ignored: another learning path" in text
    assert len(calls) > 0 and all(c == (False, 0, True) for c in calls), calls[:4]
