"""GPU tests of dcll_conv_lif_step_slab (k_lif_step_slab, the opt-in MFMA per-step forward of plain conv layers of any number of
output channels, in bands of output rows x slabs of 64 output channels; a layer dcll_conv_lif_step_wide serves is forwarded to it) on
the cases of tests/step_slab_cases.py (proven on the CPU by tests/test_step_slab_cases.py), through
snn_modulation_classification_amd.ops.conv_lif_step(slab_path=True) — the binding the product uses.

Every case, three consecutive calls on one set of state buffers, against the pinned-order C oracle: v equal bit for bit up to the
sign of a zero, pooled spikes, eps0, eps1 and arp bit for bit, pv finite, in [0, 1] and within 1e-4, p / o within 1e-4 of a float64
matmul of the oracle's pv; outputs sit in front of sentinel tails; the launch log equals the restated prediction; a second run gives
the same bits; spikes and state equal dcll_conv_lif_step's bit for bit; explicit bands = 1, 2, ph give identical bits wherever each
fits; forwarded cases equal dcll_conv_lif_step_wide bit for bit with an identical log; the other side of a step of the small-batch
rule gives the same per-sample results.  A permutation of the output channels across the 64-row boundary permutes the results.
Then the refusals, and the network level: the per-step test loop, learning steps, graph capture, learn_sequence, the rank-sharded
step, train.py and test_radio_ml.py with slab_step_path against the default path."""
import collections
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import fuzz_cases as FZ
import step_slab_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")

CASES = S.cases()
REFUSALS = S.refusals()
PV_TOL = 1e-4           # the sigmoid's contract (include/dcll_hip.h)
LOGIT_TOL = 1e-4        # the header's readout contract
LAYER_KERNELS = ("k_lif_step", "k_trace", "k_conv_lif", "k_pool", "k_seq_any_wprep", "k_step_wide_wprep", "k_step_slab_wprep")
SENT = 7.0              # sentinel behind every output of the layer call
TAIL = 64

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


def with_tail(shape, dev, off):
    """an output buffer of `shape` with TAIL sentinel floats behind it (off: its address is 4 mod 16) -> (view, tail)"""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL + 1,), SENT, device=dev)
    o = 1 if off else 0
    if not off and buf.data_ptr() % 16:
        raise AssertionError("allocator alignment")
    return buf[o:o + n].view(shape), buf[o + n:o + n + TAIL]


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


def forward(c, T, dev, B, path, want_v=True, bands=None):
    """The three steps of a case on the device at batch B (sample b = the case's sample b % c['B']) -> (per-step host copies,
    per-step kernel names).  path: "slab" (bands: the call's band count, None = the case's), "wide" or "default".  On the slab path
    the outputs of the layer call and w_scratch sit in front of sentinel tails (checked after every step); misalign: every operand
    and output one float off a 16-byte boundary."""
    from snn_modulation_classification_amd import ops
    d = conv_desc(c)
    slab = path == "slab"
    bands = c["bands"] if bands is None else bands
    off = bool(c["misalign"]) and slab
    idx = np.arange(B) % c["B"]
    ch, cw, ph, pw = FZ.conv_shape(c)
    W, b = cu(T["W"], dev, off), cu(T["b"], dev, off)
    tau = [cu(t, dev, off) for t in T["tau"]]
    eps0, eps1 = cu(T["eps0"][idx], dev, off), cu(T["eps1"][idx], dev, off)
    arp = cu(T["arp"][idx], dev, off) if c["refractory"] else None
    ro = dict(i2o_W=cu(T["i2o_W"], dev), i2o_b=cu(T["i2o_b"], dev)) if c["readout"] else {}
    if c["output_layer"]:
        ro.update(out_W=cu(T["out_W"], dev), out_b=cu(T["out_b"], dev))
    out, tails = {}, {}
    if slab:
        shapes = dict(s=(B, c["c_out"], ph, pw), pv=(B, c["c_out"], ph, pw), w_scratch=(S.scratch_floats(c),))
        if want_v:
            shapes["v"] = (B, c["c_out"], ch, cw)
        for k, shp in shapes.items():
            out[k], tails[k] = with_tail(shp, dev, off)
    kw = dict(slab_path=True, bands=bands) if slab else dict(wide_path=path == "wide")
    steps, logs = [], []
    h = lambda a: None if a is None else a.detach().cpu().numpy().copy()
    for t in range(len(T["x"])):
        with ops.kernel_trace() as tr:
            s, p, o, pv, v = ops.conv_lif_step(d, cu(T["x"][t][idx], dev, off), W, b, *tau, eps0, eps1, arp, out=out, want_v=want_v,
                                               **kw, **ro)
            torch.cuda.synchronize()
        logs.append(list(tr.names))
        steps.append(dict(s=h(s), p=h(p), o=h(o), pv=h(pv), v=h(v), eps0=h(eps0), eps1=h(eps1), arp=h(arp)))
        for k, tl in tails.items():
            assert bool((tl == SENT).all()), (c["id"], "step %d" % t, k, "written beyond its end")
    if slab:
        assert "scratch" not in out and out["w_scratch"].numel() == S.scratch_floats(c)
        assert s.data_ptr() == out["s"].data_ptr() and pv.data_ptr() == out["pv"].data_ptr()
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
        assert np.isfinite(g["pv"]).all() and g["pv"].min() >= 0.0 and g["pv"].max() <= 1.0, tag + ("pv range",)
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


def check_log(c, logs, B, bands=None):
    want = S.launch_log(c, B, bands)
    for t, names in enumerate(logs):
        assert names[:len(want)] == want, (c["id"], "step %d" % t, names, want)
        assert not any(n.startswith(LAYER_KERNELS) for n in names[len(want):]), (c["id"], names)       # behind them: readouts only
        assert bool(names[len(want):]) == bool(c["readout"]), (c["id"], names)


def assert_same(a, b, keys, what, cid, rows=None):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            if x[k] is not None and y[k] is not None:
                assert bits_equal(x[k] if rows is None else x[k][:rows], y[k]), (cid, what, "step %d" % t, k)


ALL = ("v", "s", "pv", "p", "o", "eps0", "eps1", "arp")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle(dev, case):
    c = case
    print(S.describe(c))
    T, osteps = S.run(c)
    B = c["B_run"]
    form = S.form(c, B)
    steps, logs = forward(c, T, dev, B, "slab", want_v=bool(c["want_v"]))
    assert (steps[0]["v"] is None) == (not c["want_v"])
    check_log(c, logs, B)
    check_against_oracle(c, T, osteps, steps, B)
    again, logs2 = forward(c, T, dev, B, "slab", want_v=bool(c["want_v"]))
    assert logs2 == logs
    assert_same(steps, again, ALL, "a second run", c["id"])
    # dcll_conv_lif_step serves every plain conv layer: spikes and state bit for bit, v up to a zero's sign
    default, dlogs = forward(c, T, dev, B, "default")
    assert not any(n.startswith(("k_lif_step_slab", "k_step_slab_wprep", "k_lif_step_wide", "k_lif_step_any")) for names in dlogs for n in names)
    assert_same(steps, default, ("s", "eps0", "eps1", "arp"), "dcll_conv_lif_step", c["id"])
    for t in range(FZ.STEPS):
        if steps[t]["v"] is not None:
            assert equal_up_to_zero_sign(steps[t]["v"], default[t]["v"]), (c["id"], "v of dcll_conv_lif_step", t)
        np.testing.assert_allclose(steps[t]["pv"], default[t]["pv"], atol=PV_TOL, rtol=0)
    if S.forwarded(c):                  # the call IS dcll_conv_lif_step_wide: every bit and the launch log
        wide, wlogs = forward(c, T, dev, B, "wide", want_v=bool(c["want_v"]))
        assert wlogs == logs and not any(n.startswith("k_lif_step_slab") for names in logs for n in names)
        assert_same(steps, wide, ALL, "dcll_conv_lif_step_wide", c["id"])
    # nothing depends on NB: explicit bands = 1, 2, ph wherever each fits (and a plan of the kernel's own, not a forwarded call)
    ph = FZ.conv_shape(c)[2]
    for nb in sorted({1, 2, ph}):
        if nb > ph or S.lds_max(c, nb) * 4 > S.LDS_MAX:
            continue
        assert S.plan(c, B, nb) == (nb, len(S.slabs(c)))
        other, ologs = forward(c, T, dev, B, "slab", bands=nb)
        check_log(c, ologs, B, nb)
        assert all(names[2].startswith("k_lif_step_slab") for names in ologs)
        assert_same(steps, other, ("v", "s", "pv", "eps0", "eps1", "arp"), "bands = %d" % nb, c["id"])
        SERVED[S.form(c, B, nb)] += 1
    if c["also_B"]:                     # the other side of a step of the small-batch rule: per-sample results equal
        B2 = c["also_B"]
        assert S.plan(c, B2) != S.plan(c, B)
        other, logs3 = forward(c, T, dev, B2, "slab")
        check_log(c, logs3, B2)
        assert_same(steps, other, ("v", "s", "pv", "eps0", "eps1", "arp"), "B = %d" % B2, c["id"], rows=B2)
    SERVED[form] += 1
    RAN.add(c["id"])


def test_every_form_served_a_case():
    """a parity test is only worth its name if it ran the kernel it claims to cover (runs behind the cases above)"""
    assert RAN == {c["id"] for c in CASES}, sorted({c["id"] for c in CASES} - RAN)
    assert set(S.all_forms()) <= set(SERVED), dict(SERVED)
    print("cases per form:", dict(SERVED))


@pytest.mark.parametrize("cid", ["slab-form-R1-plain", "slab-form-R1-pooling", "slab-co-cout129"])
def test_a_permutation_of_the_output_channels_permutes_the_results(dev, cid):
    """output channels moved across the 64-row boundary (W, b and arp permuted): s / pv / v / arp are the permuted results, bit for
    bit — a chain does not depend on the slab, M tile and row that computes it"""
    c = S.by_id(cid)
    T, _ = S.run(c)
    B = c["B"]
    perm = np.roll(np.arange(c["c_out"]), 37)[::-1].copy()
    assert any((p < 64) != (k < 64) for k, p in enumerate(perm)) and sorted(perm) == list(range(c["c_out"]))
    T2 = dict(T, W=T["W"][perm].copy(), b=T["b"][perm].copy(), arp=T["arp"][:, perm].copy())
    a, la = forward(c, T, dev, B, "slab")
    b, lb = forward(c, T2, dev, B, "slab")
    assert la == lb and la[0][2] == S.form(c, B)
    for t in range(FZ.STEPS):
        for k in ("s", "pv", "v", "arp"):
            assert bits_equal(a[t][k][:, perm], b[t][k]), (cid, t, k)
        assert bits_equal(a[t]["eps1"], b[t]["eps1"])
    assert a[-1]["s"][:, 64:].any() and not a[-1]["s"][:, 64:].all()


@pytest.mark.parametrize("ref", REFUSALS, ids=[r["id"] for r in REFUSALS])
def test_refusals_come_before_any_launch(dev, ref):
    """each with its code, a phrase of dcll_last_error(), an empty launch log and untouched buffers"""
    from snn_modulation_classification_amd import _lib, ops
    r = ref
    lib = _lib.get()
    d = ops.make_conv_desc(r["c_in"], r["c_out"], (r["h"], r["w"]), (r["kh"], r["kw"]), (r["pad_h"], r["pad_w"]),
                           (r["pool_h"], r["pool_w"]), 0, False, r["tau_tensor"], 1.0 if r["refractory"] else 0.0, FZ.ALPHARP,
                           r["stride"], r["dilation"], r["groups"])
    ch, cw, ph, pw = FZ.conv_shape(r) or (1, 1, 1, 1)
    B, Bn = r["B"], max(r["B"], 1)
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(x=f(Bn, r["c_in"], r["h"], r["w"]), W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]),
             alpha=f(1), tau_m=f(1), alphas=f(1), tau_s=f(1), eps0=f(Bn, r["c_in"], r["h"], r["w"]), eps1=f(Bn, r["c_in"], r["h"], r["w"]),
             arp=f(Bn, r["c_out"], ch, cw), s=f(Bn, r["c_out"], ph, pw), pv=f(Bn, r["c_out"], ph, pw), v=f(Bn, r["c_out"], ch, cw),
             w_scratch=f(max(128 * S.steps(r) * len(S.slabs(r)), 128)))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_step_slab(ctypes.byref(d), p["x"], p["W"], p["b"], p["alpha"], p["tau_m"], p["alphas"], p["tau_s"],
                                         p["eps0"], p["eps1"], p["arp"], None, None, None, None, p["s"], None, None, p["pv"], p["v"],
                                         p["w_scratch"], r["bands"], B, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode(), (r["id"], lib.dcll_last_error())
        assert "dcll_conv_lif_step_slab" in lib.dcll_last_error().decode()
    assert tr.names == [], (r["id"], tr.names)
    for k, x in t.items():
        assert bool((x == SENT).all()), (r["id"], k, "was written")
    if r["code"] == "DCLL_ERR_UNSUPPORTED":
        assert not ops.step_slab_supported(d, Bn, r["bands"]) and ops.step_slab_lds(d, Bn, r["bands"]) == 0


def test_the_older_entry_points_still_refuse_and_q8_raises(dev):
    from snn_modulation_classification_amd import _lib, ops
    c = S.by_id("slab-co-cout65")
    T, _ = S.run(c)
    d = conv_desc(c)
    args = lambda: (d, cu(T["x"][0], dev), cu(T["W"], dev), cu(T["b"], dev), *[cu(a, dev) for a in T["tau"]], cu(T["eps0"], dev),
                    cu(T["eps1"], dev), cu(T["arp"], dev))
    for kw, phrase in ((dict(wide_path=True), "c_out <= 64"), (dict(any_path=True), "c_out <= 32")):
        with ops.kernel_trace() as tr, pytest.raises(_lib.DCLLUnsupported) as e:
            ops.conv_lif_step(*args(), **kw)
        assert phrase in str(e.value) and tr.names == []
    q, scale, _ = FZ.quantize_int8(T["W"])
    for bad in (dict(q8=(torch.from_numpy(q).to(dev), torch.from_numpy(scale).to(dev))), dict(any_path=True), dict(w3_path=True),
                dict(wide_path=True)):
        with ops.kernel_trace() as tr, pytest.raises(ValueError):
            ops.conv_lif_step(*args(), slab_path=True, **bad)
        assert tr.names == []
    with pytest.raises(ValueError):
        ops.conv_lif_step(*args(), bands=2)


# ------------------------------------------------------------------------------------------------------------------------------
# network level: radio_ml_conv.yaml at netscale 3 and 4 on 16x16 (B = 3), at netscale 2 on 24x40
# ------------------------------------------------------------------------------------------------------------------------------
RADIO = "radio_ml_conv.yaml"
NETS = pytest.mark.parametrize("netscale, width", [(3.0, 96), (4.0, 128)], ids=["radio_ml_conv-ns3-16x16-B3", "radio_ml_conv-ns4-16x16-B3"])


def _spec(name):
    from snn_modulation_classification_amd.networks import load_network_spec
    return load_network_spec(os.path.join(PKG, "networks", name))


def _net(hw, B, netscale, burnin=20, learn=False, graph=False, slab_step=False, slab_learn=False, spec=RADIO, target=24, arp=1.0):
    from snn_modulation_classification_amd.networks import ConvNetwork
    torch.manual_seed(1)
    np.random.seed(1)
    args = Namespace(netscale=netscale, alpha=.92, alphas=.85, alpharp=.65, arp=arp, lc_ampl=.5, random_tau=True)
    kw = dict(loss=torch.nn.SmoothL1Loss, opt=torch.optim.Adam, opt_param={"betas": [0.0, .95], "weight_decay": 10.0},
              learning_rates=[1e-6]) if learn else dict(loss=None, opt=None, opt_param={}, learning_rates=None)
    net = ConvNetwork(args, (1,) + tuple(hw), B, _spec(spec), target, act=torch.nn.Sigmoid(), burnin=burnin, **kw)
    net.graph_learn = graph
    net.reset(True)
    if learn:
        net.train()
    if slab_learn:
        net.slab_learning_path = True
    if slab_step:
        assert net.step_slab_supported() and all(s.step_slab_supported() for s in net.dcll_slices) and net.slab_step_path is False
        assert not net.step_wide_supported()
        net.slab_step_path = True
        assert net.slab_step_path is True and all(s.dclllayer.i2h.slab_step_path for s in net.dcll_slices)
    return net


def _planes(rng, T, B, hw, dev):
    return [torch.from_numpy((rng.uniform(size=(B, 1) + tuple(hw)) < .15).astype(np.float32)).to(dev) for _ in range(T)]


def _target(rng, B, n, dev):
    y = torch.zeros(B, n)
    y[np.arange(B), rng.randint(0, n, size=B)] = 1
    return y.to(dev)


def _layer_forms(names):
    return [n for n in names if n.startswith(("k_lif_step_slab", "k_lif_step_wide", "k_lif_step_any"))]


def _assert_equal_nets(a, b, T=None):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter and (T is None or sl_a.iter == T)
        assert np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)


def _test_loop_equals_default(dev, hw, B, netscale, want, T=12):
    from snn_modulation_classification_amd import ops
    a, b = _net(hw, B, netscale), _net(hw, B, netscale, slab_step=True)
    rng = np.random.RandomState(0)
    x = _planes(rng, T, B, hw, dev)
    for t in range(T):
        a.test(x[t])
        with ops.kernel_trace() as tr:
            b.test(x[t])
        assert _layer_forms(tr.names) == want, tr.names
        assert not any(n.startswith(("k_conv_lif", "k_pool", "k_lif_step_c")) for n in tr.names), tr.names
    torch.cuda.synchronize()
    _assert_equal_nets(a, b, T)          # (the final state of every layer bit for bit, the recorded votes equal)
    for sa in a.dcll_slices:
        assert np.array(sa.clout).shape == (T, B)
    # every layer's spikes and logits, layer by layer through Conv2dDCLLlayer's own step call (from the state the loop left)
    a.reset()
    b.reset()
    spikes = 0.0
    with torch.no_grad():
        for t in range(T):
            ca, cb = x[t], x[t]
            for sla, slb in zip(a.dcll_slices, b.dcll_slices):
                La, Lb = sla.dclllayer, slb.dclllayer
                ra = La.i2h._step(ca, La.pooling, La.i2o, La.output_ if La.output_layer else None,
                                  stacked=La.stacked_readout() if La.output_layer else None)
                rb = Lb.i2h._step(cb, Lb.pooling, Lb.i2o, Lb.output_ if Lb.output_layer else None,
                                  stacked=Lb.stacked_readout() if Lb.output_layer else None)
                assert torch.equal(ra[0], rb[0]), ("spikes", t)
                assert float((ra[1] - rb[1]).abs().max()) <= LOGIT_TOL and float((ra[3] - rb[3]).abs().max()) <= PV_TOL
                ca, cb = ra[0], rb[0]
                spikes += float(ra[0].mean())
    assert 0 < spikes


@NETS
def test_network_test_loop_equals_the_default_path(dev, netscale, width):
    """`for t: net.test(x[t])` with slab_step_path against the default path: every layer's pooled spikes and the final state bit
    for bit, logits within the readout contract, recorded votes equal"""
    net = _net((16, 16), 3, netscale)
    assert [s.dclllayer.out_channels for s in net.dcll_slices] == [width] * 3
    _test_loop_equals_default(dev, (16, 16), 3, netscale, ["k_lif_step_slab<1>"] * 3)


def test_netscale_2_on_24x40_where_the_wide_step_is_refused(dev):
    """radio_ml_conv.yaml at netscale 2 on 24x40: the padded image of the 64 -> 64 layers (353 KB) is beyond a workgroup's LDS, so
    wide_step_path is refused; slab_step_path runs them in bands, the first layer on dcll_conv_lif_step_wide's kernels"""
    from snn_modulation_classification_amd import _lib
    net = _net((24, 40), 2, 2.0)
    assert not net.step_wide_supported() and net.step_slab_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.wide_step_path = True
    _test_loop_equals_default(dev, (24, 40), 2, 2.0, ["k_lif_step_wide<1> (split)", "k_lif_step_slab<1>", "k_lif_step_slab<1>"], T=6)


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


@NETS
def test_network_learning_steps_equal_the_default_forward(dev, netscale, width):
    """Two identically seeded networks with slab_learning_path, A on the default forward and B with slab_step_path: before each of
    six learning steps B takes A's parameters, optimizer state and neuron state; then both learn.  Same spikes and readouts, EQUAL
    gradients and parameters after Adam: the forward hands the backward the default path's bits (v up to a zero's sign, which
    sigmoid' does not see)."""
    from snn_modulation_classification_amd import ops
    burnin, steps, B, hw = 3, 6, 3, (16, 16)
    A = _net(hw, B, netscale, burnin=burnin, learn=True, slab_learn=True)
    Bn = _net(hw, B, netscale, burnin=burnin, learn=True, slab_learn=True, slab_step=True)
    rng = np.random.RandomState(11)
    y = _target(rng, B, 24, dev)
    for t in range(burnin - 1 + steps):
        x = _planes(rng, 1, B, hw, dev)[0]
        _copy_everything(A, Bn)
        logs = []
        for net in (A, Bn):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(tr.names)
        assert not _layer_forms(logs[0]) and "k_step_slab_wprep" not in logs[0]
        assert _layer_forms(logs[1]) == ["k_lif_step_slab<1>"] * 3 and logs[1].count("k_step_slab_wprep") == 3
        assert not any(n.startswith(("k_conv_lif", "k_pool", "k_lif_step_c")) for n in logs[1]), logs[1]
        assert any(n.startswith("k_bwd_wgrad_slab") for n in logs[1]) == (t >= burnin - 1) == any(n.startswith("k_bwd_wgrad_slab") for n in logs[0])
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
                if pa.grad is not None:
                    assert torch.equal(pa.grad, pb.grad), (netscale, t, i, name, float((pa.grad - pb.grad).abs().max()))
                assert torch.equal(pa, pb), (netscale, t, i, name, "after Adam")


def _drive(net, xs, y, learn):
    for x in xs:
        if learn:
            net.learn(x, y)
        else:
            net.test(x)
    torch.cuda.synchronize()


@pytest.mark.parametrize("learn", [False, True], ids=["test", "learn"])
def test_graph_captured_steps_equal_eager_steps(dev, learn):
    """With slab_step_path the timestep replayed from its captured graph == the step launched eagerly, bit for bit, at B = 8
    (radio_ml_conv.yaml at netscale 3 on 16x16); toggling the flag retakes the capture."""
    from snn_modulation_classification_amd import ops
    B, T, burnin, hw = 8, 16, 4, (16, 16)
    rng = np.random.RandomState(4)
    xs = _planes(rng, T, B, hw, dev)
    y = _target(rng, B, 24, dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(hw, B, 3.0, burnin=burnin, learn=learn, graph=graph, slab_step=True, slab_learn=learn)
        _drive(net, xs, y, learn)
    a, b = nets[True], nets[False]
    graphs = lambda n: n._learn_graphs if learn else n._test_graphs
    key = ((B, 1) + hw, (B, 24)) if learn else (B, 1) + hw
    g = graphs(a)[key]
    assert g["n"] >= 6 and not graphs(b), (g["n"],)
    _assert_equal_nets(a, b, T)
    sig = a._graph_signature() if learn else a._test_signature()
    a.slab_step_path = b.slab_step_path = False
    assert (a._graph_signature() if learn else a._test_signature()) != sig
    with ops.kernel_trace() as tr:
        _drive(a, xs[:1], y, learn)
    assert graphs(a).get(key) is not g and not _layer_forms(tr.names) and any(n.startswith("k_conv_lif") for n in tr.names)
    _drive(a, xs[1:8], y, learn)
    _drive(b, xs[:8], y, learn)
    g2 = graphs(a).get(key)
    assert g2 is not None and g2 is not g and g2["n"] >= 1
    _assert_equal_nets(a, b)


def test_learn_sequence_equals_per_step_learning(dev):
    """ConvNetwork.learn_sequence with slab_step_path + slab_learning_path (radio_ml_conv.yaml at netscale 3 on 16x16, cells on the
    device) == the loop `for t: net.learn(x[t], y)` with the flags: weights, Adam state and clout bit for bit"""
    from snn_modulation_classification_amd import ops
    B, T, burnin, R = 4, 9, 5, 16
    rng = np.random.RandomState(3)
    cells = rng.randint(0, R * R, size=(T, B)).astype(np.int32)
    y = _target(rng, B, 24, dev)
    mk = lambda: _net((R, R), B, 3.0, burnin=burnin, learn=True, slab_step=True, slab_learn=True)
    a, b = mk(), mk()
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    assert sum(n.startswith("k_lif_step_slab") for n in tr.names) == 3 * T and not any(n.startswith("k_conv_lif") for n in tr.names), tr.names
    x = np.zeros((T, B, R * R), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape(T, B, 1, R, R)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    _assert_equal_nets(a, b, T)
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        st_a, st_b = sl_a.optimizer.state[sl_a.dclllayer.i2h.weight], sl_b.optimizer.state[sl_b.dclllayer.i2h.weight]
        assert float(st_a["step"]) == float(st_b["step"]) == T - burnin + 1 and torch.equal(st_a["exp_avg_sq"], st_b["exp_avg_sq"])


def test_the_rank_sharded_step_runs_on_the_slab_step_path(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks (closed backward per slice, then ops.adam_step) with the collective of a
    one-rank world (the identity) == the single-process step, both with slab_step_path + slab_learning_path, bit for bit."""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 6, 3
    rng = np.random.RandomState(8)
    xs = _planes(rng, T, B, (16, 16), dev)
    y = _target(rng, B, 24, dev)
    mk = lambda: _net((16, 16), B, 3.0, burnin=burnin, learn=True, slab_step=True, slab_learn=True)
    a, b = mk(), mk()
    for t in range(T):
        a.learn(xs[t], y)
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    monkeypatch.setattr(parallel, "allreduce_slab_begin", lambda slab, local_n, global_n=None: None)
    with ops.kernel_trace() as tr:
        for t in range(T):
            b.learn(xs[t], y)
        torch.cuda.synchronize()
    monkeypatch.undo()
    assert sum(n.startswith("k_lif_step_slab") for n in tr.names) == 3 * T, tr.names
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))


def test_the_setter_refuses_what_is_not_served_and_other_step_paths(dev):
    from snn_modulation_classification_amd import _lib
    # netscale 2 on 128x128: not one pooled row of the 64 -> 64 layers fits
    net = _net((128, 128), 1, 2.0)
    assert not net.step_slab_supported()
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.slab_step_path = True
    assert "does not serve" in str(e.value) and net.slab_step_path is False
    net.slab_step_path = False                              # (switching it off is always allowed)
    # with any_step_path / wide_step_path, in either order (a netscale-1 network all three serve); the learning paths combine
    net = _net((28, 28), 2, 1.0, learn=True, spec="mnist_conv.yaml", target=10, arp=0.0)
    assert net.step_slab_supported() and net.step_wide_supported() and net.step_any_supported()
    for other in ("any_step_path", "wide_step_path"):
        setattr(net, other, True)
        with pytest.raises(_lib.DCLLUnsupported) as e:
            net.slab_step_path = True
        assert "combined" in str(e.value) and net.slab_step_path is False and getattr(net, other) is True
        setattr(net, other, False)
        net.slab_step_path = True
        with pytest.raises(_lib.DCLLUnsupported) as e:
            setattr(net, other, True)
        assert "combined" in str(e.value) and getattr(net, other) is False and net.slab_step_path is True
        net.slab_step_path = False
    net.slab_step_path = True
    for learn_path in ("any_learning_path", "wide_learning_path", "slab_learning_path"):
        setattr(net, learn_path, True)
        assert getattr(net, learn_path) is True and net.slab_step_path is True
        setattr(net, learn_path, False)
    # with w3_step_path, in either order (radio_ml_conv_ref.yaml on the (16,128) plane)
    net = _net((16, 128), 2, 1.0, learn=True, spec="radio_ml_conv_ref.yaml")
    assert net.w3_step_supported() and net.step_slab_supported()
    net.w3_step_path = True
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.slab_step_path = True
    assert "combined" in str(e.value) and net.slab_step_path is False and net.w3_step_path is True
    net.w3_step_path = False
    net.slab_step_path = True
    with pytest.raises(_lib.DCLLUnsupported) as e:
        net.w3_step_path = True
    assert "combined" in str(e.value) and net.w3_step_path is False and net.slab_step_path is True


class _trace:
    """ops.kernel_trace, imported late (the package loads the library on import of ops)"""

    def __enter__(self):
        from snn_modulation_classification_amd import ops
        self._tr = ops.kernel_trace()
        return self._tr.__enter__()

    def __exit__(self, *exc):
        return self._tr.__exit__(*exc)


def test_entry_point_train_slab_step_path(tmp_path, capsys):
    """train.py --netscale 3 --slab_learning_path --slab_step_path (RadioML on a 16x16 plane) prints and stores what the same command
    without --slab_step_path does, and runs every per-step layer call on k_lif_step_slab; on a 128x128 plane at netscale 2, and
    together with --wide_step_path on a narrow network, it prints the "ignored" notice"""
    import train
    common = ['--I_resolution', '16', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '12',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    runs = {}
    for name, flags in (("default", ['--netscale', '3', '--slab_learning_path']),
                        ("slab", ['--netscale', '3', '--slab_learning_path', '--slab_step_path'])):
        with _trace() as tr:
            out = train.main(common + ['--output', str(tmp_path / name)] + flags)
        text = capsys.readouterr().out
        runs[name] = (np.load(os.path.join(out, 'acc_test.npy')), list(tr.names), text, torch.load(os.path.join(out, 'parameters_0.pth')))
        assert "ignored" not in text
    a, names, _, pa = runs["default"]
    assert a.shape == (1, 1, 3) and np.isfinite(a).all() and not any(n.startswith("k_lif_step_slab") for n in names)
    b, names, _, pb = runs["slab"]
    assert np.array_equal(a, b), (a, b)
    assert set(pa) == set(pb) and all(torch.equal(pa[k], pb[k]) for k in pa)
    assert any(n.startswith("k_lif_step_slab") for n in names) and not any(n.startswith(("k_conv_lif", "k_pool")) for n in names)
    assert any(n.startswith("k_bwd_wgrad_slab") for n in names)
    train.main(common + ['--output', str(tmp_path / "both"), '--wide_step_path', '--slab_step_path'])
    assert "--slab_step_path ignored: another per-step path" in capsys.readouterr().out


def test_entry_point_test_radio_ml_on_the_slab_step_path(tmp_path, capsys, monkeypatch):
    """test_radio_ml.py --no_sequence_path --netscale 3 on a 16x16 plane with DCLL_SLAB_STEP_PATH=1 prints the per-SNR accuracies of
    the same command without it, and its per-step loop runs k_lif_step_slab; with DCLL_WIDE_STEP_PATH=1 beside it on a narrow
    network the switch is ignored with a notice"""
    import test_radio_ml as cli
    common = ["--I_resolution", "16", "--Q_resolution", "16", "--arp", "1.0", "--burnin", "4", "--batch_size_test", "8",
              "--n_test_samples", "8", "--synthetic", "8", "--n_iters_test", "12", "--min_snr", "10", "--max_snr", "10", "--no_sequence_path"]
    runs = {}
    for name in ("default", "slab"):
        if name == "slab":
            monkeypatch.setenv("DCLL_SLAB_STEP_PATH", "1")
        with _trace() as tr:
            cli.main(common + ["--netscale", "3", "--out_dir", str(tmp_path / name)])
        text = capsys.readouterr().out
        runs[name] = (np.load(tmp_path / name / "snr_evaluation_accs.npy"), [l for l in text.splitlines() if l.startswith("SNR")], list(tr.names))
        assert "ignored" not in text
    assert np.array_equal(runs["default"][0], runs["slab"][0]) and runs["default"][1] == runs["slab"][1] and runs["slab"][1]
    assert not _layer_forms(runs["default"][2]) and any(n.startswith("k_conv_lif") for n in runs["default"][2])
    assert any(n.startswith("k_lif_step_slab") for n in runs["slab"][2]) and not any(n.startswith(("k_conv_lif", "k_pool")) for n in runs["slab"][2])
    monkeypatch.setenv("DCLL_WIDE_STEP_PATH", "1")
    cli.main(common + ["--netscale", "1", "--out_dir", str(tmp_path / "both")])
    assert "DCLL_SLAB_STEP_PATH ignored: another per-step path" in capsys.readouterr().out
    monkeypatch.delenv("DCLL_WIDE_STEP_PATH")
    monkeypatch.delenv("DCLL_SLAB_STEP_PATH")
    net = _net((16, 16), 2, 3.0)
    assert net.slab_step_path is False                      # (unset: nothing changes)
