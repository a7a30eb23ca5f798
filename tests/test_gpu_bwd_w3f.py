"""GPU tests of the opt-in streaming weight gradient of the first (1,3) layer: dcll_conv_lif_backward_w3f[_open]
(k_bwd_wgrad_w3f), on the cases of tests/bwd_w3f_cases.py (proven on the CPU by tests/test_bwd_w3f_cases.py), through
ops.conv_lif_backward(w3_path=True, w3_first=True) — the binding the product uses — and the C ABI where the case sets its own
scratch size, and through ConvNetwork.w3_first_wgrad / train.py.

Every case: dW, db, d_outW, d_outb against fuzz_cases.conv_backward_ref in float64 (rtol 2e-3, atol 5e-5 max|ref|, the scale taken
per tensor; the fp32 restatement of the kernel's summation order stays inside it: tests/test_bwd_w3f_cases.py); a second run, the
open form + ops.grad_reduce_adam and the other alignment give the same bits; the dv plane, d_outW and d_outb are
dcll_conv_lif_backward_w3's bits; the launch log is the predicted one.  An integer-valued draw must come out exact.  Then the
refusals, and the network level: radio_ml_conv_ref.yaml on the (16,128) plane with w3_step_path + w3_first_wgrad against
w3_step_path alone."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bwd_w3f_cases as C
import fuzz_cases as FZ
import step_w3_cases as S
import test_gpu_step_w3 as W        # its helpers (network builders, comparisons); its tests are not re-exported here
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
CASES = C.cases()
HW, N_LAYERS = W.HW, W.N_LAYERS
cu, bits_equal, conv_desc, assert_grad = W.cu, W.bits_equal, W.conv_desc, W.assert_grad
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _scratch(n, off, dev):
    """(buffer, view of n floats at 0 or 4 (mod 16) bytes): the view is the call's scratch, the GUARD floats behind it stay -3.5"""
    buf = torch.full((n + GUARD + 4,), -3.5, device=dev)
    view = buf[off:off + n]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    return buf, view


def _tensors(c, T, dev):
    v = cu(T["v"], dev)
    X = dict(v=v, pv=torch.sigmoid(torch.nn.functional.max_pool2d(v, (1, 2))), i2o_W=cu(T["i2o_W"], dev) if T["g_p"] is not None else None,
             eps1={0: cu(T["eps1"], dev), 1: cu(T["eps1"], dev, True)})
    X.update({k: cu(T[k], dev) for k in ("g_p", "g_o", "g_pv", "g_v")})
    return X


def backward(c, X, dev, room, misalign, open_form=False, entry="w3f", via_ops=False):
    """One backward call -> dict(dW, db, d_outW, d_outb, dv (the plane left in scratch), names, nchunk).  via_ops: through
    ops.conv_lif_backward with its own scratch size (the view handed in must be the one it keeps); else through the C ABI with room
    for `room` partial rows.  misalign: eps1 and scratch 4 bytes off a 16-byte boundary.  open_form: + ops.grad_reduce_adam."""
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    d = conv_desc(c)
    B, nconv = c["B"], c["B"] * 64 * c["h"] * c["w"]
    n = nconv + room * 64 * (3 * c["c_in"] + 1)
    buf, scratch = _scratch(n, int(misalign), dev)
    eps1 = X["eps1"][int(misalign)]
    want_out = X["g_o"] is not None
    K = 64 * c["h"] * (c["w"] // 2)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    dW, db = nan(64, c["c_in"], 1, 3), nan(64)
    d_outW, d_outb = (nan(c["target"], K), nan(c["target"])) if want_out else (None, None)
    nchunk = None
    with ops.kernel_trace() as tr:
        if via_ops:
            out = dict(dW=dW, db=db, bwd_scratch=scratch)
            if want_out:
                out.update(d_outW=d_outW, d_outb=d_outb)
            ops.conv_lif_backward(d, eps1, X["v"], X["pv"], X["g_p"], X["g_o"], X["g_pv"], X["g_v"], X["i2o_W"], want_out=want_out,
                                  out=out, open_reduce=open_form, w3_path=True, w3_first=entry == "w3f")
            assert out["bwd_scratch"] is scratch, "ops.conv_lif_backward's scratch size is not the restated one"
            if open_form:
                nchunk = out["parts"]["nchunk"]
                assert out["parts"]["rowlen"] == 3 * c["c_in"] + 1 and out["parts"]["part"] == scratch.data_ptr() + 4 * nconv
                ops.grad_reduce_adam([dict(out["parts"])], [])
        else:
            lib = _lib.get()
            head = (ctypes.byref(d), ptr(eps1), ptr(X["v"]), ptr(X["pv"]), ptr(X["g_p"]), ptr(X["g_o"]), ptr(X["g_pv"]), ptr(X["g_v"]),
                    ptr(X["i2o_W"]))
            if open_form:
                part, nc = ctypes.c_void_p(), ctypes.c_int32(-1)
                rc = getattr(lib, "dcll_conv_lif_backward_%s_open" % entry)(*head, ptr(d_outW), ptr(d_outb), ptr(scratch), n, B,
                                                                           ctypes.byref(part), ctypes.byref(nc), stream_ptr())
                assert rc == 0, lib.dcll_last_error()
                nchunk = nc.value
                assert part.value == scratch.data_ptr() + 4 * nconv
                ops.grad_reduce_adam([dict(part=part.value, nchunk=nchunk, c_out=64, rowlen=3 * c["c_in"] + 1, dW=dW, db=db)], [])
            else:
                rc = getattr(lib, "dcll_conv_lif_backward_%s" % entry)(*head, ptr(dW), ptr(db), ptr(d_outW), ptr(d_outb), ptr(scratch), n,
                                                                      B, stream_ptr())
                assert rc == 0, lib.dcll_last_error()
        torch.cuda.synchronize()
    assert bool((buf[int(misalign) + n:] == -3.5).all()) and bool((buf[:int(misalign)] == -3.5).all()), "written outside the scratch"
    return dict(dW=dW, db=db, d_outW=d_outW, d_outb=d_outb, dv=scratch[:nconv].clone(), names=list(tr.names), nchunk=nchunk,
                part=scratch[nconv:].clone())


def expected_log(c, nchunk, misalign, open_form, want_out):
    wg = "k_bwd_wgrad_w3f (unaligned)" if misalign else "k_bwd_wgrad_w3f"
    return ["k_bwd_dv", wg] + ([] if open_form else [C.reduce_name(nchunk)]) + (["k_bwd_outgrad_mfma"] if want_out else []) + \
        (["k_grad_reduce_adam"] if open_form else [])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_backward_vs_float64_reference_and_bit_identities(dev, case):
    c, cid = case, case["id"]
    print(C.describe(c))
    T = C.draw(c)
    X = _tensors(c, T, dev)
    want_out = bool(c["output_layer"])
    if not want_out:
        X["g_o"] = None
    room, mis, via_ops = C.room(c), bool(c["misalign"]), c["scratch"] == "ops"
    nchunk = C.chunks(c, room=room)
    keys = ("dW", "db") + (("d_outW", "d_outb") if want_out else ())
    res = backward(c, X, dev, room, mis, via_ops=via_ops)
    print("kernels:", res["names"])
    # 4. the launch log: k_bwd_dv, exactly one k_bwd_wgrad_w3f of the predicted form, no generic k_bwd_wgrad, the predicted reduction
    assert res["names"] == expected_log(c, nchunk, mis, False, want_out), (cid, res["names"])
    # 1. against float64
    ref = C.reference(cid)
    for k in keys:
        assert_grad(res[k], ref[k], k, cid)
    # 3. a second run; the open form + the fused reduction; the other alignment: the same bits
    again = backward(c, X, dev, room, mis, via_ops=via_ops)
    opened = backward(c, X, dev, room, mis, open_form=True, via_ops=via_ops)
    other = backward(c, X, dev, room, not mis)
    assert opened["nchunk"] == nchunk and opened["names"] == expected_log(c, nchunk, mis, True, want_out), (cid, opened["names"])
    assert other["names"] == expected_log(c, nchunk, not mis, False, want_out), (cid, other["names"])
    for k in keys:
        assert bits_equal(again[k], res[k]), (cid, "second run", k)
        assert bits_equal(opened[k], res[k]), (cid, "open form + dcll_grad_reduce_adam", k)
        assert bits_equal(other[k], res[k]), (cid, "other alignment", k)
    assert bits_equal(other["part"][:nchunk * 256], res["part"][:nchunk * 256]), (cid, "partial rows, other alignment")
    # the dv plane, d_outW and d_outb are dcll_conv_lif_backward_w3's on the same inputs (its weight gradient: the generic kernel)
    w3 = backward(c, X, dev, room, mis, entry="w3")
    assert "k_bwd_wgrad" in w3["names"] and not any(n.startswith("k_bwd_wgrad_w3f") for n in w3["names"]), w3["names"]
    assert bits_equal(w3["dv"], res["dv"]), (cid, "dv plane")
    for k in keys[2:]:
        assert bits_equal(w3[k], res[k]), (cid, "dcll_conv_lif_backward_w3", k)
    for k in ("dW", "db"):                                                      # (another summation order: close, not equal)
        assert_grad(res[k], w3[k].detach().cpu().double(), k + " vs k_bwd_wgrad", cid)


BITWISE = ["w3f-16x2-B33", "w3f-1x256-B3", "w3f-2x128-B33", "w3f-16x128-B1"]


@pytest.mark.parametrize("cid", BITWISE)
def test_partial_rows_equal_the_restated_summation_order_bit_for_bit(dev, cid):
    """The summation order documented in the kernel's comment, restated in float32 by bwd_w3f_cases.wgrad_restated on the dv plane
    the device left in scratch, gives the kernel's partial rows bit for bit — with the case's chunk count, with one chunk and with
    three (ragged job lists, both wave parities busy), both alignments."""
    assert np.finfo(np.longdouble).nmant >= 63
    c = C.by_id(cid)
    T = C.draw(c)
    X = _tensors(c, T, dev)
    X["g_o"] = None
    for room in sorted({C.room(c), 1, 3}):
        nchunk = C.chunks(c, room=room)
        res = backward(c, X, dev, room, bool(c["misalign"]), open_form=True)
        assert res["nchunk"] == nchunk
        dv = res["dv"].cpu().numpy().reshape(c["B"], 64, c["h"], c["w"])
        part, _, _ = C.wgrad_restated(dv, T["eps1"], nchunk, fma=C.fma_ld)
        got = res["part"][:nchunk * 256].cpu().numpy().reshape(nchunk, 64, 4)
        assert np.abs(part).max() > 0
        assert bits_equal(got, part), (cid, room, int((got.view(np.uint32) != part.view(np.uint32)).sum()))


EXACT = [c for c in CASES if (c["h"], c["w"]) != (16, 128) and c["B"] <= 33]


@pytest.mark.parametrize("case", EXACT, ids=[c["id"] for c in EXACT])
def test_integer_draw_is_exact(dev, case):
    """g_p = g_pv = NULL: k_bwd_dv writes g_v itself; g_v in {-2 .. 2}, eps1 in {0 .. 3}: every product and partial sum is an integer
    below 2^24, so dW and db equal the integer reference EXACTLY in any summation order — every masking, halo or sample-boundary
    error shows without a tolerance.  Both alignments, the wrapper's scratch and a single partial row."""
    c = case
    Xd = C.exact_draw(c)
    X = dict(v=cu(Xd["v"], dev), pv=None, i2o_W=None, g_p=None, g_o=None, g_pv=None, g_v=cu(Xd["g_v"], dev),
             eps1={0: cu(Xd["eps1"], dev), 1: cu(Xd["eps1"], dev, True)})
    assert np.abs(Xd["dW"]).max() > 0
    for mis, room, via_ops in ((False, C.ops_chunks(c), True), (True, C.ops_chunks(c), False), (bool(c["misalign"]), 1, False)):
        res = backward(c, X, dev, room, mis, via_ops=via_ops)
        assert bits_equal(res["dv"].reshape(Xd["g_v"].shape), Xd["g_v"]), (c["id"], "dv = g_v")
        got_W, got_b = res["dW"].cpu().numpy().reshape(64, 3).astype(np.float64), res["db"].cpu().numpy().astype(np.float64)
        assert np.array_equal(got_W, Xd["dW"]), (c["id"], mis, room, np.argwhere(got_W != Xd["dW"])[:8])
        assert np.array_equal(got_b, Xd["db"]), (c["id"], mis, room)


def test_c_in_64_through_the_new_entry_point_is_the_w3_path(dev):
    """A 64 -> 64 layer through dcll_conv_lif_backward_w3f[_open] logs k_bwd_wgrad_w3 and gives dcll_conv_lif_backward_w3's bits."""
    c = S.by_id("w3-bwd-64to64-4x64-B3")
    T = S.bwd_draw(c)
    X = _tensors(c, T, dev)
    room = S.bwd_chunks(c, c["B"])
    keys = ("dW", "db") + (("d_outW", "d_outb") if c["output_layer"] else ())
    for open_form in (False, True):
        for via_ops in (False, True):
            a = backward(c, X, dev, room, False, open_form=open_form, entry="w3f", via_ops=via_ops)
            b = backward(c, X, dev, room, False, open_form=open_form, entry="w3", via_ops=via_ops)
            assert a["names"] == b["names"] and a["names"][:2] == ["k_bwd_dv", "k_bwd_wgrad_w3"], (a["names"], b["names"])
            for k in keys + ("dv",):
                assert bits_equal(a[k], b[k]), (open_form, via_ops, k)


def test_refusals_come_with_an_empty_launch_log(dev):
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    lib = _lib.get()
    base = dict(C.by_id("w3f-1x32-B3"), B=2)

    def call(r, open_form, scratch_floats, B, null_v=False):
        d = conv_desc(r)
        ch, cw, _, _ = FZ.conv_shape(r)
        eps1 = torch.rand(2, r["c_in"], r["h"], r["w"], device=dev)
        v = torch.randn(2, r["c_out"], ch, cw, device=dev)
        g_v = torch.randn_like(v)
        dW = torch.full((r["c_out"], r["c_in"], r["kh"], r["kw"]), -7.25, device=dev)
        db = torch.full((r["c_out"],), -7.25, device=dev)
        scratch = torch.full((max(scratch_floats, 0) + GUARD,), -3.5, device=dev)
        part, nchunk = ctypes.c_void_p(), ctypes.c_int32(-1)
        with ops.kernel_trace() as tr:
            if open_form:
                rc = lib.dcll_conv_lif_backward_w3f_open(ctypes.byref(d), ptr(eps1), None if null_v else ptr(v), None, None, None, None,
                                                         ptr(g_v), None, None, None, ptr(scratch), scratch_floats, B,
                                                         ctypes.byref(part), ctypes.byref(nchunk), stream_ptr())
            else:
                rc = lib.dcll_conv_lif_backward_w3f(ctypes.byref(d), ptr(eps1), None if null_v else ptr(v), None, None, None, None,
                                                    ptr(g_v), None, ptr(dW), ptr(db), None, None, ptr(scratch), scratch_floats, B,
                                                    stream_ptr())
            torch.cuda.synchronize()
        assert tr.names == [], (r, tr.names)
        assert bool((dW == -7.25).all()) and bool((db == -7.25).all()) and bool((scratch == -3.5).all()) and nchunk.value == -1
        return rc, lib.dcll_last_error().decode()
    need = 2 * 64 * 32 + 64 * 4
    for open_form in (False, True):
        for kw in (dict(c_out=32), dict(kh=3, kw=3, pad_h=1), dict(h=1, w=512)):
            rc, msg = call(dict(base, **kw), open_form, 10 ** 6, 2)
            assert rc == _lib.DCLL_ERR_UNSUPPORTED and "serves c_in 1 or 64, c_out 64, kernel (1,3)" in msg, (kw, rc, msg)
        rc, msg = call(base, open_form, need - 1, 2)
        assert rc == _lib.DCLL_ERR_INVALID and "scratch too small" in msg
        rc, msg = call(base, open_form, need, 2, null_v=True)
        assert rc == _lib.DCLL_ERR_INVALID and "v may be NULL only" in msg
        assert call(base, open_form, need, -1)[0] == _lib.DCLL_ERR_INVALID
        assert call(base, open_form, need, 0)[0] == _lib.DCLL_OK
    with pytest.raises(ValueError):
        ops.conv_lif_backward(conv_desc(base), torch.rand(2, 1, 1, 32, device=dev), torch.randn(2, 64, 1, 32, device=dev), None, None,
                              None, None, torch.randn(2, 64, 1, 32, device=dev), None, want_out=False, w3_first=True)


# ------------------------------------------------------------------------------------------------------------------------------
# network level: radio_ml_conv_ref.yaml on the (16,128) plane, w3_step_path (A) against w3_step_path + w3_first_wgrad (B)
# ------------------------------------------------------------------------------------------------------------------------------
def _net(B, burnin=20, first=False, **kw):
    net = W._net(B, burnin, w3=True, **kw)
    assert net.w3_first_wgrad is False and not any(s.w3_first_wgrad for s in net.dcll_slices)
    if first:
        net.w3_first_wgrad = True
        assert net.w3_first_wgrad is True and all(s.w3_first_wgrad for s in net.dcll_slices) and net.w3_step_path is True
    return net


def _wgrad_names(names):
    return [n for n in names if n.startswith("k_bwd_wgrad")]


def test_network_first_learning_step_and_six_steps_against_the_w3_path(dev):
    """Two identically seeded networks at B = 8: A with w3_step_path, Bn with w3_first_wgrad as well; before each learning step Bn
    takes A's parameters, optimizer state and neuron state (tests/test_gpu_step_w3.py's comparison against the default path), then
    both learn.  Every step: hidden spikes and state bit-identical, the gradients of layers 1-6 bit-identical, layer 0's dW / db
    within the weight-gradient tolerance; Bn logs one k_bwd_wgrad_w3f, six k_bwd_wgrad_w3 and no k_bwd_wgrad; A's log is the
    parent's."""
    from snn_modulation_classification_amd import ops
    B, burnin, steps = 8, 3, 6
    A, Bn = _net(B, burnin, learn=True), _net(B, burnin, first=True, learn=True)
    rng = np.random.RandomState(12)
    y = W._label(rng, B, dev)
    for t in range(burnin - 1 + steps):
        x = W._inputs(rng, B, 1, dev)[0]
        W._copy_everything(A, Bn)
        logs = []
        for net in (A, Bn):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(list(tr.names))
        learning = t >= burnin - 1
        assert [n for n in logs[0] if not n.startswith("k_bwd_wgrad")] == [n for n in logs[1] if not n.startswith("k_bwd_wgrad")]
        assert sorted(_wgrad_names(logs[0])) == (["k_bwd_wgrad"] + ["k_bwd_wgrad_w3"] * (N_LAYERS - 1) if learning else []), logs[0]
        assert sorted(_wgrad_names(logs[1])) == (["k_bwd_wgrad_w3"] * (N_LAYERS - 1) + ["k_bwd_wgrad_w3f"] if learning else []), logs[1]
        for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):
            for key in ("s", "p", "pv"):
                if torch.is_tensor(sa._learn_bufs.get(key)):
                    assert torch.equal(sa._learn_bufs[key], sb._learn_bufs[key]), (t, key)
            for u, v in zip(sa.dclllayer.i2h.state, sb.dclllayer.i2h.state):
                assert torch.equal(u, v), t
        if not learning:
            continue
        for i, (sa, sb) in enumerate(zip(A.dcll_slices, Bn.dcll_slices)):
            for (name, pa), (_, pb) in zip(sa.dclllayer.named_parameters(), sb.dclllayer.named_parameters()):
                assert (pa.grad is None) == (pb.grad is None), name
                if pa.grad is None:
                    continue
                if i == 0 and name in ("i2h.weight", "i2h.bias"):
                    assert float(pa.grad.abs().max()) > 0
                    assert_grad(pb.grad, pa.grad.detach().cpu().double(), "slice 0 %s.grad" % name, "step %d" % t)
                else:
                    assert torch.equal(pa.grad, pb.grad), (t, i, name)


def test_graph_captured_learning_steps_equal_eager_steps(dev):
    """With w3_first_wgrad the learning timestep replayed from its captured graph == the step launched eagerly, bit for bit, at
    B = 8; toggling the attribute changes the signature, so the capture is retaken."""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 8, 16, 4
    rng = np.random.RandomState(5)
    xs = W._inputs(rng, B, T, dev)
    y = W._label(rng, B, dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(B, burnin, first=True, learn=True, graph=graph)
        W._drive(net, xs, y, True)
    a, b = nets[True], nets[False]
    key = ((B, 1) + HW, (B, 24))
    g = a._learn_graphs[key]
    assert g["n"] >= 6 and not b._learn_graphs, (g["n"],)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter == T and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)
    sig = a._graph_signature()
    a.w3_first_wgrad = False
    assert a._graph_signature() != sig and a.w3_step_path is True
    with ops.kernel_trace() as tr:
        W._drive(a, xs[:1], y, True)
    assert a._learn_graphs.get(key) is not g and "k_bwd_wgrad" in tr.names and "k_bwd_wgrad_w3f" not in tr.names, tr.names


def test_learn_sequence_equals_per_step_learning(dev):
    """ConvNetwork.learn_sequence with w3_first_wgrad == the loop `for t: net.learn(x[t], y)` with it: weights, Adam state and clout
    bit for bit; one k_bwd_wgrad_w3f per learning step"""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 4, 9, 5
    rng = np.random.RandomState(6)
    cells = rng.randint(0, HW[0] * HW[1], size=(T, B)).astype(np.int32)
    y = W._label(rng, B, dev)
    a, b = _net(B, burnin, first=True, learn=True), _net(B, burnin, first=True, learn=True)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    n_learn = T - burnin + 1
    assert tr.names.count("k_bwd_wgrad_w3f") == n_learn and tr.names.count("k_bwd_wgrad_w3") == (N_LAYERS - 1) * n_learn, tr.names
    assert tr.names.count("k_bwd_wgrad") == 0
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


def test_the_rank_sharded_step_runs_with_the_first_layer_kernel(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks (the CLOSED backward per slice: dcll_conv_lif_backward_w3f + k_bwd_reduce, then
    ops.adam_step) with the collective of a one-rank world == the single-process step (open form + dcll_grad_reduce_adam), bit for
    bit (modelled on tests/test_gpu_step_w3.py::test_the_rank_sharded_step_runs_on_the_w3_path)."""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 5, 3
    rng = np.random.RandomState(9)
    xs = W._inputs(rng, B, T, dev)
    y = W._label(rng, B, dev)
    a, b = _net(B, burnin, first=True, learn=True), _net(B, burnin, first=True, learn=True)
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
    assert tr.names.count("k_bwd_wgrad_w3") == (N_LAYERS - 1) * n_learn and tr.names.count("k_bwd_wgrad_w3f") == n_learn, tr.names
    assert tr.names.count("k_bwd_wgrad") == 0
    assert sum(n.startswith("k_bwd_reduce") for n in tr.names) == N_LAYERS * n_learn and tr.count("k_grad_reduce_adam") == 0, tr.names
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))


def test_the_setter_refuses_without_the_w3_path_and_is_cleared_with_it(dev):
    from snn_modulation_classification_amd import _lib
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    assert DCLLBase.w3_first_wgrad is False
    net = W._net(2, learn=True)
    assert net.w3_step_path is False and net.w3_first_wgrad is False
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_first_wgrad = True
    assert net.w3_first_wgrad is False and not any(s.w3_first_wgrad for s in net.dcll_slices)
    net.w3_first_wgrad = False                      # switching it off is always allowed
    net.w3_step_path = True
    net.w3_first_wgrad = True
    assert net.w3_first_wgrad is True
    sig = net._graph_signature()
    net.w3_step_path = False                        # clears it as well
    assert net.w3_first_wgrad is False and not any(s.w3_first_wgrad for s in net.dcll_slices) and net._graph_signature() != sig
    net = W._net(2, spec="radio_ml_conv.yaml", hw=(24, 24))
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_first_wgrad = True
    assert net.w3_first_wgrad is False


def test_entry_point_train_w3_first_wgrad(tmp_path, capsys):
    """train.py --w3_step_path --w3_first_wgrad runs its first layer's weight gradient on k_bwd_wgrad_w3f and stores the accuracies of
    --w3_step_path alone (a learning rate of 1e-7 over one step: the other summation order does not reach a spike); --w3_first_wgrad
    alone prints the notice and changes nothing"""
    import train
    common = ['--I_resolution', '128', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '8',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7',
              '--network_spec', os.path.join(PKG, 'networks', 'radio_ml_conv_ref.yaml')]
    runs = {}
    for name, flags in (("w3", ['--w3_step_path']), ("first", ['--w3_step_path', '--w3_first_wgrad']), ("alone", ['--w3_first_wgrad'])):
        with W._trace() as tr:
            out = train.main(common + ['--output', str(tmp_path / name)] + flags)
        text = capsys.readouterr().out
        runs[name] = (np.load(os.path.join(out, 'acc_test.npy')), list(tr.names), text)
    a, names, text = runs["w3"]
    assert "ignored" not in text and "k_bwd_wgrad" in names and "k_bwd_wgrad_w3f" not in names and np.isfinite(a).all()
    b, names, text = runs["first"]
    assert "ignored" not in text and "k_bwd_wgrad_w3f" in names and "k_bwd_wgrad_w3" in names and "k_bwd_wgrad" not in names
    assert np.array_equal(a, b), (a, b)
    _, names, text = runs["alone"]
    assert "--w3_first_wgrad ignored" in text and not any(n.startswith(("k_bwd_wgrad_w3", "k_lif_step_w3")) for n in names)
