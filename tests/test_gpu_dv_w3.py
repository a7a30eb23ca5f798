"""GPU tests of the opt-in streaming dv kernel of the (1,3) / (1,2)-pool layers: dcll_conv_lif_backward_w3_ex[_open] with DCLL_W3_DV
(k_bwd_dv_w3), on the cases of tests/dv_w3_cases.py (proven on the CPU by tests/test_dv_w3_cases.py), through
ops.conv_lif_backward(w3_path=True, w3_first=..., w3_dv=True) — the binding the product uses — and the C ABI where the case sets its
own scratch size, and through ConvNetwork.w3_dv_path / train.py.

Every case: the dv plane left in scratch, dW, db, d_outW and d_outb are the bits of the same call with w3_dv=False (k_bwd_dv) — closed
form, open form + ops.grad_reduce_adam, flags 2 and 3; a second run and the other alignment give the same bits; the launch log is
the parent's with its "k_bwd_dv" replaced by the predicted form; on the grid draws dv is within rtol 1e-5 / atol 1e-6 max|ref| of
float64.  Then the refusals, the flag equivalences, and the network level: radio_ml_conv_ref.yaml on the (16,128) plane with
w3_step_path + w3_first_wgrad + w3_dv_path against the same network without w3_dv_path, bit for bit."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import dv_w3_cases as C
import fuzz_cases as FZ
import test_gpu_step_w3 as W        # its helpers (network builders, comparisons); its tests are not re-exported here
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
CASES = C.cases()
HW, N_LAYERS = W.HW, W.N_LAYERS
cu, bits_equal, conv_desc = W.cu, W.bits_equal, W.conv_desc
GUARD = 64
SERVED = collections.Counter()      # form (template width, alignment) -> runs it served
RAN = set()
OPT_IN = ("k_lif_step_w3", "k_bwd_wgrad_w3", "k_bwd_dv_w3")       # the kernels of the opt-in learning path


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
    """every tensor of the call in both placements: X[name][0] on a 16-byte boundary, X[name][1] one float behind one"""
    v = cu(T["v"], dev)
    X = dict(eps1=cu(T["eps1"], dev), pv=torch.sigmoid(torch.nn.functional.max_pool2d(v, (1, 2))),
             g_o=cu(T["g_o"], dev) if c["output_layer"] else None, g_p=cu(T["g_p"], dev))
    for k in ("v", "g_v", "g_pv", "i2o_W"):
        X[k] = {0: cu(T[k], dev), 1: cu(T[k], dev, True)}
    return X


def backward(c, X, dev, off, dv, first=None, open_form=False, via_ops=None, room=None):
    """One backward call -> dict(dW, db, d_outW, d_outb, dv (the plane left in scratch), names).  off: the case's bit mask of the
    pointers one float off a 16-byte boundary; dv: DCLL_W3_DV; first: DCLL_W3_FIRST_WGRAD.  via_ops: through
    ops.conv_lif_backward with its own scratch size (the view handed in must be the one it keeps); else through the C ABI with room
    for `room` partial rows — with dv through dcll_conv_lif_backward_w3_ex[_open], without through the entry points of the parent."""
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    first = bool(c["first"]) if first is None else first
    via_ops = c["scratch"] == "ops" if via_ops is None else via_ops
    room = (C.ops_room(dict(c, first=int(first))) if via_ops else 1) if room is None else room
    d = conv_desc(c)
    B, nconv = c["B"], c["B"] * 64 * c["h"] * c["w"]
    n = nconv + room * 64 * (3 * c["c_in"] + 1)
    so = int(bool(off & C.OFF_SCRATCH))
    buf, scratch = _scratch(n, so, dev)
    v, g_v = X["v"][int(bool(off & C.OFF_V))], X["g_v"][int(bool(off & C.OFF_GV))]
    g_pv, i2o_W = X["g_pv"][int(bool(off & C.OFF_GPV))], X["i2o_W"][int(bool(off & C.OFF_W))]
    want_out = X["g_o"] is not None
    K = C.K(c)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    dW, db = nan(64, c["c_in"], 1, 3), nan(64)
    d_outW, d_outb = (nan(c["target"], K), nan(c["target"])) if want_out else (None, None)
    with ops.kernel_trace() as tr:
        if via_ops:
            out = dict(dW=dW, db=db, bwd_scratch=scratch)
            if want_out:
                out.update(d_outW=d_outW, d_outb=d_outb)
            ops.conv_lif_backward(d, X["eps1"], v, X["pv"], X["g_p"], X["g_o"], g_pv, g_v, i2o_W, want_out=want_out, out=out,
                                  open_reduce=open_form, w3_path=True, w3_first=first, w3_dv=dv)
            assert out["bwd_scratch"] is scratch, "ops.conv_lif_backward's scratch size is not the restated one"
            if open_form:
                assert out["parts"]["part"] == scratch.data_ptr() + 4 * nconv
                ops.grad_reduce_adam([dict(out["parts"])], [])
        else:
            lib = _lib.get()
            head = (ctypes.byref(d), ptr(X["eps1"]), ptr(v), ptr(X["pv"]), ptr(X["g_p"]), ptr(X["g_o"]), ptr(g_pv), ptr(g_v), ptr(i2o_W))
            name = "dcll_conv_lif_backward_w3_ex" if dv else "dcll_conv_lif_backward_w3f" if first else "dcll_conv_lif_backward_w3"
            fl = ((2 | int(first)),) if dv else ()
            if open_form:
                part, nc = ctypes.c_void_p(), ctypes.c_int32(-1)
                rc = getattr(lib, name + "_open")(*head, ptr(d_outW), ptr(d_outb), ptr(scratch), n, B, ctypes.byref(part),
                                                  ctypes.byref(nc), *fl, stream_ptr())
                assert rc == 0, lib.dcll_last_error()
                assert part.value == scratch.data_ptr() + 4 * nconv
                ops.grad_reduce_adam([dict(part=part.value, nchunk=nc.value, c_out=64, rowlen=3 * c["c_in"] + 1, dW=dW, db=db)], [])
            else:
                rc = getattr(lib, name)(*head, ptr(dW), ptr(db), ptr(d_outW), ptr(d_outb), ptr(scratch), n, B, *fl, stream_ptr())
                assert rc == 0, lib.dcll_last_error()
        torch.cuda.synchronize()
    assert bool((buf[so + n:] == -3.5).all()) and bool((buf[:so] == -3.5).all()), "written outside the scratch"
    return dict(dW=dW, db=db, d_outW=d_outW, d_outb=d_outb, dv=scratch[:nconv].clone(), names=list(tr.names))


def expected_log(c, parent_names, off):
    """the parent's log with its one k_bwd_dv replaced by the predicted form (target 33: k_bwd_dv stays)"""
    assert parent_names[0] == "k_bwd_dv" and sum(n.startswith("k_bwd_dv") for n in parent_names) == 1, parent_names
    return [C.form_name(c, off)] + parent_names[1:]


def assert_dv(got, ref, cid):
    ref = ref.numpy()
    got = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    err = np.abs(got - ref)
    print("%s dv: max|err| %.3g, max|ref| %.3g, worst excess over rtol %.3g (atol %.3g)"
          % (cid, err.max(), scale, float((err - C.DV_RTOL * np.abs(ref)).max()), C.DV_ATOL * scale))
    np.testing.assert_allclose(got, ref, rtol=C.DV_RTOL, atol=C.DV_ATOL * scale + 1e-30, err_msg="%s dv" % cid)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_gives_the_bits_of_k_bwd_dv(dev, case):
    c, cid = case, case["id"]
    print(C.describe(c))
    T = C.draw(c)
    X = _tensors(c, T, dev)
    off, want_out = c["off"], bool(c["output_layer"])
    keys = ("dv", "dW", "db") + (("d_outW", "d_outb") if want_out else ())
    for first in (not c["first"], bool(c["first"])):                            # the other flag word first, then the case's (2 | first)
        parent = backward(c, X, dev, off, False, first=first)
        res = backward(c, X, dev, off, True, first=first)
        print("first %d kernels:" % first, res["names"])
        # 4. the launch log: the parent's with exactly one k_bwd_dv_w3 of the predicted form in the place of k_bwd_dv
        assert res["names"] == expected_log(c, parent["names"], off), (cid, res["names"], parent["names"])
        if C.served(c):
            assert "k_bwd_dv" not in res["names"] and sum(n.startswith("k_bwd_dv_w3") for n in res["names"]) == 1
            SERVED[C.form_key(c, off)] += 1
        else:
            assert c["target"] == 33 and res["names"][0] == "k_bwd_dv"
        # 1. + 2. the plane and every gradient, bit for bit (uint32 views)
        assert float(res["dv"].abs().max()) > 0 or (c["gsel"] == "none" and not c["with_gv"])
        for k in keys:
            assert bits_equal(res[k], parent[k]), (cid, first, k, "w3_dv=True against w3_dv=False")
        opened = backward(c, X, dev, off, True, first=first, open_form=True)
        opened_parent = backward(c, X, dev, off, False, first=first, open_form=True)
        assert opened["names"] == expected_log(c, opened_parent["names"], off), (cid, opened["names"])
        for k in keys:
            assert bits_equal(opened[k], res[k]), (cid, first, k, "open form + dcll_grad_reduce_adam")
            assert bits_equal(opened_parent[k], res[k]), (cid, first, k, "the parent's open form")
    # 3. against float64 (the grid draws: the other two are for the bit comparison only)
    if c["draw"] == "grid":
        assert_dv(res["dv"], C.reference(cid)["dv"], cid)
    # 5. a second run; the other alignment of every pointer; the other route to the library: the same bits
    again = backward(c, X, dev, off, True)
    other = backward(c, X, dev, off ^ 31, True)
    # (the wrapper's scratch size handed to the C ABI: the same partial rows; a "k1" case went through the C ABI already)
    route = backward(c, X, dev, off, True, via_ops=False, room=C.room(c))
    assert other["names"][0] == C.form_name(c, off ^ 31), (cid, other["names"])
    if C.served(c):
        SERVED[C.form_key(c, off ^ 31)] += 1
    for k in keys:
        assert bits_equal(again[k], res[k]), (cid, "second run", k)
        assert bits_equal(other[k], res[k]), (cid, "other alignment", k)
        assert bits_equal(route[k], res[k]), (cid, "C ABI / ops", k)
    RAN.add(cid)


def test_every_form_served_a_case():
    """a parity test is only worth its name if it ran the kernel it claims to cover (runs behind the cases above)"""
    assert RAN == {c["id"] for c in CASES}, sorted({c["id"] for c in CASES} - RAN)
    assert set(SERVED) == set(C.all_forms()), (set(C.all_forms()) - set(SERVED), dict(SERVED))
    print("runs per form:", dict(SERVED))


def test_flags_0_and_1_are_the_w3_and_w3f_entry_points(dev):
    """dcll_conv_lif_backward_w3_ex[_open] with flags 0 / 1 == dcll_conv_lif_backward_w3[_open] / _w3f[_open]: bits and launch logs,
    on a first layer and a 64 -> 64 layer"""
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    lib = _lib.get()
    for cid in ("dvw3-16x128-B2-32", "dvw3-4x64-B7-26"):
        c = C.by_id(cid)
        X = _tensors(c, C.draw(c), dev)
        d = conv_desc(c)
        B, nconv = c["B"], c["B"] * 64 * c["h"] * c["w"]
        n = nconv + 3 * 64 * (3 * c["c_in"] + 1)
        head = (ctypes.byref(d), ptr(X["eps1"]), ptr(X["v"][0]), ptr(X["pv"]), ptr(X["g_p"]), ptr(X["g_o"]), ptr(X["g_pv"][0]),
                ptr(X["g_v"][0]), ptr(X["i2o_W"][0]))
        want_out = X["g_o"] is not None
        for flags, old in ((0, "dcll_conv_lif_backward_w3"), (1, "dcll_conv_lif_backward_w3f")):
            for open_form in (False, True):
                got = []
                for name, fl in ((old, ()), ("dcll_conv_lif_backward_w3_ex", (flags,))):
                    scratch = torch.full((n,), -3.5, device=dev)
                    dW, db = torch.zeros(64, c["c_in"], 1, 3, device=dev), torch.zeros(64, device=dev)
                    d_outW = torch.zeros(c["target"], C.K(c), device=dev) if want_out else None
                    d_outb = torch.zeros(c["target"], device=dev) if want_out else None
                    with ops.kernel_trace() as tr:
                        if open_form:
                            part, nc = ctypes.c_void_p(), ctypes.c_int32(-1)
                            rc = getattr(lib, name + "_open")(*head, ptr(d_outW), ptr(d_outb), ptr(scratch), n, B, ctypes.byref(part),
                                                              ctypes.byref(nc), *fl, stream_ptr())
                            extra = (nc.value, part.value - scratch.data_ptr())
                        else:
                            rc = getattr(lib, name)(*head, ptr(dW), ptr(db), ptr(d_outW), ptr(d_outb), ptr(scratch), n, B, *fl, stream_ptr())
                            extra = ()
                        torch.cuda.synchronize()
                    assert rc == 0, lib.dcll_last_error()
                    got.append((list(tr.names), extra, [scratch, dW, db] + ([d_outW, d_outb] if want_out else [])))
                (na, ea, ta), (nb, eb, tb) = got
                assert na == nb and na[0] == "k_bwd_dv" and ea == eb, (cid, flags, open_form, na, nb)
                assert ("k_bwd_wgrad_w3f" in na) == (flags == 1 and c["c_in"] == 1)
                for a, b in zip(ta, tb):
                    assert bits_equal(a, b), (cid, flags, open_form)


def test_refusals_come_with_an_empty_launch_log(dev):
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    lib = _lib.get()
    base = dict(C.by_id("dvw3-1x32-B3-7"), B=2, target=10)

    def call(r, open_form, scratch_floats, B, flags, null_v=False, g_p=False, i2o_W=False):
        d = conv_desc(r)
        ch, cw, _, _ = FZ.conv_shape(r)
        eps1 = torch.rand(2, r["c_in"], r["h"], r["w"], device=dev)
        v = torch.randn(2, r["c_out"], ch, cw, device=dev)
        g_v = torch.randn_like(v)
        gp = torch.randn(2, r["target"], device=dev) if g_p else None
        Wr = torch.randn(r["target"], r["c_out"] * ch * (cw // 2), device=dev) if i2o_W else None
        dW = torch.full((r["c_out"], r["c_in"], r["kh"], r["kw"]), -7.25, device=dev)
        db = torch.full((r["c_out"],), -7.25, device=dev)
        scratch = torch.full((max(scratch_floats, 0) + GUARD,), -3.5, device=dev)
        part, nchunk = ctypes.c_void_p(), ctypes.c_int32(-1)
        with ops.kernel_trace() as tr:
            if open_form:
                rc = lib.dcll_conv_lif_backward_w3_ex_open(ctypes.byref(d), ptr(eps1), None if null_v else ptr(v), None, ptr(gp), None,
                                                           None, ptr(g_v), ptr(Wr), None, None, ptr(scratch), scratch_floats, B,
                                                           ctypes.byref(part), ctypes.byref(nchunk), flags, stream_ptr())
            else:
                rc = lib.dcll_conv_lif_backward_w3_ex(ctypes.byref(d), ptr(eps1), None if null_v else ptr(v), None, ptr(gp), None, None,
                                                      ptr(g_v), ptr(Wr), ptr(dW), ptr(db), None, None, ptr(scratch), scratch_floats, B,
                                                      flags, stream_ptr())
            torch.cuda.synchronize()
        assert tr.names == [], (r, tr.names)
        assert bool((dW == -7.25).all()) and bool((db == -7.25).all()) and bool((scratch == -3.5).all()) and nchunk.value == -1
        return rc, lib.dcll_last_error().decode()
    for open_form in (False, True):
        for c_in in (1, 64):
            r0 = dict(base, c_in=c_in)
            need = 2 * 64 * 32 + 64 * (3 * c_in + 1)
            for flags in (4, 6, 0x102):                                         # unknown flag bits
                rc, msg = call(r0, open_form, need, 2, flags)
                assert rc == _lib.DCLL_ERR_INVALID and "unknown flag bits" in msg, (flags, rc, msg)
            for flags in (2, 3):
                for kw in (dict(c_out=32), dict(kh=3, kw=3, pad_h=1), dict(h=1, w=512), dict(pool_w=1)):   # outside the w3 geometry
                    rc, msg = call(dict(r0, **kw), open_form, 10 ** 6, 2, flags)
                    assert rc == _lib.DCLL_ERR_UNSUPPORTED and "serves c_in 1 or 64, c_out 64, kernel (1,3)" in msg, (kw, rc, msg)
                rc, msg = call(r0, open_form, need, 2, flags, null_v=True)
                assert rc == _lib.DCLL_ERR_INVALID and "v may be NULL only" in msg
                rc, msg = call(r0, open_form, need, 2, flags, g_p=True)
                assert rc == _lib.DCLL_ERR_INVALID and "g_p needs i2o_W" in msg
                rc, msg = call(r0, open_form, need - 1, 2, flags)
                assert rc == _lib.DCLL_ERR_INVALID and "scratch too small" in msg
                assert call(r0, open_form, need, -1, flags)[0] == _lib.DCLL_ERR_INVALID
                assert call(r0, open_form, need, 0, flags)[0] == _lib.DCLL_OK
    with pytest.raises(ValueError):
        ops.conv_lif_backward(conv_desc(base), torch.rand(2, base["c_in"], 1, 32, device=dev), torch.randn(2, 64, 1, 32, device=dev), None,
                              None, None, None, torch.randn(2, 64, 1, 32, device=dev), None, want_out=False, w3_dv=True)


# ------------------------------------------------------------------------------------------------------------------------------
# network level: radio_ml_conv_ref.yaml on the (16,128) plane, w3_step_path + w3_first_wgrad (A) against the same + w3_dv_path (B)
# ------------------------------------------------------------------------------------------------------------------------------
def _net(B, burnin=20, dv=False, first=True, **kw):
    net = W._net(B, burnin, w3=True, **kw)
    assert net.w3_dv_path is False and not any(s.w3_dv for s in net.dcll_slices)
    net.w3_first_wgrad = first
    if dv:
        net.w3_dv_path = True
        assert net.w3_dv_path is True and all(s.w3_dv for s in net.dcll_slices) and net.w3_step_path is True
        assert net.w3_first_wgrad is first                                      # (independent of it)
    return net


def _dv_names(names):
    return [n for n in names if n.startswith("k_bwd_dv")]


def _swap(names):
    return ["k_bwd_dv_w3" if n == "k_bwd_dv" else n for n in names]


def _assert_same_networks(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        assert sl_a.iter == sl_b.iter and np.array_equal(np.asarray(sl_a.clout), np.asarray(sl_b.clout))
        for ta, tb in zip(sl_a.dclllayer.i2h.state, sl_b.dclllayer.i2h.state):
            assert torch.equal(ta, tb)
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))
        oa, ob = sl_a.optimizer, sl_b.optimizer
        for pa, pb in zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"]):
            assert (pa in oa.state) == (pb in ob.state)
            for key, val in oa.state.get(pa, {}).items():
                if torch.is_tensor(val):
                    assert torch.equal(val, ob.state[pb][key]), key


def test_network_six_learning_steps_are_bit_identical(dev):
    """Two identically seeded networks at B = 8, both with w3_step_path + w3_first_wgrad, Bn with w3_dv_path as well, driven by the same
    inputs WITHOUT copying anything across: spikes, state, every gradient, Adam's state and the parameters stay bit-identical over
    burn-in and six learning steps; Bn's log is A's with every k_bwd_dv replaced by k_bwd_dv_w3 (seven per learning step); a network
    on the default path logs what it logged before."""
    from snn_modulation_classification_amd import ops
    B, burnin, steps = 8, 3, 6
    A, Bn, D = _net(B, burnin, learn=True), _net(B, burnin, dv=True, learn=True), W._net(B, burnin, learn=True)
    rng = np.random.RandomState(12)
    y = W._label(rng, B, dev)
    for t in range(burnin - 1 + steps):
        x = W._inputs(rng, B, 1, dev)[0]
        logs = []
        for net in (A, Bn, D):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(list(tr.names))
        learning = t >= burnin - 1
        assert logs[1] == _swap(logs[0]), (t, logs[0], logs[1])
        assert _dv_names(logs[0]) == (["k_bwd_dv"] * N_LAYERS if learning else []), logs[0]
        assert _dv_names(logs[1]) == (["k_bwd_dv_w3"] * N_LAYERS if learning else []), logs[1]
        # the default path (no opt-in at all): its own dv kernel, none of the w3 kernels
        assert _dv_names(logs[2]) == (["k_bwd_dv"] * N_LAYERS if learning else []) and not any(n.startswith(OPT_IN) for n in logs[2]), logs[2]
        for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):
            for key in ("s", "p", "pv"):
                if torch.is_tensor(sa._learn_bufs.get(key)):
                    assert torch.equal(sa._learn_bufs[key], sb._learn_bufs[key]), (t, key)
        _assert_same_networks(A, Bn)
        if learning:
            assert all(float(s.dclllayer.i2h.weight.grad.abs().max()) > 0 for s in Bn.dcll_slices)


def test_graph_captured_learning_steps_equal_eager_steps(dev):
    """With w3_dv_path the learning timestep replayed from its captured graph == the step launched eagerly, bit for bit, at B = 8;
    toggling the attribute changes the signature, so the capture is retaken."""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 8, 16, 4
    rng = np.random.RandomState(5)
    xs = W._inputs(rng, B, T, dev)
    y = W._label(rng, B, dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(B, burnin, dv=True, learn=True, graph=graph)
        W._drive(net, xs, y, True)
    a, b = nets[True], nets[False]
    key = ((B, 1) + HW, (B, 24))
    g = a._learn_graphs[key]
    assert g["n"] >= 6 and not b._learn_graphs, (g["n"],)
    _assert_same_networks(a, b)
    sig = a._graph_signature()
    a.w3_dv_path = False
    assert a._graph_signature() != sig and a.w3_step_path is True and a.w3_first_wgrad is True
    with ops.kernel_trace() as tr:
        W._drive(a, xs[:1], y, True)
    assert a._learn_graphs.get(key) is not g and "k_bwd_dv" in tr.names and "k_bwd_dv_w3" not in tr.names, tr.names


def test_learn_sequence_equals_per_step_learning(dev):
    """ConvNetwork.learn_sequence with w3_dv_path == the loop `for t: net.learn(x[t], y)` with it: weights, Adam state and clout bit
    for bit; seven k_bwd_dv_w3 per learning step, no k_bwd_dv"""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 4, 9, 5
    rng = np.random.RandomState(6)
    cells = rng.randint(0, HW[0] * HW[1], size=(T, B)).astype(np.int32)
    y = W._label(rng, B, dev)
    a, b = _net(B, burnin, dv=True, learn=True), _net(B, burnin, dv=True, learn=True)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    n_learn = T - burnin + 1
    assert tr.names.count("k_bwd_dv_w3") == N_LAYERS * n_learn and tr.names.count("k_bwd_dv") == 0, tr.names
    x = np.zeros((T, B, HW[0] * HW[1]), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape(T, B, 1, *HW)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    _assert_same_networks(a, b)
    st = a.dcll_slices[0].optimizer.state[a.dcll_slices[0].dclllayer.i2h.weight]
    assert float(st["step"]) == n_learn


def test_the_rank_sharded_step_runs_with_the_dv_kernel(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks (the CLOSED backward per slice: dcll_conv_lif_backward_w3_ex + k_bwd_reduce, then
    ops.adam_step) with the collective of a one-rank world == the single-process step (open form + dcll_grad_reduce_adam), bit for
    bit (modelled on tests/test_gpu_step_w3.py::test_the_rank_sharded_step_runs_on_the_w3_path)."""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 5, 3
    rng = np.random.RandomState(9)
    xs = W._inputs(rng, B, T, dev)
    y = W._label(rng, B, dev)
    a, b = _net(B, burnin, dv=True, learn=True), _net(B, burnin, dv=True, learn=True)
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
    assert tr.names.count("k_bwd_dv_w3") == N_LAYERS * n_learn and tr.names.count("k_bwd_dv") == 0, tr.names
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
    assert DCLLBase.w3_dv is False
    net = W._net(2, learn=True)
    assert net.w3_step_path is False and net.w3_dv_path is False
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_dv_path = True
    assert net.w3_dv_path is False and not any(s.w3_dv for s in net.dcll_slices)
    net.w3_dv_path = False                          # switching it off is always allowed
    net.w3_step_path = True
    net.w3_dv_path = True                           # without w3_first_wgrad: independent of it
    assert net.w3_dv_path is True and net.w3_first_wgrad is False
    sig = net._graph_signature()
    net.w3_first_wgrad = True
    assert net.w3_dv_path is True and net._graph_signature() != sig
    sig = net._graph_signature()
    net.w3_step_path = False                        # clears both
    assert net.w3_dv_path is False and net.w3_first_wgrad is False and not any(s.w3_dv for s in net.dcll_slices)
    assert net._graph_signature() != sig
    net = W._net(2, spec="radio_ml_conv.yaml", hw=(24, 24))
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_dv_path = True
    assert net.w3_dv_path is False


def test_entry_point_train_w3_dv_path(tmp_path, capsys):
    """train.py --w3_step_path --w3_dv_path runs every layer's dv on k_bwd_dv_w3 and stores the accuracies of --w3_step_path alone;
    --w3_dv_path alone prints the notice and changes nothing; on radio_ml_conv.yaml both flags are ignored with a notice"""
    import train
    common = ['--I_resolution', '128', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '8',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7',
              '--network_spec', os.path.join(PKG, 'networks', 'radio_ml_conv_ref.yaml')]
    runs = {}
    for name, flags in (("w3", ['--w3_step_path']), ("dv", ['--w3_step_path', '--w3_dv_path']), ("alone", ['--w3_dv_path'])):
        with W._trace() as tr:
            out = train.main(common + ['--output', str(tmp_path / name)] + flags)
        text = capsys.readouterr().out
        runs[name] = (np.load(os.path.join(out, 'acc_test.npy')), list(tr.names), text)
    a, names, text = runs["w3"]
    assert "ignored" not in text and "k_bwd_dv" in names and "k_bwd_dv_w3" not in names and np.isfinite(a).all()
    b, names_dv, text = runs["dv"]
    assert "ignored" not in text and "k_bwd_dv_w3" in names_dv and "k_bwd_dv" not in names_dv
    assert names_dv == _swap(names) and np.array_equal(a, b), (a, b)
    _, names, text = runs["alone"]
    assert "--w3_dv_path ignored" in text and not any(n.startswith(OPT_IN) for n in names)
    with W._trace() as tr:
        train.main(['--I_resolution', '24', '--Q_resolution', '24', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
                    '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '6', '--n_iters_test', '6',
                    '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7', '--output', str(tmp_path / 'radio'),
                    '--w3_step_path', '--w3_dv_path'])
    text = capsys.readouterr().out
    assert "--w3_step_path ignored" in text and "--w3_dv_path ignored" in text and not any(n.startswith(OPT_IN) for n in tr.names)
