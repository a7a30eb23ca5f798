"""GPU tests of the opt-in streaming dv kernel of the layers that pool: dcll_conv_lif_backward_ex[_open] with DCLL_BWD_POOL_DV
(k_bwd_dv_pool), on the cases of tests/pool_dv_cases.py (proven on the CPU by tests/test_pool_dv_cases.py) through the C ABI, and
through ConvNetwork.pool_dv_path / train.py.

Every case: the dv plane left in scratch, dW, db, d_outW, d_outb and (open form) the partial rows are the bits of THE SAME ENTRY POINT
WITH flags = 0 — k_bwd_dv, the kernel this project ships: the reference, never the code under test; DCLL_BWD_DEFAULT with flags = 0 is
dcll_conv_lif_backward itself; the launch log is the unflagged one with its "k_bwd_dv" replaced by the predicted entry; a second run
gives the same bits; scratch and every output sit in front of a sentinel tail; on the grid draws dv is within rtol 1e-5 / atol 1e-6
max|ref| of float64 autograd; on the (1,2) cases of the radio geometry the plane is dcll_conv_lif_backward_w3_ex's with DCLL_W3_DV
too.  Then the refusals, the predicate, and the network level on mnist_conv.yaml."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import pool_dv_cases as C
import test_gpu_bwd_wide as BWT     # its helpers (network builders, state copy); its tests are not re-exported here
import test_gpu_step_w3 as W        # likewise
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
CASES = C.cases()
cu, bits_equal, conv_desc = W.cu, W.bits_equal, W.conv_desc
GUARD, SENT = 64, -3.5
SERVED = collections.Counter()      # template instance -> cases it served
RAN = set()
COUNTS = os.path.join(ROOT, "profiles", "r28_pool_dv_case_counts.txt")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _guarded(n, dev, off=0, fill=SENT):
    """(buffer, view of n floats at 0 or 4 (mod 16) bytes): GUARD sentinel floats stay behind the view"""
    buf = torch.full((n + GUARD + 4,), fill, device=dev)
    view = buf[off:off + n]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    return buf, view


def _intact(buf, off, n):
    return bool((buf[off + n:] == SENT).all()) and bool((buf[:off] == SENT).all())


def _tensors(c, T, dev):
    """every tensor of the call; v, g_v, g_pv and i2o_W in both placements (X[name][1]: one float behind a 16-byte boundary)"""
    v = cu(T["v"], dev)
    pool = (c["pool_h"], c["pool_w"])
    pv = torch.nn.functional.max_pool2d(torch.sigmoid(v), pool, pool, ((pool[0] - 1) // 2, (pool[1] - 1) // 2)).contiguous()
    X = dict(eps1=cu(T["eps1"], dev), pv=pv, g_o=cu(T["g_o"], dev), g_p=cu(T["g_p"], dev))
    for k in ("v", "g_v", "g_pv", "i2o_W"):
        X[k] = {0: cu(T[k], dev), 1: cu(T[k], dev, True)}
    return X


def backward(c, X, dev, flags, open_form=False, entry="ex", off=None):
    """One backward call through the C ABI -> dict(dv, dW, db, d_outW, d_outb, part (open form: the partial rows), names).
    entry: "ex" (dcll_conv_lif_backward_ex[_open] with the case's path and `flags`), "plain" (dcll_conv_lif_backward[_open]) or "w3"
    (dcll_conv_lif_backward_w3_ex[_open] with DCLL_W3_DV)."""
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    lib = _lib.get()
    off = c["off"] if off is None else off
    d = conv_desc(c)
    ch, cw, _, _ = C.shape(c)
    B, nconv, n = c["B"], c["B"] * c["c_out"] * ch * cw, C.scratch_floats(c)
    so = int(bool(off & C.OFF_SCRATCH))
    sbuf, scratch = _guarded(n, dev, so)
    pick = lambda k, bit: X[k][int(bool(off & bit))]
    v, g_v, g_pv, i2o_W = pick("v", C.OFF_V), pick("g_v", C.OFF_GV), pick("g_pv", C.OFF_GPV), pick("i2o_W", C.OFF_W)
    want_out = X["g_o"] is not None
    rl = C.rowlen(c)
    outs = dict(dW=_guarded(c["c_out"] * (rl - 1), dev), db=_guarded(c["c_out"], dev))
    if want_out:
        outs.update(d_outW=_guarded(c["target"] * C.K(c), dev), d_outb=_guarded(c["target"], dev))
    o = lambda k: outs[k][1] if k in outs else None
    head = (ctypes.byref(d), ptr(X["eps1"]), ptr(v), ptr(X["pv"]), ptr(X["g_p"]), ptr(X["g_o"]), ptr(g_pv), ptr(g_v), ptr(i2o_W))
    name = {"ex": "dcll_conv_lif_backward_ex", "plain": "dcll_conv_lif_backward", "w3": "dcll_conv_lif_backward_w3_ex"}[entry]
    tail = {"ex": (C.PATHS[c["path"]], c["bands"], flags), "plain": (), "w3": (2,)}[entry]
    part_rows = None
    with ops.kernel_trace() as tr:
        if open_form:
            part, nc = ctypes.c_void_p(), ctypes.c_int32(-1)
            rc = getattr(lib, name + "_open")(*head, ptr(o("d_outW")), ptr(o("d_outb")), ptr(scratch), n, B, ctypes.byref(part),
                                              ctypes.byref(nc), *tail, stream_ptr())
            assert rc == 0, lib.dcll_last_error()
            assert part.value == scratch.data_ptr() + 4 * nconv and 1 <= nc.value and nconv + nc.value * c["c_out"] * rl <= n
            torch.cuda.synchronize()
            part_rows = scratch[nconv:nconv + nc.value * c["c_out"] * rl].clone()
            ops.grad_reduce_adam([dict(part=part.value, nchunk=nc.value, c_out=c["c_out"], rowlen=rl,
                                       dW=o("dW").view(c["c_out"], -1), db=o("db"))], [])
        else:
            rc = getattr(lib, name)(*head, ptr(o("dW")), ptr(o("db")), ptr(o("d_outW")), ptr(o("d_outb")), ptr(scratch), n, B, *tail,
                                    stream_ptr())
            assert rc == 0, lib.dcll_last_error()
        torch.cuda.synchronize()
    assert _intact(sbuf, so, n), "written outside the scratch"
    for k, (buf, view) in outs.items():
        assert _intact(buf, 0, view.numel()), "written behind %s" % k
    res = {k: view.clone() for k, (buf, view) in outs.items()}
    res.update(dv=scratch[:nconv].clone(), part=part_rows, names=list(tr.names))
    return res


def expected_log(c, parent_names):
    """the unflagged log with its one dv launch replaced by the predicted entry (unserved: unchanged)"""
    assert parent_names[0] == "k_bwd_dv" and sum(n.startswith("k_bwd_dv") for n in parent_names) == 1, parent_names
    return [C.form_name(c)] + parent_names[1:]


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
    from snn_modulation_classification_amd import ops
    c, cid = case, case["id"]
    print(C.describe(c))
    T = C.draw(c)
    X = _tensors(c, T, dev)
    assert ops.bwd_dv_pool_supported(conv_desc(c), c["B"]) == C.served(c)
    keys = ("dv", "dW", "db") + (("d_outW", "d_outb") if c["output_layer"] else ())
    parent = backward(c, X, dev, 0)
    res = backward(c, X, dev, C.POOL_DV)
    print("kernels:", res["names"])
    assert res["names"] == expected_log(c, parent["names"]), (cid, res["names"], parent["names"])
    if C.served(c):
        assert "k_bwd_dv" not in res["names"] and res["names"].count("k_bwd_dv_pool") == 1
        SERVED[C.instance_key(c)] += 1
    else:
        assert c["target"] == 33 and res["names"][0] == "k_bwd_dv"
    assert not bool((res["dv"] == SENT).any()), "an element of the dv plane was left unwritten"
    for k in keys:
        assert bits_equal(res[k], parent[k]), (cid, k, "DCLL_BWD_POOL_DV against flags = 0")
    opened, opened_parent = backward(c, X, dev, C.POOL_DV, open_form=True), backward(c, X, dev, 0, open_form=True)
    assert opened["names"] == expected_log(c, opened_parent["names"]), (cid, opened["names"])
    for k in keys + ("part",):
        assert bits_equal(opened[k], opened_parent[k]), (cid, k, "open form against flags = 0")
    for k in ("dv", "dW", "db"):        # (d_outW: the two forms keep its batch chunks in different places and may split differently)
        assert bits_equal(opened[k], res[k]), (cid, k, "open form + dcll_grad_reduce_adam against the closed form")
    if c["path"] == "default":          # DCLL_BWD_DEFAULT with flags = 0 is dcll_conv_lif_backward itself
        for open_form, ex in ((False, parent), (True, opened_parent)):
            plain = backward(c, X, dev, 0, open_form=open_form, entry="plain")
            assert plain["names"] == ex["names"]
            for k in keys + (("part",) if open_form else ()):
                assert bits_equal(plain[k], ex[k]), (cid, k, "dcll_conv_lif_backward%s" % ("_open" if open_form else ""))
    if c["draw"] == "grid":
        assert_dv(res["dv"], C.reference(cid), cid)
    again, other = backward(c, X, dev, C.POOL_DV), backward(c, X, dev, C.POOL_DV, off=c["off"] ^ 31)
    assert other["names"] == res["names"]
    for k in keys:
        assert bits_equal(again[k], res[k]), (cid, "second run", k)
        assert bits_equal(other[k], res[k]), (cid, "other alignment", k)
    if (c["kh"], c["kw"], c["c_out"]) == (1, 3, 64):        # the radio geometry: k_bwd_dv_w3 serves it as well
        w3 = backward(c, X, dev, 0, entry="w3")
        assert w3["names"][0].startswith("k_bwd_dv_w3") and bits_equal(w3["dv"], res["dv"]), (cid, w3["names"])
    RAN.add(cid)


def test_every_instance_served_a_case():
    """a parity test is only worth its name if it ran the kernel it claims to cover (runs behind the cases above)"""
    assert RAN == {c["id"] for c in CASES}, sorted({c["id"] for c in CASES} - RAN)
    assert set(SERVED) == set(C.all_instances()), (set(C.all_instances()) - set(SERVED), dict(SERVED))
    lines = ["k_bwd_dv_pool: cases of tests/pool_dv_cases.py served per template instance <PH,PW,NP> (tests/test_gpu_pool_dv.py;",
             "one launch-log form, \"k_bwd_dv_pool\": scalar loads at every alignment).  %d cases, %d served, %d kept k_bwd_dv (target 33)."
             % (len(CASES), sum(SERVED.values()), len(CASES) - sum(SERVED.values())), ""]
    lines += ["%-24s %d" % (k, SERVED[k]) for k in C.all_instances()]
    try:
        with open(COUNTS, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:                                                         # (a read-only checkout: the counts are printed)
        pass
    print("\n".join(lines))


def test_refusals_come_with_an_empty_launch_log(dev):
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    lib = _lib.get()
    c = C.by_id(CASES[2]["id"])
    d = conv_desc(c)
    ch, cw, ph, pw = C.shape(c)
    B, n = 2, C.scratch_floats(dict(c, B=2))
    eps1, v = torch.rand(B, c["c_in"], c["h"], c["w"], device=dev), torch.randn(B, c["c_out"], ch, cw, device=dev)

    def call(open_form, path, bands, flags, B=B, null_part=False):
        dW, db = torch.full((c["c_out"], c["c_in"], c["kh"], c["kw"]), -7.25, device=dev), torch.full((c["c_out"],), -7.25, device=dev)
        scratch = torch.full((n + GUARD,), SENT, device=dev)
        part, nchunk = ctypes.c_void_p(), ctypes.c_int32(-1)
        head = (ctypes.byref(d), ptr(eps1), ptr(v), None, None, None, None, ptr(v), None)
        with ops.kernel_trace() as tr:
            if open_form:
                rc = lib.dcll_conv_lif_backward_ex_open(*head, None, None, ptr(scratch), n, B, None if null_part else ctypes.byref(part),
                                                        ctypes.byref(nchunk), path, bands, flags, stream_ptr())
            else:
                rc = lib.dcll_conv_lif_backward_ex(*head, ptr(dW), ptr(db), None, None, ptr(scratch), n, B, path, bands, flags, stream_ptr())
            torch.cuda.synchronize()
        assert tr.names == [], tr.names
        assert bool((dW == -7.25).all()) and bool((db == -7.25).all()) and bool((scratch == SENT).all()) and nchunk.value == -1
        return rc, lib.dcll_last_error().decode()
    for open_form in (False, True):
        for B_ in (2, 0, -1):           # (before B is looked at)
            for flags in (2, 3, 0x100):
                rc, msg = call(open_form, 0, 0, flags, B=B_)
                assert rc == _lib.DCLL_ERR_INVALID and "unknown flag bits" in msg, (flags, rc, msg)
            for path in (-1, 5, 99):
                rc, msg = call(open_form, path, 0, 1, B=B_)
                assert rc == _lib.DCLL_ERR_INVALID and "unknown path" in msg, (path, rc, msg)
            for path in (0, 1, 2, 3):
                rc, msg = call(open_form, path, 2, 1, B=B_)
                assert rc == _lib.DCLL_ERR_INVALID and "bands" in msg, (path, rc, msg)
        for flags in (0, 1):
            for path in range(5):
                assert call(open_form, path, 0, flags, B=0)[0] == _lib.DCLL_OK
            assert call(open_form, 0, 0, flags, B=-1)[0] == _lib.DCLL_ERR_INVALID
    rc, msg = call(True, 0, 0, 1, null_part=True)
    assert rc == _lib.DCLL_ERR_INVALID and "null part" in msg
    assert call(True, 0, 0, 1, B=0, null_part=True)[0] == _lib.DCLL_ERR_INVALID
    with pytest.raises(ValueError):
        ops.conv_lif_backward(d, eps1, v, None, None, None, None, v, None, want_out=False, w3_path=True, pool_dv=True)


def test_the_flag_on_a_layer_without_pooling_changes_nothing(dev):
    c = dict(C.by_id(CASES[2]["id"]), pool_h=1, pool_w=1, target=10, output_layer=0, gsel="both", with_gv=1, off=0)
    assert not C.served(c) and C.form_name(c) == "k_bwd_dv_nopool<16>"
    X = _tensors(c, C.draw(c), dev)
    a, b = backward(c, X, dev, 0), backward(c, X, dev, C.POOL_DV)
    assert a["names"] == b["names"] and a["names"][0] == "k_bwd_dv_nopool<16>"
    for k in ("dv", "dW", "db"):
        assert bits_equal(a[k], b[k]), k


def test_the_served_predicate_is_the_restated_one(dev):
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()

    def lib_served(c, B):
        return int(lib.dcll_bwd_dv_pool_served(ctypes.byref(ops.make_conv_desc(
            c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]), (c["pool_h"], c["pool_w"]),
            c["target"], 0, 0, 1.0, .65, 1, 1, 1)), B))
    for c in CASES:
        assert lib_served(c, c["B"]) == int(C.served(c)), c["id"]
    c = C.by_id(CASES[0]["id"])
    tiny = dict(c, pool_h=1, pool_w=2, h=1, w=2)
    for probe, B in ((dict(c, target=32), 1), (dict(c, target=33), 1), (dict(c, pool_h=1, pool_w=1), 1), (dict(c, pool_h=4, h=4), 1),
                     (dict(c, pool_w=4, w=4), 1), (dict(c, pool_h=3, h=2), 1), (dict(c, pool_h=3, h=3), 1), (dict(c, pool_w=3, w=2), 1),
                     (c, C.PER_BLOCK * C.MAX_CHUNKS), (c, C.PER_BLOCK * C.MAX_CHUNKS + 1), (c, 0),
                     (dict(tiny, c_out=(2 ** 31 - 13) // 2), 1), (dict(tiny, c_out=(2 ** 31 - 13) // 2 + 1), 1)):
        assert lib_served(probe, B) == int(C.served(probe, B)), (probe, B)
    assert int(lib.dcll_bwd_dv_pool_served(None, 1)) == _lib.DCLL_ERR_INVALID
    bad = conv_desc(c)
    bad.pool_h = 0
    assert int(lib.dcll_bwd_dv_pool_served(ctypes.byref(bad), 1)) == _lib.DCLL_ERR_INVALID
    with pytest.raises(Exception):
        ops.bwd_dv_pool_supported(bad)


# ------------------------------------------------------------------------------------------------------------------------------
# network level: mnist_conv.yaml (pooling 2 / 1 / 2) at B = 8
# ------------------------------------------------------------------------------------------------------------------------------
HW, TARGET = (28, 28), 10
ARMS = {"default": (1.0, ()), "any": (1.0, ("any_learning_path", "any_step_path")), "wide": (2.0, ("wide_learning_path", "wide_step_path"))}


def _net(B, burnin, arm="default", dv=False, graph=False, spec="mnist_conv.yaml", hw=HW, target=TARGET, arp=0.0):
    netscale, switches = ARMS[arm]
    net = BWT._net(BWT._spec(spec), hw, B, target, burnin, arp, graph, netscale=netscale)
    for s in switches:
        setattr(net, s, True)
        assert getattr(net, s) is True
    assert net.pool_dv_path is False and not any(s.pool_dv for s in net.dcll_slices)
    if dv:
        net.pool_dv_path = True
        assert net.pool_dv_path is True and all(s.pool_dv for s in net.dcll_slices) and all(getattr(net, s) is True for s in switches)
    return net


def _inputs(rng, B, n, dev, hw=HW):
    return [torch.from_numpy((rng.uniform(size=(B, 1) + hw) < .15).astype(np.float32)).to(dev) for _ in range(n)]


def _label(rng, B, dev, target=TARGET):
    y = torch.zeros(B, target)
    y[np.arange(B), rng.randint(0, target, size=B)] = 1
    return y.to(dev)


def _swap(names):
    return ["k_bwd_dv_pool" if n == "k_bwd_dv" else n for n in names]


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


@pytest.mark.parametrize("arm", list(ARMS))
def test_network_six_learning_steps_are_bit_identical(dev, arm):
    """Two identically seeded networks on the same paths, Bn with pool_dv_path as well; before every step Bn takes A's parameters,
    optimizer state and neuron state; then both learn: spikes, every gradient, Adam's state and the parameters are bit-identical over
    six learning steps; Bn's log is A's with the two pooling layers' k_bwd_dv replaced by k_bwd_dv_pool (the layer without pooling keeps
    k_bwd_dv_nopool)."""
    from snn_modulation_classification_amd import ops
    B, burnin, steps = 8, 3, 6
    A, Bn = _net(B, burnin, arm), _net(B, burnin, arm, dv=True)
    rng = np.random.RandomState(12)
    y = _label(rng, B, dev)
    for t in range(burnin - 1 + steps):
        x = _inputs(rng, B, 1, dev)[0]
        BWT._copy_everything(A, Bn)
        logs = []
        for net in (A, Bn):
            with ops.kernel_trace() as tr:
                net.learn(x, y)
                torch.cuda.synchronize()
            logs.append(list(tr.names))
        learning = t >= burnin - 1
        # (the default path at this batch launches its slices' backward calls together behind the tails, pool_dv_path each slice's at
        # once: the same launches in another order on the one stream; the other arms launch at once either way)
        same = sorted(logs[1]) == sorted(_swap(logs[0])) if arm == "default" else logs[1] == _swap(logs[0])
        assert same, (t, logs[0], logs[1])
        assert logs[0].count("k_bwd_dv") == (2 if learning else 0) and logs[1].count("k_bwd_dv_pool") == (2 if learning else 0)
        assert "k_bwd_dv_pool" not in logs[0] and "k_bwd_dv" not in logs[1]
        assert sum(n.startswith("k_bwd_dv_nopool") for n in logs[1]) == (1 if learning else 0), logs[1]
        for sa, sb in zip(A.dcll_slices, Bn.dcll_slices):
            for key in ("s", "p", "pv"):
                if torch.is_tensor(sa._learn_bufs.get(key)):
                    assert torch.equal(sa._learn_bufs[key], sb._learn_bufs[key]), (t, key)
        _assert_same_networks(A, Bn)
        if learning:
            assert all(float(s.dclllayer.i2h.weight.grad.abs().max()) > 0 for s in Bn.dcll_slices)


def test_graph_captured_learning_steps_equal_eager_steps(dev):
    """With pool_dv_path the learning timestep replayed from its captured graph == the step launched eagerly, bit for bit, at B = 8;
    toggling the attribute changes the signature"""
    B, T, burnin = 8, 16, 4
    rng = np.random.RandomState(5)
    xs, y = _inputs(rng, B, T, dev), _label(rng, B, dev)
    nets = {}
    for graph in (True, False):
        net = nets[graph] = _net(B, burnin, "any", dv=True, graph=graph)
        for x in xs:
            net.learn(x, y)
        torch.cuda.synchronize()
    a, b = nets[True], nets[False]
    g = a._learn_graphs[((B, 1) + HW, (B, TARGET))]
    assert g["n"] >= 6 and not b._learn_graphs, (g["n"],)
    _assert_same_networks(a, b)
    sig = a._graph_signature()
    a.pool_dv_path = False
    assert a._graph_signature() != sig and a.any_learning_path is True


def test_learn_sequence_equals_per_step_learning(dev):
    """ConvNetwork.learn_sequence with pool_dv_path == the loop `for t: net.learn(x[t], y)` with it: weights, Adam state and clout bit
    for bit; two k_bwd_dv_pool per learning step, no k_bwd_dv"""
    from snn_modulation_classification_amd import ops
    B, T, burnin = 4, 9, 5
    rng = np.random.RandomState(6)
    cells = rng.randint(0, HW[0] * HW[1], size=(T, B)).astype(np.int32)
    y = _label(rng, B, dev)
    a, b = _net(B, burnin, dv=True), _net(B, burnin, dv=True)
    with ops.kernel_trace() as tr:
        a.learn_sequence(torch.from_numpy(cells).to(dev), y)
        torch.cuda.synchronize()
    n_learn = T - burnin + 1
    assert tr.names.count("k_bwd_dv_pool") == 2 * n_learn and tr.names.count("k_bwd_dv") == 0, tr.names
    x = np.zeros((T, B, HW[0] * HW[1]), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    x = torch.from_numpy(x.reshape(T, B, 1, *HW)).to(dev)
    for t in range(T):
        b.learn(x[t], y)
    _assert_same_networks(a, b)


def test_the_rank_sharded_step_runs_with_the_dv_kernel(dev, monkeypatch):
    """The step ConvNetwork.learn takes under ranks (the CLOSED backward per slice: dcll_conv_lif_backward_ex + k_bwd_reduce, then
    ops.adam_step) with the collective of a one-rank world == the single-process step (open form + dcll_grad_reduce_adam), bit for bit"""
    from snn_modulation_classification_amd import ops, parallel
    B, T, burnin = 3, 5, 3
    rng = np.random.RandomState(9)
    xs, y = _inputs(rng, B, T, dev), _label(rng, B, dev)
    a, b = _net(B, burnin, dv=True), _net(B, burnin, dv=True)
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
    assert tr.names.count("k_bwd_dv_pool") == 2 * n_learn and tr.names.count("k_bwd_dv") == 0, tr.names
    assert sum(n.startswith("k_bwd_reduce") for n in tr.names) == 3 * n_learn and tr.count("k_grad_reduce_adam") == 0, tr.names
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for sl_a, sl_b in zip(a.dcll_slices, b.dcll_slices):
        for pa, pb in zip(sl_a.dclllayer.parameters(), sl_b.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad))


def test_the_setter_refuses_under_the_w3_path(dev):
    from snn_modulation_classification_amd import _lib
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    assert DCLLBase.pool_dv is False
    net = W._net(2, learn=True)                    # radio_ml_conv_ref.yaml on the (16,128) plane
    net.pool_dv_path = True                         # (without w3_step_path: allowed, its (1,2) layers are served)
    assert net.pool_dv_path is True
    with pytest.raises(_lib.DCLLUnsupported):
        net.w3_step_path = True
    assert net.w3_step_path is False and net.pool_dv_path is True
    net.pool_dv_path = False
    net.w3_step_path = True
    with pytest.raises(_lib.DCLLUnsupported):
        net.pool_dv_path = True
    assert net.pool_dv_path is False and not any(s.pool_dv for s in net.dcll_slices) and net.w3_step_path is True
    net.pool_dv_path = False                        # switching it off is always allowed


def test_a_network_without_pooling_is_unchanged(dev):
    """radio_ml_conv.yaml (no pooling) with the setter on: the same launch log and the same bits as without it"""
    from snn_modulation_classification_amd import ops
    B, burnin, T = 4, 3, 6
    kw = dict(spec="radio_ml_conv.yaml", hw=(16, 16), target=24, arp=1.0)
    A, Bn = _net(B, burnin, **kw), _net(B, burnin, dv=True, **kw)
    rng = np.random.RandomState(3)
    xs, y = _inputs(rng, B, T, dev, (16, 16)), _label(rng, B, dev, 24)
    logs = []
    for net in (A, Bn):
        with ops.kernel_trace() as tr:
            for x in xs:
                net.learn(x, y)
            torch.cuda.synchronize()
        logs.append(list(tr.names))
    assert logs[0] == logs[1] and not any(n.startswith("k_bwd_dv_pool") for n in logs[1]) and any(n.startswith("k_bwd_dv") for n in logs[1])
    _assert_same_networks(A, Bn)


def test_entry_point_train_pool_dv_path(tmp_path, capsys):
    """train.py --data MNIST --pool_dv_path prints the losses and accuracies of the same command without the flag and runs the
    pooling layers' dv on k_bwd_dv_pool; on radio_ml_conv.yaml (no pooling) and under --w3_step_path it is ignored with a notice"""
    import re
    import train
    common = ['--data', 'MNIST', '--network_spec', os.path.join(PKG, 'networks', 'mnist_conv.yaml'), '--synthetic', '16',
              '--batch_size', '8', '--batch_size_test', '8', '--n_test_samples', '8', '--n_steps', '2', '--n_iters', '10',
              '--n_iters_test', '10', '--burnin', '4', '--n_test_interval', '1', '--learning_rates', '1e-7']
    runs = {}
    for name, flags in (("off", []), ("on", ['--pool_dv_path'])):
        with W._trace() as tr:
            out = train.main(common + ['--output', str(tmp_path / name)] + flags)
        text = capsys.readouterr().out
        runs[name] = (np.load(os.path.join(out, 'acc_test.npy')), list(tr.names), [l for l in text.splitlines() if l.startswith("[")])        # (the [TRAIN] / [TEST] lines: losses and accuracies)
    (a, names, text), (b, names_dv, text_dv) = runs["off"], runs["on"]
    assert "k_bwd_dv" in names and "k_bwd_dv_pool" not in names and np.isfinite(a).all()
    assert "k_bwd_dv_pool" in names_dv and "k_bwd_dv" not in names_dv and sorted(names_dv) == sorted(_swap(names))
    assert np.array_equal(a, b) and not any("ignored" in l for l in text_dv)
    strip = lambda lines: [re.sub(r"\d+\.\d+ ?s\b", "", l) for l in lines]          # (wall-clock figures, if any)
    assert text and strip(text) == strip(text_dv), (text, text_dv)
    radio = ['--I_resolution', '24', '--Q_resolution', '24', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
             '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '6', '--n_iters_test', '6',
             '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    with W._trace() as tr:
        train.main(radio + ['--output', str(tmp_path / 'radio'), '--pool_dv_path'])
    assert "--pool_dv_path ignored: no layer of this network pools" in capsys.readouterr().out and "k_bwd_dv_pool" not in tr.names
    ref = ['--I_resolution', '128', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
           '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '6', '--n_iters_test', '6',
           '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7',
           '--network_spec', os.path.join(PKG, 'networks', 'radio_ml_conv_ref.yaml')]
    with W._trace() as tr:
        train.main(ref + ['--output', str(tmp_path / 'ref'), '--w3_step_path', '--pool_dv_path'])
    assert "--pool_dv_path ignored: --w3_step_path is in effect" in capsys.readouterr().out and "k_bwd_dv_pool" not in tr.names
