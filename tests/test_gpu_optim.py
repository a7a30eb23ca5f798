"""GPU tests of the opt-in native learning step for SGD, Adamax, AdamW and amsgrad: dcll_optim_step / dcll_grad_reduce_optim
(k_optim_multi / k_grad_reduce_optim) on the cases of tests/optim_cases.py (proven on the CPU by tests/test_optim_cases.py) through
the C ABI, and through DCLLBase.native_optimizers / ConvNetwork.native_optim_path / train.py.

Kernel level: parameter and every state tensor after each of three steps are the bits of the float32 restatement, with dyn and
without; every buffer sits in front of a sentinel tail; the launch log is the predicted one; a second run gives the same bits; dW / db
are dcll_grad_reduce_adam's; kind ADAM without flags is dcll_adam_step / dcll_grad_reduce_adam; refusals come with code, message and
an empty log.  Network level: radio_ml_conv.yaml on 16x16 with SGD(momentum 0.9), Adamax, AdamW and Adam(amsgrad)."""
import os

import numpy as np
import pytest
import torch

import optim_cases as C
import test_gpu_bwd_wide as BWT     # its helpers (network arguments, spec loader); its tests are not re-exported here
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
CASES = C.cases()
GUARD, SENT = 64, -3.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def bits_equal(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


class Buf:
    """n floats in front of GUARD sentinel floats; `addr` is valid for n = 0 too (an empty torch view has no address)"""

    def __init__(self, arr, n, dev):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENT, device=dev)
        if arr is not None and n:
            self.buf[:n] = torch.from_numpy(np.ascontiguousarray(arr, np.float32).reshape(-1)).to(dev)
        self.addr = self.buf.data_ptr()

    def get(self):
        return self.buf[:self.n].clone()

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all())


def _device_case(c, X, dev):
    """the case's tensors on the device: per tensor param / grad / state buffers, per layer part / dW / db"""
    D = dict(t=[], l=[])
    for t, T in zip(c["tensors"], X["tensors"]):
        D["t"].append(dict(param=Buf(T["param"], t["n"], dev), grad=Buf(None, t["n"], dev),
                           s=[None if s is None else Buf(s, t["n"], dev) for s in T["s"]]))
    for L in c["layers"]:
        D["l"].append(dict(part=Buf(None, L["nchunk"] * L["c_out"] * L["rowlen"], dev), dW=Buf(None, L["c_out"] * (L["rowlen"] - 1), dev),
                           db=Buf(None, L["c_out"], dev) if L["db"] else None))
    ref = C.referred(c)
    for k, (l, key) in ref.items():             # a referred tensor's gradient IS the layer's dW / db
        D["t"][k]["grad"] = D["l"][l][key]
    return D


def _all_bufs(D):
    for t in D["t"]:
        yield from [t["param"], t["grad"]] + [s for s in t["s"] if s is not None]
    for L in D["l"]:
        yield from [b for b in (L["part"], L["dW"], L["db"]) if b is not None]


def _structs(c, D, q, dyn):
    from snn_modulation_classification_amd import _lib
    arr = (_lib.OptimTensor * max(1, len(c["tensors"])))()
    for a, t, d in zip(arr, c["tensors"], D["t"]):
        a.param, a.grad = d["param"].addr, d["grad"].addr
        a.s0, a.s1, a.s2 = (None if s is None else s.addr for s in d["s"])
        a.n, a.kind, a.flags = t["n"], t["kind"], t["flags"] | (C.FIRST if C.first_flag(c, t, q) else 0)
        a.step, a.lr = (1, 123.0) if dyn else (c["step"] + q, t["lr"])          # (with dyn both are ignored)
        a.weight_decay, a.h0, a.h1, a.eps = t["weight_decay"], t["h0"], t["h1"], t["eps"]
    larr = (_lib.GradParts * max(1, len(c["layers"])))()
    for a, L, d in zip(larr, c["layers"], D["l"]):
        a.part, a.dW, a.db = d["part"].addr, d["dW"].addr, None if d["db"] is None else d["db"].addr
        a.rowlen, a.nchunk, a.c_out, a.adam_w, a.adam_b = L["rowlen"], L["nchunk"], L["c_out"], L["adam_w"], L["adam_b"]
    return arr, larr


def run_case(c, X, dev, dyn):
    """the case's three steps through the C ABI -> per step (per tensor (param, [s0, s1, s2]), per layer (dW, db)); asserts the log and
    the sentinels"""
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import ptr, stream_ptr
    lib = _lib.get()
    D = _device_case(c, X, dev)
    ref = C.referred(c)
    out = []
    for q in range(C.NSTEPS):
        for k, (T, d) in enumerate(zip(X["tensors"], D["t"])):
            if k not in ref and d["grad"].n:
                d["grad"].buf[:d["grad"].n] = torch.from_numpy(T["grads"][q]).to(dev)
        for P, d in zip(X["parts"], D["l"]):
            d["part"].buf[:d["part"].n] = torch.from_numpy(P[q].reshape(-1)).to(dev)
        arr, larr = _structs(c, D, q, dyn)
        dv = None
        if dyn:
            vals = ops.optim_dyn_values([dict(t, step=c["step"] + q) for t in c["tensors"]])
            assert [np.float32(v) for v in vals] == [v for t in c["tensors"] for v in C.host_values(t, c["step"] + q)]
            dv = torch.tensor(vals + [SENT] * GUARD, dtype=torch.float32, device=dev)
        with ops.kernel_trace() as tr:
            if c["call"] == "step":
                rc = lib.dcll_optim_step(arr, len(c["tensors"]), ptr(dv), stream_ptr())
            else:
                rc = lib.dcll_grad_reduce_optim(larr, len(c["layers"]), arr, len(c["tensors"]), ptr(dv), stream_ptr())
            torch.cuda.synchronize()
        assert rc == 0, lib.dcll_last_error()
        assert list(tr.names) == C.expected_log(c), (c["id"], tr.names)
        assert all(b.intact() for b in _all_bufs(D)), "written behind a buffer"
        out.append(([(d["param"].get(), [None if s is None else s.get() for s in d["s"]]) for d in D["t"]],
                    [(d["dW"].get(), None if d["db"] is None else d["db"].get()) for d in D["l"]]))
    return out


def reduce_adam_reference(c, X, dev, q):
    """dW / db of dcll_grad_reduce_adam without tensors: the kernel this project ships, the reference"""
    from snn_modulation_classification_amd import _lib
    from snn_modulation_classification_amd._lib import stream_ptr
    lib = _lib.get()
    D = _device_case(dict(c, tensors=[], layers=[dict(L, adam_w=-1, adam_b=-1) for L in c["layers"]]), dict(tensors=[], parts=X["parts"]), dev)
    for P, d in zip(X["parts"], D["l"]):
        d["part"].buf[:d["part"].n] = torch.from_numpy(P[q].reshape(-1)).to(dev)
    _, larr = _structs(dict(c, tensors=[], layers=[dict(L, adam_w=-1, adam_b=-1) for L in c["layers"]]), D, q, False)
    rc = lib.dcll_grad_reduce_adam(larr, len(c["layers"]), None, 0, None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.dcll_last_error()
    return [(d["dW"].get(), None if d["db"] is None else d["db"].get()) for d in D["l"]]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_gives_the_bits_of_the_restatement(dev, case):
    c = case
    X = C.draw(c)
    want = C.trajectory(c, X)
    runs = {dyn: run_case(c, X, dev, dyn) for dyn in (False, True)}
    again = run_case(c, X, dev, False)
    for q in range(C.NSTEPS):
        red = reduce_adam_reference(c, X, dev, q) if c["layers"] else []
        for name, got in (("host scalars", runs[False]), ("dyn", runs[True]), ("second run", again)):
            tensors, layers = got[q]
            for k, ((p, s), (wp, ws)) in enumerate(zip(tensors, want[q])):
                assert bits_equal(p, wp), (c["id"], name, q, k, "param", C.KIND_NAMES[c["tensors"][k]["kind"]])
                for j, (a, b) in enumerate(zip(s, ws)):
                    assert (a is None) == (b is None) and (a is None or bits_equal(a, b)), (c["id"], name, q, k, "s%d" % j)
            for l, ((dW, db), (rW, rb), P) in enumerate(zip(layers, red, X["parts"])):
                assert bits_equal(dW, rW) and (db is None or bits_equal(db, rb)), (c["id"], name, q, l, "dW / db against dcll_grad_reduce_adam")
                fW, fb = C.reduce_f32(P[q])
                assert bits_equal(dW, fW) and (db is None or bits_equal(db, fb)), (c["id"], name, q, l, "dW / db against reduce_f32")


def _torch_tensors(cfgs, sizes, dev, seed, step):
    """ops.optim_step's dicts (kind ADAM, no flags) and ops.adam_step's dicts on separate copies of the same values"""
    rs = np.random.RandomState(seed)
    gen, adam = [], []
    for cfg, n in zip(cfgs, sizes):
        vals = dict(param=rs.randn(n) * 0.05, grad=rs.randn(n) * 0.3, m=rs.randn(n) * 0.01, v=np.abs(rs.randn(n)) * 1e-3)
        a = {k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in vals.items()}
        b = {k: v.clone() for k, v in a.items()}
        gen.append(dict(param=a["param"], grad=a["grad"], s0=a["m"], s1=a["v"], s2=None, kind=C.ADAM, flags=0, lr=cfg["lr"],
                        weight_decay=cfg["weight_decay"], h0=cfg["h0"], h1=cfg["h1"], eps=cfg["eps"], step=step))
        adam.append(dict(param=b["param"], grad=b["grad"], exp_avg=b["m"], exp_avg_sq=b["v"], lr=cfg["lr"], weight_decay=cfg["weight_decay"],
                         beta1=cfg["h0"], beta2=cfg["h1"], eps=cfg["eps"], step=step))
    return gen, adam


@pytest.mark.parametrize("dyn", [False, True])
def test_kind_adam_without_flags_is_dcll_adam_step_and_dcll_grad_reduce_adam(dev, dyn):
    from snn_modulation_classification_amd import ops
    cfgs = [C.CONFIGS[0], dict(C.CONFIGS[1], flags=0), C.CONFIGS[0], dict(C.CONFIGS[1], flags=0, weight_decay=10.0)]
    sizes = [7 * 8, 7, 1025, 257]
    for step in (1, 12):
        gen, adam = _torch_tensors(cfgs, sizes, dev, step, step)
        d4 = torch.tensor(ops.optim_dyn_values(gen), dtype=torch.float32, device=dev) if dyn else None
        d3 = torch.tensor(ops.adam_dyn_values(adam), dtype=torch.float32, device=dev) if dyn else None
        with ops.kernel_trace() as tr:
            ops.optim_step(gen, dyn=d4)
            ops.adam_step(adam, dyn=d3)
            torch.cuda.synchronize()
        assert list(tr.names) == ["k_optim_multi", "k_adam_multi"]
        part = torch.randn(16, 7, 9, device=dev)
        layers = []
        for ts in (gen, adam):
            L = dict(part=part.data_ptr(), nchunk=16, c_out=7, rowlen=9, dW=ts[0]["grad"].view(7, 8), db=ts[1]["grad"], adam_w=0, adam_b=1)
            layers.append(L)
        with ops.kernel_trace() as tr:
            ops.grad_reduce_optim([layers[0]], gen, dyn=d4)
            ops.grad_reduce_adam([layers[1]], adam, dyn=d3)
            torch.cuda.synchronize()
        assert list(tr.names) == ["k_grad_reduce_optim", "k_grad_reduce_adam"]
        for a, b in zip(gen, adam):
            for ka, kb in (("param", "param"), ("s0", "exp_avg"), ("s1", "exp_avg_sq"), ("grad", "grad")):
                assert bits_equal(a[ka], b[kb]), (step, ka)


def test_refusals_come_with_code_message_and_an_empty_log(dev):
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd._lib import stream_ptr
    lib = _lib.get()
    cfg = lambda k: dict(C.CONFIGS[k])
    base = dict(id="refusal", call="reduce", seed=1, step=2,
                tensors=[dict(cfg(1), n=56), dict(cfg(5), n=7), dict(cfg(7), n=64), dict(cfg(0), n=8)],
                layers=[dict(c_out=7, rowlen=9, nchunk=4, db=True, adam_w=0, adam_b=1), dict(c_out=8, rowlen=9, nchunk=4, db=True, adam_w=2, adam_b=3)])
    X = C.draw(base)
    seen = set()
    for rid, what, word in C.REFUSALS:
        c = dict(base, tensors=[dict(t) for t in base["tensors"]], layers=[dict(L) for L in base["layers"]])
        D = _device_case(c, X, dev)
        n_t, n_l, null = len(c["tensors"]), len(c["layers"]), None
        if rid == "kind-4":
            c["tensors"][0]["kind"] = 4
        elif rid == "kind-neg":
            c["tensors"][3]["kind"] = -1
        elif rid == "flag-8":
            c["tensors"][0]["flags"] |= 8
        elif rid == "nesterov-adam":
            c["tensors"][3]["flags"] = C.NESTEROV
        elif rid == "amsgrad-adamax":
            c["tensors"][1]["flags"] = C.AMSGRAD
        elif rid == "first-no-momentum":
            c["tensors"][2].update(h0=0.0, flags=C.FIRST)
        elif rid == "step-0":
            c["step"] = 0
        elif rid == "nine-tensors":
            n_t = 9
        elif rid == "five-layers":
            n_l = 5
        elif rid == "twice":
            c["layers"][1]["adam_b"] = 0
        elif rid == "w-size":
            c["layers"][0]["rowlen"] = 10
        elif rid == "b-size":
            c["tensors"][1]["n"] = 8
        elif rid == "index":
            c["layers"][0]["adam_w"] = 4
        arr, larr = _structs(c, D, 0, False)
        if rid == "no-s0-adam":
            arr[0].s0 = None
        elif rid == "no-s1-adamax":
            arr[1].s1 = None
        elif rid == "no-s2-amsgrad":
            arr[0].s2 = None
        elif rid == "no-s0-momentum":
            arr[2].s0 = None
        elif rid == "null-param":
            arr[3].param = None
        if n_t == 9:
            big = (_lib.OptimTensor * 9)()
            for i in range(9):
                big[i] = arr[i % 4]
            arr = big
        if n_l == 5:
            big = (_lib.GradParts * 5)()
            for i in range(5):
                big[i] = larr[i % 2]
            larr = big
        before = [b.buf.clone() for b in _all_bufs(D)]
        calls = [("reduce", lambda: lib.dcll_grad_reduce_optim(larr, n_l, arr, n_t, null, stream_ptr()))]
        if rid not in ("five-layers", "twice", "w-size", "b-size", "index"):        # (the struct array's refusals: dcll_optim_step too)
            calls.append(("step", lambda: lib.dcll_optim_step(arr, n_t, null, stream_ptr())))
        for name, call in calls:
            with ops.kernel_trace() as tr:
                rc = call()
                torch.cuda.synchronize()
            msg = lib.dcll_last_error().decode()
            assert rc == _lib.DCLL_ERR_INVALID and word in msg, (rid, name, rc, msg)
            assert list(tr.names) == [], (rid, tr.names)
            assert all(torch.equal(a, b.buf) for a, b in zip(before, _all_bufs(D))), rid
        seen.add(rid)
    assert seen == {r[0] for r in C.REFUSALS}
    with ops.kernel_trace() as tr:
        assert lib.dcll_optim_step(None, 0, None, stream_ptr()) == 0 and lib.dcll_grad_reduce_optim(None, 0, None, 0, None, stream_ptr()) == 0
        assert lib.dcll_optim_step(None, 1, None, stream_ptr()) == _lib.DCLL_ERR_INVALID
        assert lib.dcll_grad_reduce_optim(None, 1, None, 0, None, stream_ptr()) == _lib.DCLL_ERR_INVALID
    assert list(tr.names) == []
    with pytest.raises(ValueError):
        ops.grad_reduce_optim([{}] * 5, [])


# ------------------------------------------------------------------------------------------------------------------------------
# network level: radio_ml_conv.yaml on 16x16, B = 4, T = 9, burnin 3
# ------------------------------------------------------------------------------------------------------------------------------
HW, TARGET, B, T, BURNIN = (16, 16), 24, 4, 9, 3
OPTS = {"sgd": (torch.optim.SGD, dict(momentum=0.9)), "adamax": (torch.optim.Adamax, dict(betas=[0.0, .95], weight_decay=10.0)),
        "adamw": (torch.optim.AdamW, dict(betas=[0.0, .95], weight_decay=10.0)),
        "amsgrad": (torch.optim.Adam, dict(betas=[0.0, .95], weight_decay=10.0, amsgrad=True))}
LR = {"sgd": 1e-3, "adamax": 1e-6, "adamw": 1e-6, "amsgrad": 1e-6}


def _net(opt, on=True, graph=False, spec="radio_ml_conv.yaml", hw=HW, B=B, opt_param=None, cls=None):
    from snn_modulation_classification_amd.networks import ConvNetwork
    torch.manual_seed(1)
    np.random.seed(1)
    cls_, kw = OPTS[opt] if cls is None else (cls, opt_param)
    net = ConvNetwork(BWT._args(arp=1.0, netscale=1.0), (1,) + tuple(hw), B, BWT._spec(spec), TARGET, act=torch.nn.Sigmoid(),
                      loss=torch.nn.SmoothL1Loss, opt=cls_, opt_param=dict(kw), learning_rates=[LR.get(opt, 1e-6)], burnin=BURNIN)
    net.graph_learn = graph
    net.reset(True)
    net.train()
    assert net.native_optim_path is (os.environ.get("DCLL_NATIVE_OPTIM", "0") == "1")     # (read at construction)
    if on:
        net.native_optim_path = True
        assert net.native_optim_path is True and all(s.native_optimizers for s in net.dcll_slices)
    return net


def _data(dev, hw=HW, B=B, seed=5):
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, hw[0] * hw[1], size=(T, B)).astype(np.int32)
    x = np.zeros((T, B, hw[0] * hw[1]), np.float32)
    x[np.arange(T)[:, None], np.arange(B)[None, :], cells] = 1
    y = torch.zeros(B, TARGET)
    y[np.arange(B), rng.randint(0, TARGET, size=B)] = 1
    return torch.from_numpy(cells).to(dev), torch.from_numpy(x.reshape(T, B, 1, *hw)).to(dev), y.to(dev)


def _optimizers(s):
    return [s.optimizer] + ([s.optimizer2] if s.dclllayer.output_layer else [])


def _snapshot(net):
    """per optimizer, per parameter: (param, state tensors by name, step) on the host"""
    out = []
    for s in net.dcll_slices:
        for o in _optimizers(s):
            for q in o.param_groups[0]["params"]:
                st = o.state.get(q, {})
                out.append((q.detach().cpu().numpy().copy(), {k: v.detach().cpu().numpy().copy() for k, v in st.items() if torch.is_tensor(v) and v.dim()},
                            int(st["step"]) if "step" in st else None))
    return out


def _assert_same(a, b, what):
    sa, sb = _snapshot(a), _snapshot(b)
    assert len(sa) == len(sb)
    for (pa, ta, na), (pb, tb, nb) in zip(sa, sb):
        assert bits_equal(pa, pb) and na == nb and set(ta) == set(tb), what
        for k in ta:
            assert bits_equal(ta[k], tb[k]), (what, k)
    for x, y in zip(a.dcll_slices, b.dcll_slices):
        assert x.iter == y.iter and np.array_equal(np.asarray(x.clout), np.asarray(y.clout)), what
        for pa, pb in zip(x.dclllayer.parameters(), y.dclllayer.parameters()):
            assert (pa.grad is None) == (pb.grad is None) and (pa.grad is None or torch.equal(pa.grad, pb.grad)), what


def _config_of(o, g):
    """the restatement's tensor configuration of a torch optimizer's param group"""
    if type(o) is torch.optim.SGD:
        return dict(kind=C.SGD, flags=C.NESTEROV if g["nesterov"] else 0, lr=g["lr"], weight_decay=g["weight_decay"], h0=g["momentum"],
                    h1=g["dampening"], eps=0.0)
    kind = C.ADAMAX if type(o) is torch.optim.Adamax else C.ADAMW if type(o) is torch.optim.AdamW else C.ADAM
    return dict(kind=kind, flags=C.AMSGRAD if g.get("amsgrad") else 0, lr=g["lr"], weight_decay=g["weight_decay"], h0=g["betas"][0],
                h1=g["betas"][1], eps=g["eps"])


STATE_NAMES = {C.SGD: ["momentum_buffer"], C.ADAM: ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"], C.ADAMW: ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"],
               C.ADAMAX: ["exp_avg", "exp_inf"]}


@pytest.mark.parametrize("opt", list(OPTS))
def test_served_with_the_switch_on_and_every_step_is_the_restatement(dev, opt):
    """The slices are served natively with the switch on and not with it off; after every native step each parameter and state tensor is
    the restatement applied to the previous values and to the .grad the step left, bit for bit; the update went out in one
    k_grad_reduce_optim launch and no torch optimizer ran; `step` counts the updates."""
    from snn_modulation_classification_amd import ops
    off = _net(opt, on=False)
    assert all(s._native_learning() is None for s in off.dcll_slices)
    net = _net(opt)
    assert all(s._native_learning() is not None for s in net.dcll_slices)
    net.native_optim_path = False
    assert all(s._native_learning() is None for s in net.dcll_slices)          # (the cached kind follows the switch)
    net.native_optim_path = True
    assert all(s._native_learning() is not None for s in net.dcll_slices)
    _, xs, y = _data(dev)
    n_upd = 0
    for t in range(T):
        before = _snapshot(net)
        with ops.kernel_trace() as tr:
            net.learn(xs[t], y)
            torch.cuda.synchronize()
        if t < BURNIN - 1:
            assert "k_grad_reduce_optim" not in tr.names
            continue
        n_upd += 1
        assert tr.names.count("k_grad_reduce_optim") == 1 and "k_grad_reduce_adam" not in tr.names and "k_adam_multi" not in tr.names, tr.names
        after, i = _snapshot(net), 0
        for s in net.dcll_slices:
            for o in _optimizers(s):
                g = o.param_groups[0]
                cfg = _config_of(o, g)
                for q in g["params"]:
                    p0, st0, _ = before[i]
                    p1, st1, step = after[i]
                    i += 1
                    if q.grad is None:              # (a parameter the step does not train: untouched, no state)
                        assert bits_equal(p1, p0) and not st1
                        continue
                    names = STATE_NAMES[cfg["kind"]]
                    have = cfg["kind"] != C.SGD or cfg["h0"] != 0
                    s0 = [st0.get(n, np.zeros_like(p0) if (have and (n != "max_exp_avg_sq" or cfg["flags"] & C.AMSGRAD)) else None) for n in names]
                    s0 += [None] * (3 - len(s0))
                    first = cfg["kind"] == C.SGD and cfg["h0"] != 0 and n_upd == 1
                    wp, ws = C.optim_f32(cfg, p0.reshape(-1), q.grad.detach().cpu().numpy().reshape(-1), [None if x is None else x.reshape(-1) for x in s0],
                                         n_upd, first=first)
                    assert bits_equal(p1, wp), (opt, t, s.name, "param")
                    assert float(q.grad.abs().max()) > 0, (opt, t, s.name, "an all-zero gradient: the comparison would show nothing")
                    assert cfg["weight_decay"] == 0 or not np.array_equal(p1, p0), (opt, t, s.name, "the step changed nothing")
                    assert step == (None if cfg["kind"] == C.SGD else n_upd)
                    for n, w in zip(names, ws):
                        assert (w is None) == (n not in st1), (opt, n)
                        if w is not None:
                            assert bits_equal(st1[n], w), (opt, t, s.name, n)
    assert n_upd == T - BURNIN + 1


@pytest.mark.parametrize("opt", list(OPTS))
def test_graph_replays_learn_sequence_and_the_rank_step_equal_eager_steps(dev, opt, monkeypatch):
    """Captured-graph replays == eager steps bit for bit (at least two replays happened); learn_sequence == the per-step loop; the
    rank-sharded step (closed backward per slice, then ops.optim_step) with the collective of a one-rank world == the single-process
    step, bit for bit — the gate of the sibling paths' rank tests."""
    from snn_modulation_classification_amd import ops, parallel
    cells, xs, y = _data(dev)
    eager, graph, seq, rank = _net(opt), _net(opt, graph=True), _net(opt), _net(opt)
    for t in range(T):
        eager.learn(xs[t], y)
        graph.learn(xs[t], y)
    torch.cuda.synchronize()
    g = graph._learn_graphs[((B, 1) + HW, (B, TARGET))]
    assert g["n"] >= 2 and not eager._learn_graphs and g["dyn"].numel() == 4 * sum(len(s._optim_tensors(advance=False)) for s in graph.dcll_slices)
    _assert_same(eager, graph, "graph replays")
    seq.learn_sequence(cells, y)
    _assert_same(eager, seq, "learn_sequence")
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    monkeypatch.setattr(parallel, "allreduce_slab_begin", lambda slab, local_n, global_n=None: None)
    with ops.kernel_trace() as tr:
        for t in range(T):
            rank.learn(xs[t], y)
        torch.cuda.synchronize()
    monkeypatch.undo()
    n_learn = T - BURNIN + 1
    assert tr.names.count("k_optim_multi") == n_learn and tr.count("k_grad_reduce_optim") == 0 and tr.count("k_adam_multi") == 0, tr.names
    sa, sb = eager.state_dict(), rank.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for (pa, ta, na), (pb, tb, nb) in zip(_snapshot(eager), _snapshot(rank)):
        assert na == nb and all(bits_equal(ta[k], tb[k]) for k in ta)


@pytest.mark.parametrize("opt", list(OPTS))
def test_state_dict_is_what_the_torch_class_creates_and_loads_into_it(dev, opt):
    import inspect
    _, xs, y = _data(dev)
    net = _net(opt)
    for t in range(BURNIN + 1):
        net.learn(xs[t], y)
    torch.cuda.synchronize()
    for s in net.dcll_slices:
        for o in _optimizers(s):
            params = [torch.nn.Parameter(q.detach().clone()) for q in o.param_groups[0]["params"]]
            accepted = set(inspect.signature(type(o).__init__).parameters)
            kw = {k: v for k, v in o.param_groups[0].items() if k in accepted and k != "params"}
            fresh = type(o)(params, **kw)
            for q, orig in zip(params, o.param_groups[0]["params"]):
                q.grad = None if orig.grad is None else torch.ones_like(q)
            fresh.step()
            mine, theirs = o.state_dict(), fresh.state_dict()
            assert set(mine["state"]) == set(theirs["state"])
            for i in theirs["state"]:
                assert set(mine["state"][i]) == set(theirs["state"][i]), (opt, s.name)
                for k, v in theirs["state"][i].items():
                    w = mine["state"][i][k]
                    assert torch.is_tensor(w) == torch.is_tensor(v) and (not torch.is_tensor(v) or (w.shape == v.shape and w.dtype == v.dtype and w.device == v.device)), (opt, k)
                if "step" in theirs["state"][i]:
                    assert float(mine["state"][i]["step"]) == 2.0
            fresh.load_state_dict(mine)
            for q, r in zip(o.param_groups[0]["params"], params):
                for k, v in o.state[q].items():
                    assert torch.equal(torch.as_tensor(v), torch.as_tensor(fresh.state[r][k])), k
            fresh.step()                    # and torch goes on from it


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_a_slice_on_its_own_takes_the_elementwise_launch(dev, momentum):
    """DCLLBase.train_dcll of one slice with SGD (DCLLBase's own default optimizer) and native_optimizers: the step is native, the update
    is one k_optim_multi launch, and parameters and momentum buffers are the restatement's bits; with the switch off the same call takes
    the autograd path and launches none"""
    from snn_modulation_classification_amd import ops
    _, xs, y = _data(dev)
    net = _net("sgd", on=False, cls=torch.optim.SGD, opt_param=dict(momentum=momentum))
    s = net.dcll_slices[0]
    with ops.kernel_trace() as tr:
        for t in range(BURNIN):
            s.train_dcll(xs[t], y, regularize=0)
        torch.cuda.synchronize()
    assert s._native_learning() is None and "k_optim_multi" not in tr.names
    net = _net("sgd", on=False, cls=torch.optim.SGD, opt_param=dict(momentum=momentum))
    s = net.dcll_slices[0]
    s.native_optimizers = True
    assert s._native_learning() is not None and not s._plain_adam()
    o, g = s.optimizer, s.optimizer.param_groups[0]
    cfg, n_upd = _config_of(o, g), 0
    for t in range(T):
        before = [(q.detach().cpu().numpy().copy(), {k: v.cpu().numpy().copy() for k, v in o.state.get(q, {}).items()}) for q in g["params"]]
        with ops.kernel_trace() as tr:
            s.train_dcll(xs[t], y, regularize=0)
            torch.cuda.synchronize()
        if t < BURNIN - 1:
            assert "k_optim_multi" not in tr.names
            continue
        n_upd += 1
        assert tr.names.count("k_optim_multi") == 1 and not any(n.startswith("k_grad_reduce") for n in tr.names), tr.names
        for q, (p0, st0) in zip(g["params"], before):
            if q.grad is None:
                continue
            assert float(q.grad.abs().max()) > 0
            buf0 = st0.get("momentum_buffer", np.zeros_like(p0) if momentum else None)
            wp, ws = C.optim_f32(cfg, p0.reshape(-1), q.grad.cpu().numpy().reshape(-1), [None if buf0 is None else buf0.reshape(-1), None, None],
                                 n_upd, first=bool(momentum) and n_upd == 1)
            assert bits_equal(q, wp), (t, "param")
            assert ("momentum_buffer" in o.state.get(q, {})) == bool(momentum)
            if momentum:
                assert bits_equal(o.state[q]["momentum_buffer"], ws[0]), (t, "momentum_buffer")
    assert n_upd == T - BURNIN + 1


def test_learn_sequence_trains_an_unserved_optimizer_under_autograd(dev):
    """learn_sequence runs under no_grad; the autograd step of a network the native step does not serve (Adamax with the switch off) is
    taken with gradients enabled: it trains — `step` counts the updates, the parameters move — instead of raising in loss.backward()"""
    cells, xs, y = _data(dev)
    net = _net("adamax", on=False)
    w0 = [s.dclllayer.i2h.weight.detach().clone() for s in net.dcll_slices]
    net.learn_sequence(cells, y)
    torch.cuda.synchronize()
    for s, w in zip(net.dcll_slices, w0):
        assert s._native_learning() is None
        assert int(s.optimizer.state[s.dclllayer.i2h.weight]["step"]) == T - BURNIN + 1
        assert not torch.equal(s.dclllayer.i2h.weight.detach(), w)


def test_seven_slices_go_out_in_several_launches(dev):
    """radio_ml_conv_ref.yaml on (2,128): seven slices, 16 tensors — two k_grad_reduce_optim launches per step (4 + 3 slices); graph
    replays == eager steps"""
    from snn_modulation_classification_amd import ops
    hw = (2, 128)
    _, xs, y = _data(dev, hw)
    nets = {graph: _net("adamax", graph=graph, spec="radio_ml_conv_ref.yaml", hw=hw) for graph in (False, True)}
    assert len(nets[False].dcll_slices) == 7
    for t in range(T):
        with ops.kernel_trace() as tr:
            nets[False].learn(xs[t], y)
            torch.cuda.synchronize()
        if t >= BURNIN - 1:
            assert tr.names.count("k_grad_reduce_optim") == 2 and tr.count("k_grad_reduce_adam") == 0, tr.names
        nets[True].learn(xs[t], y)
    torch.cuda.synchronize()
    assert sum(len(s._optim_tensors(advance=False)) for s in nets[False].dcll_slices) == 16
    assert next(iter(nets[True]._learn_graphs.values()))["n"] >= 2
    _assert_same(nets[False], nets[True], "seven slices, graph replays")


def test_a_plain_adam_network_keeps_its_launch_log_and_its_bits(dev):
    from snn_modulation_classification_amd import ops
    _, xs, y = _data(dev)
    kw = dict(cls=torch.optim.Adam, opt_param=dict(betas=[0.0, .95], weight_decay=10.0))
    a, b = _net("adam", on=False, **kw), _net("adam", on=True, **kw)
    logs = []
    for net in (a, b):
        with ops.kernel_trace() as tr:
            for t in range(T):
                net.learn(xs[t], y)
            torch.cuda.synchronize()
        logs.append(list(tr.names))
    assert logs[0] == logs[1] and logs[1].count("k_grad_reduce_adam") == T - BURNIN + 1
    assert not any(n in ("k_grad_reduce_optim", "k_optim_multi") for n in logs[1])
    _assert_same(a, b, "plain Adam")
    sig = b._graph_signature()
    b.native_optim_path = False
    assert b._graph_signature() == sig            # (nothing a captured plain-Adam timestep has baked in follows the switch)


def test_the_setter_refuses_what_is_not_served(dev):
    from snn_modulation_classification_amd import _lib
    for cls, kw in ((torch.optim.NAdam, dict(betas=[0.0, .95])), (torch.optim.RMSprop, {}), (torch.optim.Adamax, dict(maximize=True)),
                    (torch.optim.SGD, dict(maximize=True)), (torch.optim.AdamW, dict(capturable=True))):
        net = _net("x", on=False, cls=cls, opt_param=kw)
        with pytest.raises(_lib.DCLLUnsupported):
            net.native_optim_path = True
        assert net.native_optim_path is False and all(s._native_learning() is None for s in net.dcll_slices)
        net.native_optim_path = False                   # switching it off is always allowed
    net = _net("adamax", on=False)
    for s in net.dcll_slices:
        s.native_optimizers = True
    assert all(s._native_learning() is not None for s in net.dcll_slices) and net.native_optim_path is True


def test_the_environment_variable_sets_the_switch_at_construction(dev, monkeypatch):
    monkeypatch.setenv("DCLL_NATIVE_OPTIM", "1")
    net = _net("adamax", on=False)
    assert net.native_optim_path is True and all(s._native_learning() is not None for s in net.dcll_slices)


def test_entry_point_train_native_optim_path(tmp_path, capsys):
    """train.py --native_optim_path --optim_type Adamax --synthetic N runs the learning steps on k_grad_reduce_optim and prints no notice;
    under --optim_type Adam and NAdam the flag is ignored with one"""
    import train
    from snn_modulation_classification_amd import ops
    radio = ['--I_resolution', '24', '--Q_resolution', '24', '--arp', '1.0', '--burnin', '4', '--batch_size', '8', '--batch_size_test', '8',
             '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '6', '--n_iters_test', '6', '--n_steps', '1', '--n_test_interval', '1',
             '--learning_rates', '1e-7']
    with ops.kernel_trace() as tr:
        train.main(radio + ['--output', str(tmp_path / 'adamax'), '--native_optim_path', '--optim_type', 'Adamax'])
    text = capsys.readouterr().out
    assert "ignored" not in text and "k_grad_reduce_optim" in tr.names and "k_grad_reduce_adam" not in tr.names, text
    with ops.kernel_trace() as tr:
        train.main(radio + ['--output', str(tmp_path / 'off'), '--optim_type', 'Adamax'])
    assert "k_grad_reduce_optim" not in tr.names and "k_optim_multi" not in tr.names
    for name, more in (("Adam", []), ("NAdam", []), ("Adamax", ['--loss_type', 'MSELoss', '--lc_ampl', '0.5'])):
        with ops.kernel_trace() as tr:
            train.main(radio + ['--output', str(tmp_path / (name + str(len(more)))), '--native_optim_path', '--optim_type', name] + more)
        text = capsys.readouterr().out
        if more:            # (a loss the native step serves: no notice)
            assert "ignored" not in text and "k_grad_reduce_optim" in tr.names
        else:
            assert "--native_optim_path ignored" in text and "k_grad_reduce_optim" not in tr.names
    with ops.kernel_trace() as tr:      # a loss that keeps every slice under autograd: the switch would do nothing, so it is not set
        train.main(radio + ['--output', str(tmp_path / 'l1'), '--native_optim_path', '--optim_type', 'Adamax', '--loss_type', 'L1Loss'])
    assert "--native_optim_path ignored: the learning step of this network is not native" in capsys.readouterr().out
    assert "k_grad_reduce_optim" not in tr.names
