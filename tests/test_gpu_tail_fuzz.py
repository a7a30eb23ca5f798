"""Seeded differential tests of the readout and learning-tail C ABI — dcll_readout, dcll_readout_mode, dcll_readout_splitk,
dcll_readout_act, dcll_step_readouts, dcll_step_readouts_multi, dcll_local_loss_grad, dcll_adam_step, dcll_adam_step_dyn,
dcll_grad_reduce_adam, dcll_argmax_vote — on the cases of tests/tail_cases.py (proven on the CPU by tests/test_tail_cases.py): one
case per reachable kernel form with rows, widths and K on both sides of the form's tiles, the fused step tail with the MNIST width and
widths on tile edges, several tails in one launch, the loss gradient on SmoothL1's kink, Adam over ragged / empty / eight tensors, the
fused gradient reduction, both paths of k_argmax, free draws, refusals.

References are independent of device code: the GEMMs against a float64 matmul — BIT FOR BIT on `grid` and `probe` draws (exact by
construction), within the header's 1e-4 on `cont` draws —, the recorded argmax against numpy's first maximum, the loss gradients and
Adam against float32 restatements of the kernels' operation order bit for bit, sums against float64 within the bound of a float32
sum in any order.  Calls go through snn_modulation_classification_amd.ops, through _lib only where ops cannot express the call
(bias = NULL, db = NULL, an empty tensor, dcll_readout on a shape ops routes to the split-K entry, caller buffers for the vote).
Every output lands in a caller buffer with a 64-element sentinel tail that must stay intact, every call is wrapped in
ops.kernel_trace() — the log must equal expected_kernels(case) — and is issued twice: both results must be bit-identical.

The last test asserts that every reachable variant key was served by a case that ran to the end."""
import collections
import os
import time

import numpy as np
import pytest
import torch

import tail_cases as TC

pytestmark = pytest.mark.gpu

CASES = TC.cases()
REFUSE = TC.refusals()
STRATA = collections.defaultdict(list)
for _c in CASES:
    STRATA[_c["stratum"]].append(_c)

LOGIT_TOL = TC.LOGIT_TOL    # the header's readout contract
GUARD = 64                  # sentinel elements behind (and between) caller buffers
SENT_F, SENT_I = -7.25, 0x5a5a5a5a

SERVED = collections.Counter()          # variant key -> cases that ran to the end with a call on it
RAN = set()
TIMES = collections.Counter()
WORST = collections.defaultdict(float)  # GEMM form -> largest |err| of a cont draw


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _sent(dtype):
    return SENT_I if dtype == torch.int32 else SENT_F


def guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), _sent(dtype), device=dev, dtype=dtype)
    return buf[:n].view(shape), buf


def guard_intact(buf):
    return bool((buf[-GUARD:] == _sent(buf.dtype)).all())


def place(a, dev, off=0):
    """numpy -> device tensor `off` elements (4 bytes each) behind a 16-byte aligned allocation"""
    a = np.ascontiguousarray(a)
    buf = torch.empty((a.size + 4,), device=dev, dtype=torch.from_numpy(a).dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return v


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_bits(got, ref, tag):
    g, r = bits(got), bits(np.asarray(ref, np.float32))
    assert g.shape == r.shape, (tag, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        gf, rf = g.view(np.float32), r.view(np.float32)
        raise AssertionError((tag, "%d of %d elements differ" % (len(bad), g.size), "first", bad[:4].tolist(),
                              "got", [float(gf[tuple(b)]) for b in bad[:4]], "want", [float(rf[tuple(b)]) for b in bad[:4]]))


def same_bits(a, b, tag):
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
        (tag, "two issues of the same call differ")


def done(c, t0):
    TIMES[c["stratum"]] += time.time() - t0
    RAN.add(c["id"])
    SERVED.update(set(TC.variant_keys(c)))


# ----------------------------------------------------------------------------------------------------------------------
# the GEMM calls
# ----------------------------------------------------------------------------------------------------------------------


def ops_serves(c, aligned):
    """True if ops.readout / ops.readout_act reaches the case's entry point with the case's arguments"""
    if not c["bias"]:
        return False
    to_splitk = (c["rows"] <= 2048 or c["K"] >= 65536) and TC.splitk_scratch(c["rows"], c["K"], c["N"]) > 0 and aligned
    if c["call"] == "readout":
        return not to_splitk
    if c["call"] == "mode":
        return c["mode"] != TC.AUTO
    return to_splitk if c["call"] == "splitk" else True


def issue_gemm(c, pv, Wt, bias, out, area, need):
    from snn_modulation_classification_amd import _lib, ops
    rows, K, N = c["rows"], c["K"], c["N"]
    aligned = not (c["off_pv"] or c["off_wt"])
    with ops.kernel_trace() as tr:
        if ops_serves(c, aligned):
            if c["call"] == "act":
                ops.readout_act(pv, Wt, bias, out=out, presigmoid=c["sig"], scratch=dict(act_splitk=area))
            else:
                ops.readout(pv, Wt, bias, out=out, mode=c["mode"] if c["call"] == "mode" else ops.READOUT_AUTO, scratch=dict(splitk=area))
        else:
            lib, P, st = _lib.get(), _lib.ptr, _lib.stream_ptr()
            if c["call"] == "readout":
                rc = lib.dcll_readout(P(pv), P(Wt), P(bias), P(out), rows, K, N, st)
            elif c["call"] == "mode":
                rc = lib.dcll_readout_mode(P(pv), P(Wt), P(bias), P(out), rows, K, N, c["mode"], st)
            elif c["call"] == "splitk":
                rc = lib.dcll_readout_splitk(P(pv), P(Wt), P(bias), P(out), P(area), need, rows, K, N, st)
            else:
                rc = lib.dcll_readout_act(P(pv), P(Wt), P(bias), P(out), P(area), need, rows, K, N, int(c["sig"]), st)
            _lib.check(rc, "dcll_readout*")
    return tr.names


def run_gemm(c, dev):
    from snn_modulation_classification_amd import _lib
    print(TC.describe(c))
    t0 = time.time()
    lib = _lib.get()
    rows, K, N = c["rows"], c["K"], c["N"]
    exp = TC.expected_scratch(c)
    assert lib.dcll_readout_splitk_scratch(rows, K, N) == exp["splitk"]
    assert lib.dcll_readout_act_scratch(rows, K, N) == exp["act"]
    assert lib.dcll_step_readouts_scratch(rows, K, N, 0) == exp["step"]
    d = TC.gemm_data(c)
    if c["big"]:
        pv = torch.from_numpy(d["pv_i8"]).to(dev).to(torch.float32).mul_(d["pv_scale"])
    else:
        pv = place(d["pv"], dev, c["off_pv"])
    Wt = place(d["Wt"], dev, c["off_wt"])
    bias = place(d["bias"], dev) if c["bias"] else None
    need = exp["splitk"] if c["call"] == "splitk" else exp["act"] if c["call"] == "act" else 0
    area, abuf = guarded((need,), torch.float32, dev) if need else (None, None)
    outs = []
    for k in range(2):
        out, obuf = guarded((rows, N), torch.float32, dev)
        names = issue_gemm(c, pv, Wt, bias, out, area, need)
        torch.cuda.synchronize()
        assert names == TC.expected_kernels(c), (names, TC.expected_kernels(c))
        assert guard_intact(obuf) and (abuf is None or guard_intact(abuf)), "sentinel tail overwritten"
        outs.append(out)
    same_bits(outs[0], outs[1], c["id"])
    if c["draw"] in ("grid", "probe"):
        assert d["units"] < 2 ** 24
        assert_bits(outs[0], d["ref"], c["id"])
    else:
        err = float(np.abs(outs[0].cpu().numpy().astype(np.float64) - d["ref"]).max())
        key = TC.variant_key(c)
        print("%s: max |err| %.3g (contract %.3g)" % (" ".join(map(str, key)), err, LOGIT_TOL))
        WORST[key] = max(WORST[key], err)
        assert err <= LOGIT_TOL, err
    done(c, t0)


# ----------------------------------------------------------------------------------------------------------------------
# the fused step tail, one call or several in one launch
# ----------------------------------------------------------------------------------------------------------------------


def step_operands(it, d, c, dev):
    """device operands and guarded outputs of one step call / multi item"""
    rows, N1, N2 = it["rows"], it["N1"], it["N2"]
    need = TC.step_scratch(rows, it["K"], N1, N2)
    o = dict(pv=place(d["pv"], dev), Wt=place(d["Wt"], dev), bias=place(d["bias"], dev), bufs=[])

    def g(name, shape, dtype=torch.float32):
        o[name], b = guarded(shape, dtype, dev)
        o["bufs"].append(b)
    g("p", (rows, N1))
    g("area", (need,))
    if N2:
        g("o", (rows, N2))
    else:
        o["o"] = None
    scr = dict(step_ro=o["area"])
    fin = dict(clout=None, target=None)
    if c["clout"]:
        g("clout", (rows,), torch.int32)
        fin["clout"] = o["clout"]
    if c["target"]:
        fin.update(target=place(d["target"], dev), kind=it["kind"])
        g("g_p", (rows, N1))
        scr["g_p"] = o["g_p"]
        if N2:
            g("g_o", (rows, N2))
            scr["g_o"] = o["g_o"]
    o.update(scr=scr, fin=fin)
    return o


def check_step(it, d, c, o, tag):
    rows, N1, N2 = it["rows"], it["N1"], it["N2"]
    for b in o["bufs"]:
        assert guard_intact(b), (tag, "sentinel tail overwritten")
    got = torch.cat([o["p"], o["o"]], dim=1) if N2 else o["p"]
    if c["draw"] in ("grid", "probe"):
        assert d["units"] < 2 ** 24
        assert_bits(got, d["ref"], tag)
    else:
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - d["ref"]).max())
        print("%s: max |err| %.3g (contract %.3g)" % (tag, err, LOGIT_TOL))
        WORST[("k_readout_t16" if c["call"] == "step" else "k_readout_t16m", "step tail")] = \
            max(WORST[("k_readout_t16" if c["call"] == "step" else "k_readout_t16m", "step tail")], err)
        assert err <= LOGIT_TOL, (tag, err)
    if c["clout"]:
        cl = o["clout"].cpu().numpy()
        sure = d["sure"]
        assert np.array_equal(cl[sure], d["clout_ref"][sure]), (tag, "clout", np.argwhere(cl[sure] != d["clout_ref"][sure])[:4].tolist())
        assert ((cl >= 0) & (cl < N1)).all()
    if c["target"]:
        n = rows * N1
        assert_bits(o["g_p"], TC.loss_grad_f32(o["p"].cpu().numpy(), d["target"], it["kind"], n), tag + " g_p")
        if N2:
            assert_bits(o["g_o"], TC.loss_grad_f32(o["o"].cpu().numpy(), d["target"], it["kind"], n), tag + " g_o")


def outputs_of(o):
    return [o[k] for k in ("p", "o", "clout", "g_p", "g_o") if o.get(k) is not None]


def run_step(c, dev):
    from snn_modulation_classification_amd import _lib, ops
    print(TC.describe(c))
    t0 = time.time()
    assert _lib.get().dcll_step_readouts_scratch(c["rows"], c["K"], c["N1"], c["N2"]) == TC.expected_scratch(c)["step"]
    d = TC.step_data(c, c["draw"], c["seed"], c["target"])
    res = []
    for k in range(2):
        o = step_operands(c, d, c, dev)
        with ops.kernel_trace() as tr:
            ops.step_readouts(o["pv"], o["Wt"], o["bias"], c["N1"], c["N2"], o["p"], o["o"], scratch=o["scr"], finish=o["fin"])
        torch.cuda.synchronize()
        assert tr.names == TC.expected_kernels(c), tr.names
        assert o["fin"].get("clout") is o.get("clout") and o["fin"].get("g_p") is o.get("g_p") and o["fin"].get("g_o") is o.get("g_o")
        res.append(o)
    for a, b in zip(outputs_of(res[0]), outputs_of(res[1])):
        same_bits(a, b, c["id"])
    check_step(c, d, c, res[0], c["id"])
    done(c, t0)


def run_multi(c, dev):
    from snn_modulation_classification_amd import _lib, ops
    print(TC.describe(c))
    t0 = time.time()
    assert os.environ.get("DCLL_STEP_RO_MULTI", "1") != "0"
    lib = _lib.get()
    ds = [TC.step_data(it, c["draw"], c["seed"] + j, c["target"]) for j, it in enumerate(c["items"])]
    for it, s in zip(c["items"], TC.expected_scratch(c)["step"]):
        assert lib.dcll_step_readouts_scratch(it["rows"], it["K"], it["N1"], it["N2"]) == s
    res = []
    for k in range(2):
        os_ = [step_operands(it, d, c, dev) for it, d in zip(c["items"], ds)]
        fins = []
        for it, o in zip(c["items"], os_):
            f = dict(o["fin"])
            f.update(run_readouts=lambda: None, ro_call=(o["pv"], o["Wt"], o["bias"], it["N1"], it["N2"], o["p"], o["o"], o["scr"]))
            fins.append(f)
        with ops.kernel_trace() as tr:
            ops.run_deferred_readouts(fins)
        torch.cuda.synchronize()
        assert tr.names == TC.expected_kernels(c), tr.names
        res.append(os_)
    for j, (it, d) in enumerate(zip(c["items"], ds)):
        tag = "%s item %d" % (c["id"], j)
        for a, b in zip(outputs_of(res[0][j]), outputs_of(res[1][j])):
            same_bits(a, b, tag)
        check_step(it, d, c, res[0][j], tag)
        if c["draw"] == "cont":         # "results per item = dcll_step_readouts on it, bit for bit"
            o = step_operands(it, d, c, dev)
            ops.step_readouts(o["pv"], o["Wt"], o["bias"], it["N1"], it["N2"], o["p"], o["o"], scratch=o["scr"], finish=o["fin"])
            for a, b in zip(outputs_of(res[0][j]), outputs_of(o)):
                same_bits(a, b, tag + " vs the single call")
    done(c, t0)


# ----------------------------------------------------------------------------------------------------------------------
# loss gradient
# ----------------------------------------------------------------------------------------------------------------------


def run_loss(c, dev):
    from snn_modulation_classification_amd import ops
    print(TC.describe(c))
    t0 = time.time()
    B, N, kind = c["B"], c["N"], c["kind"]
    d = TC.loss_data(c)
    p, t = place(d["p"], dev), place(d["target"], dev)
    o = place(d["o"], dev) if c["has_o"] else None
    res = []
    for k in range(2):
        out, bufs = {}, []
        for name, shape, want in (("g_p", (B, N), True), ("g_o", (B, N), c["has_o"]), ("loss", (1,), c["want_loss"])):
            if want:
                out[name], b = guarded(shape, torch.float32, dev)
                bufs.append(b)
        clout = None
        if c["want_clout"]:
            clout, b = guarded((B,), torch.int32, dev)
            bufs.append(b)
        keep = dict(out)
        with ops.kernel_trace() as tr:
            r = ops.local_loss_grad(p, o, t, kind, out=out, want_loss=c["want_loss"], want_clout=c["want_clout"], clout_out=clout)
        torch.cuda.synchronize()
        assert tr.names == TC.expected_kernels(c), tr.names
        assert all(out[k_] is keep[k_] for k_ in keep) and r[0] is keep["g_p"], "the binding did not use the caller's buffers"
        assert (r[1] is None) == (not c["has_o"]) and (r[2] is None) == (not c["want_loss"])
        assert all(guard_intact(b) for b in bufs), "sentinel tail overwritten"
        res.append([keep[k_] for k_ in sorted(keep)] + ([clout] if clout is not None else []))
        if k == 0:
            first = dict(keep, clout=clout)
    for a, b in zip(res[0], res[1]):
        same_bits(a, b, c["id"])
    n = B * N
    assert_bits(first["g_p"], TC.loss_grad_f32(d["p"], d["target"], kind, n), c["id"] + " g_p")
    if c["has_o"]:
        assert_bits(first["g_o"], TC.loss_grad_f32(d["o"], d["target"], kind, n), c["id"] + " g_o")
    if c["want_loss"]:
        ref, bound = TC.loss_value_ref(d, kind)
        got = float(first["loss"].cpu().numpy()[0])
        print("loss %.9g, float64 %.9g, |diff| %.3g (bound %.3g)" % (got, ref, abs(got - ref), bound))
        assert abs(got - ref) <= bound, (got, ref, bound)
    if c["want_clout"]:
        rec = d["o"] if c["has_o"] else d["p"]
        assert np.array_equal(first["clout"].cpu().numpy(), rec.argmax(axis=1).astype(np.int32)), "clout"
    done(c, t0)


# ----------------------------------------------------------------------------------------------------------------------
# Adam, alone and behind the gradient reduction
# ----------------------------------------------------------------------------------------------------------------------
KEYS = ("param", "grad", "exp_avg", "exp_avg_sq")


class AdamBufs:
    """Every tensor of a case in ONE buffer per kind — GUARD sentinels in front, between and behind — so that the elements behind a
    ragged tensor and its neighbours are compared like everything else: whole buffers against whole host images."""

    def __init__(self, sizes, dev):
        self.sizes, self.dev = sizes, dev
        self.offs, pos = [], GUARD
        for n in sizes:
            self.offs.append(pos)
            pos += n + GUARD
        self.total = pos
        self.host = {k: np.full(self.total, SENT_F, np.float32) for k in KEYS}
        self.dev_bufs = {k: torch.full((self.total,), SENT_F, device=dev, dtype=torch.float32) for k in KEYS}

    def sl(self, k):
        return slice(self.offs[k], self.offs[k] + self.sizes[k])

    def upload(self, keys=KEYS):
        for key in keys:
            self.dev_bufs[key].copy_(torch.from_numpy(self.host[key]))

    def view(self, key, k):
        return self.dev_bufs[key][self.sl(k)]

    def dicts(self, hps, step, grads=None):
        """adam_step's dicts; grads[k]: a tensor that replaces the buffer's gradient (a layer's dW / db)"""
        return [dict(hps[k], step=step, param=self.view("param", k), grad=(grads or {}).get(k, self.view("grad", k)),
                     exp_avg=self.view("exp_avg", k), exp_avg_sq=self.view("exp_avg_sq", k)) for k in range(len(self.sizes))]

    def array(self, hps, step, grads=None):
        """the same as a dcll_adam_tensor array with explicit pointers: an EMPTY tensor still has its place in the buffers (a torch
        view of no elements has no data pointer, which the binding cannot hand over)"""
        from snn_modulation_classification_amd import _lib
        arr = (_lib.AdamTensor * max(1, len(self.sizes)))()
        for k, a in enumerate(arr[:len(self.sizes)]):
            base = {key: self.dev_bufs[key].data_ptr() + 4 * self.offs[k] for key in KEYS}
            if grads and k in grads:
                base["grad"] = grads[k].data_ptr()
            a.param, a.grad, a.exp_avg, a.exp_avg_sq = base["param"], base["grad"], base["exp_avg"], base["exp_avg_sq"]
            a.n, a.step = self.sizes[k], step
            hp = hps[k]
            a.lr, a.weight_decay, a.beta1, a.beta2, a.eps = hp["lr"], hp["weight_decay"], hp["beta1"], hp["beta2"], hp["eps"]
        return arr

    def snapshot(self):
        return {k: self.dev_bufs[k].clone() for k in KEYS}

    def restore(self, snap):
        for k in KEYS:
            self.dev_bufs[k].copy_(snap[k])

    def check(self, tag, keys=KEYS):
        for key in keys:
            assert_bits(self.dev_bufs[key], self.host[key], "%s %s (sentinels between the tensors included)" % (tag, key))


def dyn_tensor(c, hps, step, dev):
    from snn_modulation_classification_amd import ops
    vals = ops.adam_dyn_values([dict(hp, step=step) for hp in hps])
    mine = [float(x) for hp in hps for x in TC.adam_host_triple(hp["lr"], hp["beta1"], hp["beta2"], step)]
    assert [np.float32(v) for v in vals] == [np.float32(v) for v in mine]
    return torch.tensor(vals, device=dev, dtype=torch.float32) if vals else torch.zeros((0,), device=dev)


def run_adam(c, dev):
    from snn_modulation_classification_amd import _lib, ops
    print(TC.describe(c))
    t0 = time.time()
    sizes = c["sizes"]
    hps = [TC.adam_hp(c, k) for k in range(len(sizes))]
    data = TC.adam_data(c)
    ab = AdamBufs(sizes, dev)
    for k, t in enumerate(data):
        for key in ("param", "exp_avg", "exp_avg_sq"):
            ab.host[key][ab.sl(k)] = t[key]
    ab.upload()
    via_ops = all(n > 0 for n in sizes)
    for j in range(3):
        step = c["step"] + j
        for k, t in enumerate(data):
            ab.host["grad"][ab.sl(k)] = t["grads"][j]
        ab.upload(("grad",))
        dyn = dyn_tensor(c, hps, step, dev) if c["dyn"] else None
        snap = ab.snapshot()
        results = []
        for again in range(2):
            ab.restore(snap)
            with ops.kernel_trace() as tr:
                if via_ops:
                    ops.adam_step(ab.dicts(hps, step), dyn=dyn)
                elif dyn is not None:
                    _lib.check(_lib.get().dcll_adam_step_dyn(ab.array(hps, step), len(sizes), _lib.ptr(dyn), _lib.stream_ptr()), "dcll_adam_step_dyn")
                else:
                    _lib.check(_lib.get().dcll_adam_step(ab.array(hps, step), len(sizes), _lib.stream_ptr()), "dcll_adam_step")
            torch.cuda.synchronize()
            assert tr.names == TC.expected_kernels(c), tr.names
            results.append(ab.snapshot())
        for key in KEYS:
            same_bits(results[0][key], results[1][key], "%s step %d %s" % (c["id"], step, key))
        for k, t in enumerate(data):
            s = ab.sl(k)
            ab.host["param"][s], ab.host["exp_avg"][s], ab.host["exp_avg_sq"][s] = \
                TC.adam_f32(ab.host["param"][s], ab.host["grad"][s], ab.host["exp_avg"][s], ab.host["exp_avg_sq"][s], hps[k], step)
        ab.check("%s step %d" % (c["id"], step))
    done(c, t0)


def run_reduce_adam(c, dev):
    from snn_modulation_classification_amd import _lib, ops
    print(TC.describe(c))
    t0 = time.time()
    sizes, step = c["sizes"], c["step"]
    hps = [TC.adam_hp(c, k) for k in range(len(sizes))]
    data = TC.adam_data(c, nsteps=1)
    parts = TC.reduce_data(c)
    ab = AdamBufs(sizes, dev)
    for k, t in enumerate(data):
        for key in ("param", "exp_avg", "exp_avg_sq"):
            ab.host[key][ab.sl(k)] = t[key]
        ab.host["grad"][ab.sl(k)] = t["grads"][0]
    referred = {}
    for li, L in enumerate(c["layers"]):
        for idx, which in ((L["adam_w"], "dW"), (L["adam_b"], "db")):
            if idx >= 0:
                referred[idx] = (li, which)
                ab.host["grad"][ab.sl(idx)] = SENT_F         # (its gradient is the layer's dW / db: this slot must stay untouched)
    ab.upload()
    dyn = dyn_tensor(c, hps, step, dev) if c["dyn"] else None
    via_ops = all(n > 0 for n in sizes) and all(L["db"] for L in c["layers"])
    assert TC.reduce_adam_grid(c["layers"], sizes) > 0
    snap = ab.snapshot()
    results = []
    dparts = [place(p_, dev) for p_ in parts]
    for again in range(2):
        ab.restore(snap)
        lays, grads, outs, bufs = [], {}, [], []
        for li, L in enumerate(c["layers"]):
            dW, b1 = guarded((L["c_out"] * (L["rowlen"] - 1),), torch.float32, dev)
            db, b2 = guarded((L["c_out"],), torch.float32, dev)
            bufs += [b1, b2]
            outs += [dW, db]
            lays.append(dict(part=dparts[li].data_ptr(), dW=dW, db=db, rowlen=L["rowlen"], nchunk=L["nchunk"], c_out=L["c_out"],
                             adam_w=L["adam_w"], adam_b=L["adam_b"]))
            if L["adam_w"] >= 0:
                grads[L["adam_w"]] = dW
            if L["adam_b"] >= 0:
                grads[L["adam_b"]] = db
        with ops.kernel_trace() as tr:
            if via_ops:
                ops.grad_reduce_adam(lays, ab.dicts(hps, step, grads), dyn=dyn)
            else:
                larr = (_lib.GradParts * len(lays))()
                for a, L, Lc in zip(larr, lays, c["layers"]):
                    a.part, a.dW, a.db = L["part"], L["dW"].data_ptr(), (L["db"].data_ptr() if Lc["db"] else None)
                    a.rowlen, a.nchunk, a.c_out, a.adam_w, a.adam_b = L["rowlen"], L["nchunk"], L["c_out"], L["adam_w"], L["adam_b"]
                _lib.check(_lib.get().dcll_grad_reduce_adam(larr, len(lays), ab.array(hps, step, grads), len(sizes), _lib.ptr(dyn),
                                                            _lib.stream_ptr()), "dcll_grad_reduce_adam")
        torch.cuda.synchronize()
        assert tr.names == TC.expected_kernels(c), tr.names
        assert all(guard_intact(b) for b in bufs), "sentinel tail overwritten"
        results.append((ab.snapshot(), outs))
    for key in KEYS:
        same_bits(results[0][0][key], results[1][0][key], "%s %s" % (c["id"], key))
    for a, b in zip(results[0][1], results[1][1]):
        same_bits(a, b, c["id"] + " dW / db")
    # gradients: the float64 sum over the chunks, bit for bit on integer rows, else within nchunk 2^-24 sum_c |part| (any order)
    dev_grad = {}
    for li, L in enumerate(c["layers"]):
        dW, db = results[0][1][2 * li].cpu().numpy(), results[0][1][2 * li + 1].cpu().numpy()
        p64 = parts[li].astype(np.float64)
        tot = p64.sum(axis=0).reshape(L["c_out"], L["rowlen"])
        bound = (L["nchunk"] * 2.0 ** -24 * np.abs(p64).sum(axis=0)).reshape(L["c_out"], L["rowlen"])
        want_w, want_b = tot[:, :-1].ravel(), tot[:, -1]
        tag = "%s layer %d" % (c["id"], li)
        if c["draw"] == "int":
            assert_bits(dW, want_w, tag + " dW")
            if L["db"]:
                assert_bits(db, want_b, tag + " db")
        else:
            assert (np.abs(dW - want_w) <= bound[:, :-1].ravel()).all(), tag + " dW"
            assert not L["db"] or (np.abs(db - want_b) <= bound[:, -1]).all(), tag + " db"
        if not L["db"]:
            assert (db == np.float32(SENT_F)).all(), tag + ": db = NULL was written"
            assert c["draw"] == "int"                       # (the bias gradient Adam used is then known exactly)
            db = want_b.astype(np.float32)
        dev_grad[L["adam_w"]], dev_grad[L["adam_b"]] = dW, db
    for k in range(len(sizes)):
        s = ab.sl(k)
        g = dev_grad[k] if k in referred else ab.host["grad"][s]
        ab.host["param"][s], ab.host["exp_avg"][s], ab.host["exp_avg_sq"][s] = \
            TC.adam_f32(ab.host["param"][s], g, ab.host["exp_avg"][s], ab.host["exp_avg_sq"][s], hps[k], step)
    ab.restore(results[0][0])
    ab.check(c["id"])
    done(c, t0)


# ----------------------------------------------------------------------------------------------------------------------
# argmax and vote
# ----------------------------------------------------------------------------------------------------------------------


def run_vote(c, dev):
    from oracle import c_oracle
    from snn_modulation_classification_amd import _lib, ops
    print(TC.describe(c))
    t0 = time.time()
    T, B, N = c["T"], c["B"], c["N"]
    lg = TC.vote_data(c)
    logits = place(lg, dev, c["off"])
    with ops.kernel_trace() as tr:
        clout, vote = ops.argmax_vote(logits, c["t_begin"], want_vote=c["want_vote"])
    torch.cuda.synchronize()
    assert tr.names == TC.expected_kernels(c), tr.names
    # the second issue into caller buffers with sentinel tails (the binding allocates its own)
    cl2, b1 = guarded((T, B), torch.int32, dev)
    v2, b2 = guarded((B,), torch.int32, dev)
    with ops.kernel_trace() as tr:
        _lib.check(_lib.get().dcll_argmax_vote(_lib.ptr(logits), _lib.ptr(cl2), _lib.ptr(v2) if c["want_vote"] else None, T, B, N, c["t_begin"],
                                               _lib.stream_ptr()), "dcll_argmax_vote")
    torch.cuda.synchronize()
    assert tr.names == TC.expected_kernels(c), tr.names
    assert guard_intact(b1) and guard_intact(b2)
    same_bits(clout, cl2, c["id"] + " clout")
    ref = lg.argmax(axis=2).astype(np.int32)
    assert np.array_equal(clout.cpu().numpy(), ref), "clout != numpy's first maximum"
    if c["want_vote"]:
        same_bits(vote, v2, c["id"] + " vote")
        assert np.array_equal(vote.cpu().numpy(), TC.vote_ref(ref, c["t_begin"])), "vote != Counter.most_common(1)"
        oc, ov = c_oracle.argmax_vote(lg, c["t_begin"])
        assert np.array_equal(clout.cpu().numpy(), oc) and np.array_equal(vote.cpu().numpy(), ov), "!= the C oracle"
    else:
        assert bool((v2 == SENT_I).all())
    done(c, t0)


RUN = dict(readout=run_gemm, mode=run_gemm, splitk=run_gemm, act=run_gemm, step=run_step, multi=run_multi, loss=run_loss, adam=run_adam,
           reduce_adam=run_reduce_adam, vote=run_vote)


def _ids(cs):
    return [c["id"] for c in cs]


@pytest.mark.parametrize("case", STRATA["variants"], ids=_ids(STRATA["variants"]))
def test_every_readout_form(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["step_tail"], ids=_ids(STRATA["step_tail"]))
def test_step_tail(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["step_multi"], ids=_ids(STRATA["step_multi"]))
def test_step_tails_in_one_launch(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["loss"], ids=_ids(STRATA["loss"]))
def test_local_loss_grad(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["adam"], ids=_ids(STRATA["adam"]))
def test_adam_three_steps(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["reduce_adam"], ids=_ids(STRATA["reduce_adam"]))
def test_grad_reduce_adam(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["vote"], ids=_ids(STRATA["vote"]))
def test_argmax_vote(dev, case):
    RUN[case["call"]](case, dev)


@pytest.mark.parametrize("case", STRATA["free"], ids=_ids(STRATA["free"]))
def test_free_draws(dev, case):
    RUN[case["call"]](case, dev)


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------


def refusal_call(r, dev):
    """-> (rc, the sentinel-filled outputs of the call).  Every call is servable but for the one thing r['what'] names."""
    from snn_modulation_classification_amd import _lib
    lib, P, st = _lib.get(), _lib.ptr, _lib.stream_ptr()
    e, w = r["entry"], r["what"]
    zeros = lambda n, dt=torch.float32: torch.zeros((int(n) + 4,), device=dev, dtype=dt)
    full = lambda n, dt=torch.float32: torch.full((int(n) + 2,), _sent(dt), device=dev, dtype=dt)
    off = lambda t, yes: t[1:] if yes else t
    outs = {}
    if e in ("splitk", "act", "mode"):
        rows, K, N = 8, (64 if e == "mode" else 2048), 24
        rows = 2049 if w == "rows=2049" else rows
        K = {"K=1024": 1024, "K=2304+128": 2432, "K=100": 100}.get(w, 65536 if w.startswith("K=65536") else K)
        N = 65 if w == "N=65" else N
        pv, Wt, bias = off(zeros(rows * K), w == "off_pv"), off(zeros(N * K), w == "off_wt"), zeros(N)
        outs["out"] = full(rows * N)
        if e == "mode":
            return lib.dcll_readout_mode(P(pv), P(Wt), P(bias), P(outs["out"]), rows, K, N, int(w.split("=")[1]), st), outs
        need = (lib.dcll_readout_splitk_scratch if e == "splitk" else lib.dcll_readout_act_scratch)(rows, K, N)
        outs["scratch"] = full(max(need, 64 * rows * N))
        given = need - 1 if "one float short" in w else outs["scratch"].numel()
        scr = None if "without scratch" in w else P(outs["scratch"])
        if e == "splitk":
            assert need > 0 or "scratch" not in w
            return lib.dcll_readout_splitk(P(pv), P(Wt), P(bias), P(outs["out"]), scr, given, rows, K, N, st), outs
        return lib.dcll_readout_act(P(pv), P(Wt), P(bias), P(outs["out"]), scr, given, rows, K, N, 2 if w == "act=2" else 0, st), outs
    if e in ("step", "multi"):
        def item(i, rows=8, K=2048, N1=24, N2=0, learn=False, kind=0, g_p=True, reserved=0, share=None):
            pre = "item%d " % i
            outs[pre + "p"], outs[pre + "o"], outs[pre + "clout"] = full(max(rows, 1) * N1), full(max(rows, 1) * max(N2, 1)), full(max(rows, 1), torch.int32)
            outs[pre + "g_p"], outs[pre + "g_o"] = full(max(rows, 1) * N1), full(max(rows, 1) * max(N2, 1))
            need = lib.dcll_step_readouts_scratch(max(rows, 1), K, N1, N2)
            scratch = share if share is not None else full(max(need, 64 * max(rows, 1) * (N1 + N2)))
            outs[pre + "scratch"] = scratch
            keep = (zeros(max(rows, 1) * K), zeros((N1 + N2) * K), zeros(N1 + N2), zeros(max(rows, 1) * N1))
            it = _lib.StepRo(P(keep[0]).value, P(keep[1]).value, P(keep[2]).value, P(scratch).value, scratch.numel(), rows, K, N1, N2, kind,
                             P(outs[pre + "p"]).value, P(outs[pre + "o"]).value if N2 else None, P(outs[pre + "clout"]).value,
                             P(keep[3]).value if learn else None, P(outs[pre + "g_p"]).value if (learn and g_p) else None,
                             P(outs[pre + "g_o"]).value if (learn and N2) else None, reserved)
            return it, keep, need
        if e == "step":
            kw = {"N2!=N1": dict(N2=10), "N1+N2=66": dict(N1=33, N2=33), "rows=2049": dict(rows=2049), "K=65536": dict(K=65536),
                  "target without g_p": dict(learn=True, g_p=False), "kind=7": dict(learn=True, kind=7), "scratch one float short": {}}[w]
            it, keep, need = item(0, **kw)
            given = need - 1 if "one float short" in w else it.scratch_floats
            return lib.dcll_step_readouts(it.pv, it.Wt, it.bias, it.scratch, given, it.rows, it.K, it.N1, it.N2, it.p, it.o, it.clout,
                                          it.target, it.g_p, it.g_o, it.kind, st), outs
        n = 9 if w == "9 items" else 2
        its, keeps = [], []
        for i in range(n):
            kw = {}
            if i == 1:
                kw = {"reserved=1": dict(reserved=1), "mixed targets": dict(learn=False), "empty item": dict(rows=0),
                      "shared scratch": dict(share=outs["item0 scratch"])}.get(w, {})
            if i == 0 and w == "mixed targets":
                kw = dict(learn=True)
            it, keep, _ = item(i, **kw)
            its.append(it)
            keeps.append(keep)
        arr = (_lib.StepRo * n)(*its)
        return lib.dcll_step_readouts_multi(arr, n, st), outs
    if e == "loss":
        B, N = ((1 << 24) + 1, 1) if w.startswith("B*N") else (8, 24)
        p, t = zeros(B * N), zeros(B * N)
        o = zeros(B * N) if w == "o without g_o" else None
        outs.update(g_p=full(B * N), loss=full(1), clout=full(B, torch.int32))
        return lib.dcll_local_loss_grad(P(p), P(o), P(t), P(outs["g_p"]), None, P(outs["loss"]), P(outs["clout"]), B, N, 7 if w == "kind=7" else 0,
                                        st), outs
    if e in ("adam", "adam_dyn", "reduce_adam"):
        sizes = [16, 4] + ([100] * 7 if w == "9 tensors" else [])
        arr = (_lib.AdamTensor * len(sizes))()
        grads = []
        for k, (a, n) in enumerate(zip(arr, sizes)):
            for key in ("param", "exp_avg", "exp_avg_sq"):
                outs["%s%d" % (key, k)] = full(n)
            grads.append(zeros(n))
            a.param, a.grad, a.exp_avg = P(outs["param%d" % k]).value, P(grads[k]).value, P(outs["exp_avg%d" % k]).value
            a.exp_avg_sq = None if (w == "null moment" and k == 1) else P(outs["exp_avg_sq%d" % k]).value
            a.n, a.step = n, 0 if (w == "step=0" and k == 1) else 3
            a.lr, a.weight_decay, a.beta1, a.beta2, a.eps = 1e-3, 0.0, 0.9, 0.999, 1e-8
        if e == "adam":
            return lib.dcll_adam_step(arr, len(sizes), st), outs
        if e == "adam_dyn":
            return lib.dcll_adam_step_dyn(arr, len(sizes), None, st), outs
        nl = 5 if w == "5 layers" else 1
        larr = (_lib.GradParts * nl)()
        part = zeros(3 * 4 * 5)
        for li, a in enumerate(larr):
            outs["dW%d" % li], outs["db%d" % li] = full(16), full(4)
            a.part, a.dW, a.db = P(part).value, P(outs["dW%d" % li]).value, P(outs["db%d" % li]).value
            a.rowlen, a.nchunk, a.c_out = (1 if w == "rowlen=1" else 5), 3, 4
            a.adam_w, a.adam_b = (0, 1) if li == 0 else (-1, -1)
        if w == "tensor referred twice":
            larr[0].adam_b = 0
        if w == "index out of range":
            larr[0].adam_w = 2
        if w == "weight size mismatch":
            arr[0].n = 15
        if w == "bias size mismatch":
            arr[1].n = 5
        return lib.dcll_grad_reduce_adam(larr, nl, arr, len(sizes), None, st), outs
    assert e == "vote", e
    T, B, N = 3, 8, 65
    outs.update(clout=full(T * B, torch.int32), vote=full(B, torch.int32))
    return lib.dcll_argmax_vote(P(zeros(T * B * N)), P(outs["clout"]), P(outs["vote"]), T, B, N, 0, st), outs


@pytest.mark.parametrize("case", REFUSE, ids=_ids(REFUSE))
def test_refusals(dev, case):
    """Ordinary error returns before any launch: the right code, dcll_last_error() names the reason, the launch log is empty and every
    output — sentinel-filled, of the size the call would write if it ran — is untouched."""
    from snn_modulation_classification_amd import _lib, ops
    with ops.kernel_trace() as tr:
        rc, outs = refusal_call(case, dev)
    msg = _lib.get().dcll_last_error().decode()
    torch.cuda.synchronize()
    print("rc %d, message %r" % (rc, msg))
    assert rc == getattr(_lib, case["code"]), (rc, msg)
    assert case["phrase"] in msg, msg
    assert tr.names == [], tr.names
    for k, t in outs.items():
        assert bool((t == _sent(t.dtype)).all()), (case["id"], k, "was written")


def test_every_reachable_variant_served_a_case():
    """Coverage is asserted, not hoped for: every key of tail_cases.reachable_variants() was served by at least one case that ran to
    the end.  Prints the per-key counts, the seconds per stratum and the largest error of a continuous draw per GEMM form."""
    every = {c["id"] for c in CASES}
    if RAN != every:
        pytest.skip("depends on the case tests of this file having run (and passed) in the same process: %d of %d cases did"
                    % (len(RAN & every), len(every)))
    print("variant key: cases served (of %d)" % len(CASES))
    for key, n in sorted(SERVED.items(), key=lambda kv: tuple(map(str, kv[0]))):
        print("  %-44s %4d" % (" ".join(str(k) for k in key), n))
    print("seconds (references on the host, uploads, device calls, comparisons): " + ", ".join("%s %.1f" % kv for kv in sorted(TIMES.items())))
    print("largest |err| of a continuous draw per GEMM form (contract %.1e):" % LOGIT_TOL)
    for key, e in sorted(WORST.items(), key=lambda kv: tuple(map(str, kv[0]))):
        print("  %-44s %.3g" % (" ".join(str(k) for k in key), e))
    missing = [k for k in TC.reachable_variants() if SERVED[k] == 0]
    assert not missing, missing
    assert set(SERVED) <= set(TC.reachable_variants())
