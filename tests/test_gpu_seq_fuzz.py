"""Seeded differential tests of the fused all-T sequence C ABI — dcll_conv_lif_sequence, dcll_conv_lif_sequence_cells,
dcll_conv_lif_sequence_iq, dcll_dense_lif_sequence — through snn_modulation_classification_amd.ops (the binding the product uses),
on the cases of tests/seq_fuzz_cases.py (proven on the CPU by tests/test_seq_fuzz_cases.py): one case per reachable template
variant of every launcher, the dispatch boundaries, carried state over consecutive calls, border / seam inputs, grids beyond
residency, free draws, refusals.

Every call of every case against the pinned-order C oracle stepping on, every sample (a grid case's device sample i is a copy of
oracle sample i % B_checked): v bit for bit where it is wanted (un-pooled for the (1,3) layers), packed spikes unpacked == the
oracle's (pooled), eps0 / eps1 / arp after each call bit for bit, pv within 2e-6, a presigmoid buffer == the oracle's v bit for bit
(its (1,2) max where the layer pools), fused-readout and dense logits within 1e-4 of a float64 matmul of the oracle's pv, the pv
statistics == numpy's count on the device's own pv buffer, the launch log == expected_kernels().  int8 cases also equal the call on
the dequantised fp32 tensor, IQ cases the cells call on what ops.iq_encode produces, bit for bit.

Outputs a case asks for go through caller buffers with a sentinel-filled tail behind them (the binding takes spk / pv / logits
buffers): the tail must stay untouched.  An output that is NOT asked for crosses the binding as NULL — ops has no way to hand a
buffer it does not want written — so "untouched" is asserted on the refusals, where every buffer is sentinel-filled and the call
goes through _lib directly.

The last test asserts that every reachable variant key of every launcher was served by a case that ran to the end."""
import collections
import ctypes
import time

import numpy as np
import pytest
import torch

import seq_fuzz_cases as SF

pytestmark = pytest.mark.gpu

CASES = SF.cases()
REFUSE = SF.refusals()
STRATA = collections.defaultdict(list)
for _c in CASES:
    STRATA[_c["stratum"]].append(_c)

PV_TOL = 2e-6           # the project's (test_options_through_the_c_abi_vs_oracle)
LOGIT_TOL = 1e-4        # the header's readout contract
GUARD = 64              # sentinel elements behind every caller buffer
SENT_F, SENT_I = -7.25, 0x5a5a5a5a

SERVED = collections.Counter()          # variant key -> number of cases that ran to the end with a call on it
RAN = set()
TIMES = collections.Counter()           # seconds: oracle (tensors + C oracle), gpu (calls, copies, comparisons)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def up(a, dev, B=None, axis=0):
    """numpy -> device tensor; B: the batch axis is expanded to B samples, sample i = sample i % (its size)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if B is not None and t.shape[axis] != B:
        t = t.index_select(axis, torch.arange(B, device=dev) % t.shape[axis])
    return t.contiguous()


def guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENT_I if dtype == torch.int32 else SENT_F, device=dev, dtype=dtype)
    return buf[:n].view(shape), buf


def guard_intact(buf):
    return bool((buf[-GUARD:] == (SENT_I if buf.dtype == torch.int32 else SENT_F)).all())


def chunks(got, ref, axis):
    """device batch in blocks of the oracle's batch: (got block, ref block) pairs along `axis`"""
    B, Bc = got.shape[axis], ref.shape[axis]
    for j in range(0, B, Bc):
        n = min(Bc, B - j)
        yield j, np.take(got, np.arange(j, j + n), axis=axis), np.take(ref, np.arange(n), axis=axis)


def assert_bits(got, ref, axis, tag):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape[:axis] == ref.shape[:axis] and got.shape[axis + 1:] == ref.shape[axis + 1:], (tag, got.shape, ref.shape)
    for j, g, r in chunks(got, ref, axis):
        if not np.array_equal(g.astype(np.float32).view(np.uint32), r.astype(np.float32).view(np.uint32)):
            bad = np.argwhere(g != r)
            raise AssertionError((tag, "samples from %d" % j, "%d of %d elements differ" % (len(bad), g.size), "first", bad[:4].tolist(),
                                  "max |diff| %.3g" % float(np.abs(g - r).max())))


def assert_close(got, ref, axis, tol, tag):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape[:axis] == ref.shape[:axis] and got.shape[axis + 1:] == ref.shape[axis + 1:], (tag, got.shape, ref.shape)
    worst = 0.0
    for j, g, r in chunks(got, ref, axis):
        worst = max(worst, float(np.abs(g.astype(np.float64) - r).max()))
    print("%s: max |err| %.3g (tolerance %.3g)" % (tag, worst, tol))
    assert worst <= tol, (tag, worst)


def check_lowhigh(c, counts, pv_host, steps, tag):
    """the counters of the first / last of the 19 bins == numpy's count on the device's OWN pv buffer (the sigmoid is not
    bit-pinned).  A presigmoid buffer holds v and the sigmoid runs inside the counting pass: the count lies between numpy's counts
    at the bin edge moved by the sigmoid's tolerance either way."""
    counts = counts.cpu().numpy()
    assert counts.shape == (len(steps), 2), (tag, counts.shape, steps)
    edges = np.linspace(0, 1, 20)
    for k, t in enumerate(steps):
        if not c["presigmoid"]:
            hst = np.histogram(pv_host[t], bins=edges)[0]
            assert (int(counts[k, 0]), int(counts[k, 1])) == (int(hst[0]), int(hst[-1])), (tag, k, t)
        else:
            pv = 1.0 / (1.0 + np.exp(-pv_host[t].astype(np.float64)))
            lo = (int((pv < edges[1] - PV_TOL).sum()), int((pv < edges[1] + PV_TOL).sum()))
            hi = (int((pv >= edges[18] + PV_TOL).sum()), int((pv >= edges[18] - PV_TOL).sum()))
            assert lo[0] <= counts[k, 0] <= lo[1] and hi[0] <= counts[k, 1] <= hi[1], (tag, k, t, counts[k], lo, hi)
    return int(counts.sum())


def conv_desc(c):
    from snn_modulation_classification_amd import ops
    lay = SF.LAYERS[c["layer"]]
    d = ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), lay["k"], lay["pad"], lay["pool"], 24 if c["n_ro"] else c["target"],
                           c["n_ro"] == 48, True, 1.0 if c["refractory"] else 0.0, c.get("alpharp", SF.ALPHARP))
    assert ops.conv_out_shape(d) == SF.out_shape(c)
    return d


def conv_calls(c, T, dev, dequantised=False, cells_from_encoder=False):
    """all calls of a conv case on one set of state buffers -> per call dict(host copies of the outputs and of the state after the
    call, launch log)"""
    from snn_modulation_classification_amd import ops
    d = conv_desc(c)
    B, cin, cout, h, w = c["B"], c["c_in"], c["c_out"], c["h"], c["w"]
    ch, cw, ph, pw = SF.out_shape(c)
    W, q8 = up(T["W"], dev), None
    if T["q8"] is not None and not dequantised:
        W, q8 = None, (up(T["q8"][0], dev), up(T["q8"][1], dev))
    b, tau4 = up(T["b"], dev), up(np.stack(T["tau"]), dev)
    eps0, eps1 = up(T["eps0"], dev, B), up(T["eps1"], dev, B)
    arp = up(T["arp"], dev, B) if c["refractory"] else None
    ro = {}
    if c["n_ro"]:
        ro = dict(ro_Wp=ops.permute_readout(up(T["ro_W"], dev)), ro_b=up(T["ro_b"], dev))
    iq = tab = None
    if c["entry"] == "iq":
        iq = up(T["iq"], dev, B)
        tab = {k: up(v, dev, B if k == "mask" else None) for k, v in T["tab"].items()}
    res, t_off, iter0 = [], c["t0"], c["lowhigh_iter0"]
    for k, (T_, call) in enumerate(zip(c["Ts"], T["calls"])):
        out, bufs = {}, []
        if c["want_spikes"]:
            out["spk"], g = guarded((T_, B, cout, ph * pw // 32), torch.int32, dev)
            bufs.append(g)
        if c["want_pv"]:
            out["pv"], g = guarded((T_, B, cout, ph, pw), torch.float32, dev)
            bufs.append(g)
        if c["n_ro"]:
            out["ro"], g = guarded((T_, B, c["n_ro"]), torch.float32, dev)
            bufs.append(g)
        kw = dict(want_spikes=bool(c["want_spikes"]), want_pv=bool(c["want_pv"]), want_v=bool(c["want_v"]), out=out,
                  lowhigh_iter0=iter0, q8=q8, presigmoid=bool(c["presigmoid"]))
        if c["entry"] == "seq":
            inp = ops.pack_spikes(up(call["x"].reshape(T_, c["B_checked"], cin, h * w), dev, B, 1))
        elif c["entry"] == "cells" or cells_from_encoder:
            inp = up(call["cells"], dev, B, 1)
            if cells_from_encoder:
                enc = ops.iq_encode(iq, tab["thr_i"], tab["thr_q"], t_off, T_, w, h,
                                    tail=(tab["thr_i_tail"], tab["thr_q_tail"], tab["mask"]))
                assert torch.equal(enc, inp), (c["id"], "call %d" % k, "ops.iq_encode != the threshold count in numpy")
                inp = enc
        with ops.kernel_trace() as tr:
            if c["entry"] == "seq":
                got = ops.conv_lif_sequence(d, inp, W, b, tau4, eps0, eps1, arp, T_, B, **kw, **ro)
            elif c["entry"] == "cells" or cells_from_encoder:
                got = ops.conv_lif_sequence_cells(d, inp, W, b, tau4, eps0, eps1, arp, T_, B, **kw)
            else:
                got = ops.conv_lif_sequence_iq(d, iq, tab["thr_i"], tab["thr_q"], t_off, W, b, tau4, eps0, eps1, arp, T_, B,
                                               tail=(tab["thr_i_tail"], tab["thr_q_tail"], tab["mask"]), **kw)
        torch.cuda.synchronize()
        spk, pv, v = got[:3]
        assert (spk is None) == (not c["want_spikes"]) and (pv is None) == (not c["want_pv"]) and (v is None) == (not c["want_v"])
        assert all(guard_intact(g) for g in bufs), (c["id"], "call %d" % k, "a write behind the end of an output buffer")
        host = lambda t: None if t is None else t.detach().cpu().numpy()
        r = dict(names=tr.names, pv=host(pv), v=host(v), ro=host(got[3]) if c["n_ro"] else None, lowhigh=out.get("lowhigh"),
                 spk=None if spk is None else host(ops.unpack_spikes(spk)).reshape(T_, B, cout, ph, pw),
                 eps0=host(eps0), eps1=host(eps1), arp=host(arp), iter0=iter0)
        res.append(r)
        t_off += T_
        if iter0 is not None:
            iter0 += T_
    return res


def check_conv(c, T, traj, res):
    nstat = 0
    for k, (T_, o, g) in enumerate(zip(c["Ts"], traj, res)):
        tag = (c["id"], "call %d (T %d)" % (k, T_))
        assert g["names"] == SF.expected_kernels(c, T_, g["iter0"]), tag + (g["names"], SF.expected_kernels(c, T_, g["iter0"]))
        assert_bits(g["eps0"], o["eps0"], 0, tag + ("eps0",))
        assert_bits(g["eps1"], o["eps1"], 0, tag + ("eps1",))
        if c["refractory"]:
            assert_bits(g["arp"], o["arp"], 0, tag + ("arp",))
        if c["want_v"]:
            assert_bits(g["v"], o["v"], 1, tag + ("v",))
        if c["want_spikes"]:
            assert_bits(g["spk"], o["s"], 1, tag + ("spikes",))
        if c["want_pv"] and c["presigmoid"]:
            ov = o["v"] if c["layer"] == "k7" else np.maximum(o["v"][..., 0::2], o["v"][..., 1::2])
            assert_bits(g["pv"], ov, 1, tag + ("presigmoid buffer",))
        elif c["want_pv"]:
            assert_close(g["pv"], o["pv"], 1, PV_TOL, tag + ("pv",))
        if c["n_ro"]:
            p64 = o["pv"].astype(np.float64).reshape(T_, c["B_checked"], -1) @ T["ro_W"].astype(np.float64).T + T["ro_b"].astype(np.float64)
            assert_close(g["ro"], p64, 1, LOGIT_TOL, tag + ("fused readout",))
        steps = SF.hist_steps(g["iter0"], T_)
        if g["iter0"] is not None:
            nstat += check_lowhigh(c, g["lowhigh"], g["pv"].reshape(T_, -1), steps, tag)
    return nstat


def assert_same_calls(a, b, what, cid):
    for k, (x, y) in enumerate(zip(a, b)):
        for key in ("v", "spk", "pv", "ro", "eps0", "eps1", "arp"):
            assert (x[key] is None) == (y[key] is None)
            if x[key] is not None:
                assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), (cid, what, "call %d" % k, key)


def dense_calls(c, T, dev):
    from snn_modulation_classification_amd import ops
    B = c["B"]
    d = ops.DenseDesc(c["in_features"], c["out_features"], c["target"], c["tau_tensor"], c["refractory"], c.get("alpharp", SF.ALPHARP),
                      1.0 if c["refractory"] else 0.0)
    W, b, tau = up(T["W"], dev), up(T["b"], dev), [up(t, dev) for t in T["tau"]]
    eps0, eps1 = up(T["eps0"], dev, B), up(T["eps1"], dev, B)
    arp = up(T["arp"], dev, B) if c["refractory"] else None
    i2o_W, i2o_b = up(T["ro_W"], dev), up(T["ro_b"], dev)
    res = []
    for T_, call in zip(c["Ts"], T["calls"]):
        x = up(call["x"], dev, B, 1)
        with ops.kernel_trace() as tr:
            s, p, pv, v = ops.dense_lif_sequence(d, x, W, b, *tau, eps0, eps1, arp, i2o_W, i2o_b, want_s=bool(c["want_spikes"]),
                                                 want_v=bool(c["want_v"]))
        torch.cuda.synchronize()
        assert (s is None) == (not c["want_spikes"]) and (v is None) == (not c["want_v"])
        host = lambda t: None if t is None else t.detach().cpu().numpy()
        res.append(dict(names=tr.names, s=host(s), p=host(p), pv=host(pv), v=host(v), eps0=host(eps0), eps1=host(eps1), arp=host(arp)))
    return res


def check_dense(c, T, traj, res):
    for k, (T_, o, g) in enumerate(zip(c["Ts"], traj, res)):
        tag = (c["id"], "call %d (T %d)" % (k, T_))
        assert g["names"] == SF.expected_kernels(c, T_), tag + (g["names"][-3:], SF.expected_kernels(c, T_)[-3:])
        assert_bits(g["eps0"], o["eps0"], 0, tag + ("eps0",))
        assert_bits(g["eps1"], o["eps1"], 0, tag + ("eps1",))
        if c["refractory"]:
            assert_bits(g["arp"], o["arp"], 0, tag + ("arp",))
        if c["want_v"]:
            assert_bits(g["v"], o["v"], 1, tag + ("v",))
        if c["want_spikes"]:
            assert_bits(g["s"], o["s"], 1, tag + ("spikes",))
        assert_close(g["pv"], o["pv"], 1, PV_TOL, tag + ("pv",))
        p64 = o["pv"].astype(np.float64) @ T["ro_W"].astype(np.float64).T + T["ro_b"].astype(np.float64)
        assert_close(g["p"], p64, 1, LOGIT_TOL, tag + ("p",))


def run_case(c, dev):
    print(SF.describe(c))
    t0 = time.time()
    T, traj = SF.run(c)
    TIMES["oracle"] += time.time() - t0
    t0 = time.time()
    keys = [SF.variant(c, T_) for T_ in c["Ts"]]
    print("variants:", keys)
    if c["entry"] == "dense":
        check_dense(c, T, traj, dense_calls(c, T, dev))
    else:
        res = conv_calls(c, T, dev)
        nstat = check_conv(c, T, traj, res)
        if c["id"].startswith("seq-edge-lowhigh") and any(SF.hist_steps(g["iter0"], T_) for g, T_ in zip(res, c["Ts"])):
            assert nstat > 0, (c["id"], "no pv value in the first or the last bin")
        if c["q8"]:
            assert_same_calls(res, conv_calls(c, T, dev, dequantised=True), "int8 weights vs the dequantised fp32 tensor", c["id"])
        if c["entry"] == "iq":
            twin = conv_calls(c, T, dev, cells_from_encoder=True)
            assert_same_calls(res, twin, "IQ window vs the cells of ops.iq_encode", c["id"])
            for g, T_ in zip(twin, c["Ts"]):             # (the twin ran the cells form of the same kernel)
                assert g["names"][0] == SF.variant(dict(c, entry="cells"), T_)[0]
    TIMES["gpu"] += time.time() - t0
    RAN.add(c["id"])
    SERVED.update(set(keys))


def _ids(cs):
    return [c["id"] for c in cs]


@pytest.mark.parametrize("case", STRATA["variants"], ids=_ids(STRATA["variants"]))
def test_every_template_variant(dev, case):
    run_case(case, dev)


@pytest.mark.parametrize("case", STRATA["boundaries"], ids=_ids(STRATA["boundaries"]))
def test_dispatch_boundaries(dev, case):
    run_case(case, dev)


@pytest.mark.parametrize("case", STRATA["carry"], ids=_ids(STRATA["carry"]))
def test_carried_state_over_consecutive_calls(dev, case):
    run_case(case, dev)


@pytest.mark.parametrize("case", STRATA["inputs"], ids=_ids(STRATA["inputs"]))
def test_border_and_seam_inputs(dev, case):
    run_case(case, dev)


@pytest.mark.parametrize("case", STRATA["grids"], ids=_ids(STRATA["grids"]))
def test_grids_beyond_residency(dev, case):
    run_case(case, dev)


@pytest.mark.parametrize("case", STRATA["free"], ids=_ids(STRATA["free"]))
def test_free_draws(dev, case):
    run_case(case, dev)


@pytest.mark.parametrize("case", REFUSE, ids=_ids(REFUSE))
def test_refusals(dev, case):
    """Ordinary error returns before any launch: the right code, dcll_last_error() names the reason, the launch log is empty and
    every output and state buffer — sentinel-filled, of the size the call would write if it ran — is untouched.  T = 0 and B = 0
    return DCLL_OK and touch nothing."""
    from snn_modulation_classification_amd import _lib, ops
    lib, P, r = _lib.get(), _lib.ptr, case
    print(SF.describe(r))
    T, B = max(r["T"], 1), max(r["B"], 1)             # (buffers as for a call of at least one step and sample)
    cin, cout, h, w = r["c_in"], r["c_out"], r["h"], r["w"]
    d = _lib.ConvDesc(cin, cout, h, w, r["kh"], r["kw"], r["pad_h"], r["pad_w"], r["stride"], r["dilation"], r["groups"], r["pool_h"],
                      r["pool_w"], 24, 0, 1, 1, SF.ALPHARP, 1.0)
    words = -(-h * w // 32)
    full = lambda n, dt=torch.float32: torch.full((int(n) + 2,), SENT_I if dt != torch.float32 else SENT_F, device=dev, dtype=dt)
    st = {k: full(B * n * h * w) for k, n in (("eps0", cin), ("eps1", cin), ("arp", cout))}
    outs = dict(spk=full(T * B * cout * words, torch.int32), pv=full(T * B * cout * h * w), v=full(T * B * cout * h * w),
                ro=full(T * B * 48), scratch=full(2 * B * cin * h * w))
    off = lambda t: t[1:] if r["off4"] else t[2:]       # (allocations are 16-byte aligned: one element in = a 4-byte offset, two = 8)
    zeros = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
    Wt, b, tau4 = zeros(cout, cin, r["kh"], r["kw"]), zeros(cout), zeros(4, cin) + .9
    n_ro = r["n_ro"]
    ro_Wp, ro_b = (zeros(n_ro * cout * h * w), zeros(n_ro)) if n_ro else (None, None)
    opts = None
    if r["presigmoid"] or r["q8_no_scale"]:
        opts = _lib.LayerOpts()
        opts.pv_presigmoid = r["presigmoid"]
        if r["q8_no_scale"]:
            q = zeros(cout, cin, r["kh"], r["kw"], dt=torch.int8)
            opts.w_q8 = q.data_ptr()
        opts = ctypes.byref(opts)
    arp = None if r["no_arp"] else P(off(st["arp"]))
    scratch = None if r["no_scratch"] else P(outs["scratch"])
    spk = P(off(outs["spk"]))
    with ops.kernel_trace() as tr:
        if r["entry"] == "seq":
            inp = zeros(T, B, cin, words, dt=torch.int32)
            rc = lib.dcll_conv_lif_sequence(ctypes.byref(d), P(inp), P(Wt), P(b), P(tau4), P(off(st["eps0"])), P(off(st["eps1"])), arp,
                                            spk, P(outs["pv"]), P(off(outs["v"])), P(ro_Wp), P(ro_b), P(outs["ro"]) if n_ro else None,
                                            n_ro, scratch, None, 0, opts, r["T"], r["B"], None)
        else:
            inp = zeros(T, B, dt=torch.int32)
            rc = lib.dcll_conv_lif_sequence_cells(ctypes.byref(d), P(inp), P(Wt), P(b), P(tau4), P(off(st["eps0"])), P(off(st["eps1"])),
                                                  arp, spk, P(outs["pv"]), P(off(outs["v"])), scratch, None, 0, opts, r["T"], r["B"],
                                                  None)
    msg = lib.dcll_last_error().decode()
    torch.cuda.synchronize()
    print("rc %d, message %r" % (rc, msg))
    assert rc == getattr(_lib, r["code"]), (rc, msg)
    if rc:
        assert r["phrase"] in msg, msg
    assert tr.names == [], tr.names
    for k, t in list(st.items()) + list(outs.items()):
        assert bool((t == (SENT_I if t.dtype == torch.int32 else SENT_F)).all()), (r["id"], k, "was written")


def test_every_reachable_variant_served_a_case():
    """Coverage is asserted, not hoped for: every key of the reachable product of every launcher's switches
    (seq_fuzz_cases.reachable_variants) was served by at least one case that ran to the end."""
    every = {c["id"] for c in CASES}
    if RAN != every:
        pytest.skip("depends on the case tests of this file having run (and passed) in the same process: %d of %d cases did"
                    % (len(RAN & every), len(every)))
    print("variant key: cases served (of %d)" % len(CASES))
    for key, n in sorted(SERVED.items()):
        print("  %-44s %4d" % (" ".join(str(k) for k in key), n))
    print("seconds: tensors + C oracle %.1f, device calls + copies + comparisons %.1f" % (TIMES["oracle"], TIMES["gpu"]))
    missing = [k for k in SF.reachable_variants() if SERVED[k] == 0]
    assert not missing, missing
    assert set(SERVED) <= set(SF.reachable_variants())
