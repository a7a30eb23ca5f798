"""dcll_conv_lif_sequence_bands (k_lif_seq_band) on the GPU: the fused all-T kernel of a plain conv layer with several workgroups
per sample, each on a band of output rows, against the pinned-order C oracle stepped T times — case list tests/seq_band_cases.py
(proven on the CPU by tests/test_seq_band_cases.py) — against dcll_conv_lif_sequence_wide wherever that serves the layer, and the
network level above it: ConvNetwork.test_sequence_any(bands=...) against bands=None and the per-step loop, train.py
--band_sequence_path.  Helpers and tolerances: tests/test_gpu_seq_any.py.

v is compared bit for bit up to the sign of a zero against the oracle — and bit for bit, signs included, against the
one-workgroup kernel; pooled spikes and eps0 / eps1 / arp after every call bit for bit; pv within 1e-4.  spk_out is handed in
filled with 0xFFFFFFFF (a boundary word is ORed into: the launcher's zero fill, or a stored word, must have replaced every one),
and every output buffer sits in front of a sentinel tail."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import seq_band_cases as S
import seq_wide_cases as W
import test_gpu_seq_any as G

pytestmark = pytest.mark.gpu
LOGIT_TOL, PV_TOL = G.LOGIT_TOL, G.PV_TOL
CASES = S.cases()
REFUSE = S.refusals()
SERVED = collections.Counter()
TAIL, SENT = 64, 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _operands(c, dev):
    """device tensors of a case: weights, bias, time constants, the initial state tiled to B samples"""
    T_, traj = S.run(c)
    B = c["B"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    op = dict(W=cu(T_["W"]), b=(cu(T_["b"]) if T_["b"] is not None else None), tau4=cu(np.stack(T_["tau"]).astype(np.float32)),
              eps0=cu(G._tile(T_["eps0"], B, 0)), eps1=cu(G._tile(T_["eps1"], B, 0)),
              arp=cu(G._tile(T_["arp"], B, 0)) if c["refractory"] else None)
    calls = []
    for call in T_["calls"]:
        n = call["x"].shape[0]
        x = G._tile(call["x"], B, 1).reshape(n, B, c["c_in"], c["h"] * c["w"])
        calls.append((n, cu(S.pack_planes(x).view(np.int32))))
    return op, calls, traj


def _tailed(shape, dtype, fill, dev):
    """a buffer of `shape` in front of TAIL sentinel elements -> (the view, the tail)"""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), fill, device=dev, dtype=dtype)
    return buf[:n].view(shape), buf[n:]


def _call(c, op, n, spk_in, dev, entry="bands", bands=None):
    """one call through the C ABI on buffers with sentinel tails, spk_out handed in as 0xFFFFFFFF -> ((spk, pv, v), launch log)"""
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = G._desc(c)
    B = c["B"]
    ch, cw, ph, pw = S.out_shape(c)
    bands = c["bands"] if bands is None else bands
    spk, t_spk = _tailed((n, B, c["c_out"], (ph * pw + 31) // 32), torch.int32, -1, dev)
    pv, t_pv = _tailed((n, B, c["c_out"], ph, pw), torch.float32, SENT, dev)
    v, t_v = _tailed((n, B, c["c_out"], ch, cw), torch.float32, SENT, dev)
    ns = int(lib.dcll_conv_lif_sequence_bands_scratch(ctypes.byref(d), B)) if entry == "bands" else \
        int(lib.dcll_conv_lif_sequence_wide_scratch(ctypes.byref(d)))
    assert ns > 0
    scratch, t_scr = _tailed((ns,), torch.float32, SENT, dev)
    p = _lib.ptr
    with ops.kernel_trace() as tr:
        if entry == "bands":
            rc = lib.dcll_conv_lif_sequence_bands(ctypes.byref(d), p(spk_in), p(op["W"]), p(op["b"]), p(op["tau4"]), p(op["eps0"]),
                                                  p(op["eps1"]), p(op["arp"]), p(spk), p(pv), p(v), p(scratch), n, B, bands,
                                                  _lib.stream_ptr())
        else:
            rc = lib.dcll_conv_lif_sequence_wide(ctypes.byref(d), p(spk_in), p(op["W"]), p(op["b"]), p(op["tau4"]), p(op["eps0"]),
                                                 p(op["eps1"]), p(op["arp"]), p(spk), p(pv), p(v), p(scratch), n, B, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.DCLL_OK, (c["id"], rc, lib.dcll_last_error())
    assert bool((t_spk == -1).all()) and all(bool((t == SENT).all()) for t in (t_pv, t_v, t_scr)), (c["id"], "a sentinel tail was written")
    return (spk, pv, v), list(tr.names)


def run_case(c, dev):
    """every call of a case on the device against the oracle's trajectory -> host copies of every call's outputs and state"""
    from snn_modulation_classification_amd import ops
    op, calls, traj = _operands(c, dev)
    outs = []
    B = c["B"]
    ch, cw, ph, pw = S.out_shape(c)
    for k, ((n, spk_in), ref) in enumerate(zip(calls, traj)):
        (spk, pv, v), names = _call(c, op, n, spk_in, dev)
        assert names == S.launch_log(c), (c["id"], names)
        tag = (c["id"], "call %d" % k)
        G._same(v, ref["v"], 1, tag + ("v",), zero_sign=True)
        G._same(ops.unpack_spike_planes(spk.contiguous(), ph * pw).reshape(n, B, c["c_out"], ph, pw), ref["s"], 1, tag + ("spikes",))
        got_pv = pv.cpu().numpy()
        Bc = ref["pv"].shape[1]
        worst = max(float(np.abs(got_pv[:, j:j + Bc] - ref["pv"][:, :B - j]).max()) for j in range(0, B, Bc))
        assert worst <= PV_TOL, tag + ("pv", worst)
        if (ph * pw) % 32:          # tail bits of the last word are zero
            assert not bool((spk[..., -1].cpu().numpy().view(np.uint32) >> np.uint32((ph * pw) % 32)).any()), tag
        G._same(op["eps0"], ref["eps0"], 0, tag + ("eps0",))
        G._same(op["eps1"], ref["eps1"], 0, tag + ("eps1",))
        if c["refractory"]:
            G._same(op["arp"], ref["arp"], 0, tag + ("arp",))
        outs.append([t.cpu().numpy().copy() for t in (spk, pv, v, op["eps0"], op["eps1"]) + ((op["arp"],) if c["refractory"] else ())])
    SERVED[S.variant(c)] += 1
    return outs


def _run_plain(c, dev, entry, bands=None):
    """every call of a case through one entry point -> (host copies of every output and of the state after every call, logs)"""
    op, calls, _ = _operands(c, dev)
    outs, logs = [], []
    for n, spk_in in calls:
        res, names = _call(c, op, n, spk_in, dev, entry, bands)
        logs.append(names)
        outs.append([t.cpu().numpy().copy().view(np.uint32) for t in res + tuple(op[k] for k in ("eps0", "eps1", "arp") if op[k] is not None)])
    return outs, logs


# ---------------------------------------------------------------------------------------------- the case list
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle(dev, case):
    """every case (named layers, edges, boundaries, the B = 300 x 4 bands grid beyond residency — two consecutive calls, all 300
    samples compared —, forwarded calls, free draws) with the launch log the restated dispatch predicts; where the one-workgroup
    kernel serves the layer too, every output and the state after every call equal its, bit for bit, v and pv included"""
    mine = run_case(case, dev)
    if W.lds_bytes(case) > 0:
        theirs, _ = _run_plain(case, dev, "wide")
        for k, (a, b) in enumerate(zip(mine, theirs)):
            for name, x, y in zip(("spk", "pv", "v", "eps0", "eps1", "arp"), a, b):
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), y), (case["id"], "call %d" % k, name, "differs from dcll_conv_lif_sequence_wide")


def test_a_second_run_is_bit_identical(dev):
    """one case per template instance, and every case with a shared spike word (the ORs commute), run twice from the same state:
    every output and the state after every call equal bit for bit"""
    seen, picked = set(), []
    for c in CASES:
        n = S.band_count(c)
        if n > 1 and (S.variant(c) not in seen or (c["stratum"] == "edges" and S.shared_words(c, n))):
            seen.add(S.variant(c))
            picked.append(c)
    assert seen == set(S.all_variants())
    for c in picked:
        a, la = _run_plain(c, dev, "bands")
        b, lb = _run_plain(c, dev, "bands")
        assert la == lb == [S.launch_log(c)] * len(c["Ts"]), (c["id"], la)
        assert all(np.array_equal(x, y) for ca, cb in zip(a, b) for x, y in zip(ca, cb)), c["id"]


def test_every_template_instance_served_a_case(dev):
    """all eight instances k_lif_seq_band<MT,R,WLDS> serve a case to the end: the first case of each is run HERE, its launch log
    read back"""
    here = collections.Counter()
    for c in CASES:
        if S.band_count(c) > 1 and not here[S.variant(c)]:
            run_case(c, dev)
            here[S.variant(c)] += 1
    assert set(here) == set(S.all_variants()), dict(here)
    print("\n".join("%-28s %4d" % (k, SERVED[k]) for k in S.all_variants()))


def test_forwarded_calls_are_the_siblings(dev):
    """bands = 1, and bands = 0 where the rule picks one band: dcll_conv_lif_sequence_wide's launch log (k_lif_seq_any's up to 32
    channels) and bits"""
    for c in CASES:
        if c["stratum"] != "forwarded":
            continue
        a, la = _run_plain(c, dev, "bands")
        b, lb = _run_plain(c, dev, "wide")
        assert la == lb == [W.launch_log(c)] * len(c["Ts"]), (c["id"], la, lb)
        assert all(np.array_equal(x, y) for ca, cb in zip(a, b) for x, y in zip(ca, cb)), c["id"]


def test_ops_wrapper_reuses_one_scratch_buffer(dev):
    """ops.conv_lif_sequence_bands: the results of the C call, its scratch kept under 'band_scratch' and reused"""
    from snn_modulation_classification_amd import ops
    c = S.by_id("band-edge-pw11")
    ref, _ = _run_plain(c, dev, "bands")
    op, calls, _ = _operands(c, dev)
    bufs = {}
    for k, (n, spk_in) in enumerate(calls):
        with ops.kernel_trace() as tr:
            spk, pv, v = ops.conv_lif_sequence_bands(G._desc(c), spk_in, op["W"], op["b"], op["tau4"], op["eps0"], op["eps1"], op["arp"],
                                                     n, c["B"], want_v=True, out=bufs, bands=c["bands"])
        assert list(tr.names) == S.launch_log(c)
        assert all(np.array_equal(t.cpu().numpy().view(np.uint32), r) for t, r in zip((spk, pv, v), ref[k]))
        assert bufs["band_scratch"].numel() == S.scratch_floats(c) and "w_scratch" not in bufs
        first = bufs["band_scratch"] if k == 0 else first
        assert bufs["band_scratch"] is first


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("r", REFUSE, ids=[r["id"] for r in REFUSE])
def test_refusal(dev, r):
    """the code, a phrase of dcll_last_error(), an empty launch log, nothing written"""
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = G._desc(r)
    T, B = r["T"], r["B"]
    Tn, Bn = max(T, 1), max(B, 1)
    ch, cw, ph, pw = S.out_shape(r) if S.valid(r) else (1, 1, 1, 1)
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(spk_in=torch.zeros((Tn, Bn, r["c_in"], (r["h"] * r["w"] + 31) // 32), device=dev, dtype=torch.int32),
             W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]), tau4=f(4, r["c_in"]),
             eps0=f(Bn, r["c_in"], r["h"], r["w"]), eps1=f(Bn, r["c_in"], r["h"], r["w"]), arp=f(Bn, r["c_out"], ch, cw),
             spk=torch.full((Tn, Bn, r["c_out"], (ph * pw + 31) // 32), 77, device=dev, dtype=torch.int32),
             pv=f(Tn, Bn, r["c_out"], ph, pw), v=f(Tn, Bn, r["c_out"], ch, cw),
             scratch=f(128 * S.steps(r) + 2 * Bn * r["c_in"] * r["h"] * r["w"] + 128))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_sequence_bands(ctypes.byref(d), p["spk_in"], p["W"], p["b"], p["tau4"], p["eps0"], p["eps1"], p["arp"],
                                              p["spk"], p["pv"], p["v"], p["scratch"], T, B, r["bands"], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode(), (r["id"], lib.dcll_last_error())
    assert tr.names == [], (r["id"], tr.names)
    for k in ("eps0", "eps1", "arp", "pv", "v", "scratch"):
        assert bool((t[k] == SENT).all()), (r["id"], k, "was written")
    assert bool((t["spk"] == 77).all())
    if r["code"] == "DCLL_ERR_UNSUPPORTED":
        assert not ops.sequence_bands_supported(d, r["bands"]) and ops.sequence_bands_plan(d, Bn, r["bands"]) is None


# ---------------------------------------------------------------------------------------------- networks
def _state_equal(a, b):
    for sa, sb in zip(a.dcll_slices, b.dcll_slices):
        for u, v in zip(sa.dclllayer.i2h.state, sb.dclllayer.i2h.state):
            assert torch.equal(u, v)


def _results_equal(ra, rb, n=3):
    for i in range(n):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and torch.equal(ra["logits"][i], rb["logits"][i]), i
        assert torch.equal(ra["clout"][i], rb["clout"][i]) and torch.equal(ra["vote"][i], rb["vote"][i]), i
    assert torch.equal(ra["o"], rb["o"])


def _band_names(tr):
    return [n for n in tr.names if n.startswith("k_lif_seq")]


def test_network_radio_ml_netscale2_bands4_equals_one_workgroup(dev):
    """radio_ml_conv.yaml at netscale 2 on 16x16, B = 2, T = 6: test_sequence_any(wide=True, bands=4) == bands=None in logits,
    clout, votes, spikes and state, bit for bit; every layer on k_lif_seq_band"""
    R, T, B = 16, 6, 2
    a, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24, netscale=2.0)
    b, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24, netscale=2.0)
    assert a.sequence_any_supported(wide=True, bands=4) and a.sequence_any_supported(bands=0) and not a.sequence_any_supported(bands=17)
    cells = torch.from_numpy(np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)).to(dev)
    a.reset()
    b.reset()
    with G.ops_trace() as tr:
        ra = a.test_sequence_any(cells, keep_spikes=True, wide=True, bands=4)
    assert _band_names(tr) == ["k_lif_seq_band<2,1,1>", "k_lif_seq_band<2,1,0>", "k_lif_seq_band<2,1,0>"]
    with G.ops_trace() as tr:
        rb = b.test_sequence_any(cells, keep_spikes=True, wide=True)
    assert all(n.startswith("k_lif_seq_wide") for n in _band_names(tr))
    _results_equal(ra, rb)
    _state_equal(a, b)
    assert 0 < float(ops_mean(ra["spikes"][2])) < 1


def ops_mean(packed):
    """share of set bits of a packed spike tensor"""
    x = packed.cpu().numpy().view(np.uint32)
    return np.unpackbits(x.view(np.uint8)).mean()


def _mnist_input(dev, T, B):
    rng = np.random.RandomState(3)
    x = (rng.rand(T, B, 1, 28, 28) < .15).astype(np.float32)
    x[0] = rng.rand(B, 1, 28, 28) < .5
    return torch.from_numpy(x).to(dev)


def test_network_mnist_bands2_equals_one_workgroup(dev):
    """mnist_conv.yaml (pooled widths 13, 11, 4: band boundaries inside spike words), B = 3, T = 6: bands=2 == bands=None"""
    T, B = 6, 3
    a, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    b, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    x = _mnist_input(dev, T, B)
    a.reset()
    b.reset()
    with G.ops_trace() as tr:
        ra = a.test_sequence_any(x, keep_spikes=True, bands=2)
    assert all(n.startswith("k_lif_seq_band<1,0,") for n in _band_names(tr)) and len(_band_names(tr)) == 3
    rb = b.test_sequence_any(x, keep_spikes=True)
    _results_equal(ra, rb)
    _state_equal(a, b)


def _per_step(net, x_steps):
    """the per-step loop net.test(x[t]) beside a slice-by-slice stepping of a twin -> per layer (spikes, logits) over T"""
    spikes, logits = [[] for _ in net.dcll_slices], [[] for _ in net.dcll_slices]
    net.reset()
    with torch.no_grad():
        for t in range(len(x_steps)):
            cur = x_steps[t]
            for i, sl in enumerate(net.dcll_slices):
                L = sl.dclllayer
                s, p, o = L.i2h._step(cur, L.pooling, L.i2o, L.output_ if L.output_layer else None,
                                      stacked=L.stacked_readout() if L.output_layer else None)[:3]
                spikes[i].append(s.cpu().numpy().copy())
                logits[i].append((o if L.output_layer else p).cpu().numpy().copy())
                cur = s
    return [np.stack(s) for s in spikes], [np.stack(l) for l in logits]


def test_network_radio_ml_48x48_is_served_by_bands_alone(dev):
    """radio_ml_conv.yaml on a 48x48 plane, B = 2, T = 4: no one-workgroup path serves it; bands=0 does, and equals the per-step
    loop: spikes of all layers and the final state bit for bit, logits within 1e-4, clout and votes equal (margin rule on the
    per-step logits)"""
    from snn_modulation_classification_amd import _lib, ops
    R, T, B = 48, 4, 2
    net, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24)
    assert not net.sequence_any_supported() and not net.sequence_any_supported(wide=True) and net.sequence_any_supported(wide=True, bands=0)
    cells = torch.from_numpy(np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)).to(dev)
    with pytest.raises(_lib.DCLLUnsupported):
        net.test_sequence_any(cells, wide=True)
    net.reset()
    with G.ops_trace() as tr:
        res = net.test_sequence_any(cells, keep_spikes=True, bands=0)
    assert _band_names(tr) == ["k_lif_seq_band<1,1,1>", "k_lif_seq_band<1,1,0>", "k_lif_seq_band<1,1,0>"]
    assert not any(n.startswith(("k_conv_lif", "k_trace", "k_pool")) for n in tr.names)
    planes = ops.cells_to_planes(cells, R * R).reshape(T, B, 1, R, R)
    twin, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24)
    spikes, logits = _per_step(twin, planes)
    for i in range(3):
        got = ops.unpack_spike_planes(res["spikes"][i], R * R).cpu().numpy().reshape(T, B, 32, R, R)
        assert np.array_equal(got, spikes[i]) and 0 < spikes[i].mean() < 1, ("spikes", i)
        mine = (res["o"] if i == 2 else res["logits"][i]).cpu().numpy()
        assert float(np.abs(mine - logits[i]).max()) <= LOGIT_TOL, ("logits", i)
    _state_equal(net, twin)
    step, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24)
    G._compare_with_per_step(net, res, step, planes, np.arange(B) % 24, 24, logits, max_excluded=.05)
    _state_equal(net, step)


def test_chunked_batch_equals_whole_batch(dev):
    """test_sequence_any(bands=2) under a pv budget that splits the batch (2 + 1 samples) == the whole batch at once"""
    T, B = 6, 3
    x = _mnist_input(dev, T, B)
    whole, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    parts, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    per_sample = 4 * T * max(s.dclllayer.out_channels * int(np.prod(s.dclllayer.output_shape)) for s in parts.dcll_slices)
    parts.pv_budget_bytes = 2 * per_sample + 1
    whole.reset()
    parts.reset()
    ra = whole.test_sequence_any(x, keep_spikes=True, bands=2)
    with G.ops_trace() as tr:
        rb = parts.test_sequence_any(x, keep_spikes=True, bands=2)
    assert sum(n.startswith("k_lif_seq_band") for n in tr.names) == 6
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and ra["spikes"][i].shape[1] == B
        assert float((ra["logits"][i] - rb["logits"][i]).abs().max()) <= 2 * LOGIT_TOL
        assert torch.equal(ra["clout"][i], rb["clout"][i]) and torch.equal(ra["vote"][i], rb["vote"][i])
    _state_equal(whole, parts)


# ---------------------------------------------------------------------------------------------- entry points
def test_entry_point_train_band_sequence_path(tmp_path, capsys):
    """train.py --netscale 2 on synthetic IQ at the 16x16 plane: the periodic test with --band_sequence_path 4 runs k_lif_seq_band
    and reports the accuracies of the same command without the flag (evaluate_batch's per-step loop); it wins over
    --wide_sequence_path; at netscale 1 on 16x16 (the specialised sequence kernels) and with more bands than pooled rows the flag
    is ignored with a notice"""
    import train
    common = ['--I_resolution', '16', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '12',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    with G.ops_trace() as tr:
        out_band = train.main(common + ['--netscale', '2', '--output', str(tmp_path / 'band'), '--band_sequence_path', '4',
                                        '--wide_sequence_path'])
    assert sum(n.startswith("k_lif_seq_band") for n in tr.names) == 3 and not any(n.startswith("k_lif_seq_wide") for n in tr.names)
    assert "ignored" not in capsys.readouterr().out
    with G.ops_trace() as tr:
        out_step = train.main(common + ['--netscale', '2', '--output', str(tmp_path / 'step')])
    assert not any(n.startswith("k_lif_seq_band") for n in tr.names)
    a, b = np.load(os.path.join(out_band, 'acc_test.npy')), np.load(os.path.join(out_step, 'acc_test.npy'))
    assert a.shape == b.shape == (1, 1, 3) and np.isfinite(a).all() and np.array_equal(a, b)
    capsys.readouterr()
    with G.ops_trace() as tr:
        train.main(common + ['--output', str(tmp_path / 'n1'), '--band_sequence_path', '--eval_only'])
    assert "--band_sequence_path ignored: the network runs" in capsys.readouterr().out and not any(n.startswith("k_lif_seq_band") for n in tr.names)
    with G.ops_trace() as tr:
        train.main(common + ['--netscale', '2', '--output', str(tmp_path / 'n17'), '--band_sequence_path', '17', '--eval_only'])
    assert "--band_sequence_path ignored: dcll_conv_lif_sequence_bands does not serve" in capsys.readouterr().out
    assert not any(n.startswith("k_lif_seq_band") for n in tr.names)
