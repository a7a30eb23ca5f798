"""dcll_conv_lif_sequence_slabs (k_lif_seq_slab) on the GPU: the fused all-T kernel of a plain conv layer with MORE than 64 output
channels — a workgroup per (sample, tile of the output plane, slab of 64 output channels) — against the pinned-order C oracle
stepped T times on EVERY call, and against dcll_conv_lif_sequence_tiles run on each 64-channel slice of the layer with the same plan,
bit for bit.  Case list: tests/seq_slab_cases.py (proven on the CPU by tests/test_seq_slab_cases.py).  Then the network level:
ConvNetwork.test_sequence_any(slabs=...) against the per-step loop and tiles=, train.py --slab_sequence_path.  Helpers and
tolerances: tests/test_gpu_seq_any.py, tests/test_gpu_seq_band.py.

v is compared bit for bit up to the sign of a zero against the oracle; pooled spikes and eps0 / eps1 / arp after every
call bit for bit; pv within the header's 1e-4.  spk_out is handed in filled with 0xFFFFFFFF, and every output buffer sits in front of
a sentinel tail."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import seq_slab_cases as SL
import seq_tile_cases as X
import test_gpu_seq_any as G
import test_gpu_seq_band as GB
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
LOGIT_TOL, PV_TOL = G.LOGIT_TOL, G.PV_TOL
CASES = SL.cases()
REFUSE = SL.refusals()
SERVED = collections.Counter()
RAN = set()
TAIL, SENT = GB.TAIL, GB.SENT
_tailed = GB._tailed


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _operands(c, T_, dev):
    """device tensors of a case (or of a slice of it): weights, bias, time constants, the initial state tiled to B samples, the
    packed input of every call"""
    B = c["B"]
    op = dict(W=_cu(T_["W"], dev), b=(_cu(T_["b"], dev) if T_["b"] is not None else None), tau4=_cu(np.stack(T_["tau"]).astype(np.float32), dev),
              eps0=_cu(G._tile(T_["eps0"], B, 0), dev), eps1=_cu(G._tile(T_["eps1"], B, 0), dev),
              arp=_cu(G._tile(T_["arp"], B, 0), dev) if c["refractory"] else None)
    calls = []
    for call in T_["calls"]:
        n = call["x"].shape[0]
        x = G._tile(call["x"], B, 1).reshape(n, B, c["c_in"], c["h"] * c["w"])
        calls.append((n, _cu(SL.pack_planes(x).view(np.int32), dev)))
    return op, calls


def _call(c, op, n, spk_in, dev, entry="slabs"):
    """one call through the C ABI on buffers with sentinel tails, spk_out handed in as 0xFFFFFFFF -> ((spk, pv, v), launch log)"""
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = G._desc(c)
    B = c["B"]
    ch, cw, ph, pw = SL.out_shape(c)
    spk, t_spk = _tailed((n, B, c["c_out"], (ph * pw + 31) // 32), torch.int32, -1, dev)
    pv, t_pv = _tailed((n, B, c["c_out"], ph, pw), torch.float32, SENT, dev)
    v, t_v = _tailed((n, B, c["c_out"], ch, cw), torch.float32, SENT, dev)
    ns = int(getattr(lib, "dcll_conv_lif_sequence_%s_scratch" % entry)(ctypes.byref(d), B))
    assert ns > 0 and (entry != "slabs" or ns == SL.scratch_floats(c))
    scratch, t_scr = _tailed((ns,), torch.float32, SENT, dev)
    p = _lib.ptr
    args = (ctypes.byref(d), p(spk_in), p(op["W"]), p(op["b"]), p(op["tau4"]), p(op["eps0"]), p(op["eps1"]), p(op["arp"]), p(spk), p(pv),
            p(v), p(scratch), n, B, c["tiles"][0], c["tiles"][1], _lib.stream_ptr())
    with ops.kernel_trace() as tr:
        rc = getattr(lib, "dcll_conv_lif_sequence_%s" % entry)(*args)
    torch.cuda.synchronize()
    assert rc == _lib.DCLL_OK, (c["id"], rc, lib.dcll_last_error())
    assert bool((t_spk == -1).all()) and all(bool((t == SENT).all()) for t in (t_pv, t_v, t_scr)), (c["id"], "a sentinel tail was written")
    return (spk, pv, v), list(tr.names)


def _run_plain(c, T_, dev, entry="slabs"):
    """every call of a case through one entry point -> (host copies (uint32 views) of spk, pv, v, eps0, eps1[, arp] after every call,
    the launch logs)"""
    op, calls = _operands(c, T_, dev)
    outs, logs = [], []
    for n, spk_in in calls:
        res, names = _call(c, op, n, spk_in, dev, entry)
        logs.append(names)
        outs.append([t.cpu().numpy().copy().view(np.uint32) for t in res + tuple(op[k] for k in ("eps0", "eps1", "arp") if op[k] is not None)])
    return outs, logs


def run_case(c, dev):
    """every call of a case on the device against the oracle's trajectory -> the host copies of _run_plain"""
    from snn_modulation_classification_amd import ops
    T_, traj = SL.run(c)
    op, calls = _operands(c, T_, dev)
    B = c["B"]
    ch, cw, ph, pw = SL.out_shape(c)
    outs = []
    for k, ((n, spk_in), ref) in enumerate(zip(calls, traj)):
        (spk, pv, v), names = _call(c, op, n, spk_in, dev)
        assert names == SL.launch_log(c), (c["id"], names, SL.launch_log(c))
        tag = (c["id"], "call %d" % k)
        G._same(v, ref["v"], 1, tag + ("v",), zero_sign=True)
        G._same(ops.unpack_spike_planes(spk.contiguous(), ph * pw).reshape(n, B, c["c_out"], ph, pw), ref["s"], 1, tag + ("spikes",))
        got_pv = pv.cpu().numpy()
        Bc = ref["pv"].shape[1]
        worst = max(float(np.abs(got_pv[:, j:j + Bc] - ref["pv"][:, :B - j]).max()) for j in range(0, B, Bc))
        print(tag, "pv worst abs error %.3g (bound %.3g)" % (worst, PV_TOL))
        assert worst <= PV_TOL, tag + ("pv", worst)
        if (ph * pw) % 32:          # tail bits of the last word are zero
            assert not bool((spk[..., -1].cpu().numpy().view(np.uint32) >> np.uint32((ph * pw) % 32)).any()), tag
        G._same(op["eps0"], ref["eps0"], 0, tag + ("eps0",))
        G._same(op["eps1"], ref["eps1"], 0, tag + ("eps1",))
        if c["refractory"]:
            G._same(op["arp"], ref["arp"], 0, tag + ("arp",))
        outs.append([t.cpu().numpy().copy().view(np.uint32) for t in (spk, pv, v, op["eps0"], op["eps1"]) + ((op["arp"],) if c["refractory"] else ())])
    SERVED[SL.variant(c)] += 1
    return outs


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle_and_the_tile_kernel(dev, case):
    """every case against the oracle on every call (two consecutive calls carry state), with the predicted launch log; for
    c_out > 64 every slab's planes — spikes, pv, v, arp — and the final eps0 / eps1 equal dcll_conv_lif_sequence_tiles run on that
    64-channel slice of W / bias / arp with the same plan, bit for bit; a forwarded case (c_out <= 64) IS that call: log and bits"""
    c = case
    print(SL.describe(c))
    mine = run_case(c, dev)
    T_, _ = SL.run(c)
    if c["c_out"] <= 64:
        theirs, logs = _run_plain(c, T_, dev, "tiles")
        assert logs == [X.launch_log(c)] * len(c["Ts"]) and not any(n.startswith("k_lif_seq_slab") for l in logs for n in l)
        assert all(np.array_equal(x, y) for a, b in zip(mine, theirs) for x, y in zip(a, b)), c["id"]
    else:
        for s, (first, n) in enumerate(SL.slabs(c["c_out"])):
            sc = SL.slice_case(c, s)
            theirs, logs = _run_plain(sc, SL.slice_tensors(c, T_, s), dev, "tiles")
            assert not any(name.startswith("k_lif_seq_slab") for l in logs for name in l)
            for k, (a, b) in enumerate(zip(mine, theirs)):
                for name, x, y in zip(("spk", "pv", "v"), a[:3], b[:3]):
                    assert np.array_equal(x[:, :, first:first + n], y), (c["id"], "slab %d" % s, "call %d" % k, name)
                assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), (c["id"], "slab %d" % s, "call %d" % k, "eps0 / eps1")
                if c["refractory"]:
                    assert np.array_equal(a[5][:, first:first + n], b[5]), (c["id"], "slab %d" % s, "call %d" % k, "arp")
    RAN.add(c["id"])


def test_every_template_instance_served_a_case():
    assert RAN == {c["id"] for c in CASES}, "run the whole module: this test sums up the cases above"
    print(dict(SERVED))
    assert all(SERVED[v] >= 1 for v in SL.all_variants()), dict(SERVED)


def test_a_second_run_is_bit_identical(dev):
    """one case per template instance and the case with shared spike words (the ORs commute), run twice from the same state"""
    picked, seen = [], set()
    for c in CASES:
        if c["c_out"] > 64 and (SL.variant(c) not in seen or c["id"] == "slab-pw40-shared-words"):
            seen.add(SL.variant(c))
            picked.append(c)
    assert seen == set(SL.all_variants())
    c = SL.by_id("slab-pw40-shared-words")
    assert X.shared_words(c, *SL.plan_of(c))
    for c in picked:
        T_, _ = SL.run(c)
        a, la = _run_plain(c, T_, dev)
        b, lb = _run_plain(c, T_, dev)
        assert la == lb == [SL.launch_log(c)] * len(c["Ts"]), (c["id"], la)
        assert all(np.array_equal(x, y) for ca, cb in zip(a, b) for x, y in zip(ca, cb)), c["id"]


def test_ops_wrapper_reuses_one_scratch_buffer(dev):
    from snn_modulation_classification_amd import ops
    c = SL.by_id("slab-t2x2")
    T_, _ = SL.run(c)
    ref, _ = _run_plain(c, T_, dev)
    op, calls = _operands(c, T_, dev)
    bufs = {}
    for k, (n, spk_in) in enumerate(calls):
        with ops.kernel_trace() as tr:
            spk, pv, v = ops.conv_lif_sequence_slabs(G._desc(c), spk_in, op["W"], op["b"], op["tau4"], op["eps0"], op["eps1"], op["arp"],
                                                     n, c["B"], want_v=True, out=bufs, slabs=c["tiles"])
            torch.cuda.synchronize()
        assert tr.names == SL.launch_log(c)
        for x, y in zip((spk, pv, v, op["eps0"], op["eps1"], op["arp"]), ref[k]):
            assert np.array_equal(x.cpu().numpy().view(np.uint32).reshape(y.shape), y), (c["id"], k)
        if k == 0:
            first = bufs["slab_scratch"].data_ptr()
    assert bufs["slab_scratch"].data_ptr() == first and bufs["slab_scratch"].numel() == SL.scratch_floats(c)
    d = G._desc(c)
    assert ops.sequence_slabs_supported(d, c["tiles"]) and ops.sequence_slabs_lds(d, c["tiles"]) == SL.lds_bytes(c)
    by, bx = ops.sequence_slabs_plan(d, c["B"], (0, 0))
    assert (len(by) - 1, len(bx) - 1) == SL.plan_of(c, tiles=(0, 0))
    assert not ops.sequence_tiles_supported(d, (2, 2))          # (pinned: the tile path refuses c_out > 64)


@pytest.mark.parametrize("ref", REFUSE, ids=[r["id"] for r in REFUSE])
def test_refusals_come_before_any_launch(dev, ref):
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    c = ref
    d = G._desc(c)
    B, T = c["B"], 3
    ch, cw, ph, pw = SL.out_shape(c) if SL.valid(c) else (1, 1, 1, 1)
    t = lambda shape, fill, dt=torch.float32: torch.full(shape, fill, dtype=dt, device=dev)
    bufs = dict(spk_in=t((T, B, c["c_in"], (c["h"] * c["w"] + 31) // 32), 0, torch.int32), W=t((c["c_out"], c["c_in"], c["kh"], c["kw"]), .1),
                b=t((c["c_out"],), 0.), tau4=t((4, c["c_in"]), .9), eps0=t((B, c["c_in"], c["h"], c["w"]), 1.5), eps1=t((B, c["c_in"], c["h"], c["w"]), 2.5),
                arp=t((B, c["c_out"], ch, cw), -.5), spk=t((T, B, c["c_out"], (ph * pw + 31) // 32), -1, torch.int32),
                pv=t((T, B, c["c_out"], ph, pw), SENT), v=t((T, B, c["c_out"], ch, cw), SENT), scratch=t((1 << 20,), SENT))
    if c["null"]:
        bufs[c["null"]] = None
    p = _lib.ptr
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_sequence_slabs(ctypes.byref(d), p(bufs["spk_in"]), p(bufs["W"]), p(bufs["b"]), p(bufs["tau4"]), p(bufs["eps0"]),
                                              p(bufs["eps1"]), p(bufs["arp"]), p(bufs["spk"]), p(bufs["pv"]), p(bufs["v"]), p(bufs["scratch"]),
                                              c["T"], B, c["tiles"][0], c["tiles"][1], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, c["code"]), (c["id"], rc, lib.dcll_last_error())
    assert tr.names == []
    if c["code"] != "DCLL_OK":
        msg = lib.dcll_last_error().decode()
        assert c["phrase"] in msg and "dcll_conv_lif_sequence_slabs" in msg, msg
    for k, fill in (("spk", -1), ("pv", SENT), ("v", SENT), ("scratch", SENT), ("eps0", 1.5), ("eps1", 2.5), ("arp", -.5)):
        if bufs[k] is not None:
            assert bool((bufs[k] == fill).all()), (c["id"], k)


# ------------------------------------------------------------------------------------------------------------------------------
# network level
# ------------------------------------------------------------------------------------------------------------------------------
def _net(netscale, B, dev):
    net, _ = G._net("radio_ml_conv.yaml", (1, 16, 16), B, 24, netscale=netscale)
    return net


def _planes(T, B, dev, seed=0):
    rng = np.random.RandomState(seed)
    return torch.from_numpy((rng.uniform(size=(T, B, 1, 16, 16)) < .1).astype(np.float32)).to(dev)


@pytest.mark.parametrize("netscale", [3.0, 4.0], ids=["netscale3", "netscale4"])
def test_network_slabs_equal_the_per_step_loop(dev, netscale):
    """radio_ml_conv.yaml at netscale 3 / 4 on 16x16, B = 3, T = 6: test_sequence_any(slabs=(0, 0)) == the per-step loop: spikes of all
    layers and the final state bit for bit, logits within 1e-4, clout and votes equal (margin rule on the per-step logits);
    k_lif_seq_slab served every layer; slabs wins over tiles, bands and wide"""
    from snn_modulation_classification_amd import _lib, ops
    B, T = 3, 6
    x = _planes(T, B, dev)
    net = _net(netscale, B, dev)
    C = int(32 * netscale)
    assert [s.dclllayer.out_channels for s in net.dcll_slices] == [C, C, C]
    assert net.sequence_any_supported(slabs=(0, 0)) and not net.sequence_any_supported(tiles=(0, 0)) and not net.sequence_any_supported(wide=True)
    with pytest.raises(_lib.DCLLUnsupported):
        net.test_sequence_any(x, tiles=(0, 0))
    net.reset()
    with ops.kernel_trace() as tr:
        res = net.test_sequence_any(x, slabs=(0, 0), keep_spikes=True, tiles=(2, 2), bands=3, wide=True)
        torch.cuda.synchronize()
    assert sum(n.startswith("k_lif_seq_slab") for n in tr.names) == 3, tr.names
    assert not any(n.startswith(("k_lif_seq_tile", "k_lif_seq_band", "k_lif_seq_wide", "k_conv_lif", "k_trace", "k_pool")) for n in tr.names), tr.names
    twin = _net(netscale, B, dev)
    spikes, logits = GB._per_step(twin, x)
    for i in range(3):
        got = ops.unpack_spike_planes(res["spikes"][i], 256).cpu().numpy().reshape(T, B, C, 16, 16)
        assert np.array_equal(got, spikes[i]) and 0 < spikes[i].mean() < 1, ("spikes", i)
        mine = (res["o"] if i == 2 else res["logits"][i]).cpu().numpy()
        worst = float(np.abs(mine - logits[i]).max())
        print("layer %d logits worst abs error %.3g (bound %.3g)" % (i, worst, LOGIT_TOL))
        assert worst <= LOGIT_TOL, ("logits", i)
    GB._state_equal(net, twin)
    step = _net(netscale, B, dev)
    G._compare_with_per_step(net, res, step, x, np.arange(B) % 24, 24, logits, max_excluded=.05)
    GB._state_equal(net, step)


def test_network_slabs_equal_tiles_at_netscale_2_and_a_split_batch_equals_the_whole(dev):
    """netscale 2 (64 channels): slabs=(2, 2) IS tiles=(2, 2) — launch log and every result bit for bit; netscale 3: a batch evaluated
    in two chunks (DCLL_PV_BUDGET) == the whole batch"""
    from snn_modulation_classification_amd import ops
    B, T = 3, 6
    x = _planes(T, B, dev, 1)
    a, b = _net(2.0, B, dev), _net(2.0, B, dev)
    with ops.kernel_trace() as ta:
        ra = a.test_sequence_any(x, slabs=(2, 2), keep_spikes=True)
        torch.cuda.synchronize()
    with ops.kernel_trace() as tb:
        rb = b.test_sequence_any(x, tiles=(2, 2), keep_spikes=True)
        torch.cuda.synchronize()
    assert ta.names == tb.names and sum(n.startswith("k_lif_seq_tile") for n in ta.names) == 3, ta.names
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and torch.equal(ra["logits"][i], rb["logits"][i]) and torch.equal(ra["clout"][i], rb["clout"][i])
    a, b = _net(3.0, B, dev), _net(3.0, B, dev)
    ra = a.test_sequence_any(x, slabs=(0, 0), keep_spikes=True)
    per_sample = 4 * T * max(s.dclllayer.out_channels * int(np.prod(s.dclllayer.output_shape)) for s in b.dcll_slices)
    b.pv_budget_bytes = 2 * per_sample             # chunks of two samples: 2 + 1
    rb = b.test_sequence_any(x, slabs=(0, 0), keep_spikes=True)
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and torch.equal(ra["logits"][i], rb["logits"][i]) and torch.equal(ra["clout"][i], rb["clout"][i])
        for name in ("eps0", "eps1", "arp"):
            assert torch.equal(getattr(a.dcll_slices[i].dclllayer.i2h.state, name), getattr(b.dcll_slices[i].dclllayer.i2h.state, name))


def test_entry_point_train_with_slab_sequence_path(tmp_path, capsys, monkeypatch):
    """train.py --data MNIST --netscale 3 --slab_sequence_path on synthetic images: the test phase runs test_sequence_any(slabs=(0, 0))
    and gives the accuracies of the same command without the flag; with a plan that is not served, and where the flag does not apply,
    it prints the "ignored" notice and changes nothing."""
    import train
    from snn_modulation_classification_amd.networks import ConvNetwork
    calls = []
    real = ConvNetwork.test_sequence_any

    def counted(self, *a, **kw):
        calls.append(kw.get("slabs"))
        return real(self, *a, **kw)
    monkeypatch.setattr(ConvNetwork, "test_sequence_any", counted)
    common = ['--data', 'MNIST', '--network_spec', os.path.join(PKG, 'networks', 'mnist_conv.yaml'), '--synthetic', '16',
              '--batch_size', '8', '--batch_size_test', '8', '--n_test_samples', '8', '--n_steps', '1', '--n_iters', '8',
              '--n_iters_test', '8', '--burnin', '4', '--n_test_interval', '1', '--learning_rates', '1e-7', '--netscale', '3']
    runs = {}
    for key, extra in (("loop", []), ("slabs", ['--slab_sequence_path']), ("slabs22", ['--slab_sequence_path', '2', '2']),
                       ("unserved", ['--slab_sequence_path', '40', '40'])):
        del calls[:]
        out_dir = train.main(common + ['--output', str(tmp_path / key)] + extra)
        text = capsys.readouterr().out
        runs[key] = (list(calls), text, np.load(os.path.join(out_dir, 'acc_test.npy')))
    assert runs["loop"][0] == [] and "slab_sequence_path" not in runs["loop"][1]
    assert runs["slabs"][0] and all(s == (0, 0) for s in runs["slabs"][0]) and "ignored" not in runs["slabs"][1]
    assert runs["slabs22"][0] and all(s == (2, 2) for s in runs["slabs22"][0])
    assert np.array_equal(runs["slabs"][2], runs["loop"][2]) and np.array_equal(runs["slabs22"][2], runs["loop"][2])
    assert runs["unserved"][0] == [] and "--slab_sequence_path ignored: dcll_conv_lif_sequence_slabs does not serve" in runs["unserved"][1]
    assert np.array_equal(runs["unserved"][2], runs["loop"][2])
