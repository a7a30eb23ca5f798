"""dcll_conv_lif_sequence_tiles (k_lif_seq_tile) on the GPU: the fused all-T kernel of a plain conv layer with a 2-D grid of
workgroups per sample, each on a tile of the output plane, against the pinned-order C oracle stepped T times — case list
tests/seq_tile_cases.py (proven on the CPU by tests/test_seq_tile_cases.py) — against dcll_conv_lif_sequence_bands wherever its rule
serves the layer, and the network level above it: ConvNetwork.test_sequence_any(tiles=...) against bands=, bands=None and the
per-step loop, train.py --tile_sequence_path.  Helpers and tolerances: tests/test_gpu_seq_any.py, tests/test_gpu_seq_band.py.

v is compared bit for bit up to the sign of a zero against the oracle — and bit for bit, signs included, against the
band path; pooled spikes and eps0 / eps1 / arp after every call bit for bit; pv within 1e-4.  spk_out is handed in filled with
0xFFFFFFFF (a shared word is ORed into: the launcher's zero fill, or a stored word, must have replaced every one), and every output
buffer sits in front of a sentinel tail."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import seq_band_cases as S
import seq_tile_cases as X
import test_gpu_seq_any as G
import test_gpu_seq_band as GB

pytestmark = pytest.mark.gpu
LOGIT_TOL, PV_TOL = G.LOGIT_TOL, G.PV_TOL
CASES = X.cases()
REFUSE = X.refusals()
SERVED = collections.Counter()
TAIL, SENT = GB.TAIL, GB.SENT
_tailed = GB._tailed


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _operands(c, dev):
    """device tensors of a case: weights, bias, time constants, the initial state tiled to B samples"""
    T_, traj = X.run(c)
    B = c["B"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    op = dict(W=cu(T_["W"]), b=(cu(T_["b"]) if T_["b"] is not None else None), tau4=cu(np.stack(T_["tau"]).astype(np.float32)),
              eps0=cu(G._tile(T_["eps0"], B, 0)), eps1=cu(G._tile(T_["eps1"], B, 0)),
              arp=cu(G._tile(T_["arp"], B, 0)) if c["refractory"] else None)
    calls = []
    for call in T_["calls"]:
        n = call["x"].shape[0]
        x = G._tile(call["x"], B, 1).reshape(n, B, c["c_in"], c["h"] * c["w"])
        calls.append((n, cu(X.pack_planes(x).view(np.int32))))
    return op, calls, traj


def _call(c, op, n, spk_in, dev, entry="tiles", bands=0):
    """one call through the C ABI on buffers with sentinel tails, spk_out handed in as 0xFFFFFFFF -> ((spk, pv, v), launch log)"""
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = G._desc(c)
    B = c["B"]
    ch, cw, ph, pw = X.out_shape(c)
    spk, t_spk = _tailed((n, B, c["c_out"], (ph * pw + 31) // 32), torch.int32, -1, dev)
    pv, t_pv = _tailed((n, B, c["c_out"], ph, pw), torch.float32, SENT, dev)
    v, t_v = _tailed((n, B, c["c_out"], ch, cw), torch.float32, SENT, dev)
    ns = int(lib.dcll_conv_lif_sequence_tiles_scratch(ctypes.byref(d), B)) if entry == "tiles" else \
        int(lib.dcll_conv_lif_sequence_bands_scratch(ctypes.byref(d), B))
    assert ns > 0
    scratch, t_scr = _tailed((ns,), torch.float32, SENT, dev)
    p = _lib.ptr
    args = (ctypes.byref(d), p(spk_in), p(op["W"]), p(op["b"]), p(op["tau4"]), p(op["eps0"]), p(op["eps1"]), p(op["arp"]), p(spk), p(pv),
            p(v), p(scratch), n, B)
    with ops.kernel_trace() as tr:
        if entry == "tiles":
            rc = lib.dcll_conv_lif_sequence_tiles(*(args + (c["tiles"][0], c["tiles"][1], _lib.stream_ptr())))
        else:
            rc = lib.dcll_conv_lif_sequence_bands(*(args + (bands, _lib.stream_ptr())))
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
    ch, cw, ph, pw = X.out_shape(c)
    for k, ((n, spk_in), ref) in enumerate(zip(calls, traj)):
        (spk, pv, v), names = _call(c, op, n, spk_in, dev)
        assert names == X.launch_log(c), (c["id"], names)
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
        outs.append([t.cpu().numpy().copy() for t in (spk, pv, v, op["eps0"], op["eps1"]) + ((op["arp"],) if c["refractory"] else ())])
    SERVED[X.variant(c)] += 1
    return outs


def _run_plain(c, dev, entry, bands=0):
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
    """every case (named layers, edges, boundaries, the B = 300 x (2, 2) grid beyond residency — two consecutive calls, all 300
    samples compared —, forwarded calls, free draws) with the launch log the restated dispatch predicts; where
    dcll_conv_lif_sequence_bands (its rule's count) serves the layer too, every output and the state after every call equal its,
    bit for bit, v and pv included"""
    mine = run_case(case, dev)
    if S.band_count(case, case["B"], 0) > 0:
        theirs, _ = _run_plain(case, dev, "bands", 0)
        for k, (a, b) in enumerate(zip(mine, theirs)):
            for name, x, y in zip(("spk", "pv", "v", "eps0", "eps1", "arp"), a, b):
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), y), (case["id"], "call %d" % k, name, "differs from dcll_conv_lif_sequence_bands")


def test_the_band_path_cross_checks_enough_cases():
    """the cross-check above is not vacuous: the band rule serves most of the tiled cases, every template instance among them"""
    both = [c for c in CASES if X.tile_count(c)[1] > 1 and S.band_count(c, c["B"], 0) > 0]
    assert len(both) >= 80 and {X.variant(c) for c in both} == set(X.all_variants())


def test_a_second_run_is_bit_identical(dev):
    """one case per template instance, and every edge case with a shared spike word (the ORs commute), run twice from the same
    state: every output and the state after every call equal bit for bit"""
    seen, picked = set(), []
    for c in CASES:
        ny, nx = X.tile_count(c)
        if nx > 1 and (X.variant(c) not in seen or (c["stratum"] == "edges" and "-pw" in c["id"] and X.shared_words(c, ny, nx))):
            seen.add(X.variant(c))
            picked.append(c)
    assert seen == set(X.all_variants())
    for c in picked:
        a, la = _run_plain(c, dev, "tiles")
        b, lb = _run_plain(c, dev, "tiles")
        assert la == lb == [X.launch_log(c)] * len(c["Ts"]), (c["id"], la)
        assert all(np.array_equal(x, y) for ca, cb in zip(a, b) for x, y in zip(ca, cb)), c["id"]


def test_every_template_instance_served_a_case(dev):
    """all eight instances k_lif_seq_tile<MT,R,WLDS> serve a case to the end: the first case of each is run HERE, its launch log
    read back"""
    here = collections.Counter()
    for c in CASES:
        if X.tile_count(c)[1] > 1 and not here[X.variant(c)]:
            run_case(c, dev)
            here[X.variant(c)] += 1
    assert set(here) == set(X.all_variants()), dict(here)
    print("\n".join("%-28s %4d" % (k, SERVED[k]) for k in X.all_variants()))


def test_forwarded_calls_are_the_band_path(dev):
    """tiles_x = 1, and (0, 0) where a band count serves the layer: dcll_conv_lif_sequence_bands' launch log (its siblings' for one
    band) and bits"""
    n = 0
    for c in CASES:
        ny, nx = X.tile_count(c)
        if nx != 1:
            continue
        n += 1
        a, la = _run_plain(c, dev, "tiles")
        b, lb = _run_plain(c, dev, "bands", c["tiles"][0])
        assert la == lb == [X.launch_log(c)] * len(c["Ts"]), (c["id"], la, lb)
        assert not any(name.startswith("k_lif_seq_tile") for log in la for name in log)
        assert all(np.array_equal(x, y) for ca, cb in zip(a, b) for x, y in zip(ca, cb)), c["id"]
    assert n >= 8


def test_ops_wrapper_reuses_one_scratch_buffer(dev):
    """ops.conv_lif_sequence_tiles: the results of the C call, its scratch kept under 'tile_scratch' and reused"""
    from snn_modulation_classification_amd import ops
    c = X.by_id("tile-edge-pw11")
    ref, _ = _run_plain(c, dev, "tiles")
    op, calls, _ = _operands(c, dev)
    bufs = {}
    for k, (n, spk_in) in enumerate(calls):
        with ops.kernel_trace() as tr:
            spk, pv, v = ops.conv_lif_sequence_tiles(G._desc(c), spk_in, op["W"], op["b"], op["tau4"], op["eps0"], op["eps1"], op["arp"],
                                                     n, c["B"], want_v=True, out=bufs, tiles=c["tiles"])
        assert list(tr.names) == X.launch_log(c)
        assert all(np.array_equal(t.cpu().numpy().view(np.uint32), r) for t, r in zip((spk, pv, v), ref[k]))
        assert bufs["tile_scratch"].numel() == X.scratch_floats(c) and "w_scratch" not in bufs and "band_scratch" not in bufs
        first = bufs["tile_scratch"] if k == 0 else first
        assert bufs["tile_scratch"] is first


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("r", REFUSE, ids=[r["id"] for r in REFUSE])
def test_refusal(dev, r):
    """the code, a phrase of dcll_last_error(), an empty launch log, nothing written"""
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = G._desc(r)
    T, B = r["T"], r["B"]
    Tn, Bn = max(T, 1), max(B, 1)
    ch, cw, ph, pw = X.out_shape(r) if X.valid(r) else (1, 1, 1, 1)
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(spk_in=torch.zeros((Tn, Bn, r["c_in"], (r["h"] * r["w"] + 31) // 32), device=dev, dtype=torch.int32),
             W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]), tau4=f(4, r["c_in"]),
             eps0=f(Bn, r["c_in"], r["h"], r["w"]), eps1=f(Bn, r["c_in"], r["h"], r["w"]), arp=f(Bn, r["c_out"], ch, cw),
             spk=torch.full((Tn, Bn, r["c_out"], (ph * pw + 31) // 32), 77, device=dev, dtype=torch.int32),
             pv=f(Tn, Bn, r["c_out"], ph, pw), v=f(Tn, Bn, r["c_out"], ch, cw),
             scratch=f(128 * X.steps(r) + 2 * Bn * r["c_in"] * r["h"] * r["w"] + 128))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_sequence_tiles(ctypes.byref(d), p["spk_in"], p["W"], p["b"], p["tau4"], p["eps0"], p["eps1"], p["arp"],
                                              p["spk"], p["pv"], p["v"], p["scratch"], T, B if r["B_call"] is None else r["B_call"],
                                              r["tiles"][0], r["tiles"][1], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode(), (r["id"], lib.dcll_last_error())
    assert tr.names == [], (r["id"], tr.names)
    for k in ("eps0", "eps1", "arp", "pv", "v", "scratch"):
        assert bool((t[k] == SENT).all()), (r["id"], k, "was written")
    assert bool((t["spk"] == 77).all())
    if r["code"] == "DCLL_ERR_UNSUPPORTED":
        assert not ops.sequence_tiles_supported(d, r["tiles"]) and ops.sequence_tiles_plan(d, Bn, r["tiles"]) is None


# ---------------------------------------------------------------------------------------------- networks
_state_equal, _results_equal, _per_step, ops_mean = GB._state_equal, GB._results_equal, GB._per_step, GB.ops_mean


def _seq_names(tr):
    return [n for n in tr.names if n.startswith("k_lif_seq")]


def test_network_radio_ml_netscale2_8x64_is_served_by_tiles_alone(dev):
    """radio_ml_conv.yaml at netscale 2 on an (8, 64) plane, B = 2, T = 6: no band count serves the 64 -> 64 layers;
    test_sequence_any(tiles=(0, 0)) does, and equals the per-step loop: spikes of all layers and the final state bit for bit, logits
    within 1e-4, clout and votes equal (margin rule on the per-step logits)"""
    from snn_modulation_classification_amd import _lib, ops
    H, Wd, T, B = 8, 64, 6, 2
    net, _ = G._net("radio_ml_conv.yaml", (1, H, Wd), B, 24, netscale=2.0)
    assert not net.sequence_any_supported(wide=True) and not net.sequence_any_supported(bands=0)
    assert net.sequence_any_supported(tiles=(0, 0)) and net.sequence_any_supported(wide=True, bands=0, tiles=(0, 0))
    assert not net.sequence_any_supported(tiles=(1, 2)) and not net.sequence_any_supported(tiles=(9, 2))
    cells = torch.from_numpy(np.random.RandomState(0).randint(0, H * Wd, size=(T, B)).astype(np.int32)).to(dev)
    with pytest.raises(_lib.DCLLUnsupported, match="dcll_conv_lif_sequence_bands"):
        net.test_sequence_any(cells, bands=0)
    with pytest.raises(_lib.DCLLUnsupported, match="dcll_conv_lif_sequence_tiles"):
        net.test_sequence_any(cells, bands=0, wide=True, tiles=(1, 2))
    net.reset()
    with G.ops_trace() as tr:
        res = net.test_sequence_any(cells, keep_spikes=True, tiles=(0, 0))
    names = _seq_names(tr)
    assert len(names) == 3 and names[0].startswith("k_lif_seq_band<2,1,") and names[1:] == ["k_lif_seq_tile<2,1,0>"] * 2, names
    assert not any(n.startswith(("k_conv_lif", "k_trace", "k_pool")) for n in tr.names)
    planes = ops.cells_to_planes(cells, H * Wd).reshape(T, B, 1, H, Wd)
    twin, _ = G._net("radio_ml_conv.yaml", (1, H, Wd), B, 24, netscale=2.0)
    spikes, logits = _per_step(twin, planes)
    for i in range(3):
        got = ops.unpack_spike_planes(res["spikes"][i], H * Wd).cpu().numpy().reshape(T, B, 64, H, Wd)
        assert np.array_equal(got, spikes[i]) and 0 < spikes[i].mean() < 1, ("spikes", i)
        mine = (res["o"] if i == 2 else res["logits"][i]).cpu().numpy()
        worst = float(np.abs(mine - logits[i]).max())
        print("layer %d: logits worst abs error %.3g (bound %.3g)" % (i, worst, LOGIT_TOL))
        assert worst <= LOGIT_TOL, ("logits", i)
    _state_equal(net, twin)
    step, _ = G._net("radio_ml_conv.yaml", (1, H, Wd), B, 24, netscale=2.0)
    G._compare_with_per_step(net, res, step, planes, np.arange(B) % 24, 24, logits, max_excluded=.05)
    _state_equal(net, step)


def test_network_radio_ml_netscale2_16x16_tiles_equal_bands_equal_one_workgroup(dev):
    """radio_ml_conv.yaml at netscale 2 on 16x16, B = 2, T = 6: tiles=(2, 2) == bands=4 == bands=None (wide) in logits, clout,
    votes, spikes and state, bit for bit; tiles wins over bands and wide; every layer on k_lif_seq_tile"""
    R, T, B = 16, 6, 2
    nets = [G._net("radio_ml_conv.yaml", (1, R, R), B, 24, netscale=2.0)[0] for _ in range(3)]
    assert nets[0].sequence_any_supported(tiles=(2, 2)) and not nets[0].sequence_any_supported(tiles=(2, 17))
    cells = torch.from_numpy(np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)).to(dev)
    for n in nets:
        n.reset()
    with G.ops_trace() as tr:
        ra = nets[0].test_sequence_any(cells, keep_spikes=True, wide=True, bands=4, tiles=(2, 2))
    assert _seq_names(tr) == ["k_lif_seq_tile<2,1,1>", "k_lif_seq_tile<2,1,0>", "k_lif_seq_tile<2,1,0>"], _seq_names(tr)
    with G.ops_trace() as tr:
        rb = nets[1].test_sequence_any(cells, keep_spikes=True, wide=True, bands=4)
    assert all(n.startswith("k_lif_seq_band") for n in _seq_names(tr))
    rc = nets[2].test_sequence_any(cells, keep_spikes=True, wide=True)
    _results_equal(ra, rb)
    _results_equal(ra, rc)
    _state_equal(nets[0], nets[1])
    _state_equal(nets[0], nets[2])
    assert 0 < float(ops_mean(ra["spikes"][2])) < 1


def test_chunked_batch_equals_whole_batch(dev):
    """test_sequence_any(tiles=(2, 2)) under a pv budget that splits the batch (2 + 1 samples) == the whole batch at once"""
    T, B = 6, 3
    x = GB._mnist_input(dev, T, B)
    whole, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    parts, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    per_sample = 4 * T * max(s.dclllayer.out_channels * int(np.prod(s.dclllayer.output_shape)) for s in parts.dcll_slices)
    parts.pv_budget_bytes = 2 * per_sample + 1
    whole.reset()
    parts.reset()
    ra = whole.test_sequence_any(x, keep_spikes=True, tiles=(2, 2))
    with G.ops_trace() as tr:
        rb = parts.test_sequence_any(x, keep_spikes=True, tiles=(2, 2))
    assert sum(n.startswith("k_lif_seq_tile") for n in tr.names) == 6
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and ra["spikes"][i].shape[1] == B
        assert float((ra["logits"][i] - rb["logits"][i]).abs().max()) <= 2 * LOGIT_TOL
        assert torch.equal(ra["clout"][i], rb["clout"][i]) and torch.equal(ra["vote"][i], rb["vote"][i])
    _state_equal(whole, parts)


# ---------------------------------------------------------------------------------------------- entry points
def test_entry_point_train_tile_sequence_path(tmp_path, capsys):
    """train.py --netscale 2 on synthetic IQ at the (8, 64) plane: the periodic test with --tile_sequence_path runs k_lif_seq_tile
    and reports the accuracies of the same command without the flag (evaluate_batch's per-step loop); it wins over the three other
    sequence flags; at netscale 1 on 16x16 (the specialised sequence kernels) and with a plan of more tiles than pooled rows the
    flag is ignored with a notice"""
    import train
    common = ['--arp', '1.0', '--burnin', '4', '--batch_size', '8', '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8',
              '--n_iters', '8', '--n_iters_test', '12', '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    plane = ['--I_resolution', '64', '--Q_resolution', '8', '--netscale', '2']
    with G.ops_trace() as tr:
        out_tile = train.main(common + plane + ['--output', str(tmp_path / 'tile'), '--tile_sequence_path', '--band_sequence_path',
                                                '--wide_sequence_path', '--any_sequence_path'])
    assert sum(n.startswith("k_lif_seq_tile") for n in tr.names) == 2 and sum(n.startswith("k_lif_seq_band") for n in tr.names) == 1
    out = capsys.readouterr().out
    assert "--tile_sequence_path ignored" not in out
    with G.ops_trace() as tr:
        out_step = train.main(common + plane + ['--output', str(tmp_path / 'step')])
    assert not any(n.startswith("k_lif_seq") for n in tr.names)
    a, b = np.load(os.path.join(out_tile, 'acc_test.npy')), np.load(os.path.join(out_step, 'acc_test.npy'))
    assert a.shape == b.shape == (1, 1, 3) and np.isfinite(a).all() and np.array_equal(a, b)
    capsys.readouterr()
    with G.ops_trace() as tr:
        train.main(common + ['--I_resolution', '16', '--Q_resolution', '16', '--output', str(tmp_path / 'n1'), '--tile_sequence_path',
                             '--eval_only'])
    assert "--tile_sequence_path ignored: the network runs" in capsys.readouterr().out and not any(n.startswith("k_lif_seq_tile") for n in tr.names)
    with G.ops_trace() as tr:
        train.main(common + plane + ['--output', str(tmp_path / 'n9'), '--tile_sequence_path', '9', '2', '--eval_only'])
    assert "--tile_sequence_path ignored: dcll_conv_lif_sequence_tiles does not serve" in capsys.readouterr().out
    assert not any(n.startswith("k_lif_seq_tile") for n in tr.names)
