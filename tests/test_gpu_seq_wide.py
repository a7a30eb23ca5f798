"""dcll_conv_lif_sequence_wide (k_lif_seq_wide) on the GPU: the fused all-T kernel of plain conv layers with 33-64 output channels
against the pinned-order C oracle stepped T times, case list tests/seq_wide_cases.py (proven on the CPU by
tests/test_seq_wide_cases.py), and the network level above it — ConvNetwork.test_sequence_any(wide=True) against the oracle and the
per-step loop, train.py --wide_sequence_path.  Helpers and tolerances: tests/test_gpu_seq_any.py.

v is compared bit for bit up to the sign of a zero (a chain of odd length ends with fmaf(0, 0, acc)): a difference is
allowed only where both values are zero; pooled spikes and eps0 / eps1 / arp after every call bit for bit; pv within 1e-4."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import seq_wide_cases as W
import test_gpu_seq_any as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
LOGIT_TOL, PV_TOL = G.LOGIT_TOL, G.PV_TOL
CASES = W.cases()
REFUSE = W.refusals()
SERVED = collections.Counter()
RAN = set()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _operands(c, dev, run=None):
    """device tensors of a case: weights, bias, time constants, the initial state tiled to B samples"""
    T_, traj = W.run(c) if run is None else run
    B = c["B"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    op = dict(W=cu(T_["W"]), b=(cu(T_["b"]) if T_["b"] is not None else None), tau4=cu(np.stack(T_["tau"]).astype(np.float32)),
              eps0=cu(G._tile(T_["eps0"], B, 0)), eps1=cu(G._tile(T_["eps1"], B, 0)),
              arp=cu(G._tile(T_["arp"], B, 0)) if c["refractory"] else None)
    calls = []
    for call in T_["calls"]:
        n = call["x"].shape[0]
        x = G._tile(call["x"], B, 1).reshape(n, B, c["c_in"], c["h"] * c["w"])
        calls.append((n, cu(W.pack_planes(x).view(np.int32))))
    return op, calls, traj


def _call(c, op, n, spk_in, entry="wide"):
    from snn_modulation_classification_amd import ops
    fn = ops.conv_lif_sequence_wide if entry == "wide" else ops.conv_lif_sequence_any
    with ops.kernel_trace() as tr:
        out = fn(G._desc(c), spk_in, op["W"], op["b"], op["tau4"], op["eps0"], op["eps1"], op["arp"], n, c["B"], want_v=True)
    torch.cuda.synchronize()
    return out, list(tr.names)


def run_case(c, dev, run=None, count=True):
    """every call of a case on the device against the oracle's trajectory -> host copies of every call's outputs and state.
    run: (tensors, trajectory) of another draw of the same geometry (tests/value_cases.py), not counted as a case of this file"""
    from snn_modulation_classification_amd import ops
    op, calls, traj = _operands(c, dev, run)
    outs = []
    B = c["B"]
    ch, cw, ph, pw = W.out_shape(c)
    for k, ((n, spk_in), ref) in enumerate(zip(calls, traj)):
        (spk, pv, v), names = _call(c, op, n, spk_in)
        assert names == W.launch_log(c), (c["id"], names)
        tag = (c["id"], "call %d" % k)
        G._same(v, ref["v"], 1, tag + ("v",), zero_sign=True)
        G._same(ops.unpack_spike_planes(spk, ph * pw).reshape(n, B, c["c_out"], ph, pw), ref["s"], 1, tag + ("spikes",))
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
    if count:
        SERVED[W.variant(c)] += 1
        RAN.add(c["id"])
    return outs


# ---------------------------------------------------------------------------------------------- the case list
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle(dev, case):
    """every case (named layers, variants, edges, boundaries, the B = 1100 grid beyond residency with all 1100 samples compared,
    forwarded layers, free draws; carried state = consecutive calls on one set of state buffers against the oracle stepping
    straight through) with the launch log the restated dispatch predicts"""
    run_case(case, dev)


def test_a_second_run_is_bit_identical(dev):
    """the variants stratum run twice from the same state: every output and the final state equal bit for bit"""
    for c in CASES:
        if c["stratum"] != "variants":
            continue
        outs = []
        for _ in range(2):
            op, calls, _ = _operands(c, dev)
            res = [_call(c, op, n, spk_in)[0] for n, spk_in in calls]
            outs.append((res, op))
        for (a, b) in zip(outs[0][0], outs[1][0]):
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), c["id"]
        for k in ("eps0", "eps1", "arp"):
            if outs[0][1][k] is not None:
                assert torch.equal(outs[0][1][k].view(torch.int32), outs[1][1][k].view(torch.int32)), (c["id"], k)


def test_every_instantiated_variant_served_a_case(dev):
    """all six template instances of k_lif_seq_wide serve a case to the end: the `variants` stratum (one small case per instance)
    is run HERE, each call's launch log read back.  The counts over every case this process ran go to
    $DCLL_PROFILE_DIR/r17_seq_wide_variant_counts.txt when that is set (profiles/ holds a copy of a whole-file run)."""
    before = collections.Counter(SERVED)
    for c in CASES:
        if c["stratum"] == "variants":
            run_case(c, dev)
    here = SERVED - before
    assert set(here) == set(W.all_variants()) and all(here[k] > 0 for k in W.all_variants()), dict(here)
    whole = RAN == {c["id"] for c in CASES}
    keys = W.all_variants() + sorted(k for k in SERVED if k.startswith("k_lif_seq_any"))
    lines = ["%-28s %4d" % (k, (SERVED - here)[k] if whole else here[k]) for k in keys]
    print("\n".join(lines))
    out = os.environ.get("DCLL_PROFILE_DIR")
    if out:
        with open(os.path.join(out, "r17_seq_wide_variant_counts.txt"), "w") as f:
            f.write("k_lif_seq_wide<refractory, weights in LDS, register form>: cases served (%s, tests/test_gpu_seq_wide.py)\n"
                    % ("of all %d cases; k_lif_seq_any: the forwarded ones" % len(CASES) if whole else "the variants stratum alone"))
            f.write("\n".join(lines) + "\n")


def test_forwarded_cases_equal_sequence_any(dev):
    """c_out <= 32: dcll_conv_lif_sequence_wide == dcll_conv_lif_sequence_any bit for bit — v, pv, spikes, final state, launch log"""
    for c in CASES:
        if c["stratum"] != "forwarded":
            continue
        res = {}
        for entry in ("wide", "any"):
            op, calls, _ = _operands(c, dev)
            res[entry] = ([_call(c, op, n, spk_in, entry) for n, spk_in in calls], op)
        for (a, na), (b, nb) in zip(res["wide"][0], res["any"][0]):
            assert na == nb == ["k_seq_any_wprep", W.variant(c)], (c["id"], na, nb)
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), c["id"]
        for k in ("eps0", "eps1", "arp"):
            if res["wide"][1][k] is not None:
                assert torch.equal(res["wide"][1][k].view(torch.int32), res["any"][1][k].view(torch.int32)), (c["id"], k)


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("r", REFUSE, ids=[r["id"] for r in REFUSE])
def test_refusal(dev, r):
    """the code, a phrase of dcll_last_error(), an empty launch log, nothing written"""
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = G._desc(r)
    T, B = r["T"], r["B"]
    Tn, Bn = max(T, 1), max(B, 1)
    ch, cw, ph, pw = W.out_shape(r) if W.valid(r) else (1, 1, 1, 1)
    SENT = 12345.0
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(spk_in=torch.zeros((Tn, Bn, r["c_in"], (r["h"] * r["w"] + 31) // 32), device=dev, dtype=torch.int32),
             W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]), tau4=f(4, r["c_in"]),
             eps0=f(Bn, r["c_in"], r["h"], r["w"]), eps1=f(Bn, r["c_in"], r["h"], r["w"]), arp=f(Bn, r["c_out"], ch, cw),
             spk=torch.full((Tn, Bn, r["c_out"], (ph * pw + 31) // 32), 77, device=dev, dtype=torch.int32),
             pv=f(Tn, Bn, r["c_out"], ph, pw), v=f(Tn, Bn, r["c_out"], ch, cw), w_scratch=f(max(128 * W.steps(r), 128)))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_sequence_wide(ctypes.byref(d), p["spk_in"], p["W"], p["b"], p["tau4"], p["eps0"], p["eps1"], p["arp"],
                                             p["spk"], p["pv"], p["v"], p["w_scratch"], T, B, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == getattr(_lib, r["code"]), (r["id"], rc, lib.dcll_last_error())
    if r["code"] != "DCLL_OK":
        assert r["phrase"] in lib.dcll_last_error().decode(), (r["id"], lib.dcll_last_error())
    assert tr.names == [], (r["id"], tr.names)
    for k in ("eps0", "eps1", "arp", "pv", "v", "w_scratch"):
        assert bool((t[k] == SENT).all()), (r["id"], k, "was written")
    assert bool((t["spk"] == 77).all())
    if r["code"] == "DCLL_ERR_UNSUPPORTED":
        assert not ops.sequence_wide_supported(d)


# ---------------------------------------------------------------------------------------------- networks
def _state_equal(a, b):
    for sa, sb in zip(a.dcll_slices, b.dcll_slices):
        for u, v in zip(sa.dclllayer.i2h.state, sb.dclllayer.i2h.state):
            assert torch.equal(u, v)


def test_network_radio_ml_netscale2_16x16(dev):
    """radio_ml_conv.yaml at netscale 2 on the scripts' 16x16 plane (1 -> 64 LDS form, 64 -> 64 twice in the register form), B = 2,
    T = 6, cell indices in: test_sequence_any(wide=True) == the C oracle network (spikes of all layers bit for bit, logits within
    twice the readout tolerance) and == the per-step loop net.test(x[t]) (spikes of all layers and the final state bit for bit,
    clout and votes equal)"""
    from snn_modulation_classification_amd import _lib, ops
    R, T, B = 16, 6, 2
    net, convs = G._net("radio_ml_conv.yaml", (1, R, R), B, 24, netscale=2.0)
    assert [s.dclllayer.out_channels for s in net.dcll_slices] == [64, 64, 64]
    assert not net.sequence_supported() and not net.sequence_any_supported() and net.sequence_any_supported(wide=True)
    cells = np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)
    with pytest.raises(_lib.DCLLUnsupported):          # without wide: today's refusal
        net.test_sequence_any(torch.from_numpy(cells).to(dev))
    outs = G._radio_oracle(net, convs, R, cells)
    net.reset()
    with G.ops_trace() as tr:
        res = net.test_sequence_any(torch.from_numpy(cells).to(dev), keep_spikes=True, wide=True)
    assert [n for n in tr.names if n.startswith("k_lif_seq")] == ["k_lif_seq_wide<1,1,0>", "k_lif_seq_wide<1,0,1>", "k_lif_seq_wide<1,0,1>"]
    assert not any(n.startswith(("k_conv_lif", "k_trace", "k_pool")) for n in tr.names)
    for i in range(3):
        got = ops.unpack_spike_planes(res["spikes"][i], R * R).cpu().numpy().reshape(T, B, 64, R, R)
        assert np.array_equal(got, np.stack([o[i]["s"] for o in outs])), ("spikes", i)
        np.testing.assert_allclose(res["logits"][i].cpu().numpy(), np.stack([o[i]["p"] for o in outs]), atol=2 * LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(res["o"].cpu().numpy(), np.stack([o[2]["o"] for o in outs]), atol=2 * LOGIT_TOL, rtol=0)
    step, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24, netscale=2.0)
    planes = ops.cells_to_planes(torch.from_numpy(cells).to(dev), R * R).reshape(T, B, 1, R, R)
    orc_logits = [np.stack([o[i]["o" if i == 2 else "p"] for o in outs]) for i in range(3)]
    G._compare_with_per_step(net, res, step, planes, np.arange(B) % 24, 24, orc_logits)
    stepped, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24, netscale=2.0)
    G._assert_spikes_equal_per_step(net, res, stepped, planes)      # all three layers, every t; final state
    _state_equal(net, step)


def test_network_netscale1_wide_equals_any(dev):
    """the same network at netscale 1: every layer is forwarded — wide=True == wide=False bit for bit, k_lif_seq_any in the log"""
    R, T, B = 16, 6, 2
    a, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24)
    b, _ = G._net("radio_ml_conv.yaml", (1, R, R), B, 24)
    cells = torch.from_numpy(np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)).to(dev)
    a.reset()
    b.reset()
    with G.ops_trace() as tr:
        ra = a.test_sequence_any(cells, keep_spikes=True, wide=True)
    assert sum(n.startswith("k_lif_seq_any") for n in tr.names) == 3 and not any(n.startswith("k_lif_seq_wide") for n in tr.names)
    rb = b.test_sequence_any(cells, keep_spikes=True)
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and torch.equal(ra["logits"][i], rb["logits"][i])
        assert torch.equal(ra["clout"][i], rb["clout"][i]) and torch.equal(ra["vote"][i], rb["vote"][i])
    assert torch.equal(ra["o"], rb["o"])
    _state_equal(a, b)


def _mnist_input(dev, T, B):
    rng = np.random.RandomState(3)
    x = (rng.rand(T, B, 1, 28, 28) < .15).astype(np.float32)
    x[0] = rng.rand(B, 1, 28, 28) < .5
    return torch.from_numpy(x).to(dev)


def test_network_mnist_netscale2(dev):
    """mnist_conv.yaml at netscale 2 (32 / 48 / 64 channels: the first layer forwarded, two wide ones), B = 2, T = 6, against the
    per-step loop: spikes of all layers and the final state bit for bit, clout and votes equal (margin rule on the sequence's own
    logits)"""
    T, B = 6, 2
    net, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0, netscale=2.0)
    assert [s.dclllayer.out_channels for s in net.dcll_slices] == [32, 48, 64]
    assert not net.sequence_any_supported() and net.sequence_any_supported(wide=True)
    x = _mnist_input(dev, T, B)
    net.reset()
    with G.ops_trace() as tr:
        res = net.test_sequence_any(x, keep_spikes=True, wide=True)
    seq = [n for n in tr.names if n.startswith("k_lif_seq")]
    assert len(seq) == 3 and seq[0].startswith("k_lif_seq_any<") and all(n.startswith("k_lif_seq_wide<0,") for n in seq[1:]), seq
    step, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0, netscale=2.0)
    logits = [res["logits"][0].cpu().numpy(), res["logits"][1].cpu().numpy(), res["o"].cpu().numpy()]
    G._compare_with_per_step(net, res, step, x, np.arange(B) % 10, 10, logits)
    stepped, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0, netscale=2.0)
    G._assert_spikes_equal_per_step(net, res, stepped, x)
    _state_equal(net, step)


def test_chunked_batch_equals_whole_batch(dev):
    """test_sequence_any(wide=True) under a pv budget that splits the batch (3 + 1 samples) == the whole batch at once"""
    T, B = 6, 4
    x = _mnist_input(dev, T, B)
    whole, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0, netscale=2.0)
    parts, _ = G._net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0, netscale=2.0)
    per_sample = 4 * T * max(s.dclllayer.out_channels * int(np.prod(s.dclllayer.output_shape)) for s in parts.dcll_slices)
    parts.pv_budget_bytes = 3 * per_sample + 1
    whole.reset()
    parts.reset()
    ra = whole.test_sequence_any(x, keep_spikes=True, wide=True)
    with G.ops_trace() as tr:
        rb = parts.test_sequence_any(x, keep_spikes=True, wide=True)
    assert sum(n.startswith("k_lif_seq_wide") for n in tr.names) == 4 and sum(n.startswith("k_lif_seq_any") for n in tr.names) == 2
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and ra["spikes"][i].shape[1] == B
        assert float((ra["logits"][i] - rb["logits"][i]).abs().max()) <= 2 * LOGIT_TOL
        assert torch.equal(ra["clout"][i], rb["clout"][i]) and torch.equal(ra["vote"][i], rb["vote"][i])
        assert torch.equal(ra["lowhigh"][i], rb["lowhigh"][i])
    _state_equal(whole, parts)


# ---------------------------------------------------------------------------------------------- entry points
def test_entry_point_train_wide_sequence_path(tmp_path, capsys):
    """train.py --netscale 2 on synthetic IQ at the 16x16 plane: the periodic test with --wide_sequence_path runs k_lif_seq_wide
    and reports the accuracies of the same command without the flag (evaluate_batch's per-step loop); at netscale 1 on 16x16 the
    flag is ignored with a notice"""
    import train
    common = ['--I_resolution', '16', '--Q_resolution', '16', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '12',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    with G.ops_trace() as tr:
        out_wide = train.main(common + ['--netscale', '2', '--output', str(tmp_path / 'wide'), '--wide_sequence_path'])
    assert sum(n.startswith("k_lif_seq_wide") for n in tr.names) == 3
    assert "ignored" not in capsys.readouterr().out
    with G.ops_trace() as tr:
        out_step = train.main(common + ['--netscale', '2', '--output', str(tmp_path / 'step')])
    assert not any(n.startswith("k_lif_seq_wide") for n in tr.names)
    a, b = np.load(os.path.join(out_wide, 'acc_test.npy')), np.load(os.path.join(out_step, 'acc_test.npy'))
    assert a.shape == b.shape == (1, 1, 3) and np.isfinite(a).all() and np.array_equal(a, b)
    capsys.readouterr()
    with G.ops_trace() as tr:
        train.main(common + ['--output', str(tmp_path / 'n1'), '--wide_sequence_path', '--eval_only'])
    assert "--wide_sequence_path ignored: " in capsys.readouterr().out and not any(n.startswith("k_lif_seq_wide") for n in tr.names)

