"""dcll_conv_lif_sequence_any (ABI 8, k_lif_seq_any) on the GPU: the fused all-T kernel of any plain conv layer against the
pinned-order C oracle stepped T times, case list tests/seq_any_cases.py (proven on the CPU by tests/test_seq_any_cases.py), and
the network level above it — ConvNetwork.test_sequence_any against the oracle, the per-step loop, test_sequence and the CLI.

v is compared bit for bit up to the sign of a zero (a chain of odd length ends with fmaf(0, 0, acc), which turns an
accumulator of -0.0 into +0.0 where the oracle drops the link); pooled spikes and the final eps0 / eps1 / arp bit for bit; pv
within 1e-4."""
import collections
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import seq_any_cases as A
from conftest import ROOT, unpack_bits

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "snn_modulation_classification_amd")
LOGIT_TOL = 1e-4
PV_TOL = 1e-4
MARGIN = 2e-4           # twice the readout tolerance: below it two correct paths may order the two best logits differently
CASES = A.cases()
REFUSE = A.refusals()
SERVED = collections.Counter()
RAN = set()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c.get("tau_tensor", 0), 1.0 if c["refractory"] else 0.0, c.get("alpharp", A.ALPHARP),
                              c["stride"], c["dilation"], c["groups"])


def _tile(a, B, axis):
    """device sample i = oracle sample i % B_checked"""
    reps = -(-B // a.shape[axis])
    return np.ascontiguousarray(np.take(np.concatenate([a] * reps, axis=axis), np.arange(B), axis=axis))


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(a == 0, np.float32(0), a).view(np.uint32)          # (-0.0 == +0.0: the module docstring)


def _same(got, ref, axis, tag, zero_sign=False):
    """every block of B_checked device samples == the oracle's, bit for bit"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    Bc = ref.shape[axis]
    view = _bits if zero_sign else (lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32))
    for j in range(0, got.shape[axis], Bc):
        n = min(Bc, got.shape[axis] - j)
        g, r = np.take(got, np.arange(j, j + n), axis=axis), np.take(ref, np.arange(n), axis=axis)
        if not np.array_equal(view(g), view(r)):
            bad = np.argwhere(g != r)
            raise AssertionError((tag, "samples from %d" % j, "%d of %d differ" % (len(bad), g.size), bad[:4].tolist(),
                                  "max |diff| %.3g" % float(np.abs(g - r).max())))


def run_case(c, dev, run=None, count=True):
    """every call of a case on the device against the oracle's trajectory -> host copies of every call's outputs and state.
    run: (tensors, trajectory) of another draw of the same geometry (tests/value_cases.py), not counted as a case of this file"""
    from snn_modulation_classification_amd import ops
    T_, traj = A.run(c) if run is None else run
    outs = []
    B = c["B"]
    ch, cw, ph, pw = A.out_shape(c)
    d = _desc(c)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    W, b = cu(T_["W"]), (cu(T_["b"]) if T_["b"] is not None else None)
    tau4 = cu(np.stack(T_["tau"]).astype(np.float32))
    eps0, eps1 = cu(_tile(T_["eps0"], B, 0)), cu(_tile(T_["eps1"], B, 0))
    arp = cu(_tile(T_["arp"], B, 0)) if c["refractory"] else None
    for k, (call, ref) in enumerate(zip(T_["calls"], traj)):
        n = call["x"].shape[0]
        x = _tile(call["x"], B, 1).reshape(n, B, c["c_in"], c["h"] * c["w"])
        if c["seed"] % 2:           # the device packer, or its numpy restatement
            spk_in = ops.pack_spike_planes(cu(x))
        else:
            spk_in = cu(A.pack_planes(x).view(np.int32))
        with ops.kernel_trace() as tr:
            spk, pv, v = ops.conv_lif_sequence_any(d, spk_in, W, b, tau4, eps0, eps1, arp, n, B, want_v=True)
        torch.cuda.synchronize()
        assert tr.names == ["k_seq_any_wprep", A.variant(c)], (c["id"], tr.names)
        tag = (c["id"], "call %d" % k)
        _same(v, ref["v"], 1, tag + ("v",), zero_sign=True)
        _same(ops.unpack_spike_planes(spk, ph * pw).reshape(n, B, c["c_out"], ph, pw), ref["s"], 1, tag + ("spikes",))
        got_pv = pv.cpu().numpy()
        worst = max(float(np.abs(got_pv[:, j:j + ref["pv"].shape[1]] - ref["pv"][:, :B - j]).max()) for j in range(0, B, ref["pv"].shape[1]))
        assert worst <= PV_TOL, tag + ("pv", worst)
        if (ph * pw) % 32:          # tail bits of the last word are zero
            assert not bool((spk[..., -1].cpu().numpy().view(np.uint32) >> np.uint32((ph * pw) % 32)).any()), tag
        _same(eps0, ref["eps0"], 0, tag + ("eps0",))
        _same(eps1, ref["eps1"], 0, tag + ("eps1",))
        if c["refractory"]:
            _same(arp, ref["arp"], 0, tag + ("arp",))
        outs.append([t.cpu().numpy().copy() for t in (spk, pv, v, eps0, eps1) + ((arp,) if c["refractory"] else ())])
    if count:
        SERVED[A.variant(c)] += 1
        RAN.add(c["id"])
    return outs


# ---------------------------------------------------------------------------------------------- 1, 3, 4: the case list
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_against_the_oracle(dev, case):
    """every case (named layers, variants, boundaries, the B = 1100 grid beyond residency, free draws; carried state = consecutive
    calls on one set of state buffers against the oracle stepping straight through)"""
    run_case(case, dev)


def test_every_instantiated_variant_served_a_case(dev):
    """every template instance of k_lif_seq_any the library holds serves a case to the end: the `variants` stratum (one small
    case per instance) is run HERE, each call's launch log read back (run_case asserts it names the instance the restated dispatch
    predicts).  The counts over every case this process ran go to $DCLL_PROFILE_DIR/r09_seq_any_variant_counts.txt when that
    is set (profiles/ holds a copy of a whole-file run)."""
    before = collections.Counter(SERVED)
    for c in CASES:
        if c["stratum"] == "variants":
            run_case(c, dev)
    here = SERVED - before
    assert set(here) == set(A.all_variants()) and all(here[k] > 0 for k in A.all_variants()), dict(here)
    whole = RAN == {c["id"] for c in CASES}
    lines = ["%-28s %4d" % (k, (SERVED - here)[k] if whole else here[k]) for k in A.all_variants()]
    print("\n".join(lines))
    out = os.environ.get("DCLL_PROFILE_DIR")
    if out:
        with open(os.path.join(out, "r09_seq_any_variant_counts.txt"), "w") as f:
            f.write("k_lif_seq_any<refractory, weights in LDS, register form>: cases served (%s, tests/test_gpu_seq_any.py)\n"
                    % ("of all %d cases" % len(CASES) if whole else "the variants stratum alone"))
            f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------- 2: refusals
@pytest.mark.parametrize("r", REFUSE, ids=[r["id"] for r in REFUSE])
def test_refusal(dev, r):
    """the code, a phrase of dcll_last_error(), an empty launch log, nothing written"""
    import ctypes
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()
    d = _desc(r)
    T, B = r["T"], r["B"]
    ch, cw, ph, pw = A.out_shape(r) if A.valid(r) else (1, 1, 1, 1)
    SENT = 12345.0
    f = lambda *shape: torch.full(shape, SENT, device=dev)
    t = dict(spk_in=torch.zeros((max(T, 1), max(B, 1), r["c_in"], (r["h"] * r["w"] + 31) // 32), device=dev, dtype=torch.int32),
             W=f(r["c_out"], r["c_in"] // r["groups"], r["kh"], r["kw"]), b=f(r["c_out"]), tau4=f(4, r["c_in"]),
             eps0=f(max(B, 1), r["c_in"], r["h"], r["w"]), eps1=f(max(B, 1), r["c_in"], r["h"], r["w"]),
             arp=f(max(B, 1), r["c_out"], ch, cw), spk=torch.full((max(T, 1), max(B, 1), r["c_out"], (ph * pw + 31) // 32), 77, device=dev, dtype=torch.int32),
             pv=f(max(T, 1), max(B, 1), r["c_out"], ph, pw), v=f(max(T, 1), max(B, 1), r["c_out"], ch, cw),
             w_scratch=f(max(64 * A.steps(r), 64)))
    p = {k: (None if r["null"] == k else _lib.ptr(x)) for k, x in t.items()}
    with ops.kernel_trace() as tr:
        rc = lib.dcll_conv_lif_sequence_any(ctypes.byref(d), p["spk_in"], p["W"], p["b"], p["tau4"], p["eps0"], p["eps1"], p["arp"],
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
        assert not ops.sequence_any_supported(d)


# ---------------------------------------------------------------------------------------------- 5: the packer
@pytest.mark.parametrize("hw", [1, 31, 33, 81, 169, 256, 737])
def test_pack_unpack_round_trip(dev, hw):
    from snn_modulation_classification_amd import ops
    rng = np.random.RandomState(hw)
    dense = (rng.rand(7, 3, hw) < .4).astype(np.float32)
    packed = ops.pack_spike_planes(torch.from_numpy(dense).to(dev))
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (7, 3, (hw + 31) // 32)
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), A.pack_planes(dense))        # the word layout, tail bits zero
    back = ops.unpack_spike_planes(packed, hw)
    assert tuple(back.shape) == (7, 3, hw) and np.array_equal(back.cpu().numpy(), dense)
    if hw % 32 == 0:
        assert torch.equal(packed, ops.pack_spikes(torch.from_numpy(dense).to(dev)))         # the existing format


# ---------------------------------------------------------------------------------------------- 6 - 8: networks
def _args(**kw):
    a = dict(netscale=1.0, alpha=.92, alphas=.85, alpharp=.65, arp=1.0, lc_ampl=.5, random_tau=True)
    a.update(kw)
    return Namespace(**a)


def _net(spec, im_dims, B, target, **kw):
    from snn_modulation_classification_amd.networks import ConvNetwork, load_network_spec
    convs = load_network_spec(os.path.join(PKG, "networks", spec))
    torch.manual_seed(1)
    np.random.seed(1)
    net = ConvNetwork(_args(**kw), im_dims, B, convs, target, act=torch.nn.Sigmoid(), loss=None, opt=None, opt_param={},
                      learning_rates=None, burnin=20)
    net.reset(True)
    return net, convs


def _one_hot_labels(labels, T, n):
    y = torch.zeros(T, len(labels), n)
    y[:, np.arange(len(labels)), labels] = 1
    return y


def _wide_margin(logits):
    """(T, B) bool: the two best logits are further apart than MARGIN"""
    top2 = np.sort(np.asarray(logits), axis=-1)[..., -2:]
    return (top2[..., 1] - top2[..., 0]) > MARGIN


def _per_step_spikes(net, x_steps):
    """a network stepped slice by slice through the per-step C ABI (dcll_conv_lif_step: Conv2dDCLLlayer's own step call, which
    also hands out the output layer's spikes) -> per layer the pooled spikes (T, B, C, ph, pw)"""
    out = [[] for _ in net.dcll_slices]
    net.reset()
    with torch.no_grad():
        for t in range(len(x_steps)):
            cur = x_steps[t]
            for i, sl in enumerate(net.dcll_slices):
                L = sl.dclllayer
                cur = L.i2h._step(cur, L.pooling, L.i2o, L.output_ if L.output_layer else None,
                                  stacked=L.stacked_readout() if L.output_layer else None)[0]
                out[i].append(cur.cpu().numpy().copy())
    return [np.stack(o) for o in out]


def _assert_spikes_equal_per_step(net, res, stepped, x_steps):
    """every layer's spikes of test_sequence_any (keep_spikes) == those of network `stepped` run per step on the same input, for
    every t, bit for bit; so is the final neuron state"""
    from snn_modulation_classification_amd import ops
    ref = _per_step_spikes(stepped, x_steps)
    for i, sl in enumerate(net.dcll_slices):
        L = sl.dclllayer
        ph, pw = L.output_shape
        got = ops.unpack_spike_planes(res["spikes"][i], ph * pw).cpu().numpy().reshape(ref[i].shape)
        assert ref[i].shape == (len(x_steps), x_steps.shape[1], L.out_channels, ph, pw)
        assert np.array_equal(got, ref[i]), ("per-step spikes", i, np.argwhere(got != ref[i])[:3].tolist())
        assert 0 < ref[i].mean() < 1, ("layer %d never / always spikes" % i)
        for u, v in zip(L.i2h.state, stepped.dcll_slices[i].dclllayer.i2h.state):
            assert torch.equal(u, v), ("final state", i)
    return ref


def _compare_with_per_step(net, res, step, x_steps, labels, n_classes, orc_logits, max_excluded=.01):
    """`res` of net.test_sequence_any (collect=True) against net `step` run with the per-step loop on the same input: clout and
    votes equal wherever the ORACLE's top-2 margin exceeds MARGIN, at most max_excluded of the (layer, t, b) entries excluded;
    accuracy() and confusion_matrix() equal.  -> the excluded share"""
    T = len(x_steps)
    step.reset()
    for t in range(T):
        step.test(x_steps[t])
    wide = np.stack([_wide_margin(lg) for lg in orc_logits])                # (layer, T, B)
    excluded = 1.0 - float(wide.mean())
    print("entries excluded by the oracle's top-2 margin: %d of %d" % (int((~wide).sum()), wide.size))
    assert excluded <= max_excluded
    y = _one_hot_labels(labels, T, n_classes)
    for i, (a, b) in enumerate(zip(net.dcll_slices, step.dcll_slices)):
        seq_clout, step_clout = np.array(a.clout), np.array(b.clout)
        assert seq_clout.shape == step_clout.shape == wide[i].shape
        assert np.array_equal(seq_clout, res["clout"][i].cpu().numpy())
        assert np.array_equal(seq_clout[wide[i]], step_clout[wide[i]]), ("clout", i)
        ok = wide[i].all(axis=0)             # samples whose every step has a wide margin: the votes must agree
        assert ok.any()
        assert np.array_equal(res["vote"][i].cpu().numpy()[ok], b._predictions(y)[0].astype(np.int64)[ok]), ("vote", i)
        assert a.iter == b.iter
    assert net.accuracy(y) == step.accuracy(y)
    assert np.array_equal(net.confusion_matrix(y), step.confusion_matrix(y))
    return excluded


def test_network_mnist_config1(dev, golden):
    """BASELINE config 1 (mnist_conv.yaml on 28x28, arp 0) through test_sequence_any on fixture g2_mnist_t50_b4: spikes of layers
    0-1 bit-equal to the C oracle, logits within LOGIT_TOL, clout agreement with the reference's > .99, and equal to the per-step
    loop under the margin rule.  Share of (layer, t, b) entries the oracle's top-2 margin excludes: 0 of 600 (computed on the CPU
    with oracle/ before the first GPU run)."""
    from oracle import c_oracle as C
    g = golden("g2_mnist_t50_b4.npz")
    net, convs = _net("mnist_conv.yaml", (1, 28, 28), 4, 10, arp=0.0)
    assert not net.sequence_supported() and net.sequence_any_supported()
    orc = C.OracleConvNetwork([g.sub("sd/%d/" % i) for i in range(3)], convs, (28, 28), 0.0)
    xs = unpack_bits(g["x"], 28 * 28)
    T, B = xs.shape[:2]
    xs = xs.reshape(T, B, 1, 28, 28)
    outs = [orc.step(xs[t]) for t in range(T)]
    net.reset()
    x = torch.from_numpy(xs).to(dev)
    with ops_trace() as tr:
        res = net.test_sequence_any(x.to(torch.bool), keep_spikes=True)          # (any dtype: packed on the device)
    assert sum(n.startswith("k_lif_seq_any") for n in tr.names) == 3 and "k_conv_lif" not in " ".join(tr.names)
    from snn_modulation_classification_amd import ops
    for i, L in enumerate(s.dclllayer for s in net.dcll_slices):
        ph, pw = L.output_shape
        got = ops.unpack_spike_planes(res["spikes"][i], ph * pw).cpu().numpy().reshape(T, B, L.out_channels, ph, pw)
        if i < 2:           # (the oracle network hands out the output layer's logits in place of its spikes)
            assert np.array_equal(got, np.stack([o[i]["s"] for o in outs])), ("spikes", i)
        np.testing.assert_allclose(res["logits"][i].cpu().numpy(), np.stack([o[i]["p"] for o in outs]), atol=LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(res["o"].cpu().numpy(), np.stack([o[2]["o"] for o in outs]), atol=LOGIT_TOL, rtol=0)
    agree = np.mean([np.mean(res["clout"][i].cpu().numpy() == g["clout/%d" % i]) for i in range(3)])
    assert agree > 0.99
    step, _ = _net("mnist_conv.yaml", (1, 28, 28), 4, 10, arp=0.0)
    orc_logits = [np.stack([o[i]["o" if i == 2 else "p"] for o in outs]) for i in range(3)]
    excluded = _compare_with_per_step(net, res, step, x, np.arange(B) % 10, 10, orc_logits)
    assert excluded == 0.0
    stepped, _ = _net("mnist_conv.yaml", (1, 28, 28), 4, 10, arp=0.0)
    _assert_spikes_equal_per_step(net, res, stepped, x)           # all three layers, every t; final state
    for a, b in zip(net.dcll_slices, step.dcll_slices):          # ... and the state the net.test loop left
        for u, v in zip(a.dclllayer.i2h.state, b.dclllayer.i2h.state):
            assert torch.equal(u, v)
    # the packed form of the same planes is accepted as it is
    net.reset()
    res2 = net.test_sequence_any(ops.pack_spike_planes(x.reshape(T, B, 1, 28 * 28)), collect=False)
    assert all(torch.equal(a, b) for a, b in zip(res["clout"], res2["clout"]))


class ops_trace:
    """ops.kernel_trace, imported late (the package loads the library on import of ops)"""

    def __enter__(self):
        from snn_modulation_classification_amd import ops
        self._tr = ops.kernel_trace()
        return self._tr.__enter__()

    def __exit__(self, *exc):
        return self._tr.__exit__(*exc)


def _radio_oracle(net, convs, R, cells):
    from oracle import c_oracle as C
    sds = [{k: v.detach().cpu().numpy() for k, v in s.dclllayer.state_dict().items()} for s in net.dcll_slices]
    orc = C.OracleConvNetwork(sds, convs, (R, R), 1.0)
    T, B = cells.shape
    outs = []
    for t in range(T):
        x = np.zeros((B, 1, R * R), np.float32)
        x[np.arange(B), 0, cells[t]] = 1
        outs.append(orc.step(x.reshape(B, 1, R, R)))
    return outs


def test_network_radio_ml_24x24(dev):
    """radio_ml_conv.yaml on a 24x24 plane (no geometry-specialised sequence kernel: the 32 -> 32 layers run the register form of
    k_lif_seq_any), T = 32, B = 3, cell indices in: == the per-step loop under the margin rule and == the C oracle's spikes.
    Share of (layer, t, b) entries the oracle's top-2 margin excludes with this seed: 1 of 288 = 0.35 % (CPU, oracle/)."""
    from snn_modulation_classification_amd import ops
    R, T, B = 24, 32, 3
    net, convs = _net("radio_ml_conv.yaml", (1, R, R), B, 24)
    assert not net.sequence_supported() and net.sequence_any_supported()
    cells = np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)
    outs = _radio_oracle(net, convs, R, cells)
    net.reset()
    with ops_trace() as tr:
        res = net.test_sequence_any(torch.from_numpy(cells).to(dev), keep_spikes=True)
    assert [n for n in tr.names if n.startswith("k_lif_seq_any")] == ["k_lif_seq_any<1,1,0>", "k_lif_seq_any<1,0,1>", "k_lif_seq_any<1,0,1>"]
    for i in range(3):
        got = ops.unpack_spike_planes(res["spikes"][i], R * R).cpu().numpy().reshape(T, B, 32, R, R)
        assert np.array_equal(got, np.stack([o[i]["s"] for o in outs])), ("spikes", i)
        np.testing.assert_allclose(res["logits"][i].cpu().numpy(), np.stack([o[i]["p"] for o in outs]), atol=LOGIT_TOL, rtol=0)
    step, _ = _net("radio_ml_conv.yaml", (1, R, R), B, 24)
    planes = ops.cells_to_planes(torch.from_numpy(cells).to(dev), R * R).reshape(T, B, 1, R, R)
    orc_logits = [np.stack([o[i]["o" if i == 2 else "p"] for o in outs]) for i in range(3)]
    _compare_with_per_step(net, res, step, planes, np.arange(B) % 24, 24, orc_logits)
    stepped, _ = _net("radio_ml_conv.yaml", (1, R, R), B, 24)
    _assert_spikes_equal_per_step(net, res, stepped, planes)      # all three layers, every t; final state
    for a, b in zip(net.dcll_slices, step.dcll_slices):          # the final neuron state of both paths, bit for bit
        for u, v in zip(a.dclllayer.i2h.state, b.dclllayer.i2h.state):
            assert torch.equal(u, v)


def test_network_radio_ml_16x16_equals_test_sequence(dev):
    """on the 16x16 plane the chain is that of the specialised kernels: spikes of test_sequence_any == test_sequence(keep_spikes)
    bit for bit, logits within twice the readout tolerance, the final state equal"""
    R, T, B = 16, 32, 3
    a, _ = _net("radio_ml_conv.yaml", (1, R, R), B, 24)
    b, _ = _net("radio_ml_conv.yaml", (1, R, R), B, 24)
    assert a.sequence_supported() and a.sequence_any_supported()
    cells = torch.from_numpy(np.random.RandomState(0).randint(0, R * R, size=(T, B)).astype(np.int32)).to(dev)
    a.reset()
    b.reset()
    ra = a.test_sequence_any(cells, keep_spikes=True)
    rb = b.test_sequence(cells, keep_spikes=True)
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]), i
        assert float((ra["logits"][i] - rb["logits"][i]).abs().max()) <= 2 * LOGIT_TOL
        for u, v in zip(a.dcll_slices[i].dclllayer.i2h.state, b.dcll_slices[i].dclllayer.i2h.state):
            assert torch.equal(u, v)
        assert a.dcll_slices[i].iter == b.dcll_slices[i].iter == T


def test_unsupported_network_raises(dev):
    """radio_ml_conv.yaml on 32x32: the 32 -> 32 layers are outside both forms of the kernel (and served by test_sequence)"""
    from snn_modulation_classification_amd import _lib
    net, _ = _net("radio_ml_conv.yaml", (1, 32, 32), 2, 24)
    assert net.sequence_supported() and not net.sequence_any_supported()
    with pytest.raises(_lib.DCLLUnsupported):
        net.test_sequence_any(torch.zeros((2, 2), device=dev, dtype=torch.int32))


def test_entry_point_train_mnist_any_sequence_path(tmp_path):
    """train.py --data MNIST with mnist_conv.yaml for one short epoch: --any_sequence_path exits cleanly and reports the test
    accuracy of the same command without the flag (the per-step test phase)"""
    import train
    common = ['--data', 'MNIST', '--network_spec', os.path.join(PKG, 'networks', 'mnist_conv.yaml'), '--synthetic', '16',
              '--batch_size', '8', '--batch_size_test', '8', '--n_test_samples', '8', '--n_steps', '1', '--n_iters', '10',
              '--n_iters_test', '10', '--burnin', '4', '--n_test_interval', '1', '--learning_rates', '1e-7']
    with ops_trace() as tr:
        out_any = train.main(common + ['--output', str(tmp_path / 'any'), '--any_sequence_path'])
    assert sum(n.startswith("k_lif_seq_any") for n in tr.names) == 3
    with ops_trace() as tr:
        out_step = train.main(common + ['--output', str(tmp_path / 'step')])
    assert not any(n.startswith("k_lif_seq_any") for n in tr.names)
    a, b = np.load(os.path.join(out_any, 'acc_test.npy')), np.load(os.path.join(out_step, 'acc_test.npy'))
    assert a.shape == b.shape == (1, 1, 3) and np.isfinite(a).all() and np.array_equal(a, b)


def test_entry_point_train_radio_ml_24x24_any_sequence_path(tmp_path):
    """train.py on synthetic IQ at a 24x24 plane (no specialised sequence kernel): the periodic test with --any_sequence_path runs
    k_lif_seq_any and reports the accuracies of the same command without the flag (evaluate_batch's per-step loop)"""
    import train
    common = ['--I_resolution', '24', '--Q_resolution', '24', '--arp', '1.0', '--burnin', '4', '--batch_size', '8',
              '--batch_size_test', '8', '--n_test_samples', '8', '--synthetic', '8', '--n_iters', '8', '--n_iters_test', '12',
              '--n_steps', '1', '--n_test_interval', '1', '--learning_rates', '1e-7']
    with ops_trace() as tr:
        out_any = train.main(common + ['--output', str(tmp_path / 'any'), '--any_sequence_path'])
    assert sum(n.startswith("k_lif_seq_any") for n in tr.names) == 3
    with ops_trace() as tr:
        out_step = train.main(common + ['--output', str(tmp_path / 'step')])
    assert not any(n.startswith("k_lif_seq_any") for n in tr.names)
    a, b = np.load(os.path.join(out_any, 'acc_test.npy')), np.load(os.path.join(out_step, 'acc_test.npy'))
    assert a.shape == b.shape == (1, 1, 3) and np.isfinite(a).all() and np.array_equal(a, b)


def test_chunked_batch_equals_whole_batch(dev, golden):
    """test_sequence_any under a pv budget that splits the batch (chunks of 3 + 1 samples on rows of every layer's state) == the
    whole batch at once: spikes, clout, votes, pv statistics and the final state equal, logits within twice the readout tolerance
    (the readout picks its kernel by the row count)"""
    g = golden("g2_mnist_t50_b4.npz")
    xs = unpack_bits(g["x"], 28 * 28)
    T, B = xs.shape[:2]
    x = torch.from_numpy(xs.reshape(T, B, 1, 28, 28)).to(dev)
    whole, _ = _net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    parts, _ = _net("mnist_conv.yaml", (1, 28, 28), B, 10, arp=0.0)
    per_sample = 4 * T * max(s.dclllayer.out_channels * int(np.prod(s.dclllayer.output_shape)) for s in parts.dcll_slices)
    parts.pv_budget_bytes = 3 * per_sample + 1
    whole.reset()
    parts.reset()
    ra = whole.test_sequence_any(x, keep_spikes=True)
    with ops_trace() as tr:
        rb = parts.test_sequence_any(x, keep_spikes=True)
    assert sum(n.startswith("k_lif_seq_any") for n in tr.names) == 6          # two chunks x three layers
    y = _one_hot_labels(np.arange(B) % 10, T, 10)
    for i in range(3):
        assert torch.equal(ra["spikes"][i], rb["spikes"][i]) and ra["spikes"][i].shape[1] == B
        assert float((ra["logits"][i] - rb["logits"][i]).abs().max()) <= 2 * LOGIT_TOL
        assert torch.equal(ra["clout"][i], rb["clout"][i]) and torch.equal(ra["vote"][i], rb["vote"][i])
        assert ra["lowhigh"][i] is not None and len(ra["lowhigh"][i]) == 2 and torch.equal(ra["lowhigh"][i], rb["lowhigh"][i])
        for u, v in zip(whole.dcll_slices[i].dclllayer.i2h.state, parts.dcll_slices[i].dclllayer.i2h.state):
            assert u.shape[0] == B and torch.equal(u, v)
        assert np.array_equal(np.array(whole.dcll_slices[i].clout), np.array(parts.dcll_slices[i].clout))
    assert float((ra["o"] - rb["o"]).abs().max()) <= 2 * LOGIT_TOL
    assert whole.accuracy(y) == parts.accuracy(y)
