"""k_lif_seq_c32d, output-stationary: every wave keeps the accumulators of its two image rows from the bias to the
epilogue, the weights are streamed from a fragment-ordered copy that a helper kernel makes in front of every launch, the
eps1 images exist twice (one pair per step-pair parity) and one barrier per step pair separates them.

What that structure can get wrong, each against the pinned-order C oracle — v equal up to a zero's sign, spikes bit for bit,
final eps0 / eps1 / arp bit for bit, repeated runs bit-identical: the parity of the last step pair, carried state across
calls, the image borders, more workgroups than compute units, every kernel variant, weights changed between calls, two
streams at once, and a launch log that shows the layer kernel alone.  Geometry: 32 -> 32, 7x7, padding 3, 16x16."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import PV_TOL, _rand_layer, _sd_from, bits_equal, cu, dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _v_equal(a, b):
    """equal bit for bit, up to the sign of a zero"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))


def _train(kind, rng, T, B):
    """(T, B, 32, 16, 16) input spikes"""
    x = np.zeros((T, B, 32, 16, 16), np.float32)
    if kind == "empty":
        return x
    if kind == "corners":
        for y, c in ((0, 0), (0, 15), (15, 0), (15, 15)):
            x[:, :, :, y, c] = rng.uniform(size=(T, B, 32)) < 0.6
        x[0, :, :, 0, 0] = x[0, :, :, 0, 15] = x[0, :, :, 15, 0] = x[0, :, :, 15, 15] = 1
        return x
    if kind == "edges":
        r = (rng.uniform(size=x.shape) < 0.4).astype(np.float32)
        x[:, :, :, 0, :], x[:, :, :, 15, :] = r[:, :, :, 0, :], r[:, :, :, 15, :]
        x[:, :, :, :, 0], x[:, :, :, :, 15] = r[:, :, :, :, 0], r[:, :, :, :, 15]
        return x
    return (rng.uniform(size=x.shape) < float(kind)).astype(np.float32)


class _Layer:
    """a seeded layer: its oracle, its state on the device, its descriptor"""

    def __init__(self, dev, seed, wrp, B, int8=False, zero_state=False):
        from snn_modulation_classification_amd import ops, quant
        from oracle import c_oracle as C
        self.dev, self.B, self.wrp, self.C = dev, B, wrp, C
        self.rng = rng = np.random.RandomState(seed)
        W, b, alpha, tau_m, alphas, tau_s = _rand_layer(rng, 32, 32, gain=3.0)
        self.q8 = None
        if int8:        # the oracle runs on the dequantised weights
            q, scale = quant.quantize_int8_per_channel(torch.from_numpy(W))
            W = quant.dequantize(q, scale).numpy()
            self.q8 = (q.to(dev), scale.to(dev))
        self.sd = _sd_from(W, b, alpha, tau_m, alphas, tau_s, (16, 16), rng=rng)
        self.orc = C.OracleConvLayer(self.sd, (16, 16), 3, 1, wrp)
        self.orc.init_state(B)
        if not zero_state:
            self.orc.state[0][...] = rng.uniform(0, 5, size=self.orc.state[0].shape)
            self.orc.state[1][...] = rng.uniform(0, 50, size=self.orc.state[1].shape)
            self.orc.state[2][...] = -rng.uniform(0, 2, size=self.orc.state[2].shape)
        self.state0 = [s.copy() for s in self.orc.state]
        self.state = [cu(s, dev) for s in self.state0]
        self.d = ops.make_conv_desc(32, 32, (16, 16), 7, 3, 1, 24, False, True, wrp)
        self.tau4 = cu(np.stack([alpha, tau_m, alphas, tau_s]), dev)
        self.W, self.b = (None if int8 else cu(W, dev)), cu(b, dev)

    def set_weights(self, W):
        """new weights for the oracle (the device tensor is the caller's to change); the state carries on"""
        st = [s.copy() for s in self.orc.state]
        self.sd = dict(self.sd, **{"i2h.weight": np.ascontiguousarray(W)})
        self.orc = self.C.OracleConvLayer(self.sd, (16, 16), 3, 1, self.wrp)
        self.orc.init_state(self.B)
        for dst, src in zip(self.orc.state, st):
            dst[...] = src

    def launch(self, x, **kw):
        from snn_modulation_classification_amd import ops
        T = x.shape[0]
        spk_in = ops.pack_spikes(cu(x.reshape(T, self.B, 32, 256), self.dev))
        return ops.conv_lif_sequence(self.d, spk_in, self.W, self.b, self.tau4, *self.state, T, self.B, q8=self.q8, **kw)

    def reference(self, x):
        """the oracle stepping on: (v, pv, spikes) of every step"""
        outs = [self.orc.forward(x[t]) for t in range(x.shape[0])]
        return (np.stack([o[3] for o in outs]), np.stack([o[2] for o in outs]), np.stack([o[4] for o in outs]))

    def check(self, got, ref, presig=False, what=""):
        from snn_modulation_classification_amd import ops
        spk, pv, v = got
        ov, opv, os_ = ref
        T = ov.shape[0]
        if v is not None:
            assert _v_equal(v.cpu().numpy().reshape(ov.shape), ov), (what, "v")
        if pv is not None:
            if presig:
                assert _v_equal(pv.cpu().numpy().reshape(ov.shape), ov), (what, "pv (pre-sigmoid)")
            else:
                np.testing.assert_allclose(pv.cpu().numpy().reshape(opv.shape), opv, atol=PV_TOL, rtol=0, err_msg=what)
        if spk is not None:
            got_s = ops.unpack_spikes(spk).cpu().numpy().reshape(T, self.B, 32, 16, 16)
            assert np.array_equal(got_s, os_), (what, "spikes", np.argwhere(got_s != os_)[:8])
        e0, e1, arp = [s.cpu().numpy() for s in self.state]
        assert bits_equal(e0, self.orc.state[0]), (what, "eps0")
        assert bits_equal(e1, self.orc.state[1]), (what, "eps1")
        if self.wrp > 0:
            assert bits_equal(arp, self.orc.state[2]), (what, "arp")


@pytest.mark.parametrize("T", [8, 10, 14])
@pytest.mark.parametrize("B", [1, 3])
def test_ostat_step_pair_parity(dev, T, B):
    """4, 5 and 7 step pairs: the last pair reads either parity of the images; the run repeated from the same state is
    bit-identical."""
    L = _Layer(dev, 100 + T + B, 1.0, B)
    x = _train("0.3", L.rng, T, B)
    got = L.launch(x, want_v=True)
    L.check(got, L.reference(x), what="T=%d B=%d" % (T, B))
    first = [t.clone() for t in got] + [s.clone() for s in L.state]
    for s, s0 in zip(L.state, L.state0):
        s.copy_(cu(s0, dev))
    again = list(L.launch(x, want_v=True)) + L.state
    for a, c in zip(first, again):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "repeated run differs"


@pytest.mark.parametrize("wrp", [1.0, 0.0])
def test_ostat_carried_state_8_then_10(dev, wrp):
    """one call of T = 8 and one of T = 10 on carried state == one oracle run of 18 steps (even, then odd pair count)"""
    L = _Layer(dev, 7, wrp, 3)
    x = _train("0.3", L.rng, 18, 3)
    ov, opv, os_ = L.reference(x)
    a = L.launch(x[:8], want_v=True)
    b = L.launch(x[8:], want_v=True)
    torch.cuda.synchronize()
    from snn_modulation_classification_amd import ops
    for got, sl in ((a, slice(0, 8)), (b, slice(8, 18))):
        assert _v_equal(got[2].cpu().numpy().reshape(ov[sl].shape), ov[sl]), sl
        assert np.array_equal(ops.unpack_spikes(got[0]).cpu().numpy().reshape(os_[sl].shape), os_[sl]), sl
        np.testing.assert_allclose(got[1].cpu().numpy().reshape(opv[sl].shape), opv[sl], atol=PV_TOL, rtol=0)
    for s, o in zip(L.state[:3 if wrp > 0 else 2], L.orc.state):
        assert bits_equal(s.cpu().numpy(), o)


@pytest.mark.parametrize("kind", ["corners", "edges", "empty", "0.02", "0.3", "1.0"])
@pytest.mark.parametrize("wrp", [1.0, 0.0])
def test_ostat_borders_and_rates(dev, kind, wrp):
    """spikes only in the corner / edge pixels of every channel (the shared column padding and the skipped tap rows), an
    empty train, and rates 0.02, 0.3, 1.0"""
    L = _Layer(dev, 23, wrp, 2)
    x = _train(kind, L.rng, 10, 2)
    L.check(L.launch(x, want_v=True), L.reference(x), what=kind)


@pytest.mark.parametrize("wrp,int8", [(1.0, False), (0.0, True)])
def test_ostat_grid_beyond_residency(dev, wrp, int8):
    """B = 300 at T = 8: more workgroups than compute units, every sample checked"""
    L = _Layer(dev, 43, wrp, 300, int8=int8)
    x = _train("0.08", L.rng, 8, 300)
    L.check(L.launch(x, want_v=True), L.reference(x), what="B=300")


@pytest.mark.parametrize("out", [0, 1, 2, 3])
@pytest.mark.parametrize("wrp", [1.0, 0.0])
@pytest.mark.parametrize("spikes", [True, False])
def test_ostat_variants(dev, out, wrp, spikes):
    """refractory and plain layers, OUT = 0..3 (pv / v wanted or not), spk_out NULL (a last layer)"""
    L = _Layer(dev, 61 + out, wrp, 2)
    x = _train("0.3", L.rng, 8, 2)
    got = L.launch(x, want_pv=bool(out & 1), want_v=bool(out & 2), want_spikes=spikes)
    assert (got[0] is not None, got[1] is not None, got[2] is not None) == (spikes, bool(out & 1), bool(out & 2))
    L.check(got, L.reference(x), what="OUT=%d wrp=%g spikes=%d" % (out, wrp, spikes))


@pytest.mark.parametrize("want_v", [False, True])
def test_ostat_presigmoid(dev, want_v):
    """pv_presigmoid: the pv output holds v"""
    L = _Layer(dev, 71, 1.0, 2)
    x = _train("0.3", L.rng, 10, 2)
    L.check(L.launch(x, want_v=want_v, presigmoid=True), L.reference(x), presig=True, what="presigmoid")


@pytest.mark.parametrize("wrp", [1.0, 0.0])
def test_ostat_int8_weights(dev, wrp):
    """int8 weights through dcll_layer_opts == the oracle on the dequantised weights"""
    L = _Layer(dev, 83, wrp, 3, int8=True)
    x = _train("0.3", L.rng, 10, 3)
    L.check(L.launch(x, want_v=True), L.reference(x), what="int8")


def test_ostat_fresh_weights(dev):
    """two calls on one stream, the weight tensor modified in place between them: the second call uses the new weights"""
    L = _Layer(dev, 91, 1.0, 2)
    x = _train("0.3", L.rng, 16, 2)
    L.check(L.launch(x[:8], want_v=True), L.reference(x[:8]), what="first weights")
    W2 = (L.sd["i2h.weight"][::-1] * np.float32(-1.5)).astype(np.float32)
    L.W.copy_(cu(W2, dev))                      # in place: the same device pointer
    L.set_weights(W2)
    second = L.launch(x[8:], want_v=True)
    ref = L.reference(x[8:])
    assert int(ref[2].sum()) > 0
    L.check(second, ref, what="second weights")


def test_ostat_two_streams(dev):
    """two streams run the call at the same time on two layers with different weights, B = 64, T = 8"""
    La, Lb = _Layer(dev, 101, 1.0, 64), _Layer(dev, 103, 0.0, 64)
    xa, xb = _train("0.1", La.rng, 8, 64), _train("0.3", Lb.rng, 8, 64)
    ra, rb = La.reference(xa), Lb.reference(xb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = {}
    for rep in range(3):                        # several rounds queued back to back: the streams overlap
        for L, s, k, x in ((La, sa, "a", xa), (Lb, sb, "b", xb)):
            with torch.cuda.stream(s):
                if rep:
                    for st, s0 in zip(L.state, L.state0):
                        st.copy_(cu(s0, dev), non_blocking=True)
                got[k, rep] = L.launch(x, want_v=True)
    torch.cuda.synchronize()
    La.check(got["a", 2], ra, what="stream a")
    Lb.check(got["b", 2], rb, what="stream b")
    for k in "ab":
        for rep in range(2):
            for p, q in zip(got[k, rep], got[k, 2]):
                assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (k, rep)


@pytest.mark.parametrize("int8", [False, True])
def test_ostat_launch_log(dev, int8):
    """the weight helper is not a layer launch: the log of a call is exactly the layer kernel"""
    from snn_modulation_classification_amd import ops
    L = _Layer(dev, 5, 1.0, 2, int8=int8)
    x = _train("0.3", L.rng, 8, 2)
    spk_in = ops.pack_spikes(cu(x.reshape(8, 2, 32, 256), dev))
    with ops.kernel_trace() as tr:
        ops.conv_lif_sequence(L.d, spk_in, L.W, L.b, L.tau4, *L.state, 8, 2, q8=L.q8)
    torch.cuda.synchronize()
    assert list(tr.names) == ["k_lif_seq_c32d"], tr.names
