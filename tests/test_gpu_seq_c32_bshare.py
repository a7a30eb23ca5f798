"""k_lif_seq_c32d walks a channel pair by SOURCE ROW: the B fragment of (source row s, kx) is read once and feeds the wave's
two tiles as tap row s + 3 - row of each, and a tap row of A fragments arrives as one 16-byte and one 12-byte load from the
[cp][ky][lane][8] copy that k_c32d_wfrag makes.

What that can get wrong, each through dcll_conv_lif_sequence against the pinned-order C oracle (v equal up to a zero's sign,
pv within PV_TOL, spikes and final eps0 / eps1 / arp bit for bit): a source row credited to the wrong tile or tap row, a kx
shift or a slip in the fragment order, a tap row refetched before its last use (dense weights, carried state), int8 sources,
more workgroups than compute units, a weight workspace shared between streams.  Geometry: refractory, 32 -> 32, 7x7, 16x16."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import PV_TOL, bits_equal, cu, dev  # noqa: F401
from test_gpu_seq_c32_ostat import _Layer, _train, _v_equal

pytestmark = pytest.mark.gpu


def _with_weights(dev, seed, B, W, zero_state=False):
    """a seeded refractory layer whose weights (device tensor and oracle) are W"""
    L = _Layer(dev, seed, 1.0, B, zero_state=zero_state)
    W = np.ascontiguousarray(W, dtype=np.float32)
    L.W.copy_(cu(W, dev))
    L.set_weights(W)
    return L


def _rewind(L, dev):
    """oracle and device back to the layer's first state"""
    for dst, s0 in zip(L.orc.state, L.state0):
        dst[...] = s0
    for s, s0 in zip(L.state, L.state0):
        s.copy_(cu(s0, dev))


@pytest.mark.parametrize("ky", range(7))
def test_bshare_row_by_tap_row(dev, ky):
    """Only tap row ky is nonzero; sample i has input spikes only in image row i and starts from zero state.  Source row i
    reaches output row i + 3 - ky and no other: every other row of sample i — all 16 where that row lies outside the image,
    the 12 padded (row, tap row) combinations over the seven cases — is exactly the bias path, i.e. what the same layer gives
    with all weights zero."""
    B, T = 16, 8
    rng = np.random.RandomState(300 + ky)
    W = np.zeros((32, 32, 7, 7), np.float32)
    W[:, :, ky, :] = rng.uniform(-1, 1, size=(32, 32, 7))
    L = _with_weights(dev, 310 + ky, B, W, zero_state=True)
    Z = _with_weights(dev, 310 + ky, B, np.zeros_like(W), zero_state=True)
    x = np.zeros((T, B, 32, 16, 16), np.float32)
    for i in range(B):
        x[:, i, :, i, :] = rng.uniform(size=(T, 32, 16)) < 0.5
    ref = L.reference(x)
    got = L.launch(x, want_v=True)
    L.check(got, ref, what="ky=%d" % ky)
    v = got[2].cpu().numpy().reshape(T, B, 32, 16, 16)
    bias_path = Z.reference(x)[0]
    padded = 0
    for i in range(B):
        r = i + 3 - ky
        rows = [q for q in range(16) if q != r]
        assert _v_equal(v[:, i][:, :, rows], bias_path[:, i][:, :, rows]), ("source row", i, "leaked beyond output row", r)
        if 0 <= r <= 15:
            assert not _v_equal(v[:, i, :, r], bias_path[:, i, :, r]), ("source row", i, "missing in output row", r)
        else:
            padded += 1
    assert padded == abs(ky - 3)


@pytest.mark.parametrize("ky", range(7))
def test_bshare_single_tap(dev, ky):
    """one call per tap (ky, kx), B = 2, T = 8: only that tap is nonzero, with a distinct value per (co, ci) — a kx shift or
    a slip in the 4 + 3 packing of a tap row moves or drops it"""
    B, T = 2, 8
    L = _Layer(dev, 400 + ky, 1.0, B)
    x = _train("0.3", L.rng, T, B)
    val = ((np.arange(32 * 32, dtype=np.float32).reshape(32, 32) + 1) / 1024) * np.where(np.arange(32)[:, None] % 2, -1, 1)
    for kx in range(7):
        W = np.zeros((32, 32, 7, 7), np.float32)
        W[:, :, ky, kx] = val * np.float32(1 + kx / 8)
        L.W.copy_(cu(W, dev))
        L.set_weights(W)
        _rewind(L, dev)
        L.check(L.launch(x, want_v=True), L.reference(x), what="tap (%d, %d)" % (ky, kx))


@pytest.mark.parametrize("int8", [False, True])
def test_bshare_dense_carried_state(dev, int8):
    """dense random weights, calls of T = 8, 10, 8 on carried state at B = 3 == one oracle run of 26 steps; with int8 weights
    through dcll_layer_opts the outputs also equal, bit for bit, those of the layer given the dequantised weights as fp32"""
    B = 3
    L = _Layer(dev, 501, 1.0, B, int8=int8)
    twin = _with_weights(dev, 501, B, L.sd["i2h.weight"]) if int8 else None
    x = _train("0.3", L.rng, 26, B)
    ov, opv, os_ = L.reference(x)
    for sl in (slice(0, 8), slice(8, 18), slice(18, 26)):
        got = L.launch(x[sl], want_v=True)
        if twin is not None:
            for p, q in zip(got, twin.launch(x[sl], want_v=True)):
                assert torch.equal(p.view(torch.int32), q.view(torch.int32)), ("int8 vs dequantised twin", sl)
        from snn_modulation_classification_amd import ops
        assert _v_equal(got[2].cpu().numpy().reshape(ov[sl].shape), ov[sl]), sl
        assert np.array_equal(ops.unpack_spikes(got[0]).cpu().numpy().reshape(os_[sl].shape), os_[sl]), sl
        np.testing.assert_allclose(got[1].cpu().numpy().reshape(opv[sl].shape), opv[sl], atol=PV_TOL, rtol=0)
    for s, o in zip(L.state, L.orc.state):
        assert bits_equal(s.cpu().numpy(), o)
    if twin is not None:
        for s, q in zip(L.state, twin.state):
            assert torch.equal(s.view(torch.int32), q.view(torch.int32))


def test_bshare_grid_beyond_residency(dev):
    """B = 600 at T = 8: more than two workgroups per compute unit, every sample checked"""
    L = _Layer(dev, 601, 1.0, 600)
    x = _train("0.08", L.rng, 8, 600)
    L.check(L.launch(x, want_v=True), L.reference(x), what="B=600")


def test_bshare_two_streams(dev):
    """two layers with different weights, launched back to back on two streams: each has its own weight workspace"""
    B = 24
    La, Lb = _Layer(dev, 701, 1.0, B), _Layer(dev, 703, 1.0, B)
    xa, xb = _train("0.1", La.rng, 8, B), _train("0.3", Lb.rng, 8, B)
    ra, rb = La.reference(xa), Lb.reference(xb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = {}
    for rep in range(3):
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


def test_bshare_repeatable_and_logged(dev):
    """a second run from the same state is bit-identical, and the launch log names the layer kernel, not the weight helper"""
    from snn_modulation_classification_amd import ops
    L = _Layer(dev, 801, 1.0, 3)
    x = _train("0.3", L.rng, 10, 3)
    spk_in = ops.pack_spikes(cu(x.reshape(10, 3, 32, 256), dev))        # (the packing kernel is not part of the call)
    with ops.kernel_trace() as tr:
        got = ops.conv_lif_sequence(L.d, spk_in, L.W, L.b, L.tau4, *L.state, 10, 3, q8=L.q8, want_v=True)
    torch.cuda.synchronize()
    assert list(tr.names) == ["k_lif_seq_c32d"], tr.names
    L.check(got, L.reference(x), what="first run")
    first = [t.clone() for t in got] + [s.clone() for s in L.state]
    for s, s0 in zip(L.state, L.state0):
        s.copy_(cu(s0, dev))
    again = list(L.launch(x, want_v=True)) + L.state
    for a, c in zip(first, again):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), "repeated run differs"
