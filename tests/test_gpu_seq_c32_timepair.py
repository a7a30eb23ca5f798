"""k_lif_seq_c32d, time-paired: an MFMA tile is ONE image row at TWO consecutive timesteps, every tap row in the zero
padding is skipped, and the two LDS trace images are advanced in place (even T >= 8; odd T >= 8 runs the row-paired
k_lif_seq_c32rp).  Everything here is compared with the pinned-order C oracle bit for bit — v, spikes, final eps0 / eps1 /
arp — and pv within PV_TOL, for every sample; each case also proves, through dcll_kernel_trace, which kernel served it.

The inputs are chosen so that a wrongly skipped or wrongly kept tap row, a wrong row of the rolling trace update or a
wrong half of a spike word shows: all-ones planes (every in-image tap contributes), spikes only in the border rows /
border columns, one live pixel per corner; two consecutive calls on the same state buffers (even then odd, odd then even)
exercise the write-back of the in-place images."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import PV_TOL, _rand_layer, _sd_from, bits_equal, cu, dev  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ["ones", "border_rows", "border_cols", "corners", "random"]


def _window(kind, rng, T):
    """(T, 32, 16, 16) input spikes of one sample"""
    if kind == "ones":
        return np.ones((T, 32, 16, 16), np.float32)
    if kind == "corners":
        x = np.zeros((T, 32, 16, 16), np.float32)
        for y, c in ((0, 0), (0, 15), (15, 0), (15, 15)):
            x[:, :, y, c] = rng.uniform(size=(T, 32)) < 0.6
        x[0, :, 0, 0] = x[0, :, 0, 15] = x[0, :, 15, 0] = x[0, :, 15, 15] = 1
        return x
    x = (rng.uniform(size=(T, 32, 16, 16)) < (0.08 if kind == "random" else 0.3)).astype(np.float32)
    if kind == "random":
        x[0] = rng.uniform(size=(32, 16, 16)) < 0.5
    if kind == "border_rows":
        x[:, :, 3:13, :] = 0
    if kind == "border_cols":
        x[:, :, :, 3:13] = 0
    return x


def _inputs(kinds, rng, T, B):
    """(T, B, 32, 256): sample i takes kinds[i], the samples beyond the list are seeded random windows"""
    x = np.stack([_window(kinds[i] if i < len(kinds) else "random", rng, T) for i in range(B)], axis=1)
    return np.ascontiguousarray(x.reshape(T, B, 32, 256))


def _check_calls(dev, seed, wrp, int8, B, Ts, kinds, zero_state):
    """consecutive calls of lengths Ts on the same state buffers, every one against the oracle stepping on"""
    from snn_modulation_classification_amd import ops, quant
    from oracle import c_oracle as C
    rng = np.random.RandomState(seed)
    W, b, alpha, tau_m, alphas, tau_s = _rand_layer(rng, 32, 32, gain=3.0)
    q8 = None
    if int8:
        q, scale = quant.quantize_int8_per_channel(torch.from_numpy(W))
        W = quant.dequantize(q, scale).numpy()
        q8 = (q.to(dev), scale.to(dev))
    sd = _sd_from(W, b, alpha, tau_m, alphas, tau_s, (16, 16), rng=rng)
    orc = C.OracleConvLayer(sd, (16, 16), 3, 1, wrp)
    orc.init_state(B)
    if not zero_state:
        orc.state[0][...] = rng.uniform(0, 5, size=orc.state[0].shape)
        orc.state[1][...] = rng.uniform(0, 50, size=orc.state[1].shape)
        orc.state[2][...] = -rng.uniform(0, 2, size=orc.state[2].shape)
    eps0, eps1, arp = [cu(s.copy(), dev) for s in orc.state]
    d = ops.make_conv_desc(32, 32, (16, 16), 7, 3, 1, 24, False, True, wrp)
    tau4 = cu(np.stack([alpha, tau_m, alphas, tau_s]), dev)
    nspk = 0
    for T in Ts:
        x = _inputs(kinds, rng, T, B)
        spk_in = ops.pack_spikes(cu(x, dev))
        with ops.kernel_trace() as tr:
            spk, pv, v = ops.conv_lif_sequence(d, spk_in, None if int8 else cu(W, dev), cu(b, dev), tau4, eps0, eps1, arp,
                                               T, B, want_v=True, q8=q8)
        torch.cuda.synchronize()
        # which kernel ran: even T >= 8 the time-paired one, odd T >= 8 the row-paired fallback
        served = [n for n in tr.names if n.startswith("k_lif_seq_c32")]
        assert served == (["k_lif_seq_c32d"] if T % 2 == 0 else ["k_lif_seq_c32rp"]), (T, tr.names)
        spk_d = ops.unpack_spikes(spk).cpu().numpy().reshape(T, B, 32, 16, 16)
        v, pv = v.cpu().numpy(), pv.cpu().numpy()
        for t in range(T):
            _, _, opv, ov, os_ = orc.forward(x[t].reshape(B, 32, 16, 16))
            bad = np.argwhere(v[t].view(np.uint32) != ov.view(np.uint32))
            print("T=%d t=%d: %d of %d membranes differ, max |dv| %.3g, max |dpv| %.3g" %
                  (T, t, len(bad), ov.size, np.abs(v[t] - ov).max(), np.abs(pv[t] - opv).max()))
            assert len(bad) == 0, (T, t, bad[:8])
            assert np.array_equal(spk_d[t], os_), (T, t, np.argwhere(spk_d[t] != os_)[:8])
            np.testing.assert_allclose(pv[t], opv, atol=PV_TOL, rtol=0)
            nspk += int(os_.sum())
        assert bits_equal(eps0.cpu().numpy(), orc.state[0]), T
        assert bits_equal(eps1.cpu().numpy(), orc.state[1]), T
        if wrp > 0:
            assert bits_equal(arp.cpu().numpy(), orc.state[2]), T
    assert nspk > 0, "degenerate test: no spikes"


@pytest.mark.parametrize("kind", KINDS[:4])
@pytest.mark.parametrize("wrp,int8", [(1.0, False), (0.0, True)])
def test_timepair_border_inputs(dev, kind, wrp, int8):
    """Inputs that make a wrongly skipped or wrongly kept tap visible, all three samples of the pattern; carried state."""
    _check_calls(dev, 31, wrp, int8, 3, [10], [kind] * 3, zero_state=False)


@pytest.mark.parametrize("T,wrp,int8,B,zero_state", [(8, 1.0, False, 3, True), (10, 0.0, False, 1, False),
                                                      (12, 1.0, True, 3, False), (14, 0.0, True, 1, True),
                                                      (16, 1.0, False, 1, False), (128, 1.0, True, 1, False),
                                                      (9, 1.0, True, 3, False), (127, 0.0, False, 1, False)])
def test_timepair_lengths(dev, T, wrp, int8, B, zero_state):
    """Even T runs k_lif_seq_c32d, odd T the renamed row-paired kernel (checked by name); refractory and plain layers,
    fp32 and int8 weight sources, zero and carried state; the first samples are the fixed border windows."""
    _check_calls(dev, 37 + T, wrp, int8, B, [T], ["ones", "corners", "border_rows"], zero_state)


@pytest.mark.parametrize("Ts,wrp,int8", [((10, 9, 8), 1.0, False), ((9, 12), 0.0, True), ((8, 8), 1.0, True)])
def test_timepair_consecutive_calls_share_state(dev, Ts, wrp, int8):
    """Two or three calls on the same state buffers, even then odd and odd then even lengths: the "t+1" image is written back
    as eps1(T - 1), and the next call — of either kernel — starts from it."""
    _check_calls(dev, 41, wrp, int8, 3, list(Ts), ["border_cols", "ones"], zero_state=False)


@pytest.mark.parametrize("wrp,int8", [(1.0, True), (0.0, False)])
def test_timepair_batch_above_cu_count(dev, wrp, int8):
    """B = 300 — more workgroups than compute units: the four fixed windows plus 296 seeded random ones, every sample
    checked."""
    _check_calls(dev, 43, wrp, int8, 300, [16], KINDS[:4], zero_state=False)
