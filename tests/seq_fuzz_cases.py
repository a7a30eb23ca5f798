"""Seeded cases for the fused all-T sequence C ABI (dcll_conv_lif_sequence, dcll_conv_lif_sequence_cells, dcll_conv_lif_sequence_iq,
dcll_dense_lif_sequence), their tensors and the C oracle's trajectories.  Plain module: no GPU, no fixtures,
numpy.random.RandomState with fixed seeds only.  tests/test_seq_fuzz_cases.py proves the lists on the CPU;
tests/test_gpu_seq_fuzz.py runs the HIP kernels against them.

A case is a small dict (entry point, geometry, options, wanted outputs, the lengths `Ts` of consecutive calls on ONE set of state
buffers, batch, a sub-seed); its tensors are drawn from the sub-seed by run(), which also steps the pinned-order C oracle through
all the calls.  A failing case can be re-run alone from its id:
    python -c "import seq_fuzz_cases as S; print(S.describe(S.by_id('seq-var-w3-R1-O5-L5-F0')))"

The launchers' dispatch is restated ONCE here (launcher(), variant(), expected_kernels()): csrc/dcll_hip.hip
dcll_conv_lif_sequence_run / launch_c1 / dcll_dense_lif_sequence, csrc/dcll_seq_tiled.hip dcll_launch_seq_c1t / _c32t,
csrc/dcll_seq_w3.hip dcll_launch_seq_w3 / dcll_seq_w3_geometry, csrc/dcll_dense.hip dcll_dense_seq_fits.

Strata (uniform draws never meet the specialised kernels):
  variants    one small case per reachable template variant of every launcher (reachable_variants());
  boundaries  each dispatch condition with its neighbour on the other side;
  carry       two or three consecutive calls on the same state buffers, every family;
  inputs      border / seam / all-ones / all-zero windows for the families that had none;
  grids       grids beyond residency: B device samples that are copies of B_checked <= 8 distinct ones;
  free        uniform draws over all of the above;
  refuse      error returns before any launch (refusals())."""
import hashlib
import json

import numpy as np

import fuzz_cases as FZ

ALPHARP = FZ.ALPHARP
SEED = 20261
RATES = (.02, .1, .3)
WORK_CASE_MAX = 3e9         # multiply-adds of the oracle per case, sum over the calls
WORK_TOTAL_MAX = 6e10       # ... over all cases
WORK_FREE_MAX = 2.5e8       # a free draw
# the launchers' constants, restated once
C32D_MIN_T = 8              # DCLL_C32D_MIN_T
W3_NT = 8                   # tiles of 32 pixels per k_lif_seq_w3 workgroup
DS_MAXIN, DS_MAXOUT = 1024, 128         # dcll_dense_seq_fits
RO_KC = 32                  # the readout's K chunk (launch_readout: `fast`)
HIST_EVERY = 20             # DCLLBase.forward's histogram steps

DEFAULT = dict(entry="seq", layer="k7", c_in=32, c_out=32, h=16, w=16, refractory=1, q8=0, presigmoid=0, want_spikes=1, want_pv=1,
               want_v=1, n_ro=0, lowhigh_iter0=None, Ts=(5,), B=2, B_checked=None, rate=.1, state0=1, pattern=None, t0=0,
               in_features=0, out_features=0, tau_tensor=0, target=10)
LAYERS = {"k7": dict(k=(7, 7), pad=(3, 3), pool=(1, 1)), "w3": dict(k=(1, 3), pad=(0, 1), pool=(1, 2))}


def _case(cid, stratum, seed, **kw):
    c = dict(DEFAULT)
    unknown = set(kw) - set(c) - {"note"}
    assert not unknown, unknown
    c.update(kw)
    c["Ts"] = [int(t) for t in c["Ts"]]
    if c["B_checked"] is None:
        c["B_checked"] = c["B"]
    if c["entry"] != "dense" and c["c_in"] == 1 and c["c_out"] < 8:
        c["state0"] = 1         # (one spike per step on a zero state: v is the bias almost everywhere, a few channels hold one sign)
    if c["entry"] == "dense":
        for k in ("layer", "c_in", "c_out", "h", "w", "q8", "presigmoid", "n_ro", "lowhigh_iter0", "pattern", "t0"):
            c[k] = None
        c["want_pv"] = 1            # (the binding always hands out_pv: the local readout reads it)
    c.update(id=cid, stratum=stratum, seed=int(seed))
    c.setdefault("note", "")
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def out_shape(c):
    """(ch, cw, ph, pw)"""
    return (c["h"], c["w"], c["h"], c["w"] // 2) if c["layer"] == "w3" else (c["h"], c["w"], c["h"], c["w"])


def hist_steps(iter0, T):
    """the steps t of a call whose 1-based iteration count is a histogram step (dcll_pv_lowhigh_steps)"""
    return [] if iter0 is None else [t for t in range(T) if (iter0 + t + 1) % HIST_EVERY == 0]


def launcher(c):
    """the kernel family a case's geometry selects: c32 (16x16: c32 / c32d / c32rp by T), c32t, c1, c1t, w3, w3f, dense"""
    if c["entry"] == "dense":
        return "dense"
    tiled = (c["h"], c["w"]) != (16, 16)
    if c["layer"] == "w3":
        return "w3" if c["c_in"] == 64 else "w3f"
    if c["c_in"] == 32:
        return "c32t" if tiled else "c32"
    return "c1t" if tiled else "c1"


def _k7_outs(c):
    """(pv, v) as a 7x7 kernel gets them: in presigmoid mode v goes out through the v output (presig_outs / launch_c1)"""
    pv, v = c["want_pv"], c["want_v"]
    if c["presigmoid"] and pv:
        return 0, 1
    return pv, v


def variant(c, T):
    """the template instance a call of length T runs: (kernel, switches...)"""
    L, R = launcher(c), int(c["refractory"])
    if L == "dense":
        fits = c["in_features"] <= DS_MAXIN and c["out_features"] <= DS_MAXOUT
        return ("k_dense_lif_seq" if fits else "k_dense_lif_mfma", R)
    if L in ("w3", "w3f"):
        out = c["want_pv"] | (c["want_v"] << 1) | ((c["want_pv"] and c["presigmoid"]) << 2)
        if L == "w3f":
            return ("k_lif_seq_w3f", R, out)
        logw = c["w"].bit_length() - 1
        ntile = c["B"] * (c["h"] * c["w"] // 32)
        return ("k_lif_seq_w3", R, out, min(logw, 5), int(ntile % W3_NT == 0))
    if L in ("c32", "c32t"):
        pv, v = _k7_outs(c)
        out = pv | (v << 1)
        if L == "c32t":
            return ("k_lif_seq_c32t", R, out)
        if c["n_ro"] == 0 and T >= C32D_MIN_T:
            return ("k_lif_seq_c32d" if T % 2 == 0 else "k_lif_seq_c32rp", R, out)
        return ("k_lif_seq_c32", R, out, c["n_ro"])
    # c1 / c1t: F = 1 the fast epilogue (c_out 32, spikes + pv, no v), 2 the same writing v (presigmoid), 0 the guarded one
    both = c["presigmoid"] and c["want_pv"] and c["want_v"]           # (v_out is written, pv_out is a copy of it)
    fast = c["c_out"] == 32 and c["want_spikes"] and c["want_pv"] and not c["want_v"]
    F = 0 if (both or not fast) else (2 if c["presigmoid"] else 1)
    return ("k_lif_seq_c1t" if L == "c1t" else "k_lif_seq_c1", R, F, int(c["entry"] == "iq"))


def expected_kernels(c, T, iter0=None):
    """the launch log of one call of length T (iter0: the iteration count before the call, None = no statistics)"""
    L = launcher(c)
    if L == "dense":
        if variant(c, T)[0] == "k_dense_lif_seq":
            names = ["k_dense_lif_seq"]
        else:
            gy = -(-c["B"] // 128)
            narrow = -(-c["out_features"] // 64) * gy < 512
            names = ["k_trace", "k_dense_lif_mfma (narrow)" if narrow else "k_dense_lif_mfma (wide)"] * T
        rows = T * c["B"]
        fast = c["out_features"] % RO_KC == 0 and c["target"] <= 64         # (torch allocations are 16-byte aligned)
        return names + ["k_readout_rows" if rows <= 2048 else "k_readout_t16" if fast else "k_readout"]
    names = [variant(c, T)[0]]
    if L == "w3f":
        names.append("k_w3f_traces_advance")
    if c["want_pv"] and hist_steps(iter0, T):
        names.append("k_pv_lowhigh")
    return names


def reachable_variants():
    """the full reachable product of every launcher's switches"""
    R2 = (0, 1)
    keys = [("k_lif_seq_w3", r, o, lw, f) for r in R2 for o in (0, 1, 2, 3, 5, 7) for lw in (1, 2, 3, 4, 5) for f in R2]
    keys += [("k_lif_seq_w3f", r, o) for r in R2 for o in (0, 1, 2, 3, 5, 7)]
    keys += [("k_lif_seq_c32", r, o, n) for r in R2 for o in range(4) for n in (0, 24, 48)]
    keys += [(k, r, o) for k in ("k_lif_seq_c32d", "k_lif_seq_c32rp", "k_lif_seq_c32t") for r in R2 for o in range(4)]
    keys += [(k, r, f, q) for k in ("k_lif_seq_c1", "k_lif_seq_c1t") for r in R2 for f in (0, 1, 2) for q in R2]
    keys += [(k, r) for k in ("k_dense_lif_seq", "k_dense_lif_mfma") for r in R2]
    return keys


def work(c):
    """multiply-adds of the oracle: sum over calls of T * B_checked * c_out * ch * cw * c_in * kh * kw"""
    if c["entry"] == "dense":
        per = c["in_features"] * c["out_features"]
    else:
        kh, kw = LAYERS[c["layer"]]["k"]
        per = c["c_out"] * c["h"] * c["w"] * c["c_in"] * kh * kw
    return sum(c["Ts"]) * c["B_checked"] * per


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
def _wants(out):
    """wanted outputs of a k7 layer that reach kernel OUT `out` without presigmoid"""
    return dict(want_pv=out & 1, want_v=(out >> 1) & 1)


def _variant_cases(seed):
    out = []

    def add(name, **kw):
        k = len(out)
        kw.setdefault("rate", RATES[k % 3])
        kw.setdefault("state0", int(k % 4 != 0))
        out.append(_case("seq-var-%s" % name, "variants", seed * 100003 + k, **kw))
    # k_lif_seq_w3<64, R, OUT, LW, FULL>
    n5 = [0, 0]
    for R in (1, 0):
        for O in (0, 1, 2, 3, 5, 7):
            for LW in (1, 2, 3, 4, 5):
                for FULL in (1, 0):
                    if LW < 5:
                        w = 1 << LW
                    else:
                        ws = (32, 64, 128, 256) if FULL else (32, 64, 128)       # (w 256: 8 tiles per row, always full)
                        w = ws[n5[FULL] % len(ws)]
                        n5[FULL] += 1
                    spk = 1 if O == 0 else (len(out) // 2) % 2
                    hw = max(64, w) if spk else max(w, (32, 96)[(len(out) // 4) % 2] if w <= 32 else w)
                    tps = hw // 32
                    if FULL:
                        B = next(b for b in range(1, 9) if (b * tps) % W3_NT == 0)
                    else:
                        B = next(b for b in (3, 1, 2, 5) if (b * tps) % W3_NT != 0)
                    add("w3-R%d-O%d-L%d-F%d" % (R, O, LW, FULL), layer="w3", c_in=64, c_out=64, h=hw // w, w=w, refractory=R,
                        want_spikes=spk, want_pv=O & 1, want_v=(O >> 1) & 1, presigmoid=O >> 2, B=B, Ts=(2 + len(out) % 3,),
                        q8=int(len(out) % 3 == 0))
    # k_lif_seq_w3f<R, OUT>: h * w = 128 and a width of 256 among the planes
    planes = ((1, 128), (1, 256), (4, 32), (2, 128), (8, 16), (2, 256))
    for R in (1, 0):
        for i, O in enumerate((0, 1, 2, 3, 5, 7)):
            h, w = planes[(i + 3 * R) % len(planes)]
            add("w3f-R%d-O%d" % (R, O), entry="cells", layer="w3", c_in=1, c_out=64, h=h, w=w, refractory=R,
                want_spikes=1 if O == 0 else i % 2, want_pv=O & 1, want_v=(O >> 1) & 1, presigmoid=O >> 2, B=2 + i % 3,
                Ts=(3 + i % 4,), q8=int(i % 3 == 1))
    # k_lif_seq_c32<R, OUT, NRO>: short sequences, or the fused readout at any length (T >= 8, int8, every OUT)
    for R in (1, 0):
        for O in range(4):
            for NRO in (0, 24, 48):
                presig = int(O == 2 and NRO == 0 and R == 1)           # (kernel OUT 2 from the presigmoid pv buffer)
                T = 3 + (O + R) % 5 if NRO == 0 else (4, 9, 12, 17)[O]
                add("c32-R%d-O%d-N%d" % (R, O, NRO), refractory=R, n_ro=NRO, presigmoid=presig, Ts=(T,), B=1 + (O + NRO // 24) % 3,
                    target=24, want_spikes=1 if O == 0 else (O + R) % 2, q8=int((O + NRO // 24 + R) % 2),
                    **(dict(want_pv=1, want_v=0) if presig else _wants(O)))
    # k_lif_seq_c32d / k_lif_seq_c32rp / k_lif_seq_c32t <R, OUT>
    for kern, Ts_, plane in (("c32d", (8, 10, 12, 14), (16, 16)), ("c32rp", (9, 11, 13, 15), (16, 16)), ("c32t", (3, 4, 5, 6), None)):
        for R in (1, 0):
            for O in range(4):
                presig = int(O == 2 and R == 0)
                h, w = plane or ((8, 32), (16, 32), (8, 64), (8, 32))[O]
                add("%s-R%d-O%d" % (kern, R, O), refractory=R, h=h, w=w, presigmoid=presig, Ts=(Ts_[(O + R) % 4],), B=1 + (O + R) % 2,
                    want_spikes=1 if O == 0 else (O + R + 1) % 2, q8=int((O + R) % 3 == 0),
                    **(dict(want_pv=1, want_v=0) if presig else _wants(O)))
    # k_lif_seq_c1 / k_lif_seq_c1t <R, F> x (cells | iq); c_out drawn from 1..32, the fast epilogue at 32
    rng = np.random.RandomState(seed + 11)
    for kern, planes_ in (("c1", ((16, 16),)), ("c1t", ((8, 32), (16, 32), (8, 64)))):
        for R in (1, 0):
            for F in (0, 1, 2):
                for Q in (0, 1):
                    h, w = planes_[(F + Q) % len(planes_)]
                    if F == 0:
                        kw = dict(c_out=int(rng.randint(1, 33)), want_spikes=int(rng.rand() < .6), want_pv=int(rng.rand() < .7),
                                  want_v=1, presigmoid=int(rng.rand() < .4))
                    else:
                        kw = dict(c_out=32, want_spikes=1, want_pv=1, want_v=0, presigmoid=int(F == 2))
                    add("%s-R%d-F%d-%s" % (kern, R, F, "iq" if Q else "cells"), entry="iq" if Q else "cells", c_in=1, h=h, w=w,
                        refractory=R, Ts=(3 + (F + 2 * Q + R) % 6,), B=1 + (F + Q + R) % 4, t0=3 if Q else 0, q8=int((F + Q) % 2), **kw)
    # the dense forms
    for R in (1, 0):
        add("dense-seq-R%d" % R, entry="dense", in_features=90, out_features=40, refractory=R, tau_tensor=R, B=5, Ts=(4,))
        add("dense-step-R%d" % R, entry="dense", in_features=70, out_features=130, refractory=R, tau_tensor=1 - R, B=6, Ts=(3,))
    return out


def _boundary_cases(seed):
    out = []

    def add(name, note, **kw):
        out.append(_case("seq-edge-%s" % name, "boundaries", seed * 100003 + 1000 + len(out), note=note, **kw))
    # c32 <-> c32d <-> c32rp
    for i, T in enumerate((1, 2, 7, 8, 9, 10, 15, 16, 17, 33)):
        add("c32-T%d" % T, "T %d: %s" % (T, "k_lif_seq_c32" if T < 8 else "k_lif_seq_c32d" if T % 2 == 0 else "k_lif_seq_c32rp"),
            Ts=(T,), B=2 + i % 2, refractory=i % 2, q8=int(i % 3 == 0), state0=int(i % 4 != 1), rate=RATES[i % 3])
    add("c32-T128", "T 128: k_lif_seq_c32d", Ts=(128,), B=1, rate=.02)
    add("c32-T127", "T 127: k_lif_seq_c32rp", Ts=(127,), B=1, refractory=0, q8=1, rate=.02)
    # tile counts of the tiled 7x7 kernels: 1, 2, 3 per row and per column, one 128x128 plane
    for i, (h, w) in enumerate(((8, 32), (8, 64), (8, 96), (16, 32), (24, 32), (16, 64), (24, 96))):
        add("c32t-%dx%d" % (h, w), "%d x %d tiles" % (h // 8, w // 32), h=h, w=w, Ts=(2 + i % 3,), B=1 + i % 2, refractory=i % 2,
            q8=int(i % 3 == 2), rate=RATES[i % 3])
        add("c1t-%dx%d" % (h, w), "%d x %d tiles" % (h // 8, w // 32), entry="cells", c_in=1, c_out=(32, 13, 32, 7)[i % 4], h=h, w=w,
            Ts=(4 + i,), B=2 + i % 3, refractory=(i + 1) % 2, want_v=int(i % 2), q8=int(i % 3 == 1))
    add("c32t-128x128", "16 x 4 tiles", h=128, w=128, Ts=(3,), B=1, rate=.02, want_v=1)
    add("c1t-128x128", "16 x 4 tiles, the fast epilogue", entry="cells", c_in=1, h=128, w=128, Ts=(3,), B=1, want_v=0)
    add("c1t-128x128-iq", "16 x 4 tiles from the IQ window", entry="iq", c_in=1, c_out=9, h=128, w=128, Ts=(2,), B=1, t0=5)
    # w3 tile counts B * h * w / 32 at multiples of 8 and at +-1 around them
    for B in (7, 8, 9, 15, 16, 17):
        add("w3-tiles%d" % B, "%d tiles: %s" % (B, "FULL" if B % 8 == 0 else "ragged"), layer="w3", c_in=64, c_out=64, h=1, w=32, B=B,
            want_spikes=0, Ts=(3,), refractory=B % 2, q8=int(B % 3 == 0))
    for B in (3, 5, 8):
        add("w3-6x16-tiles%d" % (3 * B), "%d tiles on a 3-tile plane" % (3 * B), layer="w3", c_in=64, c_out=64, h=6, w=16, B=B, want_spikes=0,
            Ts=(4,), refractory=(B + 1) % 2, presigmoid=int(B == 5))
    # dense: the K chunks, the on-chip limits, the 32-sample workgroup
    dense = [(63, 127, 31, 1), (64, 128, 32, 0), (65, 129, 33, 1), (1023, 127, 65, 0), (1024, 128, 33, 1), (1025, 128, 32, 0),
             (1024, 129, 31, 0), (64, 127, 65, 1), (1023, 128, 32, 1), (65, 129, 65, 0), (63, 128, 33, 0), (1025, 127, 31, 1)]
    for i, (nin, nout, B, tt) in enumerate(dense):
        fits = nin <= DS_MAXIN and nout <= DS_MAXOUT
        add("dense-%dx%d-B%d" % (nin, nout, B), "k_dense_lif_seq" if fits else "step by step inside the call", entry="dense",
            in_features=nin, out_features=nout, B=B, tau_tensor=tt, refractory=i % 2, Ts=(3 + i % 3,), rate=RATES[i % 3],
            state0=int(i % 3 != 0))
    # pv statistics: 0, 1 and 2 histogram steps in a call, on its first and on its last step
    LH = [("c32", dict(Ts=(5,)), 19, "one step, the call's first"), ("c32-none", dict(Ts=(6,)), 3, "no step"),
          ("c32d", dict(Ts=(20,)), 0, "one step, the call's last"), ("c32rp", dict(Ts=(21,)), 19, "two steps: first and last"),
          ("c32t", dict(h=8, w=64, Ts=(4,)), 16, "one step, the call's last"),
          ("c1", dict(entry="cells", c_in=1, want_v=0, Ts=(21,)), 19, "two steps, the fast epilogue"),
          ("c1-presig", dict(entry="cells", c_in=1, c_out=11, presigmoid=1, want_v=0, Ts=(20,)), 0, "v in the buffer, last step"),
          ("c1t", dict(entry="iq", c_in=1, h=16, w=32, t0=2, Ts=(7,)), 13, "one step, the call's last, IQ window"),
          ("w3", dict(layer="w3", c_in=64, c_out=64, h=2, w=32, Ts=(3,)), 19, "one step, the call's first"),
          ("w3-presig", dict(layer="w3", c_in=64, c_out=64, h=4, w=16, presigmoid=1, want_v=0, Ts=(21,)), 19, "two steps, pooled v"),
          ("w3f", dict(entry="cells", layer="w3", c_in=1, c_out=64, h=1, w=128, Ts=(20,)), 20, "one step, the call's last")]
    for i, (name, kw, it0, note) in enumerate(LH):
        add("lowhigh-%s" % name, "pv statistics: " + note, lowhigh_iter0=it0, B=2, refractory=i % 2, **kw)
    # pv_presigmoid with pv NOT wanted: nothing moves, v_out stays the caller's (every launcher maps the outputs on its own)
    NP = [("c32", dict(Ts=(4,))), ("c32d", dict(Ts=(8,))), ("c32t", dict(h=8, w=64, Ts=(3,))),
          ("c1", dict(entry="cells", c_in=1, c_out=32, Ts=(5,))), ("c1-iq", dict(entry="iq", c_in=1, c_out=12, t0=2, Ts=(4,))),
          ("c1t", dict(entry="cells", c_in=1, c_out=32, h=16, w=32, Ts=(4,))), ("c1t-iq", dict(entry="iq", c_in=1, c_out=6, h=8, w=32, t0=1, Ts=(3,))),
          ("w3", dict(layer="w3", c_in=64, c_out=64, h=2, w=32, Ts=(3,))), ("w3f", dict(entry="cells", layer="w3", c_in=1, c_out=64, h=1, w=128, Ts=(4,)))]
    for i, (name, kw) in enumerate(NP):
        add("presig-nopv-%s" % name, "pv_presigmoid, pv not wanted, v wanted", presigmoid=1, want_pv=0, want_v=1, want_spikes=i % 2, B=2,
            refractory=(i + 1) % 2, **kw)
    return out


def _carry_cases(seed):
    out = []

    def add(name, **kw):
        out.append(_case("seq-carry-%s" % name, "carry", seed * 100003 + 2000 + len(out), **kw))
    for R in (1, 0):
        add("c32-5-10-9-R%d" % R, Ts=(5, 10, 9), B=2, refractory=R, q8=R)
        add("c32-9-10-5-R%d" % R, Ts=(9, 10, 5), B=3, refractory=R, q8=1 - R, state0=0)
        add("c32-ro-6-4-R%d" % R, Ts=(6, 4), B=2, refractory=R, n_ro=24 * (2 - R), target=24, want_v=0, want_pv=R)
        add("c32t-R%d" % R, h=16, w=64, Ts=(3, 4), B=2, refractory=R)
        add("c1-R%d" % R, entry="cells", c_in=1, c_out=32 if R else 19, Ts=(4, 5, 3), B=3, refractory=R, want_v=1 - R)
        add("c1-iq-R%d" % R, entry="iq", c_in=1, c_out=21 if R else 32, Ts=(3, 6), B=4, refractory=R, want_v=R, t0=4)
        add("c1t-R%d" % R, entry="cells", c_in=1, c_out=32 if R else 5, h=16, w=32, Ts=(5, 3, 4), B=2, refractory=R, want_v=R)
        add("c1t-iq-R%d" % R, entry="iq", c_in=1, c_out=32, h=8, w=64, Ts=(4, 4), B=3, refractory=R, want_v=0, presigmoid=R, t0=1)
        add("w3-R%d" % R, layer="w3", c_in=64, c_out=64, h=4, w=16 << R, Ts=(3, 4), B=3, refractory=R, q8=R)
        add("w3f-R%d" % R, entry="cells", layer="w3", c_in=1, c_out=64, h=2, w=128, Ts=(3, 2, 4), B=3, refractory=R)
        add("dense-seq-R%d" % R, entry="dense", in_features=200, out_features=96, Ts=(3, 4), B=7, refractory=R, tau_tensor=R)
        add("dense-step-R%d" % R, entry="dense", in_features=1100, out_features=70, Ts=(2, 3), B=5, refractory=R, tau_tensor=1 - R)
    return out


def _input_cases(seed):
    """the fixed windows: sample i of a case takes window i of the family's list (patterns()), the rest are random"""
    out = []

    def add(name, **kw):
        out.append(_case("seq-in-%s" % name, "inputs", seed * 100003 + 3000 + len(out), pattern="windows", **kw))
    for R in (1, 0):
        add("c32-R%d" % R, Ts=(6,), B=6, refractory=R, q8=R)
        add("c32rp-R%d" % R, Ts=(9,), B=6, refractory=R)
        add("c32t-16x64-R%d" % R, h=16, w=64, Ts=(3,), B=7, refractory=R, q8=1 - R)
        add("c32t-24x96-R%d" % R, h=24, w=96, Ts=(2,), B=7, refractory=R)
        add("w3-4x16-R%d" % R, layer="w3", c_in=64, c_out=64, h=4, w=16, Ts=(4,), B=6, refractory=R)
        add("w3-1x256-R%d" % R, layer="w3", c_in=64, c_out=64, h=1, w=256, Ts=(3,), B=6, refractory=R, q8=R)
        add("c1-R%d" % R, entry="cells", c_in=1, c_out=32 if R else 17, Ts=(8,), B=6, refractory=R, want_v=1)
        add("c1t-16x64-R%d" % R, entry="cells", c_in=1, c_out=32, h=16, w=64, Ts=(8,), B=6, refractory=R, want_v=R)
        add("c1t-iq-16x64-R%d" % R, entry="iq", c_in=1, c_out=23, h=16, w=64, Ts=(6,), B=6, refractory=R, t0=2)
        add("w3f-2x128-R%d" % R, entry="cells", layer="w3", c_in=1, c_out=64, h=2, w=128, Ts=(6,), B=6, refractory=R)
    return out


def _grid_cases(seed):
    """grids beyond what 256 compute units hold resident; sample i of the device batch = sample i % B_checked"""
    out = []

    def add(name, **kw):
        out.append(_case("seq-grid-%s" % name, "grids", seed * 100003 + 4000 + len(out), B_checked=8, **kw))
    add("c32", Ts=(5,), B=700, want_v=0)
    add("c32d", Ts=(8,), B=700, want_v=0, presigmoid=1, refractory=0)
    add("c32rp", Ts=(9,), B=700, want_v=0, q8=1)
    add("c32-ro", Ts=(9,), B=700, want_v=0, want_pv=0, n_ro=48, target=24)
    add("c32t", h=8, w=32, Ts=(3,), B=700, want_v=0, presigmoid=1)
    add("c1", entry="cells", c_in=1, Ts=(4,), B=2000, want_v=0, presigmoid=1)
    add("c1-iq", entry="iq", c_in=1, c_out=15, Ts=(4,), B=2000, want_v=0, presigmoid=1, refractory=0, t0=2)
    add("c1t", entry="cells", c_in=1, h=8, w=32, Ts=(4,), B=2000, want_v=0, presigmoid=1)
    add("w3", layer="w3", c_in=64, c_out=64, h=1, w=256, Ts=(3,), B=700, want_v=0, presigmoid=1)
    add("w3f", entry="cells", layer="w3", c_in=1, c_out=64, h=1, w=128, Ts=(4,), B=3000, want_v=0, presigmoid=1)
    add("dense-seq", entry="dense", in_features=64, out_features=32, Ts=(3,), B=20000, tau_tensor=1)
    add("dense-step", entry="dense", in_features=40, out_features=130, Ts=(2,), B=20000, refractory=0)
    return out


FREE_FAMILIES = ("c32", "c32", "c32t", "c1", "c1t", "w3", "w3", "w3f", "dense", "dense")
N_FREE = 100


def _free_draw(rng, k, seed):
    while True:
        fam = FREE_FAMILIES[rng.randint(len(FREE_FAMILIES))]
        c = dict(refractory=int(rng.rand() < .5), rate=float(RATES[rng.randint(3)]), state0=int(rng.rand() < .6),
                 B=int(rng.randint(1, 71)), want_spikes=int(rng.rand() < .7), want_pv=int(rng.rand() < .75), want_v=int(rng.rand() < .5))
        ncall = (1, 1, 1, 2, 3)[rng.randint(5)]
        tmax = 10 if fam in ("c32", "c32t") else 25          # (12.8e6 multiply-adds per sample and step on the 32 -> 32 layers)
        c["Ts"] = tuple(int(rng.randint(1, tmax)) for _ in range(ncall))
        if fam == "dense":
            nin = int(rng.randint(1, 1300)) if rng.rand() < .7 else int((63, 64, 65, 1023, 1024, 1025)[rng.randint(6)])
            nout = int(rng.randint(1, 200)) if rng.rand() < .7 else int((127, 128, 129)[rng.randint(3)])
            c.update(entry="dense", in_features=nin, out_features=nout, tau_tensor=int(rng.rand() < .5), target=int(rng.randint(1, 41)))
        else:
            c.update(q8=int(rng.rand() < .3), presigmoid=int(rng.rand() < .3))
            if rng.rand() < .35:
                c["lowhigh_iter0"] = int(rng.randint(0, 40))
            if fam in ("c32", "c32t"):
                h, w = (16, 16) if fam == "c32" else (8 * int(rng.randint(1, 4)), 32 * int(rng.randint(1, 3)))
                c.update(h=h, w=w)
                if fam == "c32" and rng.rand() < .3 and not c["presigmoid"]:
                    c.update(n_ro=int((24, 48)[rng.randint(2)]), target=24)
            elif fam in ("c1", "c1t"):
                h, w = (16, 16) if fam == "c1" else (8 * int(rng.randint(1, 4)), 32 * int(rng.randint(1, 3)))
                c.update(entry="iq" if rng.rand() < .4 else "cells", c_in=1, h=h, w=w,
                         c_out=32 if rng.rand() < .4 else int(rng.randint(1, 33)))
                if c["entry"] == "iq":
                    c["t0"] = int(rng.randint(1, 9))
            elif fam == "w3":
                w = 1 << int(rng.randint(1, 9))
                hw = 32 * int(rng.randint(1, 9))
                hw = -(-hw // w) * w
                if hw % 32:
                    continue
                c.update(layer="w3", c_in=64, c_out=64, h=hw // w, w=w)
                if hw % 64:
                    c["want_spikes"] = 0
            else:
                w = 1 << int(rng.randint(1, 9))
                hw = max(128, w) * int(rng.randint(1, 4))
                c.update(entry="cells", layer="w3", c_in=1, c_out=64, h=hw // w, w=w)
            if "lowhigh_iter0" in c:
                c["want_pv"] = 1
        cc = _case("seq-free-%03d" % k, "free", seed * 100003 + 5000 + k, **c)
        per = work(dict(cc, B_checked=1))
        bmax = int(WORK_FREE_MAX // per)
        if bmax < 1:
            continue
        if cc["B"] > bmax:
            cc["B"] = cc["B_checked"] = int(rng.randint(1, bmax + 1))
        return cc


def cases(seed=SEED):
    """every case that runs (the refusals: refusals())"""
    rng = np.random.RandomState(seed)
    return (_variant_cases(seed) + _boundary_cases(seed) + _carry_cases(seed) + _input_cases(seed) + _grid_cases(seed) +
            [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: (id, entry, descriptor / call changes, code, a phrase of dcll_last_error())"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    k7 = "sequence kernel supports 7x7 pad 3"
    w3 = dict(c_in=64, c_out=64, kh=1, kw=3, pad_h=0, pad_w=1, pool_h=1, pool_w=2)
    rows = [
        ("c32-cout16", "seq", dict(c_out=16), U, k7), ("cells-cout33", "cells", dict(c_in=1, c_out=33), U, k7),
        ("plane-24x24", "seq", dict(h=24, w=24), U, k7), ("plane-12x32", "seq", dict(h=12, w=32), U, k7),
        ("plane-16x48", "cells", dict(c_in=1, h=16, w=48), U, k7), ("k5-pad2", "seq", dict(kh=5, kw=5, pad_h=2, pad_w=2), U, k7),
        ("pool2", "seq", dict(pool_h=2, pool_w=2), U, k7), ("stride2", "seq", dict(stride=2), U, k7),
        ("groups2", "seq", dict(groups=2), U, k7), ("w3-w512", "seq", dict(w3, h=1, w=512), U, k7),
        ("w3-w48", "seq", dict(w3, h=4, w=48), U, k7), ("nro10", "seq", dict(n_ro=10), U, "24 or 48 rows"),
        ("nro24-32x32", "seq", dict(h=32, w=32, n_ro=24), U, "only on the 16x16 plane"),
        ("nro24-w3", "seq", dict(w3, h=4, w=16, n_ro=24), U, "fused readout only for the 7x7 layers"),
        ("w3-spikes-hw96", "seq", dict(w3, h=6, w=16), U, "h * w % 64 == 0"),
        ("w3f-hw64", "cells", dict(w3, c_in=1, h=1, w=64), U, "multiple of 128"),
        ("presig-nro", "seq", dict(n_ro=24, presigmoid=1), I, "pv_presigmoid cannot be combined"),
        ("c32t-no-scratch", "seq", dict(h=8, w=32, no_scratch=1), I, "need state_scratch"),
        ("c1t-no-scratch", "cells", dict(c_in=1, h=8, w=32, no_scratch=1), I, "need state_scratch"),
        ("no-arp", "seq", dict(no_arp=1), I, "refractory layer needs arp"),
        ("cells-no-arp", "cells", dict(c_in=1, no_arp=1), I, "refractory layer needs arp"),
        ("w3f-misaligned", "cells", dict(w3, c_in=1, h=1, w=128, off4=1), I, "8-byte aligned"),
        ("q8-no-scale", "seq", dict(q8_no_scale=1), I, "w_q8 + w_scale"),
        ("T0", "seq", dict(T=0), "DCLL_OK", ""), ("B0", "cells", dict(c_in=1, B=0), "DCLL_OK", ""),
        ("w3-T0", "seq", dict(w3, h=2, w=32, T=0), "DCLL_OK", ""),
    ]
    base = dict(c_in=32, c_out=32, h=16, w=16, kh=7, kw=7, pad_h=3, pad_w=3, pool_h=1, pool_w=1, stride=1, dilation=1, groups=1,
                n_ro=0, presigmoid=0, no_scratch=0, no_arp=0, off4=0, q8_no_scale=0, T=3, B=2)
    return [dict(base, id="seq-refuse-%s" % n, entry=e, code=code, phrase=ph, **kw) for n, e, kw, code, ph in rows]


def by_id(cid):
    for c in cases() + refusals():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def describe(c):
    return json.dumps(c, sort_keys=True)


def cases_hash(cs):
    return hashlib.sha256("\n".join(describe(c) for c in cs).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def patterns(c):
    """the fixed windows of an `inputs` case, in sample order"""
    L = launcher(c)
    if L in ("c32", "c32t"):
        return ["ones", "border_rows", "border_cols", "corners", "zeros"] + (["seams", "seams"] if L == "c32t" else [])
    if L == "w3":
        return ["ones", "col_edges", "pool_even", "pool_odd", "zeros"]
    return ["cell_edges", "cell_edges", "cell_seams", "cell_seams", "cell_first"]


def seam_cells(c):
    """cell 0, h * w - 1 and the cells either side of every seam: 8 x 32 tiles (rows 7 / 8, columns 31 / 32 and the 3-pixel halo
    29..34) of the tiled 7x7 kernels, the 128-pixel segments and the row ends of the (1,3) first layer"""
    h, w = c["h"], c["w"]
    if c["layer"] == "w3":
        flat = {0, h * w - 1} | {q for s in range(128, h * w, 128) for q in (s - 1, s)}
        flat |= {y * w + x for y in range(h) for x in (0, w - 1)}
        return sorted(flat)
    rows = sorted({y for y in range(h) if y % 8 in (7, 0)} | {0, h - 1})
    cols = sorted({x for x in range(w) if x % 32 in (29, 30, 31, 0, 1, 2)} | {0, w - 1})
    return sorted({y * w + x for y in rows for x in cols})


def _window(c, kind, rng, T):
    """(T, c_in, h, w) input spikes of one sample of a packed-spike layer"""
    cin, h, w = c["c_in"], c["h"], c["w"]
    x = (rng.uniform(size=(T, cin, h, w)) < .3).astype(np.float32)
    if kind == "ones":
        x[...] = 1
    elif kind == "zeros":
        x[...] = 0
    elif kind == "border_rows":
        x[:, :, 3:h - 3, :] = 0
    elif kind == "border_cols":
        x[:, :, :, 3:w - 3] = 0
    elif kind == "corners":
        keep = np.zeros((h, w), bool)
        keep[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = True
        x = (rng.uniform(size=(T, cin, h, w)) < .6).astype(np.float32) * keep
        x[0] = keep
    elif kind == "seams":
        keep = np.zeros(h * w, bool)
        rows = [y for y in range(h) if y % 8 in (7, 0)]
        cols = [q for q in range(w) if q % 32 in (29, 30, 31, 0, 1, 2)]
        keep = keep.reshape(h, w)
        keep[rows, :] = True
        keep[:, cols] = True
        x = x * keep
    elif kind == "col_edges":           # the (0,1) padding: first / last column of every row
        keep = np.zeros((h, w), bool)
        keep[:, [0, w - 1]] = True
        x = (rng.uniform(size=(T, cin, h, w)) < .6).astype(np.float32) * keep
    elif kind in ("pool_even", "pool_odd"):     # one half of every pooling pair
        x[:, :, :, (1 if kind == "pool_even" else 0)::2] = 0
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def _cells_window(c, kind, rng, T):
    hw = c["h"] * c["w"]
    if kind == "cell_edges":
        return np.where(rng.rand(T) < .5, 0, hw - 1).astype(np.int32)
    if kind == "cell_first":
        return np.zeros(T, np.int32)
    s = np.asarray(seam_cells(c))
    return s[rng.randint(len(s), size=T)].astype(np.int32)


def iq_tables(c, rng):
    """threshold tables of the IQ quantiser (any ascending fp32 tables are legal): jittered uniform grids, the tail tables one ulp
    above (a value ON a threshold then lands in different cells under the two tables), and a mask that marks some samples"""
    def table(n):
        edges = np.linspace(-1, 1, n + 1)[1:-1]
        return np.sort((edges + rng.uniform(-.2, .2, size=n - 1) / n).astype(np.float32))
    thr_i, thr_q = table(c["w"]), table(c["h"])
    Bc = c["B_checked"]
    mask = (rng.rand(Bc) < .4).astype(np.uint8)
    mask[0] = 1
    if Bc > 1:
        mask[1] = 0
    return dict(thr_i=thr_i, thr_q=thr_q, thr_i_tail=np.nextafter(thr_i, np.float32(2)), thr_q_tail=np.nextafter(thr_q, np.float32(2)),
                mask=mask)


def iq_cells(tab, iq, t0, T, w):
    """dcll_iq_encode in numpy: cell = #{j : x >= thr[j]} per axis, the tail tables for the samples the mask marks -> (T, B)"""
    B = iq.shape[0]
    cells = np.empty((T, B), np.int32)
    for b in range(B):
        ti, tq = (tab["thr_i_tail"], tab["thr_q_tail"]) if tab["mask"][b] else (tab["thr_i"], tab["thr_q"])
        ci = np.searchsorted(ti, iq[b, 0, t0:t0 + T], side="right")
        cq = np.searchsorted(tq, iq[b, 1, t0:t0 + T], side="right")
        cells[:, b] = cq * w + ci
    return cells


def _draw_inputs(c, rng):
    """per call: dict(x (T, Bc, c_in, h, w) or (T, Bc, in), cells (T, Bc) for the first layers); + the IQ window and tables"""
    Bc, Ts = c["B_checked"], c["Ts"]
    extra, calls = {}, []
    if c["entry"] == "dense":
        for k, T in enumerate(Ts):
            x = (rng.uniform(size=(T, Bc, c["in_features"])) < c["rate"]).astype(np.float32)
            if k == 0:
                x[0] = rng.uniform(size=x[0].shape) < .5
            calls.append(dict(x=x))
        return calls, extra
    cin, h, w = c["c_in"], c["h"], c["w"]
    kinds = patterns(c) if c["pattern"] else []
    if c["entry"] == "iq":
        tab = iq_tables(c, rng)
        L = c["t0"] + sum(Ts) + 5
        iq = (rng.randn(Bc, 2, L) * .45).astype(np.float32)
        on = rng.rand(Bc, 2, L) < .15                                     # values exactly on a threshold
        for a, thr in ((0, tab["thr_i"]), (1, tab["thr_q"])):
            pick = thr[rng.randint(len(thr), size=(Bc, L))]
            iq[:, a] = np.where(on[:, a], pick, iq[:, a])
        for b, kind in enumerate(kinds[:Bc]):                             # fixed windows: the values that encode the wanted cells
            cw_ = _cells_window(c, kind, rng, L)
            for a, (thr, idx) in enumerate(((tab["thr_i"], cw_ % w), (tab["thr_q"], cw_ // w))):
                lo = np.concatenate([[np.float32(-1.5)], thr])
                iq[b, a] = lo[idx]                                         # (x == thr[j-1] -> cell j under the main table)
        extra.update(iq=iq, tab=tab)
    t_off = c["t0"]
    for k, T in enumerate(Ts):
        if cin == 1:
            if c["entry"] == "iq":
                cells = iq_cells(extra["tab"], extra["iq"], t_off, T, w)
                t_off += T
            else:
                cells = rng.randint(0, h * w, size=(T, Bc)).astype(np.int32)
                for b, kind in enumerate(kinds[:Bc]):
                    cells[:, b] = _cells_window(c, kind, rng, T)
            x = np.zeros((T, Bc, 1, h * w), np.float32)
            x[np.arange(T)[:, None], np.arange(Bc)[None, :], 0, cells] = 1
            calls.append(dict(x=x.reshape(T, Bc, 1, h, w), cells=cells))
        else:
            x = (rng.uniform(size=(T, Bc, cin, h, w)) < c["rate"]).astype(np.float32)
            if k == 0:
                x[0] = rng.uniform(size=x[0].shape) < .5                  # the first-step burst
            for b, kind in enumerate(kinds[:Bc]):
                x[:, b] = _window(c, kind, rng, T)
            calls.append(dict(x=x))
    return calls, extra


def _sd(c, W, b, tau):
    if c["entry"] == "dense":
        sd = {"i2h.weight": W, "i2h.alpha": tau[0], "i2h.tau_m__dt": tau[1], "i2h.alphas": tau[2], "i2h.tau_s__dt": tau[3],
              "i2o.weight": np.zeros((1, c["out_features"]), np.float32), "i2o.bias": np.zeros(1, np.float32)}
    else:
        _, _, ph, pw = out_shape(c)
        bc = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, None, None], (c["c_in"], c["h"], c["w"])), dtype=np.float32)
        sd = {"i2h.weight": W, "i2h.alpha": bc(tau[0]), "i2h.tau_m__dt": bc(tau[1]), "i2h.alphas": bc(tau[2]),
              "i2h.tau_s__dt": bc(tau[3]), "i2o.weight": np.zeros((1, c["c_out"] * ph * pw), np.float32),
              "i2o.bias": np.zeros(1, np.float32)}           # (the oracle's own readout is not used: one row of zeros)
    if b is not None:
        sd["i2h.bias"] = b
    return sd


def _oracle(c, W, b, tau, wrp):
    from oracle import c_oracle as C
    if c["entry"] == "dense":
        return C.OracleDenseLayer(_sd(c, W, b, tau), wrp, c.get("alpharp", ALPHARP))
    lay = LAYERS[c["layer"]]
    orc = C.OracleConvLayer(_sd(c, W, b, tau), (c["h"], c["w"]), lay["pad"], lay["pool"], wrp, c.get("alpharp", ALPHARP))
    assert (orc.ch, orc.cw, orc.ph, orc.pw) == out_shape(c), c["id"]
    return orc


def _step(c, orc, x):
    """one oracle step -> (v un-pooled, s pooled, pv pooled)"""
    if c["entry"] == "dense":
        s, _, pv, v = orc.forward(x)
        return v, s, pv
    _, _, pv, v, s = orc.forward(x)
    return v, s, pv


def _draw(c, attempt):
    """all tensors of a case from (sub-seed, attempt): time constants per input channel, inputs per call, the initial state,
    zero-mean normal weights rescaled from a provisional plain-neuron oracle run (no bias: v is linear in W) over the case's own
    calls so that std(v) = 2, a bias of scale .5, readout weights"""
    rng = np.random.RandomState((c["seed"] + 7919 * attempt) % (2 ** 31))
    Bc = c["B_checked"]
    dense = c["entry"] == "dense"
    T = {}
    if dense:
        nin, nout = c["in_features"], c["out_features"]
        W0 = rng.randn(nout, nin).astype(np.float32)
        T["tau"] = FZ._time_constants(rng, (nin,) if c["tau_tensor"] else (1,))
        sshape, oshape, K = (Bc, nin), (Bc, nout), nout
    else:
        kh, kw = LAYERS[c["layer"]]["k"]
        ch, cw, ph, pw = out_shape(c)
        W0 = rng.randn(c["c_out"], c["c_in"], kh, kw).astype(np.float32)
        T["tau"] = FZ._time_constants(rng, (c["c_in"],))
        sshape, oshape, K = (Bc, c["c_in"], c["h"], c["w"]), (Bc, c["c_out"], ch, cw), c["c_out"] * ph * pw
        nout = c["c_out"]
    T["calls"], extra = _draw_inputs(c, rng)
    T.update(extra)
    if c["state0"]:
        T["eps0"] = rng.uniform(0, 3, size=sshape).astype(np.float32)
        T["eps1"] = rng.uniform(0, 12, size=sshape).astype(np.float32)
        T["arp"] = (-rng.uniform(0, 2, size=oshape)).astype(np.float32)
    else:
        T["eps0"], T["eps1"], T["arp"] = np.zeros(sshape, np.float32), np.zeros(sshape, np.float32), np.zeros(oshape, np.float32)
    nro = c["target"] if dense else c["n_ro"]
    T["ro_W"] = (rng.uniform(-1, 1, size=(nro, K)) * (.5 / np.sqrt(K))).astype(np.float32) if nro else None
    T["ro_b"] = rng.uniform(-.1, .1, size=(nro,)).astype(np.float32) if nro else None
    # provisional run
    Bp = min(Bc, 2)
    prov = _oracle(c, W0, None, T["tau"], 0.0)
    prov.state = [T["eps0"][:Bp].copy(), T["eps1"][:Bp].copy(), np.zeros((Bp,) + oshape[1:], np.float32)]
    vs = [_step(c, prov, call["x"][t][:Bp])[0] for call in T["calls"] for t in range(call["x"].shape[0])]
    std = float(np.concatenate([v.ravel() for v in vs]).std())
    if std == 0.0:
        std = float(max(np.abs(v).max() for v in vs))
    W = (W0 * np.float32(2.0 / std if std > 0 else 1.0)).astype(np.float32)
    T["b"] = (rng.randn(nout) * .5).astype(np.float32)
    T["q8"] = None
    if c["q8"]:
        q, scale, W = FZ.quantize_int8(W)
        T["q8"] = (q, scale)
    T["W"] = np.ascontiguousarray(W)
    return T


def _trajectory(c, T, before_step=None):
    """the oracle stepping straight through every call -> per call dict(v, s, pv (T, Bc, ...), eps0, eps1, arp after the call);
    before_step(state): run on the oracle's state in front of every step (the mutants of tests/value_cases.py)"""
    orc = _oracle(c, T["W"], T["b"], T["tau"], 1.0 if c["refractory"] else 0.0)
    orc.state = [T["eps0"].copy(), T["eps1"].copy(), T["arp"].copy()]
    out = []

    def one(x):
        if before_step is not None:
            before_step(orc.state)
        return _step(c, orc, x)
    for call in T["calls"]:
        steps = [one(call["x"][t]) for t in range(call["x"].shape[0])]
        out.append(dict(v=np.stack([s[0] for s in steps]), s=np.stack([s[1] for s in steps]), pv=np.stack([s[2] for s in steps]),
                        eps0=orc.state[0].copy(), eps1=orc.state[1].copy(), arp=orc.state[2].copy()))
    return out


def unsound(c, traj):
    """why a trajectory would prove little (None = sound): the un-pooled spike share v > 0 of some step of some call is not
    strictly between .02 and .98, or a refractory layer ends with arp == 0"""
    for k, call in enumerate(traj):
        share = (call["v"] > 0).reshape(call["v"].shape[0], -1).mean(axis=1)
        bad = np.nonzero(~((share > .02) & (share < .98)))[0]
        if len(bad):
            return "call %d step %d: spike share %.4f" % (k, bad[0], share[bad[0]])
    if c["refractory"] and not np.any(traj[-1]["arp"]):
        return "arp is zero"
    return None


def run(c, max_attempts=24):
    """(tensors, oracle trajectory) of a case: the first attempt that is sound (deterministic in the sub-seed)"""
    why = None
    for attempt in range(max_attempts):
        T = _draw(c, attempt)
        traj = _trajectory(c, T)
        why = unsound(c, traj)
        if why is None:
            T["attempt"] = attempt
            return T, traj
    raise AssertionError("%s: no sound draw in %d attempts (%s)" % (c["id"], max_attempts, why))
