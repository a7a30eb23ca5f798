"""Seeded cases for dcll_conv_lif_sequence_wide (k_lif_seq_wide: the fused all-T kernel of plain conv layers with 33-64 output
channels; layers of at most 32 are handed to dcll_conv_lif_sequence_any), their tensors and the C oracle's trajectories — in the
style of tests/seq_any_cases.py, whose case format, tensor draws and oracle stepping are used as they are.  Plain module: no GPU,
no fixtures, numpy.random.RandomState with fixed seeds only.  tests/test_seq_wide_cases.py proves the lists on the CPU;
tests/test_gpu_seq_wide.py runs the HIP kernel against them.  Re-run one alone:
    python -c "import seq_wide_cases as W; print(W.describe(W.by_id('wide-radio2-64to64')))"

The launcher's dispatch is restated ONCE here (lds_bytes(), variant(), steps(), nwl()): csrc/dcll_seq_wide.hip wide_supported /
dcll_conv_lif_sequence_wide.

Strata:
  named       radio_ml_conv.yaml at netscale 2 on 16x16 (1 -> 64 LDS form; 64 -> 64 register form, refractory and plain) and at
              netscale 1.5 (1 -> 48, 48 -> 48); mnist_conv.yaml at netscale 2 (32 -> 48 on 13x13, 48 -> 64 on 11x11 with pooling 2);
              the heavy ones at T <= 3, B <= 2;
  variants    one small case per template instance k_lif_seq_wide<R, WLDS, REGS>;
  edges       the smallest shapes at which the second M tile can go wrong;
  boundaries  both sides of the LDS form's limit, of the register form's three limits, of whole-weights-in-LDS (the far sides:
              refusals()), the half-LDS rule above 256 workgroups;
  grid        a grid beyond residency: B = 1100 from 8 distinct samples;
  forwarded   c_out <= 32: k_lif_seq_any's launch log;
  free        uniform draws: c_in 1-40, c_out 33-64, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, T 1-6, B 1-4;
  refuse      error returns before any launch (refusals())."""
import numpy as np

import seq_any_cases as A

ALPHARP = A.ALPHARP
SEED = 20317
WORK_FREE_MAX = A.WORK_FREE_MAX
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
THREADS, NW, KE = 512, 8, 36
MAX_K, MAX_COUT = 16, 64
REGS_CP_MAX = 32 * NW           # MT x (tiles per wave) <= 3: one pixel tile per wave at MT = 2

DEFAULT = dict(A.DEFAULT, c_in=2, c_out=40)
out_shape, valid, work, describe, cases_hash = A.out_shape, A.valid, A.work, A.describe, A.cases_hash
pack_planes, unpack_planes = A.pack_planes, A.unpack_planes


def _case(cid, stratum, seed, **kw):
    return A._case(cid, stratum, seed, **dict(dict(c_in=DEFAULT["c_in"], c_out=DEFAULT["c_out"]), **kw))


# ---------------------------------------------------------------------------------------------------------------------------
# geometry and dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def mt(c):
    return (c["c_out"] + 31) // 32


def _sets(c):
    """MT = 2: (floats of the LDS form, floats of the register form, register form allowed)"""
    ch, cw, _, _ = out_shape(c)
    img = c["c_in"] * (c["h"] + 2 * c["pad_h"]) * (c["w"] + 2 * c["pad_w"])
    nin, nv = c["c_in"] * c["h"] * c["w"], c["c_out"] * ch * cw
    full = img + nin + nv * (2 if c["refractory"] else 1) + 4 * c["c_in"] + 64
    regs = img + 4 * c["c_in"] + 64
    regs_ok = (c["pool_h"], c["pool_w"]) == (1, 1) and nin <= KE * THREADS and ch * cw <= REGS_CP_MAX and regs * 4 <= LDS_MAX
    return full, regs, regs_ok


def lds_bytes(c):
    """dcll_conv_lif_sequence_wide_lds: LDS bytes of the form that serves the layer, 0 = not served"""
    if not valid(c) or (c["stride"], c["dilation"], c["groups"]) != (1, 1, 1) or c["c_out"] > MAX_COUT or max(c["kh"], c["kw"]) > MAX_K:
        return 0
    if mt(c) == 1:
        return A.lds_bytes(c)
    full, regs, regs_ok = _sets(c)
    if full * 4 <= LDS_MAX:
        return full * 4
    return regs * 4 if regs_ok else 0


steps = A.steps


def scratch_floats(c):
    """dcll_conv_lif_sequence_wide_scratch"""
    return 64 * mt(c) * steps(c) if lds_bytes(c) else 0


def form(c):
    """MT = 2: (register form, weights whole in LDS, floats in front of the weights)"""
    full, regs_f, _ = _sets(c)
    regs = full * 4 > LDS_MAX
    base = regs_f if regs else full
    whole = (base + steps(c) * 128) * 4 <= LDS_MAX
    return regs, (not regs) and whole, base


def nwl(c, B):
    """chain steps whose weights the kernel keeps in LDS: all that fit behind the set — within HALF the LDS for a grid of more
    than 256 workgroups whose weights do not fit as a whole"""
    regs, wlds, base = form(c)
    whole = (base + steps(c) * 128) * 4 <= LDS_MAX
    budget = LDS_MAX // 2 if (not whole and B > 256 and base * 8 <= LDS_MAX) else LDS_MAX
    return min(steps(c), (budget // 4 - base) // 128)


def variant(c):
    """the template instance a case runs: 'k_lif_seq_wide<R,WLDS,REGS>', or k_lif_seq_any's for c_out <= 32"""
    if mt(c) == 1:
        return A.variant(c)
    regs, wlds, _ = form(c)
    return "k_lif_seq_wide<%d,%d,%d>" % (c["refractory"], int(wlds), int(regs))


def launch_log(c):
    """the launch log of one call (the wide weight permutation is not logged; k_lif_seq_any's is)"""
    return ["k_seq_any_wprep", variant(c)] if mt(c) == 1 else [variant(c)]


def all_variants():
    return ["k_lif_seq_wide<%d,%d,%d>" % (r, l, g) for r in (0, 1) for l, g in ((1, 0), (0, 0), (0, 1))]


# the kernel's index arithmetic, restated for the CPU proofs of tests/test_seq_wide_cases.py
def chain_offsets(c):
    """B-operand offsets of one chain relative to base0 = y WP + x, as the kernel's recurrence yields them:
    -> (offsets of half 0, offsets of half 1) over the MFMA steps, -1 = the zero link"""
    WP = c["w"] + 2 * c["pad_w"]
    CHS = (c["h"] + 2 * c["pad_h"]) * WP
    kh, kw, KK = c["kh"], c["kw"], c["kh"] * c["kw"]
    npair = (c["c_in"] // 2) * KK
    offs = [[], []]
    off = kx = ky = 0
    for m in range(npair):
        offs[0].append(off)
        offs[1].append(off + CHS)
        off += 1
        kx += 1
        if kx == kw:
            kx = 0
            off += WP - kw
            ky += 1
            if ky == kh:
                ky = 0
                off += 2 * CHS - kh * WP
    if c["c_in"] % 2:
        for hh in (0, 1):
            tap, tkx, tky = hh, hh, 0
            while tkx >= kw:
                tkx -= kw
                tky += 1
            for m in range(npair, steps(c)):
                offs[hh].append((c["c_in"] - 1) * CHS + tky * WP + tkx if tap < KK else -1)
                tap += 2
                tkx += 2
                while tkx >= kw:
                    tkx -= kw
                    tky += 1
    return offs


def chain_links(c):
    """the links (ci, ky, kx) of the pinned order, per half: what chain_offsets must address"""
    KK = c["kh"] * c["kw"]
    links = [[], []]
    for cp in range(c["c_in"] // 2):
        for tap in range(KK):
            for hh in (0, 1):
                links[hh].append((2 * cp + hh, tap // c["kw"], tap % c["kw"]))
    if c["c_in"] % 2:
        for q in range((KK + 1) // 2):
            for hh in (0, 1):
                tap = 2 * q + hh
                links[hh].append((c["c_in"] - 1, tap // c["kw"], tap % c["kw"]) if tap < KK else None)
    return links


def tiles_of_wave(c, wv):
    """pixel tiles wave wv owns (LDS form: wv, wv + 8, ...; register form: its one tile)"""
    ch, cw, _, _ = out_shape(c)
    ntl = (ch * cw + 31) // 32
    if form(c)[0]:
        return [wv] if wv < ntl else []
    return list(range(wv, ntl, NW))


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P2, K7P3 = A.K7P2, A.K7P3
K1 = dict(kh=1, kw=1, pad_h=0, pad_w=0)


def _named(seed):
    rows = [("radio2-1to64", dict(K7P3, c_in=1, c_out=64, h=16, w=16, tau_tensor=1, Ts=(3,), B=2, rate=.02)),
            ("radio2-64to64", dict(K7P3, c_in=64, c_out=64, h=16, w=16, tau_tensor=1, Ts=(3,), B=2, rate=.1)),
            ("radio2-64to64-plain", dict(K7P3, c_in=64, c_out=64, h=16, w=16, tau_tensor=1, refractory=0, Ts=(2,), B=2, rate=.1)),
            ("radio1p5-1to48", dict(K7P3, c_in=1, c_out=48, h=16, w=16, tau_tensor=1, Ts=(3,), B=2, rate=.02)),
            ("radio1p5-48to48", dict(K7P3, c_in=48, c_out=48, h=16, w=16, tau_tensor=1, Ts=(2,), B=2, rate=.1)),
            ("mnist2-32to48", dict(K7P2, c_in=32, c_out=48, h=13, w=13, refractory=0, tau_tensor=1, Ts=(3,), B=2, rate=.15)),
            ("mnist2-48to64", dict(K7P2, c_in=48, c_out=64, h=11, w=11, pool_h=2, pool_w=2, refractory=0, tau_tensor=1, Ts=(3,), B=2,
                                   rate=.3))]
    return [_case("wide-%s" % n, "named", seed * 100003 + i, **kw) for i, (n, kw) in enumerate(rows)]


def _variant_cases(seed):
    rows = [("R0-wlds", dict(c_in=3, c_out=40, h=9, w=7, refractory=0)), ("R1-wlds", dict(c_in=4, c_out=64, h=6, w=10, refractory=1)),
            ("R0-stream", dict(c_in=38, c_out=40, h=4, w=4, kh=9, kw=9, pad_h=4, pad_w=4, refractory=0, rate=.1, Ts=(2,))),
            ("R1-stream", dict(c_in=38, c_out=40, h=4, w=4, kh=9, kw=9, pad_h=4, pad_w=4, refractory=1, rate=.1, Ts=(2,))),
            ("R0-regs", dict(c_in=60, c_out=40, h=16, w=16, refractory=0, rate=.1, Ts=(2,))),
            ("R1-regs", dict(c_in=61, c_out=33, h=15, w=16, kh=3, kw=5, pad_h=1, pad_w=2, refractory=1, rate=.1, Ts=(2, 1)))]
    return [_case("wide-var-%s" % n, "variants", seed * 100003 + 100 + i, **kw) for i, (n, kw) in enumerate(rows)]


def _edge_cases(seed):
    rows = [("cout33", "one real row in tile 1", dict(c_in=4, c_out=33, h=7, w=9)),
            ("cout40", "", dict(c_in=6, c_out=40, h=7, w=9, kh=2, kw=4)),
            ("cout63", "", dict(c_in=2, c_out=63, h=6, w=6)),
            ("cout64", "every MFMA row of both tiles is a channel", dict(c_in=5, c_out=64, h=7, w=9, pool_h=2, pool_w=1)),
            ("cin3", "odd c_in: the last channel pairs its taps", dict(c_in=3, c_out=40, h=6, w=7)),
            ("cin5", "odd c_in, even tap count", dict(c_in=5, c_out=40, h=6, w=7, kh=2, kw=3)),
            ("k1x1", "", dict(K1, c_in=5, c_out=40, h=6, w=7, rate=.3)),
            ("k2x5", "", dict(c_in=4, c_out=40, h=6, w=9, kh=2, kw=5, pad_h=1, pad_w=2)),
            ("plane3x3", "one ragged pixel tile", dict(c_in=4, c_out=40, h=3, w=3, rate=.3)),
            ("cp32", "a conv plane of exactly one tile", dict(c_in=4, c_out=40, h=4, w=8)),
            ("cp33", "a second tile with one pixel", dict(c_in=4, c_out=40, h=3, w=11)),
            ("pool2-7x7", "", dict(c_in=4, c_out=40, h=7, w=7, pool_h=2, pool_w=2)),
            ("pool3-9x5", "pooling 3 with its padding of 1", dict(c_in=4, c_out=40, h=9, w=5, pool_h=3, pool_w=3)),
            ("hw45-out21", "hw no multiple of 32 on either side", dict(c_in=3, c_out=40, h=5, w=9, pad_h=0, pad_w=0, rate=.3)),
            ("nobias", "bias = None", dict(c_in=4, c_out=40, h=6, w=6, bias=0)),
            ("T1", "", dict(c_in=4, c_out=40, h=6, w=6, Ts=(1,))), ("T2", "", dict(c_in=4, c_out=40, h=6, w=6, Ts=(2,))),
            ("carry", "two calls on one set of state buffers", dict(c_in=4, c_out=40, h=6, w=6, Ts=(3, 2))),
            ("B1", "", dict(c_in=4, c_out=40, h=6, w=6, B=1)), ("B3", "", dict(c_in=4, c_out=40, h=6, w=6, B=3))]
    return [_case("wide-edge-%s" % n, "edges", seed * 100003 + 200 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


# c_in at the LDS limit of a pooling layer (no register form): 16x16, 3x3 pad 1, c_out 64, plain: 584 c_in + 16448 floats
LDS_EDGE = dict(c_out=64, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1)
# whole weights in LDS: 6x6, 3x3 pad 1, c_out 40, plain, even c_in: 104 c_in + 1504 floats in front of 576 c_in of weights
WLDS_EDGE = dict(c_out=40, h=6, w=6, refractory=0, rate=.1)
# the register form's LDS: 16x16, 9x9 pad 4, 576 c_in + 4 c_in + 64 floats
REGS_LDS_EDGE = dict(c_out=33, h=16, w=16, kh=9, kw=9, pad_h=4, pad_w=4, rate=.1)


def _boundary_cases(seed):
    rows = [("lds-cin41", "40392 floats of 40960: the last c_in that fits", dict(LDS_EDGE, c_in=41, Ts=(2,), B=1)),
            ("regs-nin18432", "register form: 36 eps0 values in every thread", dict(K1, c_in=72, c_out=40, h=16, w=16, Ts=(2,), rate=.1)),
            ("regs-cp256", "register form: 8 pixel tiles, one per wave", dict(c_in=60, c_out=40, h=16, w=16, Ts=(2,), rate=.1)),
            ("regs-cp255", "register form: a ragged last tile", dict(c_in=60, c_out=40, h=15, w=17, Ts=(2,), rate=.1)),
            ("regs-lds-cin70", "register form: 40664 floats of 40960", dict(REGS_LDS_EDGE, c_in=70, Ts=(1,), B=1)),
            ("wlds-cin58", "40944 floats with all the weights", dict(WLDS_EDGE, c_in=58, Ts=(2,))),
            ("wlds-cin60", "one channel pair more: the weights are streamed", dict(WLDS_EDGE, c_in=60, Ts=(2,))),
            ("b257", "more than 256 workgroups: weights within half the LDS", dict(c_in=38, c_out=40, h=4, w=4, kh=9, kw=9, pad_h=4, pad_w=4,
                                                                                  rate=.1, Ts=(2,), B=257, B_checked=2))]
    return [_case("wide-bound-%s" % n, "boundaries", seed * 100003 + 300 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _grid_cases(seed):
    return [_case("wide-grid-b1100", "grid", seed * 100003 + 400, c_in=4, c_out=40, h=8, w=8, Ts=(3,), B=1100, B_checked=8)]


def _forwarded_cases(seed):
    rows = [("R0-wlds", dict(c_in=3, c_out=9, h=9, w=7, refractory=0)), ("R1-wlds", dict(c_in=4, c_out=32, h=6, w=10)),
            ("R1-stream", dict(K7P3, c_in=32, c_out=32, h=16, w=16, rate=.1, Ts=(2,), B=1)),
            ("R1-regs", dict(c_in=31, c_out=17, h=24, w=24, kh=3, kw=5, pad_h=1, pad_w=2, rate=.1, Ts=(2,), B=1)),
            ("cout1", dict(c_in=7, c_out=1, h=9, w=9, refractory=0)), ("pool", dict(c_in=5, c_out=24, h=7, w=9, pool_h=2, pool_w=3))]
    return [_case("wide-fwd-%s" % n, "forwarded", seed * 100003 + 500 + i, **kw) for i, (n, kw) in enumerate(rows)]


N_FREE = 60


def _free_draw(rng, k, seed):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(33, 65)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(1, 23)), w=int(rng.randint(1, 23)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(A.RATES[rng.randint(3)]), B=int(rng.randint(1, 5)), state0=1)
        ncall = (1, 1, 2)[rng.randint(3)]
        c["Ts"] = tuple(int(rng.randint(1, 7)) for _ in range(ncall))
        if ncall == 1 and rng.rand() < .3:
            c["state0"] = 0
        cc = _case("wide-free-%03d" % k, "free", seed * 100003 + 1000 + k, **c)
        if not valid(cc) or lds_bytes(cc) == 0:
            continue
        per = work(dict(cc, B_checked=1, Ts=[1]))
        if per * len(cc["Ts"]) > WORK_FREE_MAX:
            continue
        while work(cc) > WORK_FREE_MAX:             # shorten the calls, then thin the batch
            if max(cc["Ts"]) > 1:
                cc["Ts"] = [max(1, t // 2) for t in cc["Ts"]]
            else:
                cc["B"] = cc["B_checked"] = max(1, cc["B"] // 2)
        return cc


def cases(seed=SEED):
    """every case that runs (the refusals: refusals())"""
    rng = np.random.RandomState(seed)
    return (_named(seed) + _variant_cases(seed) + _edge_cases(seed) + _boundary_cases(seed) + _grid_cases(seed) +
            _forwarded_cases(seed) + [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("cout65", dict(c_out=65), U, "c_out <= 64"), ("stride2", dict(stride=2), U, "plain convolutions only"),
            ("dilation2", dict(dilation=2), U, "plain convolutions only"), ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("radio2-pool2", dict(K7P3, c_in=64, c_out=64, h=16, w=16, pool_h=2, pool_w=2), U, "outside the register form"),
            ("lds-cin42", dict(LDS_EDGE, c_in=42), U, "exceeds the 160 KiB of LDS"),
            ("regs-nin18688", dict(K1, c_in=73, c_out=40, h=16, w=16), U, "outside the register form"),
            ("regs-cp272", dict(c_in=60, c_out=40, h=16, w=17), U, "outside the register form"),
            ("regs-lds-cin71", dict(REGS_LDS_EDGE, c_in=71), U, "outside the register form"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"),
            ("null-spk-in", dict(null="spk_in"), I, "null pointer"), ("null-eps0", dict(null="eps0"), I, "null pointer"),
            ("null-W", dict(null="W"), I, "null pointer"), ("null-tau4", dict(null="tau4"), I, "null pointer"),
            ("null-scratch", dict(null="w_scratch"), I, "null pointer"),
            ("T-negative", dict(T=-1), I, "negative T or B"), ("B-negative", dict(B=-2), I, "negative T or B"),
            ("T0", dict(T=0), "DCLL_OK", ""), ("B0", dict(B=0), "DCLL_OK", ""), ("T0-unsupported", dict(T=0, c_out=65), "DCLL_OK", "")]
    base = dict(DEFAULT, null=None, T=3, B=2)
    del base["Ts"], base["B_checked"], base["rate"], base["state0"]
    return [dict(base, id="wide-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


def by_id(cid):
    for c in cases() + refusals():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def unsound(c, traj):
    """seq_any_cases.unsound, and for two M tiles: each 32-row group of output channels has spikes AND non-spikes over the case —
    a kernel that dropped or duplicated the second tile cannot pass"""
    why = A.unsound(c, traj)
    if why is not None:
        return why
    for lo in range(0, c["c_out"], 32):
        s = np.concatenate([call["v"][:, :, lo:lo + 32].ravel() for call in traj]) > 0
        if s.all() or not s.any():
            return "channels %d..: every v on one side of the threshold" % lo
    return None


_RUNS = {}


def run(c, max_attempts=24):
    """(tensors, oracle trajectory) of a case: the first attempt that is sound (deterministic in the sub-seed); computed once per
    process and shared — the callers leave both unchanged"""
    if c["id"] in _RUNS:
        return _RUNS[c["id"]]
    why = None
    for attempt in range(max_attempts):
        T = A._draw(c, attempt)
        traj = A._trajectory(c, T)
        why = unsound(c, traj)
        if why is None:
            T["attempt"] = attempt
            _RUNS[c["id"]] = (T, traj)
            return T, traj
    raise AssertionError("%s: no sound draw in %d attempts (%s)" % (c["id"], max_attempts, why))
