"""Seeded cases for dcll_conv_lif_sequence_slabs (k_lif_seq_slab): all T steps of a plain conv layer with MORE than 64 output
channels, B x NY x NX x NS workgroups — a tile of the output plane and a slab of 64 output channels each.  Plain module: no GPU,
numpy.random.RandomState with fixed seeds only; a case has the fields of seq_tile_cases.DEFAULT (`tiles` = the (ty, tx) handed to
the call) and gets its tensors and the oracle's trajectory from seq_any_cases._draw / _trajectory.  tests/test_seq_slab_cases.py
proves the list on the CPU; tests/test_gpu_seq_slab.py runs the HIP kernel against it.

The slab rule (csrc/dcll_any_shared.h), restated: NS = ceil(c_out / 64); slab s owns the output channels
[64 s, min(64 s + 64, c_out)); NS <= 65 535; c_out <= 64 is handed to dcll_conv_lif_sequence_tiles unchanged (seq_tile_cases).
The plan, restated (csrc/dcll_seq_slab.hip): the tile plan is seq_tile_cases.tile_plan; a tile's LDS is seq_tile_cases.tile_floats
with 64 channels in place of c_out; (0, 0) = the fitting (NY, NX) with the fewest tiles, from ONE tile up, ties to the smallest sum
of held input elements, then to the smaller NX; an explicit plan runs as it is, 1 x 1 and N x 1 included.
  strata  named      radio_ml_conv.yaml at netscale 3 / 4 on 16x16: 96 -> 96 and 128 -> 128, B = 1, T = 3
          shape      c_out 65 / 96 / 97 / 128 / 129 / 200, c_in 1 / 3 / 64 / 70, kernels 1x1 .. 9x9, odd planes, planes of 9 / 32 / 33
                     conv pixels, poolings 1 / 2 / 3 / (1,2), refractory and plain
          plan       1 x 1, N x 1, 2 x 2 and the rule; both sides of the LDS limit and of whole-weights-in-LDS; two calls carry state
          grid       B = 300, c_out = 65, 4x4 plane, T = 3
          forwarded  c_out 40 and 64: the tile path's launch log and bits
          free       uniform draws with c_out in 65 .. 200
"""
import json

import numpy as np

import seq_any_cases as A
import seq_tile_cases as X
import seq_wide_cases as W

SEED = 20431
LDS_MAX = 160 * 1024
SLAB_ROWS, SLAB_MAX, MAX_K = 64, 65535, 16
N_FREE = 30
MAX_ATTEMPTS = 24
out_shape, valid, work, cases_hash, steps = A.out_shape, A.valid, A.work, A.cases_hash, A.steps
pack_planes = A.pack_planes


def describe(c):
    return json.dumps(c, sort_keys=True)


def slab_count(c_out):
    return (c_out + SLAB_ROWS - 1) // SLAB_ROWS


def slabs(c_out):
    """[(first channel, channels)] of the slabs of a layer"""
    return [(SLAB_ROWS * s, min(SLAB_ROWS, c_out - SLAB_ROWS * s)) for s in range(slab_count(c_out))]


def c64(c):
    """the case as a workgroup's LDS sees it: a slab's 64 channels"""
    return dict(c, c_out=SLAB_ROWS)


def gmt(c):
    return (c["c_out"] + 31) // 32


def fits(c, ny, nx):
    return X.floats_max(c64(c), ny, nx) * 4 <= LDS_MAX


def rule(c):
    """the (0, 0) rule; None: no plan fits"""
    ph, pw = out_shape(c)[2:]
    for n in range(1, ph * pw + 1):
        best = None
        for nx in range(1, min(pw, n) + 1):
            if n % nx or n // nx > ph or not fits(c, n // nx, nx):
                continue
            held = X.held_sum(c, n // nx, nx)
            if best is None or held < best[0]:
                best = (held, n // nx, nx)
        if best:
            return best[1], best[2]
    return None


def _layer_ok(c):
    return (valid(c) and (c["stride"], c["dilation"], c["groups"]) == (1, 1, 1) and max(c["kh"], c["kw"]) <= MAX_K and
            slab_count(c["c_out"]) <= SLAB_MAX and steps(c) * 64 * gmt(c) < 2 ** 31)


def plan_of(c, B=None, tiles=None):
    """dcll_conv_lif_sequence_slabs_plan: (NY, NX) the call runs, None = refused"""
    if c["c_out"] <= SLAB_ROWS:
        return X.tile_count(c, B, tiles)
    ty, tx = c["tiles"] if tiles is None else tiles
    if not _layer_ok(c) or ty < 0 or tx < 0:
        return None
    ph, pw = out_shape(c)[2:]
    if (ty, tx) == (0, 0):
        return rule(c)
    if ty == 0 or tx == 0 or ty > ph or tx > pw or not fits(c, ty, tx):
        return None
    return ty, tx


def lds_bytes(c, tiles=None):
    if c["c_out"] <= SLAB_ROWS:
        return X.lds_bytes(c, tiles)
    n = plan_of(c, 1, tiles)
    return 0 if n is None else 4 * X.floats_max(c64(c), *n)


def scratch_floats(c, B=None):
    B = c["B"] if B is None else B
    if c["c_out"] <= SLAB_ROWS:
        return X.scratch_floats(c, B)
    if B < 0 or plan_of(c, B, (0, 0)) is None:
        return 0
    return 64 * gmt(c) * steps(c) + 2 * B * c["c_in"] * c["h"] * c["w"]


def whole_weights(c, ny, nx):
    return (X.floats_max(c64(c), ny, nx) + steps(c) * 64 * 2) * 4 <= LDS_MAX


def variant(c):
    """the template instance a case runs: 'k_lif_seq_slab<R,WLDS>'; a forwarded case: the tile path's"""
    if c["c_out"] <= SLAB_ROWS:
        return X.variant(c)
    n = plan_of(c)
    assert n is not None, c["id"]
    return "k_lif_seq_slab<%d,%d>" % (c["refractory"], int(whole_weights(c, *n)))


def launch_log(c):
    return X.launch_log(c) if c["c_out"] <= SLAB_ROWS else [variant(c)]


def all_variants():
    return ["k_lif_seq_slab<%d,%d>" % (r, l) for r in (0, 1) for l in (1, 0)]


def slice_case(c, s):
    """the 64-channel slice s of the layer as a case of its own for dcll_conv_lif_sequence_tiles, with the plan the slab call runs"""
    first, n = slabs(c["c_out"])[s]
    return dict(c, c_out=n, tiles=list(plan_of(c)), id="%s-slab%d" % (c["id"], s))


def _case(cid, stratum, k, tiles=(0, 0), **kw):
    c = X._case("slab-%s" % cid, stratum, SEED * 100003 + k, tiles=tiles, **kw)
    assert plan_of(c) is not None, cid
    return c


K7P3 = A.K7P3


def _named(out):
    R = dict(K7P3, h=16, w=16, tau_tensor=1, Ts=(3,), B=1, rate=.1)
    out.append(_case("radio-ns3-c96", "named", len(out), c_in=96, c_out=96, **R))
    out.append(_case("radio-ns4-c128", "named", len(out), c_in=128, c_out=128, **R))


def _shape(out):
    add = lambda name, **kw: out.append(_case(name, "shape", 100 + len(out), **kw))
    for co in (65, 96, 97, 128, 129, 200):
        add("cout%d" % co, c_in=3, c_out=co, h=9, w=8, B=3, Ts=(3,), refractory=co & 1)
    add("cin1", c_in=1, c_out=65, h=8, w=8, B=3, Ts=(4,))
    add("cin64", c_in=64, c_out=97, h=7, w=7, B=2, Ts=(3,), refractory=0, tau_tensor=1)
    add("cin70", c_in=70, c_out=65, h=6, w=7, B=2, Ts=(3,))
    add("k1x1", c_in=7, c_out=96, kh=1, kw=1, pad_h=0, pad_w=0, h=6, w=7, B=3, Ts=(4,))
    add("k2x5", c_in=3, c_out=129, kh=2, kw=5, pad_h=1, pad_w=2, h=6, w=8, B=3, Ts=(3,), refractory=0)
    add("k7x7", c_in=3, c_out=97, kh=7, kw=7, pad_h=3, pad_w=3, h=8, w=9, B=2, Ts=(3,))
    add("k9x9", c_in=2, c_out=65, kh=9, kw=9, pad_h=4, pad_w=4, h=10, w=10, B=2, Ts=(3,))
    add("cw-odd", c_in=2, c_out=97, h=5, w=7, B=3, Ts=(4,), tiles=(2, 2))
    add("pix9", c_in=3, c_out=65, h=3, w=3, B=4, Ts=(5,), refractory=0)
    add("pix32", c_in=3, c_out=128, h=4, w=8, B=5, Ts=(3,), tiles=(2, 2))
    add("pix33", c_in=3, c_out=129, h=3, w=11, B=5, Ts=(3,), tiles=(1, 3))
    k = 0
    for pool in ((1, 1), (2, 2), (3, 3), (1, 2)):
        for tiles in ((0, 0), (2, 2)):
            add("pool%dx%d-t%dx%d" % (pool + tiles), c_in=3, c_out=(65, 97, 130)[k % 3], h=13, w=11, pool_h=pool[0], pool_w=pool[1], B=3,
                Ts=(3,), refractory=k % 2, tiles=tiles)
            k += 1


# the LDS limit at one tile: 16x16, 3x3, plain: 584 c_in + 16448 floats of 40960 -> 41 channels fit, 42 do not (the rule: two tiles)
LDS_EDGE = dict(c_out=65, h=16, w=16, refractory=0, rate=.1, Ts=(2,), B=1)
# whole weights in LDS behind one tile of a 6x6 plane, 3x3, plain: base 64 c_in + 36 c_in + 2304 + 4 c_in + 64 floats, 128 floats per
# chain step: 56 channels (40448 of 40960 floats) keep all 252 steps on chip, 57 (257 steps: 41192) stream
WLDS_EDGE = dict(c_out=97, h=6, w=6, refractory=0, rate=.1, Ts=(2,), B=2)


def _plan(out):
    add = lambda name, **kw: out.append(_case(name, "plan", 300 + len(out), **kw))
    P = dict(c_in=4, c_out=130, h=12, w=10, B=2)
    for tiles in ((1, 1), (3, 1), (1, 3), (2, 2), (0, 0), (12, 10)):
        add("t%dx%d" % tiles, tiles=tiles, Ts=(2, 3), **P)
        add("t%dx%d-plain-pool" % tiles, tiles=tiles, Ts=(3,), **dict(P, refractory=0, pool_h=2, pool_w=2) if tiles != (12, 10) else
            dict(P, refractory=0, c_out=65))
    add("lds-cin41-1x1", c_in=41, tiles=(1, 1), **LDS_EDGE)
    add("lds-cin42-rule", c_in=42, tiles=(0, 0), **LDS_EDGE)
    add("wlds-cin8", c_in=8, tiles=(1, 1), **WLDS_EDGE)
    for cin in (56, 57):
        add("wlds-cin%d" % cin, c_in=cin, tiles=(1, 1), **WLDS_EDGE)
    add("stream-refr", c_in=64, c_out=65, h=7, w=7, B=2, Ts=(2, 2), tiles=(1, 1), tau_tensor=1)
    add("pw40-shared-words", c_in=2, c_out=65, h=4, w=40, B=2, Ts=(3,), tiles=(2, 3))
    add("grid-B300", c_in=2, c_out=65, h=4, w=4, B=300, B_checked=3, Ts=(3,), tiles=(2, 2))


def _forwarded(out):
    add = lambda name, **kw: out.append(_case(name, "forwarded", 400 + len(out), **kw))
    add("fwd-cout40", c_in=3, c_out=40, h=9, w=8, B=3, Ts=(3,), tiles=(2, 2))
    add("fwd-cout64", c_in=5, c_out=64, h=9, w=11, pool_h=2, pool_w=2, B=2, Ts=(2, 2), tiles=(0, 0))


def _free_draw(rng, k):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(65, 201)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(3, 17)), w=int(rng.randint(3, 17)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(A.RATES[rng.randint(3)]), B=int(rng.randint(1, 4)), state0=1)
        ncall = (1, 1, 2)[rng.randint(3)]
        c["Ts"] = tuple(int(rng.randint(1, 5)) for _ in range(ncall))
        u, v, auto = rng.rand(), rng.rand(), rng.rand() < .3
        cc = X._case("slab-free-%02d" % k, "free", SEED * 100003 + 1000 + k, tiles=(0, 0), **c)
        if not valid(cc):
            continue
        ph, pw = out_shape(cc)[2:]
        if not auto:
            cc["tiles"] = [1 + int(u * min(ph, 4)), 1 + int(v * min(pw, 4))]
        if plan_of(cc) is None:
            continue
        rows, cols = X.tile_plan(cc, *plan_of(cc))
        if not cc["bias"] and any(r["I"][1] - r["I"][0] == 0 for r in rows + cols):
            continue
        if work(dict(cc, B_checked=1, Ts=[1])) * len(cc["Ts"]) > A.WORK_FREE_MAX:
            continue
        while work(cc) > A.WORK_FREE_MAX:
            if max(cc["Ts"]) > 1:
                cc["Ts"] = [max(1, t // 2) for t in cc["Ts"]]
            else:
                cc["B"] = cc["B_checked"] = max(1, cc["B"] // 2)
        return cc


def cases(seed=SEED):
    out = []
    _named(out)
    _shape(out)
    _plan(out)
    _forwarded(out)
    rng = np.random.RandomState(seed)
    return out + [_free_draw(rng, k) for k in range(N_FREE)]


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("stride2", dict(stride=2), U, "plain convolutions only"), ("dilation2", dict(dilation=2), U, "plain convolutions only"),
            ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("ty-above-ph", dict(tiles=[9, 2]), U, "tiles_y > ph or tiles_x > pw"),
            ("tx-above-pw", dict(tiles=[2, 9]), U, "tiles_y > ph or tiles_x > pw"),
            ("lds-cin42-1x1", dict(LDS_EDGE, c_in=42, tiles=[1, 1]), U, "exceeds the 160 KiB of LDS at this plan"),
            ("no-plan-fits", dict(c_in=100, h=16, w=17, kh=16, kw=16, pad_h=0, pad_w=0, tiles=[0, 0]), U, "no tile plan"),
            ("ty-negative", dict(tiles=[-1, 2]), I, "negative tile count"), ("tx-negative", dict(tiles=[2, -1]), I, "negative tile count"),
            ("ty0-alone", dict(tiles=[0, 2]), I, "0 in one direction only"), ("tx0-alone", dict(tiles=[2, 0]), I, "0 in one direction only"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"), ("null-scratch", dict(null="scratch"), I, "null pointer"),
            ("T-negative", dict(T=-1), I, "negative T or B"), ("T0", dict(T=0), "DCLL_OK", "")]
    base = dict(X.DEFAULT, c_out=96, null=None, T=3, B=2)
    for k in ("Ts", "B_checked", "rate", "state0"):
        base.pop(k, None)
    out = []
    for n, kw, code, ph in rows:
        c = dict(base, id="slab-refuse-%s" % n, code=code, phrase=ph, **{k: v for k, v in kw.items() if k not in ("Ts", "rate")})
        out.append(c)
    return out


def by_id(cid):
    for c in cases() + refusals():
        if c["id"] == cid:
            return c
    raise KeyError(cid)


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def unsound(c, traj):
    """seq_wide_cases.unsound (the share of spikes, arp, every 32-row group of channels), and for the slabs: EVERY slab has spikes and
    non-spikes over the case — a kernel that dropped or duplicated a slab cannot pass"""
    why = W.unsound(c, traj)
    if why is not None:
        return why
    for first, n in slabs(c["c_out"]):
        s = np.concatenate([call["v"][:, :, first:first + n].ravel() for call in traj]) > 0
        if s.all() or not s.any():
            return "slab at channel %d: every v on one side of the threshold" % first
    return None


_RUNS = {}


def run(c):
    """(tensors, oracle trajectory) of a case: the first attempt (of at most MAX_ATTEMPTS re-seeded draws) that is sound; computed
    once per process and shared, the callers leave both unchanged"""
    key = json.dumps({k: v for k, v in c.items() if k not in ("id", "tiles", "note", "stratum", "B")}, sort_keys=True)
    if key in _RUNS:
        return _RUNS[key]
    why = None
    for attempt in range(MAX_ATTEMPTS):
        T = A._draw(c, attempt)
        T["attempt"] = attempt
        traj = A._trajectory(c, T)
        why = unsound(c, traj)
        if why is None:
            _RUNS[key] = (T, traj)
            return _RUNS[key]
    raise AssertionError("%s: no sound draw in %d attempts (%s)" % (c["id"], MAX_ATTEMPTS, why))


def slice_tensors(c, T, s):
    """the tensors of slab s's slice of the layer: W, b and arp rows of its channels, everything else shared"""
    first, n = slabs(c["c_out"])[s]
    return dict(T, W=np.ascontiguousarray(T["W"][first:first + n]), b=None if T["b"] is None else np.ascontiguousarray(T["b"][first:first + n]),
                arp=np.ascontiguousarray(T["arp"][:, first:first + n]))


MUTANTS = ("mtile", "bias0", "no-state")


def slabbed_trajectory(c, T, mutant=None):
    """the oracle slab by slab — each slab on ITS slice of W / bias / arp and the whole input state — stitched as the kernel stitches:
    v, spikes, pv and arp by channel, eps0 / eps1 from slab 0.  Mutants: 'mtile' (slabs from the second on take W and bias one M tile
    = 32 channels further down), 'bias0' (every slab's bias is slab 0's), 'no-state' (nobody writes eps0 / eps1 back: the next call
    starts from the old traces — the failure when the write-back is given to a slab that does not exist)"""
    parts = []
    for s, (first, n) in enumerate(slabs(c["c_out"])):
        Ts = slice_tensors(c, T, s)
        if mutant == "mtile" and s > 0:
            Ts["W"] = np.ascontiguousarray(T["W"][first - 32:first - 32 + n])
            if T["b"] is not None:
                Ts["b"] = np.ascontiguousarray(T["b"][first - 32:first - 32 + n])
        if mutant == "bias0" and s > 0 and T["b"] is not None:
            Ts["b"] = np.ascontiguousarray(T["b"][:n])
        cs = dict(c, c_out=n)
        if mutant == "no-state":
            orc_calls, state = [], [Ts["eps0"], Ts["eps1"], Ts["arp"]]
            for call in T["calls"]:         # every call starts from the FIRST call's traces, arp carried
                one = A._trajectory(cs, dict(Ts, calls=[call], eps0=T["eps0"], eps1=T["eps1"], arp=state[2]))[0]
                state[2] = one["arp"]
                orc_calls.append(dict(one, eps0=T["eps0"].copy(), eps1=T["eps1"].copy()))
            parts.append(orc_calls)
        else:
            parts.append(A._trajectory(cs, Ts))
    out = []
    for k in range(len(T["calls"])):
        out.append(dict(v=np.concatenate([p[k]["v"] for p in parts], 2), s=np.concatenate([p[k]["s"] for p in parts], 2),
                        pv=np.concatenate([p[k]["pv"] for p in parts], 2), arp=np.concatenate([p[k]["arp"] for p in parts], 1),
                        eps0=parts[0][k]["eps0"], eps1=parts[0][k]["eps1"]))
    return out
