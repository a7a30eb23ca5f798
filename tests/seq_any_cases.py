"""Seeded cases for dcll_conv_lif_sequence_any (ABI 8: k_lif_seq_any, the fused all-T kernel of any plain conv layer), their
tensors and the C oracle's trajectories — in the style of tests/seq_fuzz_cases.py.  Plain module: no GPU, no fixtures,
numpy.random.RandomState with fixed seeds only.  tests/test_seq_any_cases.py proves the lists on the CPU;
tests/test_gpu_seq_any.py runs the HIP kernel against them.

A case is a small dict (geometry, options, the lengths `Ts` of consecutive calls on ONE set of state buffers, batch, a sub-seed);
run() draws its tensors from the sub-seed and steps the pinned-order C oracle through all the calls.  Re-run one alone:
    python -c "import seq_any_cases as A; print(A.describe(A.by_id('any-mnist-l1')))"

The launcher's dispatch is restated ONCE here (lds_bytes(), variant()): csrc/dcll_seq_any.hip any_supported /
dcll_conv_lif_sequence_any.

Strata:
  named       the three layers of mnist_conv.yaml; the two layers of radio_ml_conv.yaml (1 -> 32, 32 -> 32) on 16x16, 24x24, 12x32;
  variants    one small case per template variant k_lif_seq_any<R, WLDS, REGS> that the named layers do not reach;
  boundaries  both sides of the LDS limit, of c_out = 32, of the register form's limits (the far sides: refusals());
  grids       a grid beyond residency: mnist layer 2 at B = 1100, the device samples copies of 8 distinct ones;
  free        uniform draws: c_in 1-40, c_out 1-32, kernels 1-9 (asymmetric), pads 0-4, pools 1-3, T 1-9, B 1-5;
  refuse      error returns before any launch (refusals())."""
import hashlib
import json

import numpy as np

import fuzz_cases as FZ

ALPHARP = FZ.ALPHARP
SEED = 20262
RATES = (.05, .15, .3)
WORK_FREE_MAX = 6e7         # multiply-adds of the oracle per free draw, sum over the calls
# the launcher's constants, restated once
LDS_MAX = 160 * 1024
THREADS, NW, KE, QMAX = 512, 8, 36, 3
MAX_K, MAX_COUT = 16, 32

DEFAULT = dict(c_in=1, c_out=16, h=8, w=8, kh=3, kw=3, pad_h=1, pad_w=1, pool_h=1, pool_w=1, stride=1, dilation=1, groups=1,
               refractory=1, tau_tensor=0, bias=1, Ts=(4,), B=2, B_checked=None, rate=.15, state0=1)


def _case(cid, stratum, seed, **kw):
    c = dict(DEFAULT)
    unknown = set(kw) - set(c) - {"note"}
    assert not unknown, unknown
    c.update(kw)
    c["Ts"] = [int(t) for t in c["Ts"]]
    if c["B_checked"] is None:
        c["B_checked"] = c["B"]
    c.update(id=cid, stratum=stratum, seed=int(seed))
    c.setdefault("note", "")
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# geometry and dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
def out_shape(c):
    """(ch, cw, ph, pw): conv plane, pooled plane (MaxPool2d(kernel = stride = pool, padding (pool - 1) // 2), floor mode)"""
    ch = (c["h"] + 2 * c["pad_h"] - c["dilation"] * (c["kh"] - 1) - 1) // c["stride"] + 1
    cw = (c["w"] + 2 * c["pad_w"] - c["dilation"] * (c["kw"] - 1) - 1) // c["stride"] + 1
    ph = (ch + 2 * ((c["pool_h"] - 1) // 2) - c["pool_h"]) // c["pool_h"] + 1
    pw = (cw + 2 * ((c["pool_w"] - 1) // 2) - c["pool_w"]) // c["pool_w"] + 1
    return ch, cw, ph, pw


def valid(c):
    ch, cw, ph, pw = out_shape(c)
    return min(ch, cw, ph, pw) >= 1 and c["c_in"] % c["groups"] == 0 and c["c_out"] % c["groups"] == 0


def _sets(c):
    """(floats of the LDS form, floats of the register form, register form allowed)"""
    ch, cw, _, _ = out_shape(c)
    img = c["c_in"] * (c["h"] + 2 * c["pad_h"]) * (c["w"] + 2 * c["pad_w"])
    nin, nv = c["c_in"] * c["h"] * c["w"], c["c_out"] * ch * cw
    full = img + nin + nv * (2 if c["refractory"] else 1) + 4 * c["c_in"] + 32
    regs = img + 4 * c["c_in"] + 32
    regs_ok = (c["pool_h"], c["pool_w"]) == (1, 1) and nin <= KE * THREADS and ch * cw <= 32 * NW * QMAX and regs * 4 <= LDS_MAX
    return full, regs, regs_ok


def lds_bytes(c):
    """dcll_conv_lif_sequence_any_lds: LDS bytes of the form that serves the layer, 0 = not served"""
    if not valid(c) or (c["stride"], c["dilation"], c["groups"]) != (1, 1, 1) or c["c_out"] > MAX_COUT or max(c["kh"], c["kw"]) > MAX_K:
        return 0
    full, regs, regs_ok = _sets(c)
    if full * 4 <= LDS_MAX:
        return full * 4
    return regs * 4 if regs_ok else 0


def steps(c):
    """MFMA steps of one chain = floats / 64 of the permuted weights"""
    kk = c["kh"] * c["kw"]
    return (c["c_in"] // 2) * kk + ((kk + 1) // 2 if c["c_in"] % 2 else 0)


def variant(c):
    """the template instance a case runs: 'k_lif_seq_any<R,WLDS,REGS>'"""
    full, _, _ = _sets(c)
    regs = full * 4 > LDS_MAX
    wlds = (not regs) and (full + steps(c) * 64) * 4 <= LDS_MAX
    return "k_lif_seq_any<%d,%d,%d>" % (c["refractory"], int(wlds), int(regs))


def all_variants():
    return ["k_lif_seq_any<%d,%d,%d>" % (r, l, g) for r in (0, 1) for l, g in ((1, 0), (0, 0), (0, 1))]


def work(c):
    ch, cw, _, _ = out_shape(c)
    return sum(c["Ts"]) * c["B_checked"] * c["c_out"] * ch * cw * c["c_in"] * c["kh"] * c["kw"]


# ---------------------------------------------------------------------------------------------------------------------------
# the strata
# ---------------------------------------------------------------------------------------------------------------------------
K7P2 = dict(kh=7, kw=7, pad_h=2, pad_w=2)
K7P3 = dict(kh=7, kw=7, pad_h=3, pad_w=3)
MNIST = [dict(K7P2, c_in=1, c_out=16, h=28, w=28, pool_h=2, pool_w=2), dict(K7P2, c_in=16, c_out=24, h=13, w=13),
         dict(K7P2, c_in=24, c_out=32, h=11, w=11, pool_h=2, pool_w=2)]


def _named(seed):
    out = []
    for i, g in enumerate(MNIST):           # BASELINE config 1 runs without a refractory trace (arp 0), tensor time constants
        out.append(_case("any-mnist-l%d" % (i + 1), "named", seed * 100003 + i, refractory=0, tau_tensor=1, Ts=(4,), B=2,
                         rate=RATES[i], **g))
    k = 10
    for h, w in ((16, 16), (24, 24), (12, 32)):
        for c_in in (1, 32):
            out.append(_case("any-radio-%dto32-%dx%d" % (c_in, h, w), "named", seed * 100003 + k, c_in=c_in, c_out=32, h=h, w=w,
                             tau_tensor=1, Ts=(3,), B=2, rate=.1 if c_in == 32 else .02, **K7P3))
            k += 1
    return out


def _variant_cases(seed):
    rows = [("R0-wlds", dict(c_in=3, c_out=9, h=9, w=7, refractory=0)), ("R1-wlds", dict(c_in=4, c_out=32, h=6, w=10, refractory=1)),
            ("R0-stream", dict(K7P3, c_in=32, c_out=32, h=16, w=16, refractory=0, rate=.1)),
            ("R1-stream", dict(K7P3, c_in=32, c_out=32, h=16, w=16, refractory=1, rate=.1)),
            ("R0-regs", dict(K7P3, c_in=32, c_out=32, h=24, w=24, refractory=0, rate=.1, Ts=(2,))),
            ("R1-regs", dict(c_in=31, c_out=17, h=24, w=24, kh=3, kw=5, pad_h=1, pad_w=2, refractory=1, rate=.1, Ts=(3, 2)))]
    return [_case("any-var-%s" % n, "variants", seed * 100003 + 100 + i, **kw) for i, (n, kw) in enumerate(rows)]


# c_in at the LDS limit of a pooling layer (no register form): 16x16, 3x3 pad 1, c_out 32, plain: 584 c_in + 8224 floats
LDS_EDGE = dict(c_out=32, h=16, w=16, pool_h=2, pool_w=2, refractory=0, rate=.1)


def _boundary_cases(seed):
    rows = [("lds-cin56", "40928 floats of 40960: the last c_in that fits", dict(LDS_EDGE, c_in=56, Ts=(2,))),
            ("cout32", "c_out 32: every MFMA row is a channel", dict(c_in=5, c_out=32, h=7, w=9, pool_h=2, pool_w=1)),
            ("cout31", "c_out 31", dict(c_in=6, c_out=31, h=7, w=9, kh=2, kw=4)),
            ("cout1", "one output channel", dict(c_in=7, c_out=1, h=9, w=9, refractory=0)),
            ("regs-nin18432", "register form: 36 eps0 values in every thread", dict(c_in=32, c_out=32, h=24, w=24, kh=1, kw=1, pad_h=0, pad_w=0, Ts=(2,), rate=.1)),
            ("regs-cp768", "register form: 24 pixel tiles, three per wave", dict(c_in=8, c_out=32, h=24, w=32, Ts=(2,))),
            ("regs-cp737", "register form: a ragged last tile", dict(c_in=9, c_out=30, h=11, w=67, Ts=(2,))),
            ("k16", "a 16x16 kernel", dict(c_in=2, c_out=5, h=18, w=17, kh=16, kw=16, pad_h=2, pad_w=3, rate=.3)),
            ("k1x1-plane1x1", "one pixel", dict(c_in=3, c_out=4, h=1, w=1, kh=1, kw=1, pad_h=0, pad_w=0, rate=.3)),
            ("pad-grows", "padding larger than the kernel's half: the conv plane grows", dict(c_in=2, c_out=6, h=5, w=6, pad_h=4, pad_w=3, pool_h=3, pool_w=2, rate=.3)),
            ("pad0-shrinks", "no padding: the conv plane shrinks", dict(c_in=3, c_out=7, h=12, w=9, kh=5, kw=4, pad_h=0, pad_w=0, pool_h=2, pool_w=3, rate=.3)),
            ("hw33", "33 pixels: a second word with one bit", dict(c_in=2, c_out=8, h=3, w=11)),
            ("pool3", "pooling 3 with its padding of 1", dict(c_in=4, c_out=12, h=10, w=11, pool_h=3, pool_w=3))]
    return [_case("any-edge-%s" % n, "boundaries", seed * 100003 + 200 + i, note=note, **kw) for i, (n, note, kw) in enumerate(rows)]


def _grid_cases(seed):
    return [_case("any-grid-mnist-l2", "grids", seed * 100003 + 300, refractory=0, tau_tensor=1, Ts=(6,), B=1100, B_checked=8, **MNIST[1])]


N_FREE = 104


def _free_draw(rng, k, seed):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(1, 33)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 5)), pad_w=int(rng.randint(0, 5)), pool_h=int(rng.randint(1, 4)), pool_w=int(rng.randint(1, 4)),
                 h=int(rng.randint(1, 23)), w=int(rng.randint(1, 23)), refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5),
                 bias=int(rng.rand() < .7), rate=float(RATES[rng.randint(3)]), B=int(rng.randint(1, 6)), state0=1)
        ncall = (1, 1, 2)[rng.randint(3)]
        c["Ts"] = tuple(int(rng.randint(1, 10)) for _ in range(ncall))
        if ncall == 1 and rng.rand() < .3:
            c["state0"] = 0
        cc = _case("any-free-%03d" % k, "free", seed * 100003 + 1000 + k, **c)
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
    return (_named(seed) + _variant_cases(seed) + _boundary_cases(seed) + _grid_cases(seed) +
            [_free_draw(rng, k, seed) for k in range(N_FREE)])


def refusals():
    """error returns before any launch: descriptor / call changes on a small served layer, code, a phrase of dcll_last_error()"""
    U, I = "DCLL_ERR_UNSUPPORTED", "DCLL_ERR_INVALID"
    rows = [("stride2", dict(stride=2), U, "plain convolutions only"), ("dilation2", dict(dilation=2), U, "plain convolutions only"),
            ("groups2", dict(c_in=4, groups=2), U, "plain convolutions only"), ("cout33", dict(c_out=33), U, "c_out <= 32"),
            ("k17", dict(h=20, w=20, kh=17, kw=3), U, "kernels up to 16x16"),
            ("lds-cin57", dict(LDS_EDGE, c_in=57), U, "exceeds the 160 KiB of LDS"),
            ("lds-radio-32x32", dict(K7P3, c_in=32, c_out=32, h=32, w=32), U, "exceeds the 160 KiB of LDS"),
            ("regs-nin19008", dict(c_in=33, c_out=32, h=24, w=24, kh=1, kw=1, pad_h=0, pad_w=0), U, "outside the register form"),
            ("regs-cp792", dict(c_in=8, c_out=32, h=24, w=33), U, "outside the register form"),
            ("regs-pool2", dict(K7P3, c_in=32, c_out=32, h=24, w=24, pool_h=2, pool_w=2), U, "outside the register form"),
            ("null-spk-in", dict(null="spk_in"), I, "null pointer"), ("null-eps1", dict(null="eps1"), I, "null pointer"),
            ("null-W", dict(null="W"), I, "null pointer"), ("null-scratch", dict(null="w_scratch"), I, "null pointer"),
            ("no-arp", dict(null="arp"), I, "refractory layer needs arp"),
            ("T0", dict(T=0), "DCLL_OK", ""), ("B0", dict(B=0), "DCLL_OK", ""), ("T0-unsupported", dict(T=0, stride=2), "DCLL_OK", "")]
    base = dict(DEFAULT, c_in=2, c_out=6, null=None, T=3, B=2)
    del base["Ts"], base["B_checked"], base["rate"], base["state0"]
    return [dict(base, id="any-refuse-%s" % n, code=code, phrase=ph, **kw) for n, kw, code, ph in rows]


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
# the plane packer in numpy
# ---------------------------------------------------------------------------------------------------------------------------
def pack_planes(dense):
    """(..., hw) -> (..., ceil(hw / 32)) uint32: bit pix % 32 of word pix / 32 is pixel pix, tail bits zero"""
    dense = np.asarray(dense)
    hw = dense.shape[-1]
    words = (hw + 31) // 32
    bits = np.zeros(dense.shape[:-1] + (words * 32,), np.uint64)
    bits[..., :hw] = dense != 0
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (bits.reshape(dense.shape[:-1] + (words, 32)) * weights).sum(-1).astype(np.uint32)


def unpack_planes(packed, hw):
    packed = np.asarray(packed).view(np.uint32) if np.asarray(packed).dtype == np.int32 else np.asarray(packed, np.uint32)
    bits = (packed[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(packed.shape[:-1] + (-1,))[..., :hw].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# tensors + the oracle's trajectory
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle(c, W, b, tau, wrp):
    from oracle import c_oracle as C
    ch, cw, ph, pw = out_shape(c)
    if c["tau_tensor"]:
        full = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, None, None], (c["c_in"], c["h"], c["w"])), dtype=np.float32)
    else:
        full = lambda a: np.ascontiguousarray(a[:1], dtype=np.float32)
    sd = {"i2h.weight": W, "i2h.alpha": full(tau[0]), "i2h.tau_m__dt": full(tau[1]), "i2h.alphas": full(tau[2]),
          "i2h.tau_s__dt": full(tau[3]), "i2o.weight": np.zeros((1, c["c_out"] * ph * pw), np.float32),
          "i2o.bias": np.zeros(1, np.float32)}           # (the oracle's own readout is not used: one row of zeros)
    if b is not None:
        sd["i2h.bias"] = b
    orc = C.OracleConvLayer(sd, (c["h"], c["w"]), (c["pad_h"], c["pad_w"]), (c["pool_h"], c["pool_w"]), wrp, c.get("alpharp", ALPHARP))
    assert (orc.ch, orc.cw, orc.ph, orc.pw) == (ch, cw, ph, pw), c["id"]
    return orc


def _draw(c, attempt):
    """all tensors of a case from (sub-seed, attempt): per-channel time constants (a scalar-tau layer: the same four values for
    every channel), inputs per call, the initial state, zero-mean normal weights rescaled from a provisional plain oracle run so
    that std(v) = 2, a bias of scale .5"""
    rng = np.random.RandomState((c["seed"] + 7919 * attempt) % (2 ** 31))
    Bc, cin, h, w = c["B_checked"], c["c_in"], c["h"], c["w"]
    ch, cw, _, _ = out_shape(c)
    T = {}
    W0 = rng.randn(c["c_out"], cin, c["kh"], c["kw"]).astype(np.float32)
    tau = FZ._time_constants(rng, (cin,))
    if not c["tau_tensor"]:
        tau = tuple(np.repeat(t[:1], cin) for t in tau)
    T["tau"] = tau
    T["calls"] = []
    for k, n in enumerate(c["Ts"]):
        x = (rng.uniform(size=(n, Bc, cin, h, w)) < c["rate"]).astype(np.float32)
        if k == 0:
            x[0] = rng.uniform(size=x[0].shape) < .5                  # the first-step burst
        T["calls"].append(dict(x=x))
    sshape, oshape = (Bc, cin, h, w), (Bc, c["c_out"], ch, cw)
    if c["state0"]:
        T["eps0"] = rng.uniform(0, 3, size=sshape).astype(np.float32)
        T["eps1"] = rng.uniform(0, 12, size=sshape).astype(np.float32)
        T["arp"] = (-rng.uniform(0, 2, size=oshape)).astype(np.float32)
    else:
        T["eps0"], T["eps1"], T["arp"] = np.zeros(sshape, np.float32), np.zeros(sshape, np.float32), np.zeros(oshape, np.float32)
    Bp = min(Bc, 2)
    prov = _oracle(c, W0, None, tau, 0.0)
    prov.state = [T["eps0"][:Bp].copy(), T["eps1"][:Bp].copy(), np.zeros((Bp,) + oshape[1:], np.float32)]
    vs = [prov.forward(call["x"][t][:Bp])[3] for call in T["calls"] for t in range(call["x"].shape[0])]
    std = float(np.concatenate([v.ravel() for v in vs]).std())
    if std == 0.0:
        std = float(max(np.abs(v).max() for v in vs))
    T["W"] = np.ascontiguousarray(W0 * np.float32(2.0 / std if std > 0 else 1.0), dtype=np.float32)
    T["b"] = (rng.randn(c["c_out"]) * .5).astype(np.float32) if c["bias"] else None
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
        return orc.forward(x)           # (o, p, pv, v, s)
    for call in T["calls"]:
        st = [one(call["x"][t]) for t in range(call["x"].shape[0])]
        out.append(dict(v=np.stack([s[3] for s in st]), s=np.stack([s[4] for s in st]), pv=np.stack([s[2] for s in st]),
                        eps0=orc.state[0].copy(), eps1=orc.state[1].copy(), arp=orc.state[2].copy()))
    return out


def unsound(c, traj):
    """why a trajectory would prove little (None = sound): the un-pooled spike share of some call is not strictly between .02 and
    .98 (layers of fewer than 50 values per step: not all equal over the case), or a refractory layer ends with arp == 0"""
    small = traj[0]["v"][0].size < 50
    allv = np.concatenate([call["v"].ravel() for call in traj]) > 0
    if small:
        if allv.all() or not allv.any():
            return "every v on one side of the threshold"
    else:
        for k, call in enumerate(traj):
            share = float((call["v"] > 0).mean())
            if not .02 < share < .98:
                return "call %d: spike share %.4f" % (k, share)
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
