"""Cases and float32 restatements for dcll_optim_step / dcll_grad_reduce_optim (k_optim_multi / k_grad_reduce_optim): torch.optim's
Adam, AdamW (both with or without amsgrad), Adamax and SGD as include/dcll_hip.h states them — every operation a separate float32
rounding, the step-dependent scalars computed in float64 on the struct's float32 values and cast once.  No GPU, no library: numpy
only.  tests/test_optim_cases.py proves the restatements against torch in float64; tests/test_gpu_optim.py asks the kernels for their
bits."""
import math

import numpy as np

F = np.float32
ADAM, ADAMW, ADAMAX, SGD = 0, 1, 2, 3
AMSGRAD, NESTEROV, FIRST = 1, 2, 4
MAX_TENSORS, MAX_LAYERS, DYN = 8, 4, 4
KIND_NAMES = {ADAM: "adam", ADAMW: "adamw", ADAMAX: "adamax", SGD: "sgd"}
MUTANTS = {"coupled-adamw": ADAMW, "first-a-g": SGD, "no-nesterov": SGD, "eps-outside-max": ADAMAX, "ams-denominator-v": ADAM}


def f32(x):
    return float(F(x))


def host_values(t, step):
    """the DCLL_OPTIM_DYN scalars of a tensor at `step` as optim_fill computes them (float64 on the float32 struct values, one cast):
    (lr, 1 / bc1, 1 / sqrt(bc2), c) for ADAM / ADAMW (c: ADAMW only), (lr, 1 / bc1, 0, 0) for ADAMAX, (lr, 1 - dampening, 0, 0) for SGD"""
    h0, h1 = f32(t["h0"]), f32(t["h1"])
    row = [f32(t["lr"]), 0.0, 0.0, 0.0]
    if t["kind"] == SGD:
        row[1] = 1.0 - h1
    else:
        row[1] = 1.0 / (1.0 - math.pow(h0, step))
        if t["kind"] in (ADAM, ADAMW):
            row[2] = 1.0 / math.sqrt(1.0 - math.pow(h1, step))
        if t["kind"] == ADAMW:
            row[3] = 1.0 - f32(t["lr"]) * f32(t["weight_decay"])
    return tuple(F(x) for x in row)


def lerp_f32(m, g, w):
    """torch's lerp(m, g, w) for a scalar weight"""
    return m + w * (g - m) if w < F(0.5) else g - (g - m) * (F(1.0) - w)


def optim_f32(t, p, grad, s, step, first=False, mutant=None):
    """optim_update on float32 arrays: t = dict(kind, flags, lr, weight_decay, h0, h1, eps), s = [s0, s1, s2] (None where the kind keeps no
    such state), `first`: DCLL_OPT_FIRST -> (p, [s0, s1, s2]).  mutant: one of MUTANTS, a wrong reading of the update."""
    p, grad = np.asarray(p, F), np.asarray(grad, F)
    s0, s1, s2 = (None if x is None else np.asarray(x, F) for x in s)
    lr, d1, d2, d3 = host_values(t, step)
    wd, h0, h1, eps = F(t["weight_decay"]), F(t["h0"]), F(t["h1"]), F(t["eps"])
    kind, flags = t["kind"], t["flags"]
    if kind in (ADAM, ADAMW):
        if kind == ADAMW and mutant != "coupled-adamw":
            p = p * d3
            g = grad
        else:
            g = grad + wd * p
        m = lerp_f32(s0, g, F(1.0) - h0)
        v = s1 * h1 + ((F(1.0) - h1) * g) * g
        root = v
        if flags & AMSGRAD:
            s2 = np.maximum(s2, v)
            root = v if mutant == "ams-denominator-v" else s2
        denom = np.sqrt(root) * d2 + eps
        p = p - (lr * d1) * (m / denom)
        s0, s1 = m, v
    elif kind == ADAMAX:
        g = grad + wd * p
        m = lerp_f32(s0, g, F(1.0) - h0)
        u = np.maximum(s1 * h1, np.abs(g)) + eps if mutant == "eps-outside-max" else np.maximum(s1 * h1, np.abs(g) + eps)
        p = p - (lr * d1) * (m / u)
        s0, s1 = m, u
    else:
        g = grad + wd * p
        if h0 != 0:
            if first:
                buf = d1 * g if mutant == "first-a-g" else g.copy()
            else:
                buf = s0 * h0 + d1 * g
            g = g + h0 * buf if (flags & NESTEROV and mutant != "no-nesterov") else buf
            s0 = buf
        p = p - lr * g
    out = [s0, s1, s2]
    assert p.dtype == F and all(x is None or x.dtype == F for x in out)
    return p, out


def groups_of(nchunk):
    """partial-row groups of the reduce kernels: 16 / 4 / 1"""
    return 16 if nchunk >= 64 else 4 if nchunk >= 16 else 1


def reduce_f32(part):
    """part (nchunk, c_out, rowlen) float32 -> (dW (c_out, rowlen - 1), db (c_out)) in k_grad_reduce_adam's order: GR groups of
    ceil(nchunk / GR) consecutive chunks, each added in chunk order from 0, the group sums added in group order"""
    part = np.asarray(part, F)
    nchunk = part.shape[0]
    GR = groups_of(nchunk)
    per = (nchunk + GR - 1) // GR
    tot = None
    for grp in range(GR):
        acc = np.zeros(part.shape[1:], F)
        for c in range(grp * per, min(nchunk, (grp + 1) * per)):
            acc = acc + part[c]
        tot = acc if tot is None else tot + acc
    assert tot.dtype == F
    return np.ascontiguousarray(tot[:, :-1]), np.ascontiguousarray(tot[:, -1])


# ----------------------------------------------------------------------------------------------------------------------
# the case list
# ----------------------------------------------------------------------------------------------------------------------
def _hp(kind, flags=0, lr=1e-3, wd=0.0, h0=0.9, h1=0.999, eps=1e-8):
    return dict(kind=kind, flags=flags, lr=lr, weight_decay=wd, h0=h0, h1=h1, eps=eps)


# what the CLI and the layer API reach: train.py's betas (0, beta) and weight_decay 10, torch's defaults, SGD in all its forms
CONFIGS = [
    _hp(ADAM, wd=10.0, h0=0.0, h1=0.95, lr=5e-5), _hp(ADAM, AMSGRAD), _hp(ADAMW, wd=10.0, h0=0.0, h1=0.95, lr=5e-5),
    _hp(ADAMW, AMSGRAD, wd=0.01), _hp(ADAMAX, wd=10.0, h0=0.0, h1=0.95, lr=5e-5), _hp(ADAMAX, lr=2e-3),
    _hp(SGD, lr=5e-5, h0=0.0, h1=0.0), _hp(SGD, lr=1e-2, h0=0.9, h1=0.0), _hp(SGD, lr=1e-2, h0=0.9, h1=0.1, wd=1e-2),
    _hp(SGD, NESTEROV, lr=1e-2, h0=0.9, h1=0.0), _hp(ADAMW, wd=0.0), _hp(SGD, lr=1e-2, h0=0.0, h1=0.0, wd=10.0),
]
SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025]         # k_optim_multi: 256 elements per workgroup; the reduce launch's tail: 1024
GEOMETRIES = [(7, 9), (8, 8), (5, 13)]                  # c_out x rowlen = 63 / 64 / 65: one workgroup, exactly one, two
NCHUNKS = [1, 15, 16, 63, 64, 256]                      # both sides of the 1 -> 4 -> 16 group switches, and the ABI's most


def cases():
    out = []
    for r in range(len(CONFIGS)):           # eight ragged tensors of mixed kinds in one launch: every config meets every size
        out.append(dict(id="step-r%d" % r, call="step", seed=100 + r, step=1 if r % 2 == 0 else (7, 1000)[r % 4 == 1],
                        tensors=[dict(CONFIGS[(r + k) % len(CONFIGS)], n=n) for k, n in enumerate(SIZES)], layers=[]))
    out.append(dict(id="step-one", call="step", seed=99, step=1, tensors=[dict(CONFIGS[7], n=300)], layers=[]))
    for j, nchunk in enumerate(NCHUNKS):
        other = NCHUNKS[(j + 3) % len(NCHUNKS)]
        cfg = lambda k: CONFIGS[(2 * j + k) % len(CONFIGS)]
        (c0, r0), (c1, r1), (c2, r2) = GEOMETRIES
        tensors = [dict(cfg(0), n=c0 * (r0 - 1)), dict(cfg(1), n=c0), dict(cfg(2), n=c1 * (r1 - 1)), dict(cfg(3), n=c2 * (r2 - 1)),
                   dict(cfg(4), n=1025), dict(cfg(5), n=300)]                      # (the last two: no layer refers to them)
        layers = [dict(c_out=c0, rowlen=r0, nchunk=nchunk, db=True, adam_w=0, adam_b=1),
                  dict(c_out=c1, rowlen=r1, nchunk=nchunk, db=False, adam_w=2, adam_b=-1),          # a layer without db
                  dict(c_out=c2, rowlen=r2, nchunk=other, db=True, adam_w=3, adam_b=-1),            # db reduced, not updated
                  dict(c_out=3, rowlen=40, nchunk=nchunk, db=True, adam_w=-1, adam_b=-1)]           # reduce only
        out.append(dict(id="reduce-n%d" % nchunk, call="reduce", seed=200 + j, step=1 if j % 2 == 0 else 12, tensors=tensors,
                        layers=layers))
    out.append(dict(id="reduce-no-tensors", call="reduce", seed=300, step=1, tensors=[],
                    layers=[dict(c_out=8, rowlen=8, nchunk=16, db=True, adam_w=-1, adam_b=-1)]))
    out.append(dict(id="reduce-no-layers", call="reduce", seed=301, step=3, tensors=[dict(CONFIGS[3], n=1025), dict(CONFIGS[9], n=64)],
                    layers=[]))
    assert len({c["id"] for c in out}) == len(out)
    return out


def referred(c):
    """tensor index -> (layer index, 'dW' / 'db') for the tensors a layer's thread updates"""
    out = {}
    for l, L in enumerate(c["layers"]):
        for idx, key in ((L["adam_w"], "dW"), (L["adam_b"], "db")):
            if idx >= 0:
                assert idx not in out
                out[idx] = (l, key)
    return out


NSTEPS = 3


def draw(c):
    """-> dict(tensors=[dict(param, s=[s0, s1, s2], grads=(NSTEPS, n))], parts=[(NSTEPS, nchunk, c_out, rowlen)]).  Start step 1: torch's
    own start (zero state, SGD's buffer created by the first update); later: a running state, the amsgrad maximum above v in about half
    the elements.  Gradients of the tensors a layer refers to are the reduced partial rows (reduce_f32); some gradients are exactly 0."""
    rs = np.random.RandomState(c["seed"])
    fresh = c["step"] == 1
    parts = [(rs.randn(NSTEPS, L["nchunk"], L["c_out"], L["rowlen"]) * 10.0 ** rs.randint(-3, 1)).astype(F) for L in c["layers"]]
    ref = referred(c)
    tensors = []
    for k, t in enumerate(c["tensors"]):
        n = t["n"]
        if k in ref:
            l, key = ref[k]
            grads = np.stack([reduce_f32(parts[l][q])[0 if key == "dW" else 1].reshape(-1) for q in range(NSTEPS)])
        else:
            grads = (rs.randn(NSTEPS, n) * 10.0 ** rs.randint(-3, 1)).astype(F)
            grads[:, ::7] = 0.0
        state = lambda scale, pos=False: np.zeros(n, F) if fresh else ((np.abs(rs.randn(n)) if pos else rs.randn(n)) * scale).astype(F)
        s = [None, None, None]
        if t["kind"] == SGD:
            if t["h0"] != 0:
                s[0] = state(0.01)
        else:
            s[0], s[1] = state(0.01), state(1e-3, True)
            if t["flags"] & AMSGRAD:
                s[2] = (s[1] * rs.choice([0.5, 2.0], size=n)).astype(F)
        tensors.append(dict(param=(rs.randn(n) * 0.05).astype(F), s=s, grads=grads))
    return dict(tensors=tensors, parts=parts)


def first_flag(c, t, q):
    """DCLL_OPT_FIRST of tensor config t at the q-th of the case's steps: the update that creates the momentum buffer"""
    return t["kind"] == SGD and t["h0"] != 0 and c["step"] == 1 and q == 0


def trajectory(c, X=None, mutant=None):
    """the case's NSTEPS updates -> per step, per tensor (p, [s0, s1, s2]) after it"""
    X = draw(c) if X is None else X
    cur = [(T["param"], T["s"]) for T in X["tensors"]]
    out = []
    for q in range(NSTEPS):
        cur = [optim_f32(t, p, T["grads"][q], s, c["step"] + q, first=first_flag(c, t, q),
                         mutant=mutant if mutant and MUTANTS[mutant] == t["kind"] else None)
               for t, T, (p, s) in zip(c["tensors"], X["tensors"], cur)]
        out.append(cur)
    return out


def expected_log(c):
    """the launch log of one call of the case"""
    if c["call"] == "step":
        return ["k_optim_multi"] if sum(t["n"] for t in c["tensors"]) > 0 else []
    return ["k_grad_reduce_optim"] if (c["layers"] or sum(t["n"] for t in c["tensors"]) > 0) else []


# refusals of the C ABI: (id, what to break, a word of the message)
REFUSALS = [("no-s0-adam", "adam without exp_avg", "state"), ("no-s1-adamax", "adamax without exp_inf", "state"),
            ("no-s2-amsgrad", "amsgrad without max_exp_avg_sq", "state"), ("no-s0-momentum", "momentum without buffer", "state"),
            ("kind-4", "kind 4", "unknown kind"), ("kind-neg", "kind -1", "unknown kind"), ("flag-8", "flag bit 8", "flag bits"),
            ("nesterov-adam", "NESTEROV on adam", "flag bits"), ("amsgrad-adamax", "AMSGRAD on adamax", "flag bits"),
            ("first-no-momentum", "FIRST without momentum", "flag bits"), ("step-0", "step 0", "step < 1"),
            ("nine-tensors", "9 tensors", "tensors"), ("five-layers", "5 layers", "layers"), ("twice", "a tensor in two layers", "twice"),
            ("w-size", "weight size", "weight tensor size"), ("b-size", "bias size", "bias tensor size"),
            ("null-param", "param NULL", "null tensor"), ("index", "adam_w out of range", "out of range")]
