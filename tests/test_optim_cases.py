"""CPU proofs for tests/optim_cases.py: the float32 restatements of the four updates against torch's own classes in float64, the
mutants they must tell apart, the case list's coverage, and ops.optim_dyn_values against the restated host scalars."""
import numpy as np
import pytest
import torch

import optim_cases as C
import tail_cases as TC

U = 2.0 ** -24
CASES = C.cases()
f = C.f32


def test_kind_adam_without_flags_is_adam_f32_bit_for_bit():
    rs = np.random.RandomState(1)
    n = 3000
    p, g = (rs.randn(n) * 0.05).astype(np.float32), (rs.randn(n) * 0.3).astype(np.float32)
    m, v = (rs.randn(n) * 0.01).astype(np.float32), (np.abs(rs.randn(n)) * 1e-3).astype(np.float32)
    for b1, wd, step in ((0.0, 10.0, 1), (0.9, 0.0, 1000), (0.9, 10.0, 2)):
        hp = dict(lr=1e-3, weight_decay=wd, beta1=b1, beta2=0.999, eps=1e-8)
        t = dict(kind=C.ADAM, flags=0, lr=hp["lr"], weight_decay=wd, h0=b1, h1=hp["beta2"], eps=hp["eps"])
        p1, (m1, v1, none) = C.optim_f32(t, p, g, [m, v, None], step)
        pa, ma, va = TC.adam_f32(p, g, m, v, hp, step)
        assert none is None
        for a, b in ((p1, pa), (m1, ma), (v1, va)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert C.host_values(t, step)[:3] == TC.adam_host_triple(hp["lr"], b1, hp["beta2"], step)


# -- each restatement against its torch class in float64 -------------------------------------------------------------------------
def _t(kind, flags=0, lr=1e-3, wd=0.0, h0=0.9, h1=0.999, eps=1e-8):
    return dict(kind=kind, flags=flags, lr=lr, weight_decay=wd, h0=h0, h1=h1, eps=eps)


# (id, tensor config, step, set state?, mutants this case must catch)
TORCH_CASES = [
    ("sgd-plain", _t(C.SGD, lr=1e-2, h0=0.0, h1=0.0), 1, False, ()),
    ("sgd-wd", _t(C.SGD, lr=1e-2, h0=0.0, h1=0.0, wd=10.0), 1, False, ()),
    ("sgd-momentum-first", _t(C.SGD, lr=1e-2, h0=0.9, h1=0.0), 1, False, ()),
    ("sgd-momentum-later", _t(C.SGD, lr=1e-2, h0=0.9, h1=0.0, wd=10.0), 5, True, ()),
    ("sgd-dampening-first", _t(C.SGD, lr=1e-2, h0=0.9, h1=0.1), 1, False, ("first-a-g",)),
    ("sgd-dampening-later", _t(C.SGD, lr=1e-2, h0=0.9, h1=0.1, wd=0.01), 5, True, ()),
    ("sgd-nesterov-first", _t(C.SGD, C.NESTEROV, lr=1e-2, h0=0.9, h1=0.0), 1, False, ("no-nesterov",)),
    ("sgd-nesterov-later", _t(C.SGD, C.NESTEROV, lr=1e-2, h0=0.9, h1=0.0, wd=10.0), 5, True, ("no-nesterov",)),
    ("adamax-step1", _t(C.ADAMAX, lr=2e-3), 1, False, ()),
    ("adamax-step1-cli", _t(C.ADAMAX, lr=5e-5, wd=10.0, h0=0.0, h1=0.95), 1, False, ()),
    ("adamax-step1000", _t(C.ADAMAX, lr=2e-3, eps=1e-6), 1000, True, ("eps-outside-max",)),
    ("adamw-wd0", _t(C.ADAMW, wd=0.0), 1, False, ()),
    ("adamw-wd10", _t(C.ADAMW, wd=10.0, h0=0.0, h1=0.95), 1, False, ("coupled-adamw",)),
    ("adamw-wd10-later", _t(C.ADAMW, wd=10.0), 1000, True, ("coupled-adamw",)),
    ("adam-amsgrad-step1", _t(C.ADAM, C.AMSGRAD, wd=10.0), 1, False, ()),
    ("adam-amsgrad-below-max", _t(C.ADAM, C.AMSGRAD), 1000, True, ("ams-denominator-v",)),
    ("adamw-amsgrad-below-max", _t(C.ADAMW, C.AMSGRAD, wd=0.01), 7, True, ()),
]
# bounds in u = 2^-24: per state tensor, K of the step, P0 of the parameter the decoupled decay multiplied
BOUNDS = {C.SGD: ([6, 0, 0], 11, 0), C.ADAM: ([6, 7, 7], 18, 0), C.ADAMW: ([6, 7, 7], 18, 2), C.ADAMAX: ([6, 3, 0], 13, 0)}


def _torch_update(t, step, p0, g0, s0):
    """one update of the torch class in float64 (foreach=False), on float32-representable hyper-parameters -> (p, [s0, s1, s2])"""
    prm = torch.nn.Parameter(torch.tensor(p0.astype(np.float64)))
    ams = bool(t["flags"] & C.AMSGRAD)
    if t["kind"] == C.SGD:
        opt = torch.optim.SGD([prm], lr=f(t["lr"]), momentum=f(t["h0"]), dampening=f(t["h1"]), weight_decay=f(t["weight_decay"]),
                              nesterov=bool(t["flags"] & C.NESTEROV), foreach=False)
        names = ["momentum_buffer"] if t["h0"] != 0 else []
    else:
        cls = {C.ADAM: torch.optim.Adam, C.ADAMW: torch.optim.AdamW, C.ADAMAX: torch.optim.Adamax}[t["kind"]]
        kw = dict(amsgrad=ams) if t["kind"] != C.ADAMAX else {}
        opt = cls([prm], lr=f(t["lr"]), betas=(f(t["h0"]), f(t["h1"])), eps=f(t["eps"]), weight_decay=f(t["weight_decay"]), foreach=False, **kw)
        names = ["exp_avg", "exp_inf"] if t["kind"] == C.ADAMAX else ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if ams else [])
    prm.grad = torch.tensor(g0.astype(np.float64))
    if any(x is not None and np.any(x) for x in s0) or step > 1:
        st = {n: torch.tensor(x.astype(np.float64)) for n, x in zip(names, s0)}
        if t["kind"] != C.SGD:
            st["step"] = torch.tensor(float(step - 1))
        opt.state[prm] = st
    opt.step()
    st = opt.state[prm]
    assert t["kind"] == C.SGD or int(st["step"]) == step
    out = [st[n].numpy() for n in names]
    return prm.detach().numpy(), out + [None] * (3 - len(out))


def _draw(t, step, set_state, seed):
    """positive parameters, gradients and state, so that no subtraction but the last cancels (the lerp's g - m: m <= g / 4)"""
    rs = np.random.RandomState(seed)
    n = 4000
    p0 = rs.uniform(0.01, 0.1, n).astype(np.float32)
    g0 = (rs.uniform(0.1, 1.0, n) * 10.0 ** rs.randint(-3, 1, n)).astype(np.float32)
    zero = np.zeros(n, np.float32)
    s = [None, None, None]
    if t["kind"] == C.SGD:
        if t["h0"] != 0:
            s[0] = (g0 * rs.uniform(0.5, 2.0, n)).astype(np.float32) if set_state else zero
    elif t["kind"] == C.ADAMAX:
        s[0] = (g0 * rs.uniform(0.05, 0.25, n)).astype(np.float32) if set_state else zero
        s[1] = (g0 * rs.uniform(0.5, 2.0, n)).astype(np.float32) if set_state else zero      # (u beta2 above |g| + eps in about 2 / 3)
    else:
        s[0] = (g0 * rs.uniform(0.05, 0.25, n)).astype(np.float32) if set_state else zero
        s[1] = (g0 * g0 * rs.uniform(0.5, 2.0, n)).astype(np.float32) if set_state else zero
        if t["flags"] & C.AMSGRAD:
            s[2] = (s[1] * rs.choice([1.0, 4.0], size=n)).astype(np.float32)                 # (half of the maxima stay above the new v)
    return p0, g0, s


def _within(t, p0, got, ref):
    """the restatement's (p, state) within the counted bounds of float64 torch"""
    sb, K, P0 = BOUNDS[t["kind"]]
    (p1, s1), (p64, s64) = got, ref
    ok = True
    for a, b, k in zip(s1, s64, sb):
        assert (a is None) == (b is None)
        if a is not None:
            ok = ok and bool((np.abs(a - b) <= k * U * np.abs(b)).all())
    upd = np.abs(p64 - p0.astype(np.float64))
    ok = ok and bool((np.abs(p1 - p64) <= U * (np.abs(p64) + P0 * np.abs(p0) + K * upd)).all())
    return ok, upd, p64


@pytest.mark.parametrize("case", TORCH_CASES, ids=[c[0] for c in TORCH_CASES])
def test_restatement_vs_its_torch_class_in_float64(case):
    """One update, from torch's own start (step 1) or from a set state, positive operands so that relative errors add.  In units of
    u = 2^-24, counted from optim_update's operation sequence (a cast of a host scalar counts 1 even where the value is exact):
      g = grad + wd p: 2 roundings -> g within 2 u (ADAMW: g = grad, exact)
      lerp: g - m with m <= g / 4 amplifies g's 2 u to 8/3 u, + 1; times w (1 - beta1 is exact) + 1; m + . of positives + 1 -> m within 6 u
      v = v beta2 (1 u) + ((1 - beta2) g) g (2 + 1, then + 2 + 1 = 6 u): the sum of positives + 1 -> v within 7 u; max(vmax, v): 7 u
      Adam's step: sqrt halves 7 u, + 1; isbc2's cast 1, product 1; + eps 1 -> denom within 8 u; m / denom: 6 + 8 + 1 = 15 u;
        lr ibc1: cast 1 + product 1 = 2 u; the step: 15 + 2 + 1 = 18 u;  ADAMW's p c first: c's cast 1 + product 1 = 2 u of |p0|
      Adamax: u = max(u beta2 (1 u), |g| + eps (2 + 1 u)) within 3 u; m / u: 6 + 3 + 1 = 10 u; the step: 10 + 2 + 1 = 13 u
      SGD: buf = buf momentum (2 u) + a g (a's cast 1 + 1 for 1 - dampening, g 2, product 1: 5 u), sum + 1 -> buf within 6 u (first
        update: buf = g, 2 u); nesterov: momentum buf (1 + 6 + 1 = 8 u) + g, + 1 = 9 u; lr g': 1 + 9 + 1 = 11 u
      p' = p - step: |error| <= u (|p'| + K |step|) with K = 18 / 13 / 11 (+ 2 u |p0| for ADAMW)"""
    name, t, step, set_state, mutants = case
    p0, g0, s0 = _draw(t, step, set_state, seed=len(name) + step)
    ref = _torch_update(t, step, p0, g0, s0)
    first = t["kind"] == C.SGD and t["h0"] != 0 and not set_state
    ok, upd, p64 = _within(t, p0, C.optim_f32(t, p0, g0, s0, step, first=first), ref)
    assert ok
    assert (upd > 64 * U * np.abs(p64)).all()                      # (the update is visible in float32: the check is not vacuous)
    if t["flags"] & C.AMSGRAD and set_state:                       # v fell below its maximum somewhere, and rose above it elsewhere
        below = ref[1][1] < s0[2]
        assert below.any() and (~below).any() and np.array_equal(ref[1][2][below], s0[2][below].astype(np.float64))
    for mutant in C.MUTANTS:                                       # a wrong reading of this kind's update is outside the bounds
        if mutant in mutants:
            assert C.MUTANTS[mutant] == t["kind"]
            assert not _within(t, p0, C.optim_f32(t, p0, g0, s0, step, first=first, mutant=mutant), ref)[0], mutant


def test_every_mutant_is_caught_by_a_torch_case_and_by_every_case_of_the_list_that_can_see_it():
    """the case list: where a tensor's configuration makes the mutant a different function (AdamW with decay; a first update with
    dampening; nesterov; Adamax — from a running state, at torch's start max(0, |g| + eps) = max(0, |g|) + eps; amsgrad), its
    trajectory differs from the restatement's in some bit of some tensor"""
    assert {m for c in TORCH_CASES for m in c[4]} == set(C.MUTANTS)

    def sees(c, t, mutant):
        return {"coupled-adamw": t["kind"] == C.ADAMW and t["weight_decay"] != 0,
                "first-a-g": t["kind"] == C.SGD and t["h0"] != 0 and t["h1"] != 0 and c["step"] == 1,
                "no-nesterov": bool(t["kind"] == C.SGD and t["flags"] & C.NESTEROV),
                "eps-outside-max": t["kind"] == C.ADAMAX and c["step"] > 1,
                "ams-denominator-v": bool(t["kind"] in (C.ADAM, C.ADAMW) and t["flags"] & C.AMSGRAD) and c["step"] > 1}[mutant]
    seen = {m: 0 for m in C.MUTANTS}
    for c in CASES:
        X = C.draw(c)
        good = C.trajectory(c, X)
        for mutant in C.MUTANTS:
            ks = [k for k, t in enumerate(c["tensors"]) if t["n"] >= 255 and C.MUTANTS[mutant] == t["kind"] and sees(c, t, mutant)]
            if not ks:
                continue
            bad = C.trajectory(c, X, mutant)
            for k in ks:
                assert any(not np.array_equal(good[q][k][0].view(np.uint32), bad[q][k][0].view(np.uint32)) for q in range(C.NSTEPS)), (c["id"], mutant, k)
                seen[mutant] += 1
    assert all(n >= 2 for n in seen.values()), seen


# -- the case list -------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_the_kernels_branch_on():
    steps = [c for c in CASES if c["call"] == "step"]
    red = [c for c in CASES if c["call"] == "reduce"]
    assert any([t["n"] for t in c["tensors"]] == [0, 1, 255, 256, 257, 1023, 1024, 1025] for c in steps)
    assert all(len(c["tensors"]) <= C.MAX_TENSORS and len(c["layers"]) <= C.MAX_LAYERS for c in CASES)
    assert any(len(c["tensors"]) == 8 and len({t["kind"] for t in c["tensors"]}) == 4 for c in steps)
    # every configuration meets every size; every kind and flag is reached through the reduce launch too
    for k, cfg in enumerate(C.CONFIGS):
        assert {t["n"] for c in steps for t in c["tensors"] if all(t[q] == cfg[q] for q in cfg)} >= set(C.SIZES), k
    ref_kinds = {(c["tensors"][i]["kind"], c["tensors"][i]["flags"]) for c in red for i in C.referred(c)}
    assert ref_kinds >= {(C.ADAM, 0), (C.ADAM, C.AMSGRAD), (C.ADAMW, 0), (C.ADAMAX, 0), (C.SGD, 0), (C.SGD, C.NESTEROV)}, ref_kinds
    layers = [L for c in red for L in c["layers"]]
    assert {L["c_out"] * L["rowlen"] for L in layers} >= {63, 64, 65}
    assert {L["nchunk"] for L in layers} == {1, 15, 16, 63, 64, 256} and {C.groups_of(n) for n in (1, 15)} == {1}
    assert {C.groups_of(n) for n in (16, 63)} == {4} and {C.groups_of(n) for n in (64, 256)} == {16}
    assert any(not L["db"] for L in layers) and any(L["db"] and L["adam_b"] == -1 and L["adam_w"] >= 0 for L in layers)
    assert any(L["adam_w"] == -1 for L in layers)
    assert any(len(C.referred(c)) < len(c["tensors"]) for c in red if c["layers"])          # tensors no layer refers to
    assert any(not c["tensors"] for c in red) and any(not c["layers"] for c in red)
    assert {c["step"] == 1 for c in CASES} == {True, False}
    for c in red:
        for idx, (l, key) in C.referred(c).items():
            L = c["layers"][l]
            assert c["tensors"][idx]["n"] == (L["c_out"] * (L["rowlen"] - 1) if key == "dW" else L["c_out"])
    assert len({r[0] for r in C.REFUSALS}) == len(C.REFUSALS)


def test_draws_are_seeded_and_trajectories_move_every_tensor():
    for c in CASES[::3]:
        a, b = C.draw(c), C.draw(c)
        for Ta, Tb in zip(a["tensors"], b["tensors"]):
            assert np.array_equal(Ta["param"], Tb["param"]) and np.array_equal(Ta["grads"], Tb["grads"])
        traj = C.trajectory(c, a)
        assert len(traj) == C.NSTEPS
        for k, t in enumerate(c["tensors"]):
            ps = [a["tensors"][k]["param"]] + [traj[q][k][0] for q in range(C.NSTEPS)]
            assert all(p.dtype == np.float32 and p.shape == (t["n"],) and np.isfinite(p).all() for p in ps)
            if t["n"] >= 255:
                assert all(not np.array_equal(ps[q], ps[q + 1]) for q in range(C.NSTEPS)), (c["id"], k)
            if t["kind"] == C.SGD and t["h0"] != 0 and c["step"] == 1 and t["n"]:           # the first update: buf = g itself
                g = a["tensors"][k]["grads"][0] + np.float32(t["weight_decay"]) * a["tensors"][k]["param"]
                assert np.array_equal(traj[0][k][1][0].view(np.uint32), g.view(np.uint32))


def test_the_first_update_keeps_the_sign_of_a_zero():
    t = _t(C.SGD, lr=1e-2, h0=0.9, h1=0.0)
    g = np.array([-0.0, 0.0, 1.0], np.float32)
    p, (buf, _, _) = C.optim_f32(t, np.array([-0.0, 0.0, 1.0], np.float32), g, [np.ones(3, np.float32), None, None], 1, first=True)
    assert np.array_equal(buf.view(np.uint32), (g + np.float32(0.0) * np.array([-0.0, 0.0, 1.0], np.float32)).view(np.uint32))
    assert np.signbit(buf[0]) and not np.signbit(buf[1])


def test_reduce_restatement_is_the_sum_in_the_stated_order():
    rs = np.random.RandomState(4)
    for nchunk in C.NCHUNKS:
        part = rs.randn(nchunk, 3, 5).astype(np.float32)
        dW, db = C.reduce_f32(part)
        ref = part.astype(np.float64).sum(axis=0)
        assert np.allclose(np.concatenate([dW, db[:, None]], axis=1), ref, rtol=0, atol=nchunk * U * np.abs(part).sum(axis=0).max())
    assert np.array_equal(C.reduce_f32(np.full((1, 2, 3), 1.5, np.float32))[0], np.full((2, 2), 1.5, np.float32))


def test_optim_dyn_values_are_the_restated_host_scalars():
    from snn_modulation_classification_amd import _lib, ops
    assert (_lib.OPT_ADAM, _lib.OPT_ADAMW, _lib.OPT_ADAMAX, _lib.OPT_SGD) == (C.ADAM, C.ADAMW, C.ADAMAX, C.SGD)
    assert (_lib.OPT_AMSGRAD, _lib.OPT_NESTEROV, _lib.OPT_FIRST) == (C.AMSGRAD, C.NESTEROV, C.FIRST)
    assert (_lib.OPTIM_MAX_TENSORS, _lib.OPTIM_DYN, _lib.REDUCE_MAX_LAYERS) == (C.MAX_TENSORS, C.DYN, C.MAX_LAYERS)
    for step in (1, 2, 7, 1000, 123456):
        ts = [dict(cfg, step=step) for cfg in C.CONFIGS]
        got = [np.float32(x) for x in ops.optim_dyn_values(ts)]
        want = [x for cfg in C.CONFIGS for x in C.host_values(cfg, step)]
        assert len(got) == C.DYN * len(ts) and got == want, step


def test_adam_with_decoupled_weight_decay_is_routed_as_adamw_never_as_plain_adam():
    """torch.optim.Adam(decoupled_weight_decay=True) is AdamW's update: dcll_adam_step (coupled decay) must not take it"""
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    p = [torch.nn.Parameter(torch.ones(3))]
    plain, dec = torch.optim.Adam(p, lr=1e-3, weight_decay=10.0), torch.optim.Adam(p, lr=1e-3, weight_decay=10.0, decoupled_weight_decay=True)
    assert DCLLBase._optimizer_served(plain, False) and DCLLBase._optimizer_served(plain, True)
    assert not DCLLBase._optimizer_served(dec, False) and DCLLBase._optimizer_served(dec, True)
    for cls in (torch.optim.SGD, torch.optim.Adamax, torch.optim.AdamW):
        assert not DCLLBase._optimizer_served(cls(p, lr=1e-3), False) and DCLLBase._optimizer_served(cls(p, lr=1e-3), True)
    for cls in (torch.optim.NAdam, torch.optim.RAdam, torch.optim.RMSprop):
        assert not DCLLBase._optimizer_served(cls(p, lr=1e-3), True)
    assert not DCLLBase._optimizer_served(torch.optim.SGD(p, lr=1e-3, maximize=True), True)
    assert not DCLLBase._optimizer_served(torch.optim.Adam(p, lr=torch.tensor(1e-3)), True)
    assert not DCLLBase._optimizer_served(torch.optim.AdamW(p, lr=1e-3, weight_decay=torch.tensor(0.1)), True)

    class Slice:
        _optimizers = lambda self: [self.o]
    for o, want in ((plain, True), (dec, False), (torch.optim.Adam(p, lr=1e-3, amsgrad=True), False), (torch.optim.AdamW(p, lr=1e-3), False)):
        s = Slice()
        s.o = o
        assert DCLLBase._plain_adam(s) is want


def test_binding_header_and_switches_are_declared():
    import ctypes
    import os
    from conftest import ROOT
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import DCLLBase
    from snn_modulation_classification_amd.networks import ConvNetwork
    header = open(os.path.join(ROOT, "include", "dcll_hip.h")).read()
    for sym in ("dcll_optim_step", "dcll_grad_reduce_optim"):
        assert "int %s(" % sym in header and sym in _lib.SIGNATURES
    assert "#define DCLL_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    assert "#define DCLL_OPTIM_MAX_TENSORS 8" in header and "#define DCLL_OPTIM_DYN 4" in header
    assert ctypes.sizeof(_lib.OptimTensor) == 88 and _lib.OptimTensor.kind.offset == 56 and _lib.OptimTensor.lr.offset == 64
    assert DCLLBase.native_optimizers is False and isinstance(ConvNetwork.native_optim_path, property)
    assert all(callable(getattr(ops, n)) for n in ("optim_step", "grad_reduce_optim", "optim_dyn_values"))
