"""tests/tail_cases.py proven on the CPU, before any GPU sees it: the list is deterministic and covers every reachable variant key,
the restated dispatch answers what it must at every boundary, every grid / probe draw satisfies its exactness condition, no case
but the three named ones needs more than 64 MB, the float32 restatements agree with their definitions (torch in float64), the vote
reference agrees with the C oracle's, and the rows of a continuous draw whose argmax is left unasserted are at most 2 %."""
import numpy as np
import pytest
import torch

import tail_cases as TC

CASES = TC.cases()
BY_ID = {c["id"]: c for c in CASES}
U = 2.0 ** -24                  # unit roundoff of float32 (half an ulp of 1)


def _ids(cs):
    return [c["id"] for c in cs]


def test_ids_unique_and_list_deterministic():
    assert len(BY_ID) == len(CASES)
    again = TC.cases()
    assert [TC.describe(c) for c in again] == [TC.describe(c) for c in CASES] and _ids(again) == _ids(CASES)
    assert TC.refusals() == TC.refusals() and len({r["id"] for r in TC.refusals()}) == len(TC.refusals())
    strata = {c["stratum"] for c in CASES}
    assert strata == {"variants", "step_tail", "step_multi", "loss", "adam", "reduce_adam", "vote", "free"}
    free = [c for c in CASES if c["stratum"] == "free"]
    assert sum(c["call"] in TC.GEMM_CALLS for c in free) == 60 and sum(c["call"] not in TC.GEMM_CALLS for c in free) == 20


def test_every_reachable_variant_has_a_case():
    reach = TC.reachable_variants()
    assert len(set(reach)) == len(reach) == 16 + 6 + 3 + 4 + 4 + 4 + 2 + 4 + 3 + 4
    served = {}
    for c in CASES:
        for k in TC.variant_keys(c):
            served.setdefault(k, []).append(c["id"])
    missing = [k for k in reach if k not in served]
    assert not missing, missing
    assert set(served) <= set(reach), set(served) - set(reach)
    # and in the variants stratum alone, for the GEMM forms, with every draw kind that applies to the form
    for k in reach:
        if k[0].startswith("k_readout") and k[0] != "k_readout_t16m":
            draws = {BY_ID[i]["draw"] for i in served[k] if BY_ID[i]["stratum"] == "variants"}
            big = all(BY_ID[i].get("big") for i in served[k] if BY_ID[i]["stratum"] == "variants")
            want = {"grid"} if big else {"probe", "cont"} if (k[0] == "k_readout_t16" and k[2]) else {"grid", "probe", "cont"}
            assert draws == want, (k, draws)


def _gemm_form(k):
    return k[0].startswith("k_readout") and k[0] != "k_readout_t16m"


def test_probe_cover_groups_walk_the_whole_column_list():
    """Coverage of the probe columns is asserted, not hoped for: the rows of every cover group visit every column of
    probe_columns(K, kslice) — both sides of EVERY K-slice boundary, the chunk edges, the 8 float4 positions — and every GEMM form
    that has probe draws at all (all but the two 0.54 GB unsplit k_readout_ks forms, which get grid draws only) owns such a group."""
    groups = TC.cover_groups(CASES)
    covered = set()
    for name, (key, cols, seen) in groups.items():
        assert seen == set(cols), (name, key, len(seen), len(cols))
        covered.add(key)
        members = [c for c in CASES if c.get("cover") == name]
        K, ks = members[0]["K"], members[0]["kslice"]
        assert all(c["draw"] == "probe" and c["stratum"] == "variants" for c in members)
        for b in range(ks, K, ks) if ks else ():
            assert b - 1 in seen and b in seen, (name, b)
        assert {k % 32 // 4 for k in seen} == set(range(8)) and {0, 31, 32, 63, (K - 1) // 32 * 32, K - 1} & set(range(K)) <= seen
        assert (key[-1] == "split") == (ks > 0)
    for k in TC.reachable_variants():
        if _gemm_form(k) and k not in (("k_readout_ks", 1, "whole"), ("k_readout_ks", 2, "whole")):
            assert k in covered, k
    # the K = 65280 lists are walked too: 510 slices of 128 and 255 of 256
    assert len(groups["t16-split-k65280-slices128"][1]) == 27 + 2 * 509 - 4 and len(groups["t16-split-k65280-slices256"][1]) == 27 + 2 * 254 - 2


def test_kernels_served_only_above_2048_rows_get_every_tile_edge_in_the_last_workgroup():
    """k_readout_v4 and k_readout (and k_readout_t16 by AUTO) start at 2049 rows = 16 full workgroup tiles + a tail: the tails are the
    rows on both sides of the 32-row wave tile and of the 128-row workgroup tile"""
    for key in (("k_readout_v4", 1), ("k_readout_v4", 2), ("k_readout",)):
        tails = {c["rows"] - 2048 for c in CASES if c["stratum"] == "variants" and c["call"] in TC.GEMM_CALLS and TC.variant_key(c) == key
                 and c["rows"] > 2048 and not (c["off_pv"] or c["off_wt"])}
        assert tails >= {1, 31, 32, 33, 127, 128, 129}, (key, sorted(tails))
        for draw in ("grid", "probe", "cont"):
            assert {c["rows"] - 2048 for c in CASES if c["stratum"] == "variants" and c["call"] in TC.GEMM_CALLS and
                    TC.variant_key(c) == key and c["draw"] == draw} >= {1, 31, 32, 33, 127, 128, 129}, (key, draw)
    auto = {c["rows"] - 2048 for c in CASES if c["stratum"] == "variants" and c["call"] == "readout" and TC.variant_key(c)[0] == "k_readout_t16"}
    assert auto >= {1, 31, 32, 33, 127, 128, 129}


def test_step_strata_carry_every_draw_kind():
    for stratum in ("step_tail", "step_multi"):
        by = {}
        for c in CASES:
            if c["stratum"] == stratum:
                by.setdefault(c["id"].rsplit("-", 1)[0], set()).add(c["draw"])
        assert by and all(d == {"grid", "probe", "cont"} for d in by.values()), stratum


def test_restated_dispatch_at_its_boundaries():
    T = TC
    # column-tile ladders
    assert [T.nt16(n) for n in (1, 16, 17, 32, 33, 48, 49, 64)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [T.nt_direct(n) for n in (1, 16, 17, 32, 33, 48)] == [1, 1, 2, 2, 3, 3]
    assert [T.t16m_item_nt(l, n) for l, n in ((1, 16), (2, 17), (3, 32), (3, 33), (4, 32), (4, 33), (4, 64))] == [1, 2, 2, 3, 2, 4, 4]
    # launch_readout
    lr = T.launch_readout
    assert lr(2048, 64, 24, T.AUTO, True) == ("k_readout_rows",) and lr(2049, 64, 24, T.AUTO, True) == ("k_readout_t16", 2, 0, "whole")
    assert lr(2049, 64, 24, T.AUTO, False) == ("k_readout",) and lr(5, 64, 24, T.AUTO, False) == ("k_readout_rows",)
    assert lr(2049, 33, 24, T.AUTO, True) == ("k_readout",) and lr(2049, 64, 65, T.AUTO, True) == ("k_readout",)
    assert lr(2049, 64, 64, T.LDS, True) == ("k_readout_v4", 2) and lr(2049, 64, 32, T.LDS, True) == ("k_readout_v4", 1)
    assert lr(2048, 64, 32, T.LDS, True) == ("k_readout_rows",)
    assert lr(1, 64, 48, T.CORESIDENT, True) == ("k_readout_direct", 3) and lr(1, 64, 49, T.CORESIDENT, True) == ("k_readout_rows",)
    assert lr(1, 96, 24, T.CORESIDENT, True) == ("k_readout_rows",) and lr(1, 16384, 24, T.CORESIDENT, True) == ("k_readout_direct", 2)
    assert lr(1, 16448, 24, T.CORESIDENT, True) == ("k_readout_rows",) and lr(1, 64, 24, T.CORESIDENT, False) == ("k_readout_rows",)
    assert lr(1, 32, 64, T.T16, True) == ("k_readout_t16", 4, 0, "whole") and lr(1, 33, 64, T.T16, True) == ("k_readout_rows",)
    assert lr(2049, 65536, 32, T.AUTO, True) == ("k_readout_ks", 1, "whole") and lr(2049, 65792, 33, T.LDS, True) == ("k_readout_ks", 2, "whole")
    assert lr(2049, 65280, 32, T.AUTO, True) == ("k_readout_t16", 2, 0, "whole") and lr(32768, 65536, 32, T.AUTO, True)[0] == "k_readout_t16"
    assert lr(2049, 65536 + 32, 32, T.AUTO, True)[0] == "k_readout_t16" and lr(2049, 1 << 22, 32, T.AUTO, True) == ("k_readout",)
    # split-K slices
    sk = T.splitk_slice
    assert (sk(512, 2048, 32), sk(513, 2048, 32), sk(512, 2048, 33), sk(2048, 65280, 1), sk(2049, 2048, 24)) == (128, 256, 256, 256, 0)
    assert (sk(1, 1792, 24), sk(1, 2048 + 128, 24), sk(1, 65280, 24), sk(1, 65536, 24), sk(2048, 65536, 24), sk(2049, 65536, 24)) == \
        (0, 0, 128, 4096, 4096, 8192)
    assert (sk(1, 65536 + 256, 24), sk(1, 2048, 64), sk(1, 2048, 65), sk(0, 2048, 24)) == (0, 256, 0, 0)
    assert T.splitk_scratch(33, 65280, 32) == 510 * 33 * 32 and T.splitk_scratch(33, 65280, 33) == 255 * 33 * 33
    assert T.splitk_scratch(129, 2304, 24) == 18 * 129 * 24 and T.splitk_scratch(513, 2304, 24) == 9 * 513 * 24
    an = T.act_nslice
    assert [an(k) for k in (65504, 65536, 65536 + 32, 65792, 131072, 262144, 524288, 1 << 21)] == [0, 8, 0, 8, 16, 32, 64, 64]
    assert T.act_scratch(33, 65536, 49) == 8 * 33 * 49 and T.act_scratch(33, 2304, 49) == 0
    assert T.step_scratch(5, 2048, 24, 24) == 8 * 5 * 48 and T.step_scratch(5, 2048, 16, 16) == 16 * 5 * 32 and T.step_scratch(5, 2048, 33, 33) == 0 and T.step_scratch(5, 65536, 24, 0) == 0
    assert T.step_scratch(2049, 2048, 24, 0) == 0 and T.step_scratch(513, 2048, 10, 0) == 8 * 513 * 10
    # the learning tail
    assert [T.reduce_groups(n) for n in (1, 15, 16, 63, 64, 65, 129)] == [1, 1, 4, 4, 16, 16, 16]
    assert T.block_prefix([257, 1, 0, 256], 256) == [0, 2, 3, 3, 4] and T.block_prefix([1025, 5, 3], 1024, [False, True, False]) == [0, 2, 2, 3]
    assert T.reduce_adam_grid([dict(c_out=13, rowlen=5, adam_w=1, adam_b=-1)], [300, 52, 13, 1025]) == 2 + 1 + 1 + 2
    assert [T.argmax_path(n, o) for n, o in ((24, 0), (24, 1), (10, 0), (64, 0), (1, 0), (4, 1))] == ["v4", "scalar", "scalar", "v4", "scalar", "scalar"]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_expected_kernels_and_scratch_consistent(case):
    c = case
    ker, scr = TC.expected_kernels(c), TC.expected_scratch(c)
    keys = TC.variant_keys(c)
    assert keys and all(k in TC.reachable_variants() for k in keys)
    if c["call"] in TC.GEMM_CALLS:
        p = TC.gemm_plan(c)
        assert ker[0].split(" ")[0] == p["key"][0] and (len(ker) == 2) == (p["kslice"] > 0) == (p["key"][-1] == "split")
        assert c["kslice"] == p["kslice"]
        if p["kslice"]:
            assert c["K"] % p["kslice"] == 0 and p["kslice"] % 32 == 0
            assert scr["splitk" if c["call"] == "splitk" else "act"] == c["K"] // p["kslice"] * c["rows"] * c["N"]
        if c["call"] == "act":
            assert c["sig"] == bool(p["key"][2])
        if c["off_pv"] or c["off_wt"]:
            assert p["key"][0] in ("k_readout_rows", "k_readout")
    elif c["call"] == "step":
        assert scr["step"] > 0 and scr["step"] == TC.splitk_scratch(c["rows"], c["K"], c["N1"] + c["N2"])
    elif c["call"] == "multi":
        assert all(s > 0 for s in scr["step"]) and 2 <= len(c["items"]) <= TC.STEP_RO_MAX
    elif c["call"] == "adam":
        assert len(c["sizes"]) <= TC.ADAM_MAX_TENSORS
    elif c["call"] == "reduce_adam":
        assert len(c["layers"]) <= TC.REDUCE_MAX_LAYERS and len(c["sizes"]) <= TC.ADAM_MAX_TENSORS
        for L in c["layers"]:
            assert L["adam_w"] < 0 or c["sizes"][L["adam_w"]] == L["c_out"] * (L["rowlen"] - 1)
            assert L["adam_b"] < 0 or c["sizes"][L["adam_b"]] == L["c_out"]
    elif c["call"] == "vote":
        assert 0 <= c["t_begin"] < c["T"] and (c["N"] <= TC.VOTE_MAXN or not c["want_vote"])
    big = c["id"] in TC.BIG
    assert bool(c.get("big")) == big
    assert (TC.device_bytes(c) > TC.MB64) == big, TC.device_bytes(c)


def test_the_three_large_cases_are_the_named_ones():
    assert TC.BIG <= set(BY_ID)
    assert TC.gemm_plan(BY_ID["variants-readout-r2049k65792n24-grid"])["key"] == ("k_readout_ks", 1, "whole")
    assert TC.gemm_plan(BY_ID["variants-readout-r2049k65792n48-grid"])["key"] == ("k_readout_ks", 2, "whole")
    p = TC.gemm_plan(BY_ID["variants-splitk-r2049k65536n24-grid"])
    assert p["key"] == ("k_readout_t16", 2, 0, "split") and p["kslice"] == 65536 // 8
    for i in TC.BIG:
        assert TC.grid_of(BY_ID[i]["K"])[0] * TC.grid_of(BY_ID[i]["K"])[1] * BY_ID[i]["K"] < 2 ** 24      # (the sufficient bound)


EXACT = [c for c in CASES if c.get("draw") in ("grid", "probe") and not c.get("big") and c["call"] in TC.GEMM_CALLS + ("step", "multi")]


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_exact_draws_satisfy_their_exactness_condition(case):
    c = case
    if c["call"] in TC.GEMM_CALLS:
        ds = [(TC.gemm_data(c), c["rows"], c["K"], c["N"])]
    else:
        items = [c] if c["call"] == "step" else c["items"]
        ds = [(TC.step_data(it, c["draw"], c["seed"] + j, c["target"]), it["rows"], it["K"], it["N1"] + it["N2"]) for j, it in enumerate(items)]
    for d, rows, K, N in ds:
        assert d["units"] < 2 ** 24, d["units"]
        assert d["pv"].shape == (rows, K) and d["Wt"].shape == (N, K) and d["ref"].shape == (rows, N)
        assert d["pv"].dtype == d["Wt"].dtype == d["bias"].dtype == np.float32
        # the reference is a float32 number (what "bit for bit" compares), and on the operands' grid
        assert np.array_equal(d["ref"].astype(np.float32).astype(np.float64), d["ref"])
        q = (TC.grid_of(K)[2] / TC.grid_of(K)[0]) if c["draw"] == "grid" else 2.0 ** -11
        assert np.array_equal(np.round(d["ref"] / q) * q, d["ref"])
        if c["draw"] == "grid":
            z = float((d["pv"] == 0).mean())
            assert rows * K < 2000 or 0.25 < z < 0.45, z            # "about a third": 9 / 25 on the fine grid, 3 / 7 on the coarse one
        else:
            assert set(d["kr"].tolist()) <= set(TC.probe_columns(K, c.get("kslice", TC.splitk_slice(rows, K, N))))
            assert (np.abs(d["ref"]) >= 8 * 2.0 ** -11).all() or not c.get("bias", True)


def test_probe_columns_cover_the_edges():
    cols = TC.probe_columns(2304, 256)
    for k in (0, 31, 32, 63, 2272, 2303, 255, 256, 2047, 2048, 127, 128):
        assert k in cols
    assert {k % 32 // 4 for k in cols} == set(range(8)) and {k % 4 for k in cols} == {0, 1, 2, 3}
    assert TC.probe_columns(32) == sorted(set(TC.probe_columns(32)), key=TC.probe_columns(32).index) and max(TC.probe_columns(33)) == 32
    many = TC.probe_columns(65280, 128)
    assert all(b - 1 in many and b in many for b in range(128, 65280, 128))


# -- the float32 restatements against their definitions --------------------------------------------------------------------------


def _ulps(a32, b64):
    """|a - b| in ulps of b's float32 neighbourhood"""
    b32 = np.abs(b64).astype(np.float32)
    ulp = np.maximum(np.spacing(b32).astype(np.float64), 2.0 ** -149)
    return np.abs(a32.astype(np.float64) - b64) / ulp


@pytest.mark.parametrize("kind", [TC.SMOOTH_L1, TC.MSE])
def test_loss_restatement_vs_torch_autograd_float64(kind):
    c = dict(seed=5 + kind, B=333, N=24, has_o=True)
    d = TC.loss_data(c)
    n = c["B"] * c["N"]
    crit = torch.nn.MSELoss() if kind == TC.MSE else torch.nn.SmoothL1Loss()
    for x in (d["p"], d["o"]):
        x64 = torch.tensor(x.astype(np.float64), requires_grad=True)
        t64 = torch.tensor(d["target"].astype(np.float64))
        elem = (torch.nn.MSELoss(reduction="none") if kind == TC.MSE else torch.nn.SmoothL1Loss(reduction="none"))(x64, t64)
        crit(x64, t64).backward()
        l32, _ = TC.loss_elem_f32(x - d["target"], kind)
        g32 = TC.loss_grad_f32(x, d["target"], kind, n)
        assert l32.dtype == g32.dtype == np.float32
        # l: d rounded once (2 u in d^2), the product(s) once more: 3 u = 1.5 ulp; a - 0.5 with a >= 1: u a + u l <= 3 u l.  g / n: d,
        # 1 / n and the product rounded once each: 3 u.  Both within 2 ulp.
        assert _ulps(l32, elem.detach().numpy()).max() <= 2.0
        assert _ulps(g32, x64.grad.numpy()).max() <= 2.0
    # on the kink itself: exact values
    l, g = TC.loss_elem_f32(np.array(TC.KINK, np.float32), TC.SMOOTH_L1)
    assert l[0] == l[1] == 0.5 and g[0] == 1 and g[1] == -1 and g[2] == np.float32(TC.KINK[2]) and g[3] == 1 and g[6] == 0 and l[6] == 0
    ref, bound = TC.loss_value_ref(d, kind)
    both = crit(torch.tensor(d["p"].astype(np.float64)), torch.tensor(d["target"].astype(np.float64))) + \
        crit(torch.tensor(d["o"].astype(np.float64)), torch.tensor(d["target"].astype(np.float64)))
    assert abs(ref - float(both)) <= 1e-12 * abs(ref) and 0 < bound < 1e-3 * abs(ref)


@pytest.mark.parametrize("beta1,wd,step", [(0.0, 0.0, 1), (0.0, 10.0, 2), (0.9, 10.0, 1), (0.9, 0.0, 1000)])
def test_adam_restatement_vs_torch_optim_adam_float64(beta1, wd, step):
    """One update from zero moments (torch's own start; its step counter set to step - 1) with positive parameters and gradients, so
    that no subtraction but the last cancels and relative errors add.  In units of u = 2^-24, counted from adam_update:
      g = grad + wd p: 2 roundings                                                    -> g within 2 u
      m = w g (beta1 != 0: one product; 1 - beta1 is exact, g - 0 and 0 + . are too)  -> m within 3 u;  beta1 = 0: m = g, 2 u
      v = ((1 - beta2) g) g: two products on top of 2 x 2 u                            -> v within 6 u
      denom = sqrt(v) isbc2 + eps: 3 u + sqrt 1 + isbc2's cast 1 + product 1 + sum 1   -> within 7 u
      m / denom: 3 + 7 + 1 = 11 u;  lr ibc1: cast 1 + product 1 = 2 u;  the update: 11 + 2 + 1 = 14 u
      p - update: |error| <= u (|p'| + 14 |update|)"""
    rs = np.random.RandomState(int(beta1 * 10 + wd + step))
    n = 4000
    hp = dict(lr=1e-3, weight_decay=wd, beta1=beta1, beta2=0.999, eps=1e-8)
    p0 = rs.uniform(0.01, 0.1, n).astype(np.float32)
    g0 = (rs.uniform(0.1, 1.0, n) * 10.0 ** rs.randint(-3, 1, n)).astype(np.float32)
    zero = np.zeros(n, np.float32)
    p1, m1, v1 = TC.adam_f32(p0, g0, zero, zero, hp, step)
    f = lambda x: float(np.float32(x))
    prm = torch.nn.Parameter(torch.tensor(p0.astype(np.float64)))
    opt = torch.optim.Adam([prm], lr=f(hp["lr"]), betas=(f(beta1), f(hp["beta2"])), eps=f(hp["eps"]), weight_decay=f(wd))
    prm.grad = torch.tensor(g0.astype(np.float64))
    if step > 1:
        opt.state[prm] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.zeros_like(prm), exp_avg_sq=torch.zeros_like(prm))
    opt.step()
    st = opt.state[prm]
    assert int(st["step"]) == step
    m64, v64, p64 = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), prm.detach().numpy()
    assert (np.abs(m1 - m64) <= 3 * U * np.abs(m64)).all()
    assert (np.abs(v1 - v64) <= 6 * U * np.abs(v64)).all()
    upd = np.abs(p64 - p0.astype(np.float64))
    assert (np.abs(p1 - p64) <= U * (np.abs(p64) + 14 * upd)).all()
    assert (upd > 64 * U * np.abs(p64)).all()                      # (the update is visible in float32: the check is not vacuous)
    # the host's bias corrections are what ops.adam_dyn_values hands to the dyn form
    from snn_modulation_classification_amd import ops
    assert [np.float32(x) for x in ops.adam_dyn_values([dict(hp, step=step)])] == list(TC.adam_host_triple(hp["lr"], beta1, hp["beta2"], step))


def test_adam_restatement_takes_both_lerp_branches_and_keeps_float32():
    hp = dict(lr=1e-3, weight_decay=10.0, beta1=0.9, beta2=0.999, eps=1e-8)
    c = dict(seed=3, sizes=[300], step=2)
    t = TC.adam_data(c)[0]
    for b1 in (0.0, 0.9):
        p, m, v = TC.adam_f32(t["param"], t["grads"][0], t["exp_avg"], t["exp_avg_sq"], dict(hp, beta1=b1), 2)
        assert p.dtype == m.dtype == v.dtype == np.float32 and np.isfinite(p).all() and (v >= 0).all()
        g = t["grads"][0] + np.float32(10.0) * t["param"]
        assert b1 != 0.0 or np.array_equal(m, g)                   # beta1 = 0: lerp's second branch returns g itself


VOTES = [c for c in CASES if c["call"] == "vote" and c["want_vote"]]


@pytest.mark.parametrize("case", VOTES, ids=_ids(VOTES))
def test_vote_reference_agrees_with_the_c_oracle(case):
    from oracle import c_oracle
    c = case
    lg = TC.vote_data(c)
    clout = lg.argmax(axis=2).astype(np.int32)
    oc, ov = c_oracle.argmax_vote(lg, c["t_begin"])
    assert np.array_equal(oc, clout) and np.array_equal(ov, TC.vote_ref(clout, c["t_begin"]))
    if c["draw"] == "ties" and c["N"] > 1 and c["T"] * c["B"] > 100:
        top = np.sort(lg, axis=2)
        assert (top[..., -1] == top[..., -2]).mean() > 0.05        # the draw does meet exact ties


CONT_STEPS = [c for c in CASES if c["call"] in ("step", "multi") and c["draw"] == "cont" and c.get("clout")]


@pytest.mark.parametrize("case", CONT_STEPS, ids=_ids(CONT_STEPS))
def test_unasserted_argmax_rows_of_continuous_draws_are_at_most_two_percent(case):
    c = case
    items = [c] if c["call"] == "step" else c["items"]
    for j, it in enumerate(items):
        d = TC.step_data(it, "cont", c["seed"] + j, c["target"])
        unsure = int((~d["sure"]).sum())
        assert unsure <= 0.02 * it["rows"], (j, unsure, it["rows"])


def test_exact_step_draws_tie_across_the_block_edge():
    c = next(c for c in CASES if c["call"] == "step" and c["draw"] == "grid" and c["N2"] and c["N1"] >= 3)
    d = TC.step_data(c, "grid", c["seed"], c["target"])
    N1 = c["N1"]
    assert np.array_equal(d["ref"][:, N1 - 1], d["ref"][:, N1]) and d["sure"].all()
    i, j = TC.step_ties(N1, c["N2"], c["seed"])[0]
    assert N1 <= i < j and np.array_equal(d["ref"][:, i], d["ref"][:, j])
    assert not (d["clout_ref"] == j - N1).any()                    # the first of two equal maxima is recorded
