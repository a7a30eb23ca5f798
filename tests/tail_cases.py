"""Seeded cases of the readout and learning-tail C ABI — dcll_readout, dcll_readout_mode, dcll_readout_splitk, dcll_readout_act,
dcll_step_readouts, dcll_step_readouts_multi, dcll_local_loss_grad, dcll_adam_step, dcll_adam_step_dyn, dcll_grad_reduce_adam and
dcll_argmax_vote — with their references and the library's dispatch RESTATED (not imported: a moved threshold fails a test).
No torch.cuda here: tests/test_tail_cases.py proves the list on the CPU, tests/test_gpu_tail_fuzz.py runs it on the MI355X.

Draw kinds of the GEMMs
  grid   pv, Wt, bias = small integers times a power of two, chosen per K so that (sum_k |pv Wt| + |bias|) / q < 2^24 for every
         output: every partial sum in every order is exactly representable (split-K partials and k_readout_sum included), so the
         device must return the float64 reference BIT FOR BIT.
  probe  one non-zero operand per row (sigmoid forms: v = -100 everywhere, whose sigmoid is 0 on the device and < 4e-44 anywhere,
         and v = 0 — sigmoid exactly 0.5 — in one column): out[r, n] == c * Wt[n, k_r] + bias[n], exact on the grid, bit for bit.
         k_r walks over the chunk, slice and float4 edges (probe_columns): row r takes entry (start + r) of that list, start = the
         case's probe_start or else its seed.  A case of few rows covers only a stretch of the list; every kernel form therefore
         has `cover` cases — one with at least as many rows as the list has columns, or several with consecutive starts where
         the 64 MB limit forbids that (K = 65280) — and tests/test_tail_cases.py asserts, per variant key, that the union of k_r
         over a cover group is the whole list.
  cont   the workload's own distribution against float64, within the header's 1e-4 (LOGIT_TOL).
"""
import collections
import math
import zlib

import numpy as np

F = np.float32
LOGIT_TOL = 1e-4                                    # include/dcll_hip.h: readouts not bit-pinned, |err| <= 1e-4
AUTO, CORESIDENT, LDS, T16 = 0, 1, 2, 3             # dcll_readout_mode
ACT_NONE, ACT_SIGMOID = 0, 1
SMOOTH_L1, MSE = 0, 1
ADAM_MAX_TENSORS, REDUCE_MAX_LAYERS, STEP_RO_MAX, VOTE_MAXN = 8, 4, 8, 64
MB64 = 64 << 20

# ----------------------------------------------------------------------------------------------------------------------
# the dispatch, restated from csrc/dcll_hip.hip, csrc/dcll_readout.hip and csrc/dcll_learn.hip
# ----------------------------------------------------------------------------------------------------------------------


def nt16(N):
    """column tiles of dcll_launch_readout_t16 / _t16_multi"""
    return 1 if N <= 16 else 2 if N <= 32 else 3 if N <= 48 else 4


def nt_direct(N):
    return 1 if N <= 16 else 2 if N <= 32 else 3


def fast(K, N, aligned):
    return K % 32 == 0 and N <= 64 and aligned and K < (1 << 22)


def launch_readout(rows, K, N, mode, aligned):
    """launch_readout -> variant key of the one kernel it starts"""
    fs = fast(K, N, aligned)
    direct_ok = fs and K % 64 == 0 and N <= 48 and K <= 16384 and mode != LDS
    if direct_ok and mode == CORESIDENT:
        return ("k_readout_direct", nt_direct(N))
    if fs and mode == T16:
        return ("k_readout_t16", nt16(N), 0, "whole")
    if rows <= 2048:
        return ("k_readout_rows",)
    if fs and K % 256 == 0 and K >= 65536 and rows < 256 * 128:
        return ("k_readout_ks", 1 if N <= 32 else 2, "whole")
    if fs and mode != LDS:
        return ("k_readout_t16", nt16(N), 0, "whole")
    if fs:
        return ("k_readout_v4", 1 if N <= 32 else 2)
    return ("k_readout",)


def splitk_slice(rows, K, N):
    if rows < 1 or N < 1 or N > 64:
        return 0
    if K >= 65536 and K % 4096 == 0:
        return 4096 if rows <= 2048 else K // 8
    if rows <= 2048 and 2048 <= K < 65536 and K % 256 == 0:
        return 128 if (rows <= 512 and N <= 32) else 256
    return 0


def splitk_scratch(rows, K, N):
    ks = splitk_slice(rows, K, N)
    return K // ks * rows * N if ks else 0


def act_nslice(K):
    if K < 65536 or K % 256 != 0:
        return 0
    n = 8
    while n < 64 and K // (2 * n) >= 8192 and K % (2 * n * 32) == 0:
        n *= 2
    return n


def act_scratch(rows, K, N):
    return act_nslice(K) * rows * N if rows > 0 and N > 0 else 0


def step_scratch(rows, K, N1, N2):
    if K >= 65536 or N1 + N2 > 64 or N1 < 1 or N2 < 0:
        return 0
    return splitk_scratch(rows, K, N1 + N2)


def reduce_groups(nchunk):
    return 16 if nchunk >= 64 else 4 if nchunk >= 16 else 1


def block_prefix(sizes, per_block, skip=None):
    """adam_fill: first[] in workgroups of per_block elements; skipped tensors get none"""
    first, blocks = [], 0
    for k, n in enumerate(sizes):
        first.append(blocks)
        if not (skip and skip[k]):
            blocks += (n + per_block - 1) // per_block
    return first + [blocks]


def reduce_adam_grid(layers, sizes):
    """workgroups of k_grad_reduce_adam: 64 gradient elements each per layer, then 1024 elements of every tensor no layer refers to"""
    taken = [False] * len(sizes)
    for L in layers:
        for idx in (L["adam_w"], L["adam_b"]):
            if idx >= 0:
                taken[idx] = True
    return sum((L["c_out"] * L["rowlen"] + 63) // 64 for L in layers) + block_prefix(sizes, 1024, taken)[-1]


def argmax_path(N, off):
    """k_argmax: 16-byte loads when the rows are multiples of 16 bytes on a 16-byte base"""
    return "v4" if N % 4 == 0 and not off else "scalar"


def t16m_item_nt(nt_launch, N):
    """k_readout_t16m<NT>: an item of at most 32 columns runs the <2> body inside a <3> or <4> launch"""
    return 2 if nt_launch >= 3 and N <= 32 else nt_launch


# ----------------------------------------------------------------------------------------------------------------------
# what a case dispatches
# ----------------------------------------------------------------------------------------------------------------------
GEMM_CALLS = ("readout", "mode", "splitk", "act")


def gemm_plan(c):
    """-> dict(key, kernels, kslice): variant key, launch log and the K-slice width (0: unsplit) of a GEMM case"""
    rows, K, N = c["rows"], c["K"], c["N"]
    aligned = not (c["off_pv"] or c["off_wt"])
    if c["call"] in ("readout", "mode"):
        key = launch_readout(rows, K, N, c["mode"] if c["call"] == "mode" else AUTO, aligned)
        return dict(key=key, kernels=[key[0]], kslice=0)
    assert aligned, c["id"]
    if c["call"] == "splitk":
        ks = splitk_slice(rows, K, N)
        assert ks, c["id"]
        if ks == 4096:
            return dict(key=("k_readout_ks", 1 if N <= 32 else 2, "split"), kernels=["k_readout_ks (split K)", "k_readout_sum"], kslice=ks)
        return dict(key=("k_readout_t16", nt16(N), 0, "split"), kernels=["k_readout_t16", "k_readout_sum"], kslice=ks)
    assert c["call"] == "act" and fast(K, N, True), c["id"]
    ns, sig = act_nslice(K), int(c["sig"])
    if ns == 0:
        return dict(key=("k_readout_t16", nt16(N), sig, "whole"), kernels=["k_readout_t16"], kslice=0)
    return dict(key=("k_readout_t16", nt16(N), sig, "split"), kernels=["k_readout_t16", "k_readout_sum"], kslice=K // ns)


def variant_keys(c):
    """every variant key the case's call serves (a multi call serves one k_readout_t16m key per item)"""
    call = c["call"]
    if call in GEMM_CALLS:
        return [gemm_plan(c)["key"]]
    if call == "step":
        return [("k_step_readout_finish", int(c["target"]))]
    if call == "multi":
        ntl = nt16(max(it["N1"] + it["N2"] for it in c["items"]))
        keys = [("k_step_readout_finish_m", int(c["target"]))]
        for it in c["items"]:
            k = ("k_readout_t16m", ntl, t16m_item_nt(ntl, it["N1"] + it["N2"]))
            if k not in keys:
                keys.append(k)
        return keys
    if call == "loss":
        return [("k_loss_grad", c["kind"], int(c["has_o"]))]
    if call == "adam":
        return [("k_adam_multi", "dyn" if c["dyn"] else "host")]
    if call == "reduce_adam":
        return [("k_grad_reduce_adam", reduce_groups(L["nchunk"])) for L in c["layers"]] or [("k_grad_reduce_adam", 0)]
    assert call == "vote", call
    return [("k_argmax", argmax_path(c["N"], c["off"]))] + ([("k_vote",)] if c["want_vote"] else [])


def variant_key(c):
    return variant_keys(c)[0]


def expected_kernels(c):
    """the launch log of the case's call"""
    call = c["call"]
    if call in GEMM_CALLS:
        return gemm_plan(c)["kernels"]
    if call == "step":
        return ["k_readout_t16", "k_step_readout_finish"]
    if call == "multi":
        return ["k_readout_t16m", "k_step_readout_finish_m"]
    if call == "loss":
        return ["k_loss_grad"]
    if call == "adam":
        return ["k_adam_multi"] if block_prefix(c["sizes"], 256)[-1] else []
    if call == "reduce_adam":
        return ["k_grad_reduce_adam"]
    return ["k_argmax"] + (["k_vote"] if c["want_vote"] else [])


def expected_scratch(c):
    """what dcll_readout_splitk_scratch / dcll_readout_act_scratch / dcll_step_readouts_scratch answer for the case's shape"""
    if c["call"] in GEMM_CALLS:
        return dict(splitk=splitk_scratch(c["rows"], c["K"], c["N"]), act=act_scratch(c["rows"], c["K"], c["N"]),
                    step=step_scratch(c["rows"], c["K"], c["N"], 0))
    if c["call"] == "step":
        return dict(step=step_scratch(c["rows"], c["K"], c["N1"], c["N2"]))
    if c["call"] == "multi":
        return dict(step=[step_scratch(it["rows"], it["K"], it["N1"], it["N2"]) for it in c["items"]])
    return {}


def reachable_variants():
    keys = [("k_readout_t16", nt, sig, form) for nt in (1, 2, 3, 4) for sig in (0, 1) for form in ("split", "whole")]
    keys += [("k_readout_t16m", ntl, t16m_item_nt(ntl, n)) for ntl in (1, 2, 3, 4) for n in (16 * ntl,)]
    keys += [("k_readout_t16m", 3, 2), ("k_readout_t16m", 4, 2)]
    keys += [("k_readout_direct", nt) for nt in (1, 2, 3)]
    keys += [("k_readout_ks", nt, form) for nt in (1, 2) for form in ("split", "whole")]
    keys += [("k_readout_v4", 1), ("k_readout_v4", 2), ("k_readout_rows",), ("k_readout",)]
    keys += [("k_step_readout_finish", l) for l in (0, 1)] + [("k_step_readout_finish_m", l) for l in (0, 1)]
    keys += [("k_adam_multi", "dyn"), ("k_adam_multi", "host")] + [("k_grad_reduce_adam", g) for g in (0, 1, 4, 16)]       # (0: no layer)
    keys += [("k_argmax", "v4"), ("k_argmax", "scalar"), ("k_vote",)]
    keys += [("k_loss_grad", kind, o) for kind in (SMOOTH_L1, MSE) for o in (0, 1)]
    return keys


def device_bytes(c):
    """device memory of the case's operands, outputs and scratch"""
    call = c["call"]
    if call in GEMM_CALLS:
        s = expected_scratch(c)
        return 4 * (c["rows"] * c["K"] + c["N"] * c["K"] + c["N"] + c["rows"] * c["N"] + max(s["splitk"], s["act"]))
    if call == "step":
        N = c["N1"] + c["N2"]
        return 4 * (c["rows"] * c["K"] + N * c["K"] + N + 4 * c["rows"] * N + step_scratch(c["rows"], c["K"], c["N1"], c["N2"]))
    if call == "multi":
        return sum(device_bytes(dict(it, call="step")) for it in c["items"])
    if call == "loss":
        return 4 * 5 * c["B"] * c["N"]
    if call == "adam":
        return 4 * 4 * (sum(c["sizes"]) + 64 * (len(c["sizes"]) + 1))
    if call == "reduce_adam":
        return 4 * (sum(L["nchunk"] * L["c_out"] * L["rowlen"] for L in c["layers"]) + 4 * sum(adam_sizes(c)) + 4096)
    return 4 * c["T"] * c["B"] * (c["N"] + 1)


# ----------------------------------------------------------------------------------------------------------------------
# float32 restatements of the device arithmetic (+ - x / and sqrt only, every operation rounded: the library is built with
# -ffp-contract=off), operation order as in csrc/dcll_learn.hip
# ----------------------------------------------------------------------------------------------------------------------


def loss_elem_f32(d, kind):
    """loss_elem: (value, derivative) of one logit's local loss, d = logit - target"""
    d = np.asarray(d, F)
    if kind == MSE:
        return d * d, F(2.0) * d
    a = np.abs(d)
    l = np.where(a < F(1.0), (F(0.5) * d) * d, a - F(0.5)).astype(F)
    g = np.where(a < F(1.0), d, np.where(d > F(0.0), F(1.0), F(-1.0))).astype(F)
    return l, g


def loss_grad_f32(logits, target, kind, n):
    """g * (1.0f / n) of k_loss_grad / k_step_readout_finish"""
    inv = F(1.0) / F(n)
    return (loss_elem_f32(np.asarray(logits, F) - np.asarray(target, F), kind)[1] * inv).astype(F)


def adam_host_triple(lr, beta1, beta2, step):
    """(lr, 1 / bc1, 1 / sqrt(bc2)) as adam_fill computes them: float64 arithmetic on the struct's float32 betas, then cast"""
    b1, b2 = float(F(beta1)), float(F(beta2))
    return F(lr), F(1.0 / (1.0 - math.pow(b1, step))), F(1.0 / math.sqrt(1.0 - math.pow(b2, step)))


def adam_f32(p, grad, m, v, hp, step):
    """adam_update on float32 arrays -> (p, m, v); hp = dict(lr, weight_decay, beta1, beta2, eps)"""
    p, grad, m, v = (np.asarray(x, F) for x in (p, grad, m, v))
    lr, ibc1, isbc2 = adam_host_triple(hp["lr"], hp["beta1"], hp["beta2"], step)
    g = grad + F(hp["weight_decay"]) * p
    w = F(1.0) - F(hp["beta1"])
    m = m + w * (g - m) if w < F(0.5) else g - (g - m) * (F(1.0) - w)
    v = v * F(hp["beta2"]) + ((F(1.0) - F(hp["beta2"])) * g) * g
    denom = np.sqrt(v) * isbc2 + F(hp["eps"])
    p = p - (lr * ibc1) * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F
    return p, m, v


def vote_ref(clout, t_begin):
    """Counter(...).most_common(1) per sample over the recorded steps: ties go to the class seen first"""
    T, B = clout.shape
    return np.array([collections.Counter(clout[t_begin:, b].tolist()).most_common(1)[0][0] for b in range(B)], np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# draws
# ----------------------------------------------------------------------------------------------------------------------


def grid_of(K):
    """(A, Bw, wq, Bb): pv in {0..A} / A, Wt in {-Bw..Bw} * wq, bias in {-Bb..Bb} * wq; quantum q = wq / A.  Sufficient for the
    exactness condition: every |term| / q <= A Bw, |bias| / q <= A Bb, so K A Bw + A Bb < 2^24 bounds every output."""
    A, Bw, wq, Bb = (16, 8, 2.0 ** -10, 8) if K <= 8192 else (4, 4, 2.0 ** -3, 8)
    assert K * A * Bw + A * Bb < 2 ** 24
    return A, Bw, wq, Bb


def probe_columns(K, kslice=0):
    """the columns a probe's rows walk over: first and last of the first, second and last 32-float chunk, both sides of every
    K-slice boundary (and of the 64-float wave shares of k_readout_ks's 256-float chunk), the 8 float4 positions of a chunk"""
    cols = []
    for c0 in (0, 32, (K - 1) // 32 * 32):
        cols += [c0, min(c0 + 31, K - 1)]               # (a ragged last chunk ends at K - 1)
    cols += [4 * j + j % 4 for j in range(8)] + [32 + 4 * j + (j + 1) % 4 for j in range(8)]
    for b in (64, 128, 192, 256):
        cols += [b - 1, b]
    if kslice:
        for b in range(kslice, K, kslice):
            cols += [b - 1, b]
    seen, out = set(), []
    for k in cols:
        if 0 <= k < K and k not in seen:
            seen.add(k)
            out.append(k)
    return out


def probe_kr(c, rows=None, cols=None):
    """the column k_r of every row of a probe draw"""
    rows = c["rows"] if rows is None else rows
    cols = probe_columns(c["K"], c.get("kslice", 0)) if cols is None else cols
    start = c["seed"] if c.get("probe_start") is None else c["probe_start"]
    return np.array([cols[(start + r) % len(cols)] for r in range(rows)])


def exactness(pv_abs_units, wt_abs_units, bias_abs_units):
    """max over outputs of (sum_k |pv Wt| + |bias|) / q, from the operands in units of their quanta"""
    return float((pv_abs_units.astype(np.float64) @ wt_abs_units.astype(np.float64).T + bias_abs_units).max())


def gemm_data(c, N=None, ties=None, seed=None):
    """operands and float64 reference of a GEMM (also of the GEMM inside a step / multi item: N = N1 + N2, ties = pairs (i, j) of
    readout rows made identical so that their logits tie exactly).
    -> dict(pv | pv_i8 + pv_scale, Wt, bias, ref (float64), units = the exactness figure for grid / probe draws)"""
    rows, K = c["rows"], c["K"]
    N = c["N"] if N is None else N
    rs = np.random.RandomState(c["seed"] if seed is None else seed)
    draw, sig = c["draw"], bool(c.get("sig"))
    out = {}
    if draw == "grid":
        assert not sig
        A, Bw, wq, Bb = grid_of(K)
        x = rs.randint(0, A + A // 2 + 1, size=(rows, K), dtype=np.int8)
        x[x > A] = 0                                            # about a third of a spike trace is zero
        wi = rs.randint(-Bw, Bw + 1, size=(N, K)).astype(np.int8)
        bi = rs.randint(-Bb, Bb + 1, size=N)
        for i, j in ties or ():
            wi[j], bi[j] = wi[i], bi[i]
        Wt, bias = wi.astype(F) * F(wq), (bi * wq).astype(F)
        if c.get("big"):
            ref = np.empty((rows, N), np.float64)
            W64 = Wt.astype(np.float64)
            for r0 in range(0, rows, 256):
                ref[r0:r0 + 256] = (x[r0:r0 + 256].astype(np.float64) / A) @ W64.T
            out.update(pv_i8=x, pv_scale=1.0 / A)
            out["units"] = K * A * Bw + A * Bb                  # (the sufficient bound: the matrix product is not repeated)
        else:
            pv = x.astype(F) / F(A)
            ref = pv.astype(np.float64) @ Wt.astype(np.float64).T
            out["pv"] = pv
            out["units"] = exactness(np.abs(x), np.abs(wi), np.abs(bi) * A)
    elif draw == "probe":
        cols = probe_columns(K, c.get("kslice", 0))
        kr = probe_kr(c, rows, cols)
        pv = np.full((rows, K), -100.0 if sig else 0.0, F)
        pv[np.arange(rows), kr] = 0.0 if sig else 1.0
        wi = rs.randint(1, 9, size=(N, K)) * rs.choice([-1, 1], size=(N, K))     # never 0: a mis-routed lane cannot hide
        bi = rs.randint(16, 33, size=N)                                         # |c Wt| <= 8 < 16 <= bias: no cancellation
        for i, j in ties or ():
            wi[j], bi[j] = wi[i], bi[i]
        Wt, bias = (wi * 2.0 ** -10).astype(F), (bi * 2.0 ** -10).astype(F)
        cc = 0.5 if sig else 1.0
        ref = cc * Wt.astype(np.float64)[:, kr].T
        out.update(pv=pv, kr=kr, units=float(np.abs(wi).max() + 2 * bi.max()))     # in units of 2^-11
    else:
        assert draw == "cont", draw
        s = 0.0055 * math.sqrt(8192.0 / K)
        pv = (rs.randn(rows, K) * 2.5).astype(F) if sig else rs.uniform(0, 1, size=(rows, K)).astype(F)
        Wt, bias = rs.uniform(-s, s, size=(N, K)).astype(F), rs.uniform(-s, s, size=N).astype(F)
        a = 1.0 / (1.0 + np.exp(-pv.astype(np.float64))) if sig else pv.astype(np.float64)
        ref = a @ Wt.astype(np.float64).T
        out["pv"] = pv
    if c.get("bias", True):
        ref = ref + bias.astype(np.float64)
    out.update(Wt=Wt, bias=bias, ref=ref)
    return out


def step_ties(N1, N2, seed):
    """readout rows made identical in a step's grid / probe draw: a pair inside the recorded block and — on an output layer — the
    last row of p against the first of o, which must not leak across lo = N1"""
    rs = np.random.RandomState(seed ^ 0x5eed)
    ties = []
    lo = N1 if N2 else 0
    if N1 >= 3:
        i, j = sorted(rs.choice(N1, 2, replace=False))
        ties.append((lo + int(i), lo + int(j)))
    if N2:
        ties.append((N1 - 1, N1))
    return ties


def step_data(it, draw, seed, learn):
    """one dcll_step_readouts call (or multi item): GEMM data + target; clout_ref = first maximum of the float64 logits of the
    recorded block and sure = the rows whose two best reference logits are at least 2 LOGIT_TOL apart (all rows for exact draws)"""
    N1, N2 = it["N1"], it["N2"]
    c = dict(rows=it["rows"], K=it["K"], draw=draw, seed=seed, kslice=splitk_slice(it["rows"], it["K"], N1 + N2))
    d = gemm_data(c, N=N1 + N2, ties=step_ties(N1, N2, seed) if draw != "cont" else None)
    rec = d["ref"][:, N1:] if N2 else d["ref"][:, :N1]
    d["clout_ref"] = rec.argmax(axis=1).astype(np.int32)
    if draw == "cont" and rec.shape[1] > 1:
        top = np.sort(rec, axis=1)[:, -2:]
        d["sure"] = (top[:, 1] - top[:, 0]) >= 2 * LOGIT_TOL
    else:
        d["sure"] = np.ones(it["rows"], bool)
    if learn:
        rs = np.random.RandomState(seed ^ 0x7a9)
        d["target"] = (rs.randint(-8, 9, size=(it["rows"], N1)) / 8.0).astype(F) if draw != "cont" else \
            rs.uniform(-1, 1, size=(it["rows"], N1)).astype(F)
    return d


KINK = [1.0, -1.0, float(np.nextafter(F(1), F(0))), float(np.nextafter(F(1), F(2))), -float(np.nextafter(F(1), F(0))),
        -float(np.nextafter(F(1), F(2))), 0.0]


def loss_data(c):
    """p, o, target: the first elements sit on SmoothL1's kink (target 0, so that d = p exactly), the rest spread over +-2.5;
    logits rounded to 1/2 elsewhere in every fourth row so that the argmax meets exact ties"""
    rs = np.random.RandomState(c["seed"])
    B, N = c["B"], c["N"]
    n = B * N
    t = rs.uniform(-1, 1, size=n).astype(F)
    out = {}
    for name in ("p", "o"):
        x = (t.astype(np.float64) + rs.uniform(-2.5, 2.5, size=n)).astype(F)
        x = x.reshape(B, N)
        x[::4] = np.round(x[::4] * 2) / 2
        x = x.reshape(n)
        k = min(n, len(KINK))
        x[:k] = np.array(KINK[:k], F)
        out[name] = x.reshape(B, N)
    t[:min(n, len(KINK))] = 0.0
    out["target"] = t.reshape(B, N)
    if not c["has_o"]:
        out["o"] = None
    return out


def loss_value_ref(d, kind):
    """float64 loss (mean reduction per criterion, summed) and the bound of a float32 sum of its m summands in any order:
    (m + 3) 2^-24 sum |l_i| / n.  The device also rounds each l_i (<= 3 roundings) and the final product (<= 2): for m >= 16 the
    kernel's tree (at most ceil(m / 256) + 9 additions deep) leaves the room, for m <= 2 (n = 1) the factor 1 / n is exact."""
    t = d["target"].astype(np.float64)
    ls = []
    for x in (d["p"], d["o"]):
        if x is not None:
            dd = x.astype(np.float64) - t
            ls.append(dd * dd if kind == MSE else np.where(np.abs(dd) < 1, 0.5 * dd * dd, np.abs(dd) - 0.5))
    l = np.concatenate([x.ravel() for x in ls])
    n = t.size
    return float(l.sum() / n), (l.size + 3) * 2.0 ** -24 * float(np.abs(l).sum()) / n


def adam_hp(c, k):
    """hyper-parameters of tensor k of an adam / reduce_adam case (they differ per tensor: several optimizers in one launch)"""
    return dict(lr=[1e-3, 5e-4, 2.5e-2][k % 3], weight_decay=c["weight_decay"] if k % 2 == 0 else 10.0 - c["weight_decay"],
                beta1=c["beta1"] if k % 3 != 2 else 0.9 - c["beta1"], beta2=0.999 if k % 2 == 0 else 0.95, eps=1e-8)


def adam_sizes(c):
    return c["sizes"]


def adam_data(c, nsteps=3):
    """per tensor: param, exp_avg, exp_avg_sq (step > 1: a running state) and one gradient per step; some gradients exactly 0"""
    rs = np.random.RandomState(c["seed"])
    out = []
    for k, n in enumerate(adam_sizes(c)):
        fresh = c["step"] == 1
        g = (rs.randn(nsteps, n) * 10.0 ** rs.randint(-3, 1)).astype(F)
        g[:, ::7] = 0.0
        out.append(dict(param=(rs.randn(n) * 0.05).astype(F), exp_avg=np.zeros(n, F) if fresh else (rs.randn(n) * 0.01).astype(F),
                        exp_avg_sq=np.zeros(n, F) if fresh else (rs.randn(n) ** 2 * 1e-4).astype(F), grads=g))
    return out


def reduce_data(c):
    """partial rows of every layer: integers (exact sums in any order) or continuous"""
    rs = np.random.RandomState(c["seed"] ^ 0x9e37)
    parts = []
    for L in c["layers"]:
        shape = (L["nchunk"], L["c_out"] * L["rowlen"])
        parts.append(rs.randint(-64, 65, size=shape).astype(F) * F(2.0 ** -6) if c["draw"] == "int" else rs.randn(*shape).astype(F))
    return parts


def vote_data(c):
    """logits (T, B, N): rounded to a coarse grid (many exact ties), or every row constant"""
    rs = np.random.RandomState(c["seed"])
    T, B, N = c["T"], c["B"], c["N"]
    if c["draw"] == "equal":
        return np.repeat(rs.randint(-3, 4, size=(T, B, 1)).astype(F), N, axis=2)
    return (np.round(rs.randn(T, B, N) * 2) / 2).astype(F)


# ----------------------------------------------------------------------------------------------------------------------
# the case list
# ----------------------------------------------------------------------------------------------------------------------
NS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
R128 = [1, 31, 32, 33, 127, 128, 129]              # wave tile 32, workgroup tile 128: k_readout_t16, k_readout_v4, k_readout
RDIR = [1, 15, 16, 17, 63, 64, 65]                 # wave tile 16, workgroup tile 64: k_readout_direct
RSTEP = [1, 5, 128, 129, 512, 513, 2048]
BIG = {"variants-readout-r2049k65792n24-grid", "variants-readout-r2049k65792n48-grid", "variants-splitk-r2049k65536n24-grid"}


class _List:
    def __init__(self):
        self.cases, self.ids = [], set()

    def add(self, stratum, call, tag, **kw):
        c = dict(stratum=stratum, call=call, **kw)
        c["id"] = "%s-%s-%s" % (stratum, call if call != "mode" else "mode%d" % kw["mode"], tag)
        if c["id"] in self.ids:
            return
        c["seed"] = zlib.crc32(c["id"].encode()) & 0x3fffffff
        self.ids.add(c["id"])
        self.cases.append(c)

    def gemm(self, stratum, call, rows, K, N, mode=AUTO, sig=False, bias=True, off_pv=0, off_wt=0, big=False, draws=None, probe_start=None,
             cover=None):
        """cover: name of a group of probe cases whose rows together walk the form's whole column list (probe_start: where in the
        list the case's first row stands)"""
        if draws is None:
            draws = ("grid",) if big else ("probe", "cont") if sig else ("grid", "probe", "cont")
        for draw in draws:
            tag = "r%dk%dn%d%s%s%s%s-%s" % (rows, K, N, "-sig" if sig else "", "" if bias else "-nobias", "-offpv" if off_pv else "",
                                            "-offwt" if off_wt else "", draw) + \
                ("" if probe_start is None else "-from%d" % probe_start)
            c = dict(rows=rows, K=K, N=N, mode=mode, sig=sig, bias=bias, off_pv=off_pv, off_wt=off_wt, big=big, draw=draw, probe_start=probe_start,
                     cover=cover)
            c["kslice"] = gemm_plan(dict(c, call=call, id=tag))["kslice"]
            self.add(stratum, call, tag, **c)


def _fit_k(rows, K):
    """the largest listed K that keeps rows x K within 48 MB (the case's 64 MB include Wt, the outputs and the partial tiles)"""
    return K if rows * K * 4 <= 48 << 20 else 2304


def _variants(L):
    S = "variants"
    for i, N in enumerate(NS):
        L.gemm(S, "mode", R128[i % 7], [32, 64, 96, 2048, 2304][i % 5], N, mode=T16)
        L.gemm(S, "act", R128[(i + 3) % 7], [32, 64, 96, 2048, 2304][(i + 2) % 5], N, sig=True)
        L.gemm(S, "splitk", RSTEP[i % 7], _fit_k(RSTEP[i % 7], [2048, 2304, 8192][i % 3]), N)
    for i, N in enumerate((16, 17, 48, 64)):
        L.gemm(S, "act", R128[(i + 1) % 7], [96, 2304, 64, 32][i], N)
    L.gemm(S, "readout", 2049, 64, 24)                             # AUTO above 2048 rows: k_readout_t16, whole
    L.gemm(S, "splitk", 33, 65280, 32)                             # 510 slices of 128
    L.gemm(S, "splitk", 33, 65280, 33)                             # 255 slices of 256
    L.gemm(S, "splitk", 128, 65280, 16)
    for i, (N, rows) in enumerate(((16, 1), (17, 31), (48, 32), (49, 33))):
        L.gemm(S, "act", rows, 65536, N, sig=True)                 # the act split: 8 slices of 8192
        L.gemm(S, "act", rows, 65536, N)
    for i, N in enumerate(NS[:9]):
        L.gemm(S, "mode", RDIR[i % 7], [64, 128, 2048, 2304][i % 4], N, mode=CORESIDENT)
    for rows, N in ((31, 1), (32, 32), (33, 33), (32, 64)):
        L.gemm(S, "splitk", rows, 65536, N)                        # k_readout_ks, 16 slices of 4096
    # k_readout_v4, k_readout (and k_readout_t16 through AUTO) serve only calls of more than 2048 rows = 16 workgroup tiles: the
    # LAST workgroup gets the rows on both sides of the 32-row wave tile and of the 128-row workgroup tile
    for i, tail in enumerate(R128):
        L.gemm(S, "mode", 2048 + tail, [32, 64, 96][i % 3], (1, 31, 32)[i % 3], mode=LDS)           # k_readout_v4<1>
        L.gemm(S, "mode", 2048 + tail, [64, 96, 32][i % 3], (33, 63, 64)[(i + 1) % 3], mode=LDS)    # k_readout_v4<2>
        K, N = ((64, 65), (33, 24), (100, 17), (100, 33))[i % 4]
        L.gemm(S, "readout", 2048 + tail, K, N)                    # k_readout
        L.gemm(S, "readout", 2048 + tail, [96, 32, 64][i % 3], (16, 24, 48, 64)[i % 4])             # k_readout_t16, whole, by AUTO
    L.gemm(S, "readout", 2177, 100, 33)                            # k_readout: two row tiles past 2048 and two column blocks
    L.gemm(S, "mode", 2049, 100, 24, mode=T16)                     # not fast: T16 falls through to k_readout
    for i, (rows, N) in enumerate(((3, 3), (4, 4), (5, 5), (4, 17), (2048, 64))):
        L.gemm(S, "readout", rows, [33, 100, 32, 2048, 64][i], N)  # k_readout_rows
    L.gemm(S, "mode", 16, 96, 24, mode=CORESIDENT)                 # K % 64 != 0: not the LDS-free form
    L.gemm(S, "mode", 33, 64, 24, mode=LDS)                        # few rows: k_readout_rows in every mode but T16
    # bias = NULL once per family
    L.gemm(S, "mode", 33, 64, 17, mode=T16, bias=False)
    L.gemm(S, "mode", 17, 64, 17, mode=CORESIDENT, bias=False)
    L.gemm(S, "mode", 2049, 32, 33, mode=LDS, bias=False)
    L.gemm(S, "readout", 5, 100, 5, bias=False)
    L.gemm(S, "readout", 2049, 33, 5, bias=False)
    L.gemm(S, "splitk", 129, 2304, 24, bias=False)
    L.gemm(S, "splitk", 33, 65536, 24, bias=False)
    L.gemm(S, "act", 33, 96, 24, sig=True, bias=False)
    L.gemm(S, "act", 5, 65536, 24, bias=False)
    # pv or Wt 4 bytes off a 16-byte boundary: AUTO falls back to the kernels without vector loads
    L.gemm(S, "readout", 5, 2048, 24, off_pv=1)
    L.gemm(S, "readout", 5, 2048, 24, off_wt=1)
    L.gemm(S, "readout", 2049, 64, 24, off_pv=1)
    L.gemm(S, "readout", 2049, 64, 24, off_wt=1)
    L.gemm(S, "mode", 33, 64, 24, mode=T16, off_wt=1)
    # the three forms that need more than 2048 rows of at least 65536 columns (0.54 GB each): grid draws, generated as int8
    L.gemm(S, "readout", 2049, 65792, 24, big=True)                # k_readout_ks<1>, unsplit
    L.gemm(S, "readout", 2049, 65792, 48, big=True)                # k_readout_ks<2>, unsplit
    L.gemm(S, "splitk", 2049, 65536, 24, big=True)                 # k_readout_t16 in 8 slices of K / 8


def _probe_cover(L):
    """per kernel form probe cases whose rows walk the WHOLE list of probe_columns (see the module docstring)"""
    S = "variants"

    def whole(name, call, K, N, rows_min=0, **kw):
        plan = gemm_plan(dict(call=call, rows=max(rows_min, 1), K=K, N=N, mode=kw.get("mode", AUTO), sig=kw.get("sig", False), off_pv=0,
                              off_wt=0, id=name))
        rows = max(rows_min, len(probe_columns(K, plan["kslice"])) + 3)
        L.gemm(S, call, rows, K, N, draws=("probe",), probe_start=0, cover=name, **kw)

    for N in (15, 32, 33, 64):
        whole("t16-whole-n%d" % N, "mode", 2304, N, mode=T16)
        whole("t16-sig-whole-n%d" % N, "act", 2304, N, sig=True)
        whole("t16-split-n%d" % N, "splitk", 2304, N)                          # 18 slices of 128 / 9 of 256
        whole("t16-sig-split-n%d" % N, "act", 65536, N, sig=True)              # 8 slices of 8192
        whole("t16-act-split-n%d" % N, "act", 65536, N)
    for N in (15, 32, 33):
        whole("direct-n%d" % N, "mode", 2304, N, mode=CORESIDENT)
    for N in (32, 33):
        whole("ks-split-n%d" % N, "splitk", 65536, N)                          # 16 slices of 4096
        whole("v4-n%d" % N, "mode", 96, N, rows_min=2049, mode=LDS)
    whole("rows", "readout", 2048, 5)
    whole("k_readout", "readout", 100, 24, rows_min=2049)
    # K = 65280 in 510 slices of 128 (1041 columns) and in 255 of 256 (533): several cases of consecutive starts, each within 64 MB
    for name, N, per in (("t16-split-k65280-slices128", 32, 131), ("t16-split-k65280-slices256", 33, 134)):
        ncol = len(probe_columns(65280, splitk_slice(per, 65280, N)))
        for start in range(0, ncol, per):
            L.gemm(S, "splitk", per, 65280, N, draws=("probe",), probe_start=start, cover=name)


def cover_groups(cs):
    """cover name -> (variant key, column list, union of k_r over the group's cases)"""
    out = {}
    for c in cs:
        if c.get("cover"):
            key, cols, seen = out.setdefault(c["cover"], (variant_key(c), probe_columns(c["K"], c["kslice"]), set()))
            assert key == variant_key(c) and cols == probe_columns(c["K"], c["kslice"]), c["id"]
            seen.update(probe_kr(c).tolist())
    return out


def _step_tail(L):
    N1S = [1, 10, 16, 17, 24, 32]
    for i in range(42):
        rows, N1 = RSTEP[i % 7], N1S[i % 6]
        K = _fit_k(rows, [2048, 2304, 8192][(i // 2) % 3])
        N2 = N1 if (i // 3) % 2 else 0
        kind, clout, target = (i // 5) % 2, i % 4 != 0, i % 3 != 1
        for draw in ("grid", "cont", "probe"):
            L.add("step_tail", "step", "r%dk%dn%d+%d-k%d%s%s-%s" % (rows, K, N1, N2, kind, "-clout" if clout else "", "-learn" if target else "",
                                                                       draw), rows=rows, K=K, N1=N1, N2=N2, kind=kind, clout=clout,
                  target=target, draw=draw)


MULTI = [   # (tag, items (rows, K, N1, N2))
    ("w16+48", [(128, 2048, 16, 0), (5, 2304, 24, 24)]),
    ("w64+24", [(129, 2304, 32, 32), (513, 2048, 24, 0)]),
    ("w48+10", [(33, 8192, 24, 24), (128, 2048, 10, 0)]),
    ("w10+16+1", [(129, 2048, 10, 0), (5, 2304, 16, 0), (513, 2048, 1, 0)]),
    ("w24+32+17", [(1, 8192, 24, 0), (513, 2304, 16, 16), (128, 2048, 17, 0)]),
    ("w49+33+48", [(5, 2048, 49, 0), (129, 2304, 33, 0), (17, 2048, 24, 24)]),
    ("eight", [(128, 2048, 24, 0), (1, 2304, 32, 32), (513, 2048, 10, 0), (5, 8192, 17, 0), (129, 2304, 24, 24), (33, 2048, 1, 0),
               (512, 2048, 16, 16), (2048, 2048, 16, 0)]),
]


def _step_multi(L):
    for i, (tag, items) in enumerate(MULTI):
        its = [dict(rows=r, K=k, N1=a, N2=b, kind=(i + j) % 2) for j, (r, k, a, b) in enumerate(items)]
        for target in (False, True):
            for draw in ("grid", "cont", "probe"):
                L.add("step_multi", "multi", "%s%s-%s" % (tag, "-learn" if target else "", draw), items=its, target=target, clout=True,
                      draw=draw)


def _loss(L):
    shapes = [(1, 1), (255, 1), (256, 1), (4, 64), (257, 1), (37, 24), (65537, 1), (25, 10), (26, 10), (6554, 10), (5, 64), (64, 24)]
    for i, (B, N) in enumerate(shapes):
        for j, (kind, has_o) in enumerate(((SMOOTH_L1, False), (SMOOTH_L1, True), (MSE, False), (MSE, True))):
            clout, loss = (i + j) % 2 == 0, (i + j) % 3 != 0
            L.add("loss", "loss", "b%dn%d-k%d%s%s%s" % (B, N, kind, "-o" if has_o else "", "-clout" if clout else "", "-loss" if loss else ""),
                  B=B, N=N, kind=kind, has_o=has_o, want_clout=clout, want_loss=loss)


def _adam(L):
    configs = [[1], [255], [256], [257], [50176], [255, 1000], [1000, 257], [257, 1, 0, 256, 1000, 255, 50176, 1],
               [1, 255, 256, 257, 1000, 0, 1, 255], [0, 0, 5], [0, 0]]
    for i, sizes in enumerate(configs):
        for dyn in (False, True):
            beta1, wd, step = [0.0, 0.9][(i + dyn) % 2], [0.0, 10.0][(i // 2) % 2], [1, 2, 1000][(i + dyn) % 3]
            L.add("adam", "adam", "%s-b%g-wd%g-s%d-%s" % ("_".join(map(str, sizes)), beta1, wd, step, "dyn" if dyn else "host"), sizes=sizes,
                  dyn=dyn, beta1=beta1, weight_decay=wd, step=step)


def _reduce_adam(L):
    geo = [(1, 2), (7, 9), (16, 4), (13, 5), (40, 25)]                      # c_out x rowlen = 2, 63, 64, 65, 1000
    for i, nchunk in enumerate([1, 15, 16, 63, 64, 65, 129]):
        for j, draw in enumerate(("int", "cont")):
            co, rl = geo[(i + j) % 5]
            lay = dict(c_out=co, rowlen=rl, nchunk=nchunk, adam_w=[1, -1, 1][(i + j) % 3], adam_b=[2, 2, -1][(i + j) % 3],
                       db=not (draw == "int" and i % 2 == 1))       # (db = NULL on exact draws: the gradient Adam saw is then known)
            sizes = [300, co * (rl - 1), co, 1025]                            # unreferred tensors before and after the referred ones
            L.add("reduce_adam", "reduce_adam", "c%dx%d-n%d-w%d-b%d%s-%s" % (co, rl, nchunk, lay["adam_w"], lay["adam_b"],
                                                                            "" if lay["db"] else "-nodb", draw),
                  layers=[lay], sizes=sizes, dyn=(i + j) % 2 == 1, draw=draw, beta1=[0.0, 0.9][i % 2], weight_decay=[10.0, 0.0][j], step=[1, 2, 1000][i % 3])
    for j, draw in enumerate(("int", "cont")):
        lays = [dict(c_out=co, rowlen=rl, nchunk=n, adam_w=aw, adam_b=ab, db=True)
                for (co, rl), n, aw, ab in zip(geo[1:], (129, 1, 16, 65), (1, 3, -1, 6), (2, -1, 5, 7))]
        sizes = [5, 7 * 8, 7, 16 * 3, 0, 13, 40 * 24, 40]
        L.add("reduce_adam", "reduce_adam", "four-layers-%s" % draw, layers=lays, sizes=sizes, dyn=bool(j), draw=draw, beta1=0.9,
              weight_decay=10.0, step=2)
    # reduce only (no tensors at all), and tensors only (no layers: the plain-Adam workgroups alone, 1024 elements each)
    for dyn in (False, True):
        L.add("reduce_adam", "reduce_adam", "tensors-only-%s" % ("dyn" if dyn else "host"), layers=[], sizes=[300, 1024, 1025, 1], dyn=dyn,
              draw="int", beta1=0.9, weight_decay=10.0, step=2)
    L.add("reduce_adam", "reduce_adam", "reduce-only", layers=[dict(c_out=13, rowlen=5, nchunk=17, adam_w=-1, adam_b=-1, db=True)], sizes=[],
          dyn=False, draw="int", beta1=0.0, weight_decay=0.0, step=1)


def _vote(L):
    NV, TV, BV = [1, 3, 10, 24, 63, 64], [1, 15, 16, 17, 40], [1, 63, 64, 65, 200]
    for i in range(30):
        N, T, B = NV[i % 6], TV[i % 5], BV[(i // 2) % 5]
        tb = [0, 7, T - 1][(i // 3) % 3]
        tb = tb if tb < T else T - 1
        L.add("vote", "vote", "t%db%dn%d-from%d%s-%s" % (T, B, N, tb, "-off" if i % 7 == 3 else "", "equal" if i % 10 == 9 else "ties"),
              T=T, B=B, N=N, t_begin=tb, off=int(i % 7 == 3), want_vote=True, draw="equal" if i % 10 == 9 else "ties")
    L.add("vote", "vote", "t17b65n24-from0-off-ties", T=17, B=65, N=24, t_begin=0, off=1, want_vote=True, draw="ties")
    L.add("vote", "vote", "t3b65n65-clout-only", T=3, B=65, N=65, t_begin=0, off=0, want_vote=False, draw="ties")
    L.add("vote", "vote", "t1b300n10-clout-only", T=1, B=300, N=10, t_begin=0, off=0, want_vote=False, draw="ties")


def _free(L):
    rs = np.random.RandomState(20261)
    n = 0
    while n < 60:
        call = GEMM_CALLS[rs.randint(4)]
        many = rs.rand() < 0.2
        rows = int(rs.randint(2049, 2400)) if many else int(rs.randint(1, 300))
        N = int(rs.randint(1, 65))
        mode, sig, off = AUTO, False, 0
        if call == "splitk":
            rows, K = (rows if not many else int(rs.randint(300, 2049))), 256 * int(rs.randint(8, 40))
            K = _fit_k(rows, K)
        elif call == "act":
            K, sig = 32 * int(rs.randint(1, 80 if not many else 4)), bool(rs.randint(2))
        else:
            K = int(rs.randint(1, 130)) if (many or rs.rand() < 0.3) else 32 * int(rs.randint(1, 80))
            mode = int(rs.randint(4)) if call == "mode" else AUTO
            N = N if rs.rand() < 0.9 else int(rs.randint(65, 72))
            off = int(rs.rand() < 0.15)
        draws = ("probe", "cont") if sig else ("grid", "probe", "cont")
        L.gemm("free", call, rows, K, N, mode=mode, sig=sig, off_pv=off, draws=(draws[n % len(draws)],))
        n = sum(1 for c in L.cases if c["stratum"] == "free")
    for i in range(20):
        which = i % 5
        tag = "tail%02d" % i
        if which == 0:
            N1 = int(rs.randint(1, 33))
            N2 = N1 if rs.randint(2) else 0
            rows = int(rs.randint(1, 600))
            L.add("free", "step", tag, rows=rows, K=256 * int(rs.randint(8, 33)), N1=N1, N2=N2, kind=int(rs.randint(2)), clout=True,
                  target=bool(rs.randint(2)), draw=("grid", "cont")[i // 5 % 2])
        elif which == 1:
            L.add("free", "loss", tag, B=int(rs.randint(1, 500)), N=int(rs.randint(1, 65)), kind=int(rs.randint(2)), has_o=bool(rs.randint(2)),
                  want_clout=bool(rs.randint(2)), want_loss=True)
        elif which == 2:
            L.add("free", "adam", tag, sizes=[int(rs.randint(0, 3000)) for _ in range(rs.randint(1, 9))], dyn=bool(rs.randint(2)),
                  beta1=[0.0, 0.9][rs.randint(2)], weight_decay=[0.0, 10.0][rs.randint(2)], step=int(rs.randint(1, 2000)))
        elif which == 3:
            co, rl = int(rs.randint(1, 40)), int(rs.randint(2, 60))
            L.add("free", "reduce_adam", tag, layers=[dict(c_out=co, rowlen=rl, nchunk=int(rs.randint(1, 140)), adam_w=0, adam_b=2, db=True)],
                  sizes=[co * (rl - 1), int(rs.randint(0, 3000)), co], dyn=bool(rs.randint(2)), draw=("int", "cont")[i // 5 % 2],
                  beta1=[0.0, 0.9][rs.randint(2)], weight_decay=[0.0, 10.0][rs.randint(2)], step=int(rs.randint(1, 2000)))
        else:
            T = int(rs.randint(1, 50))
            L.add("free", "vote", tag, T=T, B=int(rs.randint(1, 260)), N=int(rs.randint(1, 65)), t_begin=int(rs.randint(0, T)),
                  off=int(rs.randint(2)), want_vote=True, draw="ties")


def cases():
    L = _List()
    for build in (_variants, _probe_cover, _step_tail, _step_multi, _loss, _adam, _reduce_adam, _vote, _free):
        build(L)
    return L.cases


def describe(c):
    return ", ".join("%s=%s" % (k, c[k]) for k in sorted(c) if k not in ("id", "stratum"))


# ----------------------------------------------------------------------------------------------------------------------
# refusals: every documented error return of these entry points (code, a phrase of dcll_last_error(), no launch, nothing written).
# `what` names the one thing that is wrong with an otherwise servable call; tests/test_gpu_tail_fuzz.py builds the call.
# ----------------------------------------------------------------------------------------------------------------------
_REFUSALS = [
    ("splitk", "K=1024", "DCLL_ERR_UNSUPPORTED", "dcll_readout_splitk: needs"),
    ("splitk", "rows=2049", "DCLL_ERR_UNSUPPORTED", "dcll_readout_splitk: needs"),
    ("splitk", "K=2304+128", "DCLL_ERR_UNSUPPORTED", "dcll_readout_splitk: needs"),
    ("splitk", "N=65", "DCLL_ERR_UNSUPPORTED", "dcll_readout_splitk: needs"),
    ("splitk", "off_pv", "DCLL_ERR_UNSUPPORTED", "dcll_readout_splitk: needs"),
    ("splitk", "off_wt", "DCLL_ERR_UNSUPPORTED", "dcll_readout_splitk: needs"),
    ("splitk", "scratch one float short", "DCLL_ERR_INVALID", "scratch too small"),
    ("act", "K=100", "DCLL_ERR_UNSUPPORTED", "dcll_readout_act: needs"),
    ("act", "N=65", "DCLL_ERR_UNSUPPORTED", "dcll_readout_act: needs"),
    ("act", "off_pv", "DCLL_ERR_UNSUPPORTED", "dcll_readout_act: needs"),
    ("act", "off_wt", "DCLL_ERR_UNSUPPORTED", "dcll_readout_act: needs"),
    ("act", "act=2", "DCLL_ERR_INVALID", "dcll_readout_act: bad argument"),
    ("act", "K=65536 without scratch", "DCLL_ERR_INVALID", "needs scratch"),
    ("act", "K=65536 scratch one float short", "DCLL_ERR_INVALID", "needs scratch"),
    ("mode", "mode=-1", "DCLL_ERR_INVALID", "dcll_readout_mode: bad argument"),
    ("mode", "mode=4", "DCLL_ERR_INVALID", "dcll_readout_mode: bad argument"),
    ("step", "N2!=N1", "DCLL_ERR_INVALID", "dcll_step_readouts: bad argument"),
    ("step", "N1+N2=66", "DCLL_ERR_UNSUPPORTED", "dcll_step_readouts: needs"),
    ("step", "rows=2049", "DCLL_ERR_UNSUPPORTED", "dcll_step_readouts: needs"),
    ("step", "K=65536", "DCLL_ERR_UNSUPPORTED", "dcll_step_readouts: needs"),
    ("step", "target without g_p", "DCLL_ERR_INVALID", "dcll_step_readouts: bad argument"),
    ("step", "kind=7", "DCLL_ERR_UNSUPPORTED", "SmoothL1Loss"),
    ("step", "scratch one float short", "DCLL_ERR_INVALID", "scratch too small"),
    ("multi", "9 items", "DCLL_ERR_INVALID", "1 .. 8 items"),
    ("multi", "shared scratch", "DCLL_ERR_INVALID", "must not share scratch"),
    ("multi", "reserved=1", "DCLL_ERR_INVALID", "reserved must be 0"),
    ("multi", "mixed targets", "DCLL_ERR_INVALID", "either every item has a target or none"),
    ("multi", "empty item", "DCLL_ERR_INVALID", "empty item"),
    ("loss", "kind=7", "DCLL_ERR_UNSUPPORTED", "SmoothL1Loss"),
    ("loss", "o without g_o", "DCLL_ERR_INVALID", "dcll_local_loss_grad: bad argument"),
    ("loss", "B*N=2^24+1", "DCLL_ERR_UNSUPPORTED", "more than 2^24 logits"),
    ("adam", "step=0", "DCLL_ERR_INVALID", "step < 1"),
    ("adam", "null moment", "DCLL_ERR_INVALID", "null tensor"),
    ("adam", "9 tensors", "DCLL_ERR_INVALID", "1..8 tensors"),
    ("adam_dyn", "null dyn", "DCLL_ERR_INVALID", "null dyn"),
    ("reduce_adam", "tensor referred twice", "DCLL_ERR_INVALID", "referred to twice"),
    ("reduce_adam", "index out of range", "DCLL_ERR_INVALID", "out of range"),
    ("reduce_adam", "weight size mismatch", "DCLL_ERR_INVALID", "weight tensor size"),
    ("reduce_adam", "bias size mismatch", "DCLL_ERR_INVALID", "bias tensor size"),
    ("reduce_adam", "rowlen=1", "DCLL_ERR_INVALID", "bad layer entry"),
    ("reduce_adam", "5 layers", "DCLL_ERR_INVALID", "0..4 layers"),
    ("vote", "N=65 with vote", "DCLL_ERR_UNSUPPORTED", "at most 64 classes"),
]


def refusals():
    return [dict(id="%s: %s" % (e, w), entry=e, what=w, code=code, phrase=ph) for e, w, code, ph in _REFUSALS]
