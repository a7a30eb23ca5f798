"""CPU proof of tests/value_cases.py: the list means what it says, and each kind would catch the fault it is aimed at — before
tests/test_gpu_values.py lets it judge the kernels.  Mutants run through the C oracle or a few lines of numpy, never through
device code.

  - the process and the oracle's OpenMP threads keep fp32 subnormals (asserted once; every other test here depends on it);
  - the seed reproduces the list; geometry is the sibling case's, B <= 3, T <= 12, <= 3 calls, <= 8 steps; every family has a case
    of every kind that applies to it, int8 weights and pv_presigmoid on every sequence launcher that takes them, and a predicted
    launch log;
  - decay / mixed: >= 10 % of the final state is subnormal and not zero; an element crosses from normal to subnormal, one from
    subnormal to exactly 0, one sticks at 2^-149;
  - threshold: the table values occur as un-pooled v bit for bit (a refractory layer: all of them, capped at 2^126; a plain layer:
    TABLE[co % n], one per output channel), a pooling window at +-0 does not spike, one at 2^-149 does;
  - mutants: (a) flush-to-zero of state and x changes state and spikes of every decay case and the state of every mixed case,
    (b) s = v >= 0 the spikes of every threshold case, (c) the single-clamp spike min(1, max(0, v 2^127)) the arp of every
    refractory threshold case, (d) x != 0 ? tau_s : 0 the traces of every analog case, (e) the naive fp32 sigmoid e^v / (1 + e^v)
    is NaN on the table;
  - no sigmoid(TABLE) lies within 1e-3 of an INNER edge of the 19 histogram bins (the counters of dcll_pv_lowhigh are pv < edge 1
    and pv >= edge 18; the outer edges 0 and 1 are the values a saturated sigmoid is meant to reach)."""
import collections
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import value_cases as V

CASES = V.cases()
BY_KIND = collections.defaultdict(list)
for _c in CASES:
    BY_KIND[_c["kind"]].append(_c)
MIN_NORMAL = np.float32(2.0 ** -126)
CASES_HASH = "1dcc6f0eed05801e037f8d6afd017774038133b9bea3e1ffc76fb685724f52ee"


def _ids(cs):
    return [c["id"] for c in cs]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _subnormal(a):
    return (a != 0) & (np.abs(a) < MIN_NORMAL)


@pytest.fixture(scope="module", autouse=True)
def subnormals_are_kept():
    """numpy in this process and the C oracle's worker threads run with flush-to-zero off: without that every reference in this
    file and in test_gpu_values.py would itself flush, and the comparisons would prove nothing"""
    from oracle import c_oracle as C
    assert np.float32(2.0 ** -149) * np.float32(1) != 0, "this process flushes fp32 subnormals: the value cases cannot be judged here"
    n = 64
    sd = {"i2h.weight": np.ones((n, n), np.float32), "i2h.alpha": np.float32([.97]), "i2h.tau_m__dt": np.float32([33]),
          "i2h.alphas": np.float32([.97]), "i2h.tau_s__dt": np.float32([33]), "i2o.weight": np.zeros((1, n), np.float32),
          "i2o.bias": np.zeros(1, np.float32)}
    orc = C.OracleDenseLayer(sd, 0.0)
    orc.state = [np.full((n, n), V.TINY, np.float32), np.full((n, n), V.TINY, np.float32), np.zeros((n, n), np.float32)]
    v = orc.forward(np.zeros((n, n), np.float32))[3]
    assert (orc.state[0] == V.TINY).all() and _subnormal(orc.state[1]).all() and _subnormal(v).all(), \
        "the C oracle flushes fp32 subnormals (on some thread): the value cases cannot be judged here"


def test_the_seed_reproduces_the_list():
    assert V.cases_hash(V.cases()) == V.cases_hash(CASES) == CASES_HASH
    assert V.cases_hash(V.cases(V.SEED + 1)) != CASES_HASH
    ids = _ids(CASES)
    assert len(set(ids)) == len(ids) and all(V.by_id(c["id"]) == c for c in CASES[::15])


GEOMETRY_KEYS = ("c_in", "c_out", "h", "w", "kh", "kw", "pad_h", "pad_w", "pool_h", "pool_w", "stride", "dilation", "groups", "layer",
                 "entry", "in_features", "out_features", "tau_tensor", "want_spikes", "want_pv", "presigmoid", "n_ro", "t0", "misalign")


def test_geometry_is_the_siblings_and_the_sizes_are_small():
    for c in CASES:
        src = V.SRC[c["src"]].by_id(c["source"])
        assert all(c[k] == src[k] for k in GEOMETRY_KEYS if k in src), c["id"]
        g = V.geometry(c)
        assert g["B"] <= V.MAX_B and max(g["Ts"]) <= V.MAX_T, c["id"]
        assert len(g["Ts"]) <= (V.MAX_STEPS if "steps" in c else V.MAX_CALLS), c["id"]
        assert c["alpharp"] == (.5 if c["kind"] == "threshold" and c["refractory"] else V.FZ.ALPHARP)


def test_every_family_has_every_kind_that_applies():
    assert len(set(V.families())) == len(V.families()) == 40
    for fam in V.families():
        cs = [c for c in CASES if c["family"] == fam]
        kinds = {(c["kind"], c["refractory"]) for c in cs}
        want = {("decay", 0), ("decay", 1), ("threshold", 0), ("threshold", 1)}
        if "presigmoid" not in fam:
            want |= {("mixed", 1)} | ({("analog", 0)} if V.float_input(cs[0]) else set())
        assert kinds == want, (fam, kinds)
        assert all(bool(c.get("presigmoid")) == ("presigmoid" in fam) for c in cs)
        if cs[0]["src"] == "seq" and cs[0]["entry"] != "dense":            # int8 weights on one case of every sequence launcher
            assert sum(c["q8"] for c in cs) == 1
    kernels = {V.SF.variant(c, c["Ts"][0])[0] for c in CASES if c["src"] == "seq"}
    assert kernels == {"k_lif_seq_c32", "k_lif_seq_c32d", "k_lif_seq_c32rp", "k_lif_seq_c32t", "k_lif_seq_c1", "k_lif_seq_c1t",
                       "k_lif_seq_w3", "k_lif_seq_w3f", "k_dense_lif_seq"}
    for k in kernels - {"k_dense_lif_seq"}:
        mine = [c for c in CASES if c["src"] == "seq" and V.SF.variant(c, c["Ts"][0])[0] == k]
        assert any(c["presigmoid"] for c in mine) and any(c["q8"] for c in mine), k
        if k in ("k_lif_seq_c1", "k_lif_seq_c1t"):
            assert {c["entry"] for c in mine} == {"cells", "iq"}
    assert {V.SA.form(c, c["B_run"]) for c in CASES if c["src"] == "step-any"} == set(V.SA.all_forms())
    assert {V.S3.form(c, c["B_run"]) for c in CASES if c["src"] == "step-w3"} == set(V.S3.all_forms())
    assert {V.A.variant(c) for c in CASES if c["src"] == "seq-any"} == set(V.A.all_variants())
    assert {V.WD.variant(c) for c in CASES if c["src"] == "seq-wide"} == set(V.WD.all_variants())


def test_every_case_predicts_its_launch_log():
    for c in CASES:
        logs = [V.expected_log(c, T) for T in V.geometry(c)["Ts"]]
        assert all(logs) or (c["names"] and all(l is None for l in logs)), c["id"]
        if c["src"] not in ("fuzz", "fuzz-dense"):
            kernel = c["family"].split(" ")[0]
            assert all(any(n.startswith(kernel) for n in l) for l in logs), (c["id"], logs)


# ---------------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------------
def _final(c, traj, D):
    e0, e1, _ = V.final_state(c, traj)
    return e0.reshape(D["eps0"].shape), e1.reshape(D["eps1"].shape)


@pytest.mark.parametrize("case", BY_KIND["decay"] + BY_KIND["mixed"], ids=_ids(BY_KIND["decay"] + BY_KIND["mixed"]))
def test_subnormal_state_and_its_three_crossings(case):
    c = case
    T, traj, D = V.run(c)
    f0, f1 = _final(c, traj, D)
    share = float(np.concatenate([_subnormal(f0).ravel(), _subnormal(f1).ravel()]).mean())
    print("%s: subnormal share of the final eps0 / eps1 %.3f" % (c["id"], share))
    assert share >= .10
    down, zero, stuck = V.crossings(c, D, traj)
    print("normal -> subnormal %d, subnormal -> 0 %d, stuck at 2^-149 %d (draw %d)" % (down, zero, stuck, D["attempt"]))
    assert down > 0 and zero > 0 and stuck > 0
    assert all(np.isfinite(s["v"]).all() for s in V.flat_steps(c, traj))


def _pooled_v(c, v):
    g = V.geometry(c)
    if (g["ch"], g["cw"]) == (g["ph"], g["pw"]):
        return v
    pool = (g["ch"] // g["ph"], g["cw"] // g["pw"]) if c["src"] == "seq" else (c["pool_h"], c["pool_w"])
    out = F.max_pool2d(torch.from_numpy(v), pool, pool, ((pool[0] - 1) // 2, (pool[1] - 1) // 2)).numpy()
    assert out.shape[2:] == (g["ph"], g["pw"])
    return out


def _expected_table(c):
    return V.TABLE_CAPPED if c["refractory"] else V.TABLE[np.arange(min(V.geometry(c)["cout"], len(V.TABLE)))]


@pytest.mark.parametrize("case", BY_KIND["threshold"], ids=_ids(BY_KIND["threshold"]))
def test_membranes_sit_on_the_table(case):
    c = case
    T, traj, D = V.run(c)
    first = V.flat_steps(c, traj)[0]
    v, s = first["v"], first["s"]
    want = set(_bits(_expected_table(c)).tolist())
    got = set(_bits(v).ravel().tolist())
    assert got == want if c["refractory"] else want <= got, (c["id"], sorted(want - got), len(got))
    assert len(want) >= 5 and {0, 1} <= want          # (the bit patterns of +0 and of 2^-149)
    if c["refractory"]:
        assert len(want) == len(V.TABLE) - 2          # (+-FLT_MAX are capped onto +-2^126)
    pv = _pooled_v(c, v)
    assert pv.shape == s.shape
    assert ((pv == 0) & (s == 0)).any() and not ((pv == 0) & (s != 0)).any(), "v == 0 must not spike"
    assert ((pv == V.TINY) & (s == 1)).any() and not ((pv == V.TINY) & (s != 1)).any(), "v == 2^-149 must spike"
    if pv.shape != v.shape:            # ties inside pooling windows: +0 with -0, and equal values
        a, b = v[..., :-1], v[..., 1:]            # (every pooling layer of the list pools along x)
        assert V.geometry(c)["pool"][1] >= 2 and ((a == b) & (a != 0)).any()
        if c["refractory"]:
            assert ((a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))).any()
    assert all(np.isfinite(st["v"]).all() for st in V.flat_steps(c, traj))


# ---------------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------------
def _flushed_inputs(c, T):
    T2 = copy.copy(T)
    if "x" in T:
        T2["x"] = [V.flush(x.copy()) for x in T["x"]]
    else:
        T2["calls"] = [dict(call, x=V.flush(call["x"].copy())) for call in T["calls"]]
    return T2


@pytest.mark.parametrize("case", BY_KIND["decay"] + BY_KIND["mixed"], ids=_ids(BY_KIND["decay"] + BY_KIND["mixed"]))
def test_mutant_a_flush_to_zero_is_caught(case):
    c = case
    T, traj, D = V.run(c)
    mut = V.trajectory(c, _flushed_inputs(c, T), before_step=lambda state: [V.flush(a) for a in state])
    state_differs = any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(V.final_state(c, traj), V.final_state(c, mut)))
    flips = sum(int((a["s"] != b["s"]).sum()) for a, b in zip(V.flat_steps(c, traj), V.flat_steps(c, mut)))
    print("%s: %d spikes differ under flush-to-zero" % (c["id"], flips))
    assert state_differs
    if c["kind"] == "decay":
        assert flips > 0


@pytest.mark.parametrize("case", BY_KIND["threshold"], ids=_ids(BY_KIND["threshold"]))
def test_mutants_b_and_c_wrong_thresholds_are_caught(case):
    c = case
    T, traj, D = V.run(c)
    first = V.flat_steps(c, traj)[0]
    v, s = first["v"], first["s"]
    assert ((_pooled_v(c, v) >= 0).astype(np.float32) != s).any(), "(b) s = v >= 0 leaves the spikes unchanged"
    if c["refractory"]:
        a = (np.float32(c["alpharp"]) * D["arp"]).astype(np.float32)
        a = a.reshape(v.shape)
        unsigned = lambda t: _bits(np.where(t == 0, np.float32(0), t))
        assert np.array_equal(unsigned(v), unsigned(a)), "the construction: v = alpharp * arp at the first step, up to a zero's sign"
        with np.errstate(over="ignore"):
            one_clamp = np.minimum(np.float32(1), np.maximum(np.float32(0), v * np.float32(2.0 ** 127))).astype(np.float32)
        arp_true = (a - (v > 0).astype(np.float32)).astype(np.float32)
        arp_mut = (a - one_clamp).astype(np.float32)
        if "steps" in c:
            assert np.array_equal(_bits(arp_true), _bits(traj[0]["arp"].reshape(v.shape))), "the restated arp update"
        assert (arp_true != arp_mut).any(), "(c) the single clamp leaves arp unchanged"
        assert (v == V.TINY).any() and (one_clamp[v == V.TINY] == np.float32(2.0 ** -22)).all()      # (what spike01_pk's second clamp is for)


@pytest.mark.parametrize("case", BY_KIND["analog"], ids=_ids(BY_KIND["analog"]))
def test_mutant_d_input_taken_as_a_flag_is_caught(case):
    c = case
    T, traj, D = V.run(c)
    x = D["calls"][0]["x"][0]
    alphas, tau_s = D["tau"][2], D["tau"][3]
    keep = (alphas * D["eps0"]).astype(np.float32)
    true = ((x * tau_s).astype(np.float32) + keep).astype(np.float32)
    mut = (np.where(x != 0, tau_s, np.float32(0)).astype(np.float32) + keep).astype(np.float32)
    if "steps" in c:
        assert np.array_equal(_bits(true), _bits(traj[0]["eps0"].reshape(true.shape))), "the restated trace update"
    assert (true != mut).mean() > .5
    vals = set(_bits(np.concatenate([call["x"].ravel() for call in D["calls"]])).tolist())
    assert set(_bits(V.ANALOG_TABLE).tolist()) <= vals and len(vals) > 100
    assert all(np.isfinite(st["v"]).all() for st in V.flat_steps(c, traj))


def test_mutant_e_the_naive_sigmoid_is_nan_on_the_table():
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(V.TABLE)
        naive = e / (np.float32(1) + e)
        good = np.float32(1) / (np.float32(1) + np.exp(-V.TABLE))
    assert naive.dtype == np.float32 and np.isnan(naive).any() and np.isfinite(good).all()
    assert ((good >= 0) & (good <= 1)).all() and good.min() == 0 and good.max() == 1


def test_no_table_value_sits_on_a_histogram_edge():
    with np.errstate(over="ignore"):
        pv = 1.0 / (1.0 + np.exp(-V.TABLE.astype(np.float64)))
    inner = np.linspace(0, 1, 20)[1:-1]
    assert np.abs(pv[:, None] - inner[None, :]).min() > 1e-3
    assert (pv < inner[0]).sum() == 7 and (pv >= inner[-1]).sum() == 7          # +-17 and beyond: the two counted bins
