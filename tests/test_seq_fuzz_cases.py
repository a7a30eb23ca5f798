"""CPU self-check of tests/seq_fuzz_cases.py: the case lists of the sequence-ABI differential test are proven here before
tests/test_gpu_seq_fuzz.py lets them judge a kernel.

  - the lists have the promised sizes per stratum and the seed reproduces them exactly (hash of the records);
  - variant() over the lists covers the FULL reachable product of every launcher's switches, the `variants` stratum alone
    already does, one case per key — the coverage claim of the GPU test is checkable without a GPU;
  - the strata hold what they promise (widths, planes, lengths, tile counts, histogram steps, grids, refusals);
  - every case is accepted by the C oracle and has a sound draw within 24 attempts (un-pooled spike share of every step of every
    call strictly between .02 and .98, refractory layers end with a non-zero arp); none is dropped or skipped;
  - the oracle's work stays below the caps."""
import collections

import numpy as np
import pytest

import seq_fuzz_cases as SF

CASES = SF.cases()
REFUSE = SF.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)

# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "79450b9f8c0a76f1fa1ece3bdd259acb1f763580b23293a4ceed00ba3b423e86"
REFUSE_HASH = "2b00e2fa5921119856ba8683484aa256feb60c25748e9ace34825b5d6601135b"


def test_lists_have_the_promised_sizes():
    assert {k: len(v) for k, v in BY.items()} == dict(variants=208, boundaries=70, carry=24, inputs=20, grids=12, free=100)
    assert len(CASES) == 434 and len(REFUSE) == 26
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert c["B"] >= 1 and 1 <= c["B_checked"] <= c["B"] and all(T >= 1 for T in c["Ts"]), c["id"]
        assert c["B_checked"] == c["B"] or (c["stratum"] == "grids" and c["B_checked"] <= 8), c["id"]
        assert c["lowhigh_iter0"] is None or c["want_pv"], c["id"]             # (the statistics need the pv output)
        assert not (c["n_ro"] and c["presigmoid"]), c["id"]
    assert all(SF.by_id(c["id"]) == c for c in CASES[::40] + REFUSE[::9])


def test_the_seed_reproduces_the_lists_exactly():
    assert SF.cases_hash(SF.cases()) == SF.cases_hash(CASES) == CASES_HASH
    assert SF.cases_hash(SF.refusals()) == REFUSE_HASH
    assert SF.cases_hash(SF.cases(SF.SEED + 1)) != CASES_HASH


def test_variants_cover_the_full_reachable_product_of_every_launcher():
    reach = SF.reachable_variants()
    assert len(reach) == len(set(reach)) == 120 + 12 + 24 + 8 + 8 + 8 + 12 + 12 + 4
    var = collections.Counter(SF.variant(c, T) for c in BY["variants"] for T in c["Ts"])
    assert set(var) == set(reach) and all(n == 1 for n in var.values())         # one case per key, every key
    every = collections.Counter(SF.variant(c, T) for c in CASES for T in c["Ts"])
    assert set(every) == set(reach)                                             # (nothing outside the restated product)
    # every key also by a case that does not come from the variants stratum's own constructor: >= 2 for most
    print("variant keys served by one case only:", sorted(k for k, n in every.items() if n == 1))


def test_the_variants_stratum_holds_what_it_promises():
    var = BY["variants"]
    w3 = [c for c in var if SF.launcher(c) == "w3"]
    assert {c["w"] for c in w3 if c["w"] >= 32} == {32, 64, 128, 256}                          # the LW = 5 widths, c_in 64
    assert any((c["h"] * c["w"]) % 64 != 0 and not c["want_spikes"] for c in w3)
    assert all((c["h"] * c["w"]) % 64 == 0 for c in w3 if c["want_spikes"]) and all((c["h"] * c["w"]) % 32 == 0 for c in w3)
    w3f = [c for c in var if SF.launcher(c) == "w3f"]
    assert any(c["h"] * c["w"] == 128 for c in w3f) and any(c["w"] == 256 for c in w3f)
    assert all((c["h"] * c["w"]) % 128 == 0 for c in CASES if SF.launcher(c) == "w3f")
    c1 = [c for c in CASES if SF.launcher(c) in ("c1", "c1t")]
    assert all(1 <= c["c_out"] <= 32 for c in c1) and len({c["c_out"] for c in c1}) >= 12
    assert all(c["c_out"] == 32 for c in c1 if SF.variant(c, 1)[2] in (1, 2))                   # the fast epilogue
    ro = [c for c in var if c["n_ro"]]
    assert any(c["Ts"][0] >= 8 for c in ro) and any(c["q8"] for c in ro) and {SF.variant(c, 1)[2] for c in ro} == {0, 1, 2, 3}
    for c in CASES:
        if c["entry"] == "iq":                      # a non-zero t0, L > t0 + T, a tail mask that marks some samples
            T, _ = SF.run(c)
            assert c["t0"] > 0 and T["iq"].shape[2] > c["t0"] + sum(c["Ts"])
            m = T["tab"]["mask"]
            assert m.any() and (c["B_checked"] == 1 or not m.all())
            assert not np.array_equal(T["tab"]["thr_i"], T["tab"]["thr_i_tail"])


def test_the_boundaries_hold_what_they_promise():
    edge = BY["boundaries"]
    Ts = sorted(c["Ts"][0] for c in edge if c["id"].startswith("seq-edge-c32-T"))
    assert Ts == [1, 2, 7, 8, 9, 10, 15, 16, 17, 33, 127, 128]
    for c in edge:
        if c["id"].startswith("seq-edge-c32-T"):
            T = c["Ts"][0]
            want = "k_lif_seq_c32" if T < 8 else "k_lif_seq_c32d" if T % 2 == 0 else "k_lif_seq_c32rp"
            assert SF.expected_kernels(c, T) == [want]
    for L in ("c32t", "c1t"):
        tiles = {(c["h"] // 8, c["w"] // 32) for c in edge if SF.launcher(c) == L}
        assert {(1, 1), (1, 2), (1, 3), (2, 1), (3, 1), (2, 2), (3, 3), (16, 4)} <= tiles
        big = [c for c in edge if SF.launcher(c) == L and (c["h"], c["w"]) == (128, 128)]
        assert big and all(c["B"] == 1 and max(c["Ts"]) <= 3 for c in big)
    ntile = {c["B"] * c["h"] * c["w"] // 32 for c in edge if SF.launcher(c) == "w3"}
    assert {7, 8, 9, 15, 16, 17, 24} <= ntile
    dense = [c for c in edge if c["entry"] == "dense"]
    assert {c["in_features"] for c in dense} == {63, 64, 65, 1023, 1024, 1025}
    assert {c["out_features"] for c in dense} == {127, 128, 129} and {c["B"] for c in dense} == {31, 32, 33, 65}
    assert {c["tau_tensor"] for c in dense} == {0, 1}
    assert {SF.variant(c, 1)[0] for c in dense} == {"k_dense_lif_seq", "k_dense_lif_mfma"}
    # 0, 1 and 2 histogram steps in a call; one on the call's first step, one on its last
    lh = [(c, SF.hist_steps(c["lowhigh_iter0"], c["Ts"][0])) for c in edge if c["lowhigh_iter0"] is not None]
    assert {len(s) for _, s in lh} == {0, 1, 2}
    assert any(s and s[0] == 0 for _, s in lh) and any(s and s[-1] == c["Ts"][0] - 1 for c, s in lh)
    assert {SF.launcher(c) for c, _ in lh} == {"c32", "c32t", "c1", "c1t", "w3", "w3f"}
    assert any(c["presigmoid"] for c, s in lh if s)
    for c, s in lh:
        assert ("k_pv_lowhigh" in SF.expected_kernels(c, c["Ts"][0], c["lowhigh_iter0"])) == bool(s)


def test_carry_inputs_grids_and_free_hold_what_they_promise():
    carry = BY["carry"]
    assert all(2 <= len(c["Ts"]) <= 3 for c in carry)
    fams = {SF.variant(c, T)[0] for c in carry for T in c["Ts"]}
    assert fams == {"k_lif_seq_c32", "k_lif_seq_c32d", "k_lif_seq_c32rp", "k_lif_seq_c32t", "k_lif_seq_c1", "k_lif_seq_c1t", "k_lif_seq_w3",
                    "k_lif_seq_w3f", "k_dense_lif_seq", "k_dense_lif_mfma"}
    orders = {tuple(SF.variant(c, T)[0][10:] for T in c["Ts"]) for c in carry if SF.launcher(c) == "c32" and not c["n_ro"]}
    assert ("c32", "c32d", "c32rp") in orders and ("c32rp", "c32d", "c32") in orders
    assert {c["refractory"] for c in carry} == {0, 1}
    inputs = BY["inputs"]
    assert {SF.launcher(c) for c in inputs} == {"c32", "c32t", "w3", "c1", "c1t", "w3f"}
    for c in inputs:
        kinds = SF.patterns(c)
        assert c["B"] > len(kinds) - 2 and ("zeros" in kinds[:c["B"]] or c["c_in"] == 1), c["id"]
        if c["c_in"] == 1:
            s = SF.seam_cells(c)
            assert 0 in s and c["h"] * c["w"] - 1 in s
            if SF.launcher(c) == "c1t":
                assert {7 * c["w"] + 31, 7 * c["w"] + 32, 8 * c["w"] + 31, 8 * c["w"] + 32, 7 * c["w"] + 29, 8 * c["w"] + 34} <= set(s)
    grids = BY["grids"]
    assert {SF.launcher(c) for c in grids} == {"c32", "c32t", "c1", "c1t", "w3", "w3f", "dense"}
    assert {SF.variant(c, c["Ts"][0])[0] for c in grids} >= {"k_lif_seq_c32", "k_lif_seq_c32d", "k_lif_seq_c32rp", "k_dense_lif_mfma"}
    assert all(c["B"] >= 700 and c["B_checked"] == 8 for c in grids)
    free = BY["free"]
    assert {SF.launcher(c) for c in free} == {"c32", "c32t", "c1", "c1t", "w3", "w3f", "dense"}
    assert all(1 <= c["B"] <= 70 for c in free) and max(c["B"] for c in free) > 32
    for key in ("refractory", "q8", "presigmoid", "want_spikes", "want_pv", "want_v", "state0"):
        assert {c[key] for c in free if c["entry"] != "dense"} == {0, 1}, key
    assert {c["entry"] for c in free} == {"seq", "cells", "iq", "dense"} and any(c["n_ro"] for c in free)
    assert any(c["lowhigh_iter0"] is not None for c in free) and {len(c["Ts"]) for c in free} == {1, 2, 3}


def test_refusals_are_what_the_issue_lists():
    by = {c["id"][len("seq-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported == {"c32-cout16", "cells-cout33", "plane-24x24", "plane-12x32", "plane-16x48", "k5-pad2", "pool2", "stride2", "groups2",
                           "w3-w512", "w3-w48", "nro10", "nro24-32x32", "nro24-w3", "w3-spikes-hw96", "w3f-hw64"}
    assert invalid == {"presig-nro", "c32t-no-scratch", "c1t-no-scratch", "no-arp", "cells-no-arp", "w3f-misaligned", "q8-no-scale"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"T0", "B0", "w3-T0"}
    assert all(c["phrase"] for c in REFUSE if c["code"] != "DCLL_OK")


def test_the_oracle_work_stays_below_the_caps():
    per = [SF.work(c) for c in CASES]
    print("oracle work: total %.3g multiply-adds, largest case %.3g (%s)" % (sum(per), max(per), CASES[int(np.argmax(per))]["id"]))
    for st, cs in BY.items():
        print("  %-10s %.3g" % (st, sum(SF.work(c) for c in cs)))
    assert max(per) <= SF.WORK_CASE_MAX == 3e9
    assert sum(per) <= SF.WORK_TOTAL_MAX == 6e10
    assert all(SF.work(c) <= SF.WORK_FREE_MAX for c in BY["free"])


def test_iq_cells_is_the_threshold_count():
    """iq_cells (numpy searchsorted) == the definition dcll_iq_encode states: cell = #{j : x >= thr[j]} per axis, q * w + i, with
    the tail tables for the marked samples — incl. values exactly on a threshold, where the two tables disagree."""
    c = SF.by_id("seq-var-c1t-R1-F0-iq")
    T, _ = SF.run(c)
    tab, iq = T["tab"], T["iq"]
    n = sum(c["Ts"])
    got = SF.iq_cells(tab, iq, c["t0"], n, c["w"])
    differ = 0
    for b in range(c["B_checked"]):
        for t in range(n):
            cell = {}
            for name, (ti, tq) in (("main", (tab["thr_i"], tab["thr_q"])), ("tail", (tab["thr_i_tail"], tab["thr_q_tail"]))):
                ci = sum(int(iq[b, 0, c["t0"] + t] >= x) for x in ti)
                cq = sum(int(iq[b, 1, c["t0"] + t] >= x) for x in tq)
                cell[name] = cq * c["w"] + ci
            assert got[t, b] == cell["tail" if tab["mask"][b] else "main"]
            differ += cell["main"] != cell["tail"]
    assert differ > 0, "no value on a threshold: the tail tables would not show"
    assert np.array_equal(np.concatenate([call["cells"] for call in T["calls"]]), got)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_sound(case):
    c = case
    T, traj = SF.run(c)                         # (asserts: accepted by the oracle, its shapes, a sound draw within 24 attempts)
    assert SF.unsound(c, traj) is None, SF.describe(c)
    assert len(traj) == len(c["Ts"]) == len(T["calls"])
    for T_, call in zip(c["Ts"], traj):
        share = (call["v"] > 0).reshape(T_, -1).mean(axis=1)
        assert share.shape == (T_,) and (share > .02).all() and (share < .98).all(), share
    if c["refractory"]:
        assert np.any(traj[-1]["arp"])
    if c["q8"]:
        q, scale = T["q8"]
        assert q.dtype == np.int8 and np.array_equal(T["W"], q.astype(np.float32) * scale.reshape(-1, 1, 1, 1))
    if c["entry"] != "dense" and c["c_in"] == 1:        # exactly one spike per sample and step, at the cell index
        for call in T["calls"]:
            x = call["x"].reshape(call["x"].shape[0], c["B_checked"], -1)
            assert np.array_equal(x.sum(-1), np.ones(x.shape[:2])) and np.array_equal(x.argmax(-1), call["cells"])
    for k, T_ in enumerate(c["Ts"]):
        names = SF.expected_kernels(c, T_, None if c["lowhigh_iter0"] is None else c["lowhigh_iter0"] + sum(c["Ts"][:k]))
        assert names[0].startswith(SF.variant(c, T_)[0]) or names[0] == "k_trace"


def test_presigmoid_without_pv_is_in_the_list_for_every_launcher():
    """pv_presigmoid with pv not wanted and v wanted (k_lif_seq_c1 / _c1t lost v_out there: seq-free-087, seq-edge-presig-nopv-*)"""
    got = {SF.launcher(c) for c in BY["boundaries"] if c["presigmoid"] and not c["want_pv"] and c["want_v"]}
    assert got == {"c32", "c32t", "c1", "c1t", "w3", "w3f"}
    assert {c["entry"] for c in BY["boundaries"] if c["presigmoid"] and not c["want_pv"] and SF.launcher(c) in ("c1", "c1t")} == {"cells", "iq"}
