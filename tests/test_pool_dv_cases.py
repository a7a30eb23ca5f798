"""CPU proof of tests/pool_dv_cases.py: the list covers what tests/test_gpu_pool_dv.py claims to run, the restated geometry is
torch's MaxPool2d, the float32 restatement of k_bwd_dv's formula stays inside the tolerance against float64 autograd, and the mutants
of the restatement that a wrong kernel would be are each caught by some case."""
import collections

import numpy as np
import torch

import fuzz_cases as FZ
import pool_dv_cases as C

CASES = C.cases()


def test_the_list_is_stable_and_small():
    assert len({c["id"] for c in CASES}) == len(CASES)
    assert C.cases_hash(CASES) == C.cases_hash(C.cases())
    for c in CASES:
        ch, cw, _, _ = C.shape(c)
        big = C.per_block(c) == C.PER_BLOCK or ch >= 100                      # (the launcher's other path needs 512 workgroups)
        assert c["B"] * c["c_out"] * ch * cw <= (6e6 if big else 1e5), c["id"]    # a single small call
    assert sum(C.shape(c)[0] >= 100 for c in CASES) == 3
    print(len(CASES), "cases")


def test_every_instance_path_and_parameter_is_covered():
    served = [c for c in CASES if C.served(c)]
    assert {C.instance_key(c) for c in served} == set(C.all_instances())
    assert {C.form_name(c) for c in CASES} == {"k_bwd_dv_pool", "k_bwd_dv"}
    assert any(c["target"] == 33 and not C.served(c) for c in CASES)
    assert {(C.per_block(c), C.in_flight(c)) for c in served} == {(C.PER_BLOCK, 4), (C.PER_BLOCK, 2), (4, 4), (2, 2)}
    assert any(C.grid(c)[0] * -(-c["B"] // C.PER_BLOCK) == C.MIN_WG for c in served)            # (on the threshold)
    assert any(C.MIN_WG // 2 <= C.grid(c)[0] * -(-c["B"] // C.PER_BLOCK) < C.MIN_WG for c in served)
    planes = collections.defaultdict(set)
    for c in CASES:
        planes[(c["pool_h"], c["pool_w"])].add(C.shape(c)[:2])
    want = {(2, 2): [(2, 2), (3, 3), (5, 4), (9, 9), (26, 26)], (1, 2): [(1, 2), (4, 7), (2, 16)], (2, 1): [(7, 1), (6, 5)],
            (3, 3): [(3, 3), (4, 4), (6, 9), (7, 8)]}
    for p in ((1, 3), (3, 1), (2, 3), (3, 2)):
        want[p] = [(5, 6), (6, 5)]
    for p, hw in want.items():
        assert set(hw) <= planes[p], (p, set(hw) - planes[p])
    assert {1, 3, 16, 33} <= {c["c_out"] for c in CASES}
    Ks = {C.K(c) for c in served}
    assert {C.WINDOWS - 1, C.WINDOWS, C.WINDOWS + 1, 2 * C.WINDOWS - 1, 2 * C.WINDOWS, 2 * C.WINDOWS + 1} <= Ks, sorted(Ks)
    assert set(C.BATCHES) <= {c["B"] for c in served} and set(C.TARGETS) <= {c["target"] for c in CASES}
    assert {(c["gsel"], c["with_gv"]) for c in served} >= {(g, v) for g in C.GSEL for v in (0, 1)}
    offs = {c["off"] for c in served}
    assert {0, C.OFF_V, C.OFF_SCRATCH, C.OFF_GV, C.OFF_GPV, C.OFF_W, 31} <= offs
    assert {c["draw"] for c in served} == set(C.DRAWS) | {"negzero"}
    assert {c["path"] for c in served} == set(C.PATHS)
    assert any(c["path"] == "bands" and c["bands"] >= 2 for c in served) and any(c["path"] == "bands" and c["bands"] == 0 for c in served)
    assert any(c["kh"] == 7 and C.shape(c)[:2] == (26, 26) for c in served) and any(c["kh"] == 7 and C.shape(c)[:2] == (9, 9) for c in served)
    assert any((c["kh"], c["kw"], c["c_out"], c["h"] * c["w"]) == (1, 3, 64, 32) and (c["pool_h"], c["pool_w"]) == (1, 2) for c in served)


def test_the_restated_shape_and_winner_are_torchs():
    for c in CASES:
        assert C.shape(c) == FZ.conv_shape(c), c["id"]
        T = C.draw(c)
        ch, cw, ph, pw = C.shape(c)
        assert T["v"].shape == (c["B"], c["c_out"], ch, cw) and not np.isnan(T["v"]).any()
        pv = C.sigmoid32(T["v"])
        pool = (c["pool_h"], c["pool_w"])
        _, idx = torch.nn.functional.max_pool2d(torch.from_numpy(pv), pool, pool, ((pool[0] - 1) // 2, (pool[1] - 1) // 2),
                                                return_indices=True)
        assert idx.shape[2:] == (ph, pw) and np.array_equal(idx.numpy(), C.winner(c, pv)), c["id"]


def test_every_grid_case_has_an_exact_tie_for_the_maximum():
    n = 0
    for c in CASES:
        if c["draw"] != "grid":
            continue
        pv = C.sigmoid32(C.draw(c)["v"])
        first, last = C.winner(c, pv), C.winner(c, pv, tie_last=True)
        assert (first != last).any(), c["id"]
        n += 1
    assert n >= 10


def test_uncovered_and_clipped_geometries_carry_g_v_there():
    """every geometry with elements in no window, or with a clipped window, has a case with a non-zero g_v on such an element (an
    uncovered one where there is one, else an element of a clipped window)"""
    need, have = set(), set()
    for c in CASES:
        cov, clipped = C.coverage(c)
        geo = (c["pool_h"], c["pool_w"]) + C.shape(c)[:2]
        if (cov.all() and not clipped) or C.shape(c)[0] >= 100:        # (the three large planes: the same geometry classes as 6x6 / 8x8)
            continue
        need.add(geo)
        T = C.draw(c)
        if T["g_v"] is None or not C.served(c):
            continue
        if not cov.all():
            ok = bool((T["g_v"][:, :, ~cov] != 0).any())
        else:
            ok = bool((T["g_v"][:, :, 0, :] != 0).any() or (T["g_v"][:, :, :, 0] != 0).any())
        if ok:
            have.add(geo)
    assert need and need == have, need - have


def test_the_float32_restatement_is_inside_the_tolerance_against_float64():
    worst = -np.inf
    for c in CASES:
        if c["draw"] != "grid":
            continue
        ref = C.reference(c["id"]).numpy()
        got = C.dv_restated(c, C.draw(c)).astype(np.float64)
        scale = float(np.abs(ref).max())
        excess = float((np.abs(got - ref) - C.DV_RTOL * np.abs(ref) - C.DV_ATOL * scale).max())
        worst = max(worst, excess)
        np.testing.assert_allclose(got, ref, rtol=C.DV_RTOL, atol=C.DV_ATOL * scale + 1e-30, err_msg=c["id"])
    print("worst excess over rtol %g |ref| + atol %g max|ref|: %.3g (negative: inside)" % (C.DV_RTOL, C.DV_ATOL, worst))
    assert worst <= 0


def _bits(a):
    return a.astype(np.float32).view(np.uint32)


def test_every_mutant_of_the_restatement_is_caught():
    killed = collections.Counter()
    for c in CASES:
        if not C.served(c):
            continue
        T = C.draw(c)
        good = C.dv_restated(c, T)
        muts = dict(tie_last=dict(tie_last=True), uncovered=dict(skip_uncovered=True), padding=dict(plus0_pad=True))
        if c["draw"] == "wide":
            muts["over_v"] = dict(over_v=True)
        if 3 in (c["pool_h"], c["pool_w"]):
            muts["clip"] = dict(no_clip_first=True)
        for name, kw in muts.items():
            if not np.array_equal(_bits(C.dv_restated(c, T, **kw)), _bits(good)):
                killed[name] += 1
    print(dict(killed))
    assert set(killed) == {"tie_last", "over_v", "uncovered", "clip", "padding"}, dict(killed)


def test_the_predicate_on_both_sides_of_each_limit():
    c = C.by_id(CASES[0]["id"])
    assert C.served(c) and not C.served(dict(c, target=33)) and C.served(dict(c, target=32))
    assert not C.served(dict(c, pool_h=1, pool_w=1)) and not C.served(dict(c, pool_h=4)) and not C.served(dict(c, pool_w=4))
    assert not C.served(dict(c, h=1, w=2)) and C.served(dict(c, pool_h=1, h=1, w=2))
    assert C.served(c, C.PER_BLOCK * C.MAX_CHUNKS) and not C.served(c, C.PER_BLOCK * C.MAX_CHUNKS + 1) and not C.served(c, 0)
    # c_out ch cw within an int less a row's margin (the limit on K = c_out ph pw is implied: a window has at least two elements)
    tiny = dict(c, pool_h=1, pool_w=2, h=1, w=2)
    assert C.served(dict(tiny, c_out=(2 ** 31 - 13) // 2)) and not C.served(dict(tiny, c_out=(2 ** 31 - 13) // 2 + 1))
