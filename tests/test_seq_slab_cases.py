"""CPU self-check of tests/seq_slab_cases.py, the cases of dcll_conv_lif_sequence_slabs (k_lif_seq_slab), before
tests/test_gpu_seq_slab.py lets them judge the kernel:

  - the slabs partition [0, c_out) exactly once for c_out 1 .. 300;
  - the list is well-formed (unique ids, the named layers, the shapes where slabs can go wrong, every plan kind, every template
    instance, both sides of the LDS limit and of whole-weights-in-LDS, the large grid, the forwarded layers) and the seed reproduces
    it exactly (hash of the records);
  - the restated plan, LDS formula and scratch size are the library's host-side answers (no GPU needed: nothing is launched) for
    every case and refusal, and every 64-channel slice of every case is served by dcll_conv_lif_sequence_tiles with the same plan;
  - every slab of every case has both spikes and non-spikes (draws are re-seeded until this holds; the cap on attempts is asserted);
  - the C oracle run slab by slab on 64-channel slices and stitched == the whole-layer oracle, bit for bit;
  - three mutants of that assembly — a slab offset by one M tile, the bias taken from slab 0, the traces never written back — are
    each caught in every multi-slab case they can touch (bias0: cases with a bias; no-state: cases of two calls)."""
import ctypes
import os

import numpy as np
import pytest

import seq_slab_cases as SL
import seq_tile_cases as X
from conftest import ROOT

CASES = SL.cases()
REFUSE = SL.refusals()
MULTI = [c for c in CASES if c["c_out"] > 64]

CASES_HASH = "b5b7236246430f3c7b773d8b740c7a14cd900ba86866d8437a0504cb53a63e53"
REFUSALS_HASH = "6f376e75b1a7cf284eea2395abaf81052f3df9a96aea0f7f34856eeef45f965a"


def test_the_slabs_partition_the_channels_exactly_once():
    for c_out in range(1, 301):
        owner = np.zeros(c_out, np.int64)
        for first, n in SL.slabs(c_out):
            assert first % 64 == 0 and 1 <= n <= 64
            owner[first:first + n] += 1
        assert (owner == 1).all() and len(SL.slabs(c_out)) == -(-c_out // 64), c_out


def test_the_list_is_well_formed():
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    strata = {s: [c for c in CASES if c["stratum"] == s] for s in ("named", "shape", "plan", "forwarded", "free")}
    assert sum(len(v) for v in strata.values()) == len(CASES) and len(strata["free"]) == SL.N_FREE == 30
    for c in CASES:
        assert SL.plan_of(c) is not None and (c["stride"], c["dilation"], c["groups"]) == (1, 1, 1), c["id"]
        assert (c["c_out"] <= 64) == (c["stratum"] == "forwarded"), c["id"]
        assert c["h"] <= 16 and c["w"] <= 16 or c["id"] == "slab-pw40-shared-words", c["id"]
        assert (c["B"] <= 5 and sum(c["Ts"]) <= 6) or c["id"] == "slab-grid-B300" or c["stratum"] == "free", c["id"]
        assert sum(c["Ts"]) <= 8 and c["B"] <= 5 or c["id"] == "slab-grid-B300", c["id"]
    named = {(c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["pad_h"], c["B"], tuple(c["Ts"])) for c in strata["named"]}
    assert named == {(96, 96, 16, 16, 7, 3, 1, (3,)), (128, 128, 16, 16, 7, 3, 1, (3,))}
    sh = strata["shape"]
    assert {65, 96, 97, 128, 129, 200} <= {c["c_out"] for c in sh} and {1, 3, 64, 70} <= {c["c_in"] for c in sh}
    assert {(1, 1), (2, 5), (3, 3), (7, 7), (9, 9)} <= {(c["kh"], c["kw"]) for c in sh}
    shapes = [SL.out_shape(c) for c in sh]
    assert any(s[1] % 2 and (s[0] * s[1]) % 2 for s in shapes) and {9, 32, 33} <= {s[0] * s[1] for s in shapes}
    assert {(c["pool_h"], c["pool_w"]) for c in sh} >= {(1, 1), (2, 2), (3, 3), (1, 2)} and {c["refractory"] for c in sh} == {0, 1}
    # plans: 1 x 1, N x 1, 1 x N, 2 x 2, one tile per pooled pixel, and the rule; the rule on both sides of one tile
    plans = {tuple(c["tiles"]) for c in strata["plan"]}
    assert {(1, 1), (3, 1), (1, 3), (2, 2), (0, 0), (12, 10)} <= plans
    assert SL.plan_of(SL.by_id("slab-lds-cin41-1x1")) == (1, 1) and SL.lds_bytes(SL.by_id("slab-lds-cin41-1x1")) == 4 * (584 * 41 + 16448)
    assert SL.plan_of(dict(SL.by_id("slab-lds-cin42-rule"), tiles=[1, 1])) is None and SL.plan_of(SL.by_id("slab-lds-cin42-rule")) == (2, 1)
    assert SL.plan_of(dict(SL.by_id("slab-lds-cin41-1x1"), tiles=[0, 0])) == (1, 1)
    # whole weights in LDS: 104 c_in + 2368 floats of base + 128 per chain step (9 (c_in / 2) + 5 for an odd last channel)
    assert [SL.whole_weights(SL.by_id("slab-wlds-cin%d" % n), 1, 1) for n in (8, 56, 57)] == [True, True, False]
    assert 104 * 56 + 2368 + 128 * 252 == 40448 <= 40960 < 104 * 57 + 2368 + 128 * 257
    assert {SL.variant(c) for c in MULTI} == set(SL.all_variants())
    g = SL.by_id("slab-grid-B300")
    assert (g["B"], g["c_out"], g["h"], g["w"], g["Ts"]) == (300, 65, 4, 4, [3]) and 300 * 4 * 2 > 256
    assert sorted(c["c_out"] for c in strata["forwarded"]) == [40, 64]
    assert all(SL.variant(c).startswith(("k_lif_seq_tile", "k_lif_seq_band")) for c in strata["forwarded"])
    assert any(len(c["Ts"]) == 2 for c in MULTI) and any(X.shared_words(c, *SL.plan_of(c)) for c in MULTI)
    assert all(65 <= c["c_out"] <= 200 for c in strata["free"])
    # the LDS of a workgroup does not grow with c_out; the grid's bound
    c = SL.by_id("slab-t2x2")
    assert SL.lds_bytes(c) == SL.lds_bytes(dict(c, c_out=6400)) and SL.plan_of(dict(c, c_out=64 * 65535 + 1)) is None


def test_the_seed_reproduces_the_list_exactly():
    assert SL.cases_hash(SL.cases()) == SL.cases_hash(CASES) == CASES_HASH
    assert SL.cases_hash(SL.refusals()) == REFUSALS_HASH
    assert SL.cases_hash(SL.cases(SL.SEED + 1)) != CASES_HASH


def test_the_binding_and_the_host_side_plan():
    import inspect
    import test_gpu_seq_any as G
    from snn_modulation_classification_amd import _lib, ops
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import Conv2dDCLLlayer
    from snn_modulation_classification_amd.networks import ConvNetwork
    header = open(os.path.join(ROOT, "include", "dcll_hip.h")).read()
    for tail in ("", "_plan", "_lds", "_scratch"):
        sym = "dcll_conv_lif_sequence_slabs" + tail
        assert sym + "(" in header and _lib.SIGNATURES[sym] == _lib.SIGNATURES["dcll_conv_lif_sequence_tiles" + tail], sym
    assert "#define DCLL_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    for fn in (Conv2dDCLLlayer.forward_sequence_any, Conv2dDCLLlayer.sequence_any_supported, ConvNetwork.test_sequence_any,
               ConvNetwork.sequence_any_supported):
        assert "slabs" in inspect.signature(fn).parameters
    import train
    assert train.parse_args(["--slab_sequence_path"]).slab_sequence_path == [] and train.parse_args([]).slab_sequence_path is None
    assert train.parse_args(["--slab_sequence_path", "2", "3"]).slab_sequence_path == [2, 3]
    lib = _lib.get()
    for c in CASES + [r for r in REFUSE if r["code"] != "DCLL_OK" and r["null"] is None and r["T"] >= 0]:
        d, B = G._desc(c), c["B"]
        nn = (ctypes.c_int32 * 2)()
        n = lib.dcll_conv_lif_sequence_slabs_plan(ctypes.byref(d), B, c["tiles"][0], c["tiles"][1], nn, None, None)
        p = SL.plan_of(c, B)
        assert (n, (nn[0], nn[1]) if n else None) == ((0, None) if p is None else (p[0] * p[1], p)), c["id"]
        assert lib.dcll_conv_lif_sequence_slabs_lds(ctypes.byref(d), c["tiles"][0], c["tiles"][1]) == SL.lds_bytes(c), c["id"]
        if p is None:
            assert c["phrase"] in lib.dcll_last_error().decode(), c["id"]
        else:
            assert lib.dcll_conv_lif_sequence_slabs_scratch(ctypes.byref(d), B) == SL.scratch_floats(c, B), c["id"]
            assert ops.sequence_slabs_supported(d, c["tiles"]) and (c["c_out"] <= 64) == ops.sequence_tiles_supported(d, c["tiles"]), c["id"]
    for c in MULTI:                 # every slice is a layer dcll_conv_lif_sequence_tiles serves with the same plan
        for s in range(SL.slab_count(c["c_out"])):
            sc = SL.slice_case(c, s)
            assert X.tile_count(sc) is not None and ops.sequence_tiles_supported(G._desc(sc), sc["tiles"]), sc["id"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x[k]), _bits(y[k])) for x, y in zip(a, b) for k in ("v", "s", "pv", "arp", "eps0", "eps1"))


@pytest.mark.parametrize("case", MULTI, ids=[c["id"] for c in MULTI])
def test_slab_sliced_oracle_equals_the_whole_and_catches_the_mutants(case):
    c = case
    T, traj = SL.run(c)                     # (sound: every slab has spikes and non-spikes; at most MAX_ATTEMPTS re-seeded draws)
    assert 0 <= T["attempt"] < SL.MAX_ATTEMPTS == 24 and SL.unsound(c, traj) is None
    for first, n in SL.slabs(c["c_out"]):
        s = np.concatenate([call["v"][:, :, first:first + n].ravel() for call in traj]) > 0
        assert s.any() and not s.all(), (c["id"], first)
    assert _same(SL.slabbed_trajectory(c, T), traj), (c["id"], "the slab-sliced oracle differs from the whole layer's")
    assert not _same(SL.slabbed_trajectory(c, T, "mtile"), traj), (c["id"], "mtile")
    if c["bias"]:
        assert not _same(SL.slabbed_trajectory(c, T, "bias0"), traj), (c["id"], "bias0")
    if len(c["Ts"]) > 1:
        assert not _same(SL.slabbed_trajectory(c, T, "no-state"), traj), (c["id"], "no-state")


def test_the_mutants_reach_enough_cases():
    assert sum(c["bias"] for c in MULTI) >= 50 and sum(len(c["Ts"]) > 1 for c in MULTI) >= 10
