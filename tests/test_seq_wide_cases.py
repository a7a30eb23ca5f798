"""CPU self-check of tests/seq_wide_cases.py: the case lists of dcll_conv_lif_sequence_wide's differential test are proven here
before tests/test_gpu_seq_wide.py lets them judge the kernel.

  - the seed reproduces the lists and the strata hold what they promise, both sides of every boundary included;
  - the restated predicate and byte counts equal dcll_conv_lif_sequence_wide_lds / _scratch of the built library (host-only
    calls) on every case and every refusal;
  - every template instance of k_lif_seq_wide has a case;
  - every B-operand offset of every chain addresses the link the pinned order names, inside the staged image;
  - the tile ranges of the eight waves partition the conv plane;
  - the C oracle runs every case with a sound draw: spikes and non-spikes in BOTH 32-row groups of output channels;
  - the binding declares the three symbols, and the wrappers keep today's refusal with wide=False."""
import collections
import ctypes
import inspect

import numpy as np
import pytest

import seq_wide_cases as W

CASES = W.cases()
REFUSE = W.refusals()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c["stratum"]].append(_c)
WIDE = [c for c in CASES if W.mt(c) == 2]


def _desc(c):
    from snn_modulation_classification_amd import ops
    return ops.make_conv_desc(c["c_in"], c["c_out"], (c["h"], c["w"]), (c["kh"], c["kw"]), (c["pad_h"], c["pad_w"]),
                              (c["pool_h"], c["pool_w"]), 0, False, c.get("tau_tensor", 0), 1.0 if c["refractory"] else 0.0, W.ALPHARP,
                              c["stride"], c["dilation"], c["groups"])


# sha256 over the JSON records: a change of the generator, of numpy's RandomState stream or of a seed shows up here
CASES_HASH = "bfbcbb8ea27f289d175d63fc8e46b08346116b57e915724fc5da862b49d12f14"
REFUSE_HASH = "2ce3b6a024a18faeb9514a4089680dc0667da5cc085a58f216174f2e45e0de8f"


def test_the_seed_reproduces_the_lists():
    assert W.cases_hash(W.cases()) == W.cases_hash(CASES) == CASES_HASH and W.cases_hash(W.refusals()) == W.cases_hash(REFUSE) == REFUSE_HASH
    assert W.cases_hash(W.cases(W.SEED + 1)) != W.cases_hash(CASES)
    ids = [c["id"] for c in CASES + REFUSE]
    assert len(set(ids)) == len(ids)
    assert all(W.by_id(c["id"]) == c for c in CASES[::20] + REFUSE[::5])


def test_the_strata_hold_what_they_promise():
    assert {k: len(v) for k, v in BY.items()} == dict(named=7, variants=6, edges=20, boundaries=8, grid=1, forwarded=6, free=60)
    named = {c["id"][len("wide-"):]: c for c in BY["named"]}
    geo = lambda c: (c["c_in"], c["c_out"], c["h"], c["w"], c["kh"], c["kw"], c["pad_h"], c["pool_h"], c["refractory"])
    # radio_ml_conv.yaml (32 / 32 / 32 channels, 7x7, pad 3, no pooling) at netscale 2 and 1.5 on the scripts' 16x16 plane
    assert geo(named["radio2-1to64"]) == (1, 64, 16, 16, 7, 7, 3, 1, 1) and W.variant(named["radio2-1to64"]) == "k_lif_seq_wide<1,1,0>"
    assert geo(named["radio2-64to64"]) == (64, 64, 16, 16, 7, 7, 3, 1, 1) and W.variant(named["radio2-64to64"]) == "k_lif_seq_wide<1,0,1>"
    assert geo(named["radio2-64to64-plain"])[:8] == (64, 64, 16, 16, 7, 7, 3, 1) and W.variant(named["radio2-64to64-plain"]) == "k_lif_seq_wide<0,0,1>"
    assert W.lds_bytes(named["radio2-64to64"]) == 4 * (64 * 22 * 22 + 4 * 64 + 64)             # the image is 121 KiB
    assert geo(named["radio1p5-1to48"])[:2] == (1, 48) and geo(named["radio1p5-48to48"])[:2] == (48, 48) == (int(32 * 1.5),) * 2
    # mnist_conv.yaml (16 / 24 / 32, 7x7, pad 2, pooling 2 / 1 / 2 on 28x28 -> 13 -> 11) at netscale 2
    assert geo(named["mnist2-32to48"]) == (32, 48, 13, 13, 7, 7, 2, 1, 0) and geo(named["mnist2-48to64"]) == (48, 64, 11, 11, 7, 7, 2, 2, 0)
    assert all(sum(c["Ts"]) <= 3 and c["B"] <= 2 for c in BY["named"])
    assert all(W.work(c) <= W.WORK_FREE_MAX for c in CASES if c["stratum"] != "named"), [c["id"] for c in CASES if W.work(c) > W.WORK_FREE_MAX]
    edge = {c["id"][len("wide-edge-"):]: c for c in BY["edges"]}
    assert [edge[k]["c_out"] for k in ("cout33", "cout40", "cout63", "cout64")] == [33, 40, 63, 64]
    assert (edge["cin3"]["c_in"], edge["cin5"]["c_in"]) == (3, 5) and edge["cin3"]["c_out"] == edge["cin5"]["c_out"] == 40
    assert (edge["k1x1"]["kh"], edge["k1x1"]["kw"], edge["k2x5"]["kh"], edge["k2x5"]["kw"]) == (1, 1, 2, 5)
    cp = lambda c: W.out_shape(c)[0] * W.out_shape(c)[1]
    assert (cp(edge["plane3x3"]), cp(edge["cp32"]), cp(edge["cp33"])) == (9, 32, 33)
    assert (edge["pool2-7x7"]["pool_h"], edge["pool3-9x5"]["pool_h"]) == (2, 3)
    assert (edge["hw45-out21"]["h"] * edge["hw45-out21"]["w"]) % 32 and cp(edge["hw45-out21"]) % 32
    assert not edge["nobias"]["bias"] and edge["T1"]["Ts"] == [1] and edge["T2"]["Ts"] == [2] and edge["carry"]["Ts"] == [3, 2]
    assert (edge["B1"]["B"], edge["B3"]["B"]) == (1, 3)
    assert all(W.mt(c) == 2 for c in BY["edges"] + BY["boundaries"] + BY["grid"] + BY["free"] + BY["variants"] + BY["named"])
    g = BY["grid"][0]
    assert (g["c_in"], g["c_out"], g["h"], g["kh"], g["Ts"], g["B"], g["B_checked"]) == (4, 40, 8, 3, [3], 1100, 8)
    assert all(c["c_out"] <= 32 and W.variant(c).startswith("k_lif_seq_any<") for c in BY["forwarded"])
    free = BY["free"]
    assert min(c["c_out"] for c in free) >= 33 and max(c["c_out"] for c in free) <= 64 and len({c["c_out"] for c in free}) > 20
    assert min(c["c_in"] for c in free) <= 3 and max(c["c_in"] for c in free) >= 36 and any(c["c_in"] % 2 and c["c_in"] > 1 for c in free)
    assert {c["kh"] for c in free} | {c["kw"] for c in free} == set(range(1, 10)) and any(c["kh"] != c["kw"] for c in free)
    assert {c["pool_h"] for c in free} == {c["pool_w"] for c in free} == {1, 2, 3}
    assert {c["pad_h"] for c in free} == {c["pad_w"] for c in free} == set(range(5))
    for key in ("refractory", "tau_tensor", "bias"):
        assert {c[key] for c in free} == {0, 1}, key
    assert max(t for c in free for t in c["Ts"]) <= 6 and {c["B"] for c in free} <= {1, 2, 3, 4}
    assert any(len(c["Ts"]) == 2 for c in free)


def test_both_sides_of_every_boundary():
    bound = {c["id"][len("wide-bound-"):]: c for c in BY["boundaries"]}
    ref = {c["id"][len("wide-refuse-"):]: c for c in REFUSE}
    # the LDS form's 160 KiB (a pooling layer: no register form behind it)
    assert W.lds_bytes(bound["lds-cin41"]) == 4 * 40392 <= W.LDS_MAX < W._sets(ref["lds-cin42"])[0] * 4 and W.lds_bytes(ref["lds-cin42"]) == 0
    # the register form: c_in h w, ch cw, its LDS
    for k in ("regs-nin18432", "regs-cp256", "regs-cp255", "regs-lds-cin70"):
        assert W.form(bound[k])[0] and W.lds_bytes(bound[k]) == 4 * W._sets(bound[k])[1], k
    assert bound["regs-nin18432"]["c_in"] * 256 == W.KE * W.THREADS < ref["regs-nin18688"]["c_in"] * 256
    cp = lambda c: W.out_shape(c)[0] * W.out_shape(c)[1]
    assert cp(bound["regs-cp256"]) == W.REGS_CP_MAX == 256 < cp(ref["regs-cp272"]) == 272 and cp(bound["regs-cp255"]) == 255
    assert W._sets(bound["regs-lds-cin70"])[1] * 4 == 4 * 40664 <= W.LDS_MAX < W._sets(ref["regs-lds-cin71"])[1] * 4
    for k in ("regs-nin18688", "regs-cp272", "regs-lds-cin71", "radio2-pool2"):
        full, regs, ok = W._sets(ref[k])
        assert full * 4 > W.LDS_MAX and not ok and W.lds_bytes(ref[k]) == 0, k
    # only ONE limit is crossed in each of the three
    assert W._sets(ref["regs-nin18688"])[1] * 4 <= W.LDS_MAX and cp(ref["regs-nin18688"]) <= 256
    assert ref["regs-cp272"]["c_in"] * 16 * 17 <= W.KE * W.THREADS and W._sets(ref["regs-cp272"])[1] * 4 <= W.LDS_MAX
    assert ref["regs-lds-cin71"]["c_in"] * 256 <= W.KE * W.THREADS and cp(ref["regs-lds-cin71"]) <= 256
    # whole weights in LDS
    a, b = bound["wlds-cin58"], bound["wlds-cin60"]
    assert (W.form(a)[2] + 128 * W.steps(a)) * 4 == 4 * 40944 <= W.LDS_MAX < (W.form(b)[2] + 128 * W.steps(b)) * 4
    assert W.variant(a) == "k_lif_seq_wide<0,1,0>" and W.variant(b) == "k_lif_seq_wide<0,0,0>"
    assert W.nwl(a, 2) == W.steps(a) and 0 < W.nwl(b, 2) < W.steps(b)
    # more than 256 workgroups: the streamed form keeps half the LDS free
    h = bound["b257"]
    assert h["B"] == 257 and 0 < W.nwl(h, 257) < W.nwl(h, 256) < W.steps(h)
    assert (W.form(h)[2] + 128 * W.nwl(h, 257)) * 4 <= W.LDS_MAX // 2 < (W.form(h)[2] + 128 * W.nwl(h, 256)) * 4 <= W.LDS_MAX
    assert ref["cout65"]["c_out"] == 65 and W.lds_bytes(ref["cout65"]) == 0


def test_refusals_cover_every_refusal_class():
    by = {c["id"][len("wide-refuse-"):]: c for c in REFUSE}
    unsupported = {k for k, c in by.items() if c["code"] == "DCLL_ERR_UNSUPPORTED"}
    invalid = {k for k, c in by.items() if c["code"] == "DCLL_ERR_INVALID"}
    assert unsupported >= {"cout65", "stride2", "dilation2", "groups2", "k17", "radio2-pool2", "lds-cin42"}
    assert invalid >= {"no-arp", "null-spk-in", "null-W", "null-scratch", "T-negative"}
    assert {k for k, c in by.items() if c["code"] == "DCLL_OK"} == {"T0", "B0", "T0-unsupported"}
    assert all(c["phrase"] for c in REFUSE if c["code"] != "DCLL_OK")
    assert by["no-arp"]["refractory"] == 1 and by["T-negative"]["T"] < 0
    p = by["radio2-pool2"]
    assert (p["c_in"], p["c_out"], p["h"], p["w"], p["pool_h"]) == (64, 64, 16, 16, 2)


def test_the_library_predicate_agrees_with_the_restated_one():
    from snn_modulation_classification_amd import _lib, ops
    lib = _lib.get()                # (loads without a GPU; the functions are host-only)
    for c in CASES:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_sequence_wide_lds(ctypes.byref(d)))
        assert got > 0 and got == W.lds_bytes(c) <= W.LDS_MAX, W.describe(c)
        assert ops.sequence_wide_lds(d) == got and ops.sequence_wide_supported(d)
        assert int(lib.dcll_conv_lif_sequence_wide_scratch(ctypes.byref(d))) == W.scratch_floats(c) == 64 * W.mt(c) * W.steps(c), W.describe(c)
        if W.mt(c) == 1:            # forwarded: the answers of dcll_conv_lif_sequence_any
            assert got == int(lib.dcll_conv_lif_sequence_any_lds(ctypes.byref(d)))
            assert W.scratch_floats(c) == int(lib.dcll_conv_lif_sequence_any_scratch(ctypes.byref(d)))
        else:                       # today's refusal stands
            assert int(lib.dcll_conv_lif_sequence_any_lds(ctypes.byref(d))) == 0 and not ops.sequence_any_supported(d)
    for c in REFUSE:
        d = _desc(c)
        got = int(lib.dcll_conv_lif_sequence_wide_lds(ctypes.byref(d)))
        if c["code"] == "DCLL_ERR_UNSUPPORTED":
            assert got == 0 == W.lds_bytes(c), W.describe(c)
            assert c["phrase"] in lib.dcll_last_error().decode(), (c["id"], lib.dcll_last_error())
            assert int(lib.dcll_conv_lif_sequence_wide_scratch(ctypes.byref(d))) == 0 and not ops.sequence_wide_supported(d)
        elif "unsupported" not in c["id"]:
            assert got > 0 and got == W.lds_bytes(c), W.describe(c)


def test_the_cases_reach_every_template_variant():
    var = collections.Counter(W.variant(c) for c in WIDE)
    assert set(var) == set(W.all_variants()) and len(var) == 6
    assert {W.variant(c) for c in BY["variants"]} == set(W.all_variants())
    assert {W.variant(c) for c in BY["free"]} >= {"k_lif_seq_wide<0,1,0>", "k_lif_seq_wide<1,0,0>"}
    print("cases per variant:", dict(var))


@pytest.mark.parametrize("case", WIDE, ids=[c["id"] for c in WIDE])
def test_chain_offsets_stay_inside_the_staged_image(case):
    """the kernel's offset recurrence addresses link (ci, ky, kx) of the pinned order at every MFMA step of both halves, and with
    the base of every pixel a lane can hold (the last tile's lanes beyond the plane are clamped to its last pixel) every read
    stays inside the c_in (h + 2 pad_h) (w + 2 pad_w) floats of the image"""
    c = case
    WP, HP = c["w"] + 2 * c["pad_w"], c["h"] + 2 * c["pad_h"]
    CHS = HP * WP
    ch, cw, _, _ = W.out_shape(c)
    offs, links = W.chain_offsets(c), W.chain_links(c)
    assert len(offs[0]) == len(offs[1]) == W.steps(c) == len(links[0]) == len(links[1])
    for hh in (0, 1):
        want = [-1 if l is None else l[0] * CHS + l[1] * WP + l[2] for l in links[hh]]
        assert offs[hh] == want
    ntl = (ch * cw + 31) // 32
    pix = np.minimum(np.arange(ntl * 32), ch * cw - 1)
    base0 = (pix // cw) * WP + pix % cw
    real = np.array([o for hh in (0, 1) for o in offs[hh] if o >= 0])
    assert base0.min() == 0 and real.min() >= 0 and base0.max() + real.max() < c["c_in"] * CHS
    assert base0.max() + (c["kh"] - 1) * WP + c["kw"] - 1 == CHS - 1          # the last pixel's last tap: the image's last float
    # the permuted weights: wperm[m][mt][lane] is inside the scratch for every step
    assert (W.steps(c) - 1) * 128 + 64 + 63 < W.scratch_floats(c)


@pytest.mark.parametrize("case", WIDE, ids=[c["id"] for c in WIDE])
def test_tile_ranges_partition_the_plane(case):
    ch, cw, _, _ = W.out_shape(case)
    owned = [tl for wv in range(W.NW) for tl in W.tiles_of_wave(case, wv)]
    assert sorted(owned) == list(range((ch * cw + 31) // 32))
    pix = sorted(p for tl in owned for p in range(tl * 32, min(tl * 32 + 32, ch * cw)))
    assert pix == list(range(ch * cw))
    if W.form(case)[0]:
        assert all(len(W.tiles_of_wave(case, wv)) <= 1 for wv in range(W.NW))


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_is_sound(case):
    c = case
    T, traj = W.run(c)                          # (asserts: accepted by the oracle, its shapes, a sound draw within 24 attempts)
    assert W.unsound(c, traj) is None, W.describe(c)
    assert len(traj) == len(c["Ts"]) == len(T["calls"])
    ch, cw, ph, pw = W.out_shape(c)
    for n, call in zip(c["Ts"], traj):
        assert call["v"].shape == (n, c["B_checked"], c["c_out"], ch, cw) and call["s"].shape == (n, c["B_checked"], c["c_out"], ph, pw)
    for lo in range(0, c["c_out"], 32):         # both M tiles: a spiking and a silent entry among the channels of the tile
        s = np.concatenate([call["v"][:, :, lo:lo + 32].ravel() for call in traj]) > 0
        assert s.any() and not s.all(), (c["id"], lo)
    assert (T["b"] is None) == (not c["bias"])


def test_the_binding_declares_the_three_symbols():
    from snn_modulation_classification_amd import _lib
    S = _lib.SIGNATURES
    assert S["dcll_conv_lif_sequence_wide"] == S["dcll_conv_lif_sequence_any"]
    assert S["dcll_conv_lif_sequence_wide_lds"] == S["dcll_conv_lif_sequence_any_lds"]
    assert S["dcll_conv_lif_sequence_wide_scratch"] == S["dcll_conv_lif_sequence_any_scratch"]
    lib = _lib.get()
    assert lib.dcll_version() == _lib.ABI_VERSION == 10
    assert all(hasattr(lib, n) for n in ("dcll_conv_lif_sequence_wide", "dcll_conv_lif_sequence_wide_lds", "dcll_conv_lif_sequence_wide_scratch"))


def test_the_wrappers_keep_todays_refusal_without_wide():
    from snn_modulation_classification_amd import ops
    from snn_modulation_classification_amd.dcll.pytorch_libdcll import Conv2dDCLLlayer
    from snn_modulation_classification_amd.networks import ConvNetwork
    for fn in (Conv2dDCLLlayer.sequence_any_supported, Conv2dDCLLlayer.forward_sequence_any, ConvNetwork.sequence_any_supported,
               ConvNetwork.test_sequence_any):
        assert inspect.signature(fn).parameters["wide"].default is False, fn
    c = W.by_id("wide-edge-cout33")
    d = _desc(c)
    assert not ops.sequence_any_supported(d) and ops.sequence_any_lds(d) == 0 and ops.sequence_wide_supported(d)
    from snn_modulation_classification_amd import _lib
    ops.sequence_any_lds(d)
    assert "c_out <= 32" in _lib.get().dcll_last_error().decode()
