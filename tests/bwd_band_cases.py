"""Seeded cases for the opt-in banded MFMA weight gradient (dcll_conv_lif_backward_bands[_open], k_bwd_wgrad_band): a sample cut into
bands of conv-output rows, so that the plane height no longer limits the layer.  Plain module: no GPU, numpy.random.RandomState with
fixed seeds only; a case has the fields of fuzz_cases.CONV_DEFAULT plus `bands` (0: the library's rule, 1: the slab call itself,
N >= 2: exactly N bands) and gets its tensors from fuzz_cases.conv_run.  tests/test_bwd_band_cases.py proves the list and the
references on the CPU; tests/test_gpu_bwd_band.py runs the HIP kernels against them.

plan() restates the launcher's layout (csrc/dcll_bwd_band.hip: wb_make_plan):
  bands == 1, or bands == 0 on a layer bwd_slab_cases.plan serves: the slab call itself (forwarded)
  bands == N >= 2: RB = ceil(ch / N), NB = N (band k covers the conv rows [min(ch, k RB), min(ch, (k + 1) RB)): the last ones may be
                   empty), TPW the largest number of column tiles <= min(NT, 32) that fits
  bands == 0 else: the largest TPW <= min(NT, 32) at which a band of min(ch, kh) rows fits (failing that at every TPW: at which ONE
                   row fits), the largest RB that fits beside it, NB = ceil(ch / RB), RB = ceil(ch / NB)
  LDS floats of (TPW, RB) = ((channels(TPW) (RB + kh - 1)(w + 2 pad_w) + 1 + 3) & ~3) + rows ((RB cwp) | 1), rows = min(c_out, 32 MT),
  MT = 1 for c_out <= 32 else 2; nchunk = min(B NB, 256, what the scratch holds); nchunk x NS < 256 workgroups: TPW lowered as in
  bwd_slab_cases.plan, never beyond the full launch's LDS.
  strata  forced     forced band counts on tiny planes: ch 2 .. 9 with N = 2, 3, ch; halo larger than the band; bands of pure padding;
                     pad_h 0; odd cw, cw 1; 1x1, 2x5, 9x9 kernels; c_in 1 / 3 / 70; c_out 1 / 32 / 33 / 64 / 65 / 96 / 129; poolings
                     and readouts; refractory and plain; the job order of a workgroup with several jobs; B = 257
          edge       every (MT, NQ, column split, pixel split) variant of the launcher, on both sides of its thresholds
          rule       bands = 0 where the whole plane does not fit (radio_ml_conv.yaml at netscale 2 on 24x40, 32 -> 32 on 48x48, 96
                     channels on 24x40) and on either side of the slab path's working-set limit, B = 1
          free       seeded draws
  refusals           descriptors / band counts the call refuses before any launch, with code and message
"""
import numpy as np

import bwd_slab_cases as BS
import fuzz_cases as FZ

SEED = 27011
LDS_FLOATS = 160 * 1024 // 4
MAX_TPW, MAX_CHUNKS, TARGET_WG = 32, 256, 256
MAX_K, SLAB_ROWS, SLAB_MAX = 16, 64, 65535
N_FREE = 30


def red_floats(MT):
    return 8 * MT * 16 * 64


def band_ranges(ch, RB, NB):
    """[(first conv row, rows)] of the NB bands of RB rows: band k covers [min(ch, k RB), min(ch, (k + 1) RB))."""
    return [(min(ch, k * RB), min(ch, (k + 1) * RB) - min(ch, k * RB)) for k in range(NB)]


def forwards(c, bands):
    return bands == 1 or (bands == 0 and isinstance(BS.plan(c), dict))


def plan(c, bands=None, nchunk=None, B=None):
    """The launch layout of dcll_conv_lif_backward_bands for case c (bands: c['bands'] unless given) with nchunk chunks (None: what
    an unlimited scratch gives, min(B NB, 256); 0: a full launch, what dcll_conv_lif_backward_bands_lds reports)
    -> dict(NB, RB, TPW, PS, NQ, NS, nsplit, nchunk, MT, lds (bytes), name, forwarded), or the refusal's message."""
    bands = c["bands"] if bands is None else bands
    B = c["B"] if B is None else B
    if forwards(c, bands):
        p = BS.plan(c, 0 if nchunk == 0 else min(B, MAX_CHUNKS) if nchunk is None else nchunk)
        if not isinstance(p, dict):
            return p
        ch = FZ.conv_shape(c)[0]
        return dict(NB=1, RB=ch, TPW=0, PS=0, NQ=0, NS=BS.slab_count(c["c_out"]) if c["c_out"] > SLAB_ROWS else 1, nsplit=0,
                    nchunk=min(B, MAX_CHUNKS), MT=0, lds=BS.plan(c)["lds"], name=p["name"], forwarded=True)
    if not (c["stride"] == 1 and c["dilation"] == 1 and c["groups"] == 1):
        return "plain convolutions only"
    if c["kh"] > MAX_K or c["kw"] > MAX_K:
        return "kernels up to 16x16"
    ch, cw, _, _ = FZ.conv_shape(c)
    if bands < 0:
        return "bands >= 0"
    if bands > ch:
        return "more bands than conv-output rows"
    MT = 1 if c["c_out"] <= 32 else 2
    NS = 1 if MT == 1 else BS.slab_count(c["c_out"])
    if NS > SLAB_MAX:
        return "more than 65535 slabs"
    rows = min(c["c_out"], 32 * MT)
    KK, kh = c["kh"] * c["kw"], c["kh"]
    N = c["c_in"] * KK
    NT = (N + 31) // 32
    RF, cwp = c["w"] + 2 * c["pad_w"], cw + (cw & 1)
    red = red_floats(MT)

    def img(tpw, rb):
        channels = max((min((t0 + tpw) * 32, N) - 1) // KK - (t0 * 32) // KK + 1 for t0 in range(0, NT, tpw))
        return (channels * (rb + kh - 1) * RF + 1 + 3) & ~3

    def floats(tpw, rb):
        return img(tpw, rb) + rows * ((rb * cwp) | 1)
    TPW = min(NT, MAX_TPW)
    if bands >= 1:
        RB = -(-ch // bands)
        while TPW >= 1 and floats(TPW, RB) > LDS_FLOATS:
            TPW -= 1
        if TPW < 1:
            return "a band of the forced plan"
        NB = bands
    else:
        want_rows, top = min(ch, kh), TPW
        while TPW >= 1 and floats(TPW, want_rows) > LDS_FLOATS:
            TPW -= 1
        if TPW < 1:
            TPW = top
            while TPW >= 1 and floats(TPW, 1) > LDS_FLOATS:
                TPW -= 1
        if TPW < 1:
            return "not even a one-row band with one column tile"
        RB = max(rb for rb in range(1, ch + 1) if floats(TPW, rb) <= LDS_FLOATS)
        NB = -(-ch // RB)
        RB = -(-ch // NB)
    lds = floats(TPW, RB)
    if nchunk is None:
        nchunk = min(B * NB, MAX_CHUNKS)
    wg = nchunk * NS
    if 0 < nchunk and wg < TARGET_WG:
        want = min(NT, (TARGET_WG + wg - 1) // wg)
        for tpw in range((NT + want - 1) // want, TPW):
            if floats(tpw, RB) <= max(lds, red):
                TPW, lds = tpw, floats(tpw, RB)
                break
    o_g = img(TPW, RB)
    lds = max(lds, red)
    PS = 1 if TPW >= 5 else 2 if TPW >= 3 else 4 if TPW == 2 else 8
    nsplit = (NT + TPW - 1) // TPW
    if nsplit > 65535:
        return "more than 65535 column splits"
    NQ = 1 if PS > 1 else {1: 1, 2: 2, 3: 4, 4: 4}[(TPW + 7) // 8]
    suffix = [s for s, on in (("column split", nsplit > 1), ("pixel split", PS > 1)) if on]
    name = "k_bwd_wgrad_band<%d,%d>" % (MT, NQ) + (" (%s)" % ", ".join(suffix) if suffix else "")
    return dict(NB=NB, RB=RB, TPW=TPW, PS=PS, NQ=NQ, NS=NS, nsplit=nsplit, nchunk=nchunk, MT=MT, lds=4 * lds, name=name, forwarded=False,
                NT=NT, o_g=o_g, rows=rows, GLD=(RB * cwp) | 1)


def served(c, bands=None):
    return FZ.conv_shape(c) is not None and isinstance(plan(c, bands, 0), dict)


VARIANTS = ["k_bwd_wgrad_band<%d,%s" % (mt, v) for mt in (1, 2) for v in
            ("1>", "1> (column split)", "1> (pixel split)", "1> (column split, pixel split)", "2>", "2> (column split)", "4>",
             "4> (column split)")]

default_serves = BS.default_serves


def _case(cid, stratum, k, bands, **kw):
    c = FZ._case("bwdband-%s" % cid, stratum, SEED * 100003 + k, **kw)
    c["bands"] = int(bands)
    assert served(c), (cid, plan(c, nchunk=0))
    return c


def _forced(out):
    add = lambda name, bands, **kw: out.append(_case(name, "forced", len(out), bands, **kw))
    couts = (1, 32, 33, 64, 65, 96, 129)
    k = 0
    for h in range(2, 10):                      # 3x3, pad 1: ch = h
        for n in sorted({2, 3, h}):
            if n > h:
                continue
            add("ch%d-N%d" % (h, n), n, note="ch %d in %d bands" % (h, n), c_in=(1, 3)[k % 2], c_out=couts[k % 7], h=h, w=(5, 6, 7, 8)[k % 4],
                B=2 + k % 2, refractory=k % 2)
            k += 1
    add("halo-gt-band", 6, note="kh - 1 = 4 > rb = 1", c_in=3, c_out=33, kh=5, kw=3, pad_h=2, pad_w=1, h=6, w=7, B=3)
    add("pad-ge-kh", 9, note="pad_h 3 >= kh 2: whole bands see padding only", c_in=2, c_out=65, kh=2, kw=2, pad_h=3, pad_w=1, h=4, w=6, B=3)
    add("pad-ge-kh-N4", 4, note="pad_h 3 >= kh 2, 4 bands of 3, 3, 3, 0 rows", c_in=2, c_out=20, kh=2, kw=2, pad_h=3, pad_w=1, h=4, w=6, B=3)
    add("pad0", 3, note="pad_h 0", c_in=3, c_out=64, kh=3, kw=3, pad_h=0, pad_w=0, h=8, w=7, B=3, refractory=0)
    add("cw1", 3, note="cw 1", c_in=2, c_out=36, h=6, w=3, pad_w=0, B=3)
    add("k1x1", 3, note="1x1 kernel", c_in=7, c_out=96, kh=1, kw=1, pad_h=0, pad_w=0, h=6, w=7, B=3)
    add("k2x5", 3, note="2x5 kernel", c_in=3, c_out=129, kh=2, kw=5, pad_h=1, pad_w=2, h=6, w=8, B=3, refractory=0)
    add("k9x9", 4, note="81 taps (above the default path's 64), bands of 3, 3, 3, 1 rows", c_in=2, c_out=65, kh=9, kw=9, pad_h=4, pad_w=4,
        h=10, w=10, B=2)
    add("k9x9-narrow", 5, note="81 taps, c_out 20", c_in=2, c_out=20, kh=9, kw=9, pad_h=4, pad_w=4, h=10, w=9, B=2)
    add("cin70", 3, note="c_in 70", c_in=70, c_out=33, h=6, w=7, B=2)
    add("order-B3-N3", 3, note="B 3, N 3: with room for two chunks one workgroup runs bands 0, 2, 1, 0, 2", c_in=3, c_out=65, h=7, w=6, B=3)
    add("order-B3-N3-narrow", 3, note="the same, c_out 9 and a short last band", c_in=2, c_out=9, kh=5, kw=3, pad_h=2, h=8, w=5, B=3)
    add("B257-4x4", 2, note="514 jobs on 256 chunks", c_in=2, c_out=33, h=4, w=4, B=257, target=3)
    k = 0
    for pool in ((1, 1), (2, 2), (1, 2)):
        for readout, outl in ((1, 0), (0, 0), (1, 1)):
            add("pool%dx%d-gp%d-go%d" % (pool + (readout, outl)), 2 + k % 3, note="pooling / readout gradients", c_in=3,
                c_out=(20, 65, 97)[k % 3], h=9, w=11, pool_h=pool[0], pool_w=pool[1], readout=readout, output_layer=outl, B=3,
                refractory=k % 2)
            k += 1


def _edge(out):
    add = lambda name, bands, **kw: out.append(_case(name, "edge", 300 + len(out), bands, **kw))
    # 4x8 kernel: 32 columns per input channel, ch = 2, two one-row bands.  Chunks x slabs reach 256 ("full": no lowering) or 128
    # ("half": the batch asks for two column splits)
    T = dict(kh=4, kw=8, pad_h=1, pad_w=3, h=3, w=5, target=3, rate=.4)
    for co, full in ((32, 128), (65, 64)):
        for nt in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33):
            add("c%d-tiles%d-full" % (co, nt), 2, note="%d column tiles, %d jobs" % (nt, 2 * full), c_in=nt, c_out=co, B=full, **T)
        add("c%d-tiles16-half" % co, 2, note="half the chunks: <1> column split without pixel split", c_in=16, c_out=co, B=full // 2, **T)
        add("c%d-tiles24-half" % co, 2, note="half the chunks: <2> column split", c_in=24, c_out=co, B=full // 2, **T)
        add("c%d-tiles4-B1" % co, 2, note="two jobs: column split and pixel split", c_in=4, c_out=co, B=1, **T)


def _rule(out):
    add = lambda name, **kw: out.append(_case(name, "rule", 500 + len(out), 0, **kw))
    R = dict(kh=7, kw=7, pad_h=3, pad_w=3, target=24, tau_tensor=1, B=1)
    add("radio-ns2-24x40-c1", note="radio_ml_conv.yaml at netscale 2 on 24x40: 1 -> 64", c_in=1, c_out=64, h=24, w=40, **R)
    add("radio-ns2-24x40-c64", note="radio_ml_conv.yaml at netscale 2 on 24x40: 64 -> 64", c_in=64, c_out=64, h=24, w=40, **R)
    add("radio-ns1-48x48-c32", note="radio_ml_conv.yaml at netscale 1 on 48x48: 32 -> 32", c_in=32, c_out=32, h=48, w=48, **R)
    add("c96-24x40", note="96 channels on 24x40", c_in=4, c_out=96, h=24, w=40, kh=3, kw=3, target=8, B=1)
    # the slab path's smallest working set: 628 + 1 + 64 x 629 = 40885 floats fit, 632 + 1 + 64 x 633 = 41145 do not
    L = dict(c_in=1, c_out=65, kh=1, kw=1, pad_h=0, pad_w=0, w=4, B=1, target=4)
    add("slab-fits-157x4", note="the slab call serves it: forwarded", h=157, **L)
    add("slab-refuses-158x4", note="the slab call refuses it: banded", h=158, **L)


def _free_draw(rng, k):
    while True:
        c = dict(c_in=int(rng.randint(1, 41)), c_out=int(rng.randint(1, 141)), kh=int(rng.randint(1, 10)), kw=int(rng.randint(1, 10)),
                 pad_h=int(rng.randint(0, 6)), pad_w=int(rng.randint(0, 6)), pool_h=int(rng.randint(1, 4)),
                 pool_w=int(rng.randint(1, 4)), h=int(rng.randint(1, 17)), w=int(rng.randint(1, 17)),
                 refractory=int(rng.rand() < .5), tau_tensor=int(rng.rand() < .5), bias=int(rng.rand() < .75),
                 target=int(rng.randint(1, 41)), readout=int(rng.rand() >= .07), output_layer=int(rng.rand() < 1. / 3),
                 B=int(rng.randint(1, 4)), rate=float(np.round(rng.uniform(.05, .5), 3)), state0=int(rng.rand() < .5))
        pick = int(rng.randint(4))
        if not c["readout"]:
            c["output_layer"] = 0
        full = dict(FZ.CONV_DEFAULT, **c)
        if FZ.conv_shape(full) is None or not FZ.sees_input(full):
            continue
        ch = FZ.conv_shape(full)[0]
        if ch < 2:
            continue
        bands = (2, 3, ch, int(rng.randint(2, ch + 1)))[pick]
        if bands > ch or not served(full, bands) or FZ.conv_work(full) > FZ.WORK_MAX:
            continue
        return _case("free-%02d" % k, "free", 1000 + k, bands, **c)


def cases(seed=SEED):
    out = []
    _forced(out)
    _edge(out)
    _rule(out)
    rng = np.random.RandomState(seed)
    return out + [_free_draw(rng, k) for k in range(N_FREE)]


def refusals():
    """(case, code name, message part): refused before any launch.  The scratch case is served; its call passes one float too few."""
    def r(name, k, bands, **kw):
        c = FZ._case("bwdband-refuse-%s" % name, "refuse", SEED * 100003 + 2000 + k, **kw)
        c["bands"] = bands
        return c
    S = dict(c_in=2, c_out=96, h=10, w=10, B=2)
    L = dict(c_in=1, c_out=65, kh=1, kw=1, pad_h=0, pad_w=0, B=1, target=4)
    return [
        (r("kh17", 1, 2, **dict(S, kh=17, kw=3, pad_h=8)), "UNSUPPORTED", "kernels up to 16x16"),
        (r("stride2", 2, 2, **dict(S, stride=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("dilation2", 3, 0, **dict(S, dilation=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("groups2", 4, 3, **dict(S, groups=2)), "UNSUPPORTED", "plain convolutions only"),
        (r("N-gt-ch", 5, 11, **S), "UNSUPPORTED", "more bands than conv-output rows"),
        (r("N-negative", 6, -1, **S), "UNSUPPORTED", "bands >= 0"),
        (r("forced-band-too-big", 7, 2, h=400, w=4, **L), "UNSUPPORTED", "a band of the forced plan"),
        (r("one-row-too-big", 8, 0, h=2, w=700, **L), "UNSUPPORTED", "not even a one-row band with one column tile"),
        (r("bands1-slab-refuses", 9, 1, h=158, w=4, **L), "UNSUPPORTED", "exceeds the 160 KiB of LDS"),
        (r("scratch", 10, 3, **S), "INVALID", "scratch too small"),
    ]


def exact_draw(c):
    """Small integers for the case's geometry (bwd_wide_cases.exact_draw): g_v in {-2 .. 2}, eps1 in {0 .. 3}, every partial sum an
    integer below 2^24 -> g_v, eps1, v and the integer dW, db."""
    return BS.exact_draw(c)


def chunk_jobs(B, NB, nchunk):
    """[[(sample, band)] in the order workgroup `chunk` runs them]: job = b NB + k; jobs chunk, chunk + nchunk, ..."""
    return [[divmod(j, NB) for j in range(chunk, B * NB, nchunk)] for chunk in range(nchunk)]


def band_assemble(c, g_v, eps1, NB, RB, nchunk, mutant=None, dtype=np.float64):
    """dW, db put together job by job as a workgroup of k_bwd_wgrad_band does — staging buffers that persist from job to job (the
    LDS: the band's dv rows; the rb + kh - 1 input rows under them, 0 where the row is the image's padding), the job's own rb rows
    summed — and chunk by chunk in order.  mutant (the exact test must catch each):
      'halo'     the last staged image row of a job is not written (a halo short by one row): stale
      'toppad'   staged rows that are the image's padding are not written: the previous job's data stands there
      'lastband' a short last band is summed over RB rows: the previous job's rows behind its own
    dtype float32: the kernel's summation in float32 (pixel after pixel, job after job, then the chunks in order)."""
    ch, cw, _, _ = FZ.conv_shape(c)
    B, ci, co, kh, kw, h, w = c["B"], c["c_in"], c["c_out"], c["kh"], c["kw"], c["h"], c["w"]
    IR = RB + kh - 1
    ranges = band_ranges(ch, RB, NB)
    g_v = np.asarray(g_v, dtype)
    ep = np.pad(np.asarray(eps1, dtype), ((0, 0), (0, 0), (0, 0), (c["pad_w"],) * 2))
    dW, db = np.zeros((co, ci, kh, kw), dtype), np.zeros(co, dtype)
    for jobs in chunk_jobs(B, NB, nchunk):
        img, gl = np.zeros((ci, IR, ep.shape[3]), dtype), np.zeros((co, RB, cw), dtype)
        pW, pb = np.zeros((co, ci, kh, kw), dtype), np.zeros(co, dtype)
        for b, k in jobs:
            r0, rb = ranges[k]
            if rb <= 0:
                continue
            gl[:, :rb] = g_v[b, :, r0:r0 + rb]
            nir = rb + kh - 1 - (1 if mutant == "halo" else 0)
            for yy in range(nir):
                iy = r0 - c["pad_h"] + yy
                if 0 <= iy < h:
                    img[:, yy] = ep[b, :, iy]
                elif mutant != "toppad":
                    img[:, yy] = 0
            use = RB if mutant == "lastband" else rb
            if dtype == np.float64:     # (integers below 2^53: exact in any order, one product of matrices per job)
                win = np.lib.stride_tricks.sliding_window_view(img, (use, cw), axis=(1, 2))[:, :kh, :kw]
                pW += (gl[:, :use].reshape(co, use * cw) @ win.reshape(ci * kh * kw, use * cw).T).reshape(co, ci, kh, kw)
                pb += gl[:, :use].sum(axis=(1, 2))
            else:
                for y in range(use):
                    for x in range(cw):
                        win = img[:, y:y + kh, x:x + kw]
                        pW += gl[:, y, x][:, None, None, None] * win[None]
                        pb += gl[:, y, x]
        dW += pW
        db += pb
    return dW, db


def by_id(cid):
    for c in cases() + [r[0] for r in refusals()]:
        if c["id"] == cid:
            return c
    raise KeyError(cid)
