// dcll_step_slab.hip — k_lif_step_slab: ONE timestep of a plain conv layer of ANY number of output channels and any plane height
// (stride = dilation = groups = 1, kernel up to 16x16, any c_in, padding, pooling and batch) on the matrix pipe
// (dcll_conv_lif_step_slab) — the opt-in MFMA form of the layers dcll_conv_lif_step serves with k_trace + k_conv_lif[_tiled] +
// k_pool and dcll_conv_lif_step_wide refuses: more than 64 output channels, or a padded eps1 image beyond a workgroup's LDS.
// The per-step sibling of k_lif_seq_slab (dcll_seq_slab.hip): k_lif_step_wide's chains, one 64-row slab of output channels and
// one band of output rows per workgroup.  A layer dcll_conv_lif_step_wide serves, asked for with bands = 0, IS that call
// (dcll_hip.hip), so a network of mixed widths goes through one entry point.
//
// Grid = B x NB x NS (blockIdx.x = sample, .y = band, .z = slab).  NS = slab_count(c_out), the slab rule of dcll_any_shared.h:
// slab s owns the channels [64 s, min(64 s + 64, c_out)), two 32-row M tiles, the second empty in a last slab of at most 32
// rows.  Band k of NB is band_plan()'s part k in the h direction (the partition k_lif_seq_band uses): pooled rows [P0, P1),
// conv rows [C0, C1); the last band owns the conv rows behind the last window of floor-mode pooling.  No tiling in w.
//
// The plan (step_slab_plan() is the ONE statement of it; tests/step_slab_cases.py restates it):
//   NB_fit = the smallest NB <= ph whose largest band fits in 160 KiB of LDS (none: the layer is refused)
//   units  = 2 ceil(ch cw / 32);  ns0 = min(ceil(units / DCLL_STEP_SLAB_UNITS), 256 / (B NS));  NB = max(NB_fit, min(ns0, ph))
//   bands = N >= 1 asks for exactly N bands instead (N > ph, or a band beyond the LDS: refused)
// LDS of the (band, slab) workgroup (floats; step_slab_lds_floats() is the ONE statement of it, its maximum over the bands is
// exported as dcll_conv_lif_step_slab_lds):
//   img   c_in x (C1 - C0 + kh - 1) x (w + 2 pad_w)   the padded eps1 rows [C0 - pad_h, C1 - pad_h + kh - 1) of this step, zero
//         padding written: the B operand of every chain link is one read at ci CHS + (y - C0 + ky) WP + x + kx
//   vpl   64 x (C1 - C0) x cw                          pooling layers only: the slab's v at conv resolution
//   bias  64
// The traces are NOT advanced in this kernel: workgroups of one sample read each other's halo rows and every slab reads the same
// traces, so an in-place update would race.  The entry point runs k_trace first; the staging here is read-only.
//
// The weights are not staged: k_step_slab_wprep writes w_scratch in front of this kernel on every call (nothing is cached, the
// learning step changes W through raw pointers), wperm[s][m][lane][mt] = weight of link 2 m + (lane >> 5) for output channel
// 64 s + 32 mt + (lane & 31): a slab streams one contiguous run of 128 floats per chain step from L2, a lane fetches both M
// tiles' A values of a step with ONE 8-byte load, eight steps in flight per wave.  A last slab of at most 32 rows loads its first
// column alone (4 bytes), so the second, which holds no channel, is never read.
//
// Arithmetic = the contract of include/dcll_hip.h and exactly k_lif_step_wide's rule: the chain of output (co, y, x) starts at
// bias[co] and runs over the links (cp, ky, kx, h), ci = 2 cp + h, one v_mfma_f32_32x32x2_f32 per two CONSECUTIVE links; the last
// channel of an odd c_in pairs its taps two by two, and a link beyond the last carries a zero weight and a zero input.  Every
// chain is unsplit, so every v is ONE fmaf chain whatever NB and NS are: nothing depends on the plan.
//
// Work units: (32-pixel tile of the band's flattened conv pixels, M tile of the slab), u = nmt tile + mt.  Wave w runs units
// w, w + 8, ..., one chain each; where the pairs (both M tiles of pixel tiles w, w + 8, ...) take no more rounds than the single
// units (two M tiles and ceil(tiles / 8) 2 <= ceil(2 tiles / 8)), a wave holds both M tiles of its pixel tiles and one LDS read
// of the B operand feeds two MFMAs, as in k_lif_step_wide's fused form.  Outputs of different (band, slab) workgroups are
// disjoint: nothing is ORed and nothing is shared.
#include "dcll_any_shared.h"
#include <mutex>

constexpr int SS_THREADS = 512, SS_NW = SS_THREADS / 64;
constexpr int SS_MAX_DEVICES = 64;
// small-batch rule: units a workgroup should keep (one chain per SIMD when CUs are idle) — the computed value, not a measured one
#ifndef DCLL_STEP_SLAB_UNITS
#define DCLL_STEP_SLAB_UNITS 4
#endif
constexpr int SS_UNITS = DCLL_STEP_SLAB_UNITS;
static_assert(SS_UNITS >= 1, "DCLL_STEP_SLAB_UNITS >= 1");

typedef float f32x2s __attribute__((ext_vector_type(2), aligned(4)));      // (w_scratch is only 4-byte aligned by contract)

struct step_slab_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int WP;                     // padded row length of img
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int nb;                     // bands per sample
    any_div dWP, dCW, dPW;
};

static inline bool step_slab_pooled(const dcll_conv_desc *d) { return !(d->pool_h == 1 && d->pool_w == 1); }

// the working set of the workgroups of band k of nb, in floats
static inline long step_slab_lds_floats(const dcll_conv_desc *d, int k, int nb)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const band_rows r = band_plan(k, nb, d->h, d->kh, d->pad_h, d->pool_h, ch, ph);
    const long img = (long)d->c_in * (r.C1 - r.C0 + d->kh - 1) * (d->w + 2 * d->pad_w);
    const long vpl = step_slab_pooled(d) ? (long)SLAB_ROWS * (r.C1 - r.C0) * cw : 0;
    return img + vpl + SLAB_ROWS;
}

// the largest band's working set under nb bands, in floats
static inline long step_slab_lds_max(const dcll_conv_desc *d, int nb)
{
    long mx = 0;
    for (int k = 0; k < nb; ++k) {
        const long f = step_slab_lds_floats(d, k, nb);
        if (f > mx) mx = f;
    }
    return mx;
}

// the layers of this file, whatever the plan: plain conv, kernel up to 16x16, a grid's worth of slabs
static int step_slab_layer_ok(const dcll_conv_desc *d, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    if (slab_count(d->c_out) > SLAB_MAX) return fail(DCLL_ERR_UNSUPPORTED, "at most 65535 slabs of 64 output channels", who);
    return DCLL_OK;
}

// The plan of a call: DCLL_OK with *nb bands and *ns slabs, or the refusal with its message.  bands = 0: the rule of the file
// header; bands = N >= 1: exactly N bands
int dcll_step_slab_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int *nb, int *ns, const char *who)
{
    int rc = step_slab_layer_ok(d, who);
    if (rc) return rc;
    if (bands < 0) return fail(DCLL_ERR_INVALID, "negative band count", who);
    if (B < 1) return fail(DCLL_ERR_INVALID, "the plan needs a batch of at least one sample", who);
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const int NS = slab_count(d->c_out);
    int n;
    if (bands > 0) {
        if (bands > ph) return fail(DCLL_ERR_UNSUPPORTED, "more bands than pooled rows", who);
        n = bands;
        if (step_slab_lds_max(d, n) * 4 > ANY_LDS_MAX)
            return fail(DCLL_ERR_UNSUPPORTED, "a band's working set (its padded eps1 rows, the v plane of a pooling layer) exceeds "
                                              "the 160 KiB of LDS", who);
    } else {
        int fit = 0;
        for (int q = 1; q <= ph && !fit; ++q)
            if (step_slab_lds_max(d, q) * 4 <= ANY_LDS_MAX) fit = q;
        if (!fit)
            return fail(DCLL_ERR_UNSUPPORTED, "not even one pooled row's working set (its padded eps1 rows, the v plane of a "
                                              "pooling layer) fits in the 160 KiB of LDS", who);
        const long units = 2 * (((long)ch * cw + 31) / 32);
        long ns0 = (units + SS_UNITS - 1) / SS_UNITS;
        const long room = ANY_CUS / ((long)B * NS);
        if (ns0 > room) ns0 = room;
        if (ns0 > ph) ns0 = ph;
        n = ns0 > fit ? (int)ns0 : fit;
        if (step_slab_lds_max(d, n) * 4 > ANY_LDS_MAX)      // (the last band is the largest under every count, so this holds)
            return fail(DCLL_ERR_UNSUPPORTED, "the band plan does not fit in the 160 KiB of LDS", who);
    }
    *nb = n;
    *ns = NS;
    return DCLL_OK;
}

// true: the call is dcll_conv_lif_step_wide's (c_out <= 64, the rule asked for, and that entry point serves the layer)
bool dcll_step_slab_forwards(const dcll_conv_desc *d, int32_t bands)
{
    return d && bands == 0 && d->c_out <= SLAB_ROWS && dcll_step_wide_check(d, "dcll_conv_lif_step_wide") == DCLL_OK;
}

extern "C" int dcll_conv_lif_step_slab_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int32_t *nb, int32_t *ns)
{
    const char *who = "dcll_conv_lif_step_slab_plan";
    if (!nb || !ns) return fail(DCLL_ERR_INVALID, "null pointer", who);
    if (bands >= 0 && B >= 1 && dcll_step_slab_forwards(d, bands)) {    // dcll_conv_lif_step_wide's call: no band, no slab
        *nb = 0;
        *ns = 0;
        return DCLL_OK;
    }
    int n = 0, s = 0;
    const int rc = dcll_step_slab_plan(d, B, bands, &n, &s, who);
    if (rc) return rc;
    *nb = n;
    *ns = s;
    return DCLL_OK;
}

extern "C" int64_t dcll_conv_lif_step_slab_lds(const dcll_conv_desc *d, int32_t B, int32_t bands)
{
    if (bands >= 0 && B >= 1 && dcll_step_slab_forwards(d, bands)) return dcll_conv_lif_step_wide_lds(d);
    int nb, ns;
    if (dcll_step_slab_plan(d, B, bands, &nb, &ns, "dcll_conv_lif_step_slab_lds") != DCLL_OK) return 0;
    return step_slab_lds_max(d, nb) * 4;
}

// floats of w_scratch: 128 per MFMA step of a chain and slab (k_step_slab_wprep's order; enough for a forwarded call too);
// 0 = not served
extern "C" int64_t dcll_conv_lif_step_slab_scratch(const dcll_conv_desc *d)
{
    if (step_slab_layer_ok(d, "dcll_conv_lif_step_slab_scratch") != DCLL_OK) return 0;
    return any_chain_steps(d) * 2 * SLAB_ROWS * slab_count(d->c_out);
}

// W (c_out, c_in, kh, kw) -> wperm[s][m][lane][mt]: link 2 m + h of channel co = 64 s + 32 mt + (lane & 31), h = lane >> 5;
// 0 beyond c_out / the chain
__global__ void k_step_slab_wprep(const float *__restrict__ W, float *__restrict__ wperm, int c_in, int c_out, int kh, int kw,
                                  int npair, int nsteps, long total)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long sm = i >> 7;
    const int s = (int)(sm / nsteps), m = (int)(sm - (long)s * nsteps);
    const int lane = (int)(i >> 1) & 63, mt = (int)i & 1, co = slab_first(s) + 32 * mt + (lane & 31), h = lane >> 5, KK = kh * kw;
    int ci, tap;
    any_link(m, h, npair, c_in, KK, ci, tap);
    wperm[i] = (co < c_out && tap < KK) ? W[((long)co * c_in + ci) * KK + tap] : 0.0f;
}

int dcll_launch_step_slab_wprep(const dcll_conv_desc *d, const float *W, float *wperm, hipStream_t st)
{
    const int npair = (int)any_chain_pairs(d), nsteps = (int)any_chain_steps(d);
    const long total = (long)nsteps * 2 * SLAB_ROWS * slab_count(d->c_out);
    hipLaunchKernelGGL(k_step_slab_wprep, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, wperm, d->c_in, d->c_out,
                       d->kh, d->kw, npair, nsteps, total);
    HIP_CHECK_LAUNCH("k_step_slab_wprep");
    return DCLL_OK;
}

// the A values of chain step m for this lane (wps: the slab's run of wperm): NM == 2 both M tiles in one 8-byte load, NM == 1
// tile mt alone
template <int NM>
__device__ __forceinline__ void ss_load_a(const float *__restrict__ wps, int m, int lane, int mt, float (&a)[NM])
{
    if constexpr (NM == 2) {
        const f32x2s v = *(const f32x2s *)(wps + (m * 64 + lane) * 2);
        a[0] = v.x;
        a[1] = v.y;
    } else {
        a[0] = wps[(m * 64 + lane) * 2 + mt];
    }
}

// the whole chain(s) of one pixel tile (k_lif_step_wide's loop; NM accumulators fed by one B read per step); rows of img are WP
// floats apart, channels CHS
template <int NM>
__device__ __forceinline__ void ss_chains(const step_slab_geom &g, int CHS, const float *__restrict__ wps, const float *img,
                                          int base0, int hh, int lane, int mt, f32x16 (&acc)[NM])
{
    const float *bp = img + base0 + hh * CHS;
    int m = 0, off = 0, kx = 0, ky = 0;
    for (; m < g.npair; m += 8) {               // (cp, ky, kx): both channels of the pair at one wave-uniform offset
        float a[8][NM];                         // eight steps' A fragments requested before the first is used (L2 latency)
#pragma unroll
        for (int u = 0; u < 8; ++u) ss_load_a<NM>(wps, m + u < g.npair ? m + u : g.npair - 1, lane, mt, a[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (m + u < g.npair) {
                const float bv = bp[off];
#pragma unroll
                for (int t = 0; t < NM; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], bv, acc[t], 0, 0, 0);
                ++off;
                if (++kx == g.kw) {
                    kx = 0;
                    off += g.WP - g.kw;
                    if (++ky == g.kh) {
                        ky = 0;
                        off += 2 * CHS - g.kh * g.WP;
                    }
                }
            }
        }
    }
    m = g.npair;
    if (g.c_in & 1) {                           // the last channel alone: taps (2 q, 2 q + 1), tap KK (odd KK) is the zero link
        const float *cb = img + (g.c_in - 1) * CHS + base0;
        const int KK = g.kh * g.kw;
        int tap = hh, tkx = hh, tky = 0;
        while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
        for (; m < g.nsteps; ++m) {
            const float bv = tap < KK ? cb[tky * g.WP + tkx] : 0.0f;
            float a[NM];
            ss_load_a<NM>(wps, m, lane, mt, a);
#pragma unroll
            for (int t = 0; t < NM; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], bv, acc[t], 0, 0, 0);
            tap += 2;
            tkx += 2;
            while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
        }
    }
}

// what becomes of the accumulators of M tile mt at the band's conv pixel pix < NPb: POOL -> the v plane; else the whole epilogue
// (conv pixel = output pixel, o0 = the element of (sample, channel co0, the band's first pixel)): refractory update on arp in
// HBM, threshold, sigmoid, stores.  Rows at or beyond the slab's nrow are never stored
template <bool R, bool POOL>
__device__ __forceinline__ void ss_epilogue(const step_slab_geom &g, const f32x16 &acc, int mt, int hh, int pix, int NPb, int nrow,
                                            long o0, float *vpl, float *__restrict__ arp_g, float *__restrict__ out_s,
                                            float *__restrict__ out_pv, float *__restrict__ out_v, float alpharp, float wrp)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int col = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (col >= nrow) continue;
        if constexpr (POOL) {
            vpl[col * NPb + pix] = acc[r];
        } else {
            const long o = o0 + (long)col * g.CP + pix;
            float v = acc[r];
            bool s;
            if (R) {
                float ar = arp_g[o];
                v = refractory(acc[r], ar, alpharp, wrp, s);
                arp_g[o] = ar;
            } else {
                s = v > 0.0f;
            }
            out_s[o] = s ? 1.0f : 0.0f;
            out_pv[o] = sigmoidf_dev(v);
            if (out_v) out_v[o] = v;
        }
    }
}

template <bool R, bool POOL>
__global__ __launch_bounds__(SS_THREADS) void k_lif_step_slab(const step_slab_geom g, const float *__restrict__ wperm,
                                                             const float *__restrict__ bias, const float *__restrict__ eps1_g,
                                                             float *__restrict__ arp_g, float *__restrict__ out_s,
                                                             float *__restrict__ out_pv, float *__restrict__ out_v, float alpharp,
                                                             float wrp)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long b = blockIdx.x;
    const int band = blockIdx.y, slab = blockIdx.z;
    const band_rows br = band_plan(band, g.nb, g.h, g.kh, g.pad_h, g.pool_h, g.ch, g.ph);
    const int crows = br.C1 - br.C0, rows = crows + g.kh - 1, CHS = rows * g.WP, NPb = crows * g.cw;
    const int co0 = slab_first(slab), nrow = slab_rows(slab, g.c_out), nmt = nrow > 32 ? 2 : 1;
    const int HW = g.h * g.w, NTL = (NPb + 31) >> 5;
    float *img = lds, *vpl = lds + g.c_in * CHS, *sb = vpl + (POOL ? SLAB_ROWS * NPb : 0);
    const float *wps = wperm + (long)slab * g.nsteps * (2 * SLAB_ROWS);

    // ---- the band's padded rows of eps1 (advanced by k_trace in front of this kernel): padding zeroed, read-only
    {
        const any_div dR = make_div(rows);
        const float *e1b = eps1_g + b * g.c_in * HW;
        for (int q = tid; q < g.c_in * CHS; q += SS_THREADS) {
            const int rr = fdiv(q, g.dWP), xp = q - rr * g.WP, ci = fdiv(rr, dR), r = rr - ci * rows;
            const int y = br.C0 + r - g.pad_h, xx = xp - g.pad_w;
            img[q] = (y >= 0 && y < g.h && xx >= 0 && xx < g.w) ? e1b[ci * HW + y * g.w + xx] : 0.0f;
        }
        if (tid < SLAB_ROWS) sb[tid] = (bias && tid < nrow) ? bias[co0 + tid] : 0.0f;
    }
    __syncthreads();

    // the lane's pixel of tile tl (a ragged lane reads the last pixel's window) and its offset in a channel of img
    auto pixel = [&](int tl, int &pix) -> int {
        pix = tl * 32 + j;
        const int pc = pix < NPb ? pix : NPb - 1;
        const int y = fdiv(pc, g.dCW), xq = pc - y * g.cw;
        return y * g.WP + xq;
    };
    const long o0 = (b * g.c_out + co0) * g.CP + (long)br.C0 * g.cw;

    if (nmt == 2 && 2 * ((NTL + SS_NW - 1) / SS_NW) <= (2 * NTL + SS_NW - 1) / SS_NW) {
        // ---- both chains of a pixel tile, interleaved: wave wv runs pixel tiles wv, wv + 8, ...
        for (int tl = wv; tl < NTL; tl += SS_NW) {
            int pix;
            const int base0 = pixel(tl, pix);
            f32x16 acc[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][r] = sb[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh];
            ss_chains<2>(g, CHS, wps, img, base0, hh, lane, 0, acc);
            if (pix < NPb) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    ss_epilogue<R, POOL>(g, acc[mt], mt, hh, pix, NPb, nrow, o0, vpl, arp_g, out_s, out_pv, out_v, alpharp, wrp);
            }
        }
    } else {
        // ---- one chain per unit: wave wv runs units wv, wv + 8, ...
        const int NU = nmt * NTL;
        for (int u = wv; u < NU; u += SS_NW) {
            const int tl = nmt == 2 ? u >> 1 : u, mt = nmt == 2 ? u & 1 : 0;
            int pix;
            const int base0 = pixel(tl, pix);
            f32x16 acc[1];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][r] = sb[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh];
            ss_chains<1>(g, CHS, wps, img, base0, hh, lane, mt, acc);
            if (pix < NPb) ss_epilogue<R, POOL>(g, acc[0], mt, hh, pix, NPb, nrow, o0, vpl, arp_g, out_s, out_pv, out_v, alpharp, wrp);
        }
    }
    if constexpr (POOL) {
        __syncthreads();
        const int NV = nrow * NPb;
        // ---- refractory update on the slab's v plane of the band (arp in HBM), out_v
        if (R || out_v) {
            const any_div dNP = make_div(NPb);
            for (int i = tid; i < NV; i += SS_THREADS) {
                const int col = fdiv(i, dNP), p = i - col * NPb;
                const long o = o0 + (long)col * g.CP + p;
                float v = vpl[i];
                if (R) {
                    float ar = arp_g[o];
                    bool s;
                    v = refractory(v, ar, alpharp, wrp, s);
                    arp_g[o] = ar;
                    vpl[i] = v;
                }
                if (out_v) out_v[o] = v;
            }
            __syncthreads();
        }
        // ---- the pooling pass over the band's pooled rows [P0, P1): MaxPool2d(kernel = stride = pool, padding (pool - 1) / 2)
        // over v; their windows, clipped to the plane, lie in the band's conv rows [C0, C1) (band_plan)
        const int pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2, NPo = (br.P1 - br.P0) * g.pw, NP = nrow * NPo;
        const any_div dNPo = make_div(NPo);
        for (int i = tid; i < NP; i += SS_THREADS) {
            const int col = fdiv(i, dNPo), pp = i - col * NPo, pyl = fdiv(pp, g.dPW), px = pp - pyl * g.pw, py = br.P0 + pyl;
            const float *vc = vpl + col * NPb;
            float mx = -INFINITY;
            for (int dy = 0; dy < g.pool_h; ++dy) {
                const int yy = py * g.pool_h - pph + dy;
                if (yy < br.C0 || yy >= br.C1) continue;
                for (int dx = 0; dx < g.pool_w; ++dx) {
                    const int xx = px * g.pool_w - ppw + dx;
                    if (xx < 0 || xx >= g.cw) continue;
                    mx = fmaxf(mx, vc[(yy - br.C0) * g.cw + xx]);
                }
            }
            const long o = (b * g.c_out + co0 + col) * g.PP + py * g.pw + px;
            out_s[o] = mx > 0.0f ? 1.0f : 0.0f;
            out_pv[o] = sigmoidf_dev(mx);
        }
    }
}

template <bool R, bool POOL>
static int launch_step_slab(const step_slab_geom &g, int ns, size_t lds_bytes, const float *wperm, const float *b,
                            const float *eps1, float *arp, float *out_s, float *out_pv, float *out_v, int B, float alpharp,
                            float wrp, hipStream_t st, const char *name, bool launch)
{
    // dynamic LDS above 64 KiB is reserved per template instance AND device (launch_step_wide's rule): asked for again only when
    // a call needs more than any before it on this device, so no attribute call falls inside a capture
    static std::mutex mu;
    static size_t reserved[SS_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_step_slab: no current device");
    }
    if (lds_bytes > 64 * 1024) {
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= SS_MAX_DEVICES || lds_bytes > reserved[dev]) {       // (a device beyond the table: asked for on every call)
            if (hipFuncSetAttribute((const void *)k_lif_step_slab<R, POOL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(DCLL_ERR_LAUNCH, "k_lif_step_slab: cannot reserve its LDS");
            }
            if (dev < SS_MAX_DEVICES) reserved[dev] = lds_bytes;
        }
    }
    if (!launch) return DCLL_OK;
    hipLaunchKernelGGL((k_lif_step_slab<R, POOL>), dim3((unsigned)B, (unsigned)g.nb, (unsigned)ns), dim3(SS_THREADS), lds_bytes, st,
                       g, wperm, b, eps1, arp, out_s, out_pv, out_v, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

// the layer kernel of a planned call (dcll_step_slab_plan: nb bands, ns slabs; the caller has run k_trace).  launch == false:
// everything that can fail short of the launch itself — the geometry, the layout and grid checks, the LDS reservation — and
// nothing else; the entry point calls this form first, so an error return never follows a launch
int dcll_launch_step_slab(const dcll_conv_desc *d, const float *wperm, const float *b, const float *eps1, float *arp,
                          float *out_s, float *out_pv, float *out_v, int nb, int ns, int32_t B, hipStream_t st, bool launch)
{
    const char *who = "dcll_conv_lif_step_slab";
    const bool pooled = step_slab_pooled(d);
    step_slab_geom g;
    g.c_in = d->c_in; g.c_out = d->c_out; g.h = d->h; g.w = d->w; g.kh = d->kh; g.kw = d->kw;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.pool_h = d->pool_h; g.pool_w = d->pool_w;
    g.WP = d->w + 2 * d->pad_w;
    conv_shape(d, &g.ch, &g.cw, &g.ph, &g.pw);
    g.CP = g.ch * g.cw;
    g.PP = g.ph * g.pw;
    g.npair = (int)any_chain_pairs(d);
    g.nsteps = (int)any_chain_steps(d);
    g.nb = nb;
    g.dWP = make_div(g.WP); g.dCW = make_div(g.cw); g.dPW = make_div(g.pw);
    if (nb < 1 || nb > g.ph || nb > 65535 || ns != slab_count(d->c_out) || ns > SLAB_MAX)
        return fail(DCLL_ERR_LAUNCH, "bad plan of bands and slabs", who);
    // the kernel's layout of every band (img, vpl, bias) against the ONE exported formula, the bands against the planes
    long mx = 0;
    int c_prev = 0, p_prev = 0;
    for (int k = 0; k < nb; ++k) {
        const band_rows r = band_plan(k, nb, d->h, d->kh, d->pad_h, d->pool_h, g.ch, g.ph);
        const long crows = r.C1 - r.C0, img = (long)d->c_in * (crows + d->kh - 1) * g.WP;
        const long fl = img + (pooled ? SLAB_ROWS * crows * g.cw : 0) + SLAB_ROWS;
        if (fl != step_slab_lds_floats(d, k, nb)) return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_step_slab_lds disagree", who);
        if (r.C0 != c_prev || r.P0 != p_prev || r.C1 <= r.C0 || r.P1 <= r.P0)
            return fail(DCLL_ERR_LAUNCH, "the bands do not partition the rows", who);
        c_prev = r.C1;
        p_prev = r.P1;
        if (fl > mx) mx = fl;
    }
    if (c_prev != g.ch || p_prev != g.ph) return fail(DCLL_ERR_LAUNCH, "the bands do not partition the rows", who);
    if (mx * 4 > ANY_LDS_MAX) return fail(DCLL_ERR_LAUNCH, "a band exceeds the 160 KiB of LDS", who);
    if ((long)B * nb * ns > 0x7fffffffL / SS_THREADS / 2) return fail(DCLL_ERR_UNSUPPORTED, "B x bands x slabs exceeds the grid", who);
    const size_t lds_bytes = (size_t)mx * 4;
#define DCLL_SS(R_, P_, name_) \
    return launch_step_slab<R_, P_>(g, ns, lds_bytes, wperm, b, eps1, arp, out_s, out_pv, out_v, B, d->alpharp, d->wrp, st, name_, launch)
    if (d->refractory) {
        if (pooled) DCLL_SS(1, 1, "k_lif_step_slab<1> (pooling)");
        DCLL_SS(1, 0, "k_lif_step_slab<1>");
    }
    if (pooled) DCLL_SS(0, 1, "k_lif_step_slab<0> (pooling)");
    DCLL_SS(0, 0, "k_lif_step_slab<0>");
#undef DCLL_SS
}
