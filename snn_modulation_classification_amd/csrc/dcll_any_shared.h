// dcll_any_shared.h — what the any-shape sequence kernels (k_lif_seq_any, k_lif_seq_wide, k_lif_seq_band, k_lif_seq_tile) and
// their per-step twins state ONCE: the chain length, the link -> (channel, tap) map of the weight permutation, the layer predicate,
// the weights-in-LDS budget, the 1-D band plan, the launch prologue and dispatch of the kernels with several workgroups per sample
// and the constant part of their kernel prologue.  These kernels are bit-identical to each other (tiles == bands == wide == any),
// so a rule of the chain, the permutation or the budget has one place.  The permutation kernel itself (k_seq_any_wprep, run-time
// MT) is dcll_seq_any.hip's, behind dcll_launch_seq_wprep (dcll_internal.h).  Not part of the ABI.
#pragma once
#include "dcll_internal.h"

constexpr long ANY_LDS_MAX = 160 * 1024;    // LDS of a workgroup
constexpr int ANY_CUS = 256;                // the device of the batch rules: an MI355X
constexpr int ANY_MAX_K = 16;

// MFMA steps of a chain (two links each): the channel pairs of every tap, then the taps of an odd last channel two by two
static inline long any_chain_pairs(const dcll_conv_desc *d) { return (long)(d->c_in / 2) * d->kh * d->kw; }
static inline long any_chain_steps(const dcll_conv_desc *d)
{
    return any_chain_pairs(d) + ((d->c_in & 1) ? ((long)d->kh * d->kw + 1) / 2 : 0);
}

// the layers of these kernels, whatever the plane: plain conv, c_out <= max_cout (32 or 64), kernel up to 16x16
static inline int any_layer_ok(const dcll_conv_desc *d, int max_cout, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->c_out > max_cout)
        return fail(DCLL_ERR_UNSUPPORTED, max_cout <= 32 ? "c_out <= 32 (one 32-row MFMA tile of output channels)"
                                                         : "c_out <= 64 (two 32-row MFMA tiles of output channels)", who);
    if (d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    return DCLL_OK;
}

// The slab rule of the kernels that go past 64 output channels (k_bwd_wgrad_slab; tests/bwd_slab_cases.py restates it): output
// channels are independent of one another, so a layer of c_out > 64 channels is cut into NS = ceil(c_out / 64) slabs of two 32-row
// M tiles, one more grid dimension.  Slab s owns the channels [64 s, min(64 s + 64, c_out)); rows at or beyond c_out are never
// stored; a last slab of at most 32 channels has an empty second M tile.  The only new bound is the grid's: NS <= 65 535.
// A layer of c_out <= 64 is no slab layer: its entry point hands it to the 64-channel path unchanged.
constexpr int SLAB_ROWS = 64;
constexpr int SLAB_MAX = 65535;
__host__ __device__ static inline int slab_count(int c_out) { return (c_out + SLAB_ROWS - 1) / SLAB_ROWS; }
__host__ __device__ static inline int slab_first(int s) { return s * SLAB_ROWS; }
__host__ __device__ static inline int slab_rows(int s, int c_out)
{
    const int n = c_out - slab_first(s);
    return n < SLAB_ROWS ? n : SLAB_ROWS;
}

// chain step m, half h -> the link's input channel and tap (tap >= KK = kh kw: no link of the chain, its weight is 0)
__device__ __forceinline__ void any_link(int m, int h, int npair, int c_in, int KK, int &ci, int &tap)
{
    if (m < npair) {
        ci = 2 * (m / KK) + h;
        tap = m % KK;
    } else {
        ci = c_in - 1;
        tap = 2 * (m - npair) + h;
    }
}

// Chain steps whose permuted weights (64 MT floats each) are kept in LDS behind a working set of base_floats: all that fit.
// Weights that do not fit as a whole: a grid of more than one workgroup per CU keeps half of the LDS free so that two workgroups
// share a CU — measured on mnist_conv.yaml's third layer at B = 512.  LDS bytes = (base_floats + nwl 64 MT) 4.
static inline int seq_weight_room(long base_floats, int nsteps, int MT, long workgroups)
{
    const long per = 64 * MT;
    const bool whole = (base_floats + nsteps * per) * 4 <= ANY_LDS_MAX;
    const long budget = (!whole && workgroups > ANY_CUS && base_floats * 4 * 2 <= ANY_LDS_MAX) ? ANY_LDS_MAX / 2 : ANY_LDS_MAX;
    const long room = (budget / 4 - base_floats) / per;
    return (int)(room < nsteps ? room : nsteps);
}

// ------------------------------------------------------------------------------------------------------------
// several workgroups per sample (k_lif_seq_band: bands of rows; k_lif_seq_tile: the product of two such plans)
// ------------------------------------------------------------------------------------------------------------
struct band_rows {
    int P0, P1, C0, C1, I0, I1, O0, O1;
};

// The 1-D plan: part k of NB (1 <= NB <= ph) in one direction (tests/seq_band_cases.py and tests/seq_tile_cases.py restate it):
//   owned pooled pixels [P0, P1) = [k ph / NB, (k + 1) ph / NB)                                                 (floor)
//   conv pixels  [C0, C1): the union of those pooling windows (py pool_h - (pool_h - 1) / 2 + dy) clipped to [0, ch); the last
//                part also takes the conv pixels behind the last window (floor-mode pooling leaves such pixels; their arp and
//                v_out exist).  C0(k + 1) == C1(k): a partition.
//   input pixels held [I0, I1) = [C0 - pad_h, C1 - pad_h + kh - 1) clipped to [0, h]; outside the image is the zero padding
//   input pixels owned [O0, O1) = [I0(k), I0(k + 1)) (last part: up to h): the one part that writes an element's final eps0 / eps1
__host__ __device__ static inline band_rows band_plan(int k, int NB, int h, int kh, int pad_h, int pool_h, int ch, int ph)
{
    const int pph = (pool_h - 1) / 2;
    band_rows r;
    r.P0 = (int)((long)k * ph / NB);
    r.P1 = (int)((long)(k + 1) * ph / NB);
    const int c0 = r.P0 * pool_h - pph, c1 = r.P1 * pool_h - pph;   // first conv pixel of the windows of pooled pixels P0, P1
    r.C0 = c0 < 0 ? 0 : c0;
    r.C1 = (k == NB - 1) ? ch : (c1 < 0 ? 0 : c1);                  // (P1 < ph: c1 < ch)
    const int i0 = r.C0 - pad_h, i1 = r.C1 - pad_h + kh - 1;
    r.I0 = i0 < 0 ? 0 : (i0 > h ? h : i0);
    r.I1 = i1 < 0 ? 0 : (i1 > h ? h : i1);
    const int o1 = r.C1 - pad_h;                                    // = I0 of part k + 1
    r.O0 = r.I0;
    r.O1 = (k == NB - 1) ? h : (o1 < 0 ? 0 : (o1 > h ? h : o1));
    return r;
}

// In front of such a kernel, on the stream: the permuted weights into scratch[0, steps 64 MT), behind them the snapshots of eps0
// and eps1 every initial read goes to (*snap0, *snap1), and spk_out zeroed when workgroups share spike words (they OR into them).
// what: the layer kernel's name, for the message
static inline int seq_split_prepare(const dcll_conv_desc *d, const float *W, float *scratch, int MT, const float *eps0,
                                    const float *eps1, uint32_t *spk_out, size_t spk_words, bool shared_words, int B,
                                    hipStream_t st, const char *what, float **snap0, float **snap1)
{
    const size_t nin = (size_t)B * d->c_in * d->h * d->w;
    *snap0 = scratch + any_chain_steps(d) * 64 * MT;
    *snap1 = *snap0 + nin;
    char where[96];
    snprintf(where, sizeof where, "%s (weight permutation, state snapshot, zero fill)", what);
    int rc = dcll_launch_seq_wprep(d, W, scratch, MT, st, false, where);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(*snap0, eps0, nin * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(*snap1, eps1, nin * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && shared_words && spk_out) e = hipMemsetAsync(spk_out, 0, spk_words * sizeof(uint32_t), st);
    return e == hipSuccess ? DCLL_OK : fail(DCLL_ERR_LAUNCH, hipGetErrorString(e), where);
}

// the <M tiles, refractory, weights in LDS> ladder of k_lif_seq_band / k_lif_seq_tile; CALL(M, R, L) returns
#define DCLL_SEQ_SPLIT_DISPATCH(CALL, MT, refr, wlds) \
    do {                                              \
        if ((MT) == 1) {                              \
            if (refr) {                               \
                if (wlds) CALL(1, 1, 1);              \
                CALL(1, 1, 0);                        \
            }                                         \
            if (wlds) CALL(1, 0, 1);                  \
            CALL(1, 0, 0);                            \
        }                                             \
        if (refr) {                                   \
            if (wlds) CALL(2, 1, 1);                  \
            CALL(2, 1, 0);                            \
        }                                             \
        if (wlds) CALL(2, 0, 1);                      \
        CALL(2, 0, 0);                                \
    } while (0)

// ------------------------------------------------------------------------------------------------------------
// device code k_lif_seq_band and k_lif_seq_tile share (their index maps, pooling passes and write-backs are their own)
// ------------------------------------------------------------------------------------------------------------
// the constant part of the prologue: tau (4 x c_in), bias (32 MT, 0 beyond c_out) and the
// permuted weights kept on chip (WLDS: all steps, else the first nwl) into LDS
template <int MT, bool WLDS, int THREADS>
__device__ __forceinline__ void any_consts_to_lds(float *taus, float *sb, float *wl, const float *__restrict__ tau4,
                                                  const float *__restrict__ bias, const float *__restrict__ wperm, int c_in,
                                                  int c_out, int nsteps, int nwl, int tid)
{
    for (int i = tid; i < 4 * c_in; i += THREADS) taus[i] = tau4[i];
    if (tid < 32 * MT) sb[tid] = (bias && tid < c_out) ? bias[tid] : 0.0f;
    for (int i = tid; i < (WLDS ? nsteps : nwl) * 64 * MT; i += THREADS) wl[i] = wperm[i];
}

// the same for ONE SLAB of a wider layer (two M tiles on chip, nmt of them real): bias of the slab's nrow channels from co0 on,
// and the slab's columns of the layer's permutation (wps = wperm at the slab's first column, gmt M tiles per step in memory)
// re-packed to two per step; a column beyond the layer's last M tile does not exist in memory and is never read
template <bool WLDS, int THREADS>
__device__ __forceinline__ void any_consts_to_lds_slab(float *taus, float *sb, float *wl, const float *__restrict__ tau4,
                                                       const float *__restrict__ bias, const float *__restrict__ wps, int c_in,
                                                       int co0, int nrow, int nmt, int gmt, int nsteps, int nwl, int tid)
{
    for (int i = tid; i < 4 * c_in; i += THREADS) taus[i] = tau4[i];
    if (tid < 64) sb[tid] = (bias && tid < nrow) ? bias[co0 + tid] : 0.0f;
    for (int i = tid; i < (WLDS ? nsteps : nwl) * 128; i += THREADS) {
        const int m = i >> 7, mtl = (i >> 6) & 1;
        wl[i] = mtl < nmt ? wps[((long)m * gmt + mtl) * 64 + (i & 63)] : 0.0f;
    }
}

template <int NM>
struct any_acc {
    f32x16 t[NM];
};

// NM chains (M tiles mt0 .. mt0 + NM - 1 of MT) of the 32 conv pixels whose lane-j pixel has its first tap at img[base0]: rows of
// img are RS floats apart, channels CHS; one B operand read per step for all NM.  sb: bias; wl / wperm: the permuted weights in LDS
// (steps below nwl; WLDS: all) / in memory.  SLAB: wperm in MEMORY has gmt M tiles per step, not MT (a slab of a wider layer
// reads its MT columns of the layer's permutation: wperm then points at the slab's first column); the LDS copy has MT
template <int NM, int MT, bool WLDS, bool SLAB = false>
__device__ __forceinline__ any_acc<NM> any_chain(const float *img, int RS, int CHS, int base0, const float *sb, const float *wl,
                                                 const float *__restrict__ wperm, int nwl, int npair, int nsteps, int c_in, int kh,
                                                 int kw, int lane, int hh, int mt0, int gmt = MT)
{
    const float *bp = img + base0 + hh * CHS;
    any_acc<NM> acc;
#pragma unroll
    for (int n = 0; n < NM; ++n)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc.t[n][q] = sb[32 * (mt0 + n) + (q & 3) + 8 * (q >> 2) + 4 * hh];
    auto wa = [&](int m, int n) -> float {
        const int o = (m * MT + mt0 + n) * 64 + lane;
        if constexpr (WLDS) return wl[o];
        else if constexpr (SLAB) return m < nwl ? wl[o] : wperm[(m * gmt + mt0 + n) * 64 + lane];
        else return m < nwl ? wl[o] : wperm[o];
    };
    int m = 0, off = 0, kx = 0, ky = 0;
    // the weights of eight steps are requested a whole batch ahead of their use: the streamed ones come from L2, and a wave
    // that waited for every batch in turn spent its chain on that latency (16 steps in flight per M tile)
    float a[NM][8], an[NM][8];
    auto fetch = [&](float (&dst)[NM][8], int m0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int mu = m0 + u < npair ? m0 + u : npair - 1;
#pragma unroll
            for (int n = 0; n < NM; ++n) dst[n][u] = wa(mu, n);
        }
    };
    if (npair > 0) fetch(an, 0);
    for (; m < npair; m += 8) {         // (cp, ky, kx): both channels of the pair at one wave-uniform offset
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int n = 0; n < NM; ++n) a[n][u] = an[n][u];
        if (m + 8 < npair) fetch(an, m + 8);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (m + u < npair) {
                const float bv = bp[off];
#pragma unroll
                for (int n = 0; n < NM; ++n) acc.t[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[n][u], bv, acc.t[n], 0, 0, 0);
                ++off;
                if (++kx == kw) {
                    kx = 0;
                    off += RS - kw;
                    if (++ky == kh) {
                        ky = 0;
                        off += 2 * CHS - kh * RS;
                    }
                }
            }
        }
    }
    m = npair;
    if (c_in & 1) {                     // the last channel alone: taps (2 q, 2 q + 1), tap KK (odd KK) is the zero link
        const float *cb = img + (c_in - 1) * CHS + base0;
        const int KK = kh * kw;
        int tap = hh, tkx = hh, tky = 0;
        while (tkx >= kw) { tkx -= kw; ++tky; }
        for (; m < nsteps; ++m) {
            const float bv = tap < KK ? cb[tky * RS + tkx] : 0.0f;
#pragma unroll
            for (int n = 0; n < NM; ++n) acc.t[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa(m, n), bv, acc.t[n], 0, 0, 0);
            tap += 2;
            tkx += 2;
            while (tkx >= kw) { tkx -= kw; ++tky; }
        }
    }
    return acc;
}

// the accumulator of M tile mt for local conv pixel pix (this lane's of its 32-pixel tile) of NP -> vpl[co][pix]
__device__ __forceinline__ void any_to_vpl(const f32x16 &acc, float *vpl, int NP, int c_out, int pix, int mt, int hh)
{
    if (pix < NP) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = 32 * mt + (q & 3) + 8 * (q >> 2) + 4 * hh;
            if (co < c_out) vpl[co * NP + pix] = acc[q];
        }
    }
}

// phase C over the NVl elements of the workgroup's v plane: refractory update (arp in LDS), v_out; conv_at(i, co) -> the channel
// of element i and its pixel in the sample's conv plane of CP pixels.  A barrier behind it
template <bool R, int THREADS, class F>
__device__ __forceinline__ void any_phase_c(float *vpl, float *arps, int NVl, float *__restrict__ v_out, long ob, int CP, int tid,
                                            float alpharp, float wrp, F &&conv_at)
{
    if (R || v_out) {
        for (int i = tid; i < NVl; i += THREADS) {
            float v = vpl[i];
            if (R) {
                float a = arps[i];
                bool s;
                v = refractory(v, a, alpharp, wrp, s);
                arps[i] = a;
                vpl[i] = v;
            }
            if (v_out) {
                int co;
                const int cp = conv_at(i, co);
                v_out[(ob + co) * CP + cp] = v;
            }
        }
        __syncthreads();
    }
}
