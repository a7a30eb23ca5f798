// dcll_seq_band.hip — k_lif_seq_band: all T timesteps of a plain conv layer (stride = dilation = groups = 1, c_out <= 64, kernel up
// to 16x16, any padding, any pooling) in one launch with SEVERAL workgroups per sample (dcll_conv_lif_sequence_bands).  Opt-in,
// beside k_lif_seq_any / k_lif_seq_wide, which put one sample on one workgroup: a small batch then leaves most of the card idle,
// and a per-sample state beyond one workgroup's 160 KiB of LDS is refused.  Here a sample is cut into NB bands of output rows;
// each band sits on its own workgroup for all T.  The conv of step t reads only the layer's input traces, and those are an
// elementwise function of the input spikes — so a band recomputes the traces of the halo rows it needs and nothing passes
// between workgroups during the sequence (the decomposition of DESIGN 4.1b, with the band count a run-time quantity).  Every v
// is still ONE unsplit chain in the pinned order: the results are bit-identical to the one-workgroup kernels.
// bands = 1 hands the call to dcll_conv_lif_sequence_wide unchanged.
//
// Band plan (band_plan() is the ONE statement of it; tests/seq_band_cases.py restates it):
//   band k of NB owns pooled rows [P0, P1) = [k ph / NB, (k + 1) ph / NB)                                     (floor)
//   conv rows  [C0, C1): the union of those pooling windows (py pool_h - (pool_h - 1) / 2 + dy) clipped to [0, ch); the last
//              band also takes the conv rows behind the last window (floor-mode pooling leaves such rows; their arp and v_out
//              exist).  C0(k + 1) == C1(k): the conv rows are a partition.
//   input rows held [I0, I1) = [C0 - pad_h, C1 - pad_h + kh - 1) clipped to [0, h]; rows outside the image are the zero padding
//   input rows owned [O0, O1) = [I0(k), I0(k + 1)) (last band: up to h): the one band that writes an element's final eps0 / eps1
//   arp, v_out of a conv pixel and pv, spike bit of a pooled pixel have one owner by construction.
//
// LDS of a band (floats; band_floats() is the ONE statement of it, exported as dcll_conv_lif_sequence_bands_lds for the largest
// band) — k_lif_seq_wide's LDS-form set on the band's rows:
//   img   c_in x (C1 - C0 + kh - 1) x (w + 2 pad_w)   eps1, zero padded
//   e0    c_in x (I1 - I0) x w                        eps0 of the held in-image rows
//   vpl   c_out x (C1 - C0) x cw                      v of ONE step at conv resolution
//   arp   c_out x (C1 - C0) x cw                      refractory layers only
//   tau   4 x c_in, bias 32 x MT
//   + behind the largest band's set as many permuted weight steps as fit (WLDS: all of them); the rest is streamed from L2.
// No register form.
//
// Two hazards:
//   halo reads against write-back — with a grid beyond residency a late band would read a neighbour's FINAL state as its initial
//     halo.  A stream-ordered device copy of eps0 / eps1 goes into the scratch in front of the launch; every initial read goes to
//     that snapshot, every write to the state (the rule of DESIGN 4.1b).
//   shared spike words — a band boundary need not fall on a multiple of 32 pooled pixels.  A band stores the words that lie wholly
//     inside its pixel range and ORs its bits into a boundary word (an ordinary vector atomicOr); when the plan has such a word the
//     launcher zero-fills spk_out on the stream first.  OR is commutative: the bits do not depend on the order.
//
// Arithmetic, weight permutation and phases are k_lif_seq_wide's (MT = 2) / k_lif_seq_any's (MT = 1), restated here: chain of
// output (co, y, x) from bias[co] over the links (cp, ky, kx, h), one v_mfma_f32_32x32x2_f32 per two consecutive links; phases
// A traces + pooling pass of t - 1 | B chains -> vpl | C refractory update + v_out, a barrier behind each.  The units of a band
// are (32-pixel tile of the band's flattened conv rows, M tile): with at least 8 tiles a wave runs all MT chains of a tile on one
// B read; with fewer, units go one per wave (an 8-wave workgroup with two tiles runs four chains at once).  Either way every
// output's chain is whole and in order.
#include "dcll_internal.h"

constexpr int BAND_THREADS = 512, BAND_NW = BAND_THREADS / 64;
constexpr long BAND_LDS_MAX = 160 * 1024;
constexpr int BAND_MAX_K = 16, BAND_MAX_COUT = 64;
constexpr int BAND_CUS = 256;       // the default rule's device: an MI355X

struct band_rows {
    int P0, P1, C0, C1, I0, I1, O0, O1;
};

// the band plan: rows of band k of NB (1 <= NB <= ph)
__host__ __device__ static inline band_rows band_plan(int k, int NB, int h, int kh, int pad_h, int pool_h, int ch, int ph)
{
    const int pph = (pool_h - 1) / 2;
    band_rows r;
    r.P0 = (int)((long)k * ph / NB);
    r.P1 = (int)((long)(k + 1) * ph / NB);
    const int c0 = r.P0 * pool_h - pph, c1 = r.P1 * pool_h - pph;   // first conv row of the windows of pooled rows P0, P1
    r.C0 = c0 < 0 ? 0 : c0;
    r.C1 = (k == NB - 1) ? ch : (c1 < 0 ? 0 : c1);                  // (P1 < ph: c1 < ch)
    const int i0 = r.C0 - pad_h, i1 = r.C1 - pad_h + kh - 1;
    r.I0 = i0 < 0 ? 0 : (i0 > h ? h : i0);
    r.I1 = i1 < 0 ? 0 : (i1 > h ? h : i1);
    const int o1 = r.C1 - pad_h;                                    // = I0 of band k + 1
    r.O0 = r.I0;
    r.O1 = (k == NB - 1) ? h : (o1 < 0 ? 0 : (o1 > h ? h : o1));
    return r;
}

struct band_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int WP;                     // padded row length of img
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane of the whole sample
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int nwl;                    // chain steps whose weights are kept in LDS (WLDS: all of them)
    int iw, ow;                 // words per input / output spike plane
    int o_w;                    // float offset of the weights in LDS: the largest band's set
    int NB;
    any_div dW, dCW, dPW;
};

// float offsets into a band's LDS (img at 0)
struct band_lay {
    int RB, CHS, HB, CPb, o_e0, o_v, o_arp, o_tau, o_bias, end;
};
__host__ __device__ static inline band_lay band_layout(const band_rows &r, int c_in, int c_out, int w, int WP, int cw, int kh, int mt,
                                                       bool refr)
{
    band_lay L;
    L.RB = r.C1 - r.C0 + kh - 1;
    L.CHS = L.RB * WP;
    L.HB = r.I1 - r.I0;
    L.CPb = (r.C1 - r.C0) * cw;
    L.o_e0 = c_in * L.CHS;
    L.o_v = L.o_e0 + c_in * L.HB * w;
    L.o_arp = L.o_v + c_out * L.CPb;
    L.o_tau = L.o_arp + (refr ? c_out * L.CPb : 0);
    L.o_bias = L.o_tau + 4 * c_in;
    L.end = L.o_bias + 32 * mt;
    return L;
}

static inline int band_mt(const dcll_conv_desc *d) { return (d->c_out + 31) / 32; }

// the working set of band k of NB in floats, without the weights
static inline long band_floats(const dcll_conv_desc *d, int k, int NB)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const band_rows r = band_plan(k, NB, d->h, d->kh, d->pad_h, d->pool_h, ch, ph);
    const long img = (long)d->c_in * (r.C1 - r.C0 + d->kh - 1) * (d->w + 2 * d->pad_w);
    const long e0 = (long)d->c_in * (r.I1 - r.I0) * d->w;
    const long vpl = (long)d->c_out * (r.C1 - r.C0) * cw;
    return img + e0 + vpl * (d->refractory ? 2 : 1) + 4L * d->c_in + 32 * band_mt(d);
}
static inline long band_floats_max(const dcll_conv_desc *d, int NB)
{
    long m = 0;
    for (int k = 0; k < NB; ++k) {
        const long f = band_floats(d, k, NB);
        if (f > m) m = f;
    }
    return m;
}
static inline long band_steps(const dcll_conv_desc *d)
{
    const long KK = (long)d->kh * d->kw;
    return (d->c_in / 2) * KK + ((d->c_in & 1) ? (KK + 1) / 2 : 0);
}

// the layers this file serves or forwards, whatever the band count
static int band_layer_ok(const dcll_conv_desc *d, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->c_out > BAND_MAX_COUT) return fail(DCLL_ERR_UNSUPPORTED, "c_out <= 64 (two 32-row MFMA tiles of output channels)", who);
    if (d->kh > BAND_MAX_K || d->kw > BAND_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    return DCLL_OK;
}
// n bands fit: one band = the one-workgroup kernels' own predicate; more = the largest band's set within the LDS
static bool band_fits(const dcll_conv_desc *d, int n)
{
    if (n == 1) return dcll_conv_lif_sequence_wide_lds(d) > 0;
    return band_floats_max(d, n) * 4 <= BAND_LDS_MAX;
}
// pixel tiles of the largest band
static int band_tiles_max(const dcll_conv_desc *d, int NB)
{
    int ch, cw, ph, pw, m = 0;
    conv_shape(d, &ch, &cw, &ph, &pw);
    for (int k = 0; k < NB; ++k) {
        const band_rows r = band_plan(k, NB, d->h, d->kh, d->pad_h, d->pool_h, ch, ph);
        const int t = ((r.C1 - r.C0) * cw + 31) / 32;
        if (t > m) m = t;
    }
    return m;
}

// The default rule (bands = 0), set from the sweep of profiles/r22_seq_band_timing.txt: the smallest band count
// that fits, raised while the grid stays within one round of the card (B n <= 256 CUs) — more bands than that lost in every cell
// of the sweep (B = 512; 8 bands at B = 64) — and not beyond the count at which more bands stopped paying: one band when the
// one-workgroup kernel already runs ONE chain per wave (MT ceil(tiles / 8) == 1: mnist_conv.yaml's 16 -> 24 and 24 -> 32 layers,
// not beaten by 2 or 4 bands at B = 32), several bands down to one pixel tile per band.  0: no band count fits.
static int band_rule(const dcll_conv_desc *d, int B)
{
    int ch, cw, ph, pw, best = 0;
    conv_shape(d, &ch, &cw, &ph, &pw);
    for (int n = 1; n <= ph; ++n) {
        if (!band_fits(d, n)) continue;
        if (best && (long)B * n > BAND_CUS) break;
        best = n;
        const int tiles = band_tiles_max(d, n);
        if (n == 1 ? band_mt(d) * ((tiles + BAND_NW - 1) / BAND_NW) == 1 : tiles <= 1) break;
    }
    return best;
}

// the band count a call runs (0: refused, rc and the message set)
static int band_count(const dcll_conv_desc *d, int B, int bands, const char *who, int *rc)
{
    *rc = band_layer_ok(d, who);
    if (*rc) return 0;
    if (bands < 0) {
        *rc = fail(DCLL_ERR_INVALID, "negative band count", who);
        return 0;
    }
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (bands > ph) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "bands > ph: a band owns at least one pooled row", who);
        return 0;
    }
    if (bands == 0) {
        const int n = band_rule(d, B < 1 ? 1 : B);
        if (!n) *rc = fail(DCLL_ERR_UNSUPPORTED, "no band count brings the largest band's working set within the 160 KiB of LDS", who);
        return n;
    }
    if (bands == 1) {
        if (!band_fits(d, 1)) *rc = DCLL_ERR_UNSUPPORTED;      // (dcll_conv_lif_sequence_wide's message stands)
        return *rc ? 0 : 1;
    }
    if (!band_fits(d, bands)) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "the largest band's working set exceeds the 160 KiB of LDS at this band count", who);
        return 0;
    }
    return bands;
}

extern "C" int32_t dcll_conv_lif_sequence_bands_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int32_t *bounds)
{
    int rc;
    const int n = band_count(d, B, bands, "dcll_conv_lif_sequence_bands_plan", &rc);
    if (n && bounds) {
        int ch, cw, ph, pw;
        conv_shape(d, &ch, &cw, &ph, &pw);
        for (int k = 0; k <= n; ++k) bounds[k] = (int32_t)((long)k * ph / n);
    }
    return n;
}
extern "C" int64_t dcll_conv_lif_sequence_bands_lds(const dcll_conv_desc *d, int32_t bands)
{
    int rc;
    const int n = band_count(d, 1, bands, "dcll_conv_lif_sequence_bands_lds", &rc);
    if (!n) return 0;
    return n == 1 ? dcll_conv_lif_sequence_wide_lds(d) : band_floats_max(d, n) * 4;
}
extern "C" int64_t dcll_conv_lif_sequence_bands_scratch(const dcll_conv_desc *d, int32_t B)
{
    int rc;
    if (!band_count(d, B, 0, "dcll_conv_lif_sequence_bands_scratch", &rc) || B < 0) return 0;
    return band_steps(d) * 64 * band_mt(d) + 2L * B * d->c_in * d->h * d->w;
}

// W (c_out, c_in, kh, kw) -> wperm[m][mt][lane]: link 2 m + h of channel co = 32 mt + (lane & 31), h = lane >> 5; 0 beyond
// c_out / the chain
__global__ void k_seq_band_wprep(const float *__restrict__ W, float *__restrict__ wperm, int c_in, int c_out, int kh, int kw,
                                 int npair, int nsteps, int MT)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsteps * 64 * MT) return;
    const int lane = i & 63, u = i >> 6, mt = u % MT, m = u / MT, co = 32 * mt + (lane & 31), h = lane >> 5, KK = kh * kw;
    int ci, tap;
    if (m < npair) {
        ci = 2 * (m / KK) + h;
        tap = m % KK;
    } else {
        ci = c_in - 1;
        tap = 2 * (m - npair) + h;
    }
    wperm[i] = (co < c_out && tap < KK) ? W[((long)co * c_in + ci) * KK + tap] : 0.0f;
}

template <int NM>
struct band_acc {
    f32x16 t[NM];
};

__device__ __forceinline__ any_div band_div(int d) { return any_div{d > 1 ? (uint32_t)(((1ull << 32) + d - 1) / d) : 0u, d}; }

template <int MT, bool R, bool WLDS>
__global__ __launch_bounds__(BAND_THREADS) void k_lif_seq_band(const band_geom g, const uint32_t *__restrict__ spk_in,
                                                              const float *__restrict__ wperm, const float *__restrict__ bias,
                                                              const float *__restrict__ tau4, const float *__restrict__ eps0_snap,
                                                              const float *__restrict__ eps1_snap, float *__restrict__ eps0_g,
                                                              float *__restrict__ eps1_g, float *__restrict__ arp_g,
                                                              uint32_t *__restrict__ spk_out, float *__restrict__ pv_out,
                                                              float *__restrict__ v_out, int T, int B, float alpharp, float wrp)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x % g.NB;
    const long b = blockIdx.x / g.NB;
    const band_rows r = band_plan(k, g.NB, g.h, g.kh, g.pad_h, g.pool_h, g.ch, g.ph);
    const band_lay L = band_layout(r, g.c_in, g.c_out, g.w, g.WP, g.cw, g.kh, MT, R);
    float *img = lds, *e0s = lds + L.o_e0, *vpl = lds + L.o_v, *arps = lds + L.o_arp, *taus = lds + L.o_tau, *sb = lds + L.o_bias,
          *wl = lds + g.o_w;
    const int HW = g.h * g.w, NIN = g.c_in * HW, NV = g.c_out * g.CP;
    const int HBW = L.HB * g.w, NINb = g.c_in * HBW, NVb = g.c_out * L.CPb, NTL = (L.CPb + 31) >> 5;
    const int pg0 = r.I0 * g.w, cp0 = r.C0 * g.cw;             // first held input pixel, first conv pixel, of the sample's planes
    const any_div dHBW = band_div(HBW), dCPb = band_div(L.CPb);

    // position of held input element i (channel ci, band pixel p = (y - I0) w + x) in img
    auto img_at = [&](int i, int &ci, int &p) -> int {
        ci = fdiv(i, dHBW);
        p = i - ci * HBW;
        const int yl = fdiv(p, g.dW), x = p - yl * g.w;
        return ci * L.CHS + (r.I0 + yl + g.pad_h - r.C0) * g.WP + x + g.pad_w;
    };

    // ---- prologue: the band's state (from the snapshot) and constants on chip
    for (int i = tid; i < g.c_in * L.CHS; i += BAND_THREADS) img[i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < NINb; i += BAND_THREADS) {
        int ci, p;
        const int q = img_at(i, ci, p);
        const long gi = b * NIN + ci * HW + pg0 + p;
        e0s[i] = eps0_snap[gi];
        img[q] = eps1_snap[gi];
    }
    if (R)
        for (int i = tid; i < NVb; i += BAND_THREADS) {
            const int co = fdiv(i, dCPb), pl = i - co * L.CPb;
            arps[i] = arp_g[b * NV + co * g.CP + cp0 + pl];
        }
    for (int i = tid; i < 4 * g.c_in; i += BAND_THREADS) taus[i] = tau4[i];
    if (tid < 32 * MT) sb[tid] = (bias && tid < g.c_out) ? bias[tid] : 0.0f;
    for (int i = tid; i < (WLDS ? g.nsteps : g.nwl) * 64 * MT; i += BAND_THREADS) wl[i] = wperm[i];
    __syncthreads();

    // the trace update of held input element i at step t (eps0 in e0s, eps1 in place in img)
    auto trace = [&](const uint32_t *sp, int i) {
        int ci, p;
        const int q = img_at(i, ci, p), pg = pg0 + p;
        const float xin = (float)((sp[ci * g.iw + (pg >> 5)] >> (pg & 31)) & 1u);
        float e0 = e0s[i], e1 = img[q];
        trace_update(xin, taus[ci], taus[g.c_in + ci], taus[2 * g.c_in + ci], taus[3 * g.c_in + ci], e0, e1);
        e0s[i] = e0;
        img[q] = e1;
    };

    // NM chains (M tiles mt0 .. mt0 + NM - 1) of pixel tile tl of the band: one B operand read per step for all of them
    auto chain = [&](auto nm_, int tl, int mt0) {
        constexpr int NM = decltype(nm_)::value;
        const int pix = tl * 32 + j, pc = pix < L.CPb ? pix : L.CPb - 1, y = fdiv(pc, g.dCW), x = pc - y * g.cw;
        const int base0 = y * g.WP + x;
        const float *bp = img + base0 + hh * L.CHS;
        band_acc<NM> acc;
#pragma unroll
        for (int n = 0; n < NM; ++n)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc.t[n][q] = sb[32 * (mt0 + n) + (q & 3) + 8 * (q >> 2) + 4 * hh];
        auto wa = [&](int m, int n) -> float {
            const int o = (m * MT + mt0 + n) * 64 + lane;
            if constexpr (WLDS) return wl[o];
            else return m < g.nwl ? wl[o] : wperm[o];
        };
        int m = 0, off = 0, kx = 0, ky = 0;
        // the weights of eight steps are requested a whole batch ahead of their use: the streamed ones come from L2, and a wave
        // that waited for every batch in turn spent its chain on that latency (16 steps in flight per M tile)
        float a[NM][8], an[NM][8];
        auto fetch = [&](float (&dst)[NM][8], int m0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int mu = m0 + u < g.npair ? m0 + u : g.npair - 1;
#pragma unroll
                for (int n = 0; n < NM; ++n) dst[n][u] = wa(mu, n);
            }
        };
        if (g.npair > 0) fetch(an, 0);
        for (; m < g.npair; m += 8) {       // (cp, ky, kx): both channels of the pair at one wave-uniform offset
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int n = 0; n < NM; ++n) a[n][u] = an[n][u];
            if (m + 8 < g.npair) fetch(an, m + 8);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (m + u < g.npair) {
                    const float bv = bp[off];
#pragma unroll
                    for (int n = 0; n < NM; ++n) acc.t[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[n][u], bv, acc.t[n], 0, 0, 0);
                    ++off;
                    if (++kx == g.kw) {
                        kx = 0;
                        off += g.WP - g.kw;
                        if (++ky == g.kh) {
                            ky = 0;
                            off += 2 * L.CHS - g.kh * g.WP;
                        }
                    }
                }
            }
        }
        m = g.npair;
        if (g.c_in & 1) {                   // the last channel alone: taps (2 q, 2 q + 1), tap KK (odd KK) is the zero link
            const float *cb = img + (g.c_in - 1) * L.CHS + base0;
            const int KK = g.kh * g.kw;
            int tap = hh, tkx = hh, tky = 0;
            while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            for (; m < g.nsteps; ++m) {
                const float bv = tap < KK ? cb[tky * g.WP + tkx] : 0.0f;
#pragma unroll
                for (int n = 0; n < NM; ++n) acc.t[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa(m, n), bv, acc.t[n], 0, 0, 0);
                tap += 2;
                tkx += 2;
                while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            }
        }
        return acc;
    };
    auto to_vpl = [&](const f32x16 &acc, int tl, int mt) {
        const int pix = tl * 32 + j;
        if (pix < L.CPb) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = 32 * mt + (q & 3) + 8 * (q >> 2) + 4 * hh;
                if (co < g.c_out) vpl[co * L.CPb + pix] = acc[q];
            }
        }
    };

    // pooling pass of step t over vpl: a half wave = the 32 pixels of one spike word of one channel, over the words that hold a
    // pooled pixel of the band.  A word wholly inside the band's range [plo, phi) is stored, a boundary word ORed.
    const int plo = r.P0 * g.pw, phi = r.P1 * g.pw, w0 = plo >> 5, nwb = ((phi + 31) >> 5) - w0;
    auto pool_pass = [&](int t) {
        if (!spk_out && !pv_out) return;
        const int units = g.c_out * nwb, pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2;
        const long ob = ((long)t * B + b) * g.c_out;
        for (int u0 = 2 * wv; u0 < units; u0 += 2 * BAND_NW) {
            const int u = u0 + hh;
            const bool uv = u < units;
            const int uc = uv ? u : 0, co = uc / nwb, wi = w0 + uc - co * nwb, pp = wi * 32 + j;
            const bool pvld = uv && pp >= plo && pp < phi;
            const int ppc = pvld ? pp : plo, py = fdiv(ppc, g.dPW), px = ppc - py * g.pw;
            const float *vc = vpl + co * L.CPb;
            float m = -INFINITY;
            for (int dy = 0; dy < g.pool_h; ++dy) {
                const int yy = py * g.pool_h - pph + dy;
                if (yy < r.C0 || yy >= r.C1) continue;          // (inside the band: outside [0, ch) only)
                for (int dx = 0; dx < g.pool_w; ++dx) {
                    const int xx = px * g.pool_w - ppw + dx;
                    if (xx < 0 || xx >= g.cw) continue;
                    m = fmaxf(m, vc[(yy - r.C0) * g.cw + xx]);
                }
            }
            const unsigned long long mk = __ballot(pvld && m > 0.0f);
            if (pvld && pv_out) pv_out[(ob + co) * g.PP + pp] = sigmoidf_dev(m);
            if (spk_out && uv && j == 0) {
                const uint32_t bits = (uint32_t)(hh ? mk >> 32 : mk);
                const int wend = wi * 32 + 32 < g.PP ? wi * 32 + 32 : g.PP;
                uint32_t *dst = spk_out + (ob + co) * g.ow + wi;
                if (wi * 32 >= plo && wend <= phi) *dst = bits;
                else if (bits) atomicOr(dst, bits);
            }
        }
    };

    for (int t = 0; t < T; ++t) {
        const uint32_t *sp = spk_in + ((long)t * B + b) * g.c_in * g.iw;
        const long ob = ((long)t * B + b) * g.c_out;
        // ---- phase A: pooled outputs of the previous step; traces of this step, in place
        if (t > 0) pool_pass(t - 1);
        for (int i = tid; i < NINb; i += BAND_THREADS) trace(sp, i);
        __syncthreads();
        // ---- phase B: the chains -> vpl
        if (MT == 1 || NTL >= BAND_NW) {
            for (int tl = wv; tl < NTL; tl += BAND_NW) {
                const band_acc<MT> acc = chain(std::integral_constant<int, MT>{}, tl, 0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) to_vpl(acc.t[mt], tl, mt);
            }
        } else {
            for (int u = wv; u < NTL * MT; u += BAND_NW) {       // few tiles: one (tile, M tile) per wave
                const int tl = u / MT, mt = u - tl * MT;
                const band_acc<1> acc = chain(std::integral_constant<int, 1>{}, tl, mt);
                to_vpl(acc.t[0], tl, mt);
            }
        }
        __syncthreads();
        // ---- phase C: refractory update on the v plane, v_out
        if (R || v_out) {
            for (int i = tid; i < NVb; i += BAND_THREADS) {
                float v = vpl[i];
                if (R) {
                    float a = arps[i];
                    bool s;
                    v = refractory(v, a, alpharp, wrp, s);
                    arps[i] = a;
                    vpl[i] = v;
                }
                if (v_out) {
                    const int co = fdiv(i, dCPb), pl = i - co * L.CPb;
                    v_out[(ob + co) * g.CP + cp0 + pl] = v;
                }
            }
            __syncthreads();
        }
    }
    // ---- last step's pooled outputs; the owned state back to HBM
    pool_pass(T - 1);
    for (int i = tid; i < NINb; i += BAND_THREADS) {
        int ci, p;
        const int q = img_at(i, ci, p), y = r.I0 + fdiv(p, g.dW);
        if (y >= r.O0 && y < r.O1) {
            const long gi = b * NIN + ci * HW + pg0 + p;
            eps0_g[gi] = e0s[i];
            eps1_g[gi] = img[q];
        }
    }
    if (R)
        for (int i = tid; i < NVb; i += BAND_THREADS) {
            const int co = fdiv(i, dCPb), pl = i - co * L.CPb;
            arp_g[b * NV + co * g.CP + cp0 + pl] = arps[i];
        }
}

// the LDS reservation, then the weight permutation, the snapshot, the zero fill, then the kernel: an error return never follows
// a launch of the layer kernel
template <int MT, bool R, bool WLDS>
static int launch_band(const band_geom &g, size_t lds_bytes, bool shared_words, const uint32_t *spk_in, const float *W, float *scratch,
                       const float *b, const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                       float *v_out, int T, int B, float alpharp, float wrp, hipStream_t st, const char *name)
{
    if (hipFuncSetAttribute((const void *)k_lif_seq_band<MT, R, WLDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_seq_band: cannot reserve its LDS");
    }
    const int n = g.nsteps * 64 * MT;
    const size_t nin = (size_t)B * g.c_in * g.h * g.w;
    float *snap0 = scratch + n, *snap1 = snap0 + nin;
    hipLaunchKernelGGL(k_seq_band_wprep, dim3((n + 255) / 256), dim3(256), 0, st, W, scratch, g.c_in, g.c_out, g.kh, g.kw, g.npair,
                       g.nsteps, MT);
    hipError_t e = hipGetLastError();           // (not in the launch log, like k_seq_wide_wprep)
    if (e == hipSuccess) e = hipMemcpyAsync(snap0, eps0, nin * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(snap1, eps1, nin * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && shared_words && spk_out)
        e = hipMemsetAsync(spk_out, 0, (size_t)T * B * g.c_out * g.ow * sizeof(uint32_t), st);
    if (e != hipSuccess) {
        snprintf(dcll_err_buf(), DCLL_ERR_LEN, "k_lif_seq_band (weight permutation, state snapshot, zero fill): %s", hipGetErrorString(e));
        return DCLL_ERR_LAUNCH;
    }
    hipLaunchKernelGGL((k_lif_seq_band<MT, R, WLDS>), dim3((unsigned)((long)B * g.NB)), dim3(BAND_THREADS), lds_bytes, st, g, spk_in,
                       scratch, b, tau4, snap0, snap1, eps0, eps1, arp, spk_out, pv_out, v_out, T, B, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

extern "C" int dcll_conv_lif_sequence_bands(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                            const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out,
                                            float *pv_out, float *v_out, float *scratch, int32_t T, int32_t B, int32_t bands,
                                            void *stream)
{
    const char *who = "dcll_conv_lif_sequence_bands";
    if (T < 0 || B < 0) return fail(DCLL_ERR_INVALID, "negative T or B", who);
    if (T == 0 || B == 0) return DCLL_OK;
    int rc;
    const int NB = band_count(d, B, bands, who, &rc);
    if (!NB) return rc;
    // one band: the one-workgroup kernels, their launch-log names, their bits (the permuted weights are the scratch's prefix)
    if (NB == 1)
        return dcll_conv_lif_sequence_wide(d, spk_in, W, b, tau4, eps0, eps1, arp, spk_out, pv_out, v_out, scratch, T, B, stream);
    if (!spk_in || !W || !tau4 || !eps0 || !eps1 || !scratch) return fail(DCLL_ERR_INVALID, "null pointer", who);
    if (d->refractory && !arp) return fail(DCLL_ERR_INVALID, "refractory layer needs arp", who);
    if ((long)B * NB > 0x7fffffffL) return fail(DCLL_ERR_INVALID, "B x bands beyond the grid", who);
    hipStream_t st = (hipStream_t)stream;
    const int MT = band_mt(d);
    band_geom g;
    g.c_in = d->c_in; g.c_out = d->c_out; g.h = d->h; g.w = d->w; g.kh = d->kh; g.kw = d->kw;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.pool_h = d->pool_h; g.pool_w = d->pool_w;
    g.WP = d->w + 2 * d->pad_w;
    conv_shape(d, &g.ch, &g.cw, &g.ph, &g.pw);
    g.CP = g.ch * g.cw;
    g.PP = g.ph * g.pw;
    g.npair = (d->c_in / 2) * d->kh * d->kw;
    g.nsteps = (int)band_steps(d);
    g.iw = (d->h * d->w + 31) / 32;
    g.ow = (g.PP + 31) / 32;
    g.NB = NB;
    g.dW = make_div(d->w); g.dCW = make_div(g.cw); g.dPW = make_div(g.pw);
    // the layout of every band against the ONE exported formula; a boundary inside a spike word?
    long base = 0;
    bool shared_words = false;
    for (int k = 0; k < NB; ++k) {
        const band_rows r = band_plan(k, NB, d->h, d->kh, d->pad_h, d->pool_h, g.ch, g.ph);
        const band_lay L = band_layout(r, d->c_in, d->c_out, d->w, g.WP, g.cw, d->kh, MT, d->refractory != 0);
        if (L.end != band_floats(d, k, NB))
            return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_sequence_bands_lds disagree", who);
        if (L.end > base) base = L.end;
        if (k && (r.P0 * g.pw) % 32) shared_words = true;
    }
    if (base * 4 > BAND_LDS_MAX) return fail(DCLL_ERR_LAUNCH, "a band's LDS beyond the limit", who);
    g.o_w = (int)base;
    // weights that do not fit as a whole: a grid of more than one workgroup per CU keeps half of the LDS free so that two bands
    // share a CU (the rule of k_lif_seq_any)
    const long per = 64 * MT;
    const bool whole = (base + (long)g.nsteps * per) * 4 <= BAND_LDS_MAX;
    const long budget = (!whole && (long)B * NB > BAND_CUS && base * 4 * 2 <= BAND_LDS_MAX) ? BAND_LDS_MAX / 2 : BAND_LDS_MAX;
    const long room = (budget / 4 - base) / per;
    g.nwl = (int)(room < g.nsteps ? room : g.nsteps);
    const bool wlds = g.nwl == g.nsteps;
    const size_t lds_bytes = (size_t)(base + (long)g.nwl * per) * 4;

    // launch-log names: k_lif_seq_band<M tiles, refractory, weights in LDS>
#define DCLL_BAND(M_, R_, L_)                                                                                                   \
    return launch_band<M_, R_, L_>(g, lds_bytes, shared_words, spk_in, W, scratch, b, tau4, eps0, eps1, arp, spk_out, pv_out,   \
                                   v_out, T, B, d->alpharp, d->wrp, st, "k_lif_seq_band<" #M_ "," #R_ "," #L_ ">")
    if (MT == 1) {
        if (d->refractory) {
            if (wlds) DCLL_BAND(1, 1, 1);
            DCLL_BAND(1, 1, 0);
        }
        if (wlds) DCLL_BAND(1, 0, 1);
        DCLL_BAND(1, 0, 0);
    }
    if (d->refractory) {
        if (wlds) DCLL_BAND(2, 1, 1);
        DCLL_BAND(2, 1, 0);
    }
    if (wlds) DCLL_BAND(2, 0, 1);
    DCLL_BAND(2, 0, 0);
#undef DCLL_BAND
}
