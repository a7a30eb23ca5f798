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
// Band plan: band_plan() of dcll_any_shared.h along the rows (tests/seq_band_cases.py restates it).  Band k of NB owns pooled rows
// [P0, P1), computes conv rows [C0, C1), holds input rows [I0, I1) and writes the final eps0 / eps1 of input rows [O0, O1); arp,
// v_out of a conv pixel and pv, spike bit of a pooled pixel have one owner by construction.
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
// Arithmetic and phases are k_lif_seq_wide's (MT = 2) / k_lif_seq_any's (MT = 1).  Chain length, weight permutation, weights-in-LDS
// budget, the launch prologue and the device code this kernel shares with k_lif_seq_tile (chain, to_vpl, phase C, constant
// prologue) come from dcll_any_shared.h.  Phases: A traces + pooling pass of t - 1 | B chains -> vpl | C refractory update + v_out,
// a barrier behind each.  The units of a band are (32-pixel tile of the band's flattened conv rows, M tile): with at least 8 tiles a
// wave runs all MT chains of a tile on one B read; with fewer, units go one per wave (an 8-wave workgroup with two tiles runs four
// chains at once).  Either way every output's chain is whole and in order.
#include "dcll_any_shared.h"

constexpr int BAND_THREADS = 512, BAND_NW = BAND_THREADS / 64;
constexpr int BAND_MAX_COUT = 64;

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

// n bands fit: one band = the one-workgroup kernels' own predicate; more = the largest band's set within the LDS
static bool band_fits(const dcll_conv_desc *d, int n)
{
    if (n == 1) return dcll_conv_lif_sequence_wide_lds(d) > 0;
    return band_floats_max(d, n) * 4 <= ANY_LDS_MAX;
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
        if (best && (long)B * n > ANY_CUS) break;
        best = n;
        const int tiles = band_tiles_max(d, n);
        if (n == 1 ? band_mt(d) * ((tiles + BAND_NW - 1) / BAND_NW) == 1 : tiles <= 1) break;
    }
    return best;
}

// the band count a call runs (0: refused, rc and the message set)
static int band_count(const dcll_conv_desc *d, int B, int bands, const char *who, int *rc)
{
    *rc = any_layer_ok(d, BAND_MAX_COUT, who);
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
    return any_chain_steps(d) * 64 * band_mt(d) + 2L * B * d->c_in * d->h * d->w;
}

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
    const any_div dHBW = make_div(HBW), dCPb = make_div(L.CPb);

    // position of held input element i (channel ci, band pixel p = (y - I0) w + x) in img
    auto img_at = [&](int i, int &ci, int &p) -> int {
        ci = fdiv(i, dHBW);
        p = i - ci * HBW;
        const int yl = fdiv(p, g.dW), x = p - yl * g.w;
        return ci * L.CHS + (r.I0 + yl + g.pad_h - r.C0) * g.WP + x + g.pad_w;
    };

    // conv element i (channel co, band pixel) -> its pixel in the sample's conv plane
    auto conv_at = [&](int i, int &co) -> int {
        co = fdiv(i, dCPb);
        return cp0 + i - co * L.CPb;
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
            int co;
            const int cp = conv_at(i, co);
            arps[i] = arp_g[b * NV + co * g.CP + cp];
        }
    any_consts_to_lds<MT, WLDS, BAND_THREADS>(taus, sb, wl, tau4, bias, wperm, g.c_in, g.c_out, g.nsteps, g.nwl, tid);
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

    // NM chains (M tiles mt0 .. mt0 + NM - 1) of pixel tile tl of the band
    auto chain = [&](auto nm_, int tl, int mt0) {
        const int pix = tl * 32 + j, pc = pix < L.CPb ? pix : L.CPb - 1, y = fdiv(pc, g.dCW), x = pc - y * g.cw;
        return any_chain<decltype(nm_)::value, MT, WLDS>(img, g.WP, L.CHS, y * g.WP + x, sb, wl, wperm, g.nwl, g.npair, g.nsteps,
                                                         g.c_in, g.kh, g.kw, lane, hh, mt0);
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
                const any_acc<MT> acc = chain(std::integral_constant<int, MT>{}, tl, 0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) any_to_vpl(acc.t[mt], vpl, L.CPb, g.c_out, tl * 32 + j, mt, hh);
            }
        } else {
            for (int u = wv; u < NTL * MT; u += BAND_NW) {       // few tiles: one (tile, M tile) per wave
                const int tl = u / MT, mt = u - tl * MT;
                const any_acc<1> acc = chain(std::integral_constant<int, 1>{}, tl, mt);
                any_to_vpl(acc.t[0], vpl, L.CPb, g.c_out, tl * 32 + j, mt, hh);
            }
        }
        __syncthreads();
        // ---- phase C: refractory update on the v plane, v_out
        any_phase_c<R, BAND_THREADS>(vpl, arps, NVb, v_out, ob, g.CP, tid, alpharp, wrp, conv_at);
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
            int co;
            const int cp = conv_at(i, co);
            arp_g[b * NV + co * g.CP + cp] = arps[i];
        }
}

// the LDS reservation, then the weight permutation, the snapshot, the zero fill, then the kernel: an error return never follows
// a launch of the layer kernel
template <int MT, bool R, bool WLDS>
static int launch_band(const dcll_conv_desc *d, const band_geom &g, size_t lds_bytes, bool shared_words, const uint32_t *spk_in,
                       const float *W, float *scratch, const float *b, const float *tau4, float *eps0, float *eps1, float *arp,
                       uint32_t *spk_out, float *pv_out, float *v_out, int T, int B, float alpharp, float wrp, hipStream_t st, const char *name)
{
    if (hipFuncSetAttribute((const void *)k_lif_seq_band<MT, R, WLDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_seq_band: cannot reserve its LDS");
    }
    float *snap0, *snap1;
    const int rc = seq_split_prepare(d, W, scratch, MT, eps0, eps1, spk_out, (size_t)T * B * g.c_out * g.ow, shared_words, B, st,
                                     "k_lif_seq_band", &snap0, &snap1);
    if (rc) return rc;
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
    g.npair = (int)any_chain_pairs(d);
    g.nsteps = (int)any_chain_steps(d);
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
    if (base * 4 > ANY_LDS_MAX) return fail(DCLL_ERR_LAUNCH, "a band's LDS beyond the limit", who);
    g.o_w = (int)base;
    g.nwl = seq_weight_room(base, g.nsteps, MT, (long)B * NB);
    const bool wlds = g.nwl == g.nsteps;
    const size_t lds_bytes = (size_t)(base + (long)g.nwl * 64 * MT) * 4;

    // launch-log names: k_lif_seq_band<M tiles, refractory, weights in LDS>
#define DCLL_BAND(M_, R_, L_)                                                                                                   \
    return launch_band<M_, R_, L_>(d, g, lds_bytes, shared_words, spk_in, W, scratch, b, tau4, eps0, eps1, arp, spk_out, pv_out,  \
                                   v_out, T, B, d->alpharp, d->wrp, st, "k_lif_seq_band<" #M_ "," #R_ "," #L_ ">")
    DCLL_SEQ_SPLIT_DISPATCH(DCLL_BAND, MT, d->refractory, wlds);
#undef DCLL_BAND
}
