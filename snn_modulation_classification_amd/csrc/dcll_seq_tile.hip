// dcll_seq_tile.hip — k_lif_seq_tile: all T timesteps of a plain conv layer (stride = dilation = groups = 1, c_out <= 64, kernel up
// to 16x16, any padding, any pooling) in one launch with a 2-D grid of NY x NX workgroups per sample
// (dcll_conv_lif_sequence_tiles).  Opt-in, beside k_lif_seq_band, whose bands span full rows: its LDS set grows with
// c_in kh (w + 2 pad_w), so a wide plane or a wide layer has no band count that fits.  Here a sample is cut in both directions.
// Each tile sits on its own workgroup for all T.  The conv of step t reads only the layer's input traces, and those are an
// elementwise function of the input spikes — so a tile recomputes the traces of the halo rows AND columns it needs and nothing
// passes between workgroups during the sequence.  Every v is still ONE unsplit chain in the pinned order: the results are
// bit-identical to k_lif_seq_band / k_lif_seq_wide / k_lif_seq_any wherever those serve the layer.
// tiles_x = 1 hands the call to dcll_conv_lif_sequence_bands unchanged (bands = tiles_y).
//
// Tile plan: the product of two 1-D band plans (band_plan() of dcll_any_shared.h; tests/seq_tile_cases.py restates it).  Tile (a, b)
// of NY x NX takes its rows from band_plan(a, NY, h, kh, pad_h, pool_h, ch, ph) and its columns from
// band_plan(b, NX, w, kw, pad_w, pool_w, cw, pw): owned pooled pixels [P0, P1), conv pixels [C0, C1), held input pixels [I0, I1),
// owned input pixels [O0, O1) in each direction.
// arp, v_out of a conv pixel and pv, spike bit of a pooled pixel have one owner by construction.
//
// LDS of a tile (floats; tile_floats() is the ONE statement of it, exported as dcll_conv_lif_sequence_tiles_lds for the largest
// tile), with CR x CC conv pixels and HR x HC held input pixels:
//   img   c_in x (CR + kh - 1) x (CC + kw - 1)   eps1, zero padded
//   e0    c_in x HR x HC                         eps0 of the held in-image pixels
//   vpl   c_out x CR x CC                        v of ONE step at conv resolution
//   arp   c_out x CR x CC                        refractory layers only
//   tau   4 x c_in, bias 32 x MT
//   + behind the largest tile's set as many permuted weight steps as fit (WLDS: all of them); the rest is streamed from L2.
// eps0 stays in LDS (no register form).
//
// The two hazards are k_lif_seq_band's: every initial read goes to a stream-ordered snapshot of eps0 / eps1 in the scratch, every
// write to the state; a tile's pooled pixels are row SEGMENTS of the flattened pooled plane, so almost every spike word is shared:
// a word wholly inside one segment is stored, every other word is ORed into (an ordinary vector atomicOr) after the launcher
// has zero-filled spk_out on the stream.  OR is commutative: the bits do not depend on the order.
//
// Arithmetic, weight prefetch, work split and phases are k_lif_seq_band's.  Chain length, weight permutation, weights-in-LDS budget,
// the launch prologue and the device code shared with k_lif_seq_band (chain, to_vpl, phase C, constant prologue) come from
// dcll_any_shared.h.  The units of a tile are (32-pixel tile of the tile's flattened conv pixels, M tile): with at least 8 pixel
// tiles a wave runs all MT chains of a pixel tile on one B read; with fewer, units go one per wave.
#include <vector>

#include "dcll_any_shared.h"

constexpr int TILE_THREADS = 512, TILE_NW = TILE_THREADS / 64;
constexpr int TILE_MAX_COUT = 64;

struct tile_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane of the whole sample
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int nwl;                    // chain steps whose weights are kept in LDS (WLDS: all of them)
    int iw, ow;                 // words per input / output spike plane
    int o_w;                    // float offset of the weights in LDS: the largest tile's set
    int NY, NX;
};

// float offsets into a tile's LDS (img at 0)
struct tile_lay {
    int RB, CB, CHS, HR, HC, CR, CC, CPt, o_e0, o_v, o_arp, o_tau, o_bias, end;
};
__host__ __device__ static inline tile_lay tile_layout(const band_rows &ry, const band_rows &rx, int c_in, int c_out, int kh, int kw,
                                                       int mt, bool refr)
{
    tile_lay L;
    L.CR = ry.C1 - ry.C0;
    L.CC = rx.C1 - rx.C0;
    L.RB = L.CR + kh - 1;
    L.CB = L.CC + kw - 1;
    L.CHS = L.RB * L.CB;
    L.HR = ry.I1 - ry.I0;
    L.HC = rx.I1 - rx.I0;
    L.CPt = L.CR * L.CC;
    L.o_e0 = c_in * L.CHS;
    L.o_v = L.o_e0 + c_in * L.HR * L.HC;
    L.o_arp = L.o_v + c_out * L.CPt;
    L.o_tau = L.o_arp + (refr ? c_out * L.CPt : 0);
    L.o_bias = L.o_tau + 4 * c_in;
    L.end = L.o_bias + 32 * mt;
    return L;
}

static inline int tile_mt(const dcll_conv_desc *d) { return (d->c_out + 31) / 32; }

// the working set in floats, without the weights, of a tile of CR x CC conv pixels that holds HR x HC input pixels
static inline long tile_floats(const dcll_conv_desc *d, long CR, long CC, long HR, long HC)
{
    const long img = d->c_in * (CR + d->kh - 1) * (CC + d->kw - 1);
    const long e0 = d->c_in * HR * HC;
    const long vpl = d->c_out * CR * CC;
    return img + e0 + vpl * (d->refractory ? 2 : 1) + 4L * d->c_in + 32 * tile_mt(d);
}

// one direction of a plan: the distinct (conv pixels, held pixels) of its parts and the sum of the held pixels
struct tile_axis {
    std::vector<std::pair<int, int>> kinds;
    long held;
};
static tile_axis tile_axis_of(int N, int h, int kh, int pad, int pool, int ch, int ph)
{
    tile_axis a;
    a.held = 0;
    for (int k = 0; k < N; ++k) {
        const band_rows r = band_plan(k, N, h, kh, pad, pool, ch, ph);
        const std::pair<int, int> p(r.C1 - r.C0, r.I1 - r.I0);
        a.held += p.second;
        bool seen = false;
        for (const auto &q : a.kinds) seen = seen || q == p;
        if (!seen) a.kinds.push_back(p);
    }
    return a;
}
// the largest tile's set of an NY x NX plan in floats; *held: the sum of held input pixels over all tiles (per channel)
static long tile_floats_max(const dcll_conv_desc *d, int NY, int NX, long *held = nullptr)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const tile_axis ay = tile_axis_of(NY, d->h, d->kh, d->pad_h, d->pool_h, ch, ph);
    const tile_axis ax = tile_axis_of(NX, d->w, d->kw, d->pad_w, d->pool_w, cw, pw);
    long m = 0;
    for (const auto &y : ay.kinds)
        for (const auto &x : ax.kinds) {
            const long f = tile_floats(d, y.first, x.first, y.second, x.second);
            if (f > m) m = f;
        }
    if (held) *held = ay.held * ax.held;
    return m;
}

static bool tile_fits(const dcll_conv_desc *d, int NY, int NX) { return tile_floats_max(d, NY, NX) * 4 <= ANY_LDS_MAX; }

// The (0, 0) rule where no band count serves the layer: the fitting (NY, NX), NX >= 2, with the fewest tiles; ties go to the
// smallest sum of held input elements over all tiles (the least recomputed trace work), then to the smaller NX.  DERIVED FROM THE
// LDS FORMULA ALONE — no measurement stands behind it.  false: no plan fits.
static bool tile_rule(const dcll_conv_desc *d, int *NY, int *NX)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    for (long n = 2; n <= (long)ph * pw; ++n) {
        long best = -1;
        for (int nx = 2; nx <= pw && nx <= n; ++nx) {
            if (n % nx || n / nx > ph) continue;
            long held;
            if (tile_floats_max(d, (int)(n / nx), nx, &held) * 4 > ANY_LDS_MAX) continue;
            if (best < 0 || held < best) {
                best = held;
                *NY = (int)(n / nx);
                *NX = nx;
            }
        }
        if (best >= 0) return true;
    }
    return false;
}

// the plan a call runs -> NY x NX (0: refused, rc and the message set).  *NX == 1: the call belongs to
// dcll_conv_lif_sequence_bands with bands = *bands
static int tile_count(const dcll_conv_desc *d, int B, int ty, int tx, const char *who, int *rc, int *NY, int *NX, int *bands)
{
    *rc = any_layer_ok(d, TILE_MAX_COUT, who);
    if (*rc) return 0;
    if (ty < 0 || tx < 0) {
        *rc = fail(DCLL_ERR_INVALID, "negative tile count", who);
        return 0;
    }
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (tx == 1 || (ty == 0 && tx == 0)) {
        const int n = dcll_conv_lif_sequence_bands_plan(d, B, ty, nullptr);
        if (n || tx == 1) {             // (tiles_x == 1: dcll_conv_lif_sequence_bands' code and message stand)
            *NY = *bands = n;
            *NX = 1;
            if (!n) *rc = DCLL_ERR_UNSUPPORTED;
            return n;
        }
        if (!tile_rule(d, NY, NX)) {
            *rc = fail(DCLL_ERR_UNSUPPORTED, "no tile plan brings the largest tile's working set within the 160 KiB of LDS", who);
            return 0;
        }
        return *NY * *NX;
    }
    if (ty == 0 || tx == 0) {
        *rc = fail(DCLL_ERR_INVALID, "a tile count of 0 in one direction only", who);
        return 0;
    }
    if (ty > ph || tx > pw) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "tiles_y > ph or tiles_x > pw: a tile owns at least one pooled pixel", who);
        return 0;
    }
    if (!tile_fits(d, ty, tx)) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "the largest tile's working set exceeds the 160 KiB of LDS at this plan", who);
        return 0;
    }
    *NY = ty;
    *NX = tx;
    return ty * tx;
}

extern "C" int32_t dcll_conv_lif_sequence_tiles_plan(const dcll_conv_desc *d, int32_t B, int32_t tiles_y, int32_t tiles_x,
                                                     int32_t *ny_nx, int32_t *bounds_y, int32_t *bounds_x)
{
    int rc, NY = 0, NX = 0, bands = 0;
    const int n = tile_count(d, B, tiles_y, tiles_x, "dcll_conv_lif_sequence_tiles_plan", &rc, &NY, &NX, &bands);
    if (!n) return 0;
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (ny_nx) {
        ny_nx[0] = NY;
        ny_nx[1] = NX;
    }
    if (bounds_y)
        for (int k = 0; k <= NY; ++k) bounds_y[k] = (int32_t)((long)k * ph / NY);
    if (bounds_x)
        for (int k = 0; k <= NX; ++k) bounds_x[k] = (int32_t)((long)k * pw / NX);
    return n;
}
extern "C" int64_t dcll_conv_lif_sequence_tiles_lds(const dcll_conv_desc *d, int32_t tiles_y, int32_t tiles_x)
{
    int rc, NY = 0, NX = 0, bands = 0;
    if (!tile_count(d, 1, tiles_y, tiles_x, "dcll_conv_lif_sequence_tiles_lds", &rc, &NY, &NX, &bands)) return 0;
    return NX == 1 ? dcll_conv_lif_sequence_bands_lds(d, bands) : tile_floats_max(d, NY, NX) * 4;
}
extern "C" int64_t dcll_conv_lif_sequence_tiles_scratch(const dcll_conv_desc *d, int32_t B)
{
    int rc, NY = 0, NX = 0, bands = 0;
    if (!tile_count(d, B, 0, 0, "dcll_conv_lif_sequence_tiles_scratch", &rc, &NY, &NX, &bands) || B < 0) return 0;
    return any_chain_steps(d) * 64 * tile_mt(d) + 2L * B * d->c_in * d->h * d->w;
}

template <int MT, bool R, bool WLDS>
__global__ __launch_bounds__(TILE_THREADS) void k_lif_seq_tile(const tile_geom g, const uint32_t *__restrict__ spk_in,
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
    const int NT = g.NY * g.NX, k = blockIdx.x % NT, ka = k / g.NX, kb = k - ka * g.NX;
    const long b = blockIdx.x / NT;
    const band_rows ry = band_plan(ka, g.NY, g.h, g.kh, g.pad_h, g.pool_h, g.ch, g.ph);
    const band_rows rx = band_plan(kb, g.NX, g.w, g.kw, g.pad_w, g.pool_w, g.cw, g.pw);
    const tile_lay L = tile_layout(ry, rx, g.c_in, g.c_out, g.kh, g.kw, MT, R);
    float *img = lds, *e0s = lds + L.o_e0, *vpl = lds + L.o_v, *arps = lds + L.o_arp, *taus = lds + L.o_tau, *sb = lds + L.o_bias,
          *wl = lds + g.o_w;
    const int HW = g.h * g.w, NIN = g.c_in * HW, NV = g.c_out * g.CP;
    const int HP = L.HR * L.HC, NINt = g.c_in * HP, NVt = g.c_out * L.CPt, NTL = (L.CPt + 31) >> 5;
    const int q0 = (ry.I0 + g.pad_h - ry.C0) * L.CB + rx.I0 + g.pad_w - rx.C0;  // the first held input pixel in a channel of img
    const int pg0 = ry.I0 * g.w + rx.I0, cp0 = ry.C0 * g.cw + rx.C0;          // ... and the first conv pixel, in the sample's planes
    const any_div dHP = make_div(HP), dHC = make_div(L.HC), dCPt = make_div(L.CPt), dCC = make_div(L.CC);

    // held input element i (channel ci, tile pixel (yl, xl)) -> its position in img; pg: its pixel in the sample's plane
    auto img_at = [&](int i, int &ci, int &yl, int &xl, int &pg) -> int {
        ci = fdiv(i, dHP);
        const int p = i - ci * HP;
        yl = fdiv(p, dHC);
        xl = p - yl * L.HC;
        pg = pg0 + yl * g.w + xl;
        return ci * L.CHS + q0 + yl * L.CB + xl;
    };
    // conv element i (channel co, tile pixel) -> its pixel in the sample's conv plane
    auto conv_at = [&](int i, int &co) -> int {
        co = fdiv(i, dCPt);
        const int pl = i - co * L.CPt, yl = fdiv(pl, dCC), xl = pl - yl * L.CC;
        return cp0 + yl * g.cw + xl;
    };

    // ---- prologue: the tile's state (from the snapshot) and constants on chip
    for (int i = tid; i < g.c_in * L.CHS; i += TILE_THREADS) img[i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < NINt; i += TILE_THREADS) {
        int ci, yl, xl, pg;
        const int q = img_at(i, ci, yl, xl, pg);
        const long gi = b * NIN + ci * HW + pg;
        e0s[i] = eps0_snap[gi];
        img[q] = eps1_snap[gi];
    }
    if (R)
        for (int i = tid; i < NVt; i += TILE_THREADS) {
            int co;
            const int cp = conv_at(i, co);
            arps[i] = arp_g[b * NV + co * g.CP + cp];
        }
    any_consts_to_lds<MT, WLDS, TILE_THREADS>(taus, sb, wl, tau4, bias, wperm, g.c_in, g.c_out, g.nsteps, g.nwl, tid);
    __syncthreads();

    // the trace update of held input element i at step t (eps0 in e0s, eps1 in place in img)
    auto trace = [&](const uint32_t *sp, int i) {
        int ci, yl, xl, pg;
        const int q = img_at(i, ci, yl, xl, pg);
        const float xin = (float)((sp[ci * g.iw + (pg >> 5)] >> (pg & 31)) & 1u);
        float e0 = e0s[i], e1 = img[q];
        trace_update(xin, taus[ci], taus[g.c_in + ci], taus[2 * g.c_in + ci], taus[3 * g.c_in + ci], e0, e1);
        e0s[i] = e0;
        img[q] = e1;
    };

    // NM chains (M tiles mt0 .. mt0 + NM - 1) of pixel tile tl of the tile
    auto chain = [&](auto nm_, int tl, int mt0) {
        const int pix = tl * 32 + j, pc = pix < L.CPt ? pix : L.CPt - 1, y = fdiv(pc, dCC), x = pc - y * L.CC;
        return any_chain<decltype(nm_)::value, MT, WLDS>(img, L.CB, L.CHS, y * L.CB + x, sb, wl, wperm, g.nwl, g.npair, g.nsteps,
                                                         g.c_in, g.kh, g.kw, lane, hh, mt0);
    };

    // pooling pass of step t over vpl: a half wave = the 32 pixels of one spike word of one channel.  The tile's pooled pixels are
    // the row segments [py pw + P0x, py pw + P1x): a unit is (channel, pooled row, k-th word the row's segment touches).  A word
    // wholly inside the segment is stored, every other word ORed into.
    const int NPR = ry.P1 - ry.P0, NPC = rx.P1 - rx.P0, nwr = (NPC + 30) / 32 + 1;
    auto pool_pass = [&](int t) {
        if (!spk_out && !pv_out) return;
        const int per = NPR * nwr, units = g.c_out * per, pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2;
        const long ob = ((long)t * B + b) * g.c_out;
        for (int u0 = 2 * wv; u0 < units; u0 += 2 * TILE_NW) {
            const int u = u0 + hh;
            const int uc = u < units ? u : 0, co = uc / per, ur = uc - co * per, pr = ur / nwr, py = ry.P0 + pr;
            const int s0 = py * g.pw + rx.P0, s1 = py * g.pw + rx.P1, wi = (s0 >> 5) + ur - pr * nwr, pp = wi * 32 + j;
            const bool uv = u < units && wi * 32 < s1;
            const bool pvld = uv && pp >= s0 && pp < s1;
            const int px = pvld ? pp - py * g.pw : rx.P0;
            const float *vc = vpl + co * L.CPt;
            float m = -INFINITY;
            for (int dy = 0; dy < g.pool_h; ++dy) {
                const int yy = py * g.pool_h - pph + dy;
                if (yy < ry.C0 || yy >= ry.C1) continue;        // (inside the tile: outside [0, ch) only)
                for (int dx = 0; dx < g.pool_w; ++dx) {
                    const int xx = px * g.pool_w - ppw + dx;
                    if (xx < rx.C0 || xx >= rx.C1) continue;    // (outside [0, cw) only)
                    m = fmaxf(m, vc[(yy - ry.C0) * L.CC + xx - rx.C0]);
                }
            }
            const unsigned long long mk = __ballot(pvld && m > 0.0f);
            if (pvld && pv_out) pv_out[(ob + co) * g.PP + pp] = sigmoidf_dev(m);
            if (spk_out && uv && j == 0) {
                const uint32_t bits = (uint32_t)(hh ? mk >> 32 : mk);
                const int wend = wi * 32 + 32 < g.PP ? wi * 32 + 32 : g.PP;
                uint32_t *dst = spk_out + (ob + co) * g.ow + wi;
                if (wi * 32 >= s0 && wend <= s1) *dst = bits;
                else if (bits) atomicOr(dst, bits);
            }
        }
    };

    for (int t = 0; t < T; ++t) {
        const uint32_t *sp = spk_in + ((long)t * B + b) * g.c_in * g.iw;
        const long ob = ((long)t * B + b) * g.c_out;
        // ---- phase A: pooled outputs of the previous step; traces of this step, in place
        if (t > 0) pool_pass(t - 1);
        for (int i = tid; i < NINt; i += TILE_THREADS) trace(sp, i);
        __syncthreads();
        // ---- phase B: the chains -> vpl
        if (MT == 1 || NTL >= TILE_NW) {
            for (int tl = wv; tl < NTL; tl += TILE_NW) {
                const any_acc<MT> acc = chain(std::integral_constant<int, MT>{}, tl, 0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) any_to_vpl(acc.t[mt], vpl, L.CPt, g.c_out, tl * 32 + j, mt, hh);
            }
        } else {
            for (int u = wv; u < NTL * MT; u += TILE_NW) {       // few pixel tiles: one (pixel tile, M tile) per wave
                const int tl = u / MT, mt = u - tl * MT;
                const any_acc<1> acc = chain(std::integral_constant<int, 1>{}, tl, mt);
                any_to_vpl(acc.t[0], vpl, L.CPt, g.c_out, tl * 32 + j, mt, hh);
            }
        }
        __syncthreads();
        // ---- phase C: refractory update on the v plane, v_out
        any_phase_c<R, TILE_THREADS>(vpl, arps, NVt, v_out, ob, g.CP, tid, alpharp, wrp, conv_at);
    }
    // ---- last step's pooled outputs; the owned state back to HBM
    pool_pass(T - 1);
    for (int i = tid; i < NINt; i += TILE_THREADS) {
        int ci, yl, xl, pg;
        const int q = img_at(i, ci, yl, xl, pg), y = ry.I0 + yl, x = rx.I0 + xl;
        if (y >= ry.O0 && y < ry.O1 && x >= rx.O0 && x < rx.O1) {
            const long gi = b * NIN + ci * HW + pg;
            eps0_g[gi] = e0s[i];
            eps1_g[gi] = img[q];
        }
    }
    if (R)
        for (int i = tid; i < NVt; i += TILE_THREADS) {
            int co;
            const int cp = conv_at(i, co);
            arp_g[b * NV + co * g.CP + cp] = arps[i];
        }
}

// the LDS reservation, then the weight permutation, the snapshot, the zero fill, then the kernel: an error return never follows
// a launch of the layer kernel
template <int MT, bool R, bool WLDS>
static int launch_tile(const dcll_conv_desc *d, const tile_geom &g, size_t lds_bytes, bool shared_words, const uint32_t *spk_in,
                       const float *W, float *scratch, const float *b, const float *tau4, float *eps0, float *eps1, float *arp,
                       uint32_t *spk_out, float *pv_out, float *v_out, int T, int B, float alpharp, float wrp, hipStream_t st, const char *name)
{
    if (hipFuncSetAttribute((const void *)k_lif_seq_tile<MT, R, WLDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_seq_tile: cannot reserve its LDS");
    }
    float *snap0, *snap1;
    const int rc = seq_split_prepare(d, W, scratch, MT, eps0, eps1, spk_out, (size_t)T * B * g.c_out * g.ow, shared_words, B, st,
                                     "k_lif_seq_tile", &snap0, &snap1);
    if (rc) return rc;
    hipLaunchKernelGGL((k_lif_seq_tile<MT, R, WLDS>), dim3((unsigned)((long)B * g.NY * g.NX)), dim3(TILE_THREADS), lds_bytes, st, g,
                       spk_in, scratch, b, tau4, snap0, snap1, eps0, eps1, arp, spk_out, pv_out, v_out, T, B, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

extern "C" int dcll_conv_lif_sequence_tiles(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                            const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out,
                                            float *pv_out, float *v_out, float *scratch, int32_t T, int32_t B, int32_t tiles_y,
                                            int32_t tiles_x, void *stream)
{
    const char *who = "dcll_conv_lif_sequence_tiles";
    if (T < 0 || B < 0) return fail(DCLL_ERR_INVALID, "negative T or B", who);
    if (T == 0 || B == 0) return DCLL_OK;
    int rc, NY = 0, NX = 0, bands = 0;
    const int NT = tile_count(d, B, tiles_y, tiles_x, who, &rc, &NY, &NX, &bands);
    // one column of tiles: the band path, its kernels, its launch-log names, its bits (its scratch is this one's)
    if (tiles_x == 1 || (NT && NX == 1))
        return dcll_conv_lif_sequence_bands(d, spk_in, W, b, tau4, eps0, eps1, arp, spk_out, pv_out, v_out, scratch, T, B,
                                            tiles_x == 1 ? tiles_y : bands, stream);
    if (!NT) return rc;
    if (!spk_in || !W || !tau4 || !eps0 || !eps1 || !scratch) return fail(DCLL_ERR_INVALID, "null pointer", who);
    if (d->refractory && !arp) return fail(DCLL_ERR_INVALID, "refractory layer needs arp", who);
    if ((long)B * NT > 0x7fffffffL) return fail(DCLL_ERR_INVALID, "B x tiles beyond the grid", who);
    hipStream_t st = (hipStream_t)stream;
    const int MT = tile_mt(d);
    tile_geom g;
    g.c_in = d->c_in; g.c_out = d->c_out; g.h = d->h; g.w = d->w; g.kh = d->kh; g.kw = d->kw;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.pool_h = d->pool_h; g.pool_w = d->pool_w;
    conv_shape(d, &g.ch, &g.cw, &g.ph, &g.pw);
    g.CP = g.ch * g.cw;
    g.PP = g.ph * g.pw;
    g.npair = (int)any_chain_pairs(d);
    g.nsteps = (int)any_chain_steps(d);
    g.iw = (d->h * d->w + 31) / 32;
    g.ow = (g.PP + 31) / 32;
    g.NY = NY;
    g.NX = NX;
    // the layout of every tile against the ONE exported formula; a segment that starts inside a spike word?
    long base = 0;
    bool shared_words = false;
    for (int ka = 0; ka < NY; ++ka) {
        const band_rows ry = band_plan(ka, NY, d->h, d->kh, d->pad_h, d->pool_h, g.ch, g.ph);
        for (int kb = 0; kb < NX; ++kb) {
            const band_rows rx = band_plan(kb, NX, d->w, d->kw, d->pad_w, d->pool_w, g.cw, g.pw);
            const tile_lay L = tile_layout(ry, rx, d->c_in, d->c_out, d->kh, d->kw, MT, d->refractory != 0);
            if (L.end != tile_floats(d, L.CR, L.CC, L.HR, L.HC))
                return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_sequence_tiles_lds disagree", who);
            if (L.end > base) base = L.end;
            for (int py = ry.P0; py < ry.P1 && !shared_words; ++py) shared_words = ((long)py * g.pw + rx.P0) % 32 != 0;
        }
    }
    if (base * 4 > ANY_LDS_MAX || base * 4 != dcll_conv_lif_sequence_tiles_lds(d, NY, NX))
        return fail(DCLL_ERR_LAUNCH, "a tile's LDS beyond the limit", who);
    g.o_w = (int)base;
    g.nwl = seq_weight_room(base, g.nsteps, MT, (long)B * NT);
    const bool wlds = g.nwl == g.nsteps;
    const size_t lds_bytes = (size_t)(base + (long)g.nwl * 64 * MT) * 4;

    // launch-log names: k_lif_seq_tile<M tiles, refractory, weights in LDS>
#define DCLL_TILE(M_, R_, L_)                                                                                                   \
    return launch_tile<M_, R_, L_>(d, g, lds_bytes, shared_words, spk_in, W, scratch, b, tau4, eps0, eps1, arp, spk_out, pv_out,  \
                                   v_out, T, B, d->alpharp, d->wrp, st, "k_lif_seq_tile<" #M_ "," #R_ "," #L_ ">")
    DCLL_SEQ_SPLIT_DISPATCH(DCLL_TILE, MT, d->refractory, wlds);
#undef DCLL_TILE
}
