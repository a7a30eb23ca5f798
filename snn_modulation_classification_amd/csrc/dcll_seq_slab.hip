// dcll_seq_slab.hip — k_lif_seq_slab: all T timesteps of a plain conv layer with MORE than 64 output channels (stride = dilation =
// groups = 1, kernel up to 16x16, any padding, any pooling) in one launch (dcll_conv_lif_sequence_slabs).  Opt-in, beside
// k_lif_seq_tile, which stops at 64 channels.  A membrane v[co] is one pinned chain over the input traces with W[co]: output channels
// are independent, so the kernel is k_lif_seq_tile with one more grid dimension, B x NY x NX x NS.  blockIdx.y is the slab (the slab
// rule: dcll_any_shared.h): slab s owns the output channels [64 s, min(64 s + 64, c_out)), two 32-row M tiles.  A layer of at most
// 64 output channels is handed to dcll_conv_lif_sequence_tiles unchanged.
//
// A workgroup = (sample, tile (a, b) of the NY x NX plan, slab).  It holds the traces of ALL c_in input channels of its tile,
// exactly as a tile workgroup does, and vpl, arp, the bias and the weights kept in LDS for ITS SLAB only: per-workgroup LDS does
// not grow with c_out.  Every slab of a tile recomputes the tile's traces (nothing passes between workgroups); slab 0 alone writes
// eps0 / eps1 back.  Every slab writes its own arp, pv, v and spike planes: a spike word belongs to one channel, so slabs never
// share one; inside a channel the tile kernel's rule stands (a word wholly inside a row segment is stored, every other word ORed
// into the zero-filled buffer).  Initial state comes from the stream-ordered snapshot of eps0 / eps1 in the scratch.
// wperm is the ONE permutation kernel's output at MT = ceil(c_out / 32); a slab reads its two columns of it (any_chain's SLAB form
// for the streamed steps, any_consts_to_lds_slab for the steps kept in LDS).  A last slab of at most 32 channels has an empty second
// M tile: it runs one chain per pixel tile, not two.
// Every v is ONE unsplit chain in the pinned order: the results are bit-identical to dcll_conv_lif_sequence_tiles run on each
// 64-channel slice of the layer (W, bias, arp) with the same plan.
//
// Tile plan: the product of two 1-D band plans (band_plan(), dcll_any_shared.h), as in k_lif_seq_tile.  LDS of a tile (floats;
// ss_floats() is the ONE statement of it, exported as dcll_conv_lif_sequence_slabs_lds for the largest tile) is k_lif_seq_tile's
// formula with the slab's channel count, 64, in place of c_out:
//   img c_in x (CR + kh - 1) x (CC + kw - 1) | e0 c_in x HR x HC | vpl 64 x CR x CC | arp 64 x CR x CC (refractory) | tau 4 c_in | bias 64
//   + behind the largest tile's set as many permuted weight steps (128 floats each) as fit (WLDS: all); the rest streamed from L2.
// This kernel runs EVERY plan itself, 1 x 1 and N x 1 included (the band and wide kernels refuse c_out > 64).  The (0, 0) rule:
// the fitting (NY, NX) with the fewest tiles, from one tile up; ties go to the smallest sum of held input elements, then to the
// smaller NX — k_lif_seq_tile's rule without its "NX >= 2".  DERIVED FROM THE LDS FORMULA ALONE, no measurement stands behind it.
#include <vector>

#include "dcll_any_shared.h"

constexpr int SS_THREADS = 512, SS_NW = SS_THREADS / 64;
constexpr int SS_MT = 2;                        // M tiles of a slab

struct ss_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane of the whole sample
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int nwl;                    // chain steps whose weights are kept in LDS (WLDS: all of them)
    int iw, ow;                 // words per input / output spike plane
    int o_w;                    // float offset of the weights in LDS: the largest tile's set
    int NY, NX, gmt;            // the plan; M tiles of the whole layer (the stride of wperm in memory)
};

// float offsets into a tile's LDS (img at 0)
struct ss_lay {
    int RB, CB, CHS, HR, HC, CR, CC, CPt, o_e0, o_v, o_arp, o_tau, o_bias, end;
};
__host__ __device__ static inline ss_lay ss_layout(const band_rows &ry, const band_rows &rx, int c_in, int kh, int kw, bool refr)
{
    ss_lay L;
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
    L.o_arp = L.o_v + SLAB_ROWS * L.CPt;
    L.o_tau = L.o_arp + (refr ? SLAB_ROWS * L.CPt : 0);
    L.o_bias = L.o_tau + 4 * c_in;
    L.end = L.o_bias + 32 * SS_MT;
    return L;
}

// the working set in floats, without the weights, of a tile of CR x CC conv pixels that holds HR x HC input pixels
static inline long ss_floats(const dcll_conv_desc *d, long CR, long CC, long HR, long HC)
{
    const long img = d->c_in * (CR + d->kh - 1) * (CC + d->kw - 1);
    const long e0 = d->c_in * HR * HC;
    const long vpl = SLAB_ROWS * CR * CC;
    return img + e0 + vpl * (d->refractory ? 2 : 1) + 4L * d->c_in + 32 * SS_MT;
}

// one direction of a plan: the distinct (conv pixels, held pixels) of its parts and the sum of the held pixels
struct ss_axis {
    std::vector<std::pair<int, int>> kinds;
    long held;
};
static ss_axis ss_axis_of(int N, int h, int kh, int pad, int pool, int ch, int ph)
{
    ss_axis a;
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
static long ss_floats_max(const dcll_conv_desc *d, int NY, int NX, long *held = nullptr)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const ss_axis ay = ss_axis_of(NY, d->h, d->kh, d->pad_h, d->pool_h, ch, ph);
    const ss_axis ax = ss_axis_of(NX, d->w, d->kw, d->pad_w, d->pool_w, cw, pw);
    long m = 0;
    for (const auto &y : ay.kinds)
        for (const auto &x : ax.kinds) {
            const long f = ss_floats(d, y.first, x.first, y.second, x.second);
            if (f > m) m = f;
        }
    if (held) *held = ay.held * ax.held;
    return m;
}

// the (0, 0) rule (file header).  false: no plan fits
static bool ss_rule(const dcll_conv_desc *d, int *NY, int *NX)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    for (long n = 1; n <= (long)ph * pw; ++n) {
        long best = -1;
        for (int nx = 1; nx <= pw && nx <= n; ++nx) {
            if (n % nx || n / nx > ph) continue;
            long held;
            if (ss_floats_max(d, (int)(n / nx), nx, &held) * 4 > ANY_LDS_MAX) continue;
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

static inline int ss_gmt(const dcll_conv_desc *d) { return (d->c_out + 31) / 32; }

// the plan a call runs on a layer of c_out > 64 -> tiles per (sample, slab) (0: refused, rc and the message set)
static int ss_count(const dcll_conv_desc *d, int ty, int tx, const char *who, int *rc, int *NY, int *NX)
{
    *rc = check_desc(d);
    if (*rc) return 0;
    if (!plain_conv(d)) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
        return 0;
    }
    if (d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
        return 0;
    }
    if (slab_count(d->c_out) > SLAB_MAX || any_chain_steps(d) * 64 * ss_gmt(d) >= (1L << 31)) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "more than 65535 slabs of 64 output channels, or 2^31 permuted weights", who);
        return 0;
    }
    if (ty < 0 || tx < 0) {
        *rc = fail(DCLL_ERR_INVALID, "negative tile count", who);
        return 0;
    }
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (ty == 0 && tx == 0) {
        if (!ss_rule(d, NY, NX)) {
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
    if (ss_floats_max(d, ty, tx) * 4 > ANY_LDS_MAX) {
        *rc = fail(DCLL_ERR_UNSUPPORTED, "the largest tile's working set exceeds the 160 KiB of LDS at this plan", who);
        return 0;
    }
    *NY = ty;
    *NX = tx;
    return ty * tx;
}

extern "C" int32_t dcll_conv_lif_sequence_slabs_plan(const dcll_conv_desc *d, int32_t B, int32_t tiles_y, int32_t tiles_x,
                                                     int32_t *ny_nx, int32_t *bounds_y, int32_t *bounds_x)
{
    if (d && d->c_out <= SLAB_ROWS) return dcll_conv_lif_sequence_tiles_plan(d, B, tiles_y, tiles_x, ny_nx, bounds_y, bounds_x);
    int rc, NY = 0, NX = 0;
    const int n = ss_count(d, tiles_y, tiles_x, "dcll_conv_lif_sequence_slabs_plan", &rc, &NY, &NX);
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
extern "C" int64_t dcll_conv_lif_sequence_slabs_lds(const dcll_conv_desc *d, int32_t tiles_y, int32_t tiles_x)
{
    if (d && d->c_out <= SLAB_ROWS) return dcll_conv_lif_sequence_tiles_lds(d, tiles_y, tiles_x);
    int rc, NY = 0, NX = 0;
    if (!ss_count(d, tiles_y, tiles_x, "dcll_conv_lif_sequence_slabs_lds", &rc, &NY, &NX)) return 0;
    return ss_floats_max(d, NY, NX) * 4;
}
extern "C" int64_t dcll_conv_lif_sequence_slabs_scratch(const dcll_conv_desc *d, int32_t B)
{
    if (d && d->c_out <= SLAB_ROWS) return dcll_conv_lif_sequence_tiles_scratch(d, B);
    int rc, NY = 0, NX = 0;
    if (!ss_count(d, 0, 0, "dcll_conv_lif_sequence_slabs_scratch", &rc, &NY, &NX) || B < 0) return 0;
    return any_chain_steps(d) * 64 * ss_gmt(d) + 2L * B * d->c_in * d->h * d->w;
}

template <bool R, bool WLDS>
__global__ __launch_bounds__(SS_THREADS) void k_lif_seq_slab(const ss_geom g, const uint32_t *__restrict__ spk_in,
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
    // the slab: channels [co0, co0 + nrow), nmt real M tiles; its first column of the layer's permutation
    const int slab = blockIdx.y, co0 = slab_first(slab), nrow = slab_rows(slab, g.c_out), nmt = (nrow + 31) >> 5;
    const float *wps = wperm + (long)slab * SS_MT * 64;
    const band_rows ry = band_plan(ka, g.NY, g.h, g.kh, g.pad_h, g.pool_h, g.ch, g.ph);
    const band_rows rx = band_plan(kb, g.NX, g.w, g.kw, g.pad_w, g.pool_w, g.cw, g.pw);
    const ss_lay L = ss_layout(ry, rx, g.c_in, g.kh, g.kw, R);
    float *img = lds, *e0s = lds + L.o_e0, *vpl = lds + L.o_v, *arps = lds + L.o_arp, *taus = lds + L.o_tau, *sb = lds + L.o_bias,
          *wl = lds + g.o_w;
    const int HW = g.h * g.w, NIN = g.c_in * HW;
    const long NV = (long)g.c_out * g.CP;
    const int HP = L.HR * L.HC, NINt = g.c_in * HP, NVt = nrow * L.CPt, NTL = (L.CPt + 31) >> 5;
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
    // conv element i of the slab's v plane (slab row, tile pixel) -> its GLOBAL channel and its pixel in the sample's conv plane
    auto conv_at = [&](int i, int &co) -> int {
        const int r = fdiv(i, dCPt), pl = i - r * L.CPt, yl = fdiv(pl, dCC), xl = pl - yl * L.CC;
        co = co0 + r;
        return cp0 + yl * g.cw + xl;
    };

    // ---- prologue: the tile's state (from the snapshot) and the slab's constants on chip
    for (int i = tid; i < g.c_in * L.CHS; i += SS_THREADS) img[i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < NINt; i += SS_THREADS) {
        int ci, yl, xl, pg;
        const int q = img_at(i, ci, yl, xl, pg);
        const long gi = b * NIN + ci * HW + pg;
        e0s[i] = eps0_snap[gi];
        img[q] = eps1_snap[gi];
    }
    if (R)
        for (int i = tid; i < NVt; i += SS_THREADS) {
            int co;
            const int cp = conv_at(i, co);
            arps[i] = arp_g[b * NV + (long)co * g.CP + cp];
        }
    any_consts_to_lds_slab<WLDS, SS_THREADS>(taus, sb, wl, tau4, bias, wps, g.c_in, co0, nrow, nmt, g.gmt, g.nsteps, g.nwl, tid);
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

    // NM chains (the slab's M tiles mt0 .. mt0 + NM - 1) of pixel tile tl of the tile
    auto chain = [&](auto nm_, int tl, int mt0) {
        const int pix = tl * 32 + j, pc = pix < L.CPt ? pix : L.CPt - 1, y = fdiv(pc, dCC), x = pc - y * L.CC;
        return any_chain<decltype(nm_)::value, SS_MT, WLDS, true>(img, L.CB, L.CHS, y * L.CB + x, sb, wl, wps, g.nwl, g.npair, g.nsteps,
                                                                  g.c_in, g.kh, g.kw, lane, hh, mt0, g.gmt);
    };

    // pooling pass of step t over vpl: k_lif_seq_tile's, over the slab's channels (a unit is (slab row, pooled row, k-th word the
    // row's segment touches); a word wholly inside the segment is stored, every other word ORed into)
    const int NPR = ry.P1 - ry.P0, NPC = rx.P1 - rx.P0, nwr = (NPC + 30) / 32 + 1;
    auto pool_pass = [&](int t) {
        if (!spk_out && !pv_out) return;
        const int per = NPR * nwr, units = nrow * per, pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2;
        const long ob = ((long)t * B + b) * g.c_out + co0;
        for (int u0 = 2 * wv; u0 < units; u0 += 2 * SS_NW) {
            const int u = u0 + hh;
            const int uc = u < units ? u : 0, r = uc / per, ur = uc - r * per, pr = ur / nwr, py = ry.P0 + pr;
            const int s0 = py * g.pw + rx.P0, s1 = py * g.pw + rx.P1, wi = (s0 >> 5) + ur - pr * nwr, pp = wi * 32 + j;
            const bool uv = u < units && wi * 32 < s1;
            const bool pvld = uv && pp >= s0 && pp < s1;
            const int px = pvld ? pp - py * g.pw : rx.P0;
            const float *vc = vpl + r * L.CPt;
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
            if (pvld && pv_out) pv_out[(ob + r) * g.PP + pp] = sigmoidf_dev(m);
            if (spk_out && uv && j == 0) {
                const uint32_t bits = (uint32_t)(hh ? mk >> 32 : mk);
                const int wend = wi * 32 + 32 < g.PP ? wi * 32 + 32 : g.PP;
                uint32_t *dst = spk_out + (ob + r) * g.ow + wi;
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
        for (int i = tid; i < NINt; i += SS_THREADS) trace(sp, i);
        __syncthreads();
        // ---- phase B: the chains -> vpl (nmt, NTL: uniform over the workgroup)
        if (nmt == 1) {
            for (int tl = wv; tl < NTL; tl += SS_NW) {          // a last slab of at most 32 channels: one chain per pixel tile
                const any_acc<1> acc = chain(std::integral_constant<int, 1>{}, tl, 0);
                any_to_vpl(acc.t[0], vpl, L.CPt, nrow, tl * 32 + j, 0, hh);
            }
        } else if (NTL >= SS_NW) {
            for (int tl = wv; tl < NTL; tl += SS_NW) {
                const any_acc<SS_MT> acc = chain(std::integral_constant<int, SS_MT>{}, tl, 0);
#pragma unroll
                for (int mt = 0; mt < SS_MT; ++mt) any_to_vpl(acc.t[mt], vpl, L.CPt, nrow, tl * 32 + j, mt, hh);
            }
        } else {
            for (int u = wv; u < NTL * SS_MT; u += SS_NW) {      // few pixel tiles: one (pixel tile, M tile) per wave
                const int tl = u / SS_MT, mt = u - tl * SS_MT;
                const any_acc<1> acc = chain(std::integral_constant<int, 1>{}, tl, mt);
                any_to_vpl(acc.t[0], vpl, L.CPt, nrow, tl * 32 + j, mt, hh);
            }
        }
        __syncthreads();
        // ---- phase C: refractory update on the slab's v plane, v_out
        any_phase_c<R, SS_THREADS>(vpl, arps, NVt, v_out, ob, g.CP, tid, alpharp, wrp, conv_at);
    }
    // ---- last step's pooled outputs; the owned state back to HBM: the traces by slab 0 alone, arp by every slab
    pool_pass(T - 1);
    if (slab == 0)
        for (int i = tid; i < NINt; i += SS_THREADS) {
            int ci, yl, xl, pg;
            const int q = img_at(i, ci, yl, xl, pg), y = ry.I0 + yl, x = rx.I0 + xl;
            if (y >= ry.O0 && y < ry.O1 && x >= rx.O0 && x < rx.O1) {
                const long gi = b * NIN + ci * HW + pg;
                eps0_g[gi] = e0s[i];
                eps1_g[gi] = img[q];
            }
        }
    if (R)
        for (int i = tid; i < NVt; i += SS_THREADS) {
            int co;
            const int cp = conv_at(i, co);
            arp_g[b * NV + (long)co * g.CP + cp] = arps[i];
        }
}

// the LDS reservation, then the weight permutation, the snapshot, the zero fill, then the kernel: an error return never follows
// a launch of the layer kernel
template <bool R, bool WLDS>
static int launch_slab(const dcll_conv_desc *d, const ss_geom &g, size_t lds_bytes, bool shared_words, int NS, const uint32_t *spk_in,
                       const float *W, float *scratch, const float *b, const float *tau4, float *eps0, float *eps1, float *arp,
                       uint32_t *spk_out, float *pv_out, float *v_out, int T, int B, float alpharp, float wrp, hipStream_t st, const char *name)
{
    if (hipFuncSetAttribute((const void *)k_lif_seq_slab<R, WLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) !=
        hipSuccess) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_seq_slab: cannot reserve its LDS");
    }
    float *snap0, *snap1;
    const int rc = seq_split_prepare(d, W, scratch, g.gmt, eps0, eps1, spk_out, (size_t)T * B * g.c_out * g.ow, shared_words, B, st,
                                     "k_lif_seq_slab", &snap0, &snap1);
    if (rc) return rc;
    hipLaunchKernelGGL((k_lif_seq_slab<R, WLDS>), dim3((unsigned)((long)B * g.NY * g.NX), (unsigned)NS), dim3(SS_THREADS), lds_bytes, st,
                       g, spk_in, scratch, b, tau4, snap0, snap1, eps0, eps1, arp, spk_out, pv_out, v_out, T, B, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

extern "C" int dcll_conv_lif_sequence_slabs(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                            const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out,
                                            float *pv_out, float *v_out, float *scratch, int32_t T, int32_t B, int32_t tiles_y,
                                            int32_t tiles_x, void *stream)
{
    const char *who = "dcll_conv_lif_sequence_slabs";
    // at most 64 output channels: the tile path, its kernels, its launch-log names, its bits, its refusals
    if (d && d->c_out <= SLAB_ROWS)
        return dcll_conv_lif_sequence_tiles(d, spk_in, W, b, tau4, eps0, eps1, arp, spk_out, pv_out, v_out, scratch, T, B, tiles_y,
                                            tiles_x, stream);
    if (T < 0 || B < 0) return fail(DCLL_ERR_INVALID, "negative T or B", who);
    if (T == 0 || B == 0) return DCLL_OK;
    int rc, NY = 0, NX = 0;
    const int NT = ss_count(d, tiles_y, tiles_x, who, &rc, &NY, &NX);
    if (!NT) return rc;
    if (!spk_in || !W || !tau4 || !eps0 || !eps1 || !scratch) return fail(DCLL_ERR_INVALID, "null pointer", who);
    if (d->refractory && !arp) return fail(DCLL_ERR_INVALID, "refractory layer needs arp", who);
    if ((long)B * NT > 0x7fffffffL) return fail(DCLL_ERR_INVALID, "B x tiles beyond the grid", who);
    hipStream_t st = (hipStream_t)stream;
    const int NS = slab_count(d->c_out);
    ss_geom g;
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
    g.gmt = ss_gmt(d);
    // the layout of every tile against the ONE exported formula; a segment that starts inside a spike word?
    long base = 0;
    bool shared_words = false;
    for (int ka = 0; ka < NY; ++ka) {
        const band_rows ry = band_plan(ka, NY, d->h, d->kh, d->pad_h, d->pool_h, g.ch, g.ph);
        for (int kb = 0; kb < NX; ++kb) {
            const band_rows rx = band_plan(kb, NX, d->w, d->kw, d->pad_w, d->pool_w, g.cw, g.pw);
            const ss_lay L = ss_layout(ry, rx, d->c_in, d->kh, d->kw, d->refractory != 0);
            if (L.end != ss_floats(d, L.CR, L.CC, L.HR, L.HC))
                return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_sequence_slabs_lds disagree", who);
            if (L.end > base) base = L.end;
            for (int py = ry.P0; py < ry.P1 && !shared_words; ++py) shared_words = ((long)py * g.pw + rx.P0) % 32 != 0;
        }
    }
    if (NS < 2 || NS > SLAB_MAX || base * 4 > ANY_LDS_MAX || base * 4 != dcll_conv_lif_sequence_slabs_lds(d, NY, NX))
        return fail(DCLL_ERR_LAUNCH, "a tile's LDS beyond the limit", who);
    g.o_w = (int)base;
    g.nwl = seq_weight_room(base, g.nsteps, SS_MT, (long)B * NT * NS);
    const bool wlds = g.nwl == g.nsteps;
    const size_t lds_bytes = (size_t)(base + (long)g.nwl * 64 * SS_MT) * 4;

    // launch-log names: k_lif_seq_slab<refractory, weights in LDS>
#define DCLL_SLAB(R_, L_)                                                                                                        \
    return launch_slab<R_, L_>(d, g, lds_bytes, shared_words, NS, spk_in, W, scratch, b, tau4, eps0, eps1, arp, spk_out, pv_out,   \
                               v_out, T, B, d->alpharp, d->wrp, st, "k_lif_seq_slab<" #R_ "," #L_ ">")
    if (d->refractory) {
        if (wlds) DCLL_SLAB(1, 1);
        DCLL_SLAB(1, 0);
    }
    if (wlds) DCLL_SLAB(0, 1);
    DCLL_SLAB(0, 0);
#undef DCLL_SLAB
}
