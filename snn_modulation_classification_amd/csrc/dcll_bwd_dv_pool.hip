// dcll_bwd_dv_pool.hip — k_bwd_dv_pool<PH, PW, NP>: the dv plane of a layer that pools, as a stream
// (dcll_conv_lif_backward_ex[_open] with DCLL_BWD_POOL_DV; found by symbol lookup, the ABI version stays 10).
//
// k_bwd_dv (dcll_hip.hip) gives every un-pooled element a thread, which recomputes the sigmoid of the rest of its pool window,
// scans the window for the first-maximum rule and, if it wins, reads its `target` readout weights once per SAMPLE.  Here a thread
// owns one pooled window k = (co, py, px) of a sample's K = c_out ph pw windows, consecutive threads consecutive k (the i2o_W rows
// and g_pv are read coalesced, the window rows of v are contiguous across a wave), with its NP readout weights in registers (NP =
// target rounded up to 8, at most 32; k_bwd_dv_w3's and bwd_dv_nopool_body's trick) over a chunk of DP_PB samples, whose g_p rows
// go through LDS and come back as broadcasts; the loads of G samples are issued before the first is used (G = 4 up to four
// elements per window, 2 above).  Workgroup = 256 windows x one batch chunk; grid (ceil(K / 256), ceil(B / pb)), pb = DP_PB samples, or
// G where DP_PB would leave fewer than DP_MIN_WG workgroups.
//
// GEOMETRY (MaxPool2d(kernel = stride = pool, padding = (pool - 1) / 2), conv_shape()): window (py, px) covers the rows
// py PH - (PH - 1) / 2 .. + PH - 1 and the columns px PW - (PW - 1) / 2 .. + PW - 1, clipped at the plane's edges (pool 3: the
// first window starts at -1, the last may end behind the plane).  The windows are disjoint and leave out only trailing rows
// >= ph PH - (PH - 1) / 2 and trailing columns >= pw PW - (PW - 1) / 2 (an odd plane under pool 2; the last row / column of a
// plane divisible by 3 under pool 3) — at most one row and one column.  Those belong to the threads of the last window row /
// column: a thread with py == ph - 1 writes the row behind its window too, one with px == pw - 1 the column behind it (their
// loads are issued with the window's) — every element of the B c_out ch cw plane is written exactly once, nothing behind it.
//
// ARITHMETIC = k_bwd_dv's, bit for bit (-ffp-contract=off; tests/pool_dv_cases.py restates it): pv = sigmoidf_dev(v) of every
// in-range element of the window, ONCE; the winner is the first maximum in row-major order (strict > on the sigmoids: a tie
// goes to the earlier element); the winner's g = (g_pv or 0) + acc, acc = 0, acc = fmaf(g_p[b][n], i2o_W[n][k], acc), n = 0 ..
// target - 1 in that order (no sum without g_p); every other element's g — the elements in no window included — is 0.0f;
// out = g * pv * (1 - pv), + g_v where given.  The padding terms n >= target are fmaf(-0, +0, acc): the product is -0, and
// x + (-0) == x for EVERY x, -0 included (a +0 product would turn an acc of -0 — reachable by underflow — into +0).
// v may be any finite value or +-inf.  A NaN membrane is OUTSIDE the contract: k_bwd_dv lets an element whose sigmoid is NaN
// win beside the window's real maximum, this kernel picks one winner per window.
// All loads are scalar: the ABI asks for 4-byte alignment only, and a window row is 4 .. 12 bytes.
#include "dcll_internal.h"

#ifndef DP_PER_BLOCK            // samples per workgroup; restated by tests/pool_dv_cases.py
#define DP_PER_BLOCK 8
#endif
constexpr int DP_THREADS = 256, DP_PB = DP_PER_BLOCK;
constexpr int DP_MIN_WG = 512;  // fewer workgroups than this at DP_PB samples each: a workgroup takes one group of samples in flight instead
__host__ __device__ constexpr int dp_group(int ph, int pw) { return ph * pw <= 4 ? 4 : 2; }       // samples in flight

template <int PH, int PW, int NP>
__global__ __launch_bounds__(DP_THREADS) void k_bwd_dv_pool(const int K, const int N, const int c_out, const int ch, const int cw,
                                                            const int ph, const int pw, const float *__restrict__ v,
                                                            const float *__restrict__ g_p, const float *__restrict__ g_pv,
                                                            const float *__restrict__ g_v, const float *__restrict__ i2o_W,
                                                            float *__restrict__ gvf, const int B, const int pb)
{
    constexpr int E = PH * PW, G = dp_group(PH, PW), X = PH + PW + 1;
    static_assert(DP_PB % G == 0, "a chunk is whole groups of samples in flight");
    __shared__ __attribute__((aligned(16))) float gp[DP_PB][32];
    const int b0 = (int)blockIdx.y * pb, b1 = min(B, b0 + pb);          // (pb = DP_PB or G: dcll_launch_bwd_dv_pool)
    for (int e = threadIdx.x; e < DP_PB * 32; e += DP_THREADS) {
        const int bb = b0 + (e >> 5), n = e & 31;
        gp[e >> 5][n] = (g_p && n < N && bb < b1) ? g_p[(long)bb * N + n] : -0.0f;
    }
    __syncthreads();
    const unsigned ku = blockIdx.x * (unsigned)DP_THREADS + threadIdx.x;
    if (ku >= (unsigned)K) return;
    const int k = (int)ku;
    const int px = k % pw, r = k / pw, py = r % ph, co = r / ph;
    const int y0 = py * PH - (PH - 1) / 2, x0 = px * PW - (PW - 1) / 2;
    const int plane = ch * cw;
    const long P = (long)c_out * plane;                 // elements of a sample
    const int base = co * plane + y0 * cw + x0;         // (element (dy, dx) of the window: base + dy cw + dx, where in range)
    bool inr[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int yy = y0 + e / PW, xx = x0 + e % PW;
        inr[e] = (unsigned)yy < (unsigned)ch && (unsigned)xx < (unsigned)cw;
    }
    // the elements in no window that this thread writes: at most ONE trailing row and ONE trailing column exist (the plane ends
    // less than a window behind the last one, and (cw + 2 pad - PW) % PW - pad <= 1 for PW <= 3) — the row behind the window of a
    // last-row thread over its columns (x = 0 .. PW - 1), the column behind the window of a last-column thread over its rows
    // (x = PW .. PW + PH - 1), and the corner behind both (x = PW + PH): X elements with fixed offsets, loaded with the window's
    const bool tr = py == ph - 1 && y0 + PH < ch, tc = px == pw - 1 && x0 + PW < cw;
    bool xin[X];
#pragma unroll
    for (int x = 0; x < X; ++x) {
        const int yy = x < PW ? y0 + PH : x < PW + PH ? y0 + (x - PW) : y0 + PH;
        const int xx = x < PW ? x0 + x : x0 + PW;
        xin[x] = (x < PW ? tr : x < PW + PH ? tc : (tr && tc)) && (unsigned)yy < (unsigned)ch && (unsigned)xx < (unsigned)cw;
    }
    const bool edge = tr || tc;
#define DP_XOFF(x) ((x) < PW ? PH * cw + (x) : (x) < PW + PH ? ((x) - PW) * cw + PW : PH * cw + PW)
    float wk[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) wk[n] = (g_p && n < N) ? i2o_W[(long)n * K + k] : 0.0f;
    for (int bg = b0; bg < b1; bg += G) {
        float vv[G][E], ga[G][E], gg[G], vx[G][X], gx[G][X];
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int b = min(bg + q, b1 - 1);
            const float *vp = v + (long)b * P + base;
            const float *ap = g_v + (long)b * P + base;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                vv[q][e] = inr[e] ? vp[(e / PW) * cw + e % PW] : 0.0f;
                ga[q][e] = (g_v && inr[e]) ? ap[(e / PW) * cw + e % PW] : 0.0f;
            }
            gg[q] = g_pv ? g_pv[(long)b * K + k] : 0.0f;
            if (edge) {
#pragma unroll
                for (int x = 0; x < X; ++x) {
                    vx[q][x] = xin[x] ? vp[DP_XOFF(x)] : 0.0f;
                    gx[q][x] = (g_v && xin[x]) ? ap[DP_XOFF(x)] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int b = min(bg + q, b1 - 1);
            float g = gg[q];
            if (g_p) {
                float acc = 0.0f;
#pragma unroll
                for (int n4 = 0; n4 < NP; n4 += 4) {
                    const f32x4 gq = *(const f32x4 *)&gp[b - b0][n4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = __builtin_fmaf(gq[u], wk[n4 + u], acc);
                }
                g += acc;
            }
            float pv[E];
            int win = -1;
            float best = 0.0f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                pv[e] = sigmoidf_dev(vv[q][e]);
                if (inr[e] && (win < 0 || pv[e] > best)) win = e, best = pv[e];
            }
            if (bg + q < b1) {
                float *op = gvf + (long)b * P + base;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float ge = e == win ? g : 0.0f;
                    float o = ge * pv[e] * (1.0f - pv[e]);
                    if (g_v) o += ga[q][e];
                    if (inr[e]) op[(e / PW) * cw + e % PW] = o;
                }
                if (edge) {
#pragma unroll
                    for (int x = 0; x < X; ++x) {
                        const float pe = sigmoidf_dev(vx[q][x]);
                        float o = 0.0f * pe * (1.0f - pe);
                        if (g_v) o += gx[q][x];
                        if (xin[x]) op[DP_XOFF(x)] = o;
                    }
                }
            }
        }
    }
}

#undef DP_XOFF

// the served set (dcll_bwd_dv_pool_served restates nothing: it is this function)
static bool dp_served(const dcll_conv_desc *d, int32_t B)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (d->pool_h < 1 || d->pool_h > 3 || d->pool_w < 1 || d->pool_w > 3 || (d->pool_h == 1 && d->pool_w == 1)) return false;
    if (ch < d->pool_h || cw < d->pool_w || d->target > 32) return false;
    // index types: k and an element's offset inside its sample are ints (the offsets of a clipped window reach one row and one
    // column before / behind the sample's plane), a workgroup's first k an unsigned; sample offsets are longs
    const long K = (long)d->c_out * ph * pw, P = (long)d->c_out * ch * cw;
    if (K > 0x7fffffffL - DP_THREADS || P > 0x7fffffffL - 4L * (cw + 1)) return false;
    if (B < 1 || ((long)B + DP_PB - 1) / DP_PB > 65535) return false;
    return true;
}

extern "C" int32_t dcll_bwd_dv_pool_served(const dcll_conv_desc *d, int32_t B)
{
    const int rc = check_desc(d);
    if (rc) return rc;
    return dp_served(d, B) ? 1 : 0;
}

// the dv launch of a backward call (check_desc passed).  *form = the kernel's name for the launch log, nullptr = not served:
// nothing launched, the caller keeps k_bwd_dv
int dcll_launch_bwd_dv_pool(const dcll_conv_desc *d, const float *v, const float *g_p, const float *g_pv, const float *g_v,
                            const float *i2o_W, float *gvf, int32_t B, hipStream_t st, const char **form)
{
    *form = nullptr;
    if (!dp_served(d, B)) return DCLL_OK;
    if (!v || !gvf || (g_p && !i2o_W)) return fail(DCLL_ERR_LAUNCH, "k_bwd_dv_pool: null pointer", "dcll_conv_lif_backward_ex");
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const int K = d->c_out * ph * pw;
    // samples per workgroup: DP_PB (the readout weights are loaded once per 8 samples), or one group of samples in flight where
    // that leaves fewer than DP_MIN_WG workgroups (small batches, small maps: the launch is latency-bound, not bandwidth-bound)
    const unsigned gx = (unsigned)((K + DP_THREADS - 1) / DP_THREADS);
    const int pb = (long)gx * ((B + DP_PB - 1) / DP_PB) < DP_MIN_WG ? dp_group(d->pool_h, d->pool_w) : DP_PB;
    const dim3 grid(gx, (unsigned)((B + pb - 1) / pb));
#define DCLL_DVP(PH_, PW_, NP_)                                                                                         \
    hipLaunchKernelGGL((k_bwd_dv_pool<PH_, PW_, NP_>), grid, dim3(DP_THREADS), 0, st, K, d->target, d->c_out, ch, cw, ph, pw, v, \
                       g_p, g_pv, g_v, i2o_W, gvf, B, pb)
#define DCLL_DVP_N(PH_, PW_)                                                                                            \
    do {                                                                                                                \
        if (d->target <= 8) DCLL_DVP(PH_, PW_, 8);                                                                      \
        else if (d->target <= 16) DCLL_DVP(PH_, PW_, 16);                                                               \
        else if (d->target <= 24) DCLL_DVP(PH_, PW_, 24);                                                               \
        else DCLL_DVP(PH_, PW_, 32);                                                                                    \
    } while (0)
    switch (d->pool_h * 4 + d->pool_w) {
    case 1 * 4 + 2: DCLL_DVP_N(1, 2); break;
    case 1 * 4 + 3: DCLL_DVP_N(1, 3); break;
    case 2 * 4 + 1: DCLL_DVP_N(2, 1); break;
    case 2 * 4 + 2: DCLL_DVP_N(2, 2); break;
    case 2 * 4 + 3: DCLL_DVP_N(2, 3); break;
    case 3 * 4 + 1: DCLL_DVP_N(3, 1); break;
    case 3 * 4 + 2: DCLL_DVP_N(3, 2); break;
    default: DCLL_DVP_N(3, 3); break;
    }
#undef DCLL_DVP_N
#undef DCLL_DVP
    *form = "k_bwd_dv_pool";
    return DCLL_OK;
}
