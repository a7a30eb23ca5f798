// dcll_bwd_slab.hip — k_bwd_wgrad_slab: the weight gradient of a plain conv layer with MORE than 64 output channels (stride =
// dilation = groups = 1, kernel up to 16x16, any c_in, padding, pooling, batch) on fp32 MFMA tiles
// (dcll_conv_lif_backward_slab[_open]) — the layers a --netscale above 2 makes.  A row of dW is a sum over the batch and the pixels
// of that channel's dv times the input traces: output channels are independent, so the kernel is k_bwd_wgrad_wide's decomposition
// (dcll_bwd_wide.hip) with one more grid dimension.  blockIdx.z is the slab (the slab rule: dcll_any_shared.h): slab s owns the
// output channels [64 s, min(64 s + 64, c_out)), two 32-row M tiles.  A layer of at most 64 output channels is handed to
// dcll_conv_lif_backward_wide unchanged (dcll_hip.hip), so a network of mixed widths goes through one entry point.  A translation
// unit of its own: k_bwd_wgrad_wide and its ISA are untouched; the geometry and the plan are restated here (ws_geom, ws_make_plan).
//
//   dW[co][n] = sum_{b,pix} g[b,co,pix] * E[b][n][pix],  n = ci kh kw + tap,   db[co] = sum g
//
// Per sample the workgroup (chunk, column split, slab) stages in LDS
//   img   cg x (h + 2 pad_h) x (w + 2 pad_w) + 1   eps1 of the input channels of ITS column tiles, zero padded
//   g     64 x GLD                                  ITS SLAB's rows of the sample's dv plane, rows of cwp = cw rounded up to even
//                                                   floats, the tail of an odd row ZERO; GLD odd
// (ws_make_plan() is the ONE statement of the layout, exported as dcll_conv_lif_backward_slab_lds): LDS does not grow with c_out.
// The M rows at or beyond the slab's last channel read the slab's last real row and are not stored (a last slab of at most 32
// channels runs its second M tile on that row: the launch's workgroups are alike, and such a slab is not the critical path).
// The partial rows carry the GLOBAL channel: part[chunk][co][c_in kh kw + 1] — the format k_bwd_reduce[4] /
// dcll_grad_reduce_adam consume, which take any c_out.  The bias gradient of a slab's rows comes from the workgroup with the first
// column tiles of that slab.
//
// Carried over from k_bwd_wgrad_wide unchanged: a wave runs both M tiles of its column tiles on one B-operand read; the odd-cw
// rule; the column split (TPW <= 32 consecutive column tiles per workgroup, lowered until img + g fit 160 KiB); the pixel split
// (TPW < 5: PS = 2 / 4 / 8, pieces through LDS, added in wave order); at most 256 batch chunks; "a tile beyond the range is computed
// on the first tile's columns and not stored"; every sum has a fixed order.  The small-batch rule counts the slabs: TPW is lowered
// until chunks x splits x slabs reach the CU count — never to a layout that needs more LDS than the full launch.  The launch plan
// is a pure function of (descriptor, B).
#include "dcll_any_shared.h"

constexpr int WS_THREADS = 512;
constexpr long WS_LDS_MAX_FLOATS = ANY_LDS_MAX / 4;
constexpr int WS_MT = 2;
constexpr int WS_MAX_TPW = 32;                   // column tiles per workgroup: 8 waves x 4 column tiles (x 2 M tiles each)
constexpr int WS_MAX_CHUNKS = 256;               // batch chunks (= partial rows)
constexpr int WS_TARGET_WG = ANY_CUS;            // workgroups a launch aims at (one per CU)
constexpr int WS_RED_FLOATS = 8 * WS_MT * 16 * 64;   // the pixel-split reduction area (reuses the staging area)

struct ws_geom {
    int c_in, c_out, HW, w, pad_h, pad_w;
    int RF, CF;                 // padded row length, padded channel stride of img
    int CP, cw, cwp, hp, PP;    // conv plane, g row pitch, pixel pairs per row / per plane
    int GLD, o_g;               // g row stride (odd: 32 rows -> 32 banks), float offset of g in LDS
    int KK, kw, N, NT, rowlen;  // taps, columns, column tiles, partial row length
    int TPW, PS, ldsf;          // column tiles per workgroup, pixel split, LDS floats
    any_div dHW, dW, dCP, dCW;
};

struct ws_plan {
    ws_geom g;
    int nsplit, NQ, NS;
};

// channels the column tiles [t0, t0 + TPW) touch, at most, over all workgroups of a launch
static int ws_max_channels(int N, int NT, int KK, int TPW)
{
    int m = 0;
    for (int t0 = 0; t0 < NT; t0 += TPW) {
        const int last = (t0 + TPW < NT ? (t0 + TPW) * 32 : N) - 1;
        const int cg = last / KK - (t0 * 32) / KK + 1;
        if (cg > m) m = cg;
    }
    return m;
}

// The support predicate and the launch layout of the layers this file serves (c_out > 64; narrower layers never get here).
// nchunk = 0: the layout of a full launch (the largest TPW that fits — what dcll_conv_lif_backward_slab_lds reports);
// nchunk > 0: TPW lowered so that nchunk x nsplit x NS approaches WS_TARGET_WG workgroups, within the full launch's LDS.
static int ws_make_plan(const dcll_conv_desc *d, int nchunk, ws_plan *p, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    p->NS = slab_count(d->c_out);
    if (p->NS > SLAB_MAX) return fail(DCLL_ERR_UNSUPPORTED, "more than 65535 slabs of 64 output channels", who);
    const char *too_big = "the smallest working set (one column tile's padded eps1 channels + a slab's rows of the sample's dv "
                          "plane) exceeds the 160 KiB of LDS";
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    ws_geom &g = p->g;
    g.c_in = d->c_in, g.c_out = d->c_out, g.w = d->w, g.pad_h = d->pad_h, g.pad_w = d->pad_w;
    g.KK = d->kh * d->kw, g.kw = d->kw;
    const long HW = (long)d->h * d->w, CF = (long)(d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w), CP = (long)ch * cw;
    const long N = (long)d->c_in * g.KK;
    const long rows = d->c_out < SLAB_ROWS ? d->c_out : SLAB_ROWS;      // g rows of a workgroup: a whole slab's
    g.cw = cw, g.cwp = cw + (cw & 1), g.hp = g.cwp / 2;
    const long grow = (long)ch * g.cwp, GLD = grow | 1;
    if (CF + 1 + rows * GLD > WS_LDS_MAX_FLOATS) return fail(DCLL_ERR_UNSUPPORTED, too_big, who);
    if (N >= (1L << 30)) return fail(DCLL_ERR_UNSUPPORTED, "c_in kh kw < 2^30", who);
    g.HW = (int)HW, g.RF = d->w + 2 * d->pad_w, g.CF = (int)CF, g.CP = (int)CP, g.PP = (int)(grow / 2), g.GLD = (int)GLD;
    g.N = (int)N, g.NT = (int)((N + 31) / 32), g.rowlen = (int)N + 1;
    // the full launch: the largest TPW whose channels fit
    auto img_floats = [&](int tpw) { return (long)((ws_max_channels(g.N, g.NT, g.KK, tpw) * CF + 1 + 3) & ~3L); };
    int TPW = g.NT < WS_MAX_TPW ? g.NT : WS_MAX_TPW;
    long ldsf = 0;
    for (;; --TPW) {
        if (TPW < 1) return fail(DCLL_ERR_UNSUPPORTED, too_big, who);
        ldsf = img_floats(TPW) + rows * GLD;
        if (ldsf <= WS_LDS_MAX_FLOATS) break;
    }
    const long wg = (long)nchunk * p->NS;                               // workgroups before any column split
    if (nchunk > 0 && wg < WS_TARGET_WG) {
        // a small batch: fewer tiles per workgroup, but never more LDS than the full launch (a shorter tile range can straddle
        // one input channel more than any range of the full layout): the first TPW from the wanted one upwards whose set is no
        // larger is taken; the full TPW always qualifies
        int want = (int)((WS_TARGET_WG + wg - 1) / wg);
        if (want > g.NT) want = g.NT;
        for (int tpw = (g.NT + want - 1) / want; tpw < TPW; ++tpw) {
            const long f = img_floats(tpw) + rows * GLD;
            if (f <= (ldsf > WS_RED_FLOATS ? ldsf : WS_RED_FLOATS)) {      // (every launch has at least the reduction area)
                TPW = tpw, ldsf = f;
                break;
            }
        }
    }
    g.o_g = (int)img_floats(TPW);
    if (ldsf < WS_RED_FLOATS) ldsf = WS_RED_FLOATS;
    g.TPW = TPW, g.ldsf = (int)ldsf;
    g.PS = TPW >= 5 ? 1 : TPW >= 3 ? 2 : TPW == 2 ? 4 : 8;
    p->nsplit = (g.NT + TPW - 1) / TPW;
    if (p->nsplit > 65535) return fail(DCLL_ERR_UNSUPPORTED, "more than 65535 column splits", who);
    const int nq = g.PS > 1 ? 1 : (TPW + 7) / 8;
    p->NQ = nq == 3 ? 4 : nq;
    // (the staging loops divide by these: every numerator is below the LDS size in floats, 40960, so n d < 2^32)
    g.dHW = make_div(g.HW), g.dW = make_div(g.w), g.dCP = make_div(g.CP), g.dCW = make_div(g.cw);
    return DCLL_OK;
}

extern "C" int64_t dcll_conv_lif_backward_slab_lds(const dcll_conv_desc *d)
{
    if (d && d->c_out <= SLAB_ROWS) return dcll_conv_lif_backward_wide_lds(d);    // (forwarded layers: that path's answer)
    ws_plan p;
    return ws_make_plan(d, 0, &p, "dcll_conv_lif_backward_slab_lds") == DCLL_OK ? (int64_t)p.g.ldsf * 4 : 0;
}

int dcll_bwd_wgrad_slab_check(const dcll_conv_desc *d, const char *who)
{
    ws_plan p;
    return ws_make_plan(d, 0, &p, who);
}

// NQ: column tiles of a wave, each with WS_MT accumulator tiles.  Wave w = (tile lane tl = w / PS, pixel segment seg = w % PS)
// owns the column tiles t0 + tl + (8 / PS) q, q < NQ, of its workgroup over the pixel pairs [seg PPs, (seg + 1) PPs), and
// both M tiles of each.  A tile beyond the workgroup's range is computed on the columns of tile t0 and not stored.
template <int NQ>
__global__ __launch_bounds__(WS_THREADS) void k_bwd_wgrad_slab(const ws_geom g, const float *__restrict__ gvf,
                                                               const float *__restrict__ eps1, float *__restrict__ part, int B)
{
    extern __shared__ float lds[];
    float *img = lds, *gl = lds + g.o_g;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int PS = g.PS, NTL = 8 / PS, seg = w % PS, tl = w / PS;
    const int co0 = slab_first(blockIdx.z), nrow = slab_rows(blockIdx.z, g.c_out);     // the slab: channels [co0, co0 + nrow)
    const int t0 = blockIdx.y * g.TPW, t1 = min(g.NT, t0 + g.TPW);
    const int c0 = (t0 * 32) / g.KK, c1 = (min(t1 * 32, g.N) - 1) / g.KK, cgn = c1 - c0 + 1;
    int nq = 0, bbase[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int t = t0 + tl + NTL * q;
        if (t < t1) nq = q + 1;
        const int n = min((t < t1 ? t : t0) * 32 + j, g.N - 1);
        const int ci = n / g.KK, tap = n - ci * g.KK, ty = tap / g.kw, tx = tap - ty * g.kw;
        bbase[q] = (ci - c0) * g.CF + ty * g.RF + tx + h;
        asm volatile("" : "+v"(bbase[q]));                     // one register per column base: else the sum is redone per read
    }
    f32x16 acc[WS_MT][NQ];
#pragma unroll
    for (int m = 0; m < WS_MT; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.0f;
    float bacc[8];                                            // bias gradient: wave w, slab rows w + 8 k, pixels lane + 64 i
#pragma unroll
    for (int k = 0; k < 8; ++k) bacc[k] = 0.0f;
    const bool bias_wg = blockIdx.y == 0;
    const int PPs = (g.PP + PS - 1) / PS, p0 = min(g.PP, seg * PPs), p1 = min(g.PP, p0 + PPs);
    const int y0 = p0 / g.hp, xp0 = p0 - y0 * g.hp;
    // zero once: the padding of img, the pad float of odd g rows and the slack are never written again
    for (int i = tid; i < g.ldsf; i += WS_THREADS) lds[i] = 0.0f;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        const float *gs = gvf + ((long)b * g.c_out + co0) * g.CP;      // the slab's rows of the sample's dv plane
        for (int i = tid; i < nrow * g.CP; i += WS_THREADS) {
            const int r = fdiv(i, g.dCP), s = i - r * g.CP, y = fdiv(s, g.dCW), x = s - y * g.cw;
            gl[r * g.GLD + y * g.cwp + x] = gs[i];
        }
        const float *es = eps1 + ((long)b * g.c_in + c0) * g.HW;
        for (int i = tid; i < cgn * g.HW; i += WS_THREADS) {
            const int c = fdiv(i, g.dHW), r = i - c * g.HW, y = fdiv(r, g.dW), x = r - y * g.w;
            img[c * g.CF + (y + g.pad_h) * g.RF + x + g.pad_w] = es[i];
        }
        __syncthreads();
        if (bias_wg) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int r = w + 8 * k;
                if (r < nrow)
                    for (int p = lane; p < 2 * g.PP; p += 64) bacc[k] += gl[r * g.GLD + p];
            }
        }
        if (nq > 0) {
            // A: slab rows j and 32 + j (rows at or beyond the slab's last read its last real row: not stored), pixel + h
            const float *ga0 = gl + min(j, nrow - 1) * g.GLD + h, *ga1 = gl + min(32 + j, nrow - 1) * g.GLD + h;
            // the operands of pair pp + 1 are read while the MFMAs of pair pp run (the last pair reads its own again)
            int xp = xp0, ioff = y0 * g.RF + 2 * xp0;
            float a0 = 0.0f, a1 = 0.0f, bv[NQ];
            if (p0 < p1) {
                a0 = ga0[2 * p0], a1 = ga1[2 * p0];
#pragma unroll
                for (int q = 0; q < NQ; ++q) bv[q] = img[bbase[q] + ioff];
            }
            for (int pp = p0; pp < p1; ++pp) {
                if (pp + 1 < p1) {
                    ++xp, ioff += 2;
                    if (xp == g.hp) xp = 0, ioff += g.RF - g.cwp;
                }
                const int pn = 2 * min(pp + 1, p1 - 1);
                const float an0 = ga0[pn], an1 = ga1[pn];
                float bn[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) bn[q] = img[bbase[q] + ioff];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[q], acc[0][q], 0, 0, 0);
                    acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[q], acc[1][q], 0, 0, 0);
                }
                a0 = an0, a1 = an1;
#pragma unroll
                for (int q = 0; q < NQ; ++q) bv[q] = bn[q];
            }
        }
    }
    float *prow = part + ((long)blockIdx.x * g.c_out + co0) * g.rowlen;     // the slab's rows of this chunk's partial rows
    if (NQ > 1 || PS == 1) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int n = (t0 + tl + NTL * q) * 32 + j;
            if (q < nq && n < g.N) {
#pragma unroll
                for (int m = 0; m < WS_MT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (row < nrow) prow[(long)row * g.rowlen + n] = acc[m][q][r];
                    }
            }
        }
    } else {
        // pixel split: the PS pieces of a tile through LDS (the staging area is free), added in wave (= segment) order
        __syncthreads();
#pragma unroll
        for (int m = 0; m < WS_MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) lds[((w * WS_MT + m) * 16 + r) * 64 + lane] = acc[m][0][r];
        __syncthreads();
        for (int e = tid; e < NTL * WS_MT * 1024; e += WS_THREADS) {
            const int tl2 = e >> 11, m = (e >> 10) & 1, r = (e >> 6) & 15, l = e & 63;
            const int n = (t0 + tl2) * 32 + (l & 31), row = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            if (t0 + tl2 >= t1 || n >= g.N || row >= nrow) continue;
            float tot = lds[(((tl2 * PS) * WS_MT + m) * 16 + r) * 64 + l];
            for (int s = 1; s < PS; ++s) tot += lds[(((tl2 * PS + s) * WS_MT + m) * 16 + r) * 64 + l];
            prow[(long)row * g.rowlen + n] = tot;
        }
    }
    if (bias_wg) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = w + 8 * k;
            if (r < nrow) {                                     // (wave-uniform)
                const float tot = wave_sum_to_lane63(bacc[k]);
                if (lane == 63) prow[(long)r * g.rowlen + g.N] = tot;
            }
        }
    }
}

template <int NQ>
static int ws_launch(const ws_plan &p, int nchunk, const float *gvf, const float *eps1, float *part, int B, hipStream_t st,
                     const char *name)
{
    const size_t lds_bytes = (size_t)p.g.ldsf * sizeof(float);
    static bool reserved = false;       // (per template instance; the attribute is the kernel's ceiling, set once to all 160 KiB)
    if (!reserved) {
        if (hipFuncSetAttribute((const void *)k_bwd_wgrad_slab<NQ>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(WS_LDS_MAX_FLOATS * sizeof(float))) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_slab: cannot reserve its LDS");
        }
        reserved = true;
    }
    hipLaunchKernelGGL(k_bwd_wgrad_slab<NQ>, dim3((unsigned)nchunk, (unsigned)p.nsplit, (unsigned)p.NS), dim3(WS_THREADS), lds_bytes,
                       st, p.g, gvf, eps1, part, B);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

// gvf: the dv plane (B, c_out, ch, cw); part: room for *nchunk partial rows on entry, the number written on return
int dcll_launch_bwd_wgrad_slab(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B,
                               long *nchunk, hipStream_t st)
{
    const char *who = "dcll_conv_lif_backward_slab";
    long nc = *nchunk;
    if (nc > WS_MAX_CHUNKS) nc = WS_MAX_CHUNKS;
    if (nc > B) nc = B;
    ws_plan p;
    int rc = ws_make_plan(d, (int)nc, &p, who);
    if (rc) return rc;
    // the layout against the exported predicate: a launch never needs more LDS than dcll_conv_lif_backward_slab_lds reports
    // (ws_make_plan keeps it so; conv_lif_backward_impl has run the predicate before the dv launch)
    if (d->c_out <= SLAB_ROWS || p.NS != slab_count(d->c_out) || p.NS < 2 || p.NS > SLAB_MAX || nc < 1 ||
        (int64_t)p.g.ldsf * 4 > dcll_conv_lif_backward_slab_lds(d) || p.g.ldsf > WS_LDS_MAX_FLOATS || p.g.ldsf < WS_RED_FLOATS ||
        p.g.o_g + (long)SLAB_ROWS * p.g.GLD > p.g.ldsf || p.g.TPW > 8 * p.NQ || (p.g.PS > 1 && (p.NQ != 1 || p.g.TPW * p.g.PS > 8)))
        return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_slab: launch layout outside the predicate's", who);
    static const char *const names[3][4] = {
        {"k_bwd_wgrad_slab<1>", "k_bwd_wgrad_slab<1> (column split)", "k_bwd_wgrad_slab<1> (pixel split)",
         "k_bwd_wgrad_slab<1> (column split, pixel split)"},
        {"k_bwd_wgrad_slab<2>", "k_bwd_wgrad_slab<2> (column split)", nullptr, nullptr},
        {"k_bwd_wgrad_slab<4>", "k_bwd_wgrad_slab<4> (column split)", nullptr, nullptr}};
    const int v = (p.nsplit > 1 ? 1 : 0) + (p.g.PS > 1 ? 2 : 0);
    if (p.NQ == 1) rc = ws_launch<1>(p, (int)nc, gvf, eps1, part, B, st, names[0][v]);
    else if (p.NQ == 2) rc = ws_launch<2>(p, (int)nc, gvf, eps1, part, B, st, names[1][v]);
    else rc = ws_launch<4>(p, (int)nc, gvf, eps1, part, B, st, names[2][v]);
    *nchunk = nc;
    return rc;
}
