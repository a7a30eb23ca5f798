// dcll_bwd_band.hip — k_bwd_wgrad_band: the weight gradient of a plain conv layer (stride = dilation = groups = 1, kernel up to
// 16x16, any c_in, c_out, padding, pooling, batch) on fp32 MFMA tiles for ANY plane height (dcll_conv_lif_backward_bands[_open]).
// k_bwd_wgrad_any / _wide / _slab stage a whole sample in LDS (the padded eps1 image of a column range + every row of the
// sample's dv plane) and refuse a layer whose sample does not fit.  A row of dW is a sum over samples and pixels, and the pixel
// pairs of the MFMA never leave an image row: a sample is cut into NB bands of RB conv-output rows, and a workgroup adds band
// after band exactly as k_bwd_wgrad_slab adds sample after sample.  A translation unit of its own: the existing kernels and their
// ISA are untouched; the geometry and the plan are restated here (wb_geom, wb_make_plan; tests/bwd_band_cases.py restates both).
//
//   dW[co][n] = sum_{b,pix} g[b,co,pix] * E[b][n][pix],  n = ci kh kw + tap,   db[co] = sum g
//
// A job is (sample b, band k), job = b NB + k; band k covers the conv rows [min(ch, k RB), min(ch, (k + 1) RB)), rb of them.  Workgroup
// (chunk, column split, slab) runs the jobs chunk, chunk + nchunk, ... in order, accumulates over all of them in registers and
// stores part[chunk][co][c_in kh kw + 1] once — the format k_bwd_reduce[4] / dcll_grad_reduce_adam consume.  Per job it stages
//   img   cg x (RB + kh - 1) x RF + 1     the rb + kh - 1 padded input rows under the band, of the input channels of ITS column
//                                         tiles (RF = w + 2 pad_w; channel stride (RB + kh - 1) RF)
//   g     rows x GLD                      the band's rows of ITS SLAB's dv rows, pitch cwp = cw rounded up to even, the tail of
//                                         an odd row ZERO; GLD = (RB cwp) | 1; rows = min(c_out, 32 MT)
// LDS does not grow with the plane height.  The image's top and bottom zero rows belong to a band, not to the launch: the staging
// loop of EVERY job writes every staged image row over the w data columns — data where the input row exists, 0.0f where it is
// padding; the left and right pad columns, the pad float of odd g rows and the slack float are zeroed once.  A short last band
// (rb < RB) runs its pixel pairs, its pixel-split segments and its bias sum over rb rows: the rows behind them hold the previous
// job's data and are never read.
//
// MT = 1 serves c_out <= 32 (one 32-row M tile), MT = 2 slabs of 64 (the slab rule: dcll_any_shared.h; blockIdx.z).  Carried over
// from k_bwd_wgrad_slab: one B-operand read feeds both M tiles; the odd-cw rule; column split; pixel split (TPW < 5: PS = 2 / 4 /
// 8, pieces through LDS, added in wave order); the next-pair prefetch; "a tile beyond the range is computed on the first tile's
// columns and not stored"; at most 256 chunks; every sum has a fixed order.  The plan is a pure function of (descriptor, B, bands).
#include "dcll_any_shared.h"

constexpr int WB_THREADS = 512;
constexpr long WB_LDS_MAX_FLOATS = ANY_LDS_MAX / 4;
constexpr int WB_MAX_TPW = 32;                   // column tiles per workgroup: 8 waves x 4 column tiles
constexpr int WB_MAX_CHUNKS = 256;               // chunks of jobs (= partial rows)
constexpr int WB_TARGET_WG = ANY_CUS;            // workgroups a launch aims at (one per CU)
static inline int wb_red_floats(int MT) { return 8 * MT * 16 * 64; }    // the pixel-split reduction area (reuses the staging area)

struct wb_geom {
    int c_in, c_out, h, w, pad_h, pad_w, kh;
    int RF, IR, CFB;            // padded row length, staged image rows of a full band (RB + kh - 1), channel stride IR RF
    int HW, CP, ch, cw, cwp, hp;
    int RB, NB;                 // rows of a full band, bands of a sample
    int GLD, o_g;               // g row stride (odd), float offset of g in LDS
    int KK, kw, N, NT, rowlen;  // taps, columns, column tiles, partial row length
    int TPW, PS, ldsf;          // column tiles per workgroup, pixel split, LDS floats
    int njob;                   // B NB
    any_div dGB, dCW, dIB, dW;  // RB cw, cw, IR w, w
};

struct wb_plan {
    wb_geom g;
    int nsplit, NQ, NS, MT, rows;
};

// channels the column tiles [t0, t0 + TPW) touch, at most, over all workgroups of a launch
static int wb_max_channels(int N, int NT, int KK, int TPW)
{
    int m = 0;
    for (int t0 = 0; t0 < NT; t0 += TPW) {
        const int last = (t0 + TPW < NT ? (t0 + TPW) * 32 : N) - 1;
        const int cg = last / KK - (t0 * 32) / KK + 1;
        if (cg > m) m = cg;
    }
    return m;
}

// The support predicate and the launch layout of a banded call: bands >= 2 forced (exactly that many bands of ceil(ch / bands)
// rows), bands == 0 the rule (callers hand bands == 1, and bands == 0 where dcll_conv_lif_backward_slab serves the layer, to
// that call and never get here with them — a bands == 0 that does get here is a layer the slab call refuses).
// The rule: the largest TPW <= min(NT, 32) at which a band of min(ch, kh) rows fits (failing that at every TPW: at which ONE row
// fits), then the largest RB that fits beside it, NB = ceil(ch / RB), RB = ceil(ch / NB).
// nchunk = 0: the layout of a full launch (what dcll_conv_lif_backward_bands_lds reports); nchunk > 0: TPW lowered so that
// nchunk x nsplit x NS approaches WB_TARGET_WG workgroups, within the full launch's LDS.
static int wb_make_plan(const dcll_conv_desc *d, int bands, long B, int nchunk, wb_plan *p, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (bands < 0) return fail(DCLL_ERR_UNSUPPORTED, "bands >= 0 (0: the library's rule)", who);
    if (bands > ch) return fail(DCLL_ERR_UNSUPPORTED, "more bands than conv-output rows", who);
    p->MT = d->c_out <= 32 ? 1 : 2;
    p->NS = p->MT == 1 ? 1 : slab_count(d->c_out);
    if (p->NS > SLAB_MAX) return fail(DCLL_ERR_UNSUPPORTED, "more than 65535 slabs of 64 output channels", who);
    const long rows = d->c_out < 32 * p->MT ? d->c_out : 32 * p->MT;    // g rows of a workgroup
    p->rows = (int)rows;
    wb_geom &g = p->g;
    g.c_in = d->c_in, g.c_out = d->c_out, g.h = d->h, g.w = d->w, g.pad_h = d->pad_h, g.pad_w = d->pad_w, g.kh = d->kh;
    g.KK = d->kh * d->kw, g.kw = d->kw;
    const long N = (long)d->c_in * g.KK;
    if (N >= (1L << 30)) return fail(DCLL_ERR_UNSUPPORTED, "c_in kh kw < 2^30", who);
    g.RF = d->w + 2 * d->pad_w, g.HW = d->h * d->w, g.CP = ch * cw, g.ch = ch, g.cw = cw, g.cwp = cw + (cw & 1), g.hp = g.cwp / 2;
    g.N = (int)N, g.NT = (int)((N + 31) / 32), g.rowlen = (int)N + 1;
    const int red = wb_red_floats(p->MT);
    auto img_floats = [&](int tpw, int rb) {
        return ((long)wb_max_channels(g.N, g.NT, g.KK, tpw) * (rb + d->kh - 1) * g.RF + 1 + 3) & ~3L;
    };
    auto floats = [&](int tpw, int rb) { return img_floats(tpw, rb) + rows * (((long)rb * g.cwp) | 1); };
    const char *too_big = "not even a one-row band with one column tile (its padded eps1 rows + a slab's rows of that dv row) "
                          "fits the 160 KiB of LDS";
    int TPW = g.NT < WB_MAX_TPW ? g.NT : WB_MAX_TPW, RB;
    if (bands >= 1) {
        RB = (ch + bands - 1) / bands;             // (exactly `bands` bands: the last ones are empty where bands RB - RB >= ch)
        for (; TPW >= 1 && floats(TPW, RB) > WB_LDS_MAX_FLOATS; --TPW) {}
        if (TPW < 1) return fail(DCLL_ERR_UNSUPPORTED, "a band of the forced plan (its padded eps1 rows of one column tile + a slab's rows of the band's dv rows) exceeds the 160 KiB of LDS", who);
    } else {
        const int want_rows = ch < d->kh ? ch : d->kh, top = TPW;
        for (; TPW >= 1 && floats(TPW, want_rows) > WB_LDS_MAX_FLOATS; --TPW) {}
        if (TPW < 1)                                // (rows too wide for kh of them: the largest TPW beside ONE row)
            for (TPW = top; TPW >= 1 && floats(TPW, 1) > WB_LDS_MAX_FLOATS; --TPW) {}
        if (TPW < 1) return fail(DCLL_ERR_UNSUPPORTED, too_big, who);
        int lo = 1, hi = ch;                        // the largest RB that fits (floats grows with RB)
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (floats(TPW, mid) <= WB_LDS_MAX_FLOATS) lo = mid;
            else hi = mid - 1;
        }
        const int nb = (ch + lo - 1) / lo;
        RB = (ch + nb - 1) / nb;
    }
    g.RB = RB, g.NB = bands >= 1 ? bands : (ch + RB - 1) / RB;
    if (B * g.NB >= (1L << 31)) return fail(DCLL_ERR_UNSUPPORTED, "B x bands < 2^31", who);
    g.njob = (int)(B * g.NB);
    long ldsf = floats(TPW, RB);
    const long wg = (long)nchunk * p->NS;                               // workgroups before any column split
    if (nchunk > 0 && wg < WB_TARGET_WG) {
        // few jobs: fewer tiles per workgroup, but never more LDS than the full launch (a shorter tile range can straddle one
        // input channel more than any range of the full layout): the first TPW from the wanted one upwards whose set is no larger
        int want = (int)((WB_TARGET_WG + wg - 1) / wg);
        if (want > g.NT) want = g.NT;
        for (int tpw = (g.NT + want - 1) / want; tpw < TPW; ++tpw) {
            const long f = floats(tpw, RB);
            if (f <= (ldsf > red ? ldsf : red)) {
                TPW = tpw, ldsf = f;
                break;
            }
        }
    }
    g.IR = RB + d->kh - 1, g.CFB = g.IR * g.RF, g.GLD = (RB * g.cwp) | 1;
    g.o_g = (int)img_floats(TPW, RB);
    if (ldsf < red) ldsf = red;
    g.TPW = TPW, g.ldsf = (int)ldsf;
    g.PS = TPW >= 5 ? 1 : TPW >= 3 ? 2 : TPW == 2 ? 4 : 8;
    p->nsplit = (g.NT + TPW - 1) / TPW;
    if (p->nsplit > 65535) return fail(DCLL_ERR_UNSUPPORTED, "more than 65535 column splits", who);
    const int nq = g.PS > 1 ? 1 : (TPW + 7) / 8;
    p->NQ = nq == 3 ? 4 : nq;
    // (the staging loops divide by these: every numerator is below the LDS size in floats, 40960, so n d < 2^32)
    g.dGB = make_div(RB * cw), g.dCW = make_div(cw), g.dIB = make_div(g.IR * d->w), g.dW = make_div(d->w);
    return DCLL_OK;
}

// the invariants of a launch layout (the launcher re-checks them; experiments/asan_bwd_band_plan.hip walks them)
static bool wb_plan_ok(const wb_plan &p)
{
    const wb_geom &g = p.g;
    const int cgmax = wb_max_channels(g.N, g.NT, g.KK, g.TPW);
    // the last B-operand read of the last pair of a full band: last channel, last tap, half 1, last row, last pixel pair
    const long last_b = (long)(cgmax - 1) * g.CFB + (long)(g.kh - 1) * g.RF + (g.kw - 1) + 1 + (long)(g.RB - 1) * g.RF + 2 * (g.hp - 1);
    return g.RB >= 1 && g.NB >= 1 && (long)g.NB * g.RB >= g.ch && last_b < g.o_g &&
           g.o_g + (long)p.rows * g.GLD <= g.ldsf && g.ldsf <= WB_LDS_MAX_FLOATS && g.ldsf >= wb_red_floats(p.MT) &&
           g.GLD >= g.RB * g.cwp && g.TPW >= 1 && g.TPW <= 8 * p.NQ && (g.PS == 1 || (p.NQ == 1 && g.TPW * g.PS <= 8)) &&
           (p.MT == 1 ? (g.c_out <= 32 && p.NS == 1) : (g.c_out > 32 && p.NS == slab_count(g.c_out))) && p.NS <= SLAB_MAX &&
           p.nsplit >= 1 && p.nsplit <= 65535 && (long)p.nsplit * g.TPW >= g.NT;
}

// bands == 1, and bands == 0 on a layer dcll_conv_lif_backward_slab serves: the call IS that call (dcll_hip.hip hands it over)
bool dcll_bwd_band_forwards(const dcll_conv_desc *d, int32_t bands)
{
    return bands == 1 || (bands == 0 && dcll_conv_lif_backward_slab_lds(d) > 0);
}

extern "C" int64_t dcll_conv_lif_backward_bands_lds(const dcll_conv_desc *d, int32_t bands)
{
    if (dcll_bwd_band_forwards(d, bands)) return dcll_conv_lif_backward_slab_lds(d);
    wb_plan p;
    return wb_make_plan(d, bands, 1, 0, &p, "dcll_conv_lif_backward_bands_lds") == DCLL_OK ? (int64_t)p.g.ldsf * 4 : 0;
}

// host only, launches nothing: out = NB, RB, TPW, PS, NQ, NS, column splits, nchunk of the call with an unlimited scratch.
// A forwarded call (above) reports NB = 1, RB = ch, its slabs and min(B, 256) chunks; TPW, PS, NQ and the column splits are that
// call's own plan and are reported as 0.
extern "C" int dcll_conv_lif_backward_bands_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int32_t out[8])
{
    const char *who = "dcll_conv_lif_backward_bands_plan";
    if (!out) return fail(DCLL_ERR_INVALID, "null out", who);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (B < 1) return fail(DCLL_ERR_INVALID, "empty batch", who);
    if (dcll_bwd_band_forwards(d, bands)) {
        if (dcll_conv_lif_backward_slab_lds(d) <= 0) return DCLL_ERR_UNSUPPORTED;       // (that call's message stands)
        int ch, cw, ph, pw;
        conv_shape(d, &ch, &cw, &ph, &pw);
        out[0] = 1, out[1] = ch, out[5] = d->c_out > SLAB_ROWS ? slab_count(d->c_out) : 1;
        out[7] = B < WB_MAX_CHUNKS ? B : WB_MAX_CHUNKS;
        return DCLL_OK;
    }
    wb_plan p;
    int rc = wb_make_plan(d, bands, B, 0, &p, who);
    if (rc) return rc;
    const long nc = p.g.njob < WB_MAX_CHUNKS ? p.g.njob : WB_MAX_CHUNKS;
    if ((rc = wb_make_plan(d, bands, B, (int)nc, &p, who)) != DCLL_OK) return rc;
    out[0] = p.g.NB, out[1] = p.g.RB, out[2] = p.g.TPW, out[3] = p.g.PS, out[4] = p.NQ, out[5] = p.NS, out[6] = p.nsplit;
    out[7] = (int32_t)nc;
    return DCLL_OK;
}

int dcll_bwd_wgrad_band_check(const dcll_conv_desc *d, int32_t bands, const char *who)
{
    wb_plan p;
    return wb_make_plan(d, bands, 1, 0, &p, who);
}

// MT: 32-row M tiles of a workgroup (its slab's rows); NQ: column tiles of a wave, each with MT accumulator tiles.  Wave w =
// (tile lane tl = w / PS, pixel segment seg = w % PS) owns the column tiles t0 + tl + (8 / PS) q, q < NQ, of its workgroup over
// the job's pixel pairs [seg PPs, (seg + 1) PPs), and all M tiles of each.  A tile beyond the workgroup's range is computed on
// the columns of tile t0 and not stored.
template <int MT, int NQ>
__global__ __launch_bounds__(WB_THREADS) void k_bwd_wgrad_band(const wb_geom g, const float *__restrict__ gvf,
                                                               const float *__restrict__ eps1, float *__restrict__ part)
{
    extern __shared__ float lds[];
    float *img = lds, *gl = lds + g.o_g;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int PS = g.PS, NTL = 8 / PS, seg = w % PS, tl = w / PS;
    const int co0 = blockIdx.z * SLAB_ROWS, nrow = min(g.c_out - co0, 32 * MT);        // the slab: channels [co0, co0 + nrow)
    const int t0 = blockIdx.y * g.TPW, t1 = min(g.NT, t0 + g.TPW);
    const int c0 = (t0 * 32) / g.KK, c1 = (min(t1 * 32, g.N) - 1) / g.KK, cgn = c1 - c0 + 1;
    int nq = 0, bbase[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int t = t0 + tl + NTL * q;
        if (t < t1) nq = q + 1;
        const int n = min((t < t1 ? t : t0) * 32 + j, g.N - 1);
        const int ci = n / g.KK, tap = n - ci * g.KK, ty = tap / g.kw, tx = tap - ty * g.kw;
        bbase[q] = (ci - c0) * g.CFB + ty * g.RF + tx + h;
        asm volatile("" : "+v"(bbase[q]));                     // one register per column base: else the sum is redone per read
    }
    f32x16 acc[MT][NQ];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.0f;
    float bacc[4 * MT];                                       // bias gradient: wave w, slab rows w + 8 k, pixels lane + 64 i
#pragma unroll
    for (int k = 0; k < 4 * MT; ++k) bacc[k] = 0.0f;
    const bool bias_wg = blockIdx.y == 0;
    // zero once: the pad columns of img, the pad float of odd g rows and the slack are never written again
    for (int i = tid; i < g.ldsf; i += WB_THREADS) lds[i] = 0.0f;
    for (int job = blockIdx.x; job < g.njob; job += gridDim.x) {
        const int b = job / g.NB, k = job - b * g.NB;
        const int r0 = k * g.RB, rb = min(g.RB, g.ch - r0);                 // the band: conv rows [r0, r0 + rb)
        if (rb <= 0) continue;                                              // (a forced band count can leave empty last bands)
        __syncthreads();
        const float *gs = gvf + ((long)b * g.c_out + co0) * g.CP + r0 * g.cw;   // the band's rows of the slab's rows of the dv plane
        for (int i = tid; i < nrow * g.RB * g.cw; i += WB_THREADS) {
            const int r = fdiv(i, g.dGB), s = i - r * (g.RB * g.cw), y = fdiv(s, g.dCW), x = s - y * g.cw;
            if (y < rb) gl[r * g.GLD + y * g.cwp + x] = gs[(long)r * g.CP + s];
        }
        // every staged image row of the job: input row r0 + yy - pad_h, or 0.0f where that is the image's zero padding
        const float *es = eps1 + ((long)b * g.c_in + c0) * g.HW;
        const int iy0 = r0 - g.pad_h, nir = rb + g.kh - 1;
        for (int i = tid; i < cgn * g.IR * g.w; i += WB_THREADS) {
            const int c = fdiv(i, g.dIB), r = i - c * (g.IR * g.w), yy = fdiv(r, g.dW), x = r - yy * g.w, iy = iy0 + yy;
            if (yy < nir) img[c * g.CFB + yy * g.RF + x + g.pad_w] = (iy >= 0 && iy < g.h) ? es[(long)c * g.HW + iy * g.w + x] : 0.0f;
        }
        __syncthreads();
        if (bias_wg) {
#pragma unroll
            for (int k2 = 0; k2 < 4 * MT; ++k2) {
                const int r = w + 8 * k2;
                if (r < nrow)
                    for (int p = lane; p < rb * g.cwp; p += 64) bacc[k2] += gl[r * g.GLD + p];
            }
        }
        if (nq > 0) {
            const int PP = rb * g.hp;                                       // the job's own pixel pairs
            const int PPs = (PP + PS - 1) / PS, p0 = min(PP, seg * PPs), p1 = min(PP, p0 + PPs);
            const int y0 = p0 / g.hp, xp0 = p0 - y0 * g.hp;
            // A: slab rows j and 32 + j (rows at or beyond the slab's last read its last real row: not stored), pixel + h
            const float *ga[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) ga[m] = gl + min(32 * m + j, nrow - 1) * g.GLD + h;
            // the operands of pair pp + 1 are read while the MFMAs of pair pp run (the last pair reads its own again)
            int xp = xp0, ioff = y0 * g.RF + 2 * xp0;
            float a[MT], bv[NQ];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = 0.0f;
            if (p0 < p1) {
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = ga[m][2 * p0];
#pragma unroll
                for (int q = 0; q < NQ; ++q) bv[q] = img[bbase[q] + ioff];
            }
            for (int pp = p0; pp < p1; ++pp) {
                if (pp + 1 < p1) {
                    ++xp, ioff += 2;
                    if (xp == g.hp) xp = 0, ioff += g.RF - g.cwp;
                }
                const int pn = 2 * min(pp + 1, p1 - 1);
                float an[MT], bn[NQ];
#pragma unroll
                for (int m = 0; m < MT; ++m) an[m] = ga[m][pn];
#pragma unroll
                for (int q = 0; q < NQ; ++q) bn[q] = img[bbase[q] + ioff];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bv[q], acc[m][q], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = an[m];
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
                for (int m = 0; m < MT; ++m)
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
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) lds[((w * MT + m) * 16 + r) * 64 + lane] = acc[m][0][r];
        __syncthreads();
        for (int e = tid; e < NTL * MT * 1024; e += WB_THREADS) {
            const int tl2 = e / (MT * 1024), m = (e >> 10) % MT, r = (e >> 6) & 15, l = e & 63;
            const int n = (t0 + tl2) * 32 + (l & 31), row = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
            if (t0 + tl2 >= t1 || n >= g.N || row >= nrow) continue;
            float tot = lds[(((tl2 * PS) * MT + m) * 16 + r) * 64 + l];
            for (int s = 1; s < PS; ++s) tot += lds[(((tl2 * PS + s) * MT + m) * 16 + r) * 64 + l];
            prow[(long)row * g.rowlen + n] = tot;
        }
    }
    if (bias_wg) {
#pragma unroll
        for (int k = 0; k < 4 * MT; ++k) {
            const int r = w + 8 * k;
            if (r < nrow) {                                     // (wave-uniform)
                const float tot = wave_sum_to_lane63(bacc[k]);
                if (lane == 63) prow[(long)r * g.rowlen + g.N] = tot;
            }
        }
    }
}

template <int MT, int NQ>
static int wb_launch(const wb_plan &p, int nchunk, const float *gvf, const float *eps1, float *part, hipStream_t st,
                     const char *name)
{
    const size_t lds_bytes = (size_t)p.g.ldsf * sizeof(float);
    static bool reserved = false;       // (per template instance; the attribute is the kernel's ceiling, set once to all 160 KiB)
    if (!reserved) {
        if (hipFuncSetAttribute((const void *)k_bwd_wgrad_band<MT, NQ>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(WB_LDS_MAX_FLOATS * sizeof(float))) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_band: cannot reserve its LDS");
        }
        reserved = true;
    }
    hipLaunchKernelGGL((k_bwd_wgrad_band<MT, NQ>), dim3((unsigned)nchunk, (unsigned)p.nsplit, (unsigned)p.NS), dim3(WB_THREADS),
                       lds_bytes, st, p.g, gvf, eps1, part);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

// gvf: the dv plane (B, c_out, ch, cw); part: room for *nchunk partial rows on entry, the number written on return
int dcll_launch_bwd_wgrad_band(const dcll_conv_desc *d, int32_t bands, const float *gvf, const float *eps1, float *part, int32_t B,
                               long *nchunk, hipStream_t st)
{
    const char *who = "dcll_conv_lif_backward_bands";
    wb_plan p;
    int rc = wb_make_plan(d, bands, B, 0, &p, who);
    if (rc) return rc;
    long nc = *nchunk;
    if (nc > WB_MAX_CHUNKS) nc = WB_MAX_CHUNKS;
    if (nc > p.g.njob) nc = p.g.njob;
    if (nc < 1) return fail(DCLL_ERR_INVALID, "no room for a partial row", who);
    if ((rc = wb_make_plan(d, bands, B, (int)nc, &p, who)) != DCLL_OK) return rc;
    // the layout against the exported predicate: a launch never needs more LDS than dcll_conv_lif_backward_bands_lds reports
    if (!wb_plan_ok(p) || (int64_t)p.g.ldsf * 4 > dcll_conv_lif_backward_bands_lds(d, bands) || (bands >= 2 && p.g.NB != bands))
        return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_band: launch layout outside the predicate's", who);
    static const char *const names[2][3][4] = {
        {{"k_bwd_wgrad_band<1,1>", "k_bwd_wgrad_band<1,1> (column split)", "k_bwd_wgrad_band<1,1> (pixel split)",
          "k_bwd_wgrad_band<1,1> (column split, pixel split)"},
         {"k_bwd_wgrad_band<1,2>", "k_bwd_wgrad_band<1,2> (column split)", nullptr, nullptr},
         {"k_bwd_wgrad_band<1,4>", "k_bwd_wgrad_band<1,4> (column split)", nullptr, nullptr}},
        {{"k_bwd_wgrad_band<2,1>", "k_bwd_wgrad_band<2,1> (column split)", "k_bwd_wgrad_band<2,1> (pixel split)",
          "k_bwd_wgrad_band<2,1> (column split, pixel split)"},
         {"k_bwd_wgrad_band<2,2>", "k_bwd_wgrad_band<2,2> (column split)", nullptr, nullptr},
         {"k_bwd_wgrad_band<2,4>", "k_bwd_wgrad_band<2,4> (column split)", nullptr, nullptr}}};
    const int v = (p.nsplit > 1 ? 1 : 0) + (p.g.PS > 1 ? 2 : 0);
#define WB_GO(M_, Q_, I_) rc = wb_launch<M_, Q_>(p, (int)nc, gvf, eps1, part, st, names[M_ - 1][I_][v])
    if (p.MT == 1) {
        if (p.NQ == 1) WB_GO(1, 1, 0);
        else if (p.NQ == 2) WB_GO(1, 2, 1);
        else WB_GO(1, 4, 2);
    } else {
        if (p.NQ == 1) WB_GO(2, 1, 0);
        else if (p.NQ == 2) WB_GO(2, 2, 1);
        else WB_GO(2, 4, 2);
    }
#undef WB_GO
    *nchunk = nc;
    return rc;
}
