// dcll_step_wide.hip — k_lif_step_wide: ONE timestep of a plain conv layer with 33..64 output channels (stride = dilation =
// groups = 1, kernel up to 16x16, any c_in, padding, pooling and batch) in one launch (dcll_conv_lif_step_wide) — the opt-in MFMA
// form of the layers dcll_conv_lif_step serves with k_trace + k_conv_lif[_tiled] + k_pool and dcll_conv_lif_step_any refuses
// (c_out <= 32).  The per-step sibling of k_lif_seq_wide (dcll_seq_wide.hip) and k_lif_step_any's decomposition with TWO 32-row
// M tiles; a layer of at most 32 output channels is handed to dcll_conv_lif_step_any unchanged (dcll_hip.hip), so a network of
// mixed widths goes through one entry point.
//
// LDS of a workgroup (floats; step_wide_lds_floats() is the ONE statement of it, exported as dcll_conv_lif_step_wide_lds):
//   img   c_in x (h + 2 pad_h) x (w + 2 pad_w)   eps1 of this step, zero padded: the B operand of every chain link is one read
//         at ci CHS + (y + ky) WP + x + kx
//   vpl   c_out x ch x cw                        pooling layers only: v at conv resolution (the pooling pass reads windows of it)
//   bias  64
// The weights are not staged: k_step_wide_wprep writes w_scratch in front of this kernel on every call (nothing is cached, the
// learning step changes W through raw pointers), wperm[m][lane][mt] = weight of link 2 m + (lane >> 5) for output channel
// 32 mt + (lane & 31), so a lane fetches both M tiles' A values of a step with ONE 8-byte load; eight steps in flight per wave.
//
// Arithmetic = the contract of include/dcll_hip.h and exactly k_lif_step_any's rule: the chain of output (co, y, x) starts at
// bias[co] and runs over the links (cp, ky, kx, h), ci = 2 cp + h, one v_mfma_f32_32x32x2_f32 per two CONSECUTIVE links; the last
// channel of an odd c_in pairs its taps two by two, and a link beyond the last carries a zero weight and a zero input.
// M = c_out padded to 64 rows (rows at or beyond c_out: zero weights, never stored), N = 32 pixels of the flattened conv plane.
// The two 32-row chains of a pixel tile are independent and each is unsplit, so every v is still ONE fmaf chain.
//
// Fused form (one workgroup per sample): the image pass of k_lif_step_any (traces advanced in it), a barrier, the chains — wave
// w runs pixel tiles w, w + 8, ... and BOTH M tiles of each, interleaved: one LDS read of the B operand feeds two MFMAs — and
// k_lif_step_any's epilogues (from the accumulators without pooling; v plane + refractory pass + pooling pass with pooling).
// Split form (NS > 1 workgroups per sample; layers without pooling, when the batch leaves CUs idle): the work unit is (pixel
// tile, M tile), u = 2 tile + mt; workgroup `part` runs units [part UPW, (part + 1) UPW), wave w the units w, w + 8, ... of that
// range, one chain each.  A single dependent chain of this instruction already issues at full rate, so parting a tile's two M
// tiles costs only the second B read.  The traces are NOT advanced in the kernel (the read-after-write race of k_lif_step_any's
// note): the entry point runs k_trace first and a workgroup stages, read-only, the padded rows its units' tiles touch.  Two
// workgroups may hold the two M tiles of one pixel tile: both stage that tile's rows; their outputs and arp elements are disjoint.
#include "dcll_any_shared.h"
#include <mutex>

constexpr int SW_THREADS = 512, SW_NW = SW_THREADS / 64;
constexpr int SW_MAX_COUT = 64, SW_MT = 2;
constexpr int SW_MAX_DEVICES = 64;
// split rule: units a workgroup should keep (one chain per SIMD when CUs are idle); -D for experiments/build_variant.sh
#ifndef DCLL_STEP_WIDE_UNITS
#define DCLL_STEP_WIDE_UNITS 4
#endif
constexpr int SW_UNITS = DCLL_STEP_WIDE_UNITS;
static_assert(SW_UNITS >= 1, "DCLL_STEP_WIDE_UNITS >= 1");

typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));      // (w_scratch is only 4-byte aligned by contract)

struct step_wide_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int WP, CHS;                // padded row length, padded channel stride of img
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int ns, upw;                // workgroups per sample, (pixel tile, M tile) units per workgroup
    int o_v, o_bias;            // float offsets into LDS (img at 0)
    int tau_is_tensor;
    any_div dCHS, dWP, dCW, dPP, dPW, dNS;
};

static inline bool step_wide_pooled(const dcll_conv_desc *d) { return !(d->pool_h == 1 && d->pool_w == 1); }

// the working set of a workgroup in floats
static inline long step_wide_lds_floats(const dcll_conv_desc *d)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const long img = (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w);
    const long vpl = step_wide_pooled(d) ? (long)d->c_out * ch * cw : 0;
    return img + vpl + 32 * SW_MT;
}

// the support predicate of the layers this file serves or forwards: DCLL_OK (c_out <= 32: the answer and the message are
// dcll_conv_lif_step_any's), or the refusal with its message
int dcll_step_wide_check(const dcll_conv_desc *d, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->c_out > SW_MAX_COUT) return fail(DCLL_ERR_UNSUPPORTED, "c_out <= 64 (two 32-row MFMA tiles of output channels)", who);
    if (d->c_out <= 32) return dcll_step_any_check(d, "dcll_conv_lif_step_any");
    if (d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    if (step_wide_lds_floats(d) * 4 > ANY_LDS_MAX)
        return fail(DCLL_ERR_UNSUPPORTED, "the per-sample working set (padded eps1 image, the v plane of a pooling layer) exceeds "
                                          "the 160 KiB of LDS", who);
    return DCLL_OK;
}

extern "C" int64_t dcll_conv_lif_step_wide_lds(const dcll_conv_desc *d)
{
    if (dcll_step_wide_check(d, "dcll_conv_lif_step_wide_lds") != DCLL_OK) return 0;
    return d->c_out <= 32 ? dcll_conv_lif_step_any_lds(d) : step_wide_lds_floats(d) * 4;
}

// floats of w_scratch: 128 per MFMA step of a chain (k_step_wide_wprep's fragment order); 0 = not served
extern "C" int64_t dcll_conv_lif_step_wide_scratch(const dcll_conv_desc *d)
{
    if (dcll_step_wide_check(d, "dcll_conv_lif_step_wide_scratch") != DCLL_OK) return 0;
    return d->c_out <= 32 ? dcll_conv_lif_step_any_scratch(d) : any_chain_steps(d) * 64 * SW_MT;
}

// workgroups per sample, a pure function of (descriptor, B): 1 = the fused form.  units = 2 tiles; ns0 = min(ceil(units / 4),
// 256 / B), then the smallest count with the same units per workgroup (no workgroup without a unit)
int dcll_step_wide_split(const dcll_conv_desc *d, int32_t B)
{
    if (step_wide_pooled(d) || B < 1) return 1;
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const int units = SW_MT * ((ch * cw + 31) / 32);
    int ns = (units + SW_UNITS - 1) / SW_UNITS;
    if (ns > ANY_CUS / B) ns = ANY_CUS / B;
    if (ns <= 1) return 1;
    const int upw = (units + ns - 1) / ns;
    return (units + upw - 1) / upw;
}

// W (c_out, c_in, kh, kw) -> wperm[m][lane][mt]: link 2 m + h of channel co = 32 mt + (lane & 31), h = lane >> 5; 0 beyond
// c_out / the chain
__global__ void k_step_wide_wprep(const float *__restrict__ W, float *__restrict__ wperm, int c_in, int c_out, int kh, int kw,
                                  int npair, int nsteps)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsteps * 64 * SW_MT) return;
    const int m = i >> 7, lane = (i >> 1) & 63, mt = i & 1, co = 32 * mt + (lane & 31), h = lane >> 5, KK = kh * kw;
    int ci, tap;
    any_link(m, h, npair, c_in, KK, ci, tap);
    wperm[i] = (co < c_out && tap < KK) ? W[((long)co * c_in + ci) * KK + tap] : 0.0f;
}

int dcll_launch_step_wide_wprep(const dcll_conv_desc *d, const float *W, float *wperm, hipStream_t st)
{
    const int npair = (int)any_chain_pairs(d), nsteps = (int)any_chain_steps(d);
    hipLaunchKernelGGL(k_step_wide_wprep, dim3((nsteps * 64 * SW_MT + 255) / 256), dim3(256), 0, st, W, wperm, d->c_in, d->c_out,
                       d->kh, d->kw, npair, nsteps);
    HIP_CHECK_LAUNCH("k_step_wide_wprep");
    return DCLL_OK;
}

// the A values of chain step m for this lane: NM == 2 both M tiles in one 8-byte load, NM == 1 tile mt alone
template <int NM>
__device__ __forceinline__ void sw_load_a(const float *__restrict__ wperm, int m, int lane, int mt, float (&a)[NM])
{
    if constexpr (NM == 2) {
        const f32x2u v = *(const f32x2u *)(wperm + (m * 64 + lane) * 2);
        a[0] = v.x;
        a[1] = v.y;
    } else {
        a[0] = wperm[(m * 64 + lane) * 2 + mt];
    }
}

// the whole chain(s) of one pixel tile (k_lif_step_any's loop; NM accumulators fed by one B read per step)
template <int NM>
__device__ __forceinline__ void sw_chains(const step_wide_geom &g, const float *__restrict__ wperm, const float *img, int base0,
                                          int hh, int lane, int mt, f32x16 (&acc)[NM])
{
    const float *bp = img + base0 + hh * g.CHS;
    int m = 0, off = 0, kx = 0, ky = 0;
    for (; m < g.npair; m += 8) {               // (cp, ky, kx): both channels of the pair at one wave-uniform offset
        float a[8][NM];                         // eight steps' A fragments requested before the first is used (L2 latency)
#pragma unroll
        for (int u = 0; u < 8; ++u) sw_load_a<NM>(wperm, m + u < g.npair ? m + u : g.npair - 1, lane, mt, a[u]);
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
                        off += 2 * g.CHS - g.kh * g.WP;
                    }
                }
            }
        }
    }
    m = g.npair;
    if (g.c_in & 1) {                           // the last channel alone: taps (2 q, 2 q + 1), tap KK (odd KK) is the zero link
        const float *cb = img + (g.c_in - 1) * g.CHS + base0;
        const int KK = g.kh * g.kw;
        int tap = hh, tkx = hh, tky = 0;
        while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
        for (; m < g.nsteps; ++m) {
            const float bv = tap < KK ? cb[tky * g.WP + tkx] : 0.0f;
            float a[NM];
            sw_load_a<NM>(wperm, m, lane, mt, a);
#pragma unroll
            for (int t = 0; t < NM; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], bv, acc[t], 0, 0, 0);
            tap += 2;
            tkx += 2;
            while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
        }
    }
}

// what becomes of the accumulators of M tile mt at pixel pix < CP: POOL -> the v plane; else the whole epilogue (conv pixel =
// output pixel): refractory update on arp in HBM, threshold, sigmoid, stores
template <bool R, bool POOL>
__device__ __forceinline__ void sw_epilogue(const step_wide_geom &g, const f32x16 &acc, int mt, int hh, int pix, long b, float *vpl,
                                            float *__restrict__ arp_g, float *__restrict__ out_s, float *__restrict__ out_pv,
                                            float *__restrict__ out_v, float alpharp, float wrp)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (co >= g.c_out) continue;
        if constexpr (POOL) {
            vpl[co * g.CP + pix] = acc[r];
        } else {
            const long o = (b * g.c_out + co) * g.CP + pix;
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

template <bool R, bool POOL, bool SPLIT>
__global__ __launch_bounds__(SW_THREADS) void k_lif_step_wide(const step_wide_geom g, const float *__restrict__ x,
                                                             const float *__restrict__ wperm, const float *__restrict__ bias,
                                                             const float *__restrict__ alpha, const float *__restrict__ tau_m,
                                                             const float *__restrict__ alphas, const float *__restrict__ tau_s,
                                                             float *__restrict__ eps0_g, float *__restrict__ eps1_g,
                                                             float *__restrict__ arp_g, float *__restrict__ out_s,
                                                             float *__restrict__ out_pv, float *__restrict__ out_v, float alpharp,
                                                             float wrp)
{
    static_assert(!(POOL && SPLIT), "the split form serves layers without pooling");
    extern __shared__ float lds[];
    float *img = lds, *vpl = lds + g.o_v, *sb = lds + g.o_bias;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HW = g.h * g.w, NIN = g.c_in * HW, NV = g.c_out * g.CP, NTL = (g.CP + 31) >> 5, NU = SW_MT * NTL;
    const long b = SPLIT ? fdiv((int)blockIdx.x, g.dNS) : (long)blockIdx.x;
    const int part = SPLIT ? (int)blockIdx.x - (int)b * g.ns : 0;
    // units [u0, u1) of this workgroup (fused: all of them), the pixel tiles [tl0, tl1) they lie in
    const int u0 = SPLIT ? part * g.upw : 0, u1 = SPLIT ? (u0 + g.upw < NU ? u0 + g.upw : NU) : NU;
    const int tl0 = u0 >> 1, tl1 = (u1 + 1) >> 1;

    // ---- the padded image: padding zeroed, interior = eps1 of this step
    {
        // (split form: only the padded rows the workgroup's tiles read, [first conv row, last conv row + kh - 1])
        const int pl = (tl1 * 32 < g.CP ? tl1 * 32 : g.CP) - 1;
        const int yp0 = SPLIT ? fdiv(tl0 * 32, g.dCW) : 0, yp1 = SPLIT ? fdiv(pl, g.dCW) + g.kh - 1 : g.h + 2 * g.pad_h - 1;
        const float *xb = x + b * NIN;
        float *e0b = eps0_g + b * NIN, *e1b = eps1_g + b * NIN;
        for (int q = tid; q < g.c_in * g.CHS; q += SW_THREADS) {
            const int ci = fdiv(q, g.dCHS), rem = q - ci * g.CHS, yp = fdiv(rem, g.dWP), xp = rem - yp * g.WP;
            const int y = yp - g.pad_h, xx = xp - g.pad_w;
            if (SPLIT && (yp < yp0 || yp > yp1)) continue;
            float e1 = 0.0f;
            if (y >= 0 && y < g.h && xx >= 0 && xx < g.w) {
                const int i = ci * HW + y * g.w + xx;
                if constexpr (SPLIT) {
                    e1 = e1b[i];
                } else {
                    const int t = g.tau_is_tensor ? i : 0;
                    float e0 = e0b[i];
                    e1 = e1b[i];
                    trace_update(xb[i], alpha[t], tau_m[t], alphas[t], tau_s[t], e0, e1);
                    e0b[i] = e0;
                    e1b[i] = e1;
                }
            }
            img[q] = e1;
        }
        if (tid < 32 * SW_MT) sb[tid] = (bias && tid < g.c_out) ? bias[tid] : 0.0f;
    }
    __syncthreads();

    // the lane's pixel of tile tl (a ragged lane reads the last pixel's window) and its offset in a channel of img
    auto pixel = [&](int tl, int &pix) -> int {
        pix = tl * 32 + j;
        const int pc = pix < g.CP ? pix : g.CP - 1;
        const int y = fdiv(pc, g.dCW), xq = pc - y * g.cw;
        return y * g.WP + xq;
    };

    if constexpr (SPLIT) {
        // ---- one chain per unit: wave wv runs units u0 + wv, u0 + wv + 8, ...
        for (int u = u0 + wv; u < u1; u += SW_NW) {
            const int tl = u >> 1, mt = u & 1;
            int pix;
            const int base0 = pixel(tl, pix);
            f32x16 acc[1];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][r] = sb[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh];
            sw_chains<1>(g, wperm, img, base0, hh, lane, mt, acc);
            if (pix < g.CP) sw_epilogue<R, false>(g, acc[0], mt, hh, pix, b, vpl, arp_g, out_s, out_pv, out_v, alpharp, wrp);
        }
    } else {
        // ---- both chains of a pixel tile, interleaved: wave wv runs pixel tiles wv, wv + 8, ...
        for (int tl = wv; tl < NTL; tl += SW_NW) {
            int pix;
            const int base0 = pixel(tl, pix);
            f32x16 acc[SW_MT];
#pragma unroll
            for (int mt = 0; mt < SW_MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][r] = sb[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh];
            sw_chains<SW_MT>(g, wperm, img, base0, hh, lane, 0, acc);
            if (pix < g.CP) {
#pragma unroll
                for (int mt = 0; mt < SW_MT; ++mt)
                    sw_epilogue<R, POOL>(g, acc[mt], mt, hh, pix, b, vpl, arp_g, out_s, out_pv, out_v, alpharp, wrp);
            }
        }
    }
    if constexpr (POOL) {
        __syncthreads();
        // ---- refractory update on the v plane (arp in HBM), out_v
        if (R || out_v) {
            for (int i = tid; i < NV; i += SW_THREADS) {
                float v = vpl[i];
                if (R) {
                    float ar = arp_g[b * NV + i];
                    bool s;
                    v = refractory(v, ar, alpharp, wrp, s);
                    arp_g[b * NV + i] = ar;
                    vpl[i] = v;
                }
                if (out_v) out_v[b * NV + i] = v;
            }
            __syncthreads();
        }
        // ---- the pooling pass: MaxPool2d(kernel = stride = pool, padding (pool - 1) / 2) over v
        const int pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2, NP = g.c_out * g.PP;
        for (int i = tid; i < NP; i += SW_THREADS) {
            const int co = fdiv(i, g.dPP), pp = i - co * g.PP, py = fdiv(pp, g.dPW), px = pp - py * g.pw;
            const float *vc = vpl + co * g.CP;
            float mx = -INFINITY;
            for (int dy = 0; dy < g.pool_h; ++dy) {
                const int yy = py * g.pool_h - pph + dy;
                if (yy < 0 || yy >= g.ch) continue;
                for (int dx = 0; dx < g.pool_w; ++dx) {
                    const int xx = px * g.pool_w - ppw + dx;
                    if (xx < 0 || xx >= g.cw) continue;
                    mx = fmaxf(mx, vc[yy * g.cw + xx]);
                }
            }
            out_s[b * NP + i] = mx > 0.0f ? 1.0f : 0.0f;
            out_pv[b * NP + i] = sigmoidf_dev(mx);
        }
    }
}

template <bool R, bool POOL, bool SPLIT>
static int launch_step_wide(const step_wide_geom &g, size_t lds_bytes, const float *x, const float *wperm, const float *b,
                            const float *alpha, const float *tau_m, const float *alphas, const float *tau_s, float *eps0,
                            float *eps1, float *arp, float *out_s, float *out_pv, float *out_v, int B, float alpharp, float wrp,
                            hipStream_t st, const char *name, bool launch)
{
    // dynamic LDS above 64 KiB is reserved per template instance AND device (the attribute belongs to the device's code object);
    // asked for again only when a call needs more than any before it on this device — a timestep under graph capture repeats
    // the geometry of the eager steps before it, so no attribute call falls inside a capture
    static std::mutex mu;
    static size_t reserved[SW_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_step_wide: no current device");
    }
    if (lds_bytes > 64 * 1024) {
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= SW_MAX_DEVICES || lds_bytes > reserved[dev]) {       // (a device beyond the table: asked for on every call)
            if (hipFuncSetAttribute((const void *)k_lif_step_wide<R, POOL, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(DCLL_ERR_LAUNCH, "k_lif_step_wide: cannot reserve its LDS");
            }
            if (dev < SW_MAX_DEVICES) reserved[dev] = lds_bytes;
        }
    }
    if (!launch) return DCLL_OK;
    hipLaunchKernelGGL((k_lif_step_wide<R, POOL, SPLIT>), dim3((unsigned)((long)B * g.ns)), dim3(SW_THREADS), lds_bytes, st, g, x,
                       wperm, b, alpha, tau_m, alphas, tau_s, eps0, eps1, arp, out_s, out_pv, out_v, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

// the layer kernel of a checked call with c_out > 32 (dcll_step_wide_check; ns = dcll_step_wide_split(d, B): with ns > 1 the
// caller has run k_trace).  launch == false: everything that can fail short of the launch itself — the geometry, the layout and
// split checks, the LDS reservation — and nothing else; the entry point calls this form first, so an error return never follows
// a launch
int dcll_launch_step_wide(const dcll_conv_desc *d, const float *x, const float *wperm, const float *b, const float *alpha,
                          const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                          float *out_s, float *out_pv, float *out_v, int ns, int32_t B, hipStream_t st, bool launch)
{
    const char *who = "dcll_conv_lif_step_wide";
    const bool pooled = step_wide_pooled(d);
    step_wide_geom g;
    g.c_in = d->c_in; g.c_out = d->c_out; g.h = d->h; g.w = d->w; g.kh = d->kh; g.kw = d->kw;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.pool_h = d->pool_h; g.pool_w = d->pool_w;
    g.WP = d->w + 2 * d->pad_w;
    g.CHS = (d->h + 2 * d->pad_h) * g.WP;
    conv_shape(d, &g.ch, &g.cw, &g.ph, &g.pw);
    g.CP = g.ch * g.cw;
    g.PP = g.ph * g.pw;
    g.npair = (int)any_chain_pairs(d);
    g.nsteps = (int)any_chain_steps(d);
    const int units = SW_MT * ((g.CP + 31) / 32);
    g.ns = ns;
    g.upw = ns >= 1 ? (units + ns - 1) / ns : units;
    g.o_v = d->c_in * g.CHS;
    g.o_bias = g.o_v + (pooled ? d->c_out * g.CP : 0);
    g.tau_is_tensor = d->tau_is_tensor;
    g.dCHS = make_div(g.CHS); g.dWP = make_div(g.WP); g.dCW = make_div(g.cw); g.dPP = make_div(g.PP); g.dPW = make_div(g.pw);
    g.dNS = make_div(ns >= 1 ? ns : 1);
    if (d->c_out <= 32 || d->c_out > SW_MAX_COUT)
        return fail(DCLL_ERR_LAUNCH, "k_lif_step_wide serves 33 .. 64 output channels", who);
    if (g.o_bias + 32 * SW_MT != step_wide_lds_floats(d))       // the layout above against the ONE exported formula
        return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_step_wide_lds disagree", who);
    if (ns < 1 || (ns > 1 && pooled) || (long)g.upw * (ns - 1) >= units || (long)B * ns > 0x7fffffffL / 2)
        return fail(DCLL_ERR_LAUNCH, "bad split of the (pixel tile, M tile) units", who);
    const size_t lds_bytes = (size_t)(g.o_bias + 32 * SW_MT) * 4;
#define DCLL_SW(R_, P_, S_, name_)                                                                                            \
    return launch_step_wide<R_, P_, S_>(g, lds_bytes, x, wperm, b, alpha, tau_m, alphas, tau_s, eps0, eps1, arp, out_s, out_pv, \
                                        out_v, B, d->alpharp, d->wrp, st, name_, launch)
    if (d->refractory) {
        if (pooled) DCLL_SW(1, 1, 0, "k_lif_step_wide<1> (pooling)");
        if (ns > 1) DCLL_SW(1, 0, 1, "k_lif_step_wide<1> (split)");
        DCLL_SW(1, 0, 0, "k_lif_step_wide<1>");
    }
    if (pooled) DCLL_SW(0, 1, 0, "k_lif_step_wide<0> (pooling)");
    if (ns > 1) DCLL_SW(0, 0, 1, "k_lif_step_wide<0> (split)");
    DCLL_SW(0, 0, 0, "k_lif_step_wide<0>");
#undef DCLL_SW
}
