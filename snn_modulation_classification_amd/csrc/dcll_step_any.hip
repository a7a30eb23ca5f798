// dcll_step_any.hip — k_lif_step_any: ONE timestep of ANY plain conv layer (stride = dilation = groups = 1, c_out <= 32, kernel
// up to 16x16, any c_in, padding, pooling and batch) in one launch (dcll_conv_lif_step_any, ABI 10) — the opt-in MFMA form of
// the layers dcll_conv_lif_step serves with k_trace + k_conv_lif[_tiled] + k_pool.  The per-step sibling of k_lif_seq_any
// (dcll_seq_any.hip), with the state in HBM.
//
// LDS of a workgroup (floats; step_any_lds_floats() is the ONE statement of it, exported as dcll_conv_lif_step_any_lds):
//   img   c_in x (h + 2 pad_h) x (w + 2 pad_w)   eps1 of this step, zero padded: the B operand of every chain link is one read
//         at ci CHS + (y + ky) WP + x + kx
//   vpl   c_out x ch x cw                        pooling layers only: v at conv resolution (the pooling pass reads windows of it)
//   bias  32
// The weights are not staged: every MFMA's A fragment is one coalesced 256-byte read of w_scratch (k_seq_any_wprep's fragment
// order, written in front of this kernel on every call), eight in flight per wave.
//
// Arithmetic = the contract of include/dcll_hip.h and exactly k_lif_seq_any's rule: the chain of output (co, y, x) starts at
// bias[co] and runs over the links (cp, ky, kx, h), ci = 2 cp + h, one v_mfma_f32_32x32x2_f32 per two CONSECUTIVE links; the last
// channel of an odd c_in pairs its taps two by two, and a link beyond the last carries a zero weight and a zero input.
// M = c_out padded to 32 rows, N = 32 pixels of the flattened conv plane; a wave owns whole tiles and runs a tile's whole chain.
//
// Fused form (one workgroup per sample): one pass over the padded image — a padding position is zeroed, an interior position
// reads x, eps0, eps1 of its element, advances them (trace_update), writes both back and keeps eps1' —, a barrier, the chains,
// and the epilogue: without pooling straight from the accumulators (refractory update on arp in HBM, threshold, sigmoid,
// stores); with pooling v goes to vpl, the refractory update and out_v run there, and behind a barrier the pooling pass takes
// max over the window of v, spike = pooled v > 0, pv = sigmoid(pooled v).
// Split form (NS > 1 workgroups per sample; layers without pooling, when the batch leaves CUs idle and a sample has more
// pixel tiles than a workgroup has waves): workgroup `part` runs tiles [part TPB, (part + 1) TPB).  Here the traces are NOT
// advanced in the kernel — a workgroup would read halo rows of eps1 that a sibling of the same sample is overwriting in
// place (the read-after-write race once found in k_lif_seq_w3f) — the launcher runs k_trace first and the kernel stages the
// rows of eps1 its tiles touch read-only.  Every chain is still whole, so the results do not depend on NS.
#include "dcll_any_shared.h"
#include <mutex>

constexpr int SA_THREADS = 512, SA_NW = SA_THREADS / 64;
constexpr long SA_LDS_MAX = 160 * 1024;
constexpr int SA_MAX_K = 16, SA_MAX_COUT = 32;
constexpr int SA_MAX_DEVICES = 64;
constexpr int SA_CUS = 256;                     // the chip's CUs (the constant of the other launchers' batch rules)

struct step_any_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int WP, CHS;                // padded row length, padded channel stride of img
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int ns, tpb;                // workgroups per sample, pixel tiles per workgroup
    int o_v, o_bias;            // float offsets into LDS (img at 0)
    int tau_is_tensor;
    any_div dCHS, dWP, dCW, dPP, dPW, dNS;
};

static inline bool step_any_pooled(const dcll_conv_desc *d) { return !(d->pool_h == 1 && d->pool_w == 1); }

// the working set of a workgroup in floats
static inline long step_any_lds_floats(const dcll_conv_desc *d)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const long img = (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w);
    const long vpl = step_any_pooled(d) ? (long)d->c_out * ch * cw : 0;
    return img + vpl + 32;
}

// the support predicate: DCLL_OK, or the refusal with its message
int dcll_step_any_check(const dcll_conv_desc *d, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!plain_conv(d)) return fail(DCLL_ERR_UNSUPPORTED, "plain convolutions only: stride, dilation and groups must be 1", who);
    if (d->c_out > SA_MAX_COUT) return fail(DCLL_ERR_UNSUPPORTED, "c_out <= 32 (one 32-row MFMA tile of output channels)", who);
    if (d->kh > SA_MAX_K || d->kw > SA_MAX_K) return fail(DCLL_ERR_UNSUPPORTED, "kernels up to 16x16", who);
    if (step_any_lds_floats(d) * 4 > SA_LDS_MAX)
        return fail(DCLL_ERR_UNSUPPORTED, "the per-sample working set (padded eps1 image, the v plane of a pooling layer) exceeds "
                                          "the 160 KiB of LDS", who);
    return DCLL_OK;
}

extern "C" int64_t dcll_conv_lif_step_any_lds(const dcll_conv_desc *d)
{
    return dcll_step_any_check(d, "dcll_conv_lif_step_any_lds") == DCLL_OK ? step_any_lds_floats(d) * 4 : 0;
}

// floats of w_scratch: 64 per MFMA step of a chain (k_seq_any_wprep's fragment order); 0 = not served
extern "C" int64_t dcll_conv_lif_step_any_scratch(const dcll_conv_desc *d)
{
    return dcll_step_any_check(d, "dcll_conv_lif_step_any_scratch") == DCLL_OK ? any_chain_steps(d) * 64 : 0;
}

// workgroups per sample, a pure function of (descriptor, B): 1 = the fused form.  min(ceil(tiles / waves), 256 / B), then the
// smallest count with the same tiles per workgroup (no workgroup without a tile)
int dcll_step_any_split(const dcll_conv_desc *d, int32_t B)
{
    if (step_any_pooled(d) || B < 1) return 1;
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const int ntl = (ch * cw + 31) / 32;
    int ns = (ntl + SA_NW - 1) / SA_NW;
    if (ns > SA_CUS / B) ns = SA_CUS / B;
    if (ns <= 1) return 1;
    const int tpb = (ntl + ns - 1) / ns;
    return (ntl + tpb - 1) / tpb;
}

template <bool R, bool POOL, bool SPLIT>
__global__ __launch_bounds__(SA_THREADS) void k_lif_step_any(const step_any_geom g, const float *__restrict__ x,
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
    const int HW = g.h * g.w, NIN = g.c_in * HW, NV = g.c_out * g.CP, NTL = (g.CP + 31) >> 5;
    const long b = SPLIT ? fdiv((int)blockIdx.x, g.dNS) : (long)blockIdx.x;
    const int part = SPLIT ? (int)blockIdx.x - (int)b * g.ns : 0;
    const int tl0 = part * g.tpb, tl1 = (tl0 + g.tpb < NTL) ? tl0 + g.tpb : NTL;

    // ---- the padded image: padding zeroed, interior = eps1 of this step
    {
        // (split form: only the padded rows the workgroup's tiles read, [first conv row, last conv row + kh - 1])
        const int pl = (tl1 * 32 < g.CP ? tl1 * 32 : g.CP) - 1;
        const int yp0 = SPLIT ? fdiv(tl0 * 32, g.dCW) : 0, yp1 = SPLIT ? fdiv(pl, g.dCW) + g.kh - 1 : g.h + 2 * g.pad_h - 1;
        const float *xb = x + b * NIN;
        float *e0b = eps0_g + b * NIN, *e1b = eps1_g + b * NIN;
        for (int q = tid; q < g.c_in * g.CHS; q += SA_THREADS) {
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
        if (tid < 32) sb[tid] = (bias && tid < g.c_out) ? bias[tid] : 0.0f;
    }
    __syncthreads();

    // ---- the chains: wave wv runs pixel tiles tl0 + wv, tl0 + wv + 8, ...
    for (int tl = tl0 + wv; tl < tl1; tl += SA_NW) {
        const int pix = tl * 32 + j, pc = pix < g.CP ? pix : g.CP - 1;      // (a ragged lane reads the last pixel's window)
        const int y = fdiv(pc, g.dCW), xq = pc - y * g.cw, base0 = y * g.WP + xq;
        const float *bp = img + base0 + hh * g.CHS;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = sb[(r & 3) + 8 * (r >> 2) + 4 * hh];
        int m = 0, off = 0, kx = 0, ky = 0;
        for (; m < g.npair; m += 8) {           // (cp, ky, kx): both channels of the pair at one wave-uniform offset
            float a[8];                         // eight A fragments requested before the first is used (L2 latency)
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = wperm[(m + u < g.npair ? m + u : g.npair - 1) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (m + u < g.npair) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bp[off], acc, 0, 0, 0);
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
        if (g.c_in & 1) {                       // the last channel alone: taps (2 q, 2 q + 1), tap KK (odd KK) is the zero link
            const float *cb = img + (g.c_in - 1) * g.CHS + base0;
            const int KK = g.kh * g.kw;
            int tap = hh, tkx = hh, tky = 0;
            while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            for (; m < g.nsteps; ++m) {
                const float bv = tap < KK ? cb[tky * g.WP + tkx] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wperm[m * 64 + lane], bv, acc, 0, 0, 0);
                tap += 2;
                tkx += 2;
                while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            }
        }
        if (pix < g.CP) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (co >= g.c_out) continue;
                if constexpr (POOL) {
                    vpl[co * g.CP + pix] = acc[r];
                } else {                        // no pooling: conv pixel = output pixel, the whole epilogue from the accumulators
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
    }
    if constexpr (POOL) {
        __syncthreads();
        // ---- refractory update on the v plane (arp in HBM), out_v
        if (R || out_v) {
            for (int i = tid; i < NV; i += SA_THREADS) {
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
        for (int i = tid; i < NP; i += SA_THREADS) {
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
static int launch_step_any(const step_any_geom &g, size_t lds_bytes, const float *x, const float *wperm, const float *b,
                           const float *alpha, const float *tau_m, const float *alphas, const float *tau_s, float *eps0,
                           float *eps1, float *arp, float *out_s, float *out_pv, float *out_v, int B, float alpharp, float wrp,
                           hipStream_t st, const char *name, bool launch)
{
    // dynamic LDS above 64 KiB is reserved per template instance AND device (the attribute belongs to the device's code object);
    // asked for again only when a call needs more than any before it on this device — a timestep under graph capture repeats
    // the geometry of the eager steps before it, so no attribute call falls inside a capture
    static std::mutex mu;
    static size_t reserved[SA_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_step_any: no current device");
    }
    if (lds_bytes > 64 * 1024) {
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= SA_MAX_DEVICES || lds_bytes > reserved[dev]) {       // (a device beyond the table: asked for on every call)
            if (hipFuncSetAttribute((const void *)k_lif_step_any<R, POOL, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(DCLL_ERR_LAUNCH, "k_lif_step_any: cannot reserve its LDS");
            }
            if (dev < SA_MAX_DEVICES) reserved[dev] = lds_bytes;
        }
    }
    if (!launch) return DCLL_OK;
    hipLaunchKernelGGL((k_lif_step_any<R, POOL, SPLIT>), dim3((unsigned)((long)B * g.ns)), dim3(SA_THREADS), lds_bytes, st, g, x,
                       wperm, b, alpha, tau_m, alphas, tau_s, eps0, eps1, arp, out_s, out_pv, out_v, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

// the layer kernel of a checked call (dcll_step_any_check; ns = dcll_step_any_split(d, B): with ns > 1 the caller has run k_trace).
// launch == false: everything that can fail short of the launch itself — the geometry, the layout and split checks, the LDS
// reservation — and nothing else; the entry point calls this form first, so an error return never follows a launch
int dcll_launch_step_any(const dcll_conv_desc *d, const float *x, const float *wperm, const float *b, const float *alpha,
                         const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                         float *out_s, float *out_pv, float *out_v, int ns, int32_t B, hipStream_t st, bool launch)
{
    const char *who = "dcll_conv_lif_step_any";
    const bool pooled = step_any_pooled(d);
    step_any_geom g;
    g.c_in = d->c_in; g.c_out = d->c_out; g.h = d->h; g.w = d->w; g.kh = d->kh; g.kw = d->kw;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.pool_h = d->pool_h; g.pool_w = d->pool_w;
    g.WP = d->w + 2 * d->pad_w;
    g.CHS = (d->h + 2 * d->pad_h) * g.WP;
    conv_shape(d, &g.ch, &g.cw, &g.ph, &g.pw);
    g.CP = g.ch * g.cw;
    g.PP = g.ph * g.pw;
    g.npair = (int)any_chain_pairs(d);
    g.nsteps = (int)any_chain_steps(d);
    const int ntl = (g.CP + 31) / 32;
    g.ns = ns;
    g.tpb = (ntl + ns - 1) / ns;
    g.o_v = d->c_in * g.CHS;
    g.o_bias = g.o_v + (pooled ? d->c_out * g.CP : 0);
    g.tau_is_tensor = d->tau_is_tensor;
    g.dCHS = make_div(g.CHS); g.dWP = make_div(g.WP); g.dCW = make_div(g.cw); g.dPP = make_div(g.PP); g.dPW = make_div(g.pw);
    g.dNS = make_div(ns);
    if (g.o_bias + 32 != step_any_lds_floats(d))        // the layout above against the ONE exported formula
        return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_step_any_lds disagree", who);
    if (ns < 1 || (ns > 1 && pooled) || (long)g.tpb * (ns - 1) >= ntl || (long)B * ns > 0x7fffffffL / 2)
        return fail(DCLL_ERR_LAUNCH, "bad split of the pixel tiles", who);
    const size_t lds_bytes = (size_t)(g.o_bias + 32) * 4;
#define DCLL_SA(R_, P_, S_, name_)                                                                                            \
    return launch_step_any<R_, P_, S_>(g, lds_bytes, x, wperm, b, alpha, tau_m, alphas, tau_s, eps0, eps1, arp, out_s, out_pv,  \
                                       out_v, B, d->alpharp, d->wrp, st, name_, launch)
    if (d->refractory) {
        if (pooled) DCLL_SA(1, 1, 0, "k_lif_step_any<1> (pooling)");
        if (ns > 1) DCLL_SA(1, 0, 1, "k_lif_step_any<1> (split)");
        DCLL_SA(1, 0, 0, "k_lif_step_any<1>");
    }
    if (pooled) DCLL_SA(0, 1, 0, "k_lif_step_any<0> (pooling)");
    if (ns > 1) DCLL_SA(0, 0, 1, "k_lif_step_any<0> (split)");
    DCLL_SA(0, 0, 0, "k_lif_step_any<0>");
#undef DCLL_SA
}
