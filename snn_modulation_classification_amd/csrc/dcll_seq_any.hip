// dcll_seq_any.hip — k_lif_seq_any: all T timesteps of ANY plain conv layer (stride = dilation = groups = 1, c_out <= 32,
// kernel up to 16x16, any padding, any pooling) in one launch, one workgroup per sample, the neuron state on chip
// (dcll_conv_lif_sequence_any, ABI 8) — the fused path of the layers none of the specialised sequence kernels serve
// (networks/mnist_conv.yaml; radio_ml_conv.yaml on planes other than 16x16 / h % 8, w % 32).
//
// LDS of a workgroup (floats; any_lds_floats() is the ONE statement of it, exported as dcll_conv_lif_sequence_any_lds):
//   img   c_in x (h + 2 pad_h) x (w + 2 pad_w)   eps1, zero padded: the B operand of every chain link is one read
//   e0    c_in x h x w                           eps0
//   vpl   c_out x ch x cw                        v of ONE step at conv resolution (the pooling pass reads windows of it)
//   arp   c_out x ch x cw                        refractory layers only
//   tau   4 x c_in, bias 32
//   + the permuted weights behind these: all of them when they fit (WLDS), else as many chain steps as fit — the rest is
//     streamed from L2, eight fragments in flight per wave.
// A layer WITHOUT pooling whose set is larger than that (radio_ml_conv.yaml's 32 -> 32 layers on 24x24 or 12x32: eps0, eps1,
// v and arp are 72 KiB EACH there) runs the register form (REGS) when c_in h w <= 18432 and ch cw <= 768: only img (+ tau, bias)
// in LDS, eps0 in the registers of the thread that advances the element (<= 36 per thread), arp in the accumulator layout of
// the wave that owns the tile (<= 3 tiles x 16), and the epilogue — refractory update, threshold, sigmoid, ballot-packed spike
// words — straight from the accumulators: no v plane, no pooling pass, two barriers per step; weights streamed.
//
// Arithmetic = the contract of include/dcll_hip.h: the chain of output (co, y, x) starts at bias[co] and runs over the links
// (cp, ky, kx, h), ci = 2 cp + h, one v_mfma_f32_32x32x2_f32 per two CONSECUTIVE links (its two k lanes: bit for bit
// acc = fmaf(a1, b1, fmaf(a0, b0, acc))).  An even c_in pairs the two channels of a tap; the last channel of an odd c_in has
// no partner, so its taps are paired two by two in tap order (the rule of k_lif_seq_c1), and a link beyond the last one carries
// a ZERO weight and a zero input: fmaf(0, 0, acc) == acc (for acc == -0.0 it yields +0.0: DESIGN §2's caveat).
// M = c_out padded to 32 rows (zero weights), N = 32 pixels of the flattened conv plane; a wave owns whole tiles and runs a
// tile's whole chain itself.  Weights are permuted once per call into A-fragment order (k_seq_any_wprep):
// wperm[m][lane] = weight of link 2 m + (lane >> 5) for output channel lane & 31.
//
// One step = three phases, a barrier behind each:
//   A  traces of step t advanced in place (eps0, the interior of img) + the pooling pass of step t - 1 (reads vpl only):
//      pooled v = max over the window, spike = pooled v > 0, pv = sigmoid(pooled v), spike words by ballot
//   B  the chains: wave w computes pixel tiles w, w + 8, ... -> vpl
//   C  refractory update on vpl (arp in LDS), v_out
// State (eps0, eps1, arp) is read once before the first step and written once behind the last.
#include "dcll_any_shared.h"

constexpr int ANY_THREADS = 512, ANY_NW = ANY_THREADS / 64;
constexpr int ANY_MAX_COUT = 32;
constexpr int ANY_KE = 36, ANY_QMAX = 3;        // register form: eps0 values per thread, pixel tiles per wave

struct any_geom {
    int c_in, c_out, h, w, kh, kw, pad_h, pad_w, pool_h, pool_w;
    int WP, CHS;                // padded row length, padded channel stride of img
    int ch, cw, CP, ph, pw, PP; // conv / pooled plane
    int npair, nsteps;          // MFMA steps of the channel-pair part, of the whole chain
    int nwl;                    // chain steps whose weights are kept in LDS (WLDS: all of them)
    int iw, ow;                 // words per input / output spike plane
    int o_e0, o_v, o_arp, o_tau, o_bias, o_w;   // float offsets into LDS (img at 0)
    any_div dHW, dW, dCW, dOW, dPW;
};

// the working set of a workgroup in floats, without the weights (refractory: + the arp plane)
static inline long any_lds_floats(const dcll_conv_desc *d)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const long img = (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w);
    const long e0 = (long)d->c_in * d->h * d->w;
    const long vpl = (long)d->c_out * ch * cw;
    return img + e0 + vpl * (d->refractory ? 2 : 1) + 4L * d->c_in + 32;
}

// the register form's set: img + tau + bias; for layers without pooling within its per-thread / per-wave register arrays
static inline long any_lds_floats_regs(const dcll_conv_desc *d)
{
    return (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w) + 4L * d->c_in + 32;
}
static inline bool any_regs_ok(const dcll_conv_desc *d)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    return d->pool_h == 1 && d->pool_w == 1 && (long)d->c_in * d->h * d->w <= (long)ANY_KE * ANY_THREADS &&
           (long)ch * cw <= 32L * ANY_NW * ANY_QMAX && any_lds_floats_regs(d) * 4 <= ANY_LDS_MAX;
}

// the support predicate: DCLL_OK (*regs: the register form serves the layer), or the refusal with its message
static int any_supported(const dcll_conv_desc *d, const char *who, bool *regs = nullptr)
{
    int rc = any_layer_ok(d, ANY_MAX_COUT, who);
    if (rc) return rc;
    const bool full = any_lds_floats(d) * 4 <= ANY_LDS_MAX;
    if (!full && !any_regs_ok(d))
        return fail(DCLL_ERR_UNSUPPORTED, "the per-sample working set (padded eps1 image, eps0, the v plane) exceeds the 160 KiB of LDS "
                                          "and the layer is outside the register form (no pooling, c_in h w <= 18432, ch cw <= 768)", who);
    if (regs) *regs = !full;
    return DCLL_OK;
}

extern "C" int64_t dcll_conv_lif_sequence_any_lds(const dcll_conv_desc *d)
{
    bool regs = false;
    if (any_supported(d, "dcll_conv_lif_sequence_any_lds", &regs) != DCLL_OK) return 0;
    return (regs ? any_lds_floats_regs(d) : any_lds_floats(d)) * 4;
}
extern "C" int64_t dcll_conv_lif_sequence_any_scratch(const dcll_conv_desc *d)
{
    return any_supported(d, "dcll_conv_lif_sequence_any_scratch") == DCLL_OK ? any_chain_steps(d) * 64 : 0;
}

// W (c_out, c_in, kh, kw) -> wperm[m][mt][lane]: link 2 m + h of channel co = 32 mt + (lane & 31), h = lane >> 5; 0 beyond
// c_out / the chain.  MT = 1: wperm[m][lane]
__global__ void k_seq_any_wprep(const float *__restrict__ W, float *__restrict__ wperm, int c_in, int c_out, int kh, int kw,
                                int npair, int nsteps, int MT)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsteps * 64 * MT) return;
    const int lane = i & 63, u = i >> 6, mt = u % MT, m = u / MT, co = 32 * mt + (lane & 31), h = lane >> 5, KK = kh * kw;
    int ci, tap;
    any_link(m, h, npair, c_in, KK, ci, tap);
    wperm[i] = (co < c_out && tap < KK) ? W[((long)co * c_in + ci) * KK + tap] : 0.0f;
}

int dcll_launch_seq_wprep(const dcll_conv_desc *d, const float *W, float *wperm, int MT, hipStream_t st, bool note,
                          const char *errname)
{
    const int npair = (int)any_chain_pairs(d), nsteps = (int)any_chain_steps(d);
    hipLaunchKernelGGL(k_seq_any_wprep, dim3((nsteps * 64 * MT + 255) / 256), dim3(256), 0, st, W, wperm, d->c_in, d->c_out, d->kh,
                       d->kw, npair, nsteps, MT);
    if (note) dcll_trace_note("k_seq_any_wprep");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DCLL_OK : fail(DCLL_ERR_LAUNCH, hipGetErrorString(e), errname);
}

template <bool R, bool WLDS, bool REGS>
__global__ __launch_bounds__(ANY_THREADS) void k_lif_seq_any(const any_geom g, const uint32_t *__restrict__ spk_in,
                                                            const float *__restrict__ wperm, const float *__restrict__ bias,
                                                            const float *__restrict__ tau4, float *__restrict__ eps0_g,
                                                            float *__restrict__ eps1_g, float *__restrict__ arp_g,
                                                            uint32_t *__restrict__ spk_out, float *__restrict__ pv_out,
                                                            float *__restrict__ v_out, int T, int B, float alpharp, float wrp)
{
    static_assert(!(REGS && WLDS), "the register form streams its weights");
    extern __shared__ float lds[];
    float *img = lds, *e0s = lds + g.o_e0, *vpl = lds + g.o_v, *arps = lds + g.o_arp, *taus = lds + g.o_tau,
          *sb = lds + g.o_bias, *wl = lds + g.o_w;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long b = blockIdx.x;
    const int HW = g.h * g.w, NIN = g.c_in * HW, NV = g.c_out * g.CP, NTL = (g.CP + 31) >> 5;
    float e0r[REGS ? ANY_KE : 1], arpr[REGS ? ANY_QMAX : 1][16];      // register form: eps0 of elements tid + 512 k; arp of tiles wv + 8 q

    // position of input element i (channel ci, pixel p) in img
    auto img_at = [&](int i, int &ci, int &p) -> int {
        ci = fdiv(i, g.dHW);
        p = i - ci * HW;
        const int y = fdiv(p, g.dW), x = p - y * g.w;
        return ci * g.CHS + (y + g.pad_h) * g.WP + x + g.pad_w;
    };

    // ---- prologue: state and constants on chip
    for (int i = tid; i < g.c_in * g.CHS; i += ANY_THREADS) img[i] = 0.0f;
    __syncthreads();
    if constexpr (REGS) {
#pragma unroll
        for (int k = 0; k < ANY_KE; ++k) {
            const int i = tid + k * ANY_THREADS;
            e0r[k] = 0.0f;
            if (i < NIN) {
                int ci, p;
                const int q = img_at(i, ci, p);
                e0r[k] = eps0_g[b * NIN + i];
                img[q] = eps1_g[b * NIN + i];
            }
        }
#pragma unroll
        for (int q = 0; q < ANY_QMAX; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (r & 3) + 8 * (r >> 2) + 4 * hh, pix = (wv + ANY_NW * q) * 32 + j;
                arpr[q][r] = (R && co < g.c_out && pix < g.CP) ? arp_g[b * NV + co * g.CP + pix] : 0.0f;
            }
    } else {
        for (int i = tid; i < NIN; i += ANY_THREADS) {
            int ci, p;
            const int q = img_at(i, ci, p);
            e0s[i] = eps0_g[b * NIN + i];
            img[q] = eps1_g[b * NIN + i];
        }
        if (R)
            for (int i = tid; i < NV; i += ANY_THREADS) arps[i] = arp_g[b * NV + i];
    }
    for (int i = tid; i < 4 * g.c_in; i += ANY_THREADS) taus[i] = tau4[i];
    if (tid < 32) sb[tid] = (bias && tid < g.c_out) ? bias[tid] : 0.0f;
    for (int i = tid; i < (WLDS ? g.nsteps : g.nwl) * 64; i += ANY_THREADS) wl[i] = wperm[i];
    __syncthreads();

    // the trace update of input element i at step t (e0: its eps0; eps1 in place in img)
    auto trace = [&](const uint32_t *sp, int i, float &e0) {
        int ci, p;
        const int q = img_at(i, ci, p);
        const float xin = (float)((sp[ci * g.iw + (p >> 5)] >> (p & 31)) & 1u);
        float e1 = img[q];
        trace_update(xin, taus[ci], taus[g.c_in + ci], taus[2 * g.c_in + ci], taus[3 * g.c_in + ci], e0, e1);
        img[q] = e1;
    };

    // the chain of pixel tile tl: 32 conv pixels x 32 channel rows
    auto chain = [&](int tl) -> f32x16 {
        const int pix = tl * 32 + j, pc = pix < g.CP ? pix : g.CP - 1, y = fdiv(pc, g.dCW), x = pc - y * g.cw;
        const int base0 = y * g.WP + x;
        const float *bp = img + base0 + hh * g.CHS;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = sb[(r & 3) + 8 * (r >> 2) + 4 * hh];
        auto wa = [&](int m) -> float {
            if constexpr (WLDS) return wl[m * 64 + lane];
            else return m < g.nwl ? wl[m * 64 + lane] : wperm[m * 64 + lane];
        };
        int m = 0, off = 0, kx = 0, ky = 0;
        for (; m < g.npair; m += 8) {       // (cp, ky, kx): both channels of the pair at one wave-uniform offset
            float a[8];                     // eight A fragments requested before the first is used (the streamed ones: L2 latency)
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = wa(m + u < g.npair ? m + u : g.npair - 1);
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
        if (g.c_in & 1) {                   // the last channel alone: taps (2 q, 2 q + 1), tap KK (odd KK) is the zero link
            const float *cb = img + (g.c_in - 1) * g.CHS + base0;
            const int KK = g.kh * g.kw;
            int tap = hh, tkx = hh, tky = 0;
            while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            for (; m < g.nsteps; ++m) {
                const float bv = tap < KK ? cb[tky * g.WP + tkx] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa(m), bv, acc, 0, 0, 0);
                tap += 2;
                tkx += 2;
                while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            }
        }
        return acc;
    };

    // pooling pass of step t over vpl: a half wave = the 32 pixels of one spike word of one channel
    auto pool_pass = [&](int t) {
        if (!spk_out && !pv_out) return;
        const int units = g.c_out * g.ow, pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2;
        const long ob = ((long)t * B + b) * g.c_out;
        for (int u0 = 2 * wv; u0 < units; u0 += 2 * ANY_NW) {
            const int u = u0 + hh;
            const bool uv = u < units;
            const int uc = uv ? u : 0, co = fdiv(uc, g.dOW), wi = uc - co * g.ow, pp = wi * 32 + j;
            const bool pvld = uv && pp < g.PP;
            const int ppc = pvld ? pp : 0, py = fdiv(ppc, g.dPW), px = ppc - py * g.pw;
            const float *vc = vpl + co * g.CP;
            float m = -INFINITY;
            for (int dy = 0; dy < g.pool_h; ++dy) {
                const int yy = py * g.pool_h - pph + dy;
                if (yy < 0 || yy >= g.ch) continue;
                for (int dx = 0; dx < g.pool_w; ++dx) {
                    const int xx = px * g.pool_w - ppw + dx;
                    if (xx < 0 || xx >= g.cw) continue;
                    m = fmaxf(m, vc[yy * g.cw + xx]);
                }
            }
            const unsigned long long mk = __ballot(pvld && m > 0.0f);
            if (pvld && pv_out) pv_out[(ob + co) * g.PP + pp] = sigmoidf_dev(m);
            if (spk_out && uv && j == 0) spk_out[(ob + co) * g.ow + wi] = (uint32_t)(hh ? mk >> 32 : mk);
        }
    };

    for (int t = 0; t < T; ++t) {
        const uint32_t *sp = spk_in + ((long)t * B + b) * g.c_in * g.iw;
        const long ob = ((long)t * B + b) * g.c_out;
        if constexpr (REGS) {
            // ---- phase A: traces of this step.  (tv, jv: the thread's indices made opaque once per step — the element and
            // store offsets derived from them do not change from step to step, and hoisted out of the time loop they would
            // occupy ~200 registers and spill)
            int tv = tid, jv = j;
            asm volatile("" : "+v"(tv), "+v"(jv));
#pragma unroll
            for (int k = 0; k < ANY_KE; ++k) {
                const int i = tv + k * ANY_THREADS;
                if (i < NIN) trace(sp, i, e0r[k]);
                if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);      // (four elements in flight, not 36)
            }
            __syncthreads();
            // ---- phase B: the chains and, from the accumulators, the whole epilogue (no pooling: conv pixel = output pixel)
#pragma unroll
            for (int q = 0; q < ANY_QMAX; ++q) {
                const int tl = wv + ANY_NW * q;
                if (tl < NTL) {
                    const f32x16 acc = chain(tl);
                    const int pix = tl * 32 + jv;
                    const bool pok = pix < g.CP;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = (r & 3) + 8 * (r >> 2) + 4 * hh;
                        const bool ok = pok && co < g.c_out;
                        float v = acc[r];
                        bool s;
                        if (R) v = refractory(acc[r], arpr[q][r], alpharp, wrp, s);
                        else s = v > 0.0f;
                        const unsigned long long mk = __ballot(s && ok);
                        if (ok) {
                            if (pv_out) pv_out[(ob + co) * g.CP + pix] = sigmoidf_dev(v);
                            if (v_out) v_out[(ob + co) * g.CP + pix] = v;
                        }
                        if (spk_out && jv == 0 && co < g.c_out) spk_out[(ob + co) * g.ow + tl] = (uint32_t)(hh ? mk >> 32 : mk);
                    }
                }
            }
            __syncthreads();
        } else {
            // ---- phase A: pooled outputs of the previous step; traces of this step, in place
            if (t > 0) pool_pass(t - 1);
            for (int i = tid; i < NIN; i += ANY_THREADS) trace(sp, i, e0s[i]);
            __syncthreads();
            // ---- phase B: the chains -> vpl
            for (int tl = wv; tl < NTL; tl += ANY_NW) {
                const f32x16 acc = chain(tl);
                const int pix = tl * 32 + j;
                if (pix < g.CP) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = (r & 3) + 8 * (r >> 2) + 4 * hh;
                        if (co < g.c_out) vpl[co * g.CP + pix] = acc[r];
                    }
                }
            }
            __syncthreads();
            // ---- phase C: refractory update on the v plane, v_out
            if (R || v_out) {
                float *vo = v_out ? v_out + ob * g.CP : nullptr;
                for (int i = tid; i < NV; i += ANY_THREADS) {
                    float v = vpl[i];
                    if (R) {
                        float a = arps[i];
                        bool s;
                        v = refractory(v, a, alpharp, wrp, s);
                        arps[i] = a;
                        vpl[i] = v;
                    }
                    if (vo) vo[i] = v;
                }
                __syncthreads();
            }
        }
    }
    // ---- last step's pooled outputs; state back to HBM
    if constexpr (REGS) {
#pragma unroll
        for (int k = 0; k < ANY_KE; ++k) {
            const int i = tid + k * ANY_THREADS;
            if (i < NIN) {
                int ci, p;
                const int q = img_at(i, ci, p);
                eps0_g[b * NIN + i] = e0r[k];
                eps1_g[b * NIN + i] = img[q];
            }
        }
        if (R) {
#pragma unroll
            for (int q = 0; q < ANY_QMAX; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = (r & 3) + 8 * (r >> 2) + 4 * hh, pix = (wv + ANY_NW * q) * 32 + j;
                    if (co < g.c_out && pix < g.CP) arp_g[b * NV + co * g.CP + pix] = arpr[q][r];
                }
        }
    } else {
        pool_pass(T - 1);
        for (int i = tid; i < NIN; i += ANY_THREADS) {
            int ci, p;
            const int q = img_at(i, ci, p);
            eps0_g[b * NIN + i] = e0s[i];
            eps1_g[b * NIN + i] = img[q];
        }
        if (R)
            for (int i = tid; i < NV; i += ANY_THREADS) arp_g[b * NV + i] = arps[i];
    }
}

template <bool R, bool WLDS, bool REGS>
static int launch_any(const any_geom &g, size_t lds_bytes, const uint32_t *spk_in, const float *wperm, const float *b,
                      const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out, float *v_out,
                      int T, int B, float alpharp, float wrp, hipStream_t st, const char *name)
{
    if (hipFuncSetAttribute((const void *)k_lif_seq_any<R, WLDS, REGS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_seq_any: cannot reserve its LDS");
    }
    hipLaunchKernelGGL((k_lif_seq_any<R, WLDS, REGS>), dim3(B), dim3(ANY_THREADS), lds_bytes, st, g, spk_in, wperm, b, tau4, eps0,
                       eps1, arp, spk_out, pv_out, v_out, T, B, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

extern "C" int dcll_conv_lif_sequence_any(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                          const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out,
                                          float *pv_out, float *v_out, float *w_scratch, int32_t T, int32_t B, void *stream)
{
    const char *who = "dcll_conv_lif_sequence_any";
    if (T < 0 || B < 0) return fail(DCLL_ERR_INVALID, "negative T or B", who);
    if (T == 0 || B == 0) return DCLL_OK;
    bool regs = false;
    int rc = any_supported(d, who, &regs);
    if (rc) return rc;
    if (!spk_in || !W || !tau4 || !eps0 || !eps1 || !w_scratch) return fail(DCLL_ERR_INVALID, "null pointer", who);
    if (d->refractory && !arp) return fail(DCLL_ERR_INVALID, "refractory layer needs arp", who);
    hipStream_t st = (hipStream_t)stream;
    any_geom g;
    g.c_in = d->c_in; g.c_out = d->c_out; g.h = d->h; g.w = d->w; g.kh = d->kh; g.kw = d->kw;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.pool_h = d->pool_h; g.pool_w = d->pool_w;
    g.WP = d->w + 2 * d->pad_w;
    g.CHS = (d->h + 2 * d->pad_h) * g.WP;
    conv_shape(d, &g.ch, &g.cw, &g.ph, &g.pw);
    g.CP = g.ch * g.cw;
    g.PP = g.ph * g.pw;
    g.npair = (int)any_chain_pairs(d);
    g.nsteps = (int)any_chain_steps(d);
    g.iw = (d->h * d->w + 31) / 32;
    g.ow = (g.PP + 31) / 32;
    g.o_e0 = d->c_in * g.CHS;
    g.o_v = g.o_e0 + (regs ? 0 : d->c_in * d->h * d->w);
    g.o_arp = g.o_v + (regs ? 0 : d->c_out * g.CP);
    g.o_tau = g.o_arp + ((d->refractory && !regs) ? d->c_out * g.CP : 0);
    g.o_bias = g.o_tau + 4 * d->c_in;
    g.o_w = g.o_bias + 32;
    g.dHW = make_div(d->h * d->w); g.dW = make_div(d->w); g.dCW = make_div(g.cw); g.dOW = make_div(g.ow); g.dPW = make_div(g.pw);
    const long base = g.o_w;
    if (base != (regs ? any_lds_floats_regs(d) : any_lds_floats(d)))        // the layout above against the ONE exported formula
        return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_sequence_any_lds disagree", who);
    g.nwl = seq_weight_room(base, g.nsteps, 1, B);
    const bool wlds = !regs && g.nwl == g.nsteps;
    const size_t lds_bytes = (size_t)(base + (long)g.nwl * 64) * 4;

    if ((rc = dcll_launch_seq_wprep(d, W, w_scratch, 1, st, true)) != DCLL_OK) return rc;
    // launch-log names: k_lif_seq_any<refractory, weights in LDS, register form>
#define DCLL_ANY(R_, L_, G_)                                                                                                  \
    return launch_any<R_, L_, G_>(g, lds_bytes, spk_in, w_scratch, b, tau4, eps0, eps1, arp, spk_out, pv_out, v_out, T, B,    \
                                  d->alpharp, d->wrp, st, "k_lif_seq_any<" #R_ "," #L_ "," #G_ ">")
    if (d->refractory) {
        if (regs) DCLL_ANY(1, 0, 1);
        if (wlds) DCLL_ANY(1, 1, 0);
        DCLL_ANY(1, 0, 0);
    }
    if (regs) DCLL_ANY(0, 0, 1);
    if (wlds) DCLL_ANY(0, 1, 0);
    DCLL_ANY(0, 0, 0);
#undef DCLL_ANY
}

// ------------------------------------------------------------------------------------------------------------
// spike planes of any size: ceil(hw / 32) words per plane, bit pix % 32 of word pix / 32, tail bits zero
// ------------------------------------------------------------------------------------------------------------
__global__ void k_pack_planes(const float *__restrict__ dense, uint32_t *__restrict__ packed, long n_units, int hw, int wpp)
{
    const int lane = threadIdx.x & 63, j = lane & 31, hh = lane >> 5;
    const long nwave = (long)gridDim.x * (blockDim.x >> 6), wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    for (long u0 = 2 * wave; u0 < n_units; u0 += 2 * nwave) {      // a half wave = one word
        const long u = u0 + hh;
        const bool uv = u < n_units;
        const long plane = uv ? u / wpp : 0;
        const int wi = uv ? (int)(u - plane * wpp) : 0, pix = wi * 32 + j;
        const bool bit = uv && pix < hw && dense[plane * hw + pix] != 0.0f;
        const unsigned long long mk = __ballot(bit);
        if (uv && j == 0) packed[u] = (uint32_t)(hh ? mk >> 32 : mk);
    }
}

__global__ void k_unpack_planes(const uint32_t *__restrict__ packed, float *__restrict__ dense, long n, int hw, int wpp)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {       // one output float
        const long plane = i / hw;
        const int pix = (int)(i - plane * hw);
        dense[i] = (float)((packed[plane * wpp + (pix >> 5)] >> (pix & 31)) & 1u);
    }
}

static inline int plane_blocks(long work, int per_block)
{
    const long n = (work + per_block - 1) / per_block;
    return (int)(n < 1 ? 1 : n > 65536 ? 65536 : n);
}

extern "C" int dcll_pack_spike_planes(const float *dense, uint32_t *packed, int64_t n_planes, int32_t hw, void *stream)
{
    if (n_planes < 0 || hw < 1) return fail(DCLL_ERR_INVALID, "dcll_pack_spike_planes: bad argument");
    if (n_planes == 0) return DCLL_OK;
    if (!dense || !packed) return fail(DCLL_ERR_INVALID, "dcll_pack_spike_planes: null pointer");
    const int wpp = (hw + 31) / 32;
    const long units = (long)n_planes * wpp;
    hipLaunchKernelGGL(k_pack_planes, dim3(plane_blocks(units, 8)), dim3(256), 0, (hipStream_t)stream, dense, packed, units, hw, wpp);
    HIP_CHECK_LAUNCH("k_pack_planes");
    return DCLL_OK;
}

extern "C" int dcll_unpack_spike_planes(const uint32_t *packed, float *dense, int64_t n_planes, int32_t hw, void *stream)
{
    if (n_planes < 0 || hw < 1) return fail(DCLL_ERR_INVALID, "dcll_unpack_spike_planes: bad argument");
    if (n_planes == 0) return DCLL_OK;
    if (!dense || !packed) return fail(DCLL_ERR_INVALID, "dcll_unpack_spike_planes: null pointer");
    const long n = (long)n_planes * hw;
    hipLaunchKernelGGL(k_unpack_planes, dim3(plane_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, packed, dense, n, hw,
                       (hw + 31) / 32);
    HIP_CHECK_LAUNCH("k_unpack_planes");
    return DCLL_OK;
}
