// dcll_seq_wide.hip — k_lif_seq_wide: all T timesteps of a plain conv layer with 33..64 output channels (stride = dilation =
// groups = 1, kernel up to 16x16, any padding, any pooling) in one launch, one workgroup per sample, the neuron state on chip
// (dcll_conv_lif_sequence_wide) — the fused path of the layers a --netscale above 1 makes (radio_ml_conv.yaml at netscale 2:
// 1 -> 64, 64 -> 64, 64 -> 64; mnist_conv.yaml at netscale 2: 32 / 48 / 64 channels).  Opt-in, beside k_lif_seq_any, whose
// decomposition this is with TWO 32-row M tiles; a layer of at most 32 output channels is handed to
// dcll_conv_lif_sequence_any unchanged, so a network of mixed widths goes through one entry point.
//
// LDS of a workgroup (floats; wide_lds_floats() is the ONE statement of it, exported as dcll_conv_lif_sequence_wide_lds):
//   img   c_in x (h + 2 pad_h) x (w + 2 pad_w)   eps1, zero padded: the B operand of every chain link is one read
//   e0    c_in x h x w                           eps0
//   vpl   c_out x ch x cw                        v of ONE step at conv resolution (the pooling pass reads windows of it)
//   arp   c_out x ch x cw                        refractory layers only
//   tau   4 x c_in, bias 32 x MT
//   + the permuted weights behind these: all of them when they fit (WLDS), else as many chain steps as fit — the rest is
//     streamed from L2, eight steps (sixteen fragments) in flight per wave.
// A layer WITHOUT pooling whose set is larger (radio_ml_conv.yaml's 64 -> 64 layers on 16x16: the image alone is 121 KiB) runs
// the register form (REGS) when c_in h w <= 18432 and ch cw <= 256: only img (+ tau, bias) in LDS, eps0 in the registers of the
// thread that advances the element (<= 36 per thread), arp in the accumulator layout of the wave that owns the tile (ONE tile
// x 2 M tiles x 16) and the epilogue straight from the accumulators.  The register budget is that of k_lif_seq_any's form:
// MT x (tiles per wave) <= 3 — 32 accumulator + 32 arp registers where that one has 16 + 48.
//
// Arithmetic = the contract of include/dcll_hip.h, as in k_lif_seq_any: the chain of output (co, y, x) starts at bias[co] and
// runs over the links (cp, ky, kx, h), ci = 2 cp + h, one v_mfma_f32_32x32x2_f32 per two CONSECUTIVE links; the last channel of
// an odd c_in pairs its taps; a chain of odd length ends with a zero link.  M = c_out padded to 64 rows (zero weights), N = 32
// pixels of the flattened conv plane; a wave owns whole pixel tiles and runs BOTH 32-row chains of a tile itself, interleaved:
// one LDS read of the B operand feeds two MFMAs, one per M tile.  The two chains are independent and each is unsplit, so every
// v is still ONE fmaf chain.  Weights are permuted in front of every launch (k_seq_any_wprep at MT = 2, nothing cached):
// wperm[m][mt][lane] = weight of link 2 m + (lane >> 5) for output channel 32 mt + (lane & 31) — one coalesced 512-byte read per
// step and wave.
//
// One step = the three phases of k_lif_seq_any (A traces + pooling pass of the previous step, B chains -> vpl, C refractory
// update + v_out), a barrier behind each.  State is read once before the first step and written once behind the last.
#include "dcll_any_shared.h"

constexpr int WIDE_THREADS = 512, WIDE_NW = WIDE_THREADS / 64;
constexpr int WIDE_MAX_COUT = 64, WIDE_MT = 2;
constexpr int WIDE_KE = 36;         // register form: eps0 values per thread (one pixel tile per wave)

struct wide_geom {
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
static inline long wide_lds_floats(const dcll_conv_desc *d)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const long img = (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w);
    const long e0 = (long)d->c_in * d->h * d->w;
    const long vpl = (long)d->c_out * ch * cw;
    return img + e0 + vpl * (d->refractory ? 2 : 1) + 4L * d->c_in + 32 * WIDE_MT;
}

// the register form's set: img + tau + bias; for layers without pooling within its per-thread / per-wave register arrays
static inline long wide_lds_floats_regs(const dcll_conv_desc *d)
{
    return (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w) + 4L * d->c_in + 32 * WIDE_MT;
}
static inline bool wide_regs_ok(const dcll_conv_desc *d)
{
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    return d->pool_h == 1 && d->pool_w == 1 && (long)d->c_in * d->h * d->w <= (long)WIDE_KE * WIDE_THREADS &&
           (long)ch * cw <= 32L * WIDE_NW && wide_lds_floats_regs(d) * 4 <= ANY_LDS_MAX;
}

// the support predicate of the layers this file serves or forwards: DCLL_OK (*regs: the register form serves the layer; c_out <=
// 32: the answer is dcll_conv_lif_sequence_any's), or the refusal with its message
static int wide_supported(const dcll_conv_desc *d, const char *who, bool *regs = nullptr)
{
    int rc = any_layer_ok(d, WIDE_MAX_COUT, who);
    if (rc) return rc;
    if (d->c_out <= 32) return dcll_conv_lif_sequence_any_lds(d) > 0 ? DCLL_OK : DCLL_ERR_UNSUPPORTED;     // (its message stands)
    const bool full = wide_lds_floats(d) * 4 <= ANY_LDS_MAX;
    if (!full && !wide_regs_ok(d))
        return fail(DCLL_ERR_UNSUPPORTED, "the per-sample working set (padded eps1 image, eps0, the v plane) exceeds the 160 KiB of LDS "
                                          "and the layer is outside the register form (no pooling, c_in h w <= 18432, ch cw <= 256)", who);
    if (regs) *regs = !full;
    return DCLL_OK;
}

extern "C" int64_t dcll_conv_lif_sequence_wide_lds(const dcll_conv_desc *d)
{
    bool regs = false;
    if (wide_supported(d, "dcll_conv_lif_sequence_wide_lds", &regs) != DCLL_OK) return 0;
    if (d->c_out <= 32) return dcll_conv_lif_sequence_any_lds(d);
    return (regs ? wide_lds_floats_regs(d) : wide_lds_floats(d)) * 4;
}
extern "C" int64_t dcll_conv_lif_sequence_wide_scratch(const dcll_conv_desc *d)
{
    if (wide_supported(d, "dcll_conv_lif_sequence_wide_scratch") != DCLL_OK) return 0;
    if (d->c_out <= 32) return dcll_conv_lif_sequence_any_scratch(d);
    return any_chain_steps(d) * 64 * WIDE_MT;
}

struct f32x16x2 {
    f32x16 t[WIDE_MT];
};

template <bool R, bool WLDS, bool REGS>
__global__ __launch_bounds__(WIDE_THREADS) void k_lif_seq_wide(const wide_geom g, const uint32_t *__restrict__ spk_in,
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
    float e0r[REGS ? WIDE_KE : 1], arpr[REGS ? WIDE_MT : 1][16];      // register form: eps0 of elements tid + 512 k; arp of tile wv

    // position of input element i (channel ci, pixel p) in img
    auto img_at = [&](int i, int &ci, int &p) -> int {
        ci = fdiv(i, g.dHW);
        p = i - ci * HW;
        const int y = fdiv(p, g.dW), x = p - y * g.w;
        return ci * g.CHS + (y + g.pad_h) * g.WP + x + g.pad_w;
    };

    // ---- prologue: state and constants on chip
    for (int i = tid; i < g.c_in * g.CHS; i += WIDE_THREADS) img[i] = 0.0f;
    __syncthreads();
    if constexpr (REGS) {
#pragma unroll
        for (int k = 0; k < WIDE_KE; ++k) {
            const int i = tid + k * WIDE_THREADS;
            e0r[k] = 0.0f;
            if (i < NIN) {
                int ci, p;
                const int q = img_at(i, ci, p);
                e0r[k] = eps0_g[b * NIN + i];
                img[q] = eps1_g[b * NIN + i];
            }
        }
#pragma unroll
        for (int mt = 0; mt < WIDE_MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh, pix = wv * 32 + j;
                arpr[mt][r] = (R && co < g.c_out && pix < g.CP) ? arp_g[b * NV + co * g.CP + pix] : 0.0f;
            }
    } else {
        for (int i = tid; i < NIN; i += WIDE_THREADS) {
            int ci, p;
            const int q = img_at(i, ci, p);
            e0s[i] = eps0_g[b * NIN + i];
            img[q] = eps1_g[b * NIN + i];
        }
        if (R)
            for (int i = tid; i < NV; i += WIDE_THREADS) arps[i] = arp_g[b * NV + i];
    }
    for (int i = tid; i < 4 * g.c_in; i += WIDE_THREADS) taus[i] = tau4[i];
    if (tid < 32 * WIDE_MT) sb[tid] = (bias && tid < g.c_out) ? bias[tid] : 0.0f;
    for (int i = tid; i < (WLDS ? g.nsteps : g.nwl) * 64 * WIDE_MT; i += WIDE_THREADS) wl[i] = wperm[i];
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

    // the two chains of pixel tile tl: 32 conv pixels x (2 x 32) channel rows, one B operand read per step for both
    auto chain = [&](int tl) -> f32x16x2 {
        const int pix = tl * 32 + j, pc = pix < g.CP ? pix : g.CP - 1, y = fdiv(pc, g.dCW), x = pc - y * g.cw;
        const int base0 = y * g.WP + x;
        const float *bp = img + base0 + hh * g.CHS;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] = sb[(r & 3) + 8 * (r >> 2) + 4 * hh];
            acc1[r] = sb[32 + (r & 3) + 8 * (r >> 2) + 4 * hh];
        }
        auto wa = [&](int m, int mt) -> float {
            const int o = (m * WIDE_MT + mt) * 64 + lane;
            if constexpr (WLDS) return wl[o];
            else return m < g.nwl ? wl[o] : wperm[o];
        };
        int m = 0, off = 0, kx = 0, ky = 0;
        for (; m < g.npair; m += 8) {       // (cp, ky, kx): both channels of the pair at one wave-uniform offset
            float a0[8], a1[8];             // eight steps requested before the first is used (the streamed ones: L2 latency)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int mu = m + u < g.npair ? m + u : g.npair - 1;
                a0[u] = wa(mu, 0);
                a1[u] = wa(mu, 1);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (m + u < g.npair) {
                    const float bv = bp[off];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], bv, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], bv, acc1, 0, 0, 0);
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
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa(m, 0), bv, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa(m, 1), bv, acc1, 0, 0, 0);
                tap += 2;
                tkx += 2;
                while (tkx >= g.kw) { tkx -= g.kw; ++tky; }
            }
        }
        f32x16x2 out;
        out.t[0] = acc0;
        out.t[1] = acc1;
        return out;
    };

    // pooling pass of step t over vpl: a half wave = the 32 pixels of one spike word of one channel
    auto pool_pass = [&](int t) {
        if (!spk_out && !pv_out) return;
        const int units = g.c_out * g.ow, pph = (g.pool_h - 1) / 2, ppw = (g.pool_w - 1) / 2;
        const long ob = ((long)t * B + b) * g.c_out;
        for (int u0 = 2 * wv; u0 < units; u0 += 2 * WIDE_NW) {
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
            // occupy registers the accumulators need)
            int tv = tid, jv = j;
            asm volatile("" : "+v"(tv), "+v"(jv));
#pragma unroll
            for (int k = 0; k < WIDE_KE; ++k) {
                const int i = tv + k * WIDE_THREADS;
                if (i < NIN) trace(sp, i, e0r[k]);
                if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);      // (four elements in flight, not 36)
            }
            __syncthreads();
            // ---- phase B: the chains and, from the accumulators, the whole epilogue (no pooling: conv pixel = output pixel)
            if (wv < NTL) {
                const f32x16x2 acc = chain(wv);
                const int pix = wv * 32 + jv;
                const bool pok = pix < g.CP;
#pragma unroll
                for (int mt = 0; mt < WIDE_MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
                        const bool ok = pok && co < g.c_out;
                        float v = acc.t[mt][r];
                        bool s;
                        if (R) v = refractory(acc.t[mt][r], arpr[mt][r], alpharp, wrp, s);
                        else s = v > 0.0f;
                        const unsigned long long mk = __ballot(s && ok);
                        if (ok) {
                            if (pv_out) pv_out[(ob + co) * g.CP + pix] = sigmoidf_dev(v);
                            if (v_out) v_out[(ob + co) * g.CP + pix] = v;
                        }
                        if (spk_out && jv == 0 && co < g.c_out) spk_out[(ob + co) * g.ow + wv] = (uint32_t)(hh ? mk >> 32 : mk);
                    }
            }
            __syncthreads();
        } else {
            // ---- phase A: pooled outputs of the previous step; traces of this step, in place
            if (t > 0) pool_pass(t - 1);
            for (int i = tid; i < NIN; i += WIDE_THREADS) trace(sp, i, e0s[i]);
            __syncthreads();
            // ---- phase B: the chains -> vpl
            for (int tl = wv; tl < NTL; tl += WIDE_NW) {
                const f32x16x2 acc = chain(tl);
                const int pix = tl * 32 + j;
                if (pix < g.CP) {
#pragma unroll
                    for (int mt = 0; mt < WIDE_MT; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
                            if (co < g.c_out) vpl[co * g.CP + pix] = acc.t[mt][r];
                        }
                }
            }
            __syncthreads();
            // ---- phase C: refractory update on the v plane, v_out
            if (R || v_out) {
                float *vo = v_out ? v_out + ob * g.CP : nullptr;
                for (int i = tid; i < NV; i += WIDE_THREADS) {
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
        for (int k = 0; k < WIDE_KE; ++k) {
            const int i = tid + k * WIDE_THREADS;
            if (i < NIN) {
                int ci, p;
                const int q = img_at(i, ci, p);
                eps0_g[b * NIN + i] = e0r[k];
                eps1_g[b * NIN + i] = img[q];
            }
        }
        if (R) {
#pragma unroll
            for (int mt = 0; mt < WIDE_MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh, pix = wv * 32 + j;
                    if (co < g.c_out && pix < g.CP) arp_g[b * NV + co * g.CP + pix] = arpr[mt][r];
                }
        }
    } else {
        pool_pass(T - 1);
        for (int i = tid; i < NIN; i += WIDE_THREADS) {
            int ci, p;
            const int q = img_at(i, ci, p);
            eps0_g[b * NIN + i] = e0s[i];
            eps1_g[b * NIN + i] = img[q];
        }
        if (R)
            for (int i = tid; i < NV; i += WIDE_THREADS) arp_g[b * NV + i] = arps[i];
    }
}

// the LDS reservation, then the weight permutation, then the kernel: an error return never follows a launch
template <bool R, bool WLDS, bool REGS>
static int launch_wide(const dcll_conv_desc *d, const wide_geom &g, size_t lds_bytes, const uint32_t *spk_in, const float *W,
                       float *wperm, const float *b, const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out, float *v_out,
                       int T, int B, float alpharp, float wrp, hipStream_t st, const char *name)
{
    if (hipFuncSetAttribute((const void *)k_lif_seq_wide<R, WLDS, REGS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_seq_wide: cannot reserve its LDS");
    }
    const int rc = dcll_launch_seq_wprep(d, W, wperm, WIDE_MT, st, false);       // (not in the launch log)
    if (rc) return rc;
    hipLaunchKernelGGL((k_lif_seq_wide<R, WLDS, REGS>), dim3(B), dim3(WIDE_THREADS), lds_bytes, st, g, spk_in, wperm, b, tau4, eps0,
                       eps1, arp, spk_out, pv_out, v_out, T, B, alpharp, wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

extern "C" int dcll_conv_lif_sequence_wide(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                           const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out,
                                           float *pv_out, float *v_out, float *w_scratch, int32_t T, int32_t B, void *stream)
{
    const char *who = "dcll_conv_lif_sequence_wide";
    if (T < 0 || B < 0) return fail(DCLL_ERR_INVALID, "negative T or B", who);
    if (T == 0 || B == 0) return DCLL_OK;
    bool regs = false;
    int rc = wide_supported(d, who, &regs);
    if (rc) return rc;
    // one M tile: k_lif_seq_any's layer, its kernels, its launch-log names
    if (d->c_out <= 32)
        return dcll_conv_lif_sequence_any(d, spk_in, W, b, tau4, eps0, eps1, arp, spk_out, pv_out, v_out, w_scratch, T, B, stream);
    if (!spk_in || !W || !tau4 || !eps0 || !eps1 || !w_scratch) return fail(DCLL_ERR_INVALID, "null pointer", who);
    if (d->refractory && !arp) return fail(DCLL_ERR_INVALID, "refractory layer needs arp", who);
    hipStream_t st = (hipStream_t)stream;
    wide_geom g;
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
    g.o_w = g.o_bias + 32 * WIDE_MT;
    g.dHW = make_div(d->h * d->w); g.dW = make_div(d->w); g.dCW = make_div(g.cw); g.dOW = make_div(g.ow); g.dPW = make_div(g.pw);
    const long base = g.o_w;
    if (base != (regs ? wide_lds_floats_regs(d) : wide_lds_floats(d)))      // the layout above against the ONE exported formula
        return fail(DCLL_ERR_LAUNCH, "LDS layout and dcll_conv_lif_sequence_wide_lds disagree", who);
    g.nwl = seq_weight_room(base, g.nsteps, WIDE_MT, B);
    const bool wlds = !regs && g.nwl == g.nsteps;
    const size_t lds_bytes = (size_t)(base + (long)g.nwl * 64 * WIDE_MT) * 4;

    // launch-log names: k_lif_seq_wide<refractory, weights in LDS, register form>
#define DCLL_WIDE(R_, L_, G_)                                                                                                 \
    return launch_wide<R_, L_, G_>(d, g, lds_bytes, spk_in, W, w_scratch, b, tau4, eps0, eps1, arp, spk_out, pv_out, v_out, T,    \
                                   B, d->alpharp, d->wrp, st, "k_lif_seq_wide<" #R_ "," #L_ "," #G_ ">")
    if (d->refractory) {
        if (regs) DCLL_WIDE(1, 0, 1);
        if (wlds) DCLL_WIDE(1, 1, 0);
        DCLL_WIDE(1, 0, 0);
    }
    if (regs) DCLL_WIDE(0, 0, 1);
    if (wlds) DCLL_WIDE(0, 1, 0);
    DCLL_WIDE(0, 0, 0);
#undef DCLL_WIDE
}
