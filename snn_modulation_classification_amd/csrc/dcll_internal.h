// dcll_internal.h — what the translation units of libdcll_hip.so share: vector typedefs, the geometry constants of
// the LDS-resident layouts, the error plumbing of the C ABI and the device helpers that define the pinned arithmetic
// (include/dcll_hip.h).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dcll_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// geometry of the LDS-resident 32-channel 16x16 eps1 image shared by k_lif_seq_c32 and k_bwd_wgrad_c32
constexpr int NWAVE = 8, CPW = 4, ROWF = 19, CHF = 361;
constexpr int IMG_FLOATS = ((32 * CHF + 3 * ROWF + 3 + 61) + 3) & ~3;     // 11676 >= offset of (ci=31, y=18, x=18) + 1
constexpr int SLOT_FLOATS = 16 * 64;

// ------------------------------------------------------------------------------------------------------------
// error plumbing (the message buffer lives in dcll_hip.hip; one per thread)
// ------------------------------------------------------------------------------------------------------------
__attribute__((visibility("hidden"))) char *dcll_err_buf(void);
constexpr size_t DCLL_ERR_LEN = 512;

static inline int fail(int code, const char *msg, const char *who = nullptr)
{
    if (who) snprintf(dcll_err_buf(), DCLL_ERR_LEN, "%s: %s", who, msg);
    else snprintf(dcll_err_buf(), DCLL_ERR_LEN, "%s", msg);
    return code;
}

// descriptor geometry and checks shared by the entry points of every translation unit
static inline void conv_shape(const dcll_conv_desc *d, int *ch, int *cw, int *ph, int *pw)
{
    // (reference get_output_shape, dcll/pytorch_libdcll.py:368-375; stride = dilation = 1: h + 2 pad - kh + 1)
    *ch = (d->h + 2 * d->pad_h - d->dilation * (d->kh - 1) - 1) / d->stride + 1;
    *cw = (d->w + 2 * d->pad_w - d->dilation * (d->kw - 1) - 1) / d->stride + 1;
    *ph = (*ch + 2 * ((d->pool_h - 1) / 2) - d->pool_h) / d->pool_h + 1;
    *pw = (*cw + 2 * ((d->pool_w - 1) / 2) - d->pool_w) / d->pool_w + 1;
}

// the specialised kernels (MFMA step / sequence / weight-gradient kernels, the tiled VALU kernel) are plain convolutions
static inline bool plain_conv(const dcll_conv_desc *d) { return d->stride == 1 && d->dilation == 1 && d->groups == 1; }

static inline int check_desc(const dcll_conv_desc *d)
{
    if (!d) return fail(DCLL_ERR_INVALID, "null descriptor");
    if (d->c_in < 1 || d->c_out < 1 || d->h < 1 || d->w < 1 || d->kh < 1 || d->kw < 1 || d->pad_h < 0 ||
        d->pad_w < 0 || d->pool_h < 1 || d->pool_w < 1 || d->target < 0)
        return fail(DCLL_ERR_INVALID, "descriptor has a non-positive dimension");
    // stride / dilation / groups other than 1 (F.conv2d's, reference :417 / :495): served by the generic per-step kernels
    // (k_conv_lif, k_bwd_wgrad) only — ConvNetwork never builds such a layer
    if (d->stride < 1 || d->dilation < 1 || d->groups < 1 || d->c_in % d->groups != 0 || d->c_out % d->groups != 0)
        return fail(DCLL_ERR_INVALID, "stride / dilation / groups must be >= 1 and groups must divide c_in and c_out");
    if (d->h + 2 * d->pad_h < d->dilation * (d->kh - 1) + 1 || d->w + 2 * d->pad_w < d->dilation * (d->kw - 1) + 1)
        return fail(DCLL_ERR_INVALID, "empty conv/pool output");
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    if (ch < 1 || cw < 1 || ph < 1 || pw < 1) return fail(DCLL_ERR_INVALID, "empty conv/pool output");
    return DCLL_OK;
}

// dcll_kernel_trace (ABI 5): while a thread records, every launch check notes the kernel's name (dcll_hip.hip)
__attribute__((visibility("hidden"))) void dcll_trace_note(const char *name);

#define HIP_CHECK_LAUNCH(name)                                                              \
    do {                                                                                    \
        dcll_trace_note(name);                                                              \
        hipError_t e_ = hipGetLastError();                                                  \
        if (e_ != hipSuccess) {                                                             \
            snprintf(dcll_err_buf(), DCLL_ERR_LEN, "%s: %s", name, hipGetErrorString(e_));  \
            return DCLL_ERR_LAUNCH;                                                         \
        }                                                                                   \
    } while (0)

// ------------------------------------------------------------------------------------------------------------
// conv weights as a kernel sees them: fp32, or int8 + one fp32 scale per output channel (dcll_layer_opts, ABI v3).
// at(idx, co) is the ONE place a weight is converted: (float)q * scale[co], a single rounded multiply — bit for bit what
// the dequantised fp32 tensor holds, so every chain downstream is unchanged.  The branch is wave-uniform.
// ------------------------------------------------------------------------------------------------------------
// thresholds of sample b of the IQ quantiser: the scalar-path table for the samples the mask marks (dcll_iq_tail)
__device__ __forceinline__ void iq_tables(const float *thr_i, const float *thr_q, const dcll_iq_tail &tail, long b,
                                          const float *&ti, const float *&tq)
{
    const bool tl = tail.tail_mask && tail.tail_mask[b];
    ti = tl ? tail.thr_i_tail : thr_i;
    tq = tl ? tail.thr_q_tail : thr_q;
}
static inline dcll_iq_tail make_iq_tail(const dcll_iq_tail *t) { return t ? *t : dcll_iq_tail{nullptr, nullptr, nullptr}; }

struct dcll_wsrc {
    const float *f;
    const int8_t *q;
    const float *scale;
    __device__ __forceinline__ float at(long idx, int co) const { return q ? (float)q[idx] * scale[co] : f[idx]; }
};
// the 2 x 49 stationary A fragments of a 32 -> 32 7x7 sequence kernel: W[j][4 w + 2 cp + h][tap]; ONE wave-uniform branch
// on the weight format around the whole load (not one per weight)
__device__ __forceinline__ void load_wf_c32(const dcll_wsrc &W, int j, int w, int h, float (&wf)[2][49])
{
    if (W.q) {
        const float sc = W.scale[j];
#pragma unroll
        for (int cp = 0; cp < 2; ++cp)
#pragma unroll
            for (int k = 0; k < 49; ++k) wf[cp][k] = (float)W.q[((long)j * 32 + 4 * w + 2 * cp + h) * 49 + k] * sc;
    } else {
#pragma unroll
        for (int cp = 0; cp < 2; ++cp)
#pragma unroll
            for (int k = 0; k < 49; ++k) wf[cp][k] = W.f[((long)j * 32 + 4 * w + 2 * cp + h) * 49 + k];
    }
}

static inline dcll_wsrc make_wsrc(const float *W, const dcll_layer_opts *o)
{
    return (o && o->w_q8) ? dcll_wsrc{nullptr, o->w_q8, o->w_scale} : dcll_wsrc{W, nullptr, nullptr};
}
// opts of a call checked once: -> DCLL_OK, or the failure code with the message set
static inline int check_opts(const float *W, const dcll_layer_opts *o, bool allow_presig, const char *who)
{
    if (!o) return W ? DCLL_OK : fail(DCLL_ERR_INVALID, "null weight pointer", who);
    if (o->reserved != 0) return fail(DCLL_ERR_INVALID, "dcll_layer_opts.reserved must be 0", who);
    if (o->w_q8 ? !o->w_scale : !W) return fail(DCLL_ERR_INVALID, "weights: need W (fp32) or w_q8 + w_scale (int8)", who);
    if (o->pv_presigmoid && !allow_presig) return fail(DCLL_ERR_INVALID, "pv_presigmoid is an option of the sequence calls", who);
    return DCLL_OK;
}

// k_lif_seq_c32t (dcll_seq_tiled.hip): the 32 -> 32 channel sequence layer on planes with h % 8 == 0, w % 32 == 0
__attribute__((visibility("hidden")))
int dcll_launch_seq_c32t(const dcll_conv_desc *d, const uint32_t *spk_in, dcll_wsrc W, const float *b,
                         const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                         float *v_out, float *state_scratch, int32_t T, int32_t B, hipStream_t st);
// k_lif_seq_c1t: the first layer (c_in 1) on such planes, input as cell indices or raw IQ
__attribute__((visibility("hidden")))
int dcll_launch_seq_c1t(const dcll_conv_desc *d, const int32_t *cells, const float *iq, const float *thr_i,
                        const float *thr_q, dcll_iq_tail tail, int L, int t0, dcll_wsrc W, const float *b, const float *tau4,
                        float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out, float *v_out,
                        float *state_scratch, int T, int B, hipStream_t st, bool presig = false);

// k_lif_seq_w3 (dcll_seq_w3.hip): the (1,3)-kernel / 64-channel / (1,2)-pool layers of radio_ml_conv_ref.yaml, all T steps
__attribute__((visibility("hidden"))) bool dcll_seq_w3_geometry(const dcll_conv_desc *d);
__attribute__((visibility("hidden")))
int dcll_launch_seq_w3(const dcll_conv_desc *d, const uint32_t *spk_in, const int32_t *cells, dcll_wsrc W, const float *b,
                       const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                       float *v_out, bool presigmoid, int32_t T, int32_t B, hipStream_t st);

// k_bwd_wgrad_any (dcll_bwd_any.hip): MFMA weight gradient of any plain conv layer (c_out <= 32, kernel up to 16x16).
// _check: DCLL_OK or the refusal with its message; the launcher caps *nchunk (partial rows there is room for) and returns it
__attribute__((visibility("hidden"))) int dcll_bwd_wgrad_any_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden")))
int dcll_launch_bwd_wgrad_any(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B,
                              long *nchunk, hipStream_t st);

// k_bwd_wgrad_wide (dcll_bwd_wide.hip): MFMA weight gradient of a plain conv layer with 33 .. 64 output channels (kernel up to
// 16x16), two 32-row M tiles per wave.  _check and launcher as for k_bwd_wgrad_any; layers of at most 32 output channels never
// reach them (dcll_conv_lif_backward_wide hands those to the _any path)
__attribute__((visibility("hidden"))) int dcll_bwd_wgrad_wide_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden")))
int dcll_launch_bwd_wgrad_wide(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B,
                               long *nchunk, hipStream_t st);

// k_bwd_wgrad_slab (dcll_bwd_slab.hip): the same for a plain conv layer with more than 64 output channels, in slabs of 64
// (blockIdx.z; the slab rule: dcll_any_shared.h).  _check and launcher as for k_bwd_wgrad_wide; layers of at most 64 output
// channels never reach them (dcll_conv_lif_backward_slab hands those to the _wide path)
__attribute__((visibility("hidden"))) int dcll_bwd_wgrad_slab_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden")))
int dcll_launch_bwd_wgrad_slab(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B,
                               long *nchunk, hipStream_t st);

// k_seq_any_wprep (dcll_seq_any.hip): the weights of a plain conv layer in MFMA fragment order, wperm[m][mt][lane], 64 MT floats
// per chain step (any_chain_steps(), dcll_any_shared.h) — the one permutation of k_lif_seq_any / k_lif_step_any (MT = 1) and of
// k_lif_seq_wide / k_lif_seq_band / k_lif_seq_tile.  note: the launch goes into the launch log (the MT = 1 entry points; the others
// only collect the error); a failure's message starts with errname
__attribute__((visibility("hidden")))
int dcll_launch_seq_wprep(const dcll_conv_desc *d, const float *W, float *wperm, int MT, hipStream_t st, bool note,
                          const char *errname = "k_seq_any_wprep");

// k_lif_step_any (dcll_step_any.hip): one MFMA layer step of any plain conv layer (c_out <= 32, kernel up to 16x16).
// _check: DCLL_OK or the refusal with its message; _split: workgroups per sample (> 1: the caller runs k_trace first);
// the launcher with launch == false only prepares (checks, LDS reservation): called before the first launch of the entry point
__attribute__((visibility("hidden"))) int dcll_step_any_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden"))) int dcll_step_any_split(const dcll_conv_desc *d, int32_t B);
__attribute__((visibility("hidden")))
int dcll_launch_step_any(const dcll_conv_desc *d, const float *x, const float *wperm, const float *b, const float *alpha,
                         const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                         float *out_s, float *out_pv, float *out_v, int ns, int32_t B, hipStream_t st, bool launch);

// k_lif_step_wide (dcll_step_wide.hip): one MFMA layer step of a plain conv layer with 33 .. 64 output channels (kernel up to
// 16x16), two 32-row M tiles.  _check: DCLL_OK or the refusal with its message (c_out <= 32: dcll_step_any_check's answer — the
// entry point hands those layers to dcll_conv_lif_step_any, they never reach the launchers here); _split: workgroups per sample
// (> 1: the caller runs k_trace first); _wprep: w_scratch in k_lif_step_wide's fragment order (128 floats per chain step); the
// launcher with launch == false only prepares (checks, LDS reservation): called before the first launch of the entry point
__attribute__((visibility("hidden"))) int dcll_step_wide_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden"))) int dcll_step_wide_split(const dcll_conv_desc *d, int32_t B);
__attribute__((visibility("hidden"))) int dcll_launch_step_wide_wprep(const dcll_conv_desc *d, const float *W, float *wperm, hipStream_t st);
__attribute__((visibility("hidden")))
int dcll_launch_step_wide(const dcll_conv_desc *d, const float *x, const float *wperm, const float *b, const float *alpha,
                          const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                          float *out_s, float *out_pv, float *out_v, int ns, int32_t B, hipStream_t st, bool launch);

// k_bwd_wgrad_band (dcll_bwd_band.hip): the same for a plain conv layer of any c_out on any plane height, a sample in bands of
// conv-output rows (bands: 0 the rule, N >= 2 forced).  _forwards: the call is dcll_conv_lif_backward_slab's (bands == 1, or
// bands == 0 on a layer that call serves) and never reaches the rest; _check and launcher as for k_bwd_wgrad_slab
__attribute__((visibility("hidden"))) bool dcll_bwd_band_forwards(const dcll_conv_desc *d, int32_t bands);
__attribute__((visibility("hidden"))) int dcll_bwd_wgrad_band_check(const dcll_conv_desc *d, int32_t bands, const char *who);
__attribute__((visibility("hidden")))
int dcll_launch_bwd_wgrad_band(const dcll_conv_desc *d, int32_t bands, const float *gvf, const float *eps1, float *part, int32_t B,
                               long *nchunk, hipStream_t st);

// k_lif_step_slab (dcll_step_slab.hip): one MFMA layer step of a plain conv layer of any number of output channels (kernel up to
// 16x16) in bands of rows and slabs of 64 channels.  _forwards: the call is dcll_conv_lif_step_wide's (c_out <= 64, bands == 0,
// served there) and never reaches the rest; _plan: DCLL_OK with the bands and slabs of a call (bands == 0: the rule) or the
// refusal with its message; _wprep: w_scratch in the kernel's order (128 floats per chain step and slab); the launcher with
// launch == false only prepares (checks, LDS reservation).  The caller runs k_trace in front of the layer kernel
__attribute__((visibility("hidden"))) bool dcll_step_slab_forwards(const dcll_conv_desc *d, int32_t bands);
__attribute__((visibility("hidden")))
int dcll_step_slab_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int *nb, int *ns, const char *who);
__attribute__((visibility("hidden"))) int dcll_launch_step_slab_wprep(const dcll_conv_desc *d, const float *W, float *wperm, hipStream_t st);
__attribute__((visibility("hidden")))
int dcll_launch_step_slab(const dcll_conv_desc *d, const float *wperm, const float *b, const float *eps1, float *arp,
                          float *out_s, float *out_pv, float *out_v, int nb, int ns, int32_t B, hipStream_t st, bool launch);

// k_lif_step_w3 (dcll_step_w3.hip): one MFMA layer step of the layers dcll_seq_w3_geometry() serves.  _check: DCLL_OK or the
// refusal with its message; _tiles: tiles per workgroup (8 or 4) for (descriptor, B); the launcher with launch == false only
// prepares (checks, LDS reservation): called before the first launch of the entry point
__attribute__((visibility("hidden"))) int dcll_step_w3_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden"))) int dcll_step_w3_tiles(const dcll_conv_desc *d, int32_t B);
__attribute__((visibility("hidden")))
int dcll_launch_step_w3(const dcll_conv_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                        const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                        float *out_s, float *out_pv, float *out_v, int nt, int32_t B, hipStream_t st, bool launch);

// k_bwd_wgrad_w3 (dcll_step_w3.hip): MFMA weight gradient of the 64 -> 64 layers of that geometry.  _check: DCLL_OK or the
// refusal; the launcher caps *nchunk (partial rows there is room for) and returns it; launch == false: checks and the LDS
// reservation only
__attribute__((visibility("hidden"))) int dcll_bwd_w3_check(const dcll_conv_desc *d, const char *who);
__attribute__((visibility("hidden")))
int dcll_launch_bwd_wgrad_w3(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B,
                             long *nchunk, hipStream_t st, bool launch);

// k_bwd_wgrad_w3f (dcll_step_w3.hip): streaming weight gradient of the first (c_in 1) layer of that geometry; the launcher
// caps *nchunk and returns it; launch == false: the checks only
__attribute__((visibility("hidden")))
int dcll_launch_bwd_wgrad_w3f(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B,
                              long *nchunk, hipStream_t st, bool launch);

// k_bwd_dv_w3 (dcll_step_w3.hip): the dv plane of a layer of that geometry, a streaming form of k_bwd_dv for its (1,2) pooling.
// Launches and sets *form to the kernel's name for the launch log; *form == nullptr: not served (target > 32), nothing launched
__attribute__((visibility("hidden")))
int dcll_launch_bwd_dv_w3(const dcll_conv_desc *d, const float *v, const float *g_p, const float *g_pv, const float *g_v,
                          const float *i2o_W, float *gvf, int32_t B, hipStream_t st, const char **form);

// k_bwd_dv_pool (dcll_bwd_dv_pool.hip): the dv plane of a layer that pools (pool sizes 1 .. 3, not both 1), a streaming form of
// k_bwd_dv: a thread owns a pooled window.  Launches and sets *form to the kernel's name for the launch log; *form == nullptr: not
// served (dcll_bwd_dv_pool_served is the predicate), nothing launched
__attribute__((visibility("hidden")))
int dcll_launch_bwd_dv_pool(const dcll_conv_desc *d, const float *v, const float *g_p, const float *g_pv, const float *g_v,
                            const float *i2o_W, float *gvf, int32_t B, hipStream_t st, const char **form);

// dense twins (dcll_dense.hip): one step as an fp32-MFMA GEMM on the updated traces; all T steps with the state on chip
__attribute__((visibility("hidden")))
int dcll_launch_dense_mfma(const dcll_dense_desc *d, const float *eps1, const float *W, const float *b, float *arp,
                           float *out_s, float *out_pv, float *out_v, int32_t B, hipStream_t st);
__attribute__((visibility("hidden"))) bool dcll_dense_seq_fits(const dcll_dense_desc *d);
__attribute__((visibility("hidden")))
int dcll_launch_dense_seq(const dcll_dense_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                          const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                          float *out_s, float *out_pv, float *out_v, int32_t T, int32_t B, hipStream_t st);

// k_readout_direct (dcll_readout.hip): LDS-free 16x16x4 readout GEMM in <= 64 VGPRs (fits beside a sequence kernel)
__attribute__((visibility("hidden")))
int dcll_launch_readout_direct(const float *pv, const float *Wt, const float *bias, float *out, long rows, int K, int N,
                               hipStream_t st);

// k_readout_t16 (dcll_readout.hip): LDS-staged 16x16x4 readout GEMM, 128 rows x 16 NT readout rows per workgroup
__attribute__((visibility("hidden")))
int dcll_launch_readout_t16(const float *pv, const float *Wt, const float *bias, float *out, long rows, int K, int N,
                            int kslice, hipStream_t st, int act = DCLL_ACT_NONE);

// the split-K passes of several per-step readouts in one launch (k_readout_t16m)
__attribute__((visibility("hidden")))
int dcll_launch_readout_t16_multi(const float *const *pv, const float *const *Wt, float *const *out, const long *rows,
                                  const int *K, const int *N, const int *kslice, int n, hipStream_t st);

// ------------------------------------------------------------------------------------------------------------
// shared device helpers
// ------------------------------------------------------------------------------------------------------------
// pv = 1/(1+exp(-v)): v_exp_f32 + v_rcp_f32 (each ~1 ulp); pv is not bit-pinned (include/dcll_hip.h), |err| ~1e-7.
__device__ __forceinline__ float sigmoidf_dev(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

// dcll/pytorch_libdcll.py:493-494 — (x*tau_s) + (alphas*eps0) ; (alpha*eps1) + (eps0'*tau_m); every op rounded.
__device__ __forceinline__ void trace_update(float x, float alpha, float tau_m, float alphas, float tau_s,
                                             float &e0, float &e1)
{
    float a = x * tau_s;
    float b = alphas * e0;
    e0 = a + b;
    float c = alpha * e1;
    float d = e0 * tau_m;
    e1 = c + d;
}

// :497-503 — returns v, updates arp, sets s.
__device__ __forceinline__ float refractory(float pvmem, float &arp, float alpharp, float wrp, bool &s)
{
    float a = alpharp * arp;
    float v = pvmem + a;
    s = v > 0.0f;
    float sw = s ? wrp : 0.0f;      // s*wrp, exact
    arp = a - sw;
    return v;
}

// The weight of a link that is no link of the pinned chain (the partner of an odd last channel or tap, a K tile's tail): -0, on a
// trace operand that is +0 or a trace (>= +0).  The product is then -0, and acc + (-0) == acc for EVERY acc, -0 included — a
// weight of +0 made the product +0 and turned a membrane of -0 into +0 where the oracle, which has no such link, keeps -0
// (tests/test_gpu_values.py: a bias of -0 under weights of -0).
constexpr float DCLL_PAD_W = -0.0f;

// (v > 0 ? 1.0f : 0.0f) on a register pair in TWO packed instructions: clamp(clamp(v * 2^127) * 2^127), clamp = the VOP3P
// clamp to [0, 1].  Exact for every fp32 value a membrane can take — a positive denormal reaches 2^-22 after the first
// multiplication and 1 after the second (fp32 denormals are on in this build), zeros and negatives clamp to +0
// (tests/test_gpu_values.py: the threshold cases put v on +-0, +-2^-149, +-2^-127 ... +-2^126 in every kernel that uses this, and
// tests/test_value_cases.py shows that ONE clamp would change arp there; experiments/pk_clamp_probe.hip checks every class of
// value on the instruction alone).  Replaces 2 v_cmp + 2 v_cndmask in the refractory
// update s * wrp of the epilogues that share their vector pipe with fp32 MFMAs.
__device__ __forceinline__ f32x2 spike01_pk(f32x2 v)
{
    const f32x2 big = {0x1p127f, 0x1p127f};          // (an SGPR pair: the kernels that use this have no vector register to spare)
    f32x2 r;
    asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(v), "s"(big));
    asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(r), "s"(big));
    return r;
}

// Buffer-store addressing for the epilogues of the sequence kernels: a 128-bit descriptor (base = a wave-uniform pointer, in
// SGPRs) + 32-bit scalar or immediate offset + 32-bit lane byte offset — no 64-bit address per store and no address
// register pairs to keep (or spill) across the time loop.  Offsets must stay below 2^31.
__device__ __forceinline__ long uniform_long(long x)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)x), hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long)x >> 32));
    return (long)(((unsigned long)hi << 32) | lo);
}
__device__ __forceinline__ auto tile_rsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)uniform_long((long)base), 0, 0x7fffffff, 0x00020000);
}

// compile-time loop: f(std::integral_constant<int, R0>{}), ..., f(std::integral_constant<int, R1 - 1>{})
template <int R0, int R1, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (R0 < R1) {
        f(std::integral_constant<int, R0>{});
        static_for<R0 + 1, R1>(f);
    }
}

// (k_lif_seq_any, k_bwd_wgrad_any, k_lif_step_any: geometry at run time) n / d for 0 <= n, d < 65536 as one multiply: M = ceil(2^32 / d) is exact while n * d < 2^32
struct any_div {
    uint32_t M;
    int d;
};
__host__ __device__ static inline any_div make_div(int d) { return any_div{d > 1 ? (uint32_t)(((1ull << 32) + d - 1) / d) : 0u, d}; }
__device__ __forceinline__ int fdiv(int n, const any_div &q) { return q.d == 1 ? n : (int)__umulhi((uint32_t)n, q.M); }

// A 32-bit LDS address the compiler cannot fold into static offsets (after `asm volatile("" : "+v"(p))`): reads through it are
// base + immediate, where a visible static offset beyond the instruction's range makes the compiler rebuild a base per read.
typedef __attribute__((address_space(3))) const float lds_cfloat;

// Workgroup barrier that orders LDS traffic only: waits for this wave's outstanding LDS (and scalar) operations, then
// s_barrier — without the s_waitcnt vmcnt(0) that __syncthreads() adds for its global-memory fence, so a wave does not
// stall on its own pv / spike stores.  The builtin keeps the barrier convergent for the compiler.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// one DPP step of a wave-wide sum: v + (v moved by CTRL); lanes without a source add 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
// sum over the 64 lanes; the total is valid in lane 63
__device__ __forceinline__ float wave_sum_to_lane63(float v)
{
    v = dpp_add<0xB1, 0xF>(v);       // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xF>(v);       // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xF>(v);      // row_half_mirror
    v = dpp_add<0x140, 0xF>(v);      // row_mirror      -> every lane holds its 16-lane row sum
    v = dpp_add<0x142, 0xA>(v);      // row_bcast15     -> rows 1,3 += previous row
    v = dpp_add<0x143, 0xC>(v);      // row_bcast31     -> rows 2,3 += row 1
    return v;
}

