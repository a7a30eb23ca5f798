/*
 * dcll_hip.h — C ABI of libdcll_hip.so: the MI355X (gfx950) replacement for the per-timestep DCLL layer
 * forward of ohjay/snn-modulation-classification.
 *
 * The reference exposes a Python object protocol, not an FFI; the seam this ABI replaces is
 *     o, p, pv, pvmem = self.dclllayer.forward(input)          dcll/pytorch_libdcll.py:657
 * i.e. Conv2dDCLLlayer.forward (:599-608) -> ContinuousConv2D.forward (:407-426) /
 * ContinuousRelativeRefractoryConv2D.forward (:485-509), and DenseDCLLlayer.forward (:250-255) ->
 * CLLDenseModule.forward (:131-148) / CLLDenseRRPModule.forward (:171-195), plus the per-step vote collection of
 * DCLLClassification.forward (:722-729) and the T-loop of test_radio_ml.py:144-145.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch types. All pointers are DEVICE pointers (HBM) unless marked host.
 *   - every buffer is allocated and owned by the caller (PyTorch-ROCm tensors); the library never allocates
 *     persistent device memory and never frees anything.
 *   - tensors are contiguous fp32, NCHW, unless a packed layout is documented at the parameter.
 *   - calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream) and never
 *     synchronise internally; thread-safe for distinct (stream, state) pairs.
 *   - return value: DCLL_OK (0) or a negative DCLL_ERR_* code; never throws across the ABI.
 *     dcll_last_error() returns a thread-local, human-readable message for the last failing call.
 *   - arithmetic contract (bit-level, see DESIGN.md "Pinned arithmetic"):
 *       eps0' = x*tau_s + alphas*eps0         three separately rounded fp32 ops (no FMA contraction)
 *       eps1' = alpha*eps1 + eps0'*tau_m      idem
 *       pvmem[co,y,x] = fmaf-chain starting from bias[co], over k = (ci-pair cp, ky, kx, ci = 2cp+h), in that
 *                       nesting order, zero padding contributing fmaf(0, w, acc); one rounding per product
 *       arp' = alpharp*arp ; v = pvmem + arp' ; s = v > 0 ; arp'' = arp' - s*wrp     (refractory variant)
 *       pv = 1/(1+exp(-v)) (not bit-pinned) ; readouts p,o fp32 (not bit-pinned; |err| <= 1e-4)
 *     value domain (tests/test_gpu_values.py): fp32 subnormals are kept in state, operands and results — nothing flushes;
 *     s = v > 0 holds for every finite v, +-0 and subnormals included; pv is finite and inside [0, 1] for every finite v.
 *     NaN and Inf inputs are unspecified.
 */
#ifndef DCLL_HIP_H
#define DCLL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCLL_ABI_VERSION 10

enum {
    DCLL_OK = 0,
    DCLL_ERR_INVALID = -1,      /* bad descriptor / null pointer / size mismatch            */
    DCLL_ERR_UNSUPPORTED = -2,  /* legal in the reference but not implemented by this build */
    DCLL_ERR_LAUNCH = -3        /* HIP runtime reported an error (message has the string)   */
};

/* Geometry + constants of one Conv2dDCLLlayer (ctor: dcll/pytorch_libdcll.py:513-581). */
typedef struct dcll_conv_desc {
    int32_t c_in, c_out;        /* i2h.weight is (c_out, c_in, kh, kw)                                   */
    int32_t h, w;               /* input plane = im_dims                                                 */
    int32_t kh, kw;             /* kernel_size                                                           */
    int32_t pad_h, pad_w;       /* padding                                                               */
    int32_t stride, dilation, groups; /* F.conv2d's (:417, :495); ConvNetwork builds 1,1,1 (networks/__init__.py:132-145).
                                       * Other values (>= 1, groups dividing c_in and c_out; W is then (c_out, c_in/groups,
                                       * kh, kw), the chain runs over the group's channel pairs) are served by the per-step
                                       * calls dcll_conv_lif_step / dcll_conv_lif_backward[_open] on their generic kernels;
                                       * the sequence calls return DCLL_ERR_UNSUPPORTED for them.  The backward calls serve
                                       * kernels of up to 64 taps (kh * kw <= 64) whose padded input row fits the LDS-staged
                                       * weight gradient (about (w + 2 pad_w) * ((kh - 1) dilation + 1) <= 12 000 floats) and
                                       * return DCLL_ERR_UNSUPPORTED beyond — F.conv2d itself has no such limit.  (Plain convs
                                       * beyond those limits: dcll_conv_lif_backward_any, ABI 9, below.)                  */
    int32_t pool_h, pool_w;     /* MaxPool2d(kernel=stride=pool, padding=(pool-1)/2)   :542-549          */
    int32_t target;             /* target_size: rows of i2o.weight (and output_.weight)                  */
    int32_t output_layer;       /* !=0: also o = output_(flatten(pv))  :605-606                          */
    int32_t tau_is_tensor;      /* 0: alpha,tau_m,alphas,tau_s hold 1 float; 1: (c_in,h,w) floats :391-405 */
    int32_t refractory;         /* !=0: wrp > 0 variant (:485-509), arp state used                       */
    float alpharp;              /* :497                                                                  */
    float wrp;                  /* :503                                                                  */
} dcll_conv_desc;

/* Geometry + constants of one DenseDCLLlayer (ctor: dcll/pytorch_libdcll.py:199-242). */
typedef struct dcll_dense_desc {
    int32_t in_features, out_features;  /* i2h.weight is (out, in)                                       */
    int32_t target;                     /* i2o is Linear(out, target)                                    */
    int32_t tau_is_tensor;              /* 0: 1 float each; 1: (in_features) floats :119-129             */
    int32_t refractory;
    float alpharp, wrp;
} dcll_dense_desc;

/*
 * Optional per-call extras of the layer calls (ABI v3).  NULL = all defaults (fp32 weights, pv = sigmoid(v)).
 *
 *   w_q8 / w_scale   BASELINE config 5 ("int8 weights"; no reference code — the build's definition): when w_q8 != NULL the
 *                    conv weight is read as int8 (c_out,c_in,kh,kw) with one fp32 scale per OUTPUT channel, w_scale
 *                    (c_out), and the fp32 `W` argument of the call is ignored (may be NULL).  Every kernel converts a
 *                    weight exactly once, where it would have loaded the fp32 value: w = (float)q * w_scale[co] — ONE
 *                    rounded fp32 multiply — and then runs the pinned fmaf chain on it, so the results are bit-identical to
 *                    the same call on the dequantised fp32 tensor.  The weight-stationary sequence kernels convert in their
 *                    prologue (once per launch); the per-step kernels where they stage the weights (1 byte per weight
 *                    through L2 instead of 4).  Not accepted by dcll_conv_lif_backward (learning updates fp32 weights).
 *   pv_presigmoid    sequence calls only.  != 0: pv_out receives v = pvmem + arp' — what the threshold saw (:498-499),
 *                    max-pooled where the layer pools — INSTEAD of pv = sigmoid(v).  The sigmoid then runs in the consumer:
 *                    dcll_readout_act(..., DCLL_ACT_SIGMOID) applies it to every value it stages (the readout is HBM-bound
 *                    and has the vector slots; the layer kernels share their vector pipe with the fp32 MFMAs), and the pv
 *                    statistics (pv_lowhigh) are counted on sigmoid(v) as before.  sigmoid is monotone, so
 *                    max-pool(sigmoid(v)) == sigmoid(max-pool(v)) up to the last ulp of the (not bit-pinned) sigmoid.
 *                    Not combined with the fused readout (n_ro > 0).
 */
/*
 * Second threshold table of the IQ quantiser (dcll_iq_encode, dcll_conv_lif_sequence_iq; NULL = one table for all samples).
 * The reference quantises one time sample of the whole batch at a time with torch CPU ops (data/utils.py:60-79); torch's
 * float `pow` runs full groups of 16 / 32 batch positions through its vector implementation and the remaining positions
 * (batch size not a multiple of the group, chunk ends of its thread pool) through scalar libm, and the two differ in the
 * last ulp at some cell boundaries — so which cell a boundary value lands in depends on the sample's POSITION in the batch.
 * thr_*_tail are the thresholds of the scalar path, tail_mask[b] != 0 marks the samples the reference would have sent
 * through it (the host derives all three from torch itself, data/utils.py IQEncoder): device cells == reference cells for
 * every batch size.
 */
typedef struct dcll_iq_tail {
    const float *thr_i_tail;    /* (w-1) */
    const float *thr_q_tail;    /* (h-1) */
    const uint8_t *tail_mask;   /* (B)   */
} dcll_iq_tail;

typedef struct dcll_layer_opts {
    const int8_t *w_q8;         /* int8 conv weights (c_out,c_in,kh,kw), or NULL: the call's fp32 W is used */
    const float *w_scale;       /* (c_out) fp32, required with w_q8                                          */
    int32_t pv_presigmoid;      /* sequence calls: pv_out = v (pooled by max) instead of sigmoid(v)          */
    int32_t reserved;           /* must be 0                                                                 */
} dcll_layer_opts;

int dcll_version(void);                 /* DCLL_ABI_VERSION of the loaded library                        */
const char *dcll_last_error(void);      /* thread-local message of the last failing call ("" if none)    */

/*
 * Which kernels did a call dispatch?  (ABI 5; diagnostics, host-side only.)  The reference has one code path per layer
 * (F.conv2d, dcll/pytorch_libdcll.py:417,495); this library picks a kernel by geometry and batch, and a parity test is
 * only worth its name if it ran the kernel it claims to cover.  dcll_kernel_trace(1) clears the calling thread's log
 * and starts recording one line per kernel launch of that thread's calls; dcll_kernel_trace(0) stops.
 * dcll_kernel_trace_read copies the log (newline-separated kernel names, NUL-terminated, truncated to cap) and returns
 * the bytes needed for all of it; the log itself stops growing at 64 KiB (last line "...").
 */
int dcll_kernel_trace(int32_t enable);
int64_t dcll_kernel_trace_read(char *buf, int64_t cap);

/* Output spatial sizes of the conv and of the pooled map (get_output_shape :368-375, :593-597). */
int dcll_conv_out_shape(const dcll_conv_desc *d, int32_t *conv_h, int32_t *conv_w, int32_t *pool_h, int32_t *pool_w);

/*
 * One timestep of Conv2dDCLLlayer.forward — exact drop-in for dcll/pytorch_libdcll.py:599-608.
 *   x        (B,c_in,h,w)   input spikes (any fp32 values are accepted, the reference does not check)
 *   W,b      i2h.weight (c_out,c_in/groups,kh,kw), i2h.bias (c_out) — b may be NULL (bias=False, :323-326: the chains start at 0)
 *   alpha,tau_m,alphas,tau_s   i2h.alpha, i2h.tau_m__dt, i2h.alphas, i2h.tau_s__dt
 *   eps0,eps1 (B,c_in,h,w)  neuron state, updated IN PLACE          arp (B,c_out,ch,cw) idem (may be NULL if !refractory)
 *   i2o_W (target, c_out*ph*pw), i2o_b (target)        out_W,out_b: output_ layer, NULL unless output_layer
 *   out_s  (B,c_out,ph,pw) pooled spikes          out_p (B,target) local readout      out_o (B,target) or NULL
 *   out_pv (B,c_out,ph,pw) pooled sigmoid         out_v (B,c_out,ch,cw) = pvmem (+arp) before pooling, may be NULL
 *   scratch 2*B*c_out*ch*cw floats, required iff pooling != 1 (un-pooled spikes and sigmoid), else may be NULL
 *   i2o_W / out_p may be NULL to skip the local readout (then the call is ContinuousConv2D.forward + pool).
 *   opts     NULL, or int8 weights (dcll_layer_opts; pv_presigmoid must be 0 here: the drop-in returns pv).
 */
int dcll_conv_lif_step(const dcll_conv_desc *d, const float *x, const float *W, const float *b,
                       const float *alpha, const float *tau_m, const float *alphas, const float *tau_s,
                       float *eps0, float *eps1, float *arp,
                       const float *i2o_W, const float *i2o_b, const float *out_W, const float *out_b,
                       float *out_s, float *out_p, float *out_o, float *out_pv, float *out_v, float *scratch,
                       const dcll_layer_opts *opts, int32_t B, void *stream);

/*
 * Backward of one Conv2dDCLLlayer step for local learning — what loss.backward() reaches in DCLLBase.train_dcll
 * (dcll/pytorch_libdcll.py:690-704).  Call after dcll_conv_lif_step of the same step, before the next one.
 *   eps1 (B,c_in,h,w) state after the step ; v = out_v of the step ; pv_pooled = out_pv of the step.  v may be NULL for a
 *   layer WITHOUT pooling and target <= 32 whose pv_pooled is given: sigmoid'(v) = pv (1 - pv) is then taken from the stored pv —
 *   the bits the kernel would recompute from v (what torch's sigmoid backward does, too) — and the step need not write out_v
 *   incoming gradients (each may be NULL): g_p (B,target) of pvoutput, g_o (B,target) of the output_ logits,
 *   g_pv (B,c_out,ph,pw) of pv, g_v (B,c_out,ch,cw) of pvmem
 *   results: dW (c_out,c_in/groups,kh,kw), db (c_out) [may be NULL]; d_outW (target, c_out*ph*pw), d_outb (target) iff g_o
 *   scratch: scratch_floats >= B*c_out*ch*cw + k*c_out*((c_in/groups)*kh*kw + 1) floats with k >= 1 batch chunks for the weight
 *   gradient's partial sums (more chunks = more parallelism; up to 256 are used).  An output_ layer with target <= 32 whose
 *   K = c_out*ph*pw is not a multiple of 32 sums its gradient over min(B, 16, m) batch chunks of target*(K+1) floats, m = what
 *   fits into the partial-sum area (closed form: the area is reused) or behind the rows in use (dcll_conv_lif_backward_open):
 *   with room for min(B, 16) chunks in either place both forms give the same bits.
 *   i2o is frozen, neuron state detached, output_ sees pv.detach() (:570,:504,:606).
 */
int dcll_conv_lif_backward(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                           const float *g_p, const float *g_o, const float *g_pv, const float *g_v,
                           const float *i2o_W, float *dW, float *db, float *d_outW, float *d_outb,
                           float *scratch, int64_t scratch_floats, int32_t B, void *stream);

/*
 * The rest of a local-learning step (DCLLBase.train_dcll :690-718) around dcll_conv_lif_step / dcll_conv_lif_backward, so
 * that the per-timestep loop needs no torch op:
 *
 * dcll_local_loss_grad — gradient and value of the local losses with mean reduction (what loss.backward() hands to the
 *   readouts): loss = crit(p, target) [+ crit(o, target) when o != NULL], g_p = d loss / d p, g_o = d loss / d o.
 *   p, o, target, g_p, g_o (B,N) fp32; loss: 1 float, may be NULL; clout (B) int32, may be NULL: the per-sample argmax of
 *   o (of p when o == NULL) that DCLLClassification.forward records (:724-728).  kind: DCLL_LOSS_SMOOTH_L1 (torch.nn.SmoothL1Loss,
 *   beta 1 — train.py's default --loss_type) or DCLL_LOSS_MSE (torch.nn.MSELoss).
 *
 * dcll_adam_step — torch.optim.Adam's update (amsgrad False; L2 weight decay added to the gradient; bias correction by
 *   `step`) over up to DCLL_ADAM_MAX_TENSORS parameter tensors — of one or of several optimizers — in one launch.  train.py
 *   (:164-168) builds the optimizers with betas (0, beta) and weight_decay 10; exp_avg / exp_avg_sq are the optimizer's
 *   own state tensors, so optimizer.state_dict() stays what torch would have produced.  `tensors` is a HOST array.
 *
 * dcll_cells_to_planes — iq2spiketrain's dense spike planes (data/utils.py:81-82) from cell indices on the device:
 *   planes (n_samples, hw) fp32 = one-hot of cells (n_samples) int32; hw % 4 == 0.
 */
enum { DCLL_LOSS_SMOOTH_L1 = 0, DCLL_LOSS_MSE = 1 };
int dcll_local_loss_grad(const float *p, const float *o, const float *target, float *g_p, float *g_o, float *loss,
                         int32_t *clout, int32_t B, int32_t N, int32_t kind, void *stream);

#define DCLL_ADAM_MAX_TENSORS 8
typedef struct dcll_adam_tensor {
    float *param;               /* updated in place                                                       */
    const float *grad;
    float *exp_avg, *exp_avg_sq; /* optimizer state, updated in place                                     */
    int64_t n;                  /* elements                                                               */
    int64_t step;               /* 1-based count of this update (bias correction)                         */
    float lr, weight_decay, beta1, beta2, eps;  /* of the tensor's param group (the slices' optimizers differ: */
                                /* optimizer2 of the output layer runs torch's default betas, :637-638)  */
} dcll_adam_tensor;
int dcll_adam_step(const dcll_adam_tensor *tensors, int32_t n_tensors, void *stream);
/* The same update with the quantities that change from step to step read from DEVICE memory at execution time: dyn
 * (n_tensors x 3 floats) = per tensor (lr, 1 / (1 - beta1^step), 1 / sqrt(1 - beta2^step)); `lr` and `step` of the structs
 * are ignored.  This is the form a captured hipGraph of a learning timestep replays (the host refreshes `dyn` with a
 * stream-ordered copy before each replay). */
int dcll_adam_step_dyn(const dcll_adam_tensor *tensors, int32_t n_tensors, const float *dyn, void *stream);

/*
 * The end of a learning timestep in one launch (ABI 5).  dcll_conv_lif_backward_open is dcll_conv_lif_backward with the last
 * step of the weight gradient left open: the partial rows stay in `scratch` — *part points at *nchunk rows of
 * c_out * ((c_in/groups)*kh*kw + 1) floats, valid until the next call that uses this scratch — and dW / db are not written.
 * dcll_grad_reduce_adam then finishes up to DCLL_REDUCE_MAX_LAYERS layers at once: the rows are added in dcll_conv_lif_backward's
 * own fixed order (bit-identical gradients), written to dW / db, and the Adam update of `tensors[adam_w]` / `tensors[adam_b]`
 * (index, or -1: no update) is applied by the thread that holds the finished gradient element; the tensors no layer refers
 * to get dcll_adam_step's elementwise update in the same launch.  dyn: NULL, or as dcll_adam_step_dyn (n_tensors x 3).
 * Replaces, per timestep of train_dcll (:690-718), one reduce launch per layer + the optimizer launch.
 */
#define DCLL_REDUCE_MAX_LAYERS 4
typedef struct dcll_grad_parts {
    const float *part;          /* nchunk partial rows (dcll_conv_lif_backward_open)                       */
    float *dW, *db;             /* (c_out, (c_in/groups)*kh*kw) and (c_out): the reduced gradients; db may be NULL */
    int64_t rowlen;             /* (c_in/groups)*kh*kw + 1                                                 */
    int32_t nchunk, c_out;
    int32_t adam_w, adam_b;     /* entries of `tensors` to update with dW / db, or -1                      */
} dcll_grad_parts;
int dcll_conv_lif_backward_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                const float *g_p, const float *g_o, const float *g_pv, const float *g_v,
                                const float *i2o_W, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                                int32_t B, const float **part, int32_t *nchunk, void *stream);
int dcll_grad_reduce_adam(const dcll_grad_parts *layers, int32_t n_layers, const dcll_adam_tensor *tensors,
                          int32_t n_tensors, const float *dyn, void *stream);

/*
 * dcll_optim_step / dcll_grad_reduce_optim — dcll_adam_step / dcll_grad_reduce_adam with the update chosen per tensor by `kind`:
 * torch.optim.Adam, AdamW, Adamax and SGD (torch 2.10's _single_tensor_* functions; maximize False), kinds mixed freely in one
 * launch.  fp32, every operation rounded separately, division and sqrtf correctly rounded.  g = grad + weight_decay * p for the
 * coupled kinds (ADAM, ADAMAX, SGD), g = grad for ADAMW.
 *   ADAM    s0 = exp_avg, s1 = exp_avg_sq, with DCLL_OPT_AMSGRAD s2 = max_exp_avg_sq.  Without the flag: dcll_adam_step's
 *           update, the same bits.  With it: s2 = max(s2, v) and the denominator is sqrt(s2) / sqrt(bc2) + eps.
 *   ADAMW   as ADAM, after p = p * c, c = (float)(1 - lr * weight_decay) (host, float64 on the struct's floats).
 *   ADAMAX  s0 = exp_avg, s1 = exp_inf: m = lerp(m, g, 1 - beta1); u = max(u * beta2, |g| + eps); p -= (lr / bc1) * (m / u).
 *   SGD     s0 = momentum_buffer (NULL when momentum is 0): buf = DCLL_OPT_FIRST ? g : buf * momentum + (1 - dampening) * g;
 *           g' = DCLL_OPT_NESTEROV ? g + momentum * buf : buf (without momentum g' = g); p -= lr * g'.
 *           DCLL_OPT_FIRST: the caller's mark of the update that creates the buffer (buf = g bit for bit, no product with the buffer's old content).
 * h0 / h1: beta1 / beta2 (ADAM, ADAMW, ADAMAX), momentum / dampening (SGD).  max(a, b) is torch.maximum's: a NaN wins.
 * dyn: NULL, or DEVICE memory, DCLL_OPTIM_DYN floats per tensor, read at execution time (the form a captured timestep replays;
 * `lr` and `step` of the structs are then ignored): (lr, 1 / bc1, 1 / sqrt(bc2), c) for ADAM / ADAMW (c unused by ADAM),
 * (lr, 1 / bc1, 0, 0) for ADAMAX, (lr, (float)(1 - dampening), 0, 0) for SGD — the values the host computes without dyn
 * (float64 on the struct's floats, cast once).
 * dcll_grad_reduce_optim: `layers` as dcll_grad_reduce_adam (adam_w / adam_b index `t`), the same partial-row grouping and
 * order: dW / db are its bits.  Launch log: "k_optim_multi" / "k_grad_reduce_optim".
 * DCLL_ERR_INVALID before any launch: a state pointer the kind needs is NULL, unknown kind or flag bits (NESTEROV / FIRST on
 * a kind other than SGD or without momentum, AMSGRAD on ADAMAX / SGD included), step < 1, n < 0, more than
 * DCLL_OPTIM_MAX_TENSORS tensors or DCLL_REDUCE_MAX_LAYERS layers, a tensor referred to by two layers, sizes that do not match
 * c_out * (rowlen - 1) / c_out.
 */
enum { DCLL_OPT_ADAM = 0, DCLL_OPT_ADAMW = 1, DCLL_OPT_ADAMAX = 2, DCLL_OPT_SGD = 3 };
enum { DCLL_OPT_AMSGRAD = 1, DCLL_OPT_NESTEROV = 2, DCLL_OPT_FIRST = 4 };
#define DCLL_OPTIM_MAX_TENSORS 8
#define DCLL_OPTIM_DYN 4      /* floats per tensor in `dyn` */
typedef struct dcll_optim_tensor {
    float *param; const float *grad;
    float *s0, *s1, *s2;      /* state by kind, above; unused ones NULL */
    int64_t n, step;
    int32_t kind, flags;
    float lr, weight_decay, h0, h1, eps;
} dcll_optim_tensor;
int dcll_optim_step(const dcll_optim_tensor *t, int32_t n, const float *dyn, void *stream);
int dcll_grad_reduce_optim(const dcll_grad_parts *layers, int32_t n_layers,
                           const dcll_optim_tensor *t, int32_t n, const float *dyn, void *stream);

/*
 * dcll_conv_lif_backward_open for SEVERAL layers — the slices of one learning timestep — in one call (ABI 6): where all of
 * them are layers without pooling with the same readout-width class their dv launches (max-pool routing / i2o^T / sigmoid')
 * run as ONE launch, then the weight / output_ gradient kernels layer by layer.  Each field is the argument of that name of
 * dcll_conv_lif_backward_open; `part` / `nchunk` are written (its outputs).  Per item the results are those of the single
 * call, bit for bit.  1 <= n <= 8, reserved must be 0.
 */
typedef struct dcll_bwd_item {
    const dcll_conv_desc *d;
    const float *eps1, *v, *pv_pooled, *g_p, *g_o, *g_pv, *g_v, *i2o_W;
    float *d_outW, *d_outb, *scratch;
    int64_t scratch_floats;
    int32_t B, reserved;
    const float *part;          /* out */
    int32_t nchunk, reserved2;  /* out; 0 */
} dcll_bwd_item;
int dcll_conv_lif_backward_open_multi(dcll_bwd_item *items, int32_t n, void *stream);

int dcll_cells_to_planes(const int32_t *cells, float *planes, int64_t n_samples, int32_t hw, void *stream);

/* One timestep of DenseDCLLlayer.forward — drop-in for dcll/pytorch_libdcll.py:250-255 (dropout = identity). */
int dcll_dense_lif_step(const dcll_dense_desc *d, const float *x, const float *W, const float *b,
                        const float *alpha, const float *tau_m, const float *alphas, const float *tau_s,
                        float *eps0, float *eps1, float *arp, const float *i2o_W, const float *i2o_b,
                        float *out_s, float *out_p, float *out_pv, float *out_v, int32_t B, void *stream);

/*
 * Backward of one DenseDCLLlayer step for local learning (ABI 7) — DCLLBase.train_dcll (:690-718) is layer-agnostic: it builds
 * the optimizer from dclllayer.i2h.parameters() (:634-635) and DenseDCLLlayer.forward keeps pvoutput in the graph (:250-255).
 *   dv = (g_p . i2o_W + g_pv) * pv * (1 - pv) + g_v ;  dW (out,in) = dv^T . eps1 ;  db (out) = sum_b dv
 * eps1 (B,in): the layer's eps1 state AFTER the step; pv (B,out) = sigmoid(v) as the step returned it; g_p (B,target), g_pv,
 * g_v (B,out): gradients of the loss w.r.t. pvoutput / pv / pvmem, each may be NULL (g_p needs i2o_W (target,out)).
 * scratch: scratch_floats >= B*out + k*out*(in+1), k >= 1 batch chunks (up to 64 are used).  The _open form leaves the last
 * reduction to dcll_grad_reduce_adam (rowlen = in + 1, c_out = out): *part / *nchunk as dcll_conv_lif_backward_open.
 * Sums run in a fixed order (an fp32-MFMA GEMM over sample pairs per chunk, chunks ascending): deterministic, and the closed
 * form is the open form + dcll_grad_reduce_adam without tensors — the same bits.
 */
int dcll_dense_lif_backward(const dcll_dense_desc *d, const float *eps1, const float *pv, const float *g_p,
                            const float *g_pv, const float *g_v, const float *i2o_W, float *dW, float *db,
                            float *scratch, int64_t scratch_floats, int32_t B, void *stream);
int dcll_dense_lif_backward_open(const dcll_dense_desc *d, const float *eps1, const float *pv, const float *g_p,
                                 const float *g_pv, const float *g_v, const float *i2o_W, float *scratch,
                                 int64_t scratch_floats, int32_t B, const float **part, int32_t *nchunk, void *stream);

/*
 * All T timesteps of a DenseDCLLlayer in one call — `for t: layer.forward(x[t])` (:250-255) — the dense twin of
 * dcll_conv_lif_sequence.  x (T,B,in) fp32; neuron state in/out as in dcll_dense_lif_step (read at t = 0, written after
 * t = T-1); out_s, out_pv, out_v (T,B,out), out_p (T,B,target), each may be NULL (out_p needs out_pv).
 * in_features <= 1024 and out_features <= 128: ONE launch with the state on chip for all T (32 samples per workgroup, eps0
 * in registers, eps1 in LDS, W streamed from L2); larger layers advance step by step inside the call with the state in
 * HBM.  The local readout runs once over all T x B rows.  Same pinned chain as the per-step call: bit-identical v / s / state.
 */
int dcll_dense_lif_sequence(const dcll_dense_desc *d, const float *x, const float *W, const float *b,
                            const float *alpha, const float *tau_m, const float *alphas, const float *tau_s,
                            float *eps0, float *eps1, float *arp, const float *i2o_W, const float *i2o_b,
                            float *out_s, float *out_p, float *out_pv, float *out_v, int32_t T, int32_t B, void *stream);

/*
 * Whole-sequence fast path behind ConvNetwork.test (networks/__init__.py:182-185) for one layer: all T timesteps
 * of dcll/pytorch_libdcll.py:485-509 / :407-426 in ONE launch with the neuron state held on-chip.
 * Supported geometry (else DCLL_ERR_UNSUPPORTED): c_in==32, c_out==32, 7x7, pad 3, pool 1, time constants constant
 * over (h,w) per input channel (what randomize_tau produces, :391-405), on the 16x16 plane of the reference's scripts
 * (one sample per workgroup) or on any plane with h % 8 == 0 and w % 32 == 0 — e.g. the 128x128 default of
 * test_radio_ml.py:52 — (one workgroup per 8x32 tile; no fused readout there).
 * Also served: the layers of networks/radio_ml_conv_ref.yaml — c_in==64 (first layer: dcll_conv_lif_sequence_cells, c_in==1),
 * c_out==64, kernel (1,3), padding (0,1), pooling (1,2), w a power of two <= 256, h*w % 32 == 0 (k_lif_seq_w3; the first
 * layer, k_lif_seq_w3f: h*w % 128 == 0, state and output pointers 8-byte aligned).  For this
 * POOLING geometry the outputs are the pooled maps: spk_out (T,B,64,h*(w/2)/32) [needs h*w % 64 == 0], pv_out
 * (T,B,64,h,w/2); v_out stays un-pooled (T,B,64,h,w); state_scratch is not used.
 *   spk_in   (T,B,c_in,h*w/32) uint32   packed input spikes: bit (y*w+x)%32 of word (y*w+x)/32
 *   tau4     (4,c_in) fp32              rows: alpha, tau_m, alphas, tau_s per input channel
 *   eps0,eps1,arp                       neuron state in/out as in dcll_conv_lif_step (read at t=0, written after t=T-1)
 *   spk_out  (T,B,c_out,h*w/32) uint32  packed output spikes (same layout, feeds the next layer); may be NULL
 *   pv_out   (T,B,c_out,h,w) fp32       sigmoid(v) for the readout GEMM; may be NULL
 *   v_out    (T,B,c_out,h,w) fp32       debugging / parity only; may be NULL
 *   fused local readout (n_ro = 24 or 48; 0 = none): ro_out (T,B,n_ro) = flatten(pv) . Wro^T + ro_b, i.e. i2o and,
 *   stacked behind it on the output layer, output_ (:602-606), computed in the epilogue so that pv never leaves the
 *   chip.  ro_Wp = the (n_ro, c_out*h*w) weight matrix re-laid-out by dcll_permute_readout; ro_b (n_ro).
 *   state_scratch  2*B*c_in*h*w floats, REQUIRED on planes other than 16x16 (may be NULL on 16x16): the tiled kernels
 *                  read a tile's initial traces plus a halo owned by neighbouring tiles, so the launch first snapshots
 *                  eps0 / eps1 there (stream-ordered copies), reads only the snapshot and writes only eps0 / eps1.
 *   pv_lowhigh     NULL = off.  Else uint64 [n][2], n = dcll_pv_lowhigh_steps(iter0, T): for every step t of this call
 *                  with (iter0 + t + 1) % 20 == 0 — DCLLBase.forward's histogram steps, :658-661 — the number of pv
 *                  values in the first and in the last of the 19 bins of np.linspace(0, 1, 20) (what write_stats
 *                  reports, :678-688).  iter0 = the slice's iteration count before the call.  Needs pv_out.
 *   opts           NULL, or int8 weights / pv_presigmoid (dcll_layer_opts above).
 */
int dcll_conv_lif_sequence(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                           const float *tau4, float *eps0, float *eps1, float *arp,
                           uint32_t *spk_out, float *pv_out, float *v_out,
                           const float *ro_Wp, const float *ro_b, float *ro_out, int32_t n_ro,
                           float *state_scratch, uint64_t *pv_lowhigh, int32_t iter0,
                           const dcll_layer_opts *opts, int32_t T, int32_t B, void *stream);

/* Re-lay-out a readout matrix Wt (N, 32*16*16) [n][co][pix] for the fused epilogue of dcll_conv_lif_sequence:
 * Wp[me][wq][n][lane][rr] with co = rr + 8*wq + 4*(lane>>5), pix = 32*me + (lane&31).  Wp has N*8192 floats. */
int dcll_permute_readout(const float *Wt, float *Wp, int32_t N, void *stream);

/*
 * First-layer sequence kernel (c_in==1): the input is exactly one spike per sample per step (iq2spiketrain,
 * data/utils.py:43-87), given as its cell index q*w+i.  Geometry: c_in==1, c_out<=32, 7x7, pad 3, pool 1, plane 16x16
 * or h % 8 == 0 and w % 32 == 0.
 *   cells (T,B) int32 ; tau4 (4,1) ; other arguments as dcll_conv_lif_sequence (state_scratch: 2*B*h*w floats).
 */
int dcll_conv_lif_sequence_cells(const dcll_conv_desc *d, const int32_t *cells, const float *W, const float *b,
                                 const float *tau4, float *eps0, float *eps1, float *arp,
                                 uint32_t *spk_out, float *pv_out, float *v_out,
                                 float *state_scratch, uint64_t *pv_lowhigh, int32_t iter0,
                                 const dcll_layer_opts *opts, int32_t T, int32_t B, void *stream);

/*
 * Same kernel with iq2spiketrain's quantisation (data/utils.py:60-82) fused in: the input is the raw IQ window
 * iq (B,2,L) fp32, samples t0..t0+T-1, quantised with the thresholds of dcll_iq_encode (thr_i: w-1 floats, thr_q:
 * h-1 floats).  T <= 4096.
 */
int dcll_conv_lif_sequence_iq(const dcll_conv_desc *d, const float *iq, const float *thr_i, const float *thr_q,
                              const dcll_iq_tail *tail, int32_t L, int32_t t0, const float *W, const float *b, const float *tau4,
                              float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out, float *v_out,
                              float *state_scratch, uint64_t *pv_lowhigh, int32_t iter0,
                              const dcll_layer_opts *opts, int32_t T, int32_t B, void *stream);

/*
 * The pv statistics of DCLLBase.forward (:658-661) as a call of its own (the per-step path uses it with T = 1):
 * pv (T, per_step) fp32 = the pv outputs of T consecutive steps, per_step = B*c_out*ph*pw values each; counts as
 * pv_lowhigh above, uint64 [dcll_pv_lowhigh_steps(iter0, T)][2].  Steps that are not histogram steps are not read.
 */
int dcll_pv_lowhigh(const float *pv, int64_t per_step, int32_t T, int32_t iter0, uint64_t *counts, void *stream);
/* The same counters for a buffer written with pv_presigmoid (act = DCLL_ACT_SIGMOID: sigmoid(v) is what is counted). */
enum { DCLL_ACT_NONE = 0, DCLL_ACT_SIGMOID = 1 };
int dcll_pv_lowhigh_act(const float *pv, int64_t per_step, int32_t T, int32_t iter0, uint64_t *counts, int32_t act,
                        void *stream);
int32_t dcll_pv_lowhigh_steps(int32_t iter0, int32_t T);    /* (iter0 + T) / 20 - iter0 / 20 */

/*
 * Local readout for many rows at once: out[r, n] = sum_k pv[r,k]*Wt[n,k] + bias[n]   (i2o / output_, :602-606),
 * fp32 MFMA.  rows = T*B, K = c_out*ph*pw, N = rows of Wt (e.g. i2o and output_ stacked: 48).
 */
int dcll_readout(const float *pv, const float *Wt, const float *bias, float *out,
                 int64_t rows, int32_t K, int32_t N, void *stream);
/*
 * The readout of the whole-sequence path (rows = T x a chunk of the batch), optionally on a pv_presigmoid buffer:
 *     out[r, n] = sum_k act(pv[r,k])*Wt[n,k] + bias[n]
 * act = DCLL_ACT_SIGMOID applies the layer kernels' sigmoid (v_exp_f32 + v_rcp_f32) to every staged value: the logits equal
 * those of the pv = sigmoid(v) form up to the readout's summation order.  Always the LDS-staged 16x16x4 kernel: whole for
 * K < 65536, in 8 ... 64 K-slices of >= 8192 columns (partials in caller scratch, summed in slice order) for longer rows —
 * chosen by K alone, so
 * a row's logits do not depend on the row count, i.e. on how the caller chunks a batch (dcll_readout / dcll_readout_splitk
 * choose by row count: they serve the per-step calls).  Needs K % 32 == 0 (K % 256 == 0 when split), K < 2^22 (32-bit
 * offsets inside a workgroup's 128 rows), N <= 64, 16-byte aligned pv / Wt — else DCLL_ERR_UNSUPPORTED (the caller keeps pv = sigmoid(v) and dcll_readout for such shapes);
 * scratch_floats >= dcll_readout_act_scratch(rows, K, N) (0: scratch may be NULL).
 */
int64_t dcll_readout_act_scratch(int64_t rows, int32_t K, int32_t N);
int dcll_readout_act(const float *pv, const float *Wt, const float *bias, float *out, float *scratch,
                     int64_t scratch_floats, int64_t rows, int32_t K, int32_t N, int32_t act, void *stream);

/*
 * The same readout with the kernel form chosen by the caller:
 *   DCLL_READOUT_AUTO        what dcll_readout does;
 *   DCLL_READOUT_CORESIDENT  the LDS-free, <= 64-VGPR form of the 16x16x4 kernel (K % 64 == 0, K <= 16384, N <= 48,
 *                            16-byte aligned rows; other shapes fall back to AUTO): a workgroup of it fits on a CU beside a
 *                            resident sequence-kernel workgroup, so a readout launched on a second stream runs in the gaps
 *                            of the next layer's kernel instead of after it;
 *   DCLL_READOUT_LDS         the LDS-staged 32x32x2 kernels only (measurements);
 *   DCLL_READOUT_T16         the LDS-staged 16x16x4 kernel (K % 32 == 0, N <= 64, aligned rows; else AUTO).
 * Logits of different modes differ by summation order only (within the 1e-4 contract).
 */
enum { DCLL_READOUT_AUTO = 0, DCLL_READOUT_CORESIDENT = 1, DCLL_READOUT_LDS = 2, DCLL_READOUT_T16 = 3 };
int dcll_readout_mode(const float *pv, const float *Wt, const float *bias, float *out,
                      int64_t rows, int32_t K, int32_t N, int32_t mode, void *stream);

/*
 * The same readout for FEW rows (per-step calls: rows = batch): K is split into slices over the workgroups, the partial
 * tiles go to caller-provided scratch and are added in slice order (deterministic).  Served, with N <= 64 and 16-byte
 * aligned pv / Wt: K >= 65536, K % 4096 == 0 (large planes, K = c_out*128*128: slices of 4096 for rows <= 2048, else 8
 * slices — any row count), or rows <= 2048 with
 * 2048 <= K < 65536, K % 256 == 0 (the 16x16 plane, K = 8192: slices of 256 — of 128 for rows <= 512 and N <= 32);
 * scratch_floats >= dcll_readout_splitk_scratch(rows, K, N) (0 = this shape is not supported, use dcll_readout).
 */
int64_t dcll_readout_splitk_scratch(int64_t rows, int32_t K, int32_t N);
int dcll_readout_splitk(const float *pv, const float *Wt, const float *bias, float *out, float *scratch,
                        int64_t scratch_floats, int64_t rows, int32_t K, int32_t N, void *stream);

/*
 * ABI 4 — the readouts of ONE layer step and everything behind them in two launches (per-step calls: rows = batch):
 *   Conv2dDCLLlayer.forward :602-606     p = i2o(flatten(pv)) and, on the output layer, o = output_(flatten(pv)): ONE
 *                                        split-K pass over pv against the N1 + N2 STACKED rows Wt / bias (N2 = 0 or N1);
 *   DCLLClassification.forward :724-728  clout (rows) int32 = argmax of o (of p when N2 == 0), first maximum; NULL = off;
 *   DCLLBase.train_dcll :692-704         target != NULL: g_p, g_o = gradients of the mean local losses of kind `kind`
 *                                        (dcll_local_loss_grad without the loss value; NULL = inference step).
 * p (rows, N1) and o (rows, N2) come out as separate contiguous arrays; per column bit-identical to a dcll_readout_splitk call
 * that splits K into slices of the same width (the slice width follows rows and N1 + N2: for rows <= 512 a call with
 * N1 <= 32 < N1 + N2 here uses 256-column slices where a call on the N1 columns alone would use 128).
 * Shapes: rows <= 2048, 2048 <= K < 65536, K % 256 == 0, N1 + N2 <= 64, 16-byte aligned pv / Wt — else
 * DCLL_ERR_UNSUPPORTED (callers fall back to dcll_readout + dcll_argmax_vote / dcll_local_loss_grad);
 * scratch_floats >= dcll_step_readouts_scratch(rows, K, N1, N2).
 */
int64_t dcll_step_readouts_scratch(int64_t rows, int32_t K, int32_t N1, int32_t N2);
int dcll_step_readouts(const float *pv, const float *Wt, const float *bias, float *scratch, int64_t scratch_floats,
                       int64_t rows, int32_t K, int32_t N1, int32_t N2, float *p, float *o, int32_t *clout,
                       const float *target, float *g_p, float *g_o, int32_t kind, void *stream);

/*
 * The readout tails of SEVERAL layer steps — the slices of one network timestep (ConvNetwork.test / .learn,
 * networks/__init__.py:175-185: slice l+1 consumes slice l's spikes, nobody's readouts) — in TWO launches instead of two per
 * layer (ABI 6): one split-K pass over all items' pv, one finishing launch.  Each field is the argument of that name of
 * dcll_step_readouts; per item the results are those of dcll_step_readouts, bit for bit.  1 <= n <= 8; every item must be one
 * dcll_step_readouts serves, with rows >= 1 and a scratch area of its own; either every item has a target (learning step) or
 * none.  reserved must be 0.
 */
typedef struct dcll_step_ro {
    const float *pv, *Wt, *bias;
    float *scratch;
    int64_t scratch_floats, rows;
    int32_t K, N1, N2, kind;
    float *p, *o;
    int32_t *clout;
    const float *target;
    float *g_p, *g_o;
    int64_t reserved;
} dcll_step_ro;
int dcll_step_readouts_multi(const dcll_step_ro *items, int32_t n, void *stream);

/*
 * Per-step argmax + vote (DCLLClassification.forward :724-728, get_predictions_by_vote :44-56):
 *   logits (T,B,N) -> clout (T,B) int32 (first maximum wins, like torch.argmax) and, if vote != NULL,
 *   vote (B) int32 = mode over t in [t_begin,T) of clout, ties broken by first occurrence in time.
 */
int dcll_argmax_vote(const float *logits, int32_t *clout, int32_t *vote, int32_t T, int32_t B, int32_t N,
                     int32_t t_begin, void *stream);

/*
 * The per-class tallies of an evaluated batch (accuracy_by_vote / confusion_matrix, dcll/pytorch_libdcll.py:44-61, :740-749, in
 * the summable form the ranks all-reduce): out (n_layers, n_classes*n_classes + 2) int64 = per layer the confusion matrix
 * [pred][label] flattened, the number of votes equal to their label, the number of votes.  votes: HOST array of n_layers
 * device pointers to (B) int32 votes (dcll_argmax_vote); labels (B) int64.  Every element of `out` is written.
 */
int dcll_vote_tallies(const int32_t *const *votes, int32_t n_layers, const int64_t *labels, int64_t *out, int32_t B,
                      int32_t n_classes, void *stream);

/*
 * iq2spiketrain on device (data/utils.py:60-82) as a threshold search: cell = #{j : x >= thr[j]} for the
 * monotone map x -> int(clamp(gamma(x),0,1)*(R-1)); thr_i (w-1) and thr_q (h-1) are produced on the host from
 * the host encoder so that the result is bit-identical to it.
 *   iq (B,2,L) fp32 ; cells (T,B) int32 = q*w + i for samples t0..t0+T-1
 */
int dcll_iq_encode(const float *iq, const float *thr_i, const float *thr_q, const dcll_iq_tail *tail, int32_t *cells,
                   int32_t B, int32_t L, int32_t t0, int32_t T, int32_t w, int32_t h, void *stream);

/* Unpack (T*B, C, HW/32) packed spikes to fp32 (T*B, C, HW) and back — glue for the tensor-level API. */
int dcll_unpack_spikes(const uint32_t *packed, float *dense, int64_t nwords, void *stream);
int dcll_pack_spikes(const float *dense, uint32_t *packed, int64_t nwords, void *stream);

/*
 * ABI 8 — all T timesteps of ANY plain conv layer in one launch (k_lif_seq_any, one workgroup per sample, the neuron state in
 * LDS): the fused path of the layers the geometry-specialised calls above refuse — networks/mnist_conv.yaml (28x28, 7x7, pad 2,
 * pooling 2 / 1 / 2, 16 / 24 / 32 channels), radio_ml_conv.yaml on planes such as 24x24 or 12x32.  Additions only: the calls
 * above, their refusals and their kernels are unchanged.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in; c_out <= 32; kh, kw <= 16;
 * any padding (the conv plane may shrink or grow); any pooling >= 1 (MaxPool2d(kernel = stride = pool, padding (pool-1)/2),
 * floor mode); time constants constant over (h, w) per input channel; and a per-sample state that one workgroup holds on chip:
 *   LDS form       4 bytes x (c_in (h + 2 pad_h)(w + 2 pad_w) [zero-padded eps1] + c_in h w [eps0] + c_out ch cw [v of one step]
 *                  + c_out ch cw [arp, refractory layers only] + 4 c_in + 32) <= 160 KiB, the LDS of a workgroup; or, beyond that,
 *   register form  layers WITHOUT pooling with c_in h w <= 18432 and ch cw <= 768 (radio_ml_conv.yaml's 32 -> 32 layers on 24x24
 *                  or 12x32): eps0 and arp live in registers, LDS holds 4 bytes x (c_in (h + 2 pad_h)(w + 2 pad_w) + 4 c_in + 32).
 * dcll_conv_lif_sequence_any_lds returns the LDS bytes of the form that serves the layer (the weights the kernel keeps behind
 * them where there is room are not counted), or 0 for a descriptor that is not served (invalid ones included).
 * Spike planes cross this call as ceil(hw / 32) words per (t, b, channel) plane: bit pix % 32 of word pix / 32, tail bits zero
 * (identical to the format above whenever hw % 32 == 0); dcll_pack_spike_planes / dcll_unpack_spike_planes convert n_planes
 * dense fp32 planes of hw values (non-zero = spike) to and from it.
 *   spk_in   (T,B,c_in,ceil(h*w/32)) uint32      tau4 (4,c_in) as above      b (c_out), or NULL: the chains start at 0
 *   eps0,eps1 (B,c_in,h,w), arp (B,c_out,ch,cw)  neuron state in/out (read at t = 0, written after t = T-1); arp may be NULL
 *                                                 for a layer that is not refractory
 *   spk_out  (T,B,c_out,ceil(ph*pw/32)) uint32   POOLED spikes = pooled v > 0; may be NULL
 *   pv_out   (T,B,c_out,ph,pw)                   sigmoid(pooled v); may be NULL
 *   v_out    (T,B,c_out,ch,cw)                   un-pooled v = pvmem (+ arp'), for tests; may be NULL
 *   w_scratch  dcll_conv_lif_sequence_any_scratch(d) floats: the weights in MFMA fragment order, written by a small kernel in
 *              front of the layer kernel on every call (the caller may reuse it once the call's work has run)
 * Arithmetic: the contract at the top of this file — every v is ONE fmaf chain from b[co] over (cp, ky, kx, h) on
 * v_mfma_f32_32x32x2_f32, two consecutive links per instruction; the unpaired last channel of an odd c_in runs its taps two by
 * two, and a chain of odd length ends with fmaf(0, 0, acc) (== acc, except that -0.0 becomes +0.0).  v, the spikes and the
 * final state are bit-identical to T calls of dcll_conv_lif_step; pv to the sigmoid's last ulp.
 * T == 0 or B == 0: DCLL_OK, nothing is looked at.  fp32 weights only (no dcll_layer_opts here).
 */
int64_t dcll_conv_lif_sequence_any_lds(const dcll_conv_desc *d);
int64_t dcll_conv_lif_sequence_any_scratch(const dcll_conv_desc *d);
int dcll_conv_lif_sequence_any(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                               const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                               float *v_out, float *w_scratch, int32_t T, int32_t B, void *stream);
int dcll_pack_spike_planes(const float *dense, uint32_t *packed, int64_t n_planes, int32_t hw, void *stream);
int dcll_unpack_spike_planes(const uint32_t *packed, float *dense, int64_t n_planes, int32_t hw, void *stream);

/*
 * Still ABI 10 (three more symbols, found by lookup) — dcll_conv_lif_sequence_any for layers of up to 64 output channels
 * (k_lif_seq_wide): the fused all-T path of the networks a --netscale above 1 makes (radio_ml_conv.yaml at netscale 2 on 16x16:
 * 1 -> 64, 64 -> 64; mnist_conv.yaml at netscale 2: 32 / 48 / 64 channels).  Arguments, buffer formats, arithmetic and results
 * are dcll_conv_lif_sequence_any's.  Additions only: the calls above, their refusals and their kernels are unchanged.
 * MT = ceil(c_out / 32) tiles of 32 MFMA rows:
 *   MT = 1  the call is handed to dcll_conv_lif_sequence_any unchanged (its kernels, launch-log names, bits, _lds and _scratch)
 *   MT = 2  k_lif_seq_wide: a wave runs both 32-row chains of a pixel tile, interleaved, each the pinned chain, unsplit.
 *     LDS form       4 bytes x (c_in (h + 2 pad_h)(w + 2 pad_w) + c_in h w + c_out ch cw + c_out ch cw [arp, refractory layers
 *                    only] + 4 c_in + 64) <= 160 KiB; or, beyond that,
 *     register form  layers WITHOUT pooling with c_in h w <= 18432 and ch cw <= 256: LDS holds 4 bytes x (c_in (h + 2 pad_h)
 *                    (w + 2 pad_w) + 4 c_in + 64) <= 160 KiB.
 *     w_scratch      dcll_conv_lif_sequence_wide_scratch(d) = 128 floats per MFMA step of a chain, written by k_seq_wide_wprep
 *                    in front of the layer kernel on every call.
 * DCLL_ERR_UNSUPPORTED, before any launch: c_out > 64, stride / dilation / groups other than 1, a kernel beyond 16x16, a working
 * set beyond both forms.  DCLL_ERR_INVALID, before any launch: a NULL required pointer, a refractory layer without arp, T < 0 or
 * B < 0.  T == 0 or B == 0: DCLL_OK, nothing is looked at.  _lds: LDS bytes of the form that serves the layer, 0 = refused.
 */
int64_t dcll_conv_lif_sequence_wide_lds(const dcll_conv_desc *d);
int64_t dcll_conv_lif_sequence_wide_scratch(const dcll_conv_desc *d);
int dcll_conv_lif_sequence_wide(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                                float *v_out, float *w_scratch, int32_t T, int32_t B, void *stream);

/*
 * Still ABI 10 (four more symbols, found by lookup) — dcll_conv_lif_sequence_wide with SEVERAL workgroups per sample
 * (k_lif_seq_band): a sample is cut into `bands` bands of output rows, each band sits on its own workgroup for all T and
 * recomputes the input traces of the halo rows it needs; nothing passes between workgroups during the sequence.  For small batches
 * (one workgroup per sample leaves CUs idle) and for layers whose per-sample state is beyond one workgroup's 160 KiB of LDS
 * (radio_ml_conv.yaml on 48x48).  Arguments, buffer formats, arithmetic and results are dcll_conv_lif_sequence_wide's: every v is
 * ONE unsplit chain in the pinned order, so v, pv, spikes and the final state are bit-identical to it wherever it serves the layer.
 * Additions only: the calls above, their refusals and their kernels are unchanged.
 *   bands     0: the library's rule — the smallest count that fits, raised while B x bands <= 256 (one round of the card) and
 *             not beyond the count at which more bands stop paying: one band when the one-workgroup kernel already runs one chain
 *             per wave (MT ceil(tiles / 8) == 1), several bands down to one 32-pixel tile per band; n >= 1: exactly n.
 *             bands == 1 (asked for or chosen): the call is handed to dcll_conv_lif_sequence_wide unchanged (its kernels,
 *             launch-log names, bits; its permuted weights are the scratch's prefix).
 *   plan      band k of NB owns pooled rows [k ph / NB, (k + 1) ph / NB) (floor); its conv rows [C0, C1) are the union of those
 *             pooling windows clipped to [0, ch), the last band's run up to ch; it holds input rows [C0 - pad_h, C1 - pad_h + kh - 1)
 *             clipped to the image and writes the final eps0 / eps1 of rows [its first held row, the next band's first held row).
 *   LDS       of a band, 4 bytes x (c_in (C1 - C0 + kh - 1)(w + 2 pad_w) + c_in (held rows) w + c_out (C1 - C0) cw + the same
 *             again [arp, refractory layers only] + 4 c_in + 32 MT), MT = ceil(c_out / 32); the largest band's <= 160 KiB.
 *   scratch   dcll_conv_lif_sequence_bands_scratch(d, B) floats = 64 MT per MFMA step of a chain (the permuted weights) +
 *             2 B c_in h w: a stream-ordered copy of eps0 / eps1 in front of the launch, which every band's initial read goes to
 *             (a late band of a grid beyond residency must not read a neighbour's final state as its halo).
 *   spk_out   a band stores the words wholly inside its pooled-pixel range and ORs its bits into a word it shares with a
 *             neighbour (atomicOr); when the plan has such a word, spk_out is zero-filled on the stream first.
 * _plan: the band count the call would run (0 = refused); bounds, when not NULL, receives its bands + 1 pooled-row bounds.
 * _lds: LDS bytes of the largest band (bands == 0: at the rule's count for B = 1; 1: dcll_conv_lif_sequence_wide_lds), 0 =
 * refused.  _plan and _lds are host-only.  DCLL_ERR_UNSUPPORTED, before any launch: c_out > 64, stride / dilation / groups other
 * than 1, a kernel beyond 16x16, bands > ph, an explicit band count whose largest set does not fit, no band count that fits.
 * DCLL_ERR_INVALID, before any launch: bands < 0, a NULL required pointer, a refractory layer without arp, T < 0 or B < 0.
 * T == 0 or B == 0: DCLL_OK, nothing is looked at.  Launch log: k_lif_seq_band<MT,R,WLDS> (M tiles, refractory, all weights in
 * LDS); the weight permutation, the snapshot and the zero fill stay out of it.
 */
int32_t dcll_conv_lif_sequence_bands_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int32_t *bounds);
int64_t dcll_conv_lif_sequence_bands_lds(const dcll_conv_desc *d, int32_t bands);
int64_t dcll_conv_lif_sequence_bands_scratch(const dcll_conv_desc *d, int32_t B);
int dcll_conv_lif_sequence_bands(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                 const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                                 float *v_out, float *scratch, int32_t T, int32_t B, int32_t bands, void *stream);

/*
 * Still ABI 10 (four more symbols, found by lookup) — dcll_conv_lif_sequence_bands cut in BOTH directions (k_lif_seq_tile): a
 * sample is cut into tiles_y x tiles_x tiles, each tile sits on its own workgroup for all T and recomputes the input traces of the
 * halo rows and columns it needs; nothing passes between workgroups during the sequence.  For the layers no band count serves:
 * a band spans full rows, so its LDS set grows with c_in kh (w + 2 pad_w) (radio_ml_conv.yaml at netscale 2 on any plane much wider
 * than 16 pixels, at netscale 1 on 100x100).  Arguments, buffer formats, arithmetic and results are dcll_conv_lif_sequence_bands':
 * every v is ONE unsplit chain in the pinned order, so v, pv, spikes and the final state are bit-identical to it wherever it serves
 * the layer.  Additions only: the calls above, their refusals and their kernels are unchanged.
 *   tiles     tiles_x == 1 (with any tiles_y, 0 included): the call is handed to dcll_conv_lif_sequence_bands unchanged with
 *             bands = tiles_y (its kernels, launch-log names, bits, refusals; its scratch is this one's).
 *             (0, 0): the library's rule — the plan of dcll_conv_lif_sequence_bands_plan(d, B, 0) where that serves the layer;
 *             otherwise the fitting (NY, NX), NX >= 2, with the fewest tiles, ties to the smallest sum of held input elements over
 *             all tiles, then to the smaller NX.  This rule is derived from the LDS formula alone: no measurement stands behind it.
 *             tiles_y >= 1, tiles_x >= 2: exactly that plan.  A 0 in one place only: DCLL_ERR_INVALID.
 *   plan      tile (a, b) of NY x NX takes its rows from the band plan above at (a, NY) and its columns from the same plan applied
 *             to (b, NX, w, kw, pad_w, pool_w, cw, pw): owned pooled pixels, conv pixels (a partition; the floor-mode leftovers go
 *             to the last tile of each direction), held input pixels, owned input pixels.  Every element of arp, v_out, pv_out,
 *             every spike bit and every final eps0 / eps1 has exactly one owner.
 *   LDS       of a tile of CR x CC conv pixels that holds HR x HC input pixels, 4 bytes x (c_in (CR + kh - 1)(CC + kw - 1) +
 *             c_in HR HC + c_out CR CC + the same again [arp, refractory layers only] + 4 c_in + 32 MT), MT = ceil(c_out / 32); the
 *             largest tile's <= 160 KiB.  Behind it as many permuted weight steps as fit, by dcll_conv_lif_sequence_bands' rule
 *             (half of the LDS where B NY NX > 256 and the weights do not fit as a whole).  eps0 is kept in LDS.
 *   scratch   dcll_conv_lif_sequence_tiles_scratch(d, B) floats = dcll_conv_lif_sequence_bands_scratch's formula: 64 MT per MFMA
 *             step of a chain + 2 B c_in h w, the stream-ordered snapshot of eps0 / eps1 every tile's initial read goes to.
 *   spk_out   a tile's pooled pixels are row segments of the flattened pooled plane.  A word wholly inside one segment is stored;
 *             every other word is ORed into (atomicOr); when the plan has such a word, spk_out is zero-filled on the stream first.
 *             Tail bits stay zero.
 * _plan: the tile count NY NX the call would run (0 = refused); ny_nx, when not NULL, receives (NY, NX), bounds_y / bounds_x their
 * NY + 1 pooled-row / NX + 1 pooled-column bounds.  _lds: LDS bytes of the largest tile ((0, 0): at the rule's plan for B = 1;
 * tiles_x == 1: dcll_conv_lif_sequence_bands_lds(d, tiles_y)), 0 = refused.  _plan, _lds and _scratch are host-only.
 * DCLL_ERR_UNSUPPORTED, before any launch: c_out > 64, stride / dilation / groups other than 1, a kernel beyond 16x16,
 * tiles_y > ph or tiles_x > pw, an explicit plan whose largest set does not fit, no plan that fits.  DCLL_ERR_INVALID, before any
 * launch: a negative count, a 0 in one place only, a NULL required pointer, a refractory layer without arp, T < 0 or B < 0,
 * B NY NX beyond the grid.  T == 0 or B == 0: DCLL_OK, nothing is looked at.  Launch log: k_lif_seq_tile<MT,R,WLDS> (M tiles,
 * refractory, all weights in LDS); the weight permutation, the snapshot and the zero fill stay out of it.
 */
int32_t dcll_conv_lif_sequence_tiles_plan(const dcll_conv_desc *d, int32_t B, int32_t tiles_y, int32_t tiles_x, int32_t *ny_nx,
                                          int32_t *bounds_y, int32_t *bounds_x);
int64_t dcll_conv_lif_sequence_tiles_lds(const dcll_conv_desc *d, int32_t tiles_y, int32_t tiles_x);
int64_t dcll_conv_lif_sequence_tiles_scratch(const dcll_conv_desc *d, int32_t B);
int dcll_conv_lif_sequence_tiles(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                 const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                                 float *v_out, float *scratch, int32_t T, int32_t B, int32_t tiles_y, int32_t tiles_x,
                                 void *stream);

/*
 * Still ABI 10 (four more symbols, found by lookup) — dcll_conv_lif_sequence_tiles for layers of MORE than 64 output channels
 * (k_lif_seq_slab, csrc/dcll_seq_slab.hip): the tile kernel with one more grid dimension, B x tiles_y x tiles_x x NS.  The slab rule:
 * NS = ceil(c_out / 64) <= 65 535; slab s owns the output channels [64 s, min(64 s + 64, c_out)); rows at or beyond c_out are never
 * stored.  Arguments, buffer formats and arithmetic are dcll_conv_lif_sequence_tiles'; every v is ONE unsplit chain in the pinned
 * order, so v, pv, spikes and the final state are bit-identical to dcll_conv_lif_sequence_tiles run on each 64-channel slice of the
 * layer (W, b, arp) with the same plan.  Additions only: the calls above, their refusals ("c_out <= 64") and kernels are unchanged.
 *   c_out <= 64   every one of the four calls IS its _tiles twin (kernels, launch-log names, bits, refusals, _lds / _scratch values).
 *   workgroup     (sample, tile, slab): holds the traces of ALL c_in channels of its tile, as a tile workgroup does, and vpl, arp,
 *                 bias and the weights kept in LDS for its slab only.  Every slab recomputes the tile's traces; slab 0 alone writes
 *                 eps0 / eps1 back; every slab writes its own arp, pv, v and spike planes (a spike word belongs to one channel; inside
 *                 a channel the tile call's store-or-OR rule stands).  A last slab of at most 32 channels runs one chain per pixel tile.
 *   tiles         (0, 0): the fitting (NY, NX) with the fewest tiles, from ONE tile up, ties to the smallest sum of held input elements,
 *                 then to the smaller NX — derived from the LDS formula alone, no measurement stands behind it.  Otherwise exactly
 *                 (tiles_y, tiles_x), 1 x 1 and N x 1 included: this kernel runs every plan itself.  A 0 in one place only:
 *                 DCLL_ERR_INVALID.  The plan of a tile is dcll_conv_lif_sequence_tiles'.
 *   LDS           dcll_conv_lif_sequence_tiles' formula with the slab's channel count, 64, in place of c_out (MT = 2): it does not
 *                 grow with c_out.  Behind it as many permuted weight steps (128 floats each) as fit, by the same rule with
 *                 B NY NX NS workgroups.
 *   scratch       dcll_conv_lif_sequence_slabs_scratch(d, B) floats = 64 ceil(c_out / 32) per MFMA step of a chain (the ONE weight
 *                 permutation of the whole layer; a slab reads its two columns) + 2 B c_in h w (the snapshot of eps0 / eps1).
 * _plan, _lds, _scratch: as the _tiles calls (host-only).  DCLL_ERR_UNSUPPORTED, before any launch: stride / dilation / groups other
 * than 1, a kernel beyond 16x16, more than 65 535 slabs, tiles_y > ph or tiles_x > pw, an explicit plan whose largest set does not
 * fit, no plan that fits.  DCLL_ERR_INVALID, before any launch: a negative count, a 0 in one place only, a NULL required pointer, a
 * refractory layer without arp, T < 0 or B < 0, B NY NX beyond the grid.  T == 0 or B == 0: DCLL_OK.  Launch log:
 * k_lif_seq_slab<R,WLDS> (refractory, all weights in LDS); the weight permutation, the snapshot and the zero fill stay out of it.
 */
int32_t dcll_conv_lif_sequence_slabs_plan(const dcll_conv_desc *d, int32_t B, int32_t tiles_y, int32_t tiles_x, int32_t *ny_nx,
                                          int32_t *bounds_y, int32_t *bounds_x);
int64_t dcll_conv_lif_sequence_slabs_lds(const dcll_conv_desc *d, int32_t tiles_y, int32_t tiles_x);
int64_t dcll_conv_lif_sequence_slabs_scratch(const dcll_conv_desc *d, int32_t B);
int dcll_conv_lif_sequence_slabs(const dcll_conv_desc *d, const uint32_t *spk_in, const float *W, const float *b,
                                 const float *tau4, float *eps0, float *eps1, float *arp, uint32_t *spk_out, float *pv_out,
                                 float *v_out, float *scratch, int32_t T, int32_t B, int32_t tiles_y, int32_t tiles_x,
                                 void *stream);

/*
 * ABI 9 — the backward of one layer step with the weight gradient of ANY plain conv layer on fp32-MFMA tiles (k_bwd_wgrad_any):
 * dcll_conv_lif_backward / dcll_conv_lif_backward_open with the same arguments, results and scratch rule (B c_out ch cw +
 * k (c_out (c_in kh kw + 1)) floats, k >= 1; less: DCLL_ERR_INVALID), for the layers whose weight gradient the calls above
 * compute on the generic VALU kernel or refuse (more than 64 taps, rows too wide).  Additions only: the calls above, their
 * kernels, launch logs and refusals are unchanged; dv, the fixed-order reduction and the output_ gradient are the same kernels.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in; c_out <= 32; kh, kw <= 16;
 * any padding, pooling and batch; and a smallest working set that fits the 160 KiB of LDS of a workgroup:
 *   4 bytes x (cg (h + 2 pad_h)(w + 2 pad_w) + 1 [zero-padded eps1 of the cg input channels that 32 consecutive weight columns
 *   touch] + c_out (ch (cw rounded up to even) | 1) [the sample's dv plane]).
 * dW[co][n] = sum_{b,pix} g[b,co,pix] E[b][n][pix], n = ci kh kw + tap, as a GEMM on v_mfma_f32_32x32x2_f32 (M = c_out padded to
 * 32, N = columns in tiles of 32, one MFMA per pixel pair of a row; an odd row's last pixel is paired with a zero).  A workgroup
 * owns up to 32 consecutive column tiles of one batch chunk — fewer where LDS or a small batch ask for it ("column split");
 * with fewer than five tiles its waves split the pixels and add their pieces in wave order ("pixel split").  The launch log
 * names the form, NQ = accumulator tiles per wave (1, 2, 4): "k_bwd_wgrad_any<NQ>", "k_bwd_wgrad_any<NQ> (column split)",
 * "k_bwd_wgrad_any<1> (pixel split)" or "k_bwd_wgrad_any<1> (column split, pixel split)".  A small batch lowers the tiles per
 * workgroup only to layouts that need no more LDS than the full launch.
 * At most 256 batch chunks (partial rows part[chunk][co][c_in kh kw + 1]); every sum has a fixed order: two runs give the same
 * bits, and _any_open + dcll_grad_reduce_adam gives _any's bits.  Not bit-identical to dcll_conv_lif_backward (another order).
 * dcll_conv_lif_backward_any_lds returns the LDS bytes per workgroup of a full launch (no launch uses more), or 0 for a
 * descriptor that is not served (invalid ones included).
 */
int64_t dcll_conv_lif_backward_any_lds(const dcll_conv_desc *d);
int dcll_conv_lif_backward_any(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                               const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                               float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                               int32_t B, void *stream);
int dcll_conv_lif_backward_any_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                    const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                    float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                    const float **part, int32_t *nchunk, void *stream);

/*
 * Added under ABI 10 (DCLL_ABI_VERSION is unchanged: a caller detects these three symbols by symbol lookup) — the calls above for
 * the layers of 33 .. 64 output channels that a --netscale above 1 makes (k_bwd_wgrad_wide, csrc/dcll_bwd_wide.hip): arguments,
 * results and scratch rule of dcll_conv_lif_backward_any / _any_open (scratch_floats >= B c_out ch cw + k (c_out (c_in kh kw + 1)),
 * k >= 1 partial rows, at most 256 are used; less: DCLL_ERR_INVALID).  Additions only: the default dispatch, the _any calls, their
 * launch logs and refusals (dcll_conv_lif_backward_any's "c_out <= 32" included) are unchanged; dv, the fixed-order reduction
 * and the output_ gradient are the same kernels.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in; c_out <= 64; kh, kw <= 16; any
 * padding, pooling and batch; and a smallest working set within the 160 KiB of LDS of a workgroup: the formula above, 4 bytes x
 * (cg (h + 2 pad_h)(w + 2 pad_w) + 1 + c_out (ch (cw rounded up to even) | 1)).
 * c_out <= 32: the call IS dcll_conv_lif_backward_any[_open] — same kernels, launch log, bits, refusals (with that call's name
 * in the message) and _lds value — so a network of mixed widths goes through one entry point.
 * c_out 33 .. 64: k_bwd_wgrad_any's decomposition with M = c_out padded to 64 rows, two 32-row tiles: a wave runs both M tiles
 * of its column tiles, one LDS read of the B operand feeding two MFMAs (rows at or beyond c_out read the last real row and are
 * not stored).  Column split, pixel split (its pieces added in wave order), the 256-chunk limit, the odd-cw rule and the
 * small-batch lowering (never more LDS than the full launch) are those of the _any call.  The launch log names the form, NQ =
 * column tiles per wave (1, 2, 4; 2 NQ accumulator tiles): "k_bwd_wgrad_wide<NQ>", "k_bwd_wgrad_wide<NQ> (column split)",
 * "k_bwd_wgrad_wide<1> (pixel split)" or "k_bwd_wgrad_wide<1> (column split, pixel split)".
 * Every sum has a fixed order: two runs give the same bits, and _wide_open + dcll_grad_reduce_adam gives _wide's bits.  Not
 * bit-identical to dcll_conv_lif_backward (another order).
 * dcll_conv_lif_backward_wide_lds returns the LDS bytes per workgroup of a full launch (no launch uses more; c_out <= 32:
 * dcll_conv_lif_backward_any_lds), or 0 for a descriptor that is not served (invalid ones included).
 */
int64_t dcll_conv_lif_backward_wide_lds(const dcll_conv_desc *d);
int dcll_conv_lif_backward_wide(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                                int32_t B, void *stream);
int dcll_conv_lif_backward_wide_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                     const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                     float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                     const float **part, int32_t *nchunk, void *stream);

/*
 * Added under ABI 10 (DCLL_ABI_VERSION is unchanged: a caller detects these three symbols by symbol lookup) — the calls above for
 * the layers of MORE than 64 output channels that a --netscale above 2 makes (k_bwd_wgrad_slab, csrc/dcll_bwd_slab.hip): arguments,
 * results and scratch rule of dcll_conv_lif_backward_wide / _wide_open (scratch_floats >= B c_out ch cw + k (c_out (c_in kh kw + 1)),
 * k >= 1 partial rows, at most 256 are used; less: DCLL_ERR_INVALID).  Additions only: the default dispatch, the _any and _wide
 * calls, their launch logs and refusals (dcll_conv_lif_backward_wide's "c_out <= 64" included) are unchanged; dv, the fixed-order
 * reduction and the output_ gradient are the same kernels (they take rows of any c_out).
 * The slab rule: NS = ceil(c_out / 64); slab s owns the output channels [64 s, min(64 s + 64, c_out)), two 32-row M tiles;
 * rows at or beyond c_out are never stored; NS <= 65 535 (the grid's third dimension, the only new bound).
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in; any c_out up to 64 x 65 535;
 * kh, kw <= 16; any padding, pooling and batch; and a smallest working set within the 160 KiB of LDS of a workgroup, which does
 * NOT grow with c_out: 4 bytes x (cg (h + 2 pad_h)(w + 2 pad_w) + 1 + min(c_out, 64) (ch (cw rounded up to even) | 1)).
 * c_out <= 64: the call IS dcll_conv_lif_backward_wide[_open] (c_out <= 32: _any[_open]) — same kernels, launch log, bits,
 * refusals (with that call's name in the message) and _lds value — so a network of mixed widths goes through one entry point.
 * c_out > 64: k_bwd_wgrad_wide's decomposition with blockIdx.z as the slab.  A workgroup stages only its slab's rows of the dv
 * plane and stores part[chunk][co][...] with the global co; the bias gradient of a slab comes from the workgroup with the first
 * column tiles of that slab.  Column split, pixel split (pieces added in wave order), the 256-chunk limit and the odd-cw rule are
 * unchanged; the small-batch lowering aims chunks x column splits x slabs at the CU count (never more LDS than the full launch).
 * The launch plan is a function of (descriptor, B) alone.  The launch log names the form, NQ = column tiles per wave (1, 2, 4):
 * "k_bwd_wgrad_slab<NQ>", "k_bwd_wgrad_slab<NQ> (column split)", "k_bwd_wgrad_slab<1> (pixel split)" or
 * "k_bwd_wgrad_slab<1> (column split, pixel split)".
 * Every sum has a fixed order: two runs give the same bits, and _slab_open + dcll_grad_reduce_adam gives _slab's bits.  A row of
 * dW is summed as k_bwd_wgrad_wide sums it under the same (TPW, PS, chunks).  Not bit-identical to dcll_conv_lif_backward.
 * dcll_conv_lif_backward_slab_lds returns the LDS bytes per workgroup of a full launch (no launch uses more; c_out <= 64:
 * dcll_conv_lif_backward_wide_lds), or 0 for a descriptor that is not served (invalid ones included).
 */
int64_t dcll_conv_lif_backward_slab_lds(const dcll_conv_desc *d);
int dcll_conv_lif_backward_slab(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                                int32_t B, void *stream);
int dcll_conv_lif_backward_slab_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                     const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                     float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                     const float **part, int32_t *nchunk, void *stream);

/*
 * Found by symbol lookup (DCLL_ABI_VERSION is unchanged) — the calls above for ANY plane height (k_bwd_wgrad_band,
 * csrc/dcll_bwd_band.hip): arguments, results and scratch rule of dcll_conv_lif_backward_slab / _slab_open plus `bands`.  Additions
 * only: the default dispatch, the _any, _wide and _slab calls, their launch logs and refusals are unchanged; dv, the fixed-order
 * reduction and the output_ gradient are the same kernels.
 * k_bwd_wgrad_any / _wide / _slab stage a whole sample in LDS and refuse a layer whose sample does not fit.  Here a sample is cut
 * into NB bands of RB conv-output rows: band k covers the rows [min(ch, k RB), min(ch, (k + 1) RB)).  A job is (sample b, band k),
 * job = b NB + k; workgroup (chunk, column split, slab) runs the jobs chunk, chunk + nchunk, ... in order, accumulates in registers
 * and stores part[chunk][co][c_in kh kw + 1] once; nchunk = min(B NB, 256, what the scratch holds).  Per job it stages the band's
 * rows of its slab's dv rows and the rb + kh - 1 padded input rows under them of its column tiles' channels:
 *   4 bytes x (cg (RB + kh - 1)(w + 2 pad_w) + 1 + min(c_out, 32 MT) ((RB (cw rounded up to even)) | 1)),  MT = c_out <= 32 ? 1 : 2
 * which does not grow with the plane height.  MT = 2: the slab rule of dcll_conv_lif_backward_slab (NS <= 65 535).
 * bands == 0: the library's rule.  Where dcll_conv_lif_backward_slab serves the layer the call IS that call — same kernels, launch
 *   log, bits, _lds value and refusals.  Otherwise: the largest TPW <= min(NT, 32) column tiles per workgroup at which a band of
 *   min(ch, kh) rows fits the 160 KiB (failing that at every TPW: at which ONE row fits), the largest RB that fits beside it, NB = ceil(ch / RB),
 *   RB = ceil(ch / NB); then the small-batch lowering of TPW over nchunk x NS workgroups, never beyond the full launch's LDS.
 * bands == 1: the _slab call itself, refused where that call refuses.
 * bands == N >= 2: exactly N bands of ceil(ch / N) rows (the last ones empty where (N - 1) ceil(ch / N) >= ch), TPW the largest
 *   that fits.
 * Refused before any launch (DCLL_ERR_UNSUPPORTED): non-plain convs, kernels beyond 16x16, bands > ch, bands < 0, a forced band that
 * does not fit, a layer of which not even a one-row band with one column tile fits, more than 65 535 slabs or column splits;
 * DCLL_ERR_INVALID: scratch_floats < B c_out ch cw + c_out (c_in kh kw + 1).
 * The launch log names the form: "k_bwd_wgrad_band<MT,NQ>[ (column split)][ (pixel split)]" (both: "(column split, pixel split)"),
 * NQ = column tiles per wave (1, 2, 4).  Every sum has a fixed order: two runs give the same bits, and _bands_open +
 * dcll_grad_reduce_adam gives _bands' bits.  Not bit-identical to the other backward calls.
 * dcll_conv_lif_backward_bands_lds: LDS bytes per workgroup of a full launch (no launch uses more), 0 where the layer is not served.
 * dcll_conv_lif_backward_bands_plan: host only, launches nothing; out = NB, RB, TPW, PS (pixel split), NQ, NS (slabs), column splits,
 * nchunk of a call with an unlimited scratch.  A call that IS the _slab call reports NB = 1, RB = ch, NS and min(B, 256) chunks,
 * and 0 for TPW, PS, NQ and the column splits (that call's own plan).  Returns DCLL_OK or the refusal's code.
 */
int64_t dcll_conv_lif_backward_bands_lds(const dcll_conv_desc *d, int32_t bands);
int dcll_conv_lif_backward_bands_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int32_t out[8]);
int dcll_conv_lif_backward_bands(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                 const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                 float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                                 int32_t B, int32_t bands, void *stream);
int dcll_conv_lif_backward_bands_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                      const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                      float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                      int32_t bands, const float **part, int32_t *nchunk, void *stream);

/*
 * ABI 10 — one layer step of ANY plain conv layer in one MFMA launch (k_lif_step_any): dcll_conv_lif_step with the same arguments
 * and results for the layers that call serves with k_trace + k_conv_lif[_tiled] + k_pool.  Additions only: dcll_conv_lif_step, its
 * dispatch, launch logs and refusals are unchanged.  Differences to dcll_conv_lif_step:
 *   scratch    gone: the pooling happens on chip
 *   w_scratch  new: dcll_conv_lif_step_any_scratch(d) floats — 64 per MFMA step of a chain, 64 (c_in / 2) kh kw + 64 (c_in odd ?
 *              (kh kw + 1) / 2 : 0); dcll_conv_lif_sequence_any_scratch(d) gives the same wherever THAT call serves the layer —: the weights in MFMA fragment order, written by k_seq_any_wprep in front of
 *              the layer kernel on EVERY call — there is no "already prepared" form, the learning step changes W behind it
 *   opts       none: fp32 weights only
 * As there: dense fp32 x of any values; b may be NULL; scalar or (c_in,h,w) time constants (tau_is_tensor); eps0 / eps1 / arp
 * updated in place; out_v may be NULL; p / o only when i2o_W && out_p / output_layer, through the same readout kernels;
 * B == 0: DCLL_OK, nothing is looked at.  Pointers need 4-byte alignment only.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in; c_out <= 32; kh, kw <= 16; any
 * padding, pooling and batch; and a working set within the 160 KiB of LDS of a workgroup:
 *   4 bytes x (c_in (h + 2 pad_h)(w + 2 pad_w) [zero-padded eps1 image] + (pooling != 1 ? c_out ch cw : 0) [v plane of the
 *   pooling pass] + 32 [bias]).
 * dcll_conv_lif_step_any_lds returns these bytes, dcll_conv_lif_step_any_scratch the floats of w_scratch; both 0 for a descriptor
 * that is not served (invalid ones included).
 * DCLL_ERR_INVALID, before any launch: a NULL required pointer (w_scratch included), a refractory layer without arp, an output
 * layer without out_W / out_o, B < 0.
 * Arithmetic: the contract at the top of this file and the rule of dcll_conv_lif_sequence_any — the traces are three separately
 * rounded operations each; every v is ONE fmaf chain from b[co] over (cp, ky, kx, h) on v_mfma_f32_32x32x2_f32, two consecutive
 * links per instruction; the unpaired last channel of an odd c_in runs its taps two by two; a chain of odd length ends with
 * fmaf(0, 0, acc).  v equals dcll_conv_lif_step bit for bit up to the sign of a zero; spikes, eps0, eps1 and arp bit for bit; pv
 * within the sigmoid's 1e-4.  Pooled outputs: max over the window of v, spike = pooled v > 0, pv = sigmoid(pooled v).
 * Forms (the launch log names them; R = refractory; k_seq_any_wprep in front of each):
 *   "k_lif_step_any<R>"                      one workgroup per sample: traces, chains and epilogue in one launch
 *   "k_lif_step_any<R> (pooling)"            the same with the v plane and the pooling pass in LDS
 *   "k_trace", "k_lif_step_any<R> (split)"   NS > 1 workgroups per sample for a layer without pooling, NS = min(ceil(tiles / 8),
 *                                            256 / B) reduced to the fewest workgroups with as many tiles each (tiles = ceil(ch cw
 *                                            / 32)); the traces advance in k_trace BEFORE the layer kernel, because workgroups of
 *                                            one sample read each other's halo rows.  Results do not depend on NS.
 */
int64_t dcll_conv_lif_step_any_lds(const dcll_conv_desc *d);
int64_t dcll_conv_lif_step_any_scratch(const dcll_conv_desc *d);
int dcll_conv_lif_step_any(const dcll_conv_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                           const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                           const float *i2o_W, const float *i2o_b, const float *out_W, const float *out_b, float *out_s,
                           float *out_p, float *out_o, float *out_pv, float *out_v, float *w_scratch, int32_t B, void *stream);

/*
 * Added under ABI 10 (DCLL_ABI_VERSION is unchanged: a caller detects these three symbols by symbol lookup) — dcll_conv_lif_step_any
 * for the layers of 33 .. 64 output channels that a --netscale above 1 makes (k_lif_step_wide, csrc/dcll_step_wide.hip): the same
 * arguments, results, alignment rule (4 bytes, w_scratch included) and DCLL_ERR_INVALID cases.  Additions only: the default
 * dispatch, dcll_conv_lif_step_any, their launch logs and refusals (that call's "c_out <= 32" included) are unchanged.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in; c_out <= 64; kh, kw <= 16; any
 * padding, pooling and batch; and a working set within the 160 KiB of LDS of a workgroup:
 *   4 bytes x (c_in (h + 2 pad_h)(w + 2 pad_w) [zero-padded eps1 image] + (pooling != 1 ? c_out ch cw : 0) [v plane of the
 *   pooling pass] + 64 [bias]).
 * dcll_conv_lif_step_wide_lds returns these bytes, dcll_conv_lif_step_wide_scratch the floats of w_scratch — 128 per MFMA step of
 * a chain, written by k_step_wide_wprep in front of the layer kernel on EVERY call —; both 0 for a descriptor that is not served.
 * c_out <= 32: the call IS dcll_conv_lif_step_any — same kernels, launch log, bits, refusals (with that call's name in the
 * message) and _lds / _scratch values — so a network of mixed widths goes through one entry point.
 * c_out 33 .. 64: k_lif_step_any's decomposition and arithmetic with M = c_out padded to 64 rows, two 32-row tiles; each of the
 * two chains of a pixel tile is the pinned order, unsplit; rows at or beyond c_out carry zero weights and are never stored.  v
 * equals dcll_conv_lif_step bit for bit up to the sign of a zero; spikes, eps0, eps1 and arp bit for bit; pv within the sigmoid's
 * 1e-4.
 * Forms (the launch log names them; R = refractory; k_step_wide_wprep in front of each):
 *   "k_lif_step_wide<R>"                      one workgroup per sample; a wave runs BOTH M tiles of its pixel tiles, one LDS read
 *                                             of the B operand feeding two MFMAs
 *   "k_lif_step_wide<R> (pooling)"            the same with the v plane and the pooling pass in LDS
 *   "k_trace", "k_lif_step_wide<R> (split)"   NS > 1 workgroups per sample for a layer without pooling.  The unit is (pixel tile,
 *                                             M tile), units = 2 ceil(ch cw / 32); ns0 = min(ceil(units / 4), 256 / B); ns0 <= 1:
 *                                             fused; else upw = ceil(units / ns0), NS = ceil(units / upw), workgroup `part` runs
 *                                             units [part upw, (part + 1) upw).  The traces advance in k_trace BEFORE the layer
 *                                             kernel.  Results do not depend on NS.
 */
int64_t dcll_conv_lif_step_wide_lds(const dcll_conv_desc *d);
int64_t dcll_conv_lif_step_wide_scratch(const dcll_conv_desc *d);
int dcll_conv_lif_step_wide(const dcll_conv_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                            const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                            const float *i2o_W, const float *i2o_b, const float *out_W, const float *out_b, float *out_s,
                            float *out_p, float *out_o, float *out_pv, float *out_v, float *w_scratch, int32_t B, void *stream);

/*
 * Added under ABI 10 (DCLL_ABI_VERSION is unchanged: a caller detects these four symbols by symbol lookup) —
 * dcll_conv_lif_step_wide for ANY number of output channels and any plane height (k_lif_step_slab, csrc/dcll_step_slab.hip): the
 * same arguments with `int32_t bands` in front of B, the same results, alignment rule (4 bytes, w_scratch included) and
 * DCLL_ERR_INVALID cases, and bands < 0 -> DCLL_ERR_INVALID.  Additions only: the default dispatch, dcll_conv_lif_step_any,
 * dcll_conv_lif_step_wide, their launch logs and refusals ("c_out <= 32", "c_out <= 64" included) are unchanged.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch): stride = dilation = groups = 1; any c_in and c_out (at most 65 535 slabs
 * of 64 output channels); kh, kw <= 16; any padding, pooling and batch; and a plan whose bands fit the 160 KiB of LDS.
 * Grid = B x NB x NS workgroups.  NS = ceil(c_out / 64) slabs: slab s owns the channels [64 s, min(64 s + 64, c_out)), two 32-row
 * M tiles (a last slab of at most 32 rows: one; its second weight column is never read); rows at or beyond c_out are never
 * stored.  NB bands of output rows; band k owns the pooled rows [k ph / NB, (k + 1) ph / NB) and the conv rows [C0, C1) of their
 * pooling windows (the last band also those behind the last window of floor-mode pooling) — k_lif_seq_band's partition in h;
 * no tiling in w.  LDS of a (band, slab) workgroup:
 *   4 bytes x (c_in (C1 - C0 + kh - 1)(w + 2 pad_w) [the band's zero-padded eps1 rows] + (pooling != 1 ? 64 (C1 - C0) cw : 0)
 *   [the slab's v plane of the pooling pass] + 64 [bias]).
 * The plan: bands = N >= 1 -> NB = N (N > ph, or a band beyond the LDS: refused).  bands = 0 -> NB_fit = the smallest NB <= ph
 * whose largest band fits (none: refused); units = 2 ceil(ch cw / 32); ns0 = min(ceil(units / 4), 256 / (B NS)); NB =
 * max(NB_fit, min(ns0, ph)).  dcll_conv_lif_step_slab_plan (host only) returns NB and NS; dcll_conv_lif_step_slab_lds the bytes of
 * the largest workgroup under the plan (0: not served); dcll_conv_lif_step_slab_scratch the floats of w_scratch, 128 per MFMA step
 * of a chain and slab (0: not served), written as [slab][step][lane][2] by k_step_slab_wprep in front of the layer kernel on
 * EVERY call.
 * c_out <= 64, bands = 0 and a layer dcll_conv_lif_step_wide serves: the call IS that call — same kernels, launch log, bits and
 * _lds value (_plan then answers NB = NS = 0) — so a network of mixed widths goes through one entry point.  Everything else that
 * is served runs k_lif_step_slab, NS = 1 included.
 * The traces advance in k_trace BEFORE the layer kernel (workgroups of a sample read each other's halo rows, every slab reads the
 * same traces); the kernel stages them read-only.  Each chain is the pinned order, unsplit: v equals dcll_conv_lif_step bit for
 * bit up to the sign of a zero; spikes, eps0, eps1 and arp bit for bit; pv within the sigmoid's 1e-4.  Nothing depends on NB.
 * Launch log (R = refractory): "k_step_slab_wprep", "k_trace", then "k_lif_step_slab<R>" or "k_lif_step_slab<R> (pooling)".
 */
int64_t dcll_conv_lif_step_slab_lds(const dcll_conv_desc *d, int32_t B, int32_t bands);
int64_t dcll_conv_lif_step_slab_scratch(const dcll_conv_desc *d);
int dcll_conv_lif_step_slab_plan(const dcll_conv_desc *d, int32_t B, int32_t bands, int32_t *nb, int32_t *ns);
int dcll_conv_lif_step_slab(const dcll_conv_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                            const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                            const float *i2o_W, const float *i2o_b, const float *out_W, const float *out_b, float *out_s,
                            float *out_p, float *out_o, float *out_pv, float *out_v, float *w_scratch, int32_t bands, int32_t B,
                            void *stream);

/*
 * Added under ABI 10 (DCLL_ABI_VERSION is unchanged: a caller detects these two symbols by symbol lookup) — one layer step of a
 * (1,3) / 64-channel / (1,2)-pool layer of radio_ml_conv_ref.yaml in one MFMA launch (k_lif_step_w3, csrc/dcll_step_w3.hip):
 * dcll_conv_lif_step_any's arguments without w_scratch, dcll_conv_lif_step's results.  Additions only: the default dispatch, its
 * launch logs and every refusal of the existing entry points are unchanged.
 * Served (else DCLL_ERR_UNSUPPORTED, before any launch) — exactly the layers the fused sequence kernel k_lif_seq_w3 serves: c_in 1
 * or 64, c_out 64, kernel (1,3), padding (0,1), pooling (1,2), w a power of two <= 256, h w % 32 == 0, h w < 2^24, stride =
 * dilation = groups = 1.  dcll_conv_lif_step_w3_lds returns the LDS bytes of a workgroup of the larger form,
 *   4 x ((256 + 256 / w + 1) x (c_in == 64 ? 65 : 1) + 64),
 * and 0 for a descriptor that is not served (invalid ones included); the launcher checks each launch against it.
 * DCLL_ERR_INVALID, before any launch: a NULL required pointer, a refractory layer without arp, an output layer without out_W /
 * out_o, B < 0, B h w / 32 beyond 2^31 - 9.  B == 0: DCLL_OK, nothing is looked at.  Nothing is allocated, nothing synchronises.
 * As dcll_conv_lif_step_any: dense fp32 x of any values; fp32 weights only, read from W on every call (the learning step changes
 * them between any two calls: no permuted copy is kept); b may be NULL; scalar or (c_in,h,w) time constants; eps0 / eps1 / arp
 * updated in place; out_v (un-pooled) may be NULL; p / o through the same readout kernels.  Pointers need 4-byte alignment only.
 * Arithmetic: the contract at the top of this file — every v is ONE fmaf chain from b[co] over (cp, kx, h), ci = 2 cp + h, on
 * v_mfma_f32_32x32x2_f32 (c_in = 1: three fmaf, kx = 0, 1, 2).  v equals dcll_conv_lif_step bit for bit up to the sign of a zero;
 * pooled spikes, eps0, eps1 and arp bit for bit; pv within the sigmoid's 1e-4.
 * Forms (the launch log names them; R = refractory): a 512-thread workgroup owns 8 or 4 consecutive 32-pixel tiles of the
 * flattened planes and advances their traces in place, so it must own whole rows (32 x tiles % w == 0):
 *   "k_lif_step_w3<R> (8 tiles)"             c_in 64
 *   "k_lif_step_w3<R> (4 tiles)"             c_in 64, w <= 128 and ceil(B h w / 256) < 256 (fewer 8-tile workgroups than CUs)
 *   "k_lif_step_w3<R> (c_in 1, 8 tiles)"     first layer, the chain on the vector pipe
 *   "k_lif_step_w3<R> (c_in 1, 4 tiles)"     the same rule
 * Results do not depend on the form.
 */
int64_t dcll_conv_lif_step_w3_lds(const dcll_conv_desc *d);
int dcll_conv_lif_step_w3(const dcll_conv_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                          const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                          const float *i2o_W, const float *i2o_b, const float *out_W, const float *out_b, float *out_s,
                          float *out_p, float *out_o, float *out_pv, float *out_v, int32_t B, void *stream);

/*
 * Added under ABI 10 (DCLL_ABI_VERSION is unchanged: a caller detects these three symbols by symbol lookup) — the backward of a
 * layer of that geometry with the weight gradient of its 64 -> 64 form as an fp32-MFMA GEMM (k_bwd_wgrad_w3,
 * csrc/dcll_step_w3.hip): arguments, results and scratch rule of dcll_conv_lif_backward / dcll_conv_lif_backward_open
 * (scratch_floats >= B 64 h w + k x 64 (3 c_in + 1), k >= 1 partial rows; at most 256 are used).  dv comes from the existing
 * k_bwd_dv, the output_ gradient from the existing kernels; dcll_conv_lif_backward and its launch logs are unchanged.
 * Served: the layers dcll_conv_lif_step_w3 serves (else DCLL_ERR_UNSUPPORTED before any launch).  dcll_conv_lif_backward_w3_lds
 * returns the LDS bytes of the weight-gradient kernel's workgroup — c_in 64: 4 x (64 CS + 64 x 129 + 16), CS = the positions of a
 * 128-pixel block (128 + 128 / w + 1; w = 256: 130) rounded up to 3 mod 32, at most 83 008 (w = 2) — and 0 for a descriptor that is
 * not served; the launcher checks each launch against it.
 * DCLL_ERR_INVALID, before any launch: a NULL required pointer, v == NULL (these layers always pool), a scratch too small for one
 * partial row, B < 0.  B == 0: DCLL_OK, nothing is looked at.
 * Launch log: "k_bwd_dv", then "k_bwd_wgrad_w3" (c_in 64) or the generic "k_bwd_wgrad" (c_in 1: 3 + 1 columns are not matrix
 * work; the entry point keeps the default kernel for it), then the reduction / output_ gradient kernels of dcll_conv_lif_backward.
 * Sums: chunk c takes the 128-pixel blocks c, c + nchunk, ... of the flattened (B x h w) pixels in order; inside a block the
 * pixel pairs [0, 32) and [32, 64) run as two fma chains (pixel 2 pp, then 2 pp + 1) that are added, first + second, at the end;
 * the chunks are reduced by k_bwd_reduce[4] / dcll_grad_reduce_adam.  Every order is fixed: two runs give the same bits, and
 * _open + dcll_grad_reduce_adam gives the closed form's.  NOT bit-identical to dcll_conv_lif_backward: the order differs.
 */
int64_t dcll_conv_lif_backward_w3_lds(const dcll_conv_desc *d);
int dcll_conv_lif_backward_w3(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                              const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                              float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                              int32_t B, void *stream);
int dcll_conv_lif_backward_w3_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                   const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                   float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                   const float **part, int32_t *nchunk, void *stream);

/*
 * Found by symbol lookup as well (DCLL_ABI_VERSION stays 10) — dcll_conv_lif_backward_w3 / _w3_open with the weight gradient of the
 * FIRST layer (c_in 1 -> 64) on k_bwd_wgrad_w3f (csrc/dcll_step_w3.hip) instead of the generic k_bwd_wgrad: a register-only
 * streaming reduction of the dv plane, 64 x (3 + 1) numbers over B h w pixels.  Arguments, served set (dcll_conv_lif_backward_w3_lds
 * is the predicate), scratch rule (scratch_floats >= B 64 h w + k x 64 (3 c_in + 1), k >= 1 partial rows; at most 256 are used, at
 * most one per 128 pixels of the flattened planes for c_in 1), refusals (all before any launch) and B == 0 are those of
 * dcll_conv_lif_backward_w3[_open]; scratch and eps1 need 4-byte alignment only.
 * Launch log: "k_bwd_dv", then for c_in 1 "k_bwd_wgrad_w3f" (scratch and eps1 both 16-byte aligned: 16-byte loads) or
 * "k_bwd_wgrad_w3f (unaligned)" (scalar loads; the same sums, the same bits), for c_in 64 "k_bwd_wgrad_w3" (bit-identical to
 * dcll_conv_lif_backward_w3), then the reduction / output_ gradient kernels of dcll_conv_lif_backward.  The dv plane left in
 * scratch[0 : B 64 h w], d_outW and d_outb are dcll_conv_lif_backward_w3's bits.
 * Sums (c_in 1): chunk c takes the 128-pixel jobs c, c + nchunk, ... of the flattened (B x h w) pixels — its job list i = 0, 1, ...;
 * the jobs of even and of odd i are two separate sums; inside each, lane q = 0 .. 31 runs the pixels 4 q .. 4 q + 3 of its jobs in
 * order as one chain per tap (fma) and for the bias (add); the 32 lanes are added by a fixed tree (q ^ 1, q ^ 2, mirror in 8,
 * mirror in 16, upper 16 + lower 16), then even + odd; the chunks are reduced by k_bwd_reduce[4] / dcll_grad_reduce_adam.  Every
 * order is fixed: two runs give the same bits, and _open + dcll_grad_reduce_adam gives the closed form's.  dW / db of the first
 * layer are NOT bit-identical to dcll_conv_lif_backward / dcll_conv_lif_backward_w3 (k_bwd_wgrad): the order differs.
 */
int dcll_conv_lif_backward_w3f(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                               const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                               float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                               int32_t B, void *stream);
int dcll_conv_lif_backward_w3f_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                    const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                    float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                    const float **part, int32_t *nchunk, void *stream);

/*
 * Found by symbol lookup as well (DCLL_ABI_VERSION stays 10) — dcll_conv_lif_backward_w3 / _w3_open with a flag word in front of
 * the stream.  flags == 0: dcll_conv_lif_backward_w3[_open], bits and launch log; DCLL_W3_FIRST_WGRAD: those of
 * dcll_conv_lif_backward_w3f[_open].  DCLL_W3_DV: the "k_bwd_dv" launch of either is replaced by k_bwd_dv_w3
 * (csrc/dcll_step_w3.hip), a streaming form of the same formula for these layers' (1,2) pooling: a thread owns two consecutive
 * pooled positions (four un-pooled elements: 16-byte loads and stores) with their readout weights in registers over a chunk of
 * samples.  The dv plane left in scratch[0 : B 64 h w] is k_bwd_dv's BIT FOR BIT (same operations in the same order; a tie of the
 * two sigmoids of a pair goes to the left element), so the weight gradient, the reduction, d_outW and d_outb behind it are the
 * bits of the same call without the flag.  Served set, scratch rule and refusals (all before any launch) are
 * dcll_conv_lif_backward_w3's; any other flag bit: DCLL_ERR_INVALID; B == 0 (with valid flags): DCLL_OK, nothing else is looked at.
 * target > 32 keeps k_bwd_dv.  g_p, g_pv and g_v may each be NULL.
 * Launch log with DCLL_W3_DV: "k_bwd_dv_w3" (v, scratch and g_v 16-byte and g_pv and i2o_W 8-byte aligned) or "k_bwd_dv_w3
 * (unaligned)" (scalar loads, the same bits; the ABI asks for 4-byte alignment only) or, for target > 32, "k_bwd_dv"; then as
 * without the flag.
 */
#define DCLL_W3_FIRST_WGRAD 1u
#define DCLL_W3_DV 2u
int dcll_conv_lif_backward_w3_ex(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                 const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                 float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                                 int32_t B, uint32_t flags, void *stream);
int dcll_conv_lif_backward_w3_ex_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                      const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                      float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                      const float **part, int32_t *nchunk, uint32_t flags, void *stream);

/*
 * Found by symbol lookup as well (DCLL_ABI_VERSION stays 10) — the backward calls behind one pair of entry points, with a flag
 * word.  path names the call: DCLL_BWD_DEFAULT dcll_conv_lif_backward[_open], DCLL_BWD_ANY / _WIDE / _SLAB / _BANDS the call of that
 * suffix; bands is the argument of dcll_conv_lif_backward_bands and must be 0 with every other path.  flags == 0 IS the named
 * call: its bits, its launch log, its refusals and its scratch rule.
 * DCLL_BWD_POOL_DV: the "k_bwd_dv" launch of that call is replaced by k_bwd_dv_pool (csrc/dcll_bwd_dv_pool.hip) where
 * dcll_bwd_dv_pool_served(d, B) == 1 — a streaming form of the same formula for a layer that pools: a thread owns one pooled
 * window (k = (co, py, px), consecutive threads consecutive k) with its readout weights in registers over a chunk of samples (8, or 4 / 2
 * where 8 would leave fewer than 512 workgroups),
 * takes the sigmoid of each of the window's in-range elements once, picks the first maximum in row-major order (strict > on the
 * sigmoids) and writes the window; the trailing rows / columns that belong to no window (an odd plane under pool 2, the last row /
 * column of a plane divisible by 3 under pool 3) are written by the threads of the last window row / column.  The dv plane left in
 * scratch[0 : B c_out ch cw] is k_bwd_dv's BIT FOR BIT for every finite or infinite membrane (same operations in the same order),
 * so the weight gradient, the reduction, d_outW and d_outb behind it are the bits of the same call without the flag.  A NaN
 * membrane is outside that contract (k_bwd_dv lets a NaN element win beside its window's maximum; k_bwd_dv_pool picks one winner).
 * Served: pool_h, pool_w in {1, 2, 3}, not both 1; ch >= pool_h, cw >= pool_w; target <= 32; c_out ph pw and c_out ch cw below
 * 2^31 (less a margin of one workgroup / one plane row); at most 65535 chunks of 8 samples.  The conv's own parameters do not
 * enter.  The flag on a layer without pooling ("k_bwd_dv_nopool<..>") or on an unserved layer ("k_bwd_dv") is accepted and changes
 * nothing.  v, scratch, g_v, g_pv and i2o_W need 4-byte alignment only (one form, scalar loads); g_p, g_pv and g_v may each be NULL.
 * DCLL_ERR_INVALID before anything is launched and before B is looked at: an unknown flag bit, an unknown path, bands != 0 with a
 * path other than DCLL_BWD_BANDS, (open form) a NULL part / nchunk.  B == 0 with those valid: DCLL_OK, nothing else is looked at.
 * Launch log with the flag on a served layer: "k_bwd_dv_pool", then as without the flag.
 * dcll_bwd_dv_pool_served: host only, launches nothing; 1 served, 0 not served (B < 1 included), a negative DCLL_ERR_* for an
 * invalid descriptor.
 */
#define DCLL_BWD_DEFAULT 0   /* dcll_conv_lif_backward        */
#define DCLL_BWD_ANY     1   /* dcll_conv_lif_backward_any    */
#define DCLL_BWD_WIDE    2   /* dcll_conv_lif_backward_wide   */
#define DCLL_BWD_SLAB    3   /* dcll_conv_lif_backward_slab   */
#define DCLL_BWD_BANDS   4   /* dcll_conv_lif_backward_bands  */
#define DCLL_BWD_POOL_DV 1u
int dcll_conv_lif_backward_ex(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                              const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                              float *dW, float *db, float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats,
                              int32_t B, int32_t path, int32_t bands, uint32_t flags, void *stream);
int dcll_conv_lif_backward_ex_open(const dcll_conv_desc *d, const float *eps1, const float *v, const float *pv_pooled,
                                   const float *g_p, const float *g_o, const float *g_pv, const float *g_v, const float *i2o_W,
                                   float *d_outW, float *d_outb, float *scratch, int64_t scratch_floats, int32_t B,
                                   const float **part, int32_t *nchunk, int32_t path, int32_t bands, uint32_t flags, void *stream);
int32_t dcll_bwd_dv_pool_served(const dcll_conv_desc *d, int32_t B);

#ifdef __cplusplus
}
#endif
#endif /* DCLL_HIP_H */
