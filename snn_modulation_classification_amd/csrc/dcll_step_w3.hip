// dcll_step_w3.hip — k_lif_step_w3: ONE timestep of a layer of networks/radio_ml_conv_ref.yaml (c_in 1 or 64, 64 output
// channels, kernel (1,3), padding (0,1), max-pool (1,2), w a power of two <= 256, h w % 32 == 0: exactly the layers
// dcll_seq_w3_geometry() serves) in one launch (dcll_conv_lif_step_w3; added under ABI 10, found by symbol lookup) — the opt-in
// MFMA form of the layers dcll_conv_lif_step serves with k_trace + k_conv_lif_tiled<1,3> + k_pool.  The per-step sibling of
// k_lif_seq_w3 (dcll_seq_w3.hip), with the state in HBM and dense fp32 input of any values.
//
// Decomposition = k_lif_seq_w3's: the kernel height is 1, so rows are independent, and pooling pairs are neighbours in the
// flattened plane.  A layer is a stream of 32-pixel TILES of the flattened (B x H W) pixels (h w % 32 == 0: a tile lies in one
// sample); a 512-thread workgroup owns NT consecutive tiles.  Wave (mt, g) = (wave & 1, wave >> 1) runs the whole pinned chain
// bias -> (cp, kx, h), ci = 2 cp + h, of tiles (NT / 4) g ... for output channels 32 mt ... 32 mt + 31 on
// v_mfma_f32_32x32x2_f32: 96 MFMAs per tile, every v is ONE chain, so v, spikes and state are bit-identical to the per-step
// kernels and the C oracle (include/dcll_hip.h).
//
// Two forms, chosen by dcll_step_w3_tiles(descriptor, B) alone: NT = 8 (256 pixels; two tiles per wave), and NT = 4 (128
// pixels; one tile per wave) for launches whose 8-tile grid would have fewer than 256 workgroups.  Every chain is whole in
// either form: the results do not depend on it.
// RACE NOTE: a workgroup advances the traces of its pixels IN PLACE and reads the +-1 halo of every pixel, so it must own whole
// rows — 32 NT % w == 0 — or a sibling would read halo traces this workgroup is overwriting (the race once found in
// k_lif_seq_w3f).  256 % w == 0 for every served width; the 4-tile form is legal for w <= 128 only.  dcll_launch_step_w3
// checks the condition for the form it is handed.
//
// Phases of a workgroup:
//   1. traces: wave = one tile (NT = 4: one tile and half the channels), lane = (pixel jj = lane & 31, channel parity
//      lane >> 5): every wave access to x / eps0 / eps1 (layout (B, c_in, h, w)) is two whole 128-byte lines.  x, eps0, eps1
//      are read, advanced with the contract's three separately rounded operations (trace_update), eps0' / eps1' written back
//      and eps1' kept in the LDS image; four channel pairs are in flight per wave.
//   2. barrier; per tile the chain (B fragments from the image, A fragments = 96 registers read straight from W — 48 KB,
//      L2-resident — on every call: weights change between any two calls of a learning loop, nothing is cached), then the
//      epilogue from the accumulators: refractory update on arp in HBM, un-pooled out_v if asked, (1,2) max-pool of v by one
//      v_permlane16_swap + v_max per register pair (lanes 0..15 of a tile hold the EVEN pixels, 16..31 the ODD ones, as in
//      k_lif_seq_w3), spike = pooled v > 0, pv = sigmoid(pooled v).  No un-pooled map makes a round trip through HBM.
//
// LDS image, PIXEL-major: element (ci, position q) at q PST + ci, PST = 65; q = p + (p >> log2 w) + 1 for pixel p of the
// workgroup — one shared zero position in front of every row and behind the last one (the conv's horizontal padding):
// 32 NT + 32 NT / w + 1 positions.  Bank = dword address % 32 for ds_read_b32 / ds_write_b32, conflicts counted inside a
// 32-lane half:
//   - trace write (a half = 32 consecutive pixels of one channel): banks (65 q + ci) % 32 = (q + ci) % 32 — conflict-free for
//     w >= 32 (32 consecutive q); for w < 32 the 32 pixels span 32 + 32 / w - 1 <= 47 positions: 2-way at worst;
//   - B-fragment read (a half = the 32 pixels of a tile, one channel, one tap): the same 32 positions shifted: conflict-free
//     for w >= 32, 2-way at worst below.
// c_in = 1 (first layer: a store stream, not matrix work): same phases with a one-channel image (PST = 1); the chain is the
// contract's three fmaf on the vector pipe, wave = 8 output channels, lane = pixel, pooling partner by one DPP quad permute.
//
// Not bit-identical in pv, p and o only where the contract leaves them free (1e-4); everything else equals dcll_conv_lif_step.
#include "dcll_internal.h"
#include <mutex>

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int SW_THREADS = 512;
constexpr int SW_PST = 65;
constexpr int SW_MAX_DEVICES = 64;
constexpr int SW_MIN_WGS = 256;         // the chip's CUs: below that many 8-tile workgroups the 4-tile form is taken

// floats of a workgroup of nt tiles: the image (positions x channel stride) and 64 bias values
static inline long step_w3_lds_floats(const dcll_conv_desc *d, int nt)
{
    const long npos = 32L * nt + 32L * nt / d->w + 1;
    return npos * (d->c_in == 64 ? SW_PST : 1) + 64;
}

// the support predicate: DCLL_OK, or the refusal with its message
int dcll_step_w3_check(const dcll_conv_desc *d, const char *who)
{
    int rc = check_desc(d);
    if (rc) return rc;
    if (!dcll_seq_w3_geometry(d))
        return fail(DCLL_ERR_UNSUPPORTED, "serves c_in 1 or 64, c_out 64, kernel (1,3), padding (0,1), pooling (1,2), w a power of "
                                          "two <= 256, h * w % 32 == 0, stride = dilation = groups = 1", who);
    if ((long)d->h * d->w >= (1L << 24)) return fail(DCLL_ERR_UNSUPPORTED, "plane larger than 2^24 pixels", who);
    return DCLL_OK;
}

// LDS bytes of the larger (8-tile) form; 0 = not served
extern "C" int64_t dcll_conv_lif_step_w3_lds(const dcll_conv_desc *d)
{
    return dcll_step_w3_check(d, "dcll_conv_lif_step_w3_lds") == DCLL_OK ? step_w3_lds_floats(d, 8) * 4 : 0;
}

// tiles per workgroup, a pure function of (descriptor, B): 4 where the race note allows it (128 % w == 0) and the 8-tile grid
// would have fewer than SW_MIN_WGS workgroups, else 8
int dcll_step_w3_tiles(const dcll_conv_desc *d, int32_t B)
{
    const long ntot = (long)B * ((long)d->h * d->w / 32);
    return (d->w <= 128 && (ntot + 7) / 8 < SW_MIN_WGS) ? 4 : 8;
}

template <int CIN, bool R, int NT>
__global__ __launch_bounds__(SW_THREADS) void k_lif_step_w3(const float *__restrict__ x, const float *__restrict__ W,
                                                           const float *__restrict__ bias, const float *__restrict__ alpha,
                                                           const float *__restrict__ tau_m, const float *__restrict__ alphas,
                                                           const float *__restrict__ tau_s, int tau_is_tensor,
                                                           float *__restrict__ eps0_g, float *__restrict__ eps1_g,
                                                           float *__restrict__ arp_g, float *__restrict__ out_s,
                                                           float *__restrict__ out_pv, float *__restrict__ out_v, int ntot, int HW,
                                                           int logW, float alpharp, float wrp)
{
    static_assert((CIN == 64 || CIN == 1) && (NT == 8 || NT == 4), "two channel counts, two forms");
    extern __shared__ float lds[];
    constexpr int PST = CIN == 64 ? SW_PST : 1, P = 32 * NT;
    const int npos = P + (P >> logW) + 1;
    float *img = lds, *sb = lds + npos * PST;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, jj = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NTS = HW >> 5, HW2 = HW >> 1;             // tiles per sample, pooled pixels per channel plane
    const int G0 = (int)blockIdx.x * NT;                // first tile of this workgroup (ntot < 2^31: the launcher)

    // ---- the zero positions k (w + 1), k = 0 .. P / w, of every channel; the bias
    for (int i = tid; i < ((P >> logW) + 1) * CIN; i += SW_THREADS) {
        const int k = i / CIN, c = i - k * CIN;
        img[k * ((1 << logW) + 1) * PST + c] = 0.0f;
    }
    if (tid < 64) sb[tid] = bias ? bias[tid] : 0.0f;

    // ---- weights of my output-channel tile (CIN = 64): A[co = 32 mt + jj][step s = 3 cp + kx] = W[co][2 cp + h][kx]
    const int mt = wv & 1, g = wv >> 1;
    float wf[CIN == 64 ? 96 : 1];
    if constexpr (CIN == 64) {
        const float *wr = W + (32 * mt + jj) * 192 + 3 * h;
#pragma unroll
        for (int s = 0; s < 96; ++s) wf[s] = wr[6 * (s / 3) + s % 3];
    }

    // ---- (1) traces: wave = tile tt (NT = 4: waves tt and tt + 4 share it, half the channels each)
    {
        const int tt = wv % NT, cpart = wv / NT;
        const int Gt = G0 + tt;
        if (Gt < ntot && (CIN == 64 || (cpart == 0 && h == 0))) {
            const int bt = Gt / NTS, m = Gt - bt * NTS;
            const int p = 32 * tt + jj, q = p + (p >> logW) + 1;
            const long sbase = (long)bt * CIN * HW;
            if constexpr (CIN == 64) {
                constexpr int NC = 8 * NT, U = 4;               // channels of this wave, channel pairs in flight
                for (int k0 = 0; k0 < NC / 2; k0 += U) {
                    float xs[U], e0[U], e1[U], ta[U], tm[U], tas[U], ts[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int ci = cpart * NC + 2 * (k0 + u) + h, is = ci * HW + 32 * m + jj, t = tau_is_tensor ? is : 0;
                        xs[u] = x[sbase + is];
                        e0[u] = eps0_g[sbase + is];
                        e1[u] = eps1_g[sbase + is];
                        ta[u] = alpha[t], tm[u] = tau_m[t], tas[u] = alphas[t], ts[u] = tau_s[t];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int ci = cpart * NC + 2 * (k0 + u) + h, is = ci * HW + 32 * m + jj;
                        trace_update(xs[u], ta[u], tm[u], tas[u], ts[u], e0[u], e1[u]);
                        eps0_g[sbase + is] = e0[u];
                        eps1_g[sbase + is] = e1[u];
                        img[q * PST + ci] = e1[u];
                    }
                }
            } else {
                const int is = 32 * m + jj, t = tau_is_tensor ? is : 0;
                float e0 = eps0_g[sbase + is], e1 = eps1_g[sbase + is];
                trace_update(x[sbase + is], alpha[t], tau_m[t], alphas[t], tau_s[t], e0, e1);
                eps0_g[sbase + is] = e0;
                eps1_g[sbase + is] = e1;
                img[q] = e1;
            }
        }
    }
    __syncthreads();

    if constexpr (CIN == 64) {
        // ---- (2) per tile: the chain in the pinned order (cp, kx, h), then its epilogue
        constexpr int TPW = NT / 4;
        const int perm = jj < 16 ? 2 * jj : 2 * (jj - 16) + 1;         // lane -> pixel of the tile (even | odd)
        const int rw = lane >> 4;
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int tl = TPW * g + u, G = G0 + tl;
            if (G >= ntot) break;                                       // (wave-uniform)
            const int b = __builtin_amdgcn_readfirstlane(G / NTS), m = __builtin_amdgcn_readfirstlane(G - (G / NTS) * NTS);
            const int p = 32 * tl + perm;
            const int base = h + (p + (p >> logW)) * PST;              // B-fragment lane base: channel h of pair 0, tap 0
            // value r of lane (h, jj): channel 32 mt + (r & 3) + 8 (r >> 2) + 4 h, pixel perm
            const long ov = ((long)b * 64 + 32 * mt + 4 * h) * HW + 32 * m + perm;
            float arp[16];
            if (R) {
#pragma unroll
                for (int r = 0; r < 16; ++r) arp[r] = arp_g[ov + (long)((r & 3) + 8 * (r >> 2)) * HW];
            }
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = sb[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h];
            // the 6 B fragments of channel pairs 2 c2 + 2, 2 c2 + 3 are fetched before the MFMAs of pairs 2 c2, 2 c2 + 1
            float bq[2][6];
#pragma unroll
            for (int q = 0; q < 6; ++q) bq[0][q] = img[base + (q / 3) * 2 + (q % 3) * PST];
#pragma unroll
            for (int c2 = 0; c2 < 16; ++c2) {
                if (c2 + 1 < 16) {
#pragma unroll
                    for (int q = 0; q < 6; ++q) bq[(c2 + 1) & 1][q] = img[base + (2 * (c2 + 1) + q / 3) * 2 + (q % 3) * PST];
                }
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[c2 * 6 + q], bq[c2 & 1][q], acc, 0, 0, 0);
            }
            // pooled map after the row swap: lane row rw holds channel cr + (rw & 1) + 4 (rw >> 1), pooled pixel lane & 15
            const long op = ((long)b * 64 + 32 * mt + (rw & 1) + 4 * (rw >> 1)) * HW2 + 16 * m + (lane & 15);
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int cr = (r & 3) + 8 * (r >> 2);
                const long o0 = ov + (long)cr * HW, o1 = o0 + HW;
                float vx = acc[r], vy = acc[r + 1];
                if (R) {
                    bool s;
                    float ax = arp[r], ay = arp[r + 1];
                    vx = refractory(acc[r], ax, alpharp, wrp, s);
                    vy = refractory(acc[r + 1], ay, alpharp, wrp, s);
                    arp_g[o0] = ax;
                    arp_g[o1] = ay;
                }
                if (out_v) {
                    out_v[o0] = vx;
                    out_v[o1] = vy;
                }
                // rows (16 lanes) of vx: [even px | odd px] of channel cr (h = 0), the same of channel cr + 4 (h = 1); after the
                // swap sw[0] = [vx.row0, vy.row0, vx.row2, vy.row2], sw[1] = [vx.row1, vy.row1, vx.row3, vy.row3]: their
                // maximum is the pooled v of channel cr in rows 0 / 2 and of channel cr + 1 in rows 1 / 3
                const u32x2 sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(vx), __float_as_uint(vy), false, false);
                const float pm = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                out_s[op + (long)cr * HW2] = pm > 0.0f ? 1.0f : 0.0f;
                out_pv[op + (long)cr * HW2] = sigmoidf_dev(pm);
            }
        }
    } else {
        // ---- (2) first layer: wave = output channels 8 wv .. 8 wv + 7, lane = pixel; bias -> kx = 0, 1, 2 as three fmaf
        float w0[8], w1[8], w2[8], bv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int co = 8 * wv + c;
            w0[c] = W[co * 3], w1[c] = W[co * 3 + 1], w2[c] = W[co * 3 + 2], bv[c] = sb[co];
        }
        for (int pp = 0; pp < P / 64; ++pp) {
            const int p = 64 * pp + lane, G = G0 + (p >> 5);
            const bool valid = G < ntot;
            const int b = valid ? G / NTS : 0, m = valid ? G - b * NTS : 0;
            const int q = p + (p >> logW) + 1;
            const float eL = img[q - 1], eC = img[q], eR = img[q + 1];  // (a tile beyond the last: unwritten LDS, never stored)
            const long o = (long)b * 64 * HW + 32 * m + (p & 31), op = (long)b * 64 * HW2 + 16 * m + ((p & 31) >> 1);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int co = 8 * wv + c;
                float v = bv[c];
                v = __builtin_fmaf(eL, w0[c], v);
                v = __builtin_fmaf(eC, w1[c], v);
                v = __builtin_fmaf(eR, w2[c], v);
                if (R && valid) {
                    bool s;
                    float ar = arp_g[o + (long)co * HW];
                    v = refractory(v, ar, alpharp, wrp, s);
                    arp_g[o + (long)co * HW] = ar;
                }
                if (out_v && valid) out_v[o + (long)co * HW] = v;
                // the pooling partner: pixel p ^ 1 = lane ^ 1 (quad_perm [1,0,3,2]); the even lane stores the pair
                const float vn = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
                const float pm = fmaxf(v, vn);
                if (valid && !(lane & 1)) {
                    out_s[op + (long)co * HW2] = pm > 0.0f ? 1.0f : 0.0f;
                    out_pv[op + (long)co * HW2] = sigmoidf_dev(pm);
                }
            }
        }
    }
}

template <int CIN, bool R, int NT>
static int launch_step_w3(const dcll_conv_desc *d, size_t lds_bytes, const float *x, const float *W, const float *b,
                          const float *alpha, const float *tau_m, const float *alphas, const float *tau_s, float *eps0,
                          float *eps1, float *arp, float *out_s, float *out_pv, float *out_v, int ntot, int logW, hipStream_t st,
                          const char *name, bool launch)
{
    // dynamic LDS above 64 KiB is reserved per template instance AND device, asked for again only when a call needs more than
    // any before it on this device (as launch_step_any does: no attribute call falls inside a graph capture that repeats the
    // geometry of the eager steps before it)
    static std::mutex mu;
    static size_t reserved[SW_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_lif_step_w3: no current device");
    }
    if (lds_bytes > 64 * 1024) {
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= SW_MAX_DEVICES || lds_bytes > reserved[dev]) {
            if (hipFuncSetAttribute((const void *)k_lif_step_w3<CIN, R, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(DCLL_ERR_LAUNCH, "k_lif_step_w3: cannot reserve its LDS");
            }
            if (dev < SW_MAX_DEVICES) reserved[dev] = lds_bytes;
        }
    }
    if (!launch) return DCLL_OK;
    hipLaunchKernelGGL((k_lif_step_w3<CIN, R, NT>), dim3((unsigned)((ntot + NT - 1) / NT)), dim3(SW_THREADS), lds_bytes, st, x, W,
                       b, alpha, tau_m, alphas, tau_s, d->tau_is_tensor, eps0, eps1, arp, out_s, out_pv, out_v, ntot, d->h * d->w,
                       logW, d->alpharp, d->wrp);
    HIP_CHECK_LAUNCH(name);
    return DCLL_OK;
}

// the layer kernel of a checked call (dcll_step_w3_check; nt = dcll_step_w3_tiles(d, B)).  launch == false: everything that can
// fail short of the launch itself — the form, grid and LDS checks, the LDS reservation — and nothing else; the entry point
// calls this form first, so an error return never follows a launch
int dcll_launch_step_w3(const dcll_conv_desc *d, const float *x, const float *W, const float *b, const float *alpha,
                        const float *tau_m, const float *alphas, const float *tau_s, float *eps0, float *eps1, float *arp,
                        float *out_s, float *out_pv, float *out_v, int nt, int32_t B, hipStream_t st, bool launch)
{
    const char *who = "dcll_conv_lif_step_w3";
    // RACE NOTE (file header): the in-place trace write-back needs workgroups of whole rows
    if ((nt != 8 && nt != 4) || (32 * nt) % d->w != 0)
        return fail(DCLL_ERR_LAUNCH, "a workgroup's pixels must be whole rows (32 * tiles % w == 0)", who);
    const long ntot = (long)B * ((long)d->h * d->w / 32);
    if (ntot > 0x7fffffffL - 8) return fail(DCLL_ERR_INVALID, "batch x tiles exceeds the grid limit", who);
    const size_t lds_bytes = (size_t)step_w3_lds_floats(d, nt) * 4;
    if ((int64_t)lds_bytes > dcll_conv_lif_step_w3_lds(d))      // each launch against the exported bytes
        return fail(DCLL_ERR_LAUNCH, "LDS of this form exceeds dcll_conv_lif_step_w3_lds", who);
    int logW = 0;
    while ((1 << logW) < d->w) ++logW;
#define DCLL_SW(C_, R_, N_, name_)                                                                                            \
    return launch_step_w3<C_, R_, N_>(d, lds_bytes, x, W, b, alpha, tau_m, alphas, tau_s, eps0, eps1, arp, out_s, out_pv, out_v, \
                                      (int)ntot, logW, st, name_, launch)
    if (d->c_in == 64) {
        if (d->refractory) {
            if (nt == 8) DCLL_SW(64, true, 8, "k_lif_step_w3<1> (8 tiles)");
            DCLL_SW(64, true, 4, "k_lif_step_w3<1> (4 tiles)");
        }
        if (nt == 8) DCLL_SW(64, false, 8, "k_lif_step_w3<0> (8 tiles)");
        DCLL_SW(64, false, 4, "k_lif_step_w3<0> (4 tiles)");
    }
    if (d->refractory) {
        if (nt == 8) DCLL_SW(1, true, 8, "k_lif_step_w3<1> (c_in 1, 8 tiles)");
        DCLL_SW(1, true, 4, "k_lif_step_w3<1> (c_in 1, 4 tiles)");
    }
    if (nt == 8) DCLL_SW(1, false, 8, "k_lif_step_w3<0> (c_in 1, 8 tiles)");
    DCLL_SW(1, false, 4, "k_lif_step_w3<0> (c_in 1, 4 tiles)");
#undef DCLL_SW
}

// ---------------------------------------------------------------------------------------------------------------------
// k_bwd_wgrad_w3 — the weight gradient of a 64 -> 64 layer of that geometry as an fp32-MFMA GEMM
// (dcll_conv_lif_backward_w3[_open]; added under ABI 10):
//
//   dW[co][ci 3 + kx] = sum_{b,p} g[b,co,p] * eps1[b,ci,p + kx - 1]  (zero beyond a row's ends),   db[co] = sum g
//
// M = 64 output channels (two 32-row tiles mt), N = 192 columns n = 3 ci + kx (six 32-column tiles ct), K = the pixels of the
// flattened planes two at a time: the two k lanes of one v_mfma_f32_32x32x2_f32 are the pixels 2 pp, 2 pp + 1 — w is even, a
// pair never straddles a row.  g is the dv plane the existing k_bwd_dv wrote.
// The pixel stream (B x H W) is cut into BLOCKS of four 32-pixel tiles (128 pixels: whole rows for w <= 128, half a row for
// w = 256, whose +-1 halo is read from the neighbouring half — nothing is written here, there is no race); chunk = blockIdx.x
// takes blocks chunk, chunk + gridDim.x, ... in order.  Per block the workgroup stages in LDS
//   img   64 x CS   eps1 at positions q = p + (p >> log2 w) + 1 (one shared zero position in front of every row and behind the
//                   last; w = 256: positions 0 and 129 hold the halo pixel, or zero at a row end), channel-major.  CS = the
//                   positions (128 + 128 / w + 1, w = 256: 130) rounded up to 3 mod 32: the B read of lane n = 32 ct + j is at
//                   (n / 3) CS + n % 3 + const — bank (3 (n / 3) + n % 3) % 32 = n % 32: conflict-free; the staging write of a
//                   wave is 64 consecutive floats: conflict-free
//   g     64 x 129  the block's dv values, row stride odd: the A read of lane co = 32 mt + j is conflict-free, the staging write
//                   64 consecutive floats
// (bwd_w3_lds_floats() is the ONE statement of it, exported as dcll_conv_lif_backward_w3_lds: 83 008 bytes at w = 2, the largest;
// a tile beyond the stream's end is staged as zeros.)
// Wave (mt, column half, pixel half) = (wave & 1, (wave >> 1) & 1, wave >> 2) keeps the 3 accumulator tiles ct = 3 half + q
// (48 registers) over all blocks of its chunk and runs the pixel pairs [32 half, 32 half + 32) of every block in order; at the
// end the second pixel half goes through LDS and is added to the first: acc(half 0) + acc(half 1).  The bias gradient: wave w
// sums rows co = w + 8 k, lane l the pixels l, l + 64 of every block in order, then the fixed DPP tree (wave_sum_to_lane63).
// Partial rows: part[chunk][co][193] (last = bias gradient), at most 256 chunks — the format k_bwd_reduce[4] and
// dcll_grad_reduce_adam consume.  Every sum has a fixed order: two runs give the same bits, and the open form + the fused
// reduction gives the closed form's bits.  NOT bit-identical to the default path (k_bwd_wgrad): the summation order differs.
// The first layer (c_in = 1, 3 + 1 columns) keeps the generic k_bwd_wgrad inside the new entry points (the launch log says so).
constexpr int BW_THREADS = 512, BW_PB = 128, BW_GLD = 129, BW_MAX_CHUNKS = 256;

static inline int bwd_w3_npos(int w) { return w == 256 ? BW_PB + 2 : BW_PB + BW_PB / w + 1; }
static inline int bwd_w3_cs(int w) { return ((bwd_w3_npos(w) - 3 + 31) / 32) * 32 + 3; }
// floats of a workgroup: the image, the dv block, the tile table (4 x (offset as two words, valid, sample pixel) = 16 words)
static inline long bwd_w3_lds_floats(const dcll_conv_desc *d) { return 64L * bwd_w3_cs(d->w) + 64L * BW_GLD + 16; }

int dcll_bwd_w3_check(const dcll_conv_desc *d, const char *who) { return dcll_step_w3_check(d, who); }

// LDS bytes of k_bwd_wgrad_w3 (c_in = 1: of the generic k_bwd_wgrad these entry points keep for that layer); 0 = not served
extern "C" int64_t dcll_conv_lif_backward_w3_lds(const dcll_conv_desc *d)
{
    if (dcll_bwd_w3_check(d, "dcll_conv_lif_backward_w3_lds") != DCLL_OK) return 0;
    if (d->c_in == 64) return bwd_w3_lds_floats(d) * 4;
    const int WP = d->w + 2, rows_fit = (48 * 1024 / 4 - 4 * 65) / WP;     // (conv_lif_backward_impl's row bands, kh = 1)
    return ((long)(rows_fit < d->h ? rows_fit : d->h) * WP + 4 * 65) * 4;
}

__global__ __launch_bounds__(BW_THREADS) void k_bwd_wgrad_w3(const float *__restrict__ gvf, const float *__restrict__ eps1,
                                                            float *__restrict__ part, int ntot, int HW, int w, int logW, int CS)
{
    extern __shared__ float lds[];
    float *img = lds, *gl = lds + 64 * CS;
    int *tab = (int *)(gl + 64 * BW_GLD);                // per tile tt: [4 tt] offset lo, hi; valid; first pixel in its sample
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = wv & 1, chalf = (wv >> 1) & 1, phalf = wv >> 2;
    const int NTS = HW >> 5, nblk = (ntot + 3) >> 2;
    const int npos = w == 256 ? BW_PB + 2 : BW_PB + (BW_PB >> logW) + 1;
    // position -> pixel of the block, the same for every block: -2 = zero, -1 / 128 = halo pixel of a half row (w = 256)
    int pmap[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int q = lane + 64 * s, k = q / (w + 1), r = q - k * (w + 1);
        pmap[s] = q >= npos ? -2 : r == 0 ? ((k == 0 && w == 256) ? -1 : -2) : k * w + r - 1;
    }
    int bbase[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int n = 32 * (3 * chalf + q) + j;
        bbase[q] = (n / 3) * CS + n % 3 - 1 + h;
    }
    const float *ga = gl + (32 * mt + j) * BW_GLD + h;
    f32x16 acc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
    float bacc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        if (tid < 4) {          // (every wave is past the staging of the block before: nothing reads the table now)
            const int G = blk * 4 + tid, val = G < ntot, b = val ? G / NTS : 0, m = val ? G - b * NTS : 0;
            const long off = (long)b * 64 * HW + 32 * m;
            tab[4 * tid] = (int)(unsigned)off, tab[4 * tid + 1] = (int)(off >> 32), tab[4 * tid + 2] = val, tab[4 * tid + 3] = 32 * m;
        }
        __syncthreads();        // the table is written, the chains of the block before are done with img and g
        for (int c = wv; c < 64; c += 8) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int i = lane + 64 * s, tt = i >> 5;
                const long off = ((long)tab[4 * tt + 1] << 32) | (unsigned)tab[4 * tt];
                gl[c * BW_GLD + i] = tab[4 * tt + 2] ? gvf[off + (long)c * HW + (i & 31)] : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int q = lane + 64 * s, pi = pmap[s];
                if (q >= npos) continue;
                float e = 0.0f;
                if (pi != -2) {
                    // the halo of a half row lies in the sample (and row) of tile 0 / 3: zero where the row ends there
                    const int tt = pi < 0 ? 0 : pi >= BW_PB ? 3 : pi >> 5, dp = pi - 32 * tt;
                    const long off = ((long)tab[4 * tt + 1] << 32) | (unsigned)tab[4 * tt];
                    const bool in_row = (dp >= 0 && dp < 32) || ((tab[4 * tt + 3] + dp) & (w - 1)) != (dp < 0 ? w - 1 : 0);
                    if (tab[4 * tt + 2] && in_row) e = eps1[off + (long)c * HW + dp];
                }
                img[c * CS + q] = e;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            bacc[k] += gl[(wv + 8 * k) * BW_GLD + lane];
            bacc[k] += gl[(wv + 8 * k) * BW_GLD + lane + 64];
        }
#pragma unroll 4
        for (int pp = 32 * phalf; pp < 32 * phalf + 32; ++pp) {
            const int qq = 2 * pp + ((2 * pp) >> logW) + 1;
            const float a = ga[2 * pp];
            float bv[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) bv[q] = img[bbase[q] + qq];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[q], acc[q], 0, 0, 0);
        }
    }
    // ---- the two pixel halves through LDS (the staging area is free), half 0 + half 1
    __syncthreads();
    if (phalf == 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) lds[(((wv - 4) * 3 + q) * 16 + r) * 64 + lane] = acc[q][r];
    }
    __syncthreads();
    float *prow = part + (long)blockIdx.x * 64 * 193;
    if (phalf == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
                prow[co * 193 + 32 * (3 * chalf + q) + j] = acc[q][r] + lds[((wv * 3 + q) * 16 + r) * 64 + lane];
            }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float tot = wave_sum_to_lane63(bacc[k]);
        if (lane == 63) prow[(wv + 8 * k) * 193 + 192] = tot;
    }
}

// gvf: the dv plane (B, 64, h, w); part: room for *nchunk partial rows on entry, the number written on return.  launch ==
// false: the checks and the LDS reservation only (conv_lif_backward_impl calls this form before its first launch)
int dcll_launch_bwd_wgrad_w3(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B, long *nchunk,
                             hipStream_t st, bool launch)
{
    const char *who = "dcll_conv_lif_backward_w3";
    const long ntot = (long)B * ((long)d->h * d->w / 32);
    if (ntot > 0x7fffffffL - 8) return fail(DCLL_ERR_INVALID, "batch x tiles exceeds the grid limit", who);
    long nc = *nchunk;
    const long nblk = (ntot + 3) / 4;
    if (nc > BW_MAX_CHUNKS) nc = BW_MAX_CHUNKS;
    if (nc > nblk) nc = nblk;
    const int CS = bwd_w3_cs(d->w);
    const size_t lds_bytes = (size_t)(64L * CS + 64L * BW_GLD + 16) * 4;
    // each launch against the exported bytes; the half-sum area (4 waves x 3 tiles x 1024 floats) lies inside the staging area
    if (d->c_in != 64 || (int64_t)lds_bytes != dcll_conv_lif_backward_w3_lds(d) || 64L * CS + 64L * BW_GLD < 12 * 1024 ||
        CS < bwd_w3_npos(d->w) || nc < 1)
        return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_w3: launch layout outside the predicate's", who);
    static std::mutex mu;
    static bool reserved[SW_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) {
        (void)hipGetLastError();
        return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_w3: no current device");
    }
    {
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= SW_MAX_DEVICES || !reserved[dev]) {      // (the largest layout of any served width: asked for once per device)
            if (hipFuncSetAttribute((const void *)k_bwd_wgrad_w3, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((64L * 195 + 64L * BW_GLD + 16) * 4)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_w3: cannot reserve its LDS");
            }
            if (dev < SW_MAX_DEVICES) reserved[dev] = true;
        }
    }
    *nchunk = nc;
    if (!launch) return DCLL_OK;
    int logW = 0;
    while ((1 << logW) < d->w) ++logW;
    hipLaunchKernelGGL(k_bwd_wgrad_w3, dim3((unsigned)nc), dim3(BW_THREADS), lds_bytes, st, gvf, eps1, part, (int)ntot,
                       d->h * d->w, d->w, logW, CS);
    HIP_CHECK_LAUNCH("k_bwd_wgrad_w3");
    return DCLL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_bwd_wgrad_w3f — the weight gradient of the FIRST layer (c_in 1 -> 64) of that geometry
// (dcll_conv_lif_backward_w3f[_open]; found by symbol lookup, the ABI version stays 10):
//
//   dW[co][kx] = sum_{b,p} g[b,co,p] * eps1[b,0,p + kx - 1]  (kx = 0, 1, 2; zero beyond a row's ends),   db[co] = sum g
//
// 64 x 3 + 64 numbers reduced over B h w pixels: not matrix work but a streaming reduction of the dv plane g (B 64 h w floats,
// read once) against the one-channel eps1 plane (B h w floats, cache-resident).  Registers only: nothing is written during the
// sweep, so a lane reads the +-1 neighbours of its pixels straight from global memory — no LDS image, no row-ownership rule.
// The flattened pixel stream P = b h w + p (B x H W pixels) is cut into JOBS of WF_PB = 128 consecutive pixels (h w % 32 == 0:
// a job may span samples and the last one may be short by a multiple of 32; a lane's 4 pixels never leave a row pair, let alone
// a sample).  chunk = blockIdx.x takes the jobs chunk, chunk + nchunk, chunk + 2 nchunk, ... — the chunk's job list i = 0, 1, ...
// Wave (cg, jp) = (wave & 3, wave >> 2) of the 512-thread workgroup owns the 16 output channels 16 cg .. 16 cg + 15 and the
// jobs i = jp, jp + 2, ... of the list; lane (ch, q) = (lane >> 5, lane & 31) owns the channels 16 cg + 8 ch + c, c = 0 .. 7,
// and the pixels 128 J + 4 q + j, j = 0 .. 3 of every job J of its wave: 8 independent 16-byte loads of g per lane and job.
// SUMMATION ORDER of one output (co, column) of chunk k — restated on the CPU by tests/bwd_w3f_cases.py:
//   1. lane (q), wave jp: four accumulators a0, a1, a2 (taps) and ab (bias) start at 0 and take the wave's jobs in increasing i
//      and inside a job the pixels j = 0, 1, 2, 3 in order: a0 = fma(g, eL, a0), a1 = fma(g, eC, a1), a2 = fma(g, eR, a2),
//      ab = ab + g, with eL / eR = the left / right neighbour in the row, 0 at x = 0 / x = w - 1;
//   2. the 32 lanes q of a half wave by the fixed DPP tree (half_sum_to_lane31: v += v[q ^ 1]; v += v[q ^ 2]; v += mirror in
//      the group of 8; v += mirror in the row of 16; row 1 += row 0);
//   3. the two waves of a channel group through LDS: total(jp 0) + total(jp 1).
// Partial rows: part[chunk][co][4] = (kx 0, kx 1, kx 2, bias): the rowlen-4 format k_bwd_reduce[4] and dcll_grad_reduce_adam
// consume; at most WF_MAX_CHUNKS = 256 chunks and at most one per job.  Every sum has a fixed order: two runs give the same
// bits, and the open form + the fused reduction gives the closed form's bits.  NOT bit-identical to k_bwd_wgrad (the default
// path and dcll_conv_lif_backward_w3 on this layer): the summation order differs.
// Two forms with the SAME order, hence the same bits: 16-byte loads of g and eps1 where both pointers are 16-byte aligned
// (h w % 4 == 0 keeps every lane's 4 pixels aligned then), scalar loads otherwise (the ABI asks for 4-byte alignment only).
constexpr int WF_THREADS = 512, WF_PB = 128, WF_MAX_CHUNKS = 256;

// sum over each 32-lane half of the wave; valid in lanes 31 and 63 (wave_sum_to_lane63 without its last step)
__device__ __forceinline__ float half_sum_to_lane31(float v)
{
    v = dpp_add<0xB1, 0xF>(v);       // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xF>(v);       // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xF>(v);      // row_half_mirror
    v = dpp_add<0x140, 0xF>(v);      // row_mirror      -> every lane holds its 16-lane row sum
    v = dpp_add<0x142, 0xA>(v);      // row_bcast15     -> rows 1,3 += previous row
    return v;
}

template <bool ALIGNED>
__device__ __forceinline__ void wf_load4(const float *__restrict__ p, float (&r)[4])
{
    if constexpr (ALIGNED) {
        const f32x4 t = *(const f32x4 *)p;
        r[0] = t[0], r[1] = t[1], r[2] = t[2], r[3] = t[3];
    } else {
        r[0] = p[0], r[1] = p[1], r[2] = p[2], r[3] = p[3];
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(WF_THREADS) void k_bwd_wgrad_w3f(const float *__restrict__ gvf, const float *__restrict__ eps1,
                                                             float *__restrict__ part, int ntot, int HW, int w)
{
    __shared__ float red[4 * 16 * 4];                   // the totals of the waves jp = 1: [cg][channel of the group][column]
    const int tid = threadIdx.x, lane = tid & 63, ch = lane >> 5, q = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = wv & 3, jp = wv >> 2;
    const int NTS = HW >> 5;                            // 32-pixel tiles per sample
    const int njob = (ntot + 3) >> 2;                   // 4 tiles per job; ntot = B NTS < 2^31 - 8 (the launcher)
    const int c0 = 16 * cg + 8 * ch;
    float a0[8], a1[8], a2[8], ab[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) a0[c] = a1[c] = a2[c] = ab[c] = 0.0f;

    for (long J = (long)blockIdx.x + (long)jp * gridDim.x; J < njob; J += 2L * gridDim.x) {
        const int G = (int)J * 4 + (q >> 3);            // the 32-pixel tile of this lane's 4 pixels
        if (G >= ntot) continue;                        // (the short last job)
        const int b = G / NTS, ps = (G - b * NTS) * 32 + 4 * (q & 7);   // sample, first of the 4 pixels in it
        const float *ep = eps1 + (long)b * HW + ps;
        const float *gp = gvf + ((long)b * 64 + c0) * HW + ps;
        float g[8][4], e[6];
#pragma unroll
        for (int c = 0; c < 8; ++c) wf_load4<ALIGNED>(gp + (long)c * HW, g[c]);
        {
            float ec[4];
            wf_load4<ALIGNED>(ep, ec);
            e[1] = ec[0], e[2] = ec[1], e[3] = ec[2], e[4] = ec[3];
        }
        // the neighbours outside the 4 pixels: read only where they lie in the row (then in the sample); w >= 4: the 4 pixels
        // are in one row; w = 2: two rows, the masks below cut every neighbour
        const int x0 = ps & (w - 1);
        e[0] = x0 != 0 ? ep[-1] : 0.0f;
        e[5] = ((x0 + 3) & (w - 1)) != w - 1 ? ep[4] : 0.0f;
        float eL[4], eR[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = (x0 + j) & (w - 1);
            eL[j] = x != 0 ? e[j] : 0.0f;
            eR[j] = x != w - 1 ? e[j + 2] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0[c] = __builtin_fmaf(g[c][j], eL[j], a0[c]);
                a1[c] = __builtin_fmaf(g[c][j], e[j + 1], a1[c]);
                a2[c] = __builtin_fmaf(g[c][j], eR[j], a2[c]);
                ab[c] = ab[c] + g[c][j];
            }
    }
    // ---- the 32 lanes of a half wave (fixed tree), then the two waves of the channel group: jp 0 + jp 1
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        a0[c] = half_sum_to_lane31(a0[c]);
        a1[c] = half_sum_to_lane31(a1[c]);
        a2[c] = half_sum_to_lane31(a2[c]);
        ab[c] = half_sum_to_lane31(ab[c]);
    }
    float *rr = red + (cg * 16 + 8 * ch) * 4;
    if (jp == 1 && q == 31) {
#pragma unroll
        for (int c = 0; c < 8; ++c) rr[4 * c] = a0[c], rr[4 * c + 1] = a1[c], rr[4 * c + 2] = a2[c], rr[4 * c + 3] = ab[c];
    }
    __syncthreads();
    if (jp == 0 && q == 31) {
        float *prow = part + ((long)blockIdx.x * 64 + c0) * 4;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            prow[4 * c] = a0[c] + rr[4 * c];
            prow[4 * c + 1] = a1[c] + rr[4 * c + 1];
            prow[4 * c + 2] = a2[c] + rr[4 * c + 2];
            prow[4 * c + 3] = ab[c] + rr[4 * c + 3];
        }
    }
}

// gvf: the dv plane (B, 64, h, w); part: room for *nchunk partial rows of 64 x 4 floats on entry, the number written on
// return.  launch == false: the checks only (conv_lif_backward_impl calls this form before its first launch)
int dcll_launch_bwd_wgrad_w3f(const dcll_conv_desc *d, const float *gvf, const float *eps1, float *part, int32_t B, long *nchunk,
                              hipStream_t st, bool launch)
{
    const char *who = "dcll_conv_lif_backward_w3f";
    const long ntot = (long)B * ((long)d->h * d->w / 32);
    if (ntot > 0x7fffffffL - 8) return fail(DCLL_ERR_INVALID, "batch x tiles exceeds the grid limit", who);
    long nc = *nchunk;
    const long njob = (ntot + WF_PB / 32 - 1) / (WF_PB / 32);
    if (nc > WF_MAX_CHUNKS) nc = WF_MAX_CHUNKS;
    if (nc > njob) nc = njob;
    if (d->c_in != 1 || d->c_out != 64 || ((long)d->h * d->w) % 32 != 0 || d->w < 2 || (d->w & (d->w - 1)) != 0 || nc < 1)
        return fail(DCLL_ERR_LAUNCH, "k_bwd_wgrad_w3f: launch layout outside the predicate's", who);
    *nchunk = nc;
    if (!launch) return DCLL_OK;
    const bool aligned = (((uintptr_t)gvf | (uintptr_t)eps1) & 15) == 0;
    if (aligned)
        hipLaunchKernelGGL(k_bwd_wgrad_w3f<true>, dim3((unsigned)nc), dim3(WF_THREADS), 0, st, gvf, eps1, part, (int)ntot,
                           d->h * d->w, d->w);
    else
        hipLaunchKernelGGL(k_bwd_wgrad_w3f<false>, dim3((unsigned)nc), dim3(WF_THREADS), 0, st, gvf, eps1, part, (int)ntot,
                           d->h * d->w, d->w);
    HIP_CHECK_LAUNCH(aligned ? "k_bwd_wgrad_w3f" : "k_bwd_wgrad_w3f (unaligned)");
    return DCLL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_bwd_dv_w3 — the dv plane of a layer of that geometry (dcll_conv_lif_backward_w3_ex[_open] with DCLL_W3_DV; found by symbol
// lookup, the ABI version stays 10): k_bwd_dv (dcll_hip.hip) for pooling (1,2) on an even width, where the geometry is flat —
// pooled position k of a sample's K = 64 h w / 2 is the un-pooled pair 2k, 2k + 1 of its 2K elements, K % 1024 == 0 (h w % 32
// == 0): no tail in k, only the batch is ragged.  A thread owns TWO consecutive pooled positions — one 16-byte load of v (and of
// g_v), one 16-byte store of dv, 8-byte loads of g_pv and of every i2o_W row — with its NP x 2 readout weights in registers
// (NP = target rounded up to 8; bwd_dv_nopool_body's trick) over a chunk of DW_PB samples, whose g_p rows go through LDS and
// come back as broadcasts; the loads of DW_G samples are issued before the first is used.  Workgroup = 512 pooled positions x
// one batch chunk; grid (K / 512, ceil(B / DW_PB)).
// ARITHMETIC = k_bwd_dv's, bit for bit (-ffp-contract=off; tests/dv_w3_cases.py restates it): pv = sigmoidf_dev(v) of both
// elements; element 0 wins unless pv1 > pv0 (the comparison is on the sigmoids: a first-maximum tie goes to element 0); the
// winner's g = (g_pv or 0) + acc, acc = 0, acc = fmaf(g_p[b][n], i2o_W[n][k], acc), n = 0 .. target - 1 in that order (no sum
// without g_p), the loser's g = 0; out = g * pv * (1 - pv), + g_v where given.  The padding terms n >= target are
// fmaf(-0, +0, acc): the product is -0, and x + (-0) == x for EVERY x, -0 included (a +0 product would turn an acc of -0 —
// reachable by underflow — into +0).
// Two forms with the same bits: the vector loads above where v, dv and g_v are 16-byte and g_pv and i2o_W 8-byte aligned (K is
// even: every row then is), scalar loads otherwise — the ABI asks for 4-byte alignment only.
#ifndef DW_PER_BLOCK            // samples per workgroup (experiments/build_variant.sh -DDW_PER_BLOCK=..: the sweep in
#define DW_PER_BLOCK 8          // profiles/r15_w3_dv_timing.txt); restated by tests/dv_w3_cases.py
#endif
constexpr int DW_THREADS = 256, DW_POS = 2 * DW_THREADS, DW_PB = DW_PER_BLOCK, DW_G = 4;

template <bool ALIGNED>
__device__ __forceinline__ void dw_load2(const float *__restrict__ p, float (&r)[2])
{
    if constexpr (ALIGNED) {
        const f32x2 t = *(const f32x2 *)p;
        r[0] = t[0], r[1] = t[1];
    } else {
        r[0] = p[0], r[1] = p[1];
    }
}

template <int NP, bool ALIGNED>
__global__ __launch_bounds__(DW_THREADS, NP <= 24 ? 4 : 3) void k_bwd_dv_w3(const int K, const int N, const float *__restrict__ v,
                                                         const float *__restrict__ g_p, const float *__restrict__ g_pv,
                                                         const float *__restrict__ g_v, const float *__restrict__ i2o_W,
                                                         float *__restrict__ gvf, const int B)
{
    __shared__ __attribute__((aligned(16))) float gp[DW_PB][32];
    const int b0 = (int)blockIdx.y * DW_PB, b1 = min(B, b0 + DW_PB);
    for (int e = threadIdx.x; e < DW_PB * 32; e += DW_THREADS) {
        const int bb = b0 + (e >> 5), n = e & 31;
        gp[e >> 5][n] = (g_p && n < N && bb < b1) ? g_p[(long)bb * N + n] : -0.0f;
    }
    __syncthreads();
    const int k = (int)blockIdx.x * DW_POS + 2 * threadIdx.x;          // (K % DW_POS == 0: every thread has its two positions)
    float wk[NP][2];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        wk[n][0] = wk[n][1] = 0.0f;
        if (g_p && n < N) dw_load2<ALIGNED>(i2o_W + (long)n * K + k, wk[n]);
    }
    for (int bg = b0; bg < b1; bg += DW_G) {
        float vv[DW_G][4], gg[DW_G][2], ga[DW_G][4];
#pragma unroll
        for (int q = 0; q < DW_G; ++q) {
            const int b = min(bg + q, b1 - 1);
            const long ip = (long)b * K + k;
            wf_load4<ALIGNED>(v + 2 * ip, vv[q]);
            gg[q][0] = gg[q][1] = 0.0f;
            if (g_pv) dw_load2<ALIGNED>(g_pv + ip, gg[q]);
            ga[q][0] = ga[q][1] = ga[q][2] = ga[q][3] = 0.0f;
            if (g_v) wf_load4<ALIGNED>(g_v + 2 * ip, ga[q]);
        }
#pragma unroll
        for (int q = 0; q < DW_G; ++q) {
            const int b = min(bg + q, b1 - 1);
            float g[2] = {gg[q][0], gg[q][1]};
            if (g_p) {
                float acc[2] = {0.0f, 0.0f};
#pragma unroll
                for (int n4 = 0; n4 < NP; n4 += 4) {
                    const f32x4 gq = *(const f32x4 *)&gp[b - b0][n4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[0] = __builtin_fmaf(gq[u], wk[n4 + u][0], acc[0]);
                        acc[1] = __builtin_fmaf(gq[u], wk[n4 + u][1], acc[1]);
                    }
                }
                g[0] += acc[0], g[1] += acc[1];
            }
            float o[4];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float pv0 = sigmoidf_dev(vv[q][2 * p]), pv1 = sigmoidf_dev(vv[q][2 * p + 1]);
                const bool right = pv1 > pv0;
                const float g0 = right ? 0.0f : g[p], g1 = right ? g[p] : 0.0f;
                o[2 * p] = g0 * pv0 * (1.0f - pv0);
                o[2 * p + 1] = g1 * pv1 * (1.0f - pv1);
            }
            if (g_v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] += ga[q][j];
            }
            if (bg + q < b1) {
                float *op = gvf + 2 * ((long)b * K + k);
                if constexpr (ALIGNED) {
                    *(f32x4 *)op = f32x4{o[0], o[1], o[2], o[3]};
                } else {
                    op[0] = o[0], op[1] = o[1], op[2] = o[2], op[3] = o[3];
                }
            }
        }
    }
}

// the dv launch of a backward call of that geometry (dcll_bwd_w3_check passed).  *form = the kernel's name for the launch log,
// nullptr = not served (target > 32, or more batch chunks than a grid's y takes): the caller keeps k_bwd_dv
int dcll_launch_bwd_dv_w3(const dcll_conv_desc *d, const float *v, const float *g_p, const float *g_pv, const float *g_v,
                          const float *i2o_W, float *gvf, int32_t B, hipStream_t st, const char **form)
{
    static_assert(DW_PB >= 1 && DW_PB % DW_G == 0, "a chunk is whole groups of samples in flight");
    *form = nullptr;
    const long K = 32L * d->h * d->w;                      // 64 channels x h x w / 2 pooled positions; % 1024 == 0
    const long nby = ((long)B + DW_PB - 1) / DW_PB;
    if (d->target > 32 || nby > 65535) return DCLL_OK;
    if (d->c_out != 64 || d->pool_h != 1 || d->pool_w != 2 || (d->w & 1) || K % DW_POS != 0 || K > 0x7fffffffL / 2 || !v || !gvf ||
        (g_p && !i2o_W))
        return fail(DCLL_ERR_LAUNCH, "k_bwd_dv_w3: launch layout outside the predicate's", "dcll_conv_lif_backward_w3_ex");
    const bool aligned = ((((uintptr_t)v | (uintptr_t)gvf | (uintptr_t)g_v) & 15) | (((uintptr_t)g_pv | (uintptr_t)i2o_W) & 7)) == 0;
    const dim3 grid((unsigned)(K / DW_POS), (unsigned)nby);
#define DCLL_DVW3(NP_)                                                                                                  \
    do {                                                                                                                \
        if (aligned)                                                                                                    \
            hipLaunchKernelGGL((k_bwd_dv_w3<NP_, true>), grid, dim3(DW_THREADS), 0, st, (int)K, d->target, v, g_p, g_pv, g_v,   \
                               i2o_W, gvf, B);                                                                          \
        else                                                                                                            \
            hipLaunchKernelGGL((k_bwd_dv_w3<NP_, false>), grid, dim3(DW_THREADS), 0, st, (int)K, d->target, v, g_p, g_pv, g_v,  \
                               i2o_W, gvf, B);                                                                          \
    } while (0)
    if (d->target <= 8) DCLL_DVW3(8);
    else if (d->target <= 16) DCLL_DVW3(16);
    else if (d->target <= 24) DCLL_DVW3(24);
    else DCLL_DVW3(32);
#undef DCLL_DVW3
    *form = aligned ? "k_bwd_dv_w3" : "k_bwd_dv_w3 (unaligned)";
    return DCLL_OK;
}
