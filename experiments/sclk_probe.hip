// What does the shader clock do under a full fp32-MFMA load?  (diagnostic, not product)   ./sclk_probe
// Every wave runs a dependent chain of v_mfma_f32_32x32x2_f32 (optionally with LDS operand reads, as the layer kernels
// do) and reads both timers before and after: s_memtime counts shader-clock cycles, s_memrealtime the constant 100 MHz
// reference.  Their ratio is the average shader clock DURING the kernel; MFMAs / s_memtime cycles is the issue rate in
// the hardware's own clock.  Peak figures quoted against 2.4 GHz assume the clock holds under this load.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
#include <string.h>
#include <stdlib.h>
#include <type_traits>
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int LDSOPS>
__global__ __launch_bounds__(256) void k_probe(unsigned long long *out, float *sink, int iters)
{
    __shared__ float lds[8192];
    for (int i = threadIdx.x; i < 8192; i += 256) lds[i] = 1e-3f * (i & 7);
    __syncthreads();
    f32x16 a0, a1;
    for (int r = 0; r < 16; ++r) a0[r] = a1[r] = 0.0f;
    const int lane = threadIdx.x & 63;
    const unsigned long long t0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    float x = 1.0f + lane * 1e-6f, y = 0.5f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (LDSOPS == 1) {                 // scattered addresses (conflicts), computed per read
                x = lds[(lane + 67 * u + it) & 8191];
                y = lds[(lane * 2 + 129 * u + it) & 8191];
            } else if (LDSOPS == 2) {          // conflict-free, immediate offsets from one lane base
                const float *pl = lds + lane + (it & 7) * 16;
                x = pl[64 * u];
                y = pl[64 * u + 2048];
            } else if (LDSOPS == 3) {          // the layer kernels' pattern: A fragment conflict-free, B fragment from the
                const float *pa = lds + lane + (it & 7) * 16;                  // 19-float-row image (2-way on 3 banks)
                const float *pb = lds + 4096 + (lane >> 5) * 361 + ((lane & 31) >> 4) * 19 + (lane & 15) + (it & 7) * 19;
                x = pa[64 * u];
                y = pb[u];
            }
            a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(y, x, a1, 0, 0, 0);
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.0f;
    for (int r = 0; r < 16; ++r) s += a0[r] + a1[r];
    if (s == 12345.678f) sink[0] = s;
    if (lane == 0) {
        const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
        out[2 * w] = t1 - t0;
        out[2 * w + 1] = r1 - r0;
    }
}
// ---- "mix" modes: what do the NON-MFMA instructions of k_lif_seq_c32d's chain loop cost?   ./sclk_probe mix
// A wave walks the chain of a 14-row position (two adjacent image rows, 7 tap rows each: 98 MFMAs per channel pair into two
// alternating accumulators) with the kernel's operand delivery around it: B fragments from the 19-float-row images of pitch
// 9744 (base + immediate, one row ahead), A fragments streamed from an L2-resident copy (one channel pair ahead, refetched
// right after their use, one SGPR offset per load).
//   MIX 0  today's walk: by (tap row, kx), each tile reads its own B fragment: 98 LDS dwords and 49 buffer_load_dword
//   MIX 1  B shared: by (source row, kx), one B fragment feeds both tiles: 56 LDS dwords, A as in 0
//   MIX 2  MIX 1 + wide A loads: a tap row is [lane][8] floats, one dwordx4 + one dwordx3 per row
constexpr int MX_ROWF = 19, MX_CHF = 16 * MX_ROWF, MX_IMGP = 9744, MX_LDS = 2 * MX_IMGP;
constexpr int MX_WFLOATS = 16 * 49 * 64, MX_WFLOATS8 = 16 * 7 * 64 * 8;
// largest LDS index: lane base (h = 1, image 1, column 15) + channel pair 15 + source row 7, kx = 6
static_assert(MX_CHF + MX_IMGP + 15 + 15 * 2 * MX_CHF + 7 * MX_ROWF + 6 < MX_LDS, "B reads inside the two images");
static_assert(7 * MX_ROWF + 6 < 256, "B offsets within ds_read2_b32's range");
typedef __attribute__((address_space(3))) const float lds_cf;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x3 __attribute__((ext_vector_type(3)));
template <int R0, int R1, class F>
__device__ __forceinline__ void sfor(F &&f)
{
    if constexpr (R0 < R1) { f(std::integral_constant<int, R0>{}); sfor<R0 + 1, R1>(f); }
}
template <int MIX, int NT>
__global__ __launch_bounds__(NT) void k_mix(const float *__restrict__ wfrag, unsigned wbytes, float *sink, int iters)
{
    __shared__ float lds[MX_LDS];
    for (int i = threadIdx.x; i < MX_LDS; i += NT) lds[i] = 1e-3f * (i & 7);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc((void *)wfrag, 0, (int)wbytes, 0x00020000);
    const unsigned wlane = (MIX == 2 ? 32u : 4u) * lane;
    constexpr int NKX = MIX == 2 ? 8 : 7;
    constexpr unsigned ROWB = MIX == 2 ? 64u * 32u : 7u * 256u, CPB = 7u * ROWB;       // bytes of a tap row / a channel pair
    float wb[7][NKX];
    auto load_a = [&](auto KYC, const unsigned wo) {
        constexpr int KY = decltype(KYC)::value;
        if constexpr (MIX == 2) {
            const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane, wo + KY * ROWB, 0));
            const f32x3 r = __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(wrs, wlane + 16u, wo + KY * ROWB, 0));
            wb[KY][0] = q[0]; wb[KY][1] = q[1]; wb[KY][2] = q[2]; wb[KY][3] = q[3];
            wb[KY][4] = r[0]; wb[KY][5] = r[1]; wb[KY][6] = r[2];
        } else {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx)
                wb[KY][kx] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, wlane, wo + (KY * 7 + kx) * 256, 0));
        }
    };
    sfor<0, 7>([&](auto KYC) { load_a(KYC, 0u); });
    f32x16 accA, accB;
    for (int r = 0; r < 16; ++r) accA[r] = accB[r] = 0.0f;
    lds_cf *ib = (lds_cf *)(lds + h * MX_CHF + (j >> 4) * MX_IMGP + (j & 15));
    asm volatile("" : "+v"(ib));
    if constexpr (MIX == 0) {
        float bqA[2][7], bqB[2][7];
        auto fetch_b = [&](auto SETC, auto KYC, lds_cf *base) {
            constexpr int SET = decltype(SETC)::value, KY = decltype(KYC)::value;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                bqA[SET][kx] = base[KY * MX_ROWF + kx];
                bqB[SET][kx] = base[(KY + 1) * MX_ROWF + kx];
            }
        };
        fetch_b(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, ib);
#pragma nounroll
        for (int it = 0; it < iters; ++it) {
            const unsigned wnext = (unsigned)((it + 1) & 15) * CPB;
            lds_cf *cur = ib + (it & 15) * 2 * MX_CHF, *nxt = ib + ((it + 1) & 15) * 2 * MX_CHF;
            asm volatile("" : "+v"(cur), "+v"(nxt));
            sfor<0, 7>([&](auto KYC) {
                constexpr int KY = decltype(KYC)::value;
                if constexpr (KY < 6) fetch_b(std::integral_constant<int, (KY + 1) & 1>{}, std::integral_constant<int, KY + 1>{}, cur);
                else fetch_b(std::integral_constant<int, (KY + 1) & 1>{}, std::integral_constant<int, 0>{}, nxt);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    accA = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[KY][kx], bqA[KY & 1][kx], accA, 0, 0, 0);
                    accB = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[KY][kx], bqB[KY & 1][kx], accB, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                load_a(KYC, wnext);
                __builtin_amdgcn_sched_barrier(0);
            });
            // (7 tap rows: the set of tap row 0 alternates from one channel pair to the next; two pairs per trip keep it fixed)
            const unsigned wnext2 = (unsigned)((it + 2) & 15) * CPB;
            lds_cf *nx2 = ib + ((it + 2) & 15) * 2 * MX_CHF;
            asm volatile("" : "+v"(nx2));
            sfor<0, 7>([&](auto KYC) {
                constexpr int KY = decltype(KYC)::value;
                if constexpr (KY < 6) fetch_b(std::integral_constant<int, KY & 1>{}, std::integral_constant<int, KY + 1>{}, nxt);
                else fetch_b(std::integral_constant<int, KY & 1>{}, std::integral_constant<int, 0>{}, nx2);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    accA = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[KY][kx], bqA[(KY + 1) & 1][kx], accA, 0, 0, 0);
                    accB = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[KY][kx], bqB[(KY + 1) & 1][kx], accB, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                load_a(KYC, wnext2);
                __builtin_amdgcn_sched_barrier(0);
            });
            ++it;
        }
    } else {
        // source rows s = 0..7 of the pair: tile A takes tap row s (s < 7), tile B tap row s - 1 (s > 0); 8 rows per channel
        // pair, so the two B register sets keep their places from one pair to the next
        float bq[2][7];
        auto fetch_b = [&](auto SETC, auto SC, lds_cf *base) {
            constexpr int SET = decltype(SETC)::value, S = decltype(SC)::value;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) bq[SET][kx] = base[S * MX_ROWF + kx];
        };
        fetch_b(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, ib);
#pragma nounroll
        for (int it = 0; it < iters; ++it) {
            const unsigned wnext = (unsigned)((it + 1) & 15) * CPB;
            lds_cf *cur = ib + (it & 15) * 2 * MX_CHF, *nxt = ib + ((it + 1) & 15) * 2 * MX_CHF;
            asm volatile("" : "+v"(cur), "+v"(nxt));
            sfor<0, 8>([&](auto SC) {
                constexpr int S = decltype(SC)::value;
                if constexpr (S < 7) fetch_b(std::integral_constant<int, (S + 1) & 1>{}, std::integral_constant<int, S + 1>{}, cur);
                else fetch_b(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, nxt);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    if constexpr (S < 7) accA = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[S < 7 ? S : 0][kx], bq[S & 1][kx], accA, 0, 0, 0);
                    if constexpr (S > 0) accB = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[S > 0 ? S - 1 : 0][kx], bq[S & 1][kx], accB, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // tap row S - 1 has had its later use (tile B's): refetch it for the next channel pair
                if constexpr (S > 0) load_a(std::integral_constant<int, (S > 0 ? S - 1 : 0)>{}, wnext);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
    }
    float s = 0.0f;
    for (int r = 0; r < 16; ++r) s += accA[r] + accB[r];
    if (s == 12345.678f) sink[0] = s;
}
template <int MIX, int NT>
static void run_mix(int iters, int reps, const char *what)
{
    const size_t wfloats = MIX == 2 ? MX_WFLOATS8 : MX_WFLOATS;
    std::vector<float> hw(wfloats);
    for (size_t i = 0; i < wfloats; ++i) hw[i] = 1e-3f * (float)((i * 7) % 11);
    float *w, *sink;
    hipMalloc(&w, wfloats * 4); hipMalloc(&sink, 16);
    hipMemcpy(w, hw.data(), wfloats * 4, hipMemcpyHostToDevice);
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    double lo = 1e30, hi = 0, sum = 0;
    for (int rep = 0; rep < reps + 1; ++rep) {          // the first launch warms the clock and is not counted
        hipEventRecord(a);
        hipLaunchKernelGGL((k_mix<MIX, NT>), dim3(256), dim3(NT), 0, 0, w, (unsigned)(wfloats * 4), sink, iters);
        hipEventRecord(b);
        if (hipEventSynchronize(b) != hipSuccess) { printf("%s: launch failed\n", what); exit(1); }
        float ms; hipEventElapsedTime(&ms, a, b);
        const double pct = 256.0 * (NT / 64) * 98.0 * iters * 4096 / (ms * 1e-3) / 157.3e12 * 100;
        if (rep == 0) continue;
        lo = pct < lo ? pct : lo; hi = pct > hi ? pct : hi; sum += pct;
    }
    printf("%-44s %d w/SIMD: %.2f %% of 157.3 TFLOP/s (min %.2f, max %.2f, %d launches)\n", what, NT / 256, sum / reps, lo, hi, reps);
    hipFree(w); hipFree(sink);
}
static int main_mix()
{
    const int iters = 4000, reps = 7;       // iters even: MIX 0 walks two channel pairs per trip
    for (int round = 0; round < 2; ++round) {           // the whole table twice: drift between modes shows as a difference between rounds
        run_mix<0, 256>(iters, reps, "(a) today: 98 LDS dwords, 49 dword A loads");
        run_mix<1, 256>(iters, reps, "(b) B shared: 56 LDS dwords");
        run_mix<2, 256>(iters, reps, "(c) B shared + x4/x3 A loads");
        run_mix<0, 512>(iters, reps, "(a) today: 98 LDS dwords, 49 dword A loads");
        run_mix<1, 512>(iters, reps, "(b) B shared: 56 LDS dwords");
        run_mix<2, 512>(iters, reps, "(c) B shared + x4/x3 A loads");
    }
    return 0;
}
template <int LDSOPS>
static void run(int nwg, int iters, const char *what)
{
    unsigned long long *out; float *sink;
    hipMalloc(&out, (size_t)nwg * 4 * 16); hipMalloc(&sink, 16);
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int rep = 0; rep < 2; ++rep) {
        hipEventRecord(a);
        hipLaunchKernelGGL(k_probe<LDSOPS>, dim3(nwg), dim3(256), 0, 0, out, sink, iters);
        hipEventRecord(b); hipEventSynchronize(b);
        float ms; hipEventElapsedTime(&ms, a, b);
        std::vector<unsigned long long> h((size_t)nwg * 8);
        hipMemcpy(h.data(), out, h.size() * 8, hipMemcpyDeviceToHost);
        double st = 0, rt = 0;
        for (int w = 0; w < nwg * 4; ++w) { st += h[2 * w]; rt += h[2 * w + 1]; }
        const double mfma = 32.0 * iters, waves = nwg * 4.0;
        printf("%-28s %5d WGs: %.2f ms | shader clock %.0f MHz | %.1f shader cycles per MFMA per wave | %.1f TFLOP/s = %.1f %% of 157.3\n", what, nwg, ms,
               st / rt * 100.0, st / waves / mfma, waves * mfma * 4096 / (ms * 1e-3) / 1e12, waves * mfma * 4096 / (ms * 1e-3) / 157.3e12 * 100);
    }
    hipFree(out); hipFree(sink);
}
int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "mix")) return main_mix();
    run<0>(256, 20000, "registers only, 1 wave/SIMD");
    run<0>(512, 20000, "registers only, 2 waves/SIMD");
    run<1>(256, 20000, "LDS scattered, 1 wave/SIMD");
    run<1>(512, 20000, "LDS scattered, 2 waves/SIMD");
    run<2>(256, 20000, "LDS conflict-free, 1 w/SIMD");
    run<2>(512, 20000, "LDS conflict-free, 2 w/SIMD");
    run<3>(256, 20000, "LDS layer pattern, 1 w/SIMD");
    run<3>(512, 20000, "LDS layer pattern, 2 w/SIMD");
    run<0>(64, 20000, "registers only, 64 CUs");
    return 0;
}
