// What a DEPENDENT fp64 issue costs at the occupancy of db_scan_topk_multi, and the clock the loop runs at.  The arithmetic of that kernel is,
// per query vector, four blocks of `v_cvt_f64_f32 w, q[c]` followed at once by the four `v_fmac_f64 acc[rr], w, x[rr][c]` that read w.  Two forms
// of that loop body on 36 independent accumulators per lane (4 rows x 9 queries), every operand in registers, the order pinned by one asm
// statement per instruction:
//   A "dependent": as the kernel has it -- the conversion of element c directly in front of its four users;
//   B "ahead":     the conversion of element c + 1 behind the SECOND fmac of element c (one more fp64 temporary), so that no instruction reads
//                  the result of one of the two instructions in front of it.
// Each at one and at two waves per SIMD (one workgroup of 256 / 512 threads per CU).  EVERY wave stamps s_memtime and s_memrealtime around its
// loop (the stamps go to a buffer of their own).  Printed per configuration, over REPS launches that alternate between the forms, each figure
// the median over workgroups, then min / median / max over launches:
//   * per SIMD: the workgroup's span, from the first wave to enter its loop to the LAST wave to leave it, over the wave-instructions one SIMD
//     issued in it (those of one wave x waves per SIMD) -- what the pipe sustains; a wave the arbiter favours cannot hide the other's bubbles here;
//   * fastest and slowest wave of the workgroup: shader cycles per wave-instruction as that wave saw them;
//   * the in-loop clock, delta s_memtime / delta s_memrealtime x 100 MHz of a wave, after at least two seconds of back-to-back launches;
//   * cross-check without stamps: the launch's time between two events x that clock over the same instruction count (includes launch and ramp).
//   hipcc --offload-arch=gfx950 -O3 -o scripts/ubench/dep_issue_f64 scripts/ubench/dep_issue_f64.hip && scripts/ubench/dep_issue_f64
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr int NQ = 9, R = 4;
constexpr int kInstsPerIter = NQ * (4 + 4 * R);          // 180: 36 conversions, 144 fmac

#define CVT(d, s) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d) : "v"(s))
#define FMAC(a, w, x) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(a) : "v"(w), "v"(x))

template <bool AHEAD> __global__ void __launch_bounds__(512) loop(const float *in, double *sink, unsigned long long *stamps, int iters)
{
    float q[NQ][4];
    double x[R][4], acc[R][NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) q[i][c] = in[(threadIdx.x * 53 + i * 4 + c) & 4095];
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
        for (int c = 0; c < 4; c++) x[rr][c] = in[(threadIdx.x * 29 + 1024 + rr * 4 + c) & 4095];
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
        for (int i = 0; i < NQ; i++) acc[rr][i] = 0.0;

    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int it = 0; it < iters; it++) {
        if (!AHEAD) {
#pragma unroll
            for (int i = 0; i < NQ; i++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    double w;
                    CVT(w, q[i][c]);
#pragma unroll
                    for (int rr = 0; rr < R; rr++) FMAC(acc[rr][i], w, x[rr][c]);
                }
        } else {
            double w[2];
            CVT(w[0], q[0][0]);
#pragma unroll
            for (int e = 0; e < NQ * 4; e++) {
                const int i = e / 4, c = e % 4, n = (e + 1) % (NQ * 4);
                FMAC(acc[0][i], w[e & 1], x[0][c]);
                FMAC(acc[1][i], w[e & 1], x[1][c]);
                if (e + 1 < NQ * 4) CVT(w[(e + 1) & 1], q[n / 4][n % 4]);
                FMAC(acc[2][i], w[e & 1], x[2][c]);
                FMAC(acc[3][i], w[e & 1], x[3][c]);
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    double s = 0;
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
        for (int i = 0; i < NQ; i++) s += acc[rr][i];
    sink[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *o = stamps + 4 * ((size_t)blockIdx.x * 8 + (threadIdx.x >> 6));
        o[0] = t0; o[1] = t1; o[2] = r0; o[3] = r1;
    }
}

struct Sample { double simd, fast, slow, ghz, wall; };   // cycles per wave-instruction: per SIMD over the span, fastest / slowest wave, events

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

template <bool AHEAD> static Sample run(int blocks, int threads, int iters, const float *in, double *sink, unsigned long long *stamps, std::vector<unsigned long long> &h,
                                         hipEvent_t e0, hipEvent_t e1)
{
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(loop<AHEAD>, dim3(blocks), dim3(threads), 0, 0, in, sink, stamps, iters);
    (void)hipEventRecord(e1, 0);
    if (hipMemcpy(h.data(), stamps, sizeof(unsigned long long) * 32 * blocks, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "copy failed\n"); exit(2); }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const int waves = threads / 64, wps = threads / 256;
    const double insts = (double)kInstsPerIter * iters;
    std::vector<double> simd, fast, slow, ghz;
    for (int b = 0; b < blocks; b++) {
        unsigned long long first = ~0ull, last = 0, lo = ~0ull, hi = 0;
        for (int w = 0; w < waves; w++) {
            const unsigned long long *o = h.data() + 4 * ((size_t)b * 8 + w);
            first = std::min(first, o[0]); last = std::max(last, o[1]);
            lo = std::min(lo, o[1] - o[0]); hi = std::max(hi, o[1] - o[0]);
            ghz.push_back((double)(o[1] - o[0]) / (double)(o[3] - o[2]) * 0.1);      // s_memrealtime ticks at 100 MHz
        }
        simd.push_back((double)(last - first) / (insts * wps));
        fast.push_back((double)lo / insts); slow.push_back((double)hi / insts);
    }
    const double g = median(ghz);
    return {median(simd), median(fast), median(slow), g, ms * 1e-3 * g * 1e9 / (insts * wps)};
}

int main(int argc, char **argv)
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 2; }
    const int cus = p.multiProcessorCount, iters = argc > 1 ? atoi(argv[1]) : 20000, reps = argc > 2 ? atoi(argv[2]) : 7;
    float *in; double *sink; unsigned long long *stamps;
    std::vector<float> hin(4096);
    unsigned seed = 12345u;
    for (auto &v : hin) { seed = seed * 1664525u + 1013904223u; v = ((int)(seed >> 8) - (1 << 23)) * (1.0f / (1 << 23)) * 0.03125f; }
    (void)hipMalloc(&in, sizeof(float) * 4096);
    (void)hipMalloc(&sink, sizeof(double) * 512 * cus);
    (void)hipMalloc(&stamps, sizeof(unsigned long long) * 32 * cus);      // [workgroup][8 waves][t0, t1, r0, r1]
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    if (hipMemcpy(in, hin.data(), sizeof(float) * 4096, hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "copy failed\n"); return 2; }
    std::vector<unsigned long long> h(32 * cus);

    printf("device %s  CUs %d  one workgroup per CU, %d iterations of 180 instructions (36 v_cvt_f64_f32, 144 v_fmac_f64), 36 accumulators per lane\n",
           p.gcnArchName, cus, iters);
    const auto start = std::chrono::steady_clock::now();
    int warm = 0;
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count() < 2.5) {   // the clock settles under load first
        run<false>(cus, 512, iters, in, sink, stamps, h, e0, e1);
        run<true>(cus, 512, iters, in, sink, stamps, h, e0, e1);
        warm += 2;
    }
    printf("%d launches in the first 2.5 s (not reported); then %d launches per line, the forms alternating\n", warm, reps);
    printf("shader cycles per wave-instruction, min / median / max over the launches\n");
    printf("%-11s %-13s %-26s %-26s %-26s %-26s %s\n", "waves/SIMD", "form", "per SIMD (span of the WG)", "fastest wave of the WG", "slowest wave of the WG",
           "per SIMD (events x clock)", "in-loop clock, GHz");
    for (int threads : {256, 512}) {
        std::vector<double> v[2][5];
        for (int r = 0; r < reps; r++)
            for (int f = 0; f < 2; f++) {
                const Sample a = f ? run<true>(cus, threads, iters, in, sink, stamps, h, e0, e1) : run<false>(cus, threads, iters, in, sink, stamps, h, e0, e1);
                const double x[5] = {a.simd, a.fast, a.slow, a.wall, a.ghz};
                for (int k = 0; k < 5; k++) v[f][k].push_back(x[k]);
            }
        for (int f = 0; f < 2; f++) {
            printf("%-11d %-13s", threads / 256, f ? "B ahead" : "A dependent");
            for (int k = 0; k < 5; k++) {
                std::sort(v[f][k].begin(), v[f][k].end());
                printf(" %6.3f / %6.3f / %6.3f   ", v[f][k].front(), v[f][k][reps / 2], v[f][k].back());
            }
            printf("\n");
        }
    }
    return 0;
}
