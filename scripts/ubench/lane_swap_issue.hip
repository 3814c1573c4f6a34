// Issue rate of gfx950's lane swaps, measured the way fp64_peak.hip measures the fp64 pipe: every wave runs a dense loop of INDEPENDENT
// instructions of one kind on eight register pairs, 8 waves per SIMD so that the pipe never waits for a result.  Prints the time of one
// wave-instruction in cycles of the nominal clock, per SIMD (4.0 = one instruction per quad-cycle, the rate of a plain VALU instruction).
// The kinds: v_mov_b32 (the yardstick), v_mov_b32_dpp, v_add_f64, v_permlane32_swap_b32, v_permlane16_swap_b32, ds_bpermute_b32 (with its
// counted wait), and the two reduction steps of db_scan_topk_multi as they are built (two swaps + one v_add_f64 per double pair; a
// v_mul_f64 makes the next pair's second operand, so the mix is 2 : 1 : 1).  The
// swaps go through the builtins: the compiler places the wait states of the "VALU write -> permlane read" hazard itself.
// It also checks, lane by lane, what the two swaps exchange (the transposed reduction of kernels.hip relies on it).
//   hipcc --offload-arch=gfx950 -O3 -o scripts/ubench/lane_swap_issue scripts/ubench/lane_swap_issue.hip && scripts/ubench/lane_swap_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define REP4(x) x x x x
#define REP16(x) REP4(x) REP4(x) REP4(x) REP4(x)

enum { MOV, DPP, ADD64, SWAP32, SWAP16, BPERM, STEP32, STEP16, NKIND };

__device__ __forceinline__ void swap32(unsigned &a, unsigned &b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
}
__device__ __forceinline__ void swap16(unsigned &a, unsigned &b)
{
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0]; b = r[1];
}
template <bool WIDE> __device__ __forceinline__ void step(double &a, double &b)     // one transposed reduction step on a pair of doubles
{
    unsigned al = __double2loint(a), ah = __double2hiint(a), bl = __double2loint(b), bh = __double2hiint(b);
    if (WIDE) { swap32(al, bl); swap32(ah, bh); } else { swap16(al, bl); swap16(ah, bh); }
    a = __hiloint2double(ah, al) + __hiloint2double(bh, bl);
}

template <int KIND> __global__ void __launch_bounds__(256) dense(double *sink, int iters)
{
    unsigned u[16];
    double d[8];
#pragma unroll
    for (int i = 0; i < 16; i++) u[i] = threadIdx.x * 2654435761u + i;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = 1.0 + 1e-9 * (threadIdx.x + i);
    const unsigned sel = ((threadIdx.x * 7 + 3) & 63) << 2;
    const double eps = 1e-9 * sel;
    for (int it = 0; it < iters; it++) {
        REP16({
_Pragma("unroll")
            for (int i = 0; i < 8; i++) {
                if (KIND == MOV) asm volatile("v_mov_b32 %0, %1" : "+v"(u[2 * i]) : "v"(sel));
                if (KIND == DPP) asm volatile("v_mov_b32_dpp %0, %1 row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(u[2 * i]) : "v"(sel));
                if (KIND == ADD64) asm volatile("v_add_f64 %0, %0, %1" : "+v"(d[i]) : "v"(eps));
                if (KIND == SWAP32) swap32(u[2 * i], u[2 * i + 1]);
                if (KIND == SWAP16) swap16(u[2 * i], u[2 * i + 1]);
                if (KIND == BPERM) u[2 * i] = __builtin_amdgcn_ds_bpermute(sel, u[2 * i]);
            }
            if (KIND == STEP32 || KIND == STEP16) {
_Pragma("unroll")
                for (int i = 0; i < 4; i++) { step<KIND == STEP32>(d[2 * i], d[2 * i + 1]); d[2 * i + 1] = d[2 * i] * 0.5; }
            }
        })
    }
    double s = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) s += u[i];
#pragma unroll
    for (int i = 0; i < 8; i++) s += d[i];
    sink[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int KIND> static double cycles_per_wave_instruction(int blocks, int iters, double *sink, double clk_hz, int simds, double insts_per_rep)
{
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(dense<KIND>, dim3(blocks), dim3(256), 0, 0, sink, 16);
    (void)hipDeviceSynchronize();
    float best = 1e30f;
    for (int rep = 0; rep < 5; rep++) {
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL(dense<KIND>, dim3(blocks), dim3(256), 0, 0, sink, iters);
        (void)hipEventRecord(e1, 0);
        (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    const double wave_insts = insts_per_rep * 16.0 * iters * (256 / 64) * (double)blocks;
    return best * 1e-3 * clk_hz * simds / wave_insts;
}

// what the swaps exchange: a = 100 + lane, b = 200 + lane going in
__global__ void semantics(unsigned *out)
{
    unsigned a = 100 + threadIdx.x, b = 200 + threadIdx.x, c = a, e = b;
    swap32(a, b);
    swap16(c, e);
    out[threadIdx.x] = a; out[64 + threadIdx.x] = b; out[128 + threadIdx.x] = c; out[192 + threadIdx.x] = e;
}

int main(int argc, char **argv)
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 2; }
    const int cus = p.multiProcessorCount, blocks = cus * 8, iters = argc > 1 ? atoi(argv[1]) : 2000;   // 8 x 256 threads per CU = 8 waves per SIMD
    const double clk = 2.4e9;
    double *sink; (void)hipMalloc(&sink, sizeof(double) * 256 * blocks);
    unsigned *sem, h[256];
    (void)hipMalloc(&sem, sizeof h);
    hipLaunchKernelGGL(semantics, dim3(1), dim3(64), 0, 0, sem);
    if (hipMemcpy(h, sem, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "copy failed\n"); return 2; }
    int bad = 0;
    for (unsigned l = 0; l < 64; l++) {
        // swap32: lanes 32-63 of a <-> lanes 0-31 of b;  swap16: odd 16-lane rows of a <-> the even rows below them of b
        const unsigned a32 = l < 32 ? 100 + l : 200 + l - 32, b32 = l < 32 ? 100 + l + 32 : 200 + l;
        const bool odd = (l >> 4) & 1;
        const unsigned a16 = odd ? 200 + l - 16 : 100 + l, b16 = odd ? 200 + l : 100 + l + 16;
        bad += (h[l] != a32) + (h[64 + l] != b32) + (h[128 + l] != a16) + (h[192 + l] != b16);
    }
    printf("device %s  CUs %d  lane swaps exchange what kernels.hip assumes: %s\n", p.gcnArchName, cus, bad ? "NO" : "yes");
    if (bad) return 1;
    const int simds = cus * 4;
    printf("cycles of the nominal 2.4 GHz clock per wave-instruction and SIMD, dense independent instructions, 8 waves per SIMD:\n");
    printf("  v_mov_b32                          %6.2f\n", cycles_per_wave_instruction<MOV>(blocks, iters, sink, clk, simds, 8));
    printf("  v_mov_b32_dpp row_ror:8            %6.2f\n", cycles_per_wave_instruction<DPP>(blocks, iters, sink, clk, simds, 8));
    printf("  v_add_f64                          %6.2f\n", cycles_per_wave_instruction<ADD64>(blocks, iters, sink, clk, simds, 8));
    printf("  v_permlane32_swap_b32              %6.2f\n", cycles_per_wave_instruction<SWAP32>(blocks, iters, sink, clk, simds, 8));
    printf("  v_permlane16_swap_b32              %6.2f\n", cycles_per_wave_instruction<SWAP16>(blocks, iters, sink, clk, simds, 8));
    printf("  ds_bpermute_b32                    %6.2f\n", cycles_per_wave_instruction<BPERM>(blocks, iters, sink, clk, simds, 8));
    printf("  step 32 (2 swaps, v_add_f64, v_mul_f64: per 4 instructions -> per instruction) %6.2f\n", cycles_per_wave_instruction<STEP32>(blocks, iters, sink, clk, simds, 16));
    printf("  step 16 (2 swaps, v_add_f64, v_mul_f64: per 4 instructions -> per instruction) %6.2f\n", cycles_per_wave_instruction<STEP16>(blocks, iters, sink, clk, simds, 16));
    return 0;
}
