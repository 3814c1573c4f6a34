// project.hip -- the descriptor projection on the device: z = normalise(Mt x + b)  (include/cerebro_hip.h "descriptor projection").
//
// What the reference's descriptor server does on a host core for its one 4096-D model (scripts/whole_image_desc_compute_server.py:145-149:
// a 32768 x 4096 matrix streamed through a CPU for every keyframe) is, read the other way round, the score vector of ONE query against
// a database of D rows of in_dim elements -- the arithmetic kernels.hip owns, in the orders of DESIGN.md 3:
//   project_rows<MT> : y_j = dot_tree(x, Mt[j]) + b_j.  One wave per output row, grid-stride over j; x staged once per workgroup in LDS
//                      as float32 (in_dim <= 32768: 128 KiB); the matrix streamed with 16 B per lane, eight 1-KiB wave loads in flight
//                      per wave behind counted waits (the idiom of kernels.hip rows_dot), non-temporal.
//   project_pass<MT, NB> : the same y for up to NB descriptors in ONE pass over the matrix (below, where it stands)
//   project_finish   : s = dot_tree_f64(y, y), r = sqrt(s), z_j = y_j / r into the row's place in the append's staging buffer.  One
//                      workgroup per descriptor of the group, a launch of its own: y is complete at the kernel boundary and nothing else
//                      orders the two.
// The host side below owns the ctx's projection (matrix, bias, y, the staged raw descriptors) and the calls that need nothing of the
// DB: chip_project_set / _clear / _info / chip_project.  chip_db_append_projected_f32 is ctx_append with a second kind of source
// (chip_api.hip append_pass), which comes back here for every staging-sized chunk through project_chunk; that walks the chunk's
// descriptors in groups (project_plan): a group of one is a project_rows launch, a larger one a project_pass launch.
#include "chip_internal.h"
#include <cstring>

namespace chip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct ProjectArgs {        // wave-uniform
    const void *Mt;         // D rows of in_dim elements of MT, contiguous
    const float *x;         // in_dim floats (device, 16-B aligned)
    const double *bias;     // D doubles or null
    double *y;              // D doubles
    int32_t in_dim;
    int32_t D;
};

constexpr int kProjBlock = 1024;   // one workgroup per CU: 128 KiB of x leave room for no second one (the headline scan's geometry)
constexpr int kProjU = 8;          // 1-KiB wave loads in flight per wave

__device__ __forceinline__ double proj_butterfly(double a)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a = a + __shfl_xor(a, m, 64);
    return a;
}

// One 1-KiB chunk of the row against the staged x: lane L holds elements 4L + c (float matrix) / 2L + c (double matrix) of the chunk.
// Float matrix: the product of two fp32 values is exact in fp64, fma == multiply-then-add (orc_dot_tree_f32).  Double matrix: x is
// widened on use and the fma's single rounding IS the definition (orc_dot_tree_f64 on (double)x).
__device__ __forceinline__ void proj_take(const f32x4 v, const float *xs_chunk, int lane, double &acc, float)
{
    const f32x4 w = *reinterpret_cast<const f32x4 *>(xs_chunk + 4 * lane);
#pragma unroll
    for (int c = 0; c < 4; c++) acc = __builtin_fma((double)w[c], (double)v[c], acc);
}
__device__ __forceinline__ void proj_take(const f32x4 v, const float *xs_chunk, int lane, double &acc, double)
{
    const f32x2 w = *reinterpret_cast<const f32x2 *>(xs_chunk + 2 * lane);
    const f64x2 m = __builtin_bit_cast(f64x2, v);
#pragma unroll
    for (int c = 0; c < 2; c++) acc = __builtin_fma((double)w[c], m[c], acc);
}

template <typename MT>
__global__ __launch_bounds__(kProjBlock) void project_rows(ProjectArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    constexpr int CH = 1024 / (int)sizeof(MT);     // elements of one wave load: 256 floats / 128 doubles
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int e = tid * 4; e < a.in_dim; e += kProjBlock * 4) *reinterpret_cast<f32x4 *>(xs + e) = *reinterpret_cast<const f32x4 *>(a.x + e);
    __syncthreads();
    const int n_chunks = a.in_dim / CH;            // in_dim % 256 == 0: whole chunks only
    const int n_batched = n_chunks - n_chunks % kProjU;
    for (int j = blockIdx.x + (int)gridDim.x * wave; j < a.D; j += (int)gridDim.x * (kProjBlock / 64)) {
        const char *row = static_cast<const char *>(a.Mt) + (size_t)j * a.in_dim * sizeof(MT) + lane * 16;
        double acc = 0.0;
        for (int k = 0; k < n_batched; k += kProjU) {
            // the batch's loads issued back to back from one address (immediate offsets) and consumed behind COUNTED waits: left to
            // itself hipcc sinks each load next to its use and the wave runs with 1-2 KiB in flight (kernels.hip rows_dot)
            f32x4 v[kProjU];
            const char *mid = row + (size_t)k * 1024 + 4096;
#pragma unroll
            for (int u = 0; u < kProjU; u++)
                asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(v[u]) : "v"(mid), "n"(u * 1024 - 4096) : "memory");
#pragma unroll
            for (int u = 0; u < kProjU; u++) {
                asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v[u]) : "n"(kProjU - 1 - u) : "memory");   // loads return in order
                proj_take(v[u], xs + (k + u) * CH, lane, acc, MT());
            }
        }
        for (int k = n_batched; k < n_chunks; k++) {   // the chunks that fill no batch (in_dim % 2048 floats / 1024 doubles), one by one
            const f32x4 *p = reinterpret_cast<const f32x4 *>(row + (size_t)k * 1024);
            const f32x4 v = __builtin_nontemporal_load((const __attribute__((address_space(1))) f32x4 *)p);
            proj_take(v, xs + k * CH, lane, acc, MT());
        }
        const double t = proj_butterfly(acc);
        if (lane == 0) a.y[j] = a.bias ? t + a.bias[j] : t;
    }
}

// ---- several descriptors per pass over the matrix --------------------------------------------------------------------------------
// project_pass<MT, NB> : y[b][j] = dot_tree(x_b, Mt[j]) + b_j for b < nb <= NB in ONE pass over Mt: the bits project_rows<MT> gives for
//                        each x_b alone.  A wave owns an output row as there and keeps nb accumulators for it; per (row, descriptor)
//                        the lane's elements arrive in the same order (k ascending, c ascending, one fma each), so how x is staged
//                        changes nothing.  NB copies of x do not fit the LDS, so the workgroup stages x in slabs of proj_slab() elements
//                        per descriptor along in_dim -- what one batch of the row meets --, double-buffered: the loads of slab s + 1
//                        (out of the L2, straight into the other buffer: no register holds them) are issued before slab s is consumed
//                        and waited for after it, one barrier per slab.  The matrix is streamed as in
//                        project_rows (asm-issued non-temporal 16-B loads, eight 1-KiB wave loads in flight behind counted waits), but
//                        as a ROLLING window: slot u of the next batch is issued as soon as slot u of this one is consumed, so the
//                        stream does not drain at a batch or slab boundary -- the workgroup's waves are in step here (the barriers),
//                        which project_rows' waves are not.
#ifndef CHIP_PROJ_WIDTH
#define CHIP_PROJ_WIDTH 8   // profiles/project_batch.md: the width with more descriptors per second at n = 64
#endif
constexpr int kProjWidth = CHIP_PROJ_WIDTH;   // descriptors one shared pass serves
// elements of x per descriptor and slab: what one batch of kProjU wave loads of the row meets -- 2048 (float matrix) or 1024 (double)
constexpr int proj_slab(int matrix_elem_bytes) { return kProjU * 1024 / matrix_elem_bytes; }
static_assert(kProjWidth % 4 == 0 && 2 * kProjWidth * proj_slab(4) * (int)sizeof(float) <= 160 * 1024, "two slabs of every descriptor in the LDS, whole staging loads per wave");

struct ProjectPassArgs {    // wave-uniform
    const void *Mt;
    const float *x;         // nb descriptors of in_dim floats, one after the other
    const double *bias;
    double *y;              // [nb][D]
    int32_t in_dim;
    int32_t D;
    int32_t nb;
};

// 16 bytes per lane, global -> LDS at (wave-uniform LDS byte address in M0) + lane * 16, without passing a register; M0 is saved and
// restored around the load (the idiom of kernels.hip glds16_q).  The load counts in vmcnt like any other.
__device__ __forceinline__ void proj_glds16(const void *gsrc_lane, uint32_t lds_base_wave_uniform)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc_lane), "s"(lds_base_wave_uniform)
                 : "memory");
}

// The staging loads of one slab into buffer `buf`: the slab is NB x PIECES pieces of 1 KiB (256 elements of one descriptor), dealt round
// robin to the 16 waves, NB / 2 (float matrix) or NB / 4 (double) loads each.  No load is left out (the counted waits count them): a descriptor past nb re-reads the last
// one, a piece past in_dim reads the descriptor's first, and what they bring is never read.
template <typename MT, int NB>
__device__ __forceinline__ void proj_stage_issue(const ProjectPassArgs &a, uint32_t lds0, int slab, int buf, int wave, int lane)
{
    constexpr int SLAB = kProjU * 1024 / (int)sizeof(MT), PIECES = SLAB / 256;   // 8 pieces per descriptor (float matrix) or 4 (double)
#pragma unroll
    for (int i = 0; i < NB * PIECES / (kProjBlock / 64); i++) {
        const int unit = i * (kProjBlock / 64) + wave, b = unit / PIECES, q = unit % PIECES, e = slab * SLAB + q * 256;   // wave-uniform
        const float *p = a.x + (size_t)(b < a.nb ? b : a.nb - 1) * a.in_dim + (e < a.in_dim ? e : 0) + lane * 4;
        const uint32_t dst = lds0 + (uint32_t)(((buf * NB + b) * SLAB + q * 256) * (int)sizeof(float));
        proj_glds16(p, (uint32_t)__builtin_amdgcn_readfirstlane((int)dst));
    }
}

// One 1-KiB chunk of the row against the nb staged descriptors: proj_take, nb times over, in two steps -- the chunk's elements of every
// descriptor out of the LDS (xc: the chunk's place in descriptor 0 of the slab; a descriptor past nb reads stale LDS that is never
// used), then the fmas -- so that a caller can put the LDS reads BEFORE its counted wait: they are under way while the chunk lands.
template <typename MT> struct ProjX { typedef f32x4 type; };          // what a lane holds of x per chunk: 4 floats against a float matrix,
template <> struct ProjX<double> { typedef f32x2 type; };             // 2 against a double one
template <typename MT, int NB, int SLAB>
__device__ __forceinline__ void proj_read_x(typename ProjX<MT>::type (&w)[NB], const float *xc, int lane)
{
    typedef typename ProjX<MT>::type X;
    constexpr int N = (int)(sizeof(X) / sizeof(float));
#pragma unroll
    for (int b = 0; b < NB; b++) w[b] = *reinterpret_cast<const X *>(xc + b * SLAB + N * lane);
}
template <int NB>
__device__ __forceinline__ void proj_fma_nb(const f32x4 v, const f32x4 (&w)[NB], double *acc)
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double m = (double)v[c];
#pragma unroll
        for (int b = 0; b < NB; b++)
            acc[b] = __builtin_fma((double)w[b][c], m, acc[b]);
    }
}
template <int NB>
__device__ __forceinline__ void proj_fma_nb(const f32x4 v, const f32x2 (&w)[NB], double *acc)
{
    const f64x2 m = __builtin_bit_cast(f64x2, v);
#pragma unroll
    for (int c = 0; c < 2; c++) {
#pragma unroll
        for (int b = 0; b < NB; b++)
            acc[b] = __builtin_fma((double)w[b][c], m[c], acc[b]);
    }
}

// One batch of kProjU chunks, whose loads are under way in v.  ROLL: slot u of the NEXT batch (at `next`) is issued once slot u of this
// one is consumed, so eight loads stay in flight; otherwise this is the row's last batch and the window runs empty.  EXTRA: loads
// younger than this batch's and older than the next one's (the staging loads of the slab after this one), which the counts let pass.
template <typename MT, int NB, bool ROLL, int EXTRA>
__device__ __forceinline__ void proj_batch(f32x4 (&v)[kProjU], const char *next, const float *xc, int lane, double (&acc)[NB])
{
    constexpr int CH = 1024 / (int)sizeof(MT), SLAB = kProjU * CH;
#pragma unroll
    for (int u = 0; u < kProjU; u++) {
        // the descriptors in two halves, so that a lane holds NB / 2 of them at a time: the first half's LDS reads stand before the
        // wait, the second half's are hidden behind the first half's fmas
        constexpr int H = NB / 2;
        typename ProjX<MT>::type w0[H], w1[H];
        proj_read_x<MT, H, SLAB>(w0, xc + u * CH, lane);
        asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v[u]) : "n"((ROLL ? kProjU - 1 : kProjU - 1 - u) + EXTRA) : "memory");   // loads return in order
        proj_read_x<MT, H, SLAB>(w1, xc + H * SLAB + u * CH, lane);
        proj_fma_nb<H>(v[u], w0, acc);
        __builtin_amdgcn_sched_barrier(0);
        proj_fma_nb<H>(v[u], w1, acc + H);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ROLL) asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(v[u]) : "v"(next), "n"(u * 1024 - 4096) : "memory");
    }
}

template <typename MT, int NB>
__global__ __launch_bounds__(kProjBlock) void project_pass(ProjectPassArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xs = reinterpret_cast<float *>(smem);   // [2][NB][SLAB]
    constexpr int CH = 1024 / (int)sizeof(MT);     // elements of one wave load
    constexpr int SLAB = kProjU * CH;              // elements of x per descriptor and slab: one batch of the row
    constexpr int NL = NB * (SLAB / 256) / (kProjBlock / 64);   // staging loads per wave and slab
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)smem;
    const int n_chunks = a.in_dim / CH;
    const int n_full = n_chunks / kProjU;          // slabs that are a whole batch; the chunks that fill none are the last slab
    const int stride = (int)gridDim.x * (kProjBlock / 64);
    for (int base = blockIdx.x; base < a.D; base += stride) {   // the workgroup's waves take rows base + gridDim.x * wave: project_rows' map
        const int j = base + (int)gridDim.x * wave;
        if (base != (int)blockIdx.x) __syncthreads();   // every wave has left the buffers of the rows before
        proj_stage_issue<MT, NB>(a, lds0, 0, 0, wave, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // Every wave stages its share of each slab and meets one barrier per whole slab; the two branches below differ in nothing else.
        // No register that a load is under way into lives across a branch or a join: the matrix window belongs to the first branch alone.
        if (j < a.D) {   // wave-uniform
            const char *row = static_cast<const char *>(a.Mt) + (size_t)j * a.in_dim * sizeof(MT) + lane * 16;
            double acc[NB];
#pragma unroll
            for (int b = 0; b < NB; b++) acc[b] = 0.0;
            if (n_full > 0) {
                f32x4 v[kProjU];
#pragma unroll
                for (int u = 0; u < kProjU; u++)
                    asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(v[u]) : "v"(row + 4096), "n"(u * 1024 - 4096) : "memory");
                int s = 0;
                for (; s + 1 < n_full; s++) {
                    proj_stage_issue<MT, NB>(a, lds0, s + 1, (s + 1) & 1, wave, lane);   // NL loads younger than the batch under way; that buffer
                                                                                         // was read last in slab s - 1, a barrier ago
                    proj_batch<MT, NB, true, NL>(v, row + (size_t)(s + 1) * (kProjU * 1024) + 4096, xs + (size_t)(s & 1) * NB * SLAB, lane, acc);
                    // this wave's share of slab s + 1 has landed: its loads are older than the kProjU of the next batch
                    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(kProjU) : "memory");
                }
                // the last whole batch: the window runs empty.  The slab after it holds the chunks that fill no batch, or does not exist
                // (then the staging loads re-read the descriptors' first piece into the buffer nobody reads: the counts stay the same)
                proj_stage_issue<MT, NB>(a, lds0, s + 1, (s + 1) & 1, wave, lane);
                proj_batch<MT, NB, false, NL>(v, row, xs + (size_t)(s & 1) * NB * SLAB, lane, acc);
                asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            }
            // the chunks that fill no batch (in_dim % 2048 floats / 1024 doubles), one by one
            const float *xb = xs + (size_t)(n_full & 1) * NB * SLAB;
            for (int k = n_full * kProjU; k < n_chunks; k++) {
                const f32x4 *p = reinterpret_cast<const f32x4 *>(row + (size_t)k * 1024);
                const f32x4 t = __builtin_nontemporal_load((const __attribute__((address_space(1))) f32x4 *)p);
                typename ProjX<MT>::type w[NB];
                proj_read_x<MT, NB, SLAB>(w, xb + (k - n_full * kProjU) * CH, lane);
                proj_fma_nb<NB>(t, w, acc);
            }
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const double t = proj_butterfly(acc[b]);
                if (lane == 0 && b < a.nb) a.y[(size_t)b * a.D + j] = a.bias ? t + a.bias[j] : t;
            }
        } else {
            for (int s = 0; s < n_full; s++) {
                proj_stage_issue<MT, NB>(a, lds0, s + 1, (s + 1) & 1, wave, lane);
                asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
    }
}

// s = orc_dot_tree_f64(y, y, D) by wave 0 (lane L: elements base + 2L + c, base in steps of 128; D % 4 == 0, so a pair is inside or
// outside as a whole), r = sqrt(s) correctly rounded, z_j = y_j / r by IEEE division.  Nothing is special-cased: r == 0 gives NaN.
// One workgroup per descriptor of the group: y and z of descriptor blockIdx.x are D doubles further on.
__global__ __launch_bounds__(kProjBlock) void project_finish(const double *y, double *z, int32_t D)
{
    __shared__ double s_sum;
    const int tid = threadIdx.x, lane = tid & 63;
    y += (size_t)blockIdx.x * D;
    z += (size_t)blockIdx.x * D;
    if (tid < 64) {
        double acc = 0.0;
        for (int base = 0; base < D; base += 128) {
            const int e = base + 2 * lane;
            if (e < D) {
                const f64x2 v = *reinterpret_cast<const f64x2 *>(y + e);
                acc = __builtin_fma(v[0], v[0], acc);
                acc = __builtin_fma(v[1], v[1], acc);
            }
        }
        acc = proj_butterfly(acc);
        if (lane == 0) s_sum = acc;
    }
    __syncthreads();
    const double r = sqrt(s_sum);
    for (int e = tid; e < D; e += kProjBlock) z[e] = y[e] / r;
}

// What a projecting call over n descriptors launches (chip_project_plan): the ONE place that decides it; launch_project_group launches
// what this says.  Groups of kProjWidth descriptors; a group of one is project_rows, as before there was a shared pass.
static void project_plan(int in_dim, int matrix_type, int64_t n, chip_project_plan_out *f)
{
    std::memset(f, 0, sizeof *f);
    f->width = kProjWidth;
    f->passes = n > 0 ? (n + kProjWidth - 1) / kProjWidth : 0;
    f->single_launches = n > 0 && n % kProjWidth == 1 ? 1 : 0;
    f->shared_passes = f->passes - f->single_launches;
    f->slab = proj_slab(matrix_type == CHIP_PROJ_F64 ? 8 : 4);
    f->lds_bytes = 2 * kProjWidth * f->slab * (int)sizeof(float);
    f->single_lds_bytes = in_dim * (int)sizeof(float);
    f->block = kProjBlock;
}

// Descriptors x_dev[0 .. m) (m <= kProjWidth) -> rows z_dev[0 .. m): one pass over the matrix, one finishing launch
static int launch_project_group(Ctx *c, hipStream_t s, const float *x_dev, double *z_dev, int m)
{
    Projection &p = c->proj;
    const int waves = kProjBlock / 64;
    int grid = (c->D + waves - 1) / waves;
    if (grid > c->n_cus) grid = c->n_cus;
    chip_project_plan_out f;
    project_plan(p.in_dim, p.matrix_type, m, &f);
    const bool f64 = p.matrix_type == CHIP_PROJ_F64;
    if (f.shared_passes == 0) {
        ProjectArgs a;
        a.Mt = p.buf.get();
        a.x = x_dev;
        a.bias = p.has_bias ? p.bias() : nullptr;
        a.y = p.y();
        a.in_dim = p.in_dim;
        a.D = c->D;
        const int lds = f.single_lds_bytes;
        const void *fn = f64 ? (const void *)project_rows<double> : (const void *)project_rows<float>;
        if (lds > 65536) CHIP_HIP(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        void *args[] = {&a};
        CHIP_HIP(c, hipLaunchKernel(fn, dim3(grid), dim3(kProjBlock), args, (size_t)lds, s));
        p.last_singles++;
    } else {
        ProjectPassArgs a;
        a.Mt = p.buf.get();
        a.x = x_dev;
        a.bias = p.has_bias ? p.bias() : nullptr;
        a.y = p.y();
        a.in_dim = p.in_dim;
        a.D = c->D;
        a.nb = m;
        const void *fn = f64 ? (const void *)project_pass<double, kProjWidth> : (const void *)project_pass<float, kProjWidth>;
        if (f.lds_bytes > 65536) CHIP_HIP(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, f.lds_bytes));
        void *args[] = {&a};
        CHIP_HIP(c, hipLaunchKernel(fn, dim3(grid), dim3(f.block), args, (size_t)f.lds_bytes, s));
        p.last_passes++;
        p.last_pass_descriptors += m;
    }
    hipLaunchKernelGGL(project_finish, dim3(m), dim3(kProjBlock), 0, s, (const double *)p.y(), z_dev, c->D);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// The raw descriptors of one call -> Projection::x (the append lock is held).  x: host memory, or device memory of the ctx's device.
int project_stage_input(Ctx *c, const float *x, int64_t n)
{
    const size_t count = (size_t)n * c->proj.in_dim;
    const int rc = c->proj.x.reserve(c, count);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemcpyAsync(c->proj.x, x, count * sizeof(float), hipMemcpyDefault, c->s_append));
    return CHIP_OK;
}

void project_count_reset(Ctx *c) { c->proj.last_passes = c->proj.last_singles = c->proj.last_pass_descriptors = 0; }

// Rows [from, from + m) of the staged raw descriptors, projected into the first m rows of stage_dev (m * D doubles fit: append_pass),
// in groups of kProjWidth that share a pass over the matrix.
// The caller holds a ResidentPause: project_rows puts a 1024-thread workgroup with up to 128 KiB of LDS on every CU (project_pass: the
// same block, 128 KiB), which cannot be placed beside the resident scan instance's workgroup (48 - 96 KiB of LDS at D = 4096) -- and
// ticks at 10 Hz renew that instance's lease, so the launch would wait for as long as the loop runs (the rule of batch.hip: a kernel
// that fills every CU pauses it).
int project_chunk(Ctx *c, int64_t from, int64_t m)
{
    double *stage = reinterpret_cast<double *>(c->stage_dev.get());
    for (int64_t i = 0; i < m; i += kProjWidth) {
        const int g = (int)(m - i < kProjWidth ? m - i : kProjWidth);
        const int rc = launch_project_group(c, c->s_append, c->proj.x + (size_t)(from + i) * c->proj.in_dim, stage + (size_t)i * c->D, g);
        if (rc != CHIP_OK) return rc;
    }
    return CHIP_OK;
}

static int check_projectable(const Ctx *c) { return (c->group || c->nranks > 1) ? CHIP_ERR_UNSUPPORTED : CHIP_OK; }

}  // namespace chip

using namespace chip;

extern "C" {

int chip_build_has_project(void) { return 1; }

int chip_project_set(chip_ctx *c, int32_t in_dim, const void *Mt, int32_t matrix_type, const double *bias)
{
    if (!c || !Mt) return CHIP_ERR_INVALID_ARG;
    if (in_dim < 256 || in_dim > CHIP_PROJ_MAX_IN_DIM || in_dim % 256 != 0) return CHIP_ERR_UNSUPPORTED;
    if (matrix_type != CHIP_PROJ_F32 && matrix_type != CHIP_PROJ_F64) return CHIP_ERR_UNSUPPORTED;
    int rc = check_projectable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    const size_t mat_bytes = (size_t)in_dim * c->D * (matrix_type == CHIP_PROJ_F64 ? 8 : 4);
    // The new matrix is complete in a buffer of its own before it replaces the old one, so that a failure leaves the earlier
    // projection in place.  One pause over the whole exchange (declared first: the old buffer is freed before it ends).
    ResidentPause paused(c);
    DevBuf<char> fresh;
    rc = fresh.reserve(c, mat_bytes + (1 + (size_t)kProjWidth) * c->D * sizeof(double));   // [matrix][bias][y of one group]
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemcpyAsync(fresh, Mt, mat_bytes, hipMemcpyHostToDevice, c->s_append));
    if (bias) CHIP_HIP(c, hipMemcpyAsync(fresh + mat_bytes, bias, (size_t)c->D * sizeof(double), hipMemcpyHostToDevice, c->s_append));
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    Projection &p = c->proj;
    p.buf.swap(fresh);
    p.in_dim = in_dim;
    p.matrix_type = matrix_type;
    p.has_bias = bias != nullptr;
    p.mat_bytes = mat_bytes;
    p.D = c->D;
    return CHIP_OK;
}

int chip_project_clear(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_projectable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    ResidentPause paused(c, c->proj.in_dim != 0);
    c->proj.buf.release();
    c->proj.x.release();
    c->proj.in_dim = 0;
    c->proj.matrix_type = 0;
    c->proj.has_bias = false;
    return CHIP_OK;
}

int chip_project_info(const chip_ctx *cc, int32_t *in_dim, int32_t *matrix_type, int32_t *has_bias)
{
    if (!cc) return CHIP_ERR_INVALID_ARG;
    chip_ctx *c = const_cast<chip_ctx *>(cc);
    const int rc = check_projectable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    if (in_dim) *in_dim = c->proj.in_dim;
    if (matrix_type) *matrix_type = c->proj.matrix_type;
    if (has_bias) *has_bias = c->proj.has_bias ? 1 : 0;
    return CHIP_OK;
}

int chip_project(chip_ctx *c, const float *x, int64_t n, double *z)
{
    if (!c || !x || !z || n < 0) return CHIP_ERR_INVALID_ARG;
    int rc = check_projectable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    if (!c->proj.in_dim) return CHIP_ERR_BUSY;
    if (n == 0) return CHIP_OK;
    CHIP_HIP(c, hipSetDevice(c->device));
    ResidentPause paused(c);   // project_rows fills every CU and does not fit beside the instance (project_chunk); ticks are launched meanwhile
    project_count_reset(c);
    rc = project_stage_input(c, x, n);
    if (rc != CHIP_OK) return rc;
    const size_t row_bytes = (size_t)c->D * sizeof(double);
    const int64_t chunk_rows = (int64_t)(c->stage_bytes / row_bytes);      // the chunks of append_pass
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = (n - done) < chunk_rows ? (n - done) : chunk_rows;
        rc = project_chunk(c, done, m);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipMemcpyAsync(reinterpret_cast<char *>(z) + (size_t)done * row_bytes, c->stage_dev, (size_t)m * row_bytes, hipMemcpyDeviceToHost, c->s_append));
    }
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    return CHIP_OK;
}

int chip_project_plan(int32_t in_dim, int32_t matrix_type, int64_t n, chip_project_plan_out *out)
{
    if (!out || n < 0) return CHIP_ERR_INVALID_ARG;
    if (in_dim < 256 || in_dim > CHIP_PROJ_MAX_IN_DIM || in_dim % 256 != 0) return CHIP_ERR_UNSUPPORTED;
    if (matrix_type != CHIP_PROJ_F32 && matrix_type != CHIP_PROJ_F64) return CHIP_ERR_UNSUPPORTED;
    project_plan(in_dim, matrix_type, n, out);
    return CHIP_OK;
}

int chip_debug_project_last(chip_ctx *c, int64_t *passes, int64_t *descriptors, int32_t *width)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_projectable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    const Projection &p = c->proj;
    if (passes) { passes[0] = p.last_passes; passes[1] = p.last_singles; }
    if (descriptors) { descriptors[0] = p.last_pass_descriptors; descriptors[1] = p.last_singles; }
    if (width) *width = kProjWidth;
    return CHIP_OK;
}

}  // extern "C"
