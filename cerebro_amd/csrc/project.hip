// project.hip -- the descriptor projection on the device: z = normalise(Mt x + b)  (include/cerebro_hip.h "descriptor projection").
//
// What the reference's descriptor server does on a host core for its one 4096-D model (scripts/whole_image_desc_compute_server.py:145-149:
// a 32768 x 4096 matrix streamed through a CPU for every keyframe) is, read the other way round, the score vector of ONE query against
// a database of D rows of in_dim elements -- the arithmetic kernels.hip owns, in the orders of DESIGN.md 3:
//   project_rows<MT> : y_j = dot_tree(x, Mt[j]) + b_j.  One wave per output row, grid-stride over j; x staged once per workgroup in LDS
//                      as float32 (in_dim <= 32768: 128 KiB); the matrix streamed with 16 B per lane, eight 1-KiB wave loads in flight
//                      per wave behind counted waits (the idiom of kernels.hip rows_dot), non-temporal.
//   project_finish   : s = dot_tree_f64(y, y), r = sqrt(s), z_j = y_j / r into the row's place in the append's staging buffer.  One
//                      workgroup, a launch of its own: y is complete at the kernel boundary and nothing else orders the two.
// The host side below owns the ctx's projection (matrix, bias, y, the staged raw descriptors) and the calls that need nothing of the
// DB: chip_project_set / _clear / _info / chip_project.  chip_db_append_projected_f32 is ctx_append with a second kind of source
// (chip_api.hip append_pass), which comes back here for every staging-sized chunk through project_chunk.
#include "chip_internal.h"

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

// s = orc_dot_tree_f64(y, y, D) by wave 0 (lane L: elements base + 2L + c, base in steps of 128; D % 4 == 0, so a pair is inside or
// outside as a whole), r = sqrt(s) correctly rounded, z_j = y_j / r by IEEE division.  Nothing is special-cased: r == 0 gives NaN.
__global__ __launch_bounds__(kProjBlock) void project_finish(const double *y, double *z, int32_t D)
{
    __shared__ double s_sum;
    const int tid = threadIdx.x, lane = tid & 63;
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

static int launch_project_row(Ctx *c, hipStream_t s, const float *x_dev, double *z_dev)
{
    const Projection &p = c->proj;
    ProjectArgs a;
    a.Mt = p.buf.get();
    a.x = x_dev;
    a.bias = p.has_bias ? p.bias() : nullptr;
    a.y = p.y();
    a.in_dim = p.in_dim;
    a.D = c->D;
    const int waves = kProjBlock / 64;
    int grid = (c->D + waves - 1) / waves;
    if (grid > c->n_cus) grid = c->n_cus;
    const int lds = p.in_dim * (int)sizeof(float);
    const void *fn = p.matrix_type == CHIP_PROJ_F64 ? (const void *)project_rows<double> : (const void *)project_rows<float>;
    if (lds > 65536) CHIP_HIP(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    void *args[] = {&a};
    CHIP_HIP(c, hipLaunchKernel(fn, dim3(grid), dim3(kProjBlock), args, (size_t)lds, s));
    hipLaunchKernelGGL(project_finish, dim3(1), dim3(kProjBlock), 0, s, (const double *)p.y(), z_dev, c->D);
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

// Rows [from, from + m) of the staged raw descriptors, projected into the first m rows of stage_dev (m * D doubles fit: append_pass).
// The caller holds a ResidentPause: project_rows puts a 1024-thread workgroup with up to 128 KiB of LDS on every CU, which cannot be
// placed beside the resident scan instance's workgroup (48 - 96 KiB of LDS at D = 4096) -- and ticks at 10 Hz renew that instance's
// lease, so the launch would wait for as long as the loop runs (the rule of batch.hip: a kernel that fills every CU pauses it).
int project_chunk(Ctx *c, int64_t from, int64_t m)
{
    double *stage = reinterpret_cast<double *>(c->stage_dev.get());
    for (int64_t i = 0; i < m; i++) {
        const int rc = launch_project_row(c, c->s_append, c->proj.x + (size_t)(from + i) * c->proj.in_dim, stage + (size_t)i * c->D);
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
    rc = fresh.reserve(c, mat_bytes + 2 * (size_t)c->D * sizeof(double));   // [matrix][bias][y]
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

}  // extern "C"
