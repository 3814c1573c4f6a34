// vlad.hip -- the NetVLAD / GhostVLAD pooling on the device: the trunk's last feature map -> the pooled float32 vector
// (include/cerebro_hip.h "NetVLAD pooling").
//
// The one non-stock layer of both of the reference's models (scripts/predict_utils.py NetVLADLayer / GhostVLADLayer), in this
// project's own definition: all fp64, every operation rounded once, in stated orders.  The work is tiny (12 - 18 M multiply-adds at
// the production shapes); the call is bound by launches and latency, so every stage is spread over many CUs and none is tuned further:
//   vlad_transpose : a CHIP_VLAD_NCHW map x[c][n] -> the ctx's copy x[n][c], tiled through LDS so that both sides coalesce
//   vlad_assign    : one wave per position, grid-stride.  The position's channels stay in registers (C <= 1024: four float4 per lane),
//                    the K+G weight rows are read in place out of the L2 (at most 128 KiB, shared by every wave of the launch); one
//                    butterfly per score, lane k & 63 keeps score k, the softmax is spread over the lanes, Z is the ascending chain
//   vlad_aggregate : grid = position blocks x 64-channel slices x groups of 8 clusters, one wave each; a thread owns one channel and
//                    eight clusters and walks the block's 64 positions in order (a[n][k] staged in 4 KiB of LDS and broadcast, x[n][c]
//                    coalesced, sixteen loads in flight) -> P_j, S_j
//   vlad_reduce    : one workgroup per kept cluster: the chains over j, the centres, q_k by wave 0 (the project_finish idiom) -> V, A, U
//   vlad_finish    : one workgroup, a launch of its own (U is complete at the kernel boundary): q, v as float32 into
//                    Projection::x / chip_vlad's buffer, or (double)v into the append's staging buffer
// Every launch serves a GROUP of maps of one shape (the batched calls; a single call is a group of one): the positions of the group lie one
// map after the other, vlad_assign walks them all, the others take their map from a grid axis -- the 64-position blocks of the definition
// are per map and never straddle two.
// The host side owns the ctx's weights and scratch (Vlad, chip_internal.h) and the calls that need nothing of the DB; the pooled append
// is ctx_append with a third kind of source (chip_api.hip append_pass), which comes back here through vlad_chunk.
#include "chip_internal.h"
#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)   // as the build's -ffp-contract=off: nothing below is fused unless it says __builtin_fma

namespace chip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

struct VladArgs {            // wave-uniform; the arrays of a group's maps lie one after the other
    const float *x;          // N x C
    const float *Wt;         // (K+G) x C
    const double *bias;      // K+G
    const float *centres;    // K x C
    double *a;               // N x (K+G)
    double *P;               // blocks x K x C
    double *S;               // blocks x K
    double *V;               // K x C
    double *U;               // K x C
    double *A;               // K
    uint32_t *flag;          // bit1 (2u) is raised by a non-finite score: the append's flag word, or chip_vlad's own
    int32_t N, C, K, KG, blocks;   // positions and 64-position blocks of ONE map
    int32_t maps;
};

constexpr int kVladAssignBlock = 256;   // four positions per workgroup
constexpr int kVladKT = 8;              // clusters per thread of vlad_aggregate
constexpr int kVladReduceBlock = 256;
constexpr int kVladFinishBlock = 1024;

__device__ __forceinline__ double vlad_butterfly(double a)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a = a + __shfl_xor(a, m, 64);
    return a;
}

// lane `l` (wave-uniform) of v, to every lane
__device__ __forceinline__ double vlad_read_lane(double v, int l)
{
    i32x2 w = __builtin_bit_cast(i32x2, v);
    w[0] = __builtin_amdgcn_readlane(w[0], l);
    w[1] = __builtin_amdgcn_readlane(w[1], l);
    return __builtin_bit_cast(double, w);
}

// exp(t) for t <= 0 as the header defines it: one table-free reduction, a degree-13 Horner form, an exact scaling
__device__ __forceinline__ double vlad_exp(double t)
{
    constexpr double LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                              1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    if (t < -700.0) return 0.0;
    const double kf = __builtin_rint(t * LOG2E);
    const double r = (t - kf * LN2_HI) - kf * LN2_LO;
    double p = c[13];
#pragma unroll
    for (int i = 12; i >= 0; i--) p = p * r + c[i];
    const unsigned long long bits = (unsigned long long)(1023 + (int)kf) << 52;   // kf >= -1010: a normal power of two
    return p * __builtin_bit_cast(double, bits);
}

// x[c][n] (C x N) -> y[n][c] (N x C) of map blockIdx.z: 32 x 32 tiles, the LDS rows padded by one float
__global__ __launch_bounds__(256) void vlad_transpose(const float *x, float *y, int32_t N, int32_t C)
{
    __shared__ float tile[32][33];
    x += (size_t)blockIdx.z * N * C;
    y += (size_t)blockIdx.z * N * C;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const int c = c0 + ty + i, n = n0 + tx;
        if (c < C && n < N) tile[ty + i][tx] = x[(size_t)c * N + n];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const int n = n0 + ty + i, c = c0 + tx;
        if (c < C && n < N) y[(size_t)n * C + c] = tile[tx][ty + i];
    }
}

// Scores and softmax of one position per wave.  s[n][k] = orc_dot_tree_f32(x[n], Wt[k], C) + bias[k]: lane L holds elements
// j * 256 + 4L + c of the position (a lane's four are inside C or outside as a whole: C % 4 == 0); float x float is exact in fp64, so the
// fma is multiply-then-add.  No LDS, 256 threads: the launch is placed wherever a CU has four wave slots.
__global__ __launch_bounds__(kVladAssignBlock) void vlad_assign(VladArgs p)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = kVladAssignBlock / 64;
    const bool h0 = lane < p.KG, h1 = lane + 64 < p.KG;
    const int total = p.N * p.maps;   // a score is per position: the group's maps are walked as one
    for (int n = blockIdx.x * waves + wave; n < total; n += (int)gridDim.x * waves) {
        f32x4 xv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = j * 256 + 4 * lane;
            xv[j] = e < p.C ? *reinterpret_cast<const f32x4 *>(p.x + (size_t)n * p.C + e) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        double s0 = 0.0, s1 = 0.0;   // scores k = lane and k = lane + 64
        bool bad = false;
        constexpr int UK = 4;   // weight rows whose loads are in flight together
        for (int kb = 0; kb < p.KG; kb += UK) {
            f32x4 wv[UK][4];
#pragma unroll
            for (int u = 0; u < UK; u++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const bool in = kb + u < p.KG && j * 256 + 4 * lane < p.C;
                    wv[u][j] = in ? *reinterpret_cast<const f32x4 *>(p.Wt + (size_t)(kb + u) * p.C + j * 256 + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int u = 0; u < UK; u++) {
                const int k = kb + u;
                if (k < p.KG) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (j * 256 + 4 * lane < p.C) {
#pragma unroll
                            for (int c = 0; c < 4; c++) acc = __builtin_fma((double)xv[j][c], (double)wv[u][j][c], acc);
                        }
                    }
                    const double t = vlad_butterfly(acc) + p.bias[k];
                    bad |= !(__builtin_fabs(t) <= 0x1.fffffffffffffp+1023);
                    if (lane == (k & 63)) {
                        if (k < 64) s0 = t; else s1 = t;
                    }
                }
            }
        }
        if (bad && lane == 0) atomicOr(p.flag, 2u);
        // the largest score.  The definition walks k upwards with >; as a VALUE the maximum is the same in any order (two zeros of
        // different sign are the one exception, and vlad_exp(+0) == vlad_exp(-0) == 1)
        double m = h0 ? s0 : -__builtin_inf();
        if (h1 && s1 > m) m = s1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double o = __shfl_xor(m, d, 64);
            if (o > m) m = o;
        }
        const double e0 = h0 ? vlad_exp(s0 - m) : 0.0, e1 = h1 ? vlad_exp(s1 - m) : 0.0;
        double Z = 0.0;   // ((0 + e_0) + e_1) + ...: every lane walks the same chain
        for (int k = 0; k < p.KG; k++) Z = Z + vlad_read_lane(k < 64 ? e0 : e1, k & 63);
        double *an = p.a + (size_t)n * p.KG;
        if (h0) an[lane] = e0 / Z;
        if (h1) an[lane + 64] = e1 / Z;
    }
}

// P_j[k][c] and S_j[k] of position block j = blockIdx.x % blocks of map blockIdx.x / blocks for channel blockIdx.y * 64 + lane and clusters blockIdx.z * 8 .. + 7 (k < K:
// ghost rows are never formed): acc = acc + (a[n][k] * (double)x[n][c]), product rounded, sum rounded, n ascending from 0.0.
__global__ __launch_bounds__(64) void vlad_aggregate(VladArgs p)
{
    const int j = blockIdx.x, c = blockIdx.y * 64 + (int)threadIdx.x, k0 = blockIdx.z * kVladKT;   // j counts the blocks of all maps: P, S
    const int map = j / p.blocks, first = map * p.N, last = first + p.N;                             // are indexed by it as they are
    const int n0 = first + (j - map * p.blocks) * CHIP_VLAD_BLOCK, n1 = n0 + CHIP_VLAD_BLOCK < last ? n0 + CHIP_VLAD_BLOCK : last;
    const bool live = c < p.C, sums = blockIdx.y == 0;
    // the block's assignments of these eight clusters, staged once (4 KiB; a cluster past K or a position past the block reads 0.0 and
    // is never stored): the walk below is then bound by its 64 dependent additions, not by 64 trips to the L2
    __shared__ double as[CHIP_VLAD_BLOCK][kVladKT];
    for (int i = threadIdx.x; i < CHIP_VLAD_BLOCK * kVladKT; i += 64) {
        const int n = n0 + i / kVladKT, k = k0 + i % kVladKT;
        as[i / kVladKT][i % kVladKT] = (n < n1 && k < p.K) ? p.a[(size_t)n * p.KG + k] : 0.0;
    }
    __syncthreads();
    double acc[kVladKT], sacc[kVladKT];
#pragma unroll
    for (int i = 0; i < kVladKT; i++) acc[i] = sacc[i] = 0.0;
    constexpr int UX = 16;   // map loads in flight per thread
    // No branch inside the walk, so that the LDS reads and the map loads of a batch are issued together: a position past the block's end
    // and a cluster past K carry a == +0.0 (above), and acc + (+0.0 * x) == acc bit for bit for every finite x -- acc is never -0.0, it
    // starts at +0.0 and a sum that cancels exactly is +0.0.  The address of such a position is clamped to the block's last one and its
    // value replaced by zero; a lane past C reads channel 0 and stores nothing.
    const int cc = live ? c : 0;
    for (int nb = n0; nb < n1; nb += UX) {
        float xs[UX];
#pragma unroll
        for (int u = 0; u < UX; u++) {
            const int n = nb + u < n1 ? nb + u : n1 - 1;
            const float t = p.x[(size_t)n * p.C + cc];
            xs[u] = nb + u < n1 ? t : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UX; u++) {
            const double xv = (double)xs[u];
            const int r = nb + u - n0;   // < CHIP_VLAD_BLOCK: nb - n0 is a multiple of UX below 64, and 64 % UX == 0
#pragma unroll
            for (int i = 0; i < kVladKT; i++) {
                const double av = as[r][i];
                acc[i] = acc[i] + av * xv;
                sacc[i] = sacc[i] + av;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kVladKT; i++) {
        if (k0 + i < p.K) {
            if (live) p.P[((size_t)j * p.K + k0 + i) * p.C + c] = acc[i];
            if (sums && threadIdx.x == 0) p.S[(size_t)j * p.K + k0 + i] = sacc[i];
        }
    }
}

// Cluster k = blockIdx.x of map blockIdx.y: V[k][c] and A[k] (the chains over j), Wv = V + (A * (double)centres), q_k = orc_dot_tree_f64(Wv, Wv, C) by
// wave 0 (lane L: elements base + 2L + c, base in steps of 128; C % 4 == 0), U = Wv / sqrt(q_k > 1e-12 ? q_k : 1e-12).
__global__ __launch_bounds__(kVladReduceBlock) void vlad_reduce(VladArgs p)
{
    __shared__ double wv[1024];
    __shared__ double s_q;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t KC = (size_t)p.K * p.C;
    p.P += (size_t)blockIdx.y * p.blocks * KC;
    p.S += (size_t)blockIdx.y * p.blocks * p.K;
    p.V += (size_t)blockIdx.y * KC;
    p.U += (size_t)blockIdx.y * KC;
    p.A += (size_t)blockIdx.y * p.K;
    double A = 0.0;
    for (int j = 0; j < p.blocks; j++) A = A + p.S[(size_t)j * p.K + k];
    if (tid == 0) p.A[k] = A;
    for (int c = tid; c < p.C; c += kVladReduceBlock) {
        double V = 0.0;
#pragma unroll 4
        for (int j = 0; j < p.blocks; j++) V = V + p.P[((size_t)j * p.K + k) * p.C + c];
        p.V[(size_t)k * p.C + c] = V;
        wv[c] = V + (A * (double)p.centres[(size_t)k * p.C + c]);
    }
    __syncthreads();
    if (tid < 64) {
        double acc = 0.0;
        for (int base = 0; base < p.C; base += 128) {
            const int e = base + 2 * lane;
            if (e < p.C) {
                acc = __builtin_fma(wv[e], wv[e], acc);
                acc = __builtin_fma(wv[e + 1], wv[e + 1], acc);
            }
        }
        acc = vlad_butterfly(acc);
        if (lane == 0) s_q = acc;
    }
    __syncthreads();
    const double q = s_q;
    const double r = sqrt(q > 1e-12 ? q : 1e-12);
    for (int c = tid; c < p.C; c += kVladReduceBlock) p.U[(size_t)k * p.C + c] = wv[c] / r;
}

// q = orc_dot_tree_f64(U, U, n) over the k-major flattening by wave 0, v = (float)(U / sqrt(q > 1e-12 ? q : 1e-12)); the vector goes out
// as float32 (vf) and / or as the doubles the append's staging buffer holds (vd), whichever is not null.  One workgroup per map of the
// group: U, vf and vd of map blockIdx.x are n elements further on.
__global__ __launch_bounds__(kVladFinishBlock) void vlad_finish(const double *U, float *vf, double *vd, int32_t n)
{
    __shared__ double s_q;
    const int tid = threadIdx.x, lane = tid & 63;
    U += (size_t)blockIdx.x * n;
    if (vf) vf += (size_t)blockIdx.x * n;
    if (vd) vd += (size_t)blockIdx.x * n;
    if (tid < 64) {
        double acc = 0.0;
        constexpr int UF = 16;   // 1-KiB wave loads in flight: the chain is 2 n / 128 fmas long, the trips to the L2 are what it waits for
        for (int base = 0; base < n; base += 128 * UF) {
            f64x2 u[UF];
#pragma unroll
            for (int i = 0; i < UF; i++) {
                const int e = base + 128 * i + 2 * lane;
                u[i] = e < n ? *reinterpret_cast<const f64x2 *>(U + e) : f64x2{0.0, 0.0};
            }
#pragma unroll
            for (int i = 0; i < UF; i++) {
                if (base + 128 * i + 2 * lane < n) {
                    acc = __builtin_fma(u[i][0], u[i][0], acc);
                    acc = __builtin_fma(u[i][1], u[i][1], acc);
                }
            }
        }
        acc = vlad_butterfly(acc);
        if (lane == 0) s_q = acc;
    }
    __syncthreads();
    const double q = s_q;
    const double r = sqrt(q > 1e-12 ? q : 1e-12);
    for (int e = tid; e < n; e += kVladFinishBlock) {
        const float f = (float)(U[e] / r);
        if (vf) vf[e] = f;
        if (vd) vd[e] = (double)f;
    }
}

static bool vlad_limits_ok(int32_t C, int32_t K, int32_t G)
{
    if (C < 4 || C > 1024 || C % 4 != 0) return false;
    if (K < 1 || G < 0 || K > 128 || G > 128 || K + G > 128) return false;
    return (K + G) * C <= 32768 && K * C <= CHIP_PROJ_MAX_IN_DIM;
}

// A group: as many maps as keep its positions <= 32768, at least 1 and at most 16.  The scratch is sized for one group, and a group
// costs the launches one map costs.
static int vlad_group_maps(int32_t N)
{
    const int g = 32768 / N;
    return g < 1 ? 1 : g > 16 ? 16 : g;
}

// `maps` maps of N positions each, one after the other in `layout` at fmaps (host memory, or device memory of the ctx's device) -> Vlad::x
// as maps x N x C, then pooled: map m's v as float32 into vf + m * K*C and / or as doubles into vd + m * K*C; a non-finite score raises
// bit1 of *flag.  The append lock is held.  A copy (NCHW: and the transposing launch), then four launches on s_append.
// Every caller holds a ResidentPause, and this is the argument for it.  vlad_assign (256 threads, no LDS), vlad_aggregate (64
// threads, 4 KiB) and vlad_reduce (256 threads, 8 KiB) would find room beside the resident scan instance's one workgroup per CU on any CU
// with four free wave slots and their registers -- but that is a statement about the instance's register allocation, which this file
// does not own, and vlad_finish is a 1024-thread workgroup, which has no room beside another of that size.  A launch that cannot be
// placed waits for as long as ticks renew the instance's lease (project.hip project_chunk), so the pooling does not clearly fit and
// pauses: correctness first.  The route through a projection pauses for project_rows anyway.
static int vlad_group(Ctx *c, const float *fmaps, int maps, int32_t N, int32_t layout, float *vf, double *vd, uint32_t *flag)
{
    Vlad &v = c->vlad;
    const int KG = v.K + v.G, blocks = (N + CHIP_VLAD_BLOCK - 1) / CHIP_VLAD_BLOCK;
    const size_t KC = (size_t)v.K * v.C, count = (size_t)maps * N * v.C;
    v.last_n = 0;
    int rc = v.x.reserve(c, count);
    if (rc == CHIP_OK && layout != CHIP_VLAD_NHWC) rc = v.raw.reserve(c, count);
    if (rc == CHIP_OK) rc = v.a.reserve(c, (size_t)maps * N * KG);
    if (rc == CHIP_OK) rc = v.part.reserve(c, (size_t)maps * blocks * (KC + v.K));
    if (rc == CHIP_OK) rc = v.vu.reserve(c, (size_t)maps * (2 * KC + v.K));
    if (rc != CHIP_OK) return rc;
    if (layout == CHIP_VLAD_NHWC) {
        CHIP_HIP(c, hipMemcpyAsync(v.x, fmaps, count * sizeof(float), hipMemcpyDefault, c->s_append));
    } else {
        CHIP_HIP(c, hipMemcpyAsync(v.raw, fmaps, count * sizeof(float), hipMemcpyDefault, c->s_append));
        hipLaunchKernelGGL(vlad_transpose, dim3((N + 31) / 32, (v.C + 31) / 32, maps), dim3(256), 0, c->s_append, (const float *)v.raw.get(), v.x.get(), N, v.C);
    }
    VladArgs p;
    p.x = v.x;
    p.Wt = v.Wt();
    p.bias = v.bias();
    p.centres = v.centres();
    p.a = v.a;
    p.P = v.part;
    p.S = v.part + (size_t)maps * blocks * KC;
    p.V = v.vu;
    p.U = v.vu + (size_t)maps * KC;
    p.A = v.vu + 2 * (size_t)maps * KC;
    p.flag = flag;
    p.N = N;
    p.C = v.C;
    p.K = v.K;
    p.KG = KG;
    p.blocks = blocks;
    p.maps = maps;
    const int waves = kVladAssignBlock / 64;
    int grid = (maps * N + waves - 1) / waves;
    if (grid > c->n_cus * 8) grid = c->n_cus * 8;
    hipLaunchKernelGGL(vlad_assign, dim3(grid), dim3(kVladAssignBlock), 0, c->s_append, p);
    hipLaunchKernelGGL(vlad_aggregate, dim3(maps * blocks, (v.C + 63) / 64, (v.K + kVladKT - 1) / kVladKT), dim3(64), 0, c->s_append, p);
    hipLaunchKernelGGL(vlad_reduce, dim3(v.K, maps), dim3(kVladReduceBlock), 0, c->s_append, p);
    hipLaunchKernelGGL(vlad_finish, dim3(maps), dim3(kVladFinishBlock), 0, c->s_append, (const double *)p.U, vf, vd, (int32_t)KC);
    CHIP_HIP(c, hipGetLastError());
    v.last_n = N;
    v.last_maps = maps;
    return CHIP_OK;
}

// Maps [from, from + m) of a pooled append -> rows 0 .. m-1 of stage_dev (append_pass; ctx_append has checked the shapes and holds the
// pause), group by group.  With a projection the pooled vectors are written where project_stage_input would have put them -- the chunk's
// own m descriptors, from 0 -- and the chunk goes on as the projected append does, its groups sharing the passes over the matrix;
// without one the last kernel writes (double)v into the staging buffer.  The flag word is the append's own: store_rows reads it next.
// The maps are read from the caller's memory here, so a call that is run twice (an empty undecided DB that becomes a double-row DB)
// copies them twice.
int vlad_chunk(Ctx *c, const AppendSrc &src, int64_t from, int64_t m)
{
    Vlad &v = c->vlad;
    const size_t KC = (size_t)v.K * v.C, map_elems = (size_t)src.positions * v.C;
    const bool through = c->proj.in_dim != 0;
    if (through) {
        const int rc = c->proj.x.reserve(c, (size_t)m * KC);
        if (rc != CHIP_OK) return rc;
    }
    double *stage = reinterpret_cast<double *>(c->stage_dev.get());
    const int gmax = vlad_group_maps(src.positions);
    for (int64_t i = 0; i < m; i += gmax) {
        const int g = (int)(m - i < gmax ? m - i : gmax);
        const int rc = vlad_group(c, src.fmap + (size_t)(from + i) * map_elems, g, src.positions, src.layout,
                                  through ? c->proj.x + (size_t)i * KC : nullptr, through ? nullptr : stage + (size_t)i * KC, c->flags_dev);
        if (rc != CHIP_OK) return rc;
    }
    return through ? project_chunk(c, 0, m) : CHIP_OK;
}

static int check_poolable(const Ctx *c) { return (c->group || c->nranks > 1) ? CHIP_ERR_UNSUPPORTED : CHIP_OK; }

}  // namespace chip

using namespace chip;

extern "C" {

int chip_build_has_vlad(void) { return 1; }

int chip_vlad_set(chip_ctx *c, int32_t channels, int32_t clusters, int32_t ghost, const float *Wt, const float *bias, const float *centres)
{
    if (!c || !Wt || !bias || !centres) return CHIP_ERR_INVALID_ARG;
    if (!vlad_limits_ok(channels, clusters, ghost)) return CHIP_ERR_UNSUPPORTED;
    int rc = check_poolable(c);
    if (rc != CHIP_OK) return rc;
    const int KG = clusters + ghost;
    const size_t nw = (size_t)KG * channels, nc = (size_t)clusters * channels;
    for (size_t i = 0; i < nw; i++) if (!std::isfinite(Wt[i])) return CHIP_ERR_NONFINITE;
    for (int i = 0; i < KG; i++) if (!std::isfinite(bias[i])) return CHIP_ERR_NONFINITE;
    for (size_t i = 0; i < nc; i++) if (!std::isfinite(centres[i])) return CHIP_ERR_NONFINITE;
    std::lock_guard<std::mutex> alk(c->append_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    Vlad fresh_layout;   // only for the offsets of the new shape
    fresh_layout.C = channels;
    fresh_layout.K = clusters;
    fresh_layout.G = ghost;
    const size_t nb = (size_t)fresh_layout.bias_count();
    std::vector<double> bias64(nb, 0.0);
    for (int i = 0; i < KG; i++) bias64[(size_t)i] = (double)bias[i];
    // The new weights are complete in a buffer of their own before they replace the old ones (chip_project_set): a failure leaves the
    // earlier set in place.  One pause over the exchange (declared first: the old buffer is freed before it ends).
    ResidentPause paused(c);
    DevBuf<char> fresh;
    rc = fresh.reserve(c, nb * sizeof(double) + (nw + nc) * sizeof(float));
    if (rc != CHIP_OK) return rc;
    char *base = fresh.get();
    CHIP_HIP(c, hipMemcpyAsync(base, bias64.data(), nb * sizeof(double), hipMemcpyHostToDevice, c->s_append));
    CHIP_HIP(c, hipMemcpyAsync(base + nb * sizeof(double), Wt, nw * sizeof(float), hipMemcpyHostToDevice, c->s_append));
    CHIP_HIP(c, hipMemcpyAsync(base + nb * sizeof(double) + nw * sizeof(float), centres, nc * sizeof(float), hipMemcpyHostToDevice, c->s_append));
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    Vlad &v = c->vlad;
    v.w.swap(fresh);
    v.C = channels;
    v.K = clusters;
    v.G = ghost;
    v.last_n = 0;
    return CHIP_OK;
}

int chip_vlad_clear(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_poolable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    Vlad &v = c->vlad;
    ResidentPause paused(c, v.C != 0);
    v.w.release();
    v.raw.release();
    v.x.release();
    v.a.release();
    v.part.release();
    v.vu.release();
    v.out.release();
    v.C = v.K = v.G = 0;
    v.last_n = 0;
    return CHIP_OK;
}

int chip_vlad_info(const chip_ctx *cc, int32_t *channels, int32_t *clusters, int32_t *ghost)
{
    if (!cc) return CHIP_ERR_INVALID_ARG;
    chip_ctx *c = const_cast<chip_ctx *>(cc);
    const int rc = check_poolable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    if (channels) *channels = c->vlad.C;
    if (clusters) *clusters = c->vlad.K;
    if (ghost) *ghost = c->vlad.G;
    return CHIP_OK;
}

int chip_vlad_batch(chip_ctx *c, const float *fmaps, int32_t n_maps, int32_t positions, int32_t layout, float *out)
{
    if (!c || !fmaps || !out || n_maps < 0) return CHIP_ERR_INVALID_ARG;
    if (positions < 1 || positions > CHIP_VLAD_MAX_POSITIONS || (layout != CHIP_VLAD_NHWC && layout != CHIP_VLAD_NCHW)) return CHIP_ERR_UNSUPPORTED;
    int rc = check_poolable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    Vlad &v = c->vlad;
    if (!v.C) return CHIP_ERR_BUSY;
    if (n_maps == 0) return CHIP_OK;
    CHIP_HIP(c, hipSetDevice(c->device));
    ResidentPause paused(c);   // vlad_group says why
    const size_t KC = (size_t)v.K * v.C, map_elems = (size_t)positions * v.C;
    const int gmax = vlad_group_maps(positions), g0 = n_maps < gmax ? n_maps : gmax;
    rc = v.out.reserve(c, (size_t)g0 * KC + 1);   // a group's vectors and the flag word behind them
    if (rc != CHIP_OK) return rc;
    uint32_t *flag = reinterpret_cast<uint32_t *>(v.out.get() + (size_t)g0 * KC);
    CHIP_HIP(c, hipMemsetAsync(flag, 0, sizeof(uint32_t), c->s_append));
    std::vector<float> host((size_t)n_maps * KC + 1);   // v is written only once every map is known to be finite
    for (int i = 0; i < n_maps; i += gmax) {
        const int g = n_maps - i < gmax ? n_maps - i : gmax;
        rc = vlad_group(c, fmaps + (size_t)i * map_elems, g, positions, layout, v.out, nullptr, flag);
        if (rc != CHIP_OK) return rc;
        // the last group of full size takes the flag word along: a call of one group is one copy
        const bool with_flag = i + g == n_maps && g == g0;
        CHIP_HIP(c, hipMemcpyAsync(host.data() + (size_t)i * KC, v.out, ((size_t)g * KC + (with_flag ? 1 : 0)) * sizeof(float), hipMemcpyDeviceToHost, c->s_append));
        if (i + g == n_maps && !with_flag)
            CHIP_HIP(c, hipMemcpyAsync(host.data() + (size_t)n_maps * KC, flag, sizeof(float), hipMemcpyDeviceToHost, c->s_append));
    }
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    uint32_t bad;
    std::memcpy(&bad, &host[(size_t)n_maps * KC], sizeof bad);
    if (bad & 2u) return CHIP_ERR_NONFINITE;
    std::memcpy(out, host.data(), (size_t)n_maps * KC * sizeof(float));
    return CHIP_OK;
}

int chip_vlad(chip_ctx *c, const float *fmap, int32_t positions, int32_t layout, float *out)
{
    return chip_vlad_batch(c, fmap, 1, positions, layout, out);
}

int chip_debug_vlad_stage(chip_ctx *c, double *a, double *V, double *A)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_poolable(c);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> alk(c->append_mu);
    Vlad &v = c->vlad;
    if (!v.C || v.last_n <= 0) return CHIP_ERR_BUSY;
    CHIP_HIP(c, hipSetDevice(c->device));
    const size_t KC = (size_t)v.K * v.C, an = (size_t)v.last_n * (v.K + v.G), m = (size_t)v.last_maps - 1;   // the last map of the last group
    if (a) CHIP_HIP(c, hipMemcpyAsync(a, v.a + m * an, an * sizeof(double), hipMemcpyDeviceToHost, c->s_append));
    if (V) CHIP_HIP(c, hipMemcpyAsync(V, v.vu + m * KC, KC * sizeof(double), hipMemcpyDeviceToHost, c->s_append));
    if (A) CHIP_HIP(c, hipMemcpyAsync(A, v.vu + 2 * (m + 1) * KC + m * v.K, (size_t)v.K * sizeof(double), hipMemcpyDeviceToHost, c->s_append));
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    return CHIP_OK;
}

}  // extern "C"
