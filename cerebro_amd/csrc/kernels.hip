// kernels.hip -- hand-written gfx950 kernels for the descriptor dot-product scan path.
//
//   K1 db_scan_topk   : replaces  u = v^T * M.leftCols(k) (x3) + maxCoeff + last-index argmax
//                       (/root/reference/src/Cerebro.cpp:1026-1043).  HBM-bound streaming kernel:
//                       one DB pass for all queries, fp64 accumulation of exact fp32 products in the
//                       fixed order of DESIGN.md 3, per-wave register top-K, per-block LDS merge.
//   K2 topk_merge     : merges per-block (or per-GPU) lists and applies the accept rule Cerebro.cpp:1056.
//   K3 narrow/copy    : M.col(_s) = desc (Cerebro.cpp:1005-1006): f64 -> f32 with a losslessness check.
//   synth             : on-device synthetic DB (spec = oracle/dot_scan.c).
//
// Storage type T is float (default: NetVLAD descriptors are float32 values on a float64 wire) or double (descriptors that
// are genuinely float64, e.g. ReljaNetVLAD's numpy WPCA output, whole_image_desc_compute_server.py:148-149).
// CDNA4 notes: wave = 64; queries live in LDS (NQ*D*sizeof(T) B) and are read with conflict-free ds_read_b128;
// DB rows are streamed with 16-B-per-lane non-temporal global loads (1 KiB per wave-instruction, U in flight
// per lane); the wave id is readfirstlane'd so row bases stay in SGPRs.  No MFMA: AI = NQ/2 flop/B.
#include "chip_internal.h"
#include "topk_merge.h"
#include <cmath>
#include <type_traits>

namespace chip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ K1
// scan -> per-wave register top-K -> per-block LDS merge -> one sorted partial list per workgroup in global memory.
// The cross-workgroup merge (+ accept decision) is K2 on the ctx stream, behind an event, so that it overlaps the
// NEXT tick's scan (a fused last-workgroup merge was measured to serialise ~28 us per tick).
template <typename T> struct Vec16;                       // 16 bytes of storage elements = one lane's share of a wave load
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<double> { typedef f64x2 type; static constexpr int N = 2; };

// DB rows are reached through a pointer loaded from the segment table, which the compiler can only treat as a GENERIC pointer:
// it would emit flat_load, which is tracked by BOTH vmcnt and lgkmcnt -- every wait for an LDS read (the staged queries) then
// also waits for the row loads in flight.  The explicit address-space cast makes them global_load (vmcnt only).
template <typename V>
__device__ __forceinline__ const __attribute__((address_space(1))) V *as_global(const V *p)
{
    return (const __attribute__((address_space(1))) V *)p;
}

// One 16-byte streaming load of a DB row chunk with the non-temporal hint, scheduled by the compiler (rows_dot, NT == 1).
template <typename V>
__device__ __forceinline__ V stream_load(const V *p)
{
    return __builtin_nontemporal_load(as_global(p));
}

// Dot products of one DB row with NQ staged queries in the fixed order of DESIGN.md 3: lane L accumulates elements
// j*CH + N*L + c (j ascending, c = 0..N-1; N = 4 / CH = 256 for float storage, N = 2 / CH = 128 for double) into one fp64
// accumulator per query by fma -- for float storage the product of two fp32 values is exact in fp64, so fma == mul-then-add;
// for double storage the single rounding of the fma IS the definition (oracle: orc_dot_tree_f64) -- then the xor butterfly
// acc[L] += acc[L ^ m], m = 32..1, after which every lane holds the same bits.
template <typename T, int NQ, int U, bool FULL, int NT, int R>
__device__ __forceinline__ void rows_dot(const T *const (&row)[R], const T *qs, int D, int lane, double (&acc)[R][NQ])
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N, CH = 64 * N;
    const int e0 = lane * N;
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[rr][q] = 0.0;
    for (int base = 0; base < D; base += CH * U) {
        V v[R][U];
        if constexpr (NT == 6 || NT == 8) {
            // all R*U loads of the batch issued back to back from one address register pair (immediate offsets), consumed
            // below behind COUNTED waits: hipcc's scheduler otherwise sinks the loads next to their uses (register pressure)
            // and the wave runs with 1-2 KiB in flight instead of U KiB
            static_assert(FULL && U <= 8, "asm path: whole batches only");
#pragma unroll
            for (int rr = 0; rr < R; rr++) {
                const char *mid = reinterpret_cast<const char *>(row[rr] + base + e0) + 4096;
#pragma unroll
                for (int u = 0; u < U; u++)
                    asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(v[rr][u]) : "v"(mid), "n"(u * 1024 - 4096) : "memory");
            }
        } else {
#pragma unroll
        for (int rr = 0; rr < R; rr++) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = base + u * CH + e0;
                if (FULL || e < D) v[rr][u] = stream_load(reinterpret_cast<const V *>(row[rr] + e));
            }
        }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int e = base + u * CH + e0;
            if constexpr (NT == 6 || NT == 8) {
#pragma unroll
                for (int rr = 0; rr < R; rr++)   // loads return in order: load (rr, u) is done once at most this many are outstanding
                    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v[rr][u]) : "n"((R - 1 - rr) * U + (U - 1 - u) < 63 ? (R - 1 - rr) * U + (U - 1 - u) : 63) : "memory");
            }
            if constexpr (NT == 8) {
                // queries staged as fp64 (scan_q64): per 64 vectors of 4 elements [64 x (d0, d1)][64 x (d2, d3)] = 2 KiB,
                // read as two conflict-free 16-B loads per lane; the products are the same exact fp64 values as (double)w * (double)v
                const char *q64 = reinterpret_cast<const char *>(qs);
                const int t = e >> 2;                                   // vector index of this lane
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const char *blk = q64 + (size_t)q * D * 8 + (size_t)(t >> 6) * 2048 + (t & 63) * 16;
                    const f64x2 wl = *reinterpret_cast<const f64x2 *>(blk), wh = *reinterpret_cast<const f64x2 *>(blk + 1024);
#pragma unroll
                    for (int rr = 0; rr < R; rr++) {
                        acc[rr][q] = __builtin_fma(wl[0], (double)v[rr][u][0], acc[rr][q]);
                        acc[rr][q] = __builtin_fma(wl[1], (double)v[rr][u][1], acc[rr][q]);
                        acc[rr][q] = __builtin_fma(wh[0], (double)v[rr][u][2], acc[rr][q]);
                        acc[rr][q] = __builtin_fma(wh[1], (double)v[rr][u][3], acc[rr][q]);
                    }
                }
            } else
            if (FULL || e < D) {
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const V w = *reinterpret_cast<const V *>(qs + q * D + e);
#pragma unroll
                    for (int rr = 0; rr < R; rr++)
#pragma unroll
                        for (int c = 0; c < N; c++) acc[rr][q] = __builtin_fma((double)w[c], (double)v[rr][u][c], acc[rr][q]);
                }
            }
        }
    }
}

__device__ __forceinline__ double butterfly_sum(double a)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a = a + __shfl_xor(a, m, 64);
    return a;
}

template <typename T, int NQ>
__device__ __forceinline__ void stage_queries(const ScanArgs &a, T *qs, int tid, int nthreads)
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const T *src = static_cast<const T *>(a.q[q]);
        for (int e = tid * N; e < a.D; e += nthreads * N)
            *reinterpret_cast<V *>(qs + q * a.D + e) = *reinterpret_cast<const V *>(src + e);
    }
}

template <typename T>
__device__ __forceinline__ const T *row_base(const ScanArgs &a, int64_t r)
{
    return static_cast<const T *>(a.seg_table[r >> a.seg_shift]) + (r & a.seg_mask) * (int64_t)a.D;
}

// Per-wave running top-K of one query: lane j < K holds the j-th best (score desc, index desc); (thr_s, thr_i) = the K-th.
// Offering a candidate is wave-uniform and rare after warm-up; NaN never enters.
__device__ __forceinline__ void wave_topk_offer(double s, int64_t gi, int K, int lane, double &my_s, int64_t &my_i, double &thr_s, int64_t &thr_i)
{
    if (key_gt(s, gi, thr_s, thr_i)) {
        const bool worse = key_gt(s, gi, my_s, my_i);
        const unsigned long long m = __ballot(worse) & ((1ull << K) - 1ull);
        const int pos = __builtin_ctzll(m);
        const double up_s = __shfl_up(my_s, 1, 64);
        const int64_t up_i = __shfl_up(my_i, 1, 64);
        if (lane < K) {
            if (lane > pos) { my_s = up_s; my_i = up_i; }
            else if (lane == pos) { my_s = s; my_i = gi; }
        }
        thr_s = __shfl(my_s, K - 1, 64);
        thr_i = __shfl(my_i, K - 1, 64);
    }
}

// Block merge: wpb sorted lists of K per query, cand[wpb][NQ][K] in LDS -> one sorted list of K per query at out_of(q), by waves 0..NQ-1.
template <int NQ, typename OutOf>
__device__ __forceinline__ void block_merge_cand(const chip_topk_entry *cand, int K, int lane, int wave, int wpb, OutOf out_of)
{
    __syncthreads();  // every wave's lists are in LDS
    for (int q = wave; q < NQ; q += wpb) {
        const int ncand = wpb * K;  // <= 16 waves * 16 = 256 -> at most 4 per lane
        double cs[4];
        int64_t ci[4];
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const int c = lane + 64 * h;
            if (c < ncand) {
                const chip_topk_entry t = cand[((c / K) * NQ + q) * K + (c % K)];
                cs[h] = t.score;
                ci[h] = t.idx;
            } else { cs[h] = -INFINITY; ci[h] = -1; }
        }
        chip_topk_entry *outp = out_of(q);   // where this query's list of K goes
        for (int j = 0; j < K; j++) {
            double bs = cs[0];
            int64_t bi = ci[0];
#pragma unroll
            for (int h = 1; h < 4; h++)
                if (key_gt(cs[h], ci[h], bs, bi)) { bs = cs[h]; bi = ci[h]; }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double os = __shfl_xor(bs, m, 64);
                const int64_t oi = __shfl_xor(bi, m, 64);
                if (key_gt(os, oi, bs, bi)) { bs = os; bi = oi; }
            }
#pragma unroll
            for (int h = 0; h < 4; h++)
                if (ci[h] == bi && cs[h] == bs) { cs[h] = -INFINITY; ci[h] = -1; }
            if (lane == 0) { chip_topk_entry t; t.score = bs; t.idx = bi; outp[j] = t; }
        }
    }
}

// The same for lists held in registers: they go to LDS over the staged queries first.
template <int NQ, typename OutOf>
__device__ __forceinline__ void block_merge_store(char *smem, const double (&my_s)[NQ], const int64_t (&my_i)[NQ],
                                                  int K, int lane, int wave, int wpb, OutOf out_of)
{
    __syncthreads();  // all waves done with the staged queries; reuse LDS
    chip_topk_entry *cand = reinterpret_cast<chip_topk_entry *>(smem);  // [wpb][NQ][K]
    if (lane < K) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            chip_topk_entry t;
            t.score = my_s[q];
            t.idx = my_i[q];
            cand[(wave * NQ + q) * K + lane] = t;
        }
    }
    block_merge_cand<NQ>(cand, K, lane, wave, wpb, out_of);
}

// The same for a WAVE-UNIFORM row through the scalar cache: the table is read with s_load (constant address space; entries of
// published rows never change), so the lookup neither costs a vector-memory round trip nor touches vmcnt.
template <typename T, typename Args>
__device__ __forceinline__ const T *row_base_uniform(const Args &a, int64_t r)
{
    typedef const uint64_t __attribute__((address_space(4))) *ctab;
    const uint64_t seg = ((ctab)(uintptr_t)a.seg_table)[r >> a.seg_shift];
    return reinterpret_cast<const T *>((uintptr_t)seg) + (r & a.seg_mask) * (int64_t)a.D;
}

// a wave-uniform pointer the compiler cannot prove uniform (it came out of the segment table) -> SGPR pair
template <typename P>
__device__ __forceinline__ const P *uniform_ptr(const P *p)
{
    const uint64_t b = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return reinterpret_cast<const P *>((uintptr_t)(((uint64_t)hi << 32) | lo));
}

template <typename T, int NQ, int U, bool FULL, int NT, int R>
__global__ __launch_bounds__(1024) void db_scan_topk(ScanArgs a)
{
    static_assert(R == 1, "one row per wave at a time");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *qs = reinterpret_cast<T *>(smem);  // [NQ][D]
    const int D = a.D;
    const int K = a.K;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpb = blockDim.x >> 6;

    // stage the query descriptors once per block (L2-resident after the first block)
    if constexpr (NT == 8) {
        char *q64 = reinterpret_cast<char *>(smem);
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float *src = static_cast<const float *>(a.q[q]);
            for (int t = tid; t < (a.D >> 2); t += blockDim.x) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(src + 4 * t);
                char *blk = q64 + (size_t)q * a.D * 8 + (size_t)(t >> 6) * 2048 + (t & 63) * 16;
                *reinterpret_cast<f64x2 *>(blk) = (f64x2){(double)w[0], (double)w[1]};
                *reinterpret_cast<f64x2 *>(blk + 1024) = (f64x2){(double)w[2], (double)w[3]};
            }
        }
    } else {
        stage_queries<T, NQ>(a, qs, tid, blockDim.x);
    }
    __syncthreads();

    // per-wave running top-K: lane j < K holds the j-th best (score desc, index desc)
    double my_s[NQ], thr_s[NQ];
    int64_t my_i[NQ], thr_i[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) { my_s[q] = -INFINITY; my_i[q] = -1; thr_s[q] = -INFINITY; thr_i[q] = -1; }

    // Row -> wave map: wave g (global index) owns rows g, g + tw, g + 2 tw, ... -- adjacent waves read adjacent rows and all
    // waves together read ONE window of tw consecutive rows that slides through the DB.  Measured alternatives, all slower or
    // not worth their machinery: a contiguous run of rows per wave / per workgroup / per XCD (-3 .. -6 %);
    // chunks claimed from a device-wide counter so that the XCDs that get less HBM bandwidth claim fewer (same-address atomics
    // sustain ~85 M/s and VMEM returns in order, so the claiming wave's row loads wait for its atomic: -2 %); a static 3-5 %
    // skew of the row share between even and odd XCDs (+0.5 .. +1.9 % depending on the box).
    const int64_t tw = (int64_t)gridDim.x * wpb;
    for (int64_t r = (int64_t)blockIdx.x * wpb + wave; r < a.n_rows; r += tw) {
        const T *row[1] = {row_base<T>(a, r)};
        double acc[1][NQ];
        rows_dot<T, NQ, U, FULL, NT, 1>(row, qs, D, lane, acc);
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[0][q] = butterfly_sum(acc[0][q]);
        const int64_t gi = r * a.idx_mul + a.idx_add;
#pragma unroll
        for (int q = 0; q < NQ; q++) wave_topk_offer(acc[0][q], gi, K, lane, my_s[q], my_i[q], thr_s[q], thr_i[q]);
    }

    block_merge_store<NQ>(smem, my_s, my_i, K, lane, wave, wpb, [&](int q) { return a.partial + ((int64_t)blockIdx.x * NQ + q) * K; });
}

// ------------------------------------------------------------------------------------------------ K1, several ticks per pass
// ONE pass over rows [0, max k_t) answers T queued ticks of 3 queries each (chip_api.hip coalesce_*): the pass is as HBM-bound as a
// one-tick launch, so T ticks cost one DB read.  Four kernels, ONE skeleton (shared_pass below) and one arithmetic policy each:
//   db_scan_topk_multi<T>     float rows,  T = 2, 3, fp64 arithmetic (PassF64<float, T, 0>): every query staged in LDS;
//   db_scan_shared_f64<T, NG> double rows, T = 2,    fp64 arithmetic (PassF64<double, T, NG>): NG queries read in place;
//   db_scan_prefilter<NG>     float rows,  T = 4,    fp32 arithmetic (PassF32<NG>): candidates for tick_rescore, NG queries in place;
//   db_scan_halfq             float rows,  T = 5,    fp32 arithmetic on queries staged as fp16 (PassF32H): candidates for tick_rescore.
// What the skeleton owns, whatever the arithmetic:
//   * register blocking: R = 4 rows per wave in flight, U = 4 KiB of each per batch (16 KiB per wave, one workgroup of 8 waves per CU),
//     rows of whole 4 KiB batches, plain ctx;
//   * queries: the first NS = 3T - NG staged in LDS in the rows' type ([NS][D]), read by ds_read_b128 two vectors ahead of their use;
//     the last NG (those the LDS does not hold) read IN PLACE from global memory: every wave of the launch reads the same bytes, so they
//     come out of the L2.  Vector loads return in order and share vmcnt with the row stream, so an in-place query vector is one more
//     slot OF that stream: the stream of a wave is r0 r1 r2 r3 g0 .. g(NG-1) per KiB, L = 4 (4 + NG) loads in flight;
//   * per-tick prefix: a row is offered to tick t's lists only if row < k_t (wave-uniform compare); the running lists sit in LDS
//     behind the queries ([wave][3T][K] entries), the admission thresholds in SGPRs; one vector compare per query tells whether any
//     row of a group can enter a list at all, and the offers of such a group are walked list by list;
//   * output [tick][workgroup][3][K]: the merge + decision kernel runs unchanged, once per tick, on its own block of lists.
constexpr int kMultiR = 4, kMultiU = 4, kMultiBlock = 512;

// The load slots of a wave (1 KiB each) are PHYSICAL registers that the compiler does not own, as in db_scan_topk_rows below (same
// reason, same technique: amdgpu_num_vgpr leaves the top of the file to the asm statements, which name their targets literally;
// tests/test_codeobj_multi.py, test_codeobj_shared_f64.py check the partition).  One map for all three kernels:
//   rows   : slot (u, rr), KiB u of the batch of row rr      -> v[192 + 4 (4 u + rr) ..]: v[192..255];
//   queries: slot (u, g),  KiB u of the batch of in-place g  -> v[192 - 16 NG + 4 (NG u + g) ..], right below the row slots.
// A kernel's attribute takes no template argument, so the compiler's share is what the widest instantiation of the kernel leaves.
constexpr int kMultiVgprBase = 192;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the shared-pass kernels name physical VGPRs: gfx950 (MI355X) only -- build with --offload-arch=gfx950"
#endif
#define CHIP_PASS_SLOTS_192_255                                                                                                         \
    "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207",     \
    "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223",     \
    "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239",     \
    "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"
#define CHIP_PASS_SLOTS_160_191                                                                                                         \
    "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175",     \
    "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191"
#define CHIP_PASS_SLOTS_144_159                                                                                                         \
    "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159"
__host__ __device__ constexpr int pass_row_slot(int u, int rr) { return kMultiVgprBase + 4 * (u * kMultiR + rr); }
__host__ __device__ constexpr int pass_query_slot(int ng, int u, int g) { return kMultiVgprBase - 4 * kMultiU * ng + 4 * (u * ng + g); }
__host__ __device__ constexpr int pass_vgpr_base(int max_ng) { return kMultiVgprBase - 4 * kMultiU * max_ng; }   // what the compiler owns

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose counter names registers (template arguments of the asm statements)
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}
#define CHIP_INLINE_LAMBDA __attribute__((always_inline))

// 1 KiB (16 bytes per lane) into a slot: wave-uniform base in an SGPR pair, one shared 32-bit lane offset; rows non-temporal (read once),
// in-place queries cached (every wave reads them)
template <int REG, int OFF, bool NTL>
__device__ __forceinline__ void slot_issue(uint32_t voff, const void *base_uniform)
{
    if constexpr (NTL)
        asm volatile("global_load_dwordx4 v[%2:%3], %0, %1 offset:%4 nt" ::"v"(voff), "s"(base_uniform), "n"(REG), "n"(REG + 3), "n"(OFF) : "memory");
    else
        asm volatile("global_load_dwordx4 v[%2:%3], %0, %1 offset:%4" ::"v"(voff), "s"(base_uniform), "n"(REG), "n"(REG + 3), "n"(OFF) : "memory");
}
// KiB U_ of a batch, in the stream's order: the four row slots, then the NG query slots
template <int U_, int NG, typename T>
__device__ __forceinline__ void slots_issue_kib(uint32_t voff, const T *const (&row)[kMultiR], const T *const (&qg)[NG > 0 ? NG : 1])
{
    static_for<kMultiR>([&](auto rr) CHIP_INLINE_LAMBDA { slot_issue<pass_row_slot(U_, rr), U_ * 1024, true>(voff, row[rr]); });
    static_for<NG>([&](auto g) CHIP_INLINE_LAMBDA { slot_issue<pass_query_slot(NG, U_, g), U_ * 1024, false>(voff, qg[g]); });
}
// wait until at most CNT loads of the stream are outstanding (they return in order) ...
template <int CNT>
__device__ __forceinline__ void slot_wait()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CNT) : "memory");
}
// ... and hand the slot's elements to the compiler as fp64 in the same statement: once it has been issued the slot may be loaded again.
// Four floats are converted (fp32 x fp32 is exact in fp64 wherever the conversion happens), two doubles are copied out.
template <int REG, int CNT>
__device__ __forceinline__ void slot_take(double (&d)[4])
{
    asm volatile("s_waitcnt vmcnt(%4)\n\tv_cvt_f64_f32 %0, v[%5]\n\tv_cvt_f64_f32 %1, v[%6]\n\tv_cvt_f64_f32 %2, v[%7]\n\tv_cvt_f64_f32 %3, v[%8]"
                 : "=v"(d[0]), "=v"(d[1]), "=v"(d[2]), "=v"(d[3])
                 : "n"(CNT), "n"(REG), "n"(REG + 1), "n"(REG + 2), "n"(REG + 3)
                 : "memory");
}
template <int REG, int CNT>
__device__ __forceinline__ void slot_take(double (&d)[2])
{
    asm volatile("s_waitcnt vmcnt(%2)\n\tv_mov_b64 %0, v[%3:%4]\n\tv_mov_b64 %1, v[%5:%6]"
                 : "=&v"(d[0]), "=&v"(d[1])
                 : "n"(CNT), "n"(REG), "n"(REG + 1), "n"(REG + 2), "n"(REG + 3)
                 : "memory");
}

// The running top-K lists of the shared-pass and the row-batched kernels live in LDS behind the staged queries, only the admission
// threshold (the K-th entry) stays in SGPRs: after warm-up an offer is rare, and lists held in VGPRs (as in db_scan_topk) would cost
// 4 NQ registers of kernels that keep 16 load slots per wave in flight.
__device__ __forceinline__ void wave_topk_offer_lds(double s, int64_t gi, int K, int lane, chip_topk_entry *list, double &thr_s, int64_t &thr_i)
{
    if (key_gt(s, gi, thr_s, thr_i)) {   // wave-uniform; NaN never enters
        chip_topk_entry me, up;
        me.score = -INFINITY; me.idx = -1; up = me;
        if (lane < K) { me = list[lane]; if (lane > 0) up = list[lane - 1]; }
        const bool worse = key_gt(s, gi, me.score, me.idx);
        const unsigned long long m = __ballot(worse) & ((1ull << K) - 1ull);
        const int pos = __builtin_ctzll(m);
        if (lane < K) {
            if (lane > pos) me = up;
            else if (lane == pos) { me.score = s; me.idx = gi; }
            list[lane] = me;      // every read of the old list precedes this write in program order (one wave, in-order LDS)
        }
        thr_s = readlane_f64(me.score, K - 1);
        thr_i = readlane_i64(me.idx, K - 1);
    }
}

// Lane exchanges of the transposed reduction, on a double (both dwords) or a float.  dpp: the value of the lane that the DPP control
// CTRL pairs this lane with (all lanes active).  The controls used here (row_ror, quad_perm) read a valid lane for every lane, so the
// `old` operand never shows: bound_ctrl saves the compiler the move that would fill it in.
template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// gfx950's half exchanges.  WIDTH 32: lanes 32-63 of a change places with lanes 0-31 of b; WIDTH 16: the odd 16-lane rows of a with the
// even rows of b.  (Builtins: the compiler places the wait states a VALU write of an operand needs.)
template <int WIDTH>
__device__ __forceinline__ void lane_swap(unsigned &a, unsigned &b)
{
    static_assert(WIDTH == 32 || WIDTH == 16, "v_permlane32_swap / v_permlane16_swap");
    if constexpr (WIDTH == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
        a = r[0];
        b = r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
        a = r[0];
        b = r[1];
    }
}
template <int WIDTH>
__device__ __forceinline__ void lane_swap(float &a, float &b)
{
    unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
    lane_swap<WIDTH>(ua, ub);
    a = __uint_as_float(ua);
    b = __uint_as_float(ub);
}
template <int WIDTH>
__device__ __forceinline__ void lane_swap(double &a, double &b)
{
    unsigned la = (unsigned)__double2loint(a), lb = (unsigned)__double2loint(b), ha = (unsigned)__double2hiint(a), hb = (unsigned)__double2hiint(b);
    lane_swap<WIDTH>(la, lb);
    lane_swap<WIDTH>(ha, hb);
    a = __hiloint2double((int)ha, (int)la);
    b = __hiloint2double((int)hb, (int)lb);
}
__device__ __forceinline__ double lane_value(double v, int l) { return readlane_f64(v, l); }
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The lane sums a0 .. a3 of four rows against one query -> one register whose 16-lane row k holds, in all 16 lanes, the sum of data row k.
// Per row the xor butterfly's pairing tree (m = 32, 16, 8, 4, 2, 1: lane l with lane l ^ m) is computed TRANSPOSED, each row's tree in a
// quarter of the lanes, without LDS:
//   step 32: swap32(rows 0, 2), one addition: lanes 0-31 hold row 0's a[l] + a[l ^ 32], lanes 32-63 row 2's; likewise rows 1, 3;
//   step 16: swap16 of the two results, one addition: 16-lane row k holds the sums of data row k after steps 32 and 16;
//   steps 8, 4, 2, 1 stay inside a 16-lane row and take the partner's value by DPP: row_ror:8 IS lane ^ 8; after step 8 a value
//     depends on lane & 7 only, so row_ror:4 delivers the bits of lane ^ 4, and the quad permutations are lane ^ 2 and lane ^ 1.
// The same pairs as butterfly_sum, and a + b == b + a: all 16 lanes of row k end with the bits lane 0 of the full tree holds.
template <typename S>
__device__ __forceinline__ S reduce_rows4(S a0, S a1, S a2, S a3)
{
    static_assert(kMultiR == 4, "the transposed reduction folds four rows into the four 16-lane rows of a wave");
    lane_swap<32>(a0, a2);
    lane_swap<32>(a1, a3);
    S p02 = a0 + a2, p13 = a1 + a3;
    lane_swap<16>(p02, p13);
    S v = p02 + p13;
    v = v + dpp<0x128>(v);
    v = v + dpp<0x124>(v);
    v = v + dpp<0x4E>(v);
    v = v + dpp<0xB1>(v);
    return v;
}

// Admission of a row to one running list of a shared pass; S is the type of score and threshold (the list entry is a double either way:
// a float widens exactly).  The score comes in SGPRs (all 16 lanes of the row's share of the wave hold the same bits after the
// reduction), so the compare is a scalar branch and the threshold stays in SGPRs.  A wave meets its rows in ascending order, so gi is
// larger than every index already in its lists and key_gt(s, gi, thr_s, thr_i) is just s >= thr_s (false for NaN, which never
// enters): the K-th index need not be kept.  The list's LDS address is formed inside the branch (hoisted out of the scan loop, the
// 3T x 2 addresses would be held in registers for an insertion that is rare after the first rows).
// SCALED (db_scan_halfq): scores and thresholds of the pass are 2^e times the scores the lists hold; a score is multiplied by sc_down = 2^-e on
// its way into the list and the K-th entry by sc_up = 2^e on its way back, both in fp64 and both exact, so the order is the same on either side.
template <typename S, bool SCALED = false>
__device__ __forceinline__ void pass_offer(S s_uniform, int64_t gi, int K, int lane, chip_topk_entry *list, S &thr_s, double sc_down = 1.0, double sc_up = 1.0)
{
    if (s_uniform >= thr_s) {
        asm volatile("" : "+v"(lane));
        double s = (double)s_uniform;
        if constexpr (SCALED) s *= sc_down;
        chip_topk_entry me, up;
        me.score = -INFINITY; me.idx = -1; up = me;
        if (lane < K) { me = list[lane]; if (lane > 0) up = list[lane - 1]; }
        const bool worse = key_gt(s, gi, me.score, me.idx);
        const unsigned long long m = __ballot(worse) & ((1ull << K) - 1ull);
        const int pos = __builtin_ctzll(m);
        if (lane < K) {
            if (lane > pos) me = up;
            else if (lane == pos) { me.score = s; me.idx = gi; }
            list[lane] = me;      // every read of the old list precedes this write in program order (one wave, in-order LDS)
        }
        if constexpr (SCALED) thr_s = (S)(readlane_f64(me.score, K - 1) * sc_up);
        else thr_s = (S)readlane_f64(me.score, K - 1);   // exact: every score of the list came in as an S
    }
}

// Staging as most policies do it: the first NS queries copied into LDS as they are, [NS][D] in the rows' type.
template <typename T, int NS>
__device__ __forceinline__ void pass_stage_copy(T *qs, const PassArgs &a, int tid)
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N;
    const int D = a.D;
    for (int e = tid * N; e < D; e += blockDim.x * N) {   // all NS loads of a lane in flight together (L2-resident after the first workgroup)
        V w[NS];
#pragma unroll
        for (int q = 0; q < NS; q++) w[q] = *as_global(reinterpret_cast<const V *>(static_cast<const T *>(a.q[q]) + e));
#pragma unroll
        for (int q = 0; q < NS; q++) *reinterpret_cast<V *>(qs + q * D + e) = w[q];
    }
}

// The skeleton.  A policy P says how the staged queries look in LDS (P::Staged, P::stage), what one batch does to the accumulators (P::batch: takes and re-issues every slot of the batch once, in the
// stream's order) and how a lane's accumulator becomes its sum (P::lane_sum); everything else is here, once.
template <class P>
__device__ __forceinline__ void shared_pass(const PassArgs &a)
{
    typedef typename P::Elem T;          // rows and queries as stored
    typedef typename P::Score S;         // scores and thresholds
    typedef typename P::Staged Q;        // a staged query element in LDS
    constexpr int NQ = P::NQ, NG = P::NG, NS = NQ - NG, R = kMultiR, U = kMultiU, N = Vec16<T>::N;
    constexpr int BATCH = 64 * N * U;    // elements of a 4 KiB batch
    static_assert(pass_vgpr_base(NG) >= P::kVgprBase && pass_row_slot(U - 1, R - 1) + 4 <= 256, "load slots inside the asm's share of the register file");
    static_assert(NG >= 0 && NS >= 2 && P::L == U * (R + NG) && P::L <= 64, "at least two staged queries (the LDS read-ahead), vmcnt counts to 63");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    asm volatile("" ::: CHIP_PASS_SLOTS_192_255);                    // makes the code object allocate the asm-owned registers
    if constexpr (P::kVgprBase <= 160) asm volatile("" ::: CHIP_PASS_SLOTS_160_191);
    if constexpr (P::kVgprBase <= 144) asm volatile("" ::: CHIP_PASS_SLOTS_144_159);
    Q *qs = reinterpret_cast<Q *>(smem);  // [NS][D]
    const int D = a.D;
    const int K = a.K;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpb = blockDim.x >> 6;

    P::stage(qs, a, tid);
    __syncthreads();
    const T *qg[NG > 0 ? NG : 1];   // the queries read in place (SGPRs)
#pragma unroll
    for (int g = 0; g < NG; g++) qg[g] = uniform_ptr(static_cast<const T *>(a.q[NS + g]));

    // running top-K lists: LDS behind the queries, [wave][3T][K] (this wave's lists are touched by this wave only until the merge)
    chip_topk_entry *lists = reinterpret_cast<chip_topk_entry *>(smem + (size_t)NS * D * sizeof(Q));
    chip_topk_entry *mylists = lists + (size_t)wave * NQ * K;
    S thr_s[NQ];   // score of the K-th entry of each list (SGPRs)
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        thr_s[q] = -INFINITY;
        if (lane < K) { chip_topk_entry t; t.score = -INFINITY; t.idx = -1; mylists[q * K + lane] = t; }
    }

    // Row -> wave map: as db_scan_topk (wave g owns rows g, g + tw, ...), four consecutive rows of that sequence (a GROUP) at a time --
    // all waves together read one window of 4 tw consecutive rows that slides through the DB.  A row of a group that falls beyond the
    // pass is replaced by the wave's first row (in bounds, never offered).
    //
    // The wave walks the (group, 4 KiB batch) sequence of its rows as ONE stream: a slot is loaded again -- for the next batch of
    // the group, or the first batch of the next group -- right behind the statement that took its contents, so nearly all L KiB per
    // wave are in flight through the arithmetic, through the reduction and through the offers, and every wait is counted.
    // Nothing is ever loaded from outside rows [0, n_rows) and the NG query vectors: every row base comes from row_of() below, i.e. from
    // a row < n_rows through the segment table, and every offset (rows and queries alike: both are D elements) is below one row's length.
    const int64_t tw = (int64_t)gridDim.x * wpb;
    const int64_t rbase = (int64_t)blockIdx.x * wpb + wave;
    const int nb = D / BATCH;                                                                 // batches per row
    const int ngroups = rbase < a.n_rows ? (int)((a.n_rows - 1 - rbase) / (R * tw)) + 1 : 0;  // groups of this wave (wave-uniform)
    const int total = ngroups * nb;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    const int e0 = lane * N;
    auto row_of = [&](int group, int rr) {
        const int64_t r = rbase + ((int64_t)group * R + rr) * tw;
        return uniform_ptr(row_base_uniform<T>(a, r < a.n_rows ? r : rbase));
    };
    const T *row[R], *nrow[R];   // bases the NEXT loads read from, and those of the group after (looked up one group ahead; SGPRs)
    if (total > 0) {
#pragma unroll
        for (int rr = 0; rr < R; rr++) { row[rr] = row_of(0, rr); nrow[rr] = row[rr]; }
        if (ngroups > 1) {
#pragma unroll
            for (int rr = 0; rr < R; rr++) nrow[rr] = row_of(1, rr);
        }
        static_assert(U == 4, "the prologue names the KiBs of the first batch one by one");
        slots_issue_kib<0, NG>(lane_off, row, qg); slots_issue_kib<1, NG>(lane_off, row, qg); slots_issue_kib<2, NG>(lane_off, row, qg); slots_issue_kib<3, NG>(lane_off, row, qg);
    }

    typename P::Acc acc[R][NQ];
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[rr][q] = P::zero();

    // One batch per iteration.  What the slots load next (at byte offset noff of row[] and qg[]): the next batch of the group; at the
    // group's last batch the first batch of the wave's next group; at the wave's last batch the first KiBs of the rows (and in-place
    // queries) it has just read once more (in bounds, taken by nobody), so that one loop body and one set of wait counts serve the whole stream.
    int b = 0, group = 0;
    for (int t = 0; t < total; t++) {
        const int base = b * BATCH;
        uint32_t noff = (uint32_t)(base + BATCH) * (uint32_t)sizeof(T);
        if (b + 1 == nb) {
            noff = 0;
            if (group + 1 < ngroups) {   // the slots start on the next group; its successor's bases are looked up for the boundary after
#pragma unroll
                for (int rr = 0; rr < R; rr++) row[rr] = nrow[rr];
                if (group + 2 < ngroups) {
#pragma unroll
                    for (int rr = 0; rr < R; rr++) nrow[rr] = row_of(group + 2, rr);
                }
            }
        }
        P::batch(acc, qs + base + e0, D, noff + lane_off, row, qg);
        if (++b == nb) {
            // The rows of this group are complete: R x 3T lane sums, all in one basic block ahead of the offers' branches.
            S s[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++) s[q] = reduce_rows4<S>(P::lane_sum(acc[0][q]), P::lane_sum(acc[1][q]), P::lane_sum(acc[2][q]), P::lane_sum(acc[3][q]));
            // Offers.  One vector compare per query first: s[q] holds the four rows' scores against query q, and a threshold only rises
            // while the group is offered, so a score that the loop below would admit is >= the threshold the group starts with (NaN on
            // neither side).  No lane set: nothing of this group enters any list.  Otherwise each list is offered its rows one by one, in
            // order, each against the threshold as it stands then.  (A lane may be set by a row some tick must not see, or by the stand-in
            // of a row beyond the pass: that costs the walk below, which tests both, and nothing else.)
            unsigned long long hit = 0;
#pragma unroll
            for (int q = 0; q < NQ; q++) hit |= __ballot(s[q] >= thr_s[q]);
            if (hit) {
                // The lists are independent of one another; only the rows offered to ONE list must come in ascending order.  So the walk goes
                // query first: the query's own compare once more (one vector instruction; 3T masks kept from the pre-check do not fit
                // the SGPRs), and a query none of whose four scores reaches its threshold is stepped over as a whole.  thr_s[q] changes
                // only inside q's own turn, so the compare is still against the threshold the group started with.  The empty asm below is
                // what makes it a second compare: without it the compiler reuses the pre-check's masks, keeps them live across the
                // walk and spills SGPRs, which tests/test_codeobj_multi.py refuses.
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    asm volatile("" : "+v"(s[q]));   // a value the pre-check has not seen: the compare is made again, not kept
                    if (__ballot(s[q] >= thr_s[q])) {
#pragma unroll
                        for (int rr = 0; rr < R; rr++) {
                            const int64_t r = rbase + ((int64_t)group * R + rr) * tw;
                            if (r < a.n_rows && r < a.k[q / 3]) pass_offer<S, P::kScaled>(lane_value(s[q], 16 * rr), r, K, lane, mylists + q * K, thr_s[q], P::kScaled ? a.s_down : 1.0, P::kScaled ? a.s_up : 1.0);
                        }
                    }
                }
            }
#pragma unroll
            for (int rr = 0; rr < R; rr++)
#pragma unroll
                for (int q = 0; q < NQ; q++) acc[rr][q] = P::zero();
            b = 0;
            group++;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the read-ahead of the wave's last batch

    block_merge_cand<NQ>(lists, K, lane, wave, wpb,
                         [&](int q) { return a.partial + (((int64_t)(q / 3) * gridDim.x + blockIdx.x) * 3 + q % 3) * K; });
}

// fp64 arithmetic, the bits of the one-tick kernels: per (row, query) exactly rows_dot's order -- lane L accumulates elements
// j*64N + N L + c (j ascending, c = 0 .. N - 1; N = 4 floats or 2 doubles per lane and KiB) into one fp64 accumulator by fma, then the
// pairing tree above.  Float rows are converted by the statement that takes their slot, their queries (fp32 in LDS) at use; doubles are
// copied out (2 x v_mov_b64): either way the slot is loaded again in the next statement, and EVERY wait of the loop is vmcnt(L - 1): the
// load waited for is always the oldest one.  Per KiB u: the four row slots, then the queries in order, each read (staged: two vectors
// ahead, counted lgkmcnt waits) or taken and re-issued (in place) once per 4 rows and multiplied into the four rows.
// Registers, double rows: the compiler owns v[0 .. 160): acc[4][3T] (48 at T = 2) + the 16 of a row KiB + 4 of a query vector + 12 of
// the LDS read-ahead.  T = 3 needs NG = 5 at D = 4096: 80 registers of query slots leave the compiler v[0 .. 112) for 72 of accumulators
// and everything else.  Compiled that way the kernel spills 90 registers (560 bytes of scratch per lane); a scratch access drains the
// stream, so it is dropped (kSharedF64MaxTicks).
constexpr int kSharedMaxNG = 2;          // in-place queries of the double instantiations that are built: D <= 4608 at T = 2
constexpr int kSharedF64MaxTicks = 2;
template <typename T, int NTICKS, int NG_, int MAX_NG>
struct PassF64 {
    typedef T Elem;
    typedef T Staged;
    typedef double Score;
    typedef double Acc;
    static constexpr bool kScaled = false;
    static constexpr int NQ = 3 * NTICKS, NG = NG_, NS = NQ - NG, R = kMultiR, U = kMultiU, L = U * (R + NG), kVgprBase = pass_vgpr_base(MAX_NG);
    static __device__ __forceinline__ void stage(T *qs, const PassArgs &a, int tid) { pass_stage_copy<T, NS>(qs, a, tid); }
    static __device__ __forceinline__ Acc zero() { return 0.0; }
    static __device__ __forceinline__ double lane_sum(Acc v) { return v; }
    static __device__ __forceinline__ void batch(Acc (&acc)[R][NQ], const T *qv, int D, uint32_t voff, const T *const (&row)[R], const T *const (&qg)[NG > 0 ? NG : 1])
    {
        typedef typename Vec16<T>::type V;
        constexpr int N = Vec16<T>::N, SS = U * NS;
        V w[SS];            // staged query vectors in the order they are used: (u, q < NS)
        w[0] = *reinterpret_cast<const V *>(qv);
        w[1] = *reinterpret_cast<const V *>(qv + D);
        double x[R][N];
        static_for<U * NQ>([&](auto sc) CHIP_INLINE_LAMBDA {
            constexpr int u = sc / NQ, q = sc % NQ;
            if constexpr (q == 0)
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA {
                    slot_take<pass_row_slot(u, rr), L - 1>(x[rr]);
                    slot_issue<pass_row_slot(u, rr), u * 1024, true>(voff, row[rr]);
                });
            double wd[N];
            if constexpr (q < NS) {
                constexpr int i = u * NS + q;
                if constexpr (i + 2 < SS) w[i + 2] = *reinterpret_cast<const V *>(qv + ((i + 2) % NS) * D + ((i + 2) / NS) * (64 * N));
            } else {
                slot_take<pass_query_slot(NG, u, q - NS), L - 1>(wd);
                slot_issue<pass_query_slot(NG, u, q - NS), u * 1024, false>(voff, qg[q - NS]);
            }
#pragma unroll
            for (int c = 0; c < N; c++) {
                if constexpr (q < NS) wd[c] = (double)w[u * NS + q][c];
#pragma unroll
                for (int rr = 0; rr < R; rr++) acc[rr][q] = __builtin_fma(wd[c], x[rr][c], acc[rr][q]);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
};

template <int NTICKS>
__global__ __launch_bounds__(kMultiBlock) __attribute__((amdgpu_num_vgpr(pass_vgpr_base(0) / 2))) void db_scan_topk_multi(PassArgs a)
{
    shared_pass<PassF64<float, NTICKS, 0, 0>>(a);
}

template <int NTICKS, int NG>
__global__ __launch_bounds__(kMultiBlock) __attribute__((amdgpu_num_vgpr(pass_vgpr_base(kSharedMaxNG) / 2))) void db_scan_shared_f64(PassArgs a)
{
    static_assert(NG <= kSharedMaxNG, "the compiler's share is sized for kSharedMaxNG query slots per KiB");
    shared_pass<PassF64<double, NTICKS, NG, kSharedMaxNG>>(a);
}

// ------------------------------------------------------------------------------------------------ K1, four ticks per pass, fp32 prefilter
// db_scan_prefilter<NG>: the shared pass over float rows for FOUR queued ticks (12 queries) -- in fp32.  Its lists do not decide anything:
// they are the candidate sets from which tick_rescore below PROVES which rows can be in each exact top-K and scores only those in fp64, in
// rows_dot's order (|fp32 score - exact score| <= E for every pair of published rows, whatever the order of the fp32 sum).
// What differs from the fp64 policy:
//   * arithmetic: v_pk_fma_f32 straight on the loaded registers -- per (row vector, query) two instructions, no conversion; lane L keeps
//     one accumulator PAIR per (row, query): elements 4L, 4L + 2 of every 256 go to its low half, 4L + 1, 4L + 3 to its high half.  A slot
//     is therefore loaded again only when all 12 queries have read it: per KiB u the wave waits for its four row slots at once, multiplies
//     the staged queries in, then the in-place ones (one more counted wait each), then issues the slots of u for the next batch (12 of the
//     16 row KiB stay in flight);
//   * queries: D = 4096 stages 9 (144 KiB) and reads NG = 3 in place;
//   * reduction: low + high half, then the pairing tree on single registers (any tree will do here);
//   * lists: (score widened to double -- exact --, row), thresholds as fp32 in SGPRs.  A workgroup's merged list of K holds its K best rows
//     by fp32 score; its K-th score bounds every row the workgroup dropped (each wave dropped only rows at or below its own K-th).
constexpr int kPrefilterMaxNG = 3;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// acc += (the element pair at REG of a row slot) * w, both halves at once; w in compiler registers or in a query slot at QREG
template <int REG>
__device__ __forceinline__ void prefilter_fma(f32x2 &acc, f32x2 w)
{
    asm volatile("v_pk_fma_f32 %0, v[%2:%3], %1, %0" : "+v"(acc) : "v"(w), "n"(REG), "n"(REG + 1));
}
template <int REG, int QREG>
__device__ __forceinline__ void prefilter_fma_slot(f32x2 &acc)
{
    asm volatile("v_pk_fma_f32 %0, v[%1:%2], v[%3:%4], %0" : "+v"(acc) : "n"(REG), "n"(REG + 1), "n"(QREG), "n"(QREG + 1));
}

template <int NG_>
struct PassF32 {
    typedef float Elem;
    typedef float Staged;
    typedef float Score;
    typedef f32x2 Acc;
    static constexpr bool kScaled = false;
    static constexpr int NQ = 3 * kPrefilterTicks, NG = NG_, NS = NQ - NG, R = kMultiR, U = kMultiU, L = U * (R + NG), kVgprBase = pass_vgpr_base(kPrefilterMaxNG);
    static __device__ __forceinline__ void stage(float *qs, const PassArgs &a, int tid) { pass_stage_copy<float, NS>(qs, a, tid); }
    static __device__ __forceinline__ Acc zero() { return (f32x2){0.0f, 0.0f}; }
    static __device__ __forceinline__ float lane_sum(Acc v) { return v[0] + v[1]; }
    static __device__ __forceinline__ void batch(Acc (&acc)[R][NQ], const float *qv, int D, uint32_t voff, const float *const (&row)[R], const float *const (&qg)[NG > 0 ? NG : 1])
    {
        constexpr int SS = U * NS;
        f32x4 w[SS];        // staged query vectors in the order they are used: (u, q < NS), read two ahead
        w[0] = *reinterpret_cast<const f32x4 *>(qv);
        w[1] = *reinterpret_cast<const f32x4 *>(qv + D);
        static_for<U>([&](auto uc) CHIP_INLINE_LAMBDA {
            constexpr int u = uc;
            slot_wait<L - R>();                      // the four row slots of this KiB are the oldest loads of the stream
            static_for<NS>([&](auto qc) CHIP_INLINE_LAMBDA {
                constexpr int q = qc, i = u * NS + q;
                if constexpr (i + 2 < SS) w[i + 2] = *reinterpret_cast<const f32x4 *>(qv + ((i + 2) % NS) * D + ((i + 2) / NS) * 256);
                const f32x2 wl = __builtin_shufflevector(w[i], w[i], 0, 1), wh = __builtin_shufflevector(w[i], w[i], 2, 3);
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA { prefilter_fma<pass_row_slot(u, rr)>(acc[rr][q], wl); });
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA { prefilter_fma<pass_row_slot(u, rr) + 2>(acc[rr][q], wh); });
                __builtin_amdgcn_sched_barrier(0);
            });
            static_for<NG>([&](auto gc) CHIP_INLINE_LAMBDA {
                constexpr int g = gc, QR = pass_query_slot(NG, u, g);
                slot_wait<L - R - 1 - g>();
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA { prefilter_fma_slot<pass_row_slot(u, rr), QR>(acc[rr][NS + g]); });
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA { prefilter_fma_slot<pass_row_slot(u, rr) + 2, QR + 2>(acc[rr][NS + g]); });
            });
            slots_issue_kib<u, NG>(voff, row, qg);
        });
    }
};

template <int NG>
__global__ __launch_bounds__(kMultiBlock) __attribute__((amdgpu_num_vgpr(pass_vgpr_base(kPrefilterMaxNG) / 2))) void db_scan_prefilter(PassArgs a)
{
    static_assert(NG <= kPrefilterMaxNG, "the compiler's share is sized for kPrefilterMaxNG query slots per KiB");
    shared_pass<PassF32<NG>>(a);
}

// ------------------------------------------------------------------------------------------------ K1, five ticks per pass, queries staged as fp16
// db_scan_halfq: the prefilter pass for FIVE queued ticks (15 queries).  What keeps a fifth tick out of db_scan_prefilter is LDS bytes per
// query, not arithmetic: here every query is staged as fp16, [15][D] halves (120 KiB at D = 4096), and none is read in place.  The
// certificate is the one of the four-tick pass with a larger error bound (E_h): the lists only propose, tick_rescore decides.
//   * staging: every workgroup reads the 15 fp32 query rows once and stores fl16(2^e q), round to nearest even.  2^e (PassArgs::q_up) is
//     chosen by the host from the row-norm bound N so that 2^e N <= 2^15: no element of a published row overflows fp16, small norms keep
//     their bits above the fp16 subnormals;
//   * batch step: per KiB the four row slots are waited for once; per query one ds_read_b64 (four halves, read two vectors ahead), four
//     conversions to fp32 (exact) and eight v_pk_fma_f32 on the slot registers -- the accumulator pairs and their element order are
//     PassF32's; then the KiB's slots are issued again;
//   * scores and thresholds stay 2^e times too large inside the pass; pass_offer scales what enters a list by 2^-e in fp64 (exact).
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
struct PassF32H {
    typedef float Elem;
    typedef _Float16 Staged;
    typedef float Score;
    typedef f32x2 Acc;
    static constexpr bool kScaled = true;
    static constexpr int NQ = 3 * kHalfqTicks, NG = 0, NS = NQ, R = kMultiR, U = kMultiU, L = U * R, kVgprBase = pass_vgpr_base(0);
    static __device__ __forceinline__ void stage(_Float16 *qs, const PassArgs &a, int tid)
    {
        const int D = a.D;
        const float up = a.q_up;
        for (int e = tid * 4; e < D; e += blockDim.x * 4) {
            f32x4 w[NS];
#pragma unroll
            for (int q = 0; q < NS; q++) w[q] = *as_global(reinterpret_cast<const f32x4 *>(static_cast<const float *>(a.q[q]) + e));
#pragma unroll
            for (int q = 0; q < NS; q++) {
                f16x4 h;
#pragma unroll
                for (int c = 0; c < 4; c++) h[c] = (_Float16)(w[q][c] * up);   // the product is exact (a power of two), the conversion rounds to nearest even
                *reinterpret_cast<f16x4 *>(qs + q * D + e) = h;
            }
        }
    }
    static __device__ __forceinline__ Acc zero() { return (f32x2){0.0f, 0.0f}; }
    static __device__ __forceinline__ float lane_sum(Acc v) { return v[0] + v[1]; }
    static __device__ __forceinline__ void batch(Acc (&acc)[R][NQ], const _Float16 *qv, int D, uint32_t voff, const float *const (&row)[R], const float *const (&qg)[1])
    {
        constexpr int SS = U * NS;
        f16x4 w[SS];        // staged query vectors in the order they are used: (u, q), read two ahead
        w[0] = *reinterpret_cast<const f16x4 *>(qv);
        w[1] = *reinterpret_cast<const f16x4 *>(qv + D);
        static_for<U>([&](auto uc) CHIP_INLINE_LAMBDA {
            constexpr int u = uc;
            slot_wait<L - R>();                      // the four row slots of this KiB are the oldest loads of the stream
            static_for<NS>([&](auto qc) CHIP_INLINE_LAMBDA {
                constexpr int q = qc, i = u * NS + q;
                if constexpr (i + 2 < SS) w[i + 2] = *reinterpret_cast<const f16x4 *>(qv + ((i + 2) % NS) * D + ((i + 2) / NS) * 256);
                const f32x2 wl = {(float)w[i][0], (float)w[i][1]}, wh = {(float)w[i][2], (float)w[i][3]};
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA { prefilter_fma<pass_row_slot(u, rr)>(acc[rr][q], wl); });
                static_for<R>([&](auto rr) CHIP_INLINE_LAMBDA { prefilter_fma<pass_row_slot(u, rr) + 2>(acc[rr][q], wh); });
                __builtin_amdgcn_sched_barrier(0);
            });
            slots_issue_kib<u, 0>(voff, row, qg);
        });
    }
};

__global__ __launch_bounds__(kMultiBlock) __attribute__((amdgpu_num_vgpr(pass_vgpr_base(0) / 2))) void db_scan_halfq(PassArgs a)
{
    shared_pass<PassF32H>(a);
}

// ------------------------------------------------------------------------------------------------ exact rescoring of one prefiltered tick
// tick_rescore: ONE launch per pass, one workgroup per (tick, query), in front of the ticks' K2 launches.  (The pass fills every CU's register
// file, so whatever follows it on the ctx stream runs in the gap between two passes: a chain of one launch per tick did not fit there and
// stalled the pipeline.)  Per query, from the n_lists workgroup lists of db_scan_prefilter
// (C = all their entries):  G = the K-th largest fp32 score of C (-inf with fewer than K rows),  M = the largest K-th score of a list whose
// workgroup owned more than K rows of the prefix (-inf if there is none: nothing was dropped),  R = { r in C : score >= G - 2E }.  Certificate: M < G - 2E (or nothing dropped)
// and |R| <= kRescoreCap -- then the exact top-K is the top-K of R by exact score.  The rows of R are scored by rows_dot + butterfly_sum (the
// bits of every other scan kernel) and written as ONE sorted list per query, which topk_merge reads as a launch of one workgroup's lists.
__device__ __forceinline__ void block_best(double &bs, int64_t &bi, double *red_s, int64_t *red_i, int lane, int wave)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(bs, m, 64);
        const int64_t oi = __shfl_xor(bi, m, 64);
        if (key_gt(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    __syncthreads();   // (red_* of the previous round has been read by everybody)
    if (lane == 0) { red_s[wave] = bs; red_i[wave] = bi; }
    __syncthreads();
    bs = red_s[0]; bi = red_i[0];
#pragma unroll
    for (int w = 1; w < 8; w++)
        if (key_gt(red_s[w], red_i[w], bs, bi)) { bs = red_s[w]; bi = red_i[w]; }
}

__global__ __launch_bounds__(512) void tick_rescore(RescoreArgs a)
{
    constexpr int MAXH = 512 * CHIP_MAX_TOPK / 512;   // entries per thread: n_lists <= 512 lists of K <= CHIP_MAX_TOPK
    __shared__ double red_s[8];
    __shared__ int64_t red_i[8];
    __shared__ chip_topk_entry cand[kRescoreCap];
    __shared__ int n_cand;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tick = blockIdx.x / 3, q = blockIdx.x % 3;     // one workgroup per (tick of the pass, query of the tick)
    const int K = a.K, n = a.n_lists * K;
    const chip_topk_entry *in = a.in + (int64_t)tick * a.n_lists * 3 * K;
    const int64_t k = a.k[tick];
    if (tid == 0) n_cand = 0;
    double es[MAXH];
    int64_t ei[MAXH];
#pragma unroll
    for (int h = 0; h < MAXH; h++) {
        const int c = tid + 512 * h;
        es[h] = -INFINITY; ei[h] = -1;
        if (c < n) { const chip_topk_entry t = in[((int64_t)(c / K) * 3 + q) * K + (c % K)]; es[h] = t.score; ei[h] = t.idx; }
    }
    // M: the K-th entries of the lists whose workgroup owned more than K rows of the prefix (the others dropped nothing).  Workgroup b
    // owns the rows r with r mod tw in [b wpb, (b + 1) wpb), tw = n_lists wpb (db_scan_prefilter's row -> wave map).
    double ms = -INFINITY;
    int64_t mi = -1;
    const int64_t tw = (int64_t)a.n_lists * a.wpb;
#pragma unroll
    for (int h = 0; h < MAXH; h++) {
        const int c = tid + 512 * h;
        if (c % K != K - 1 || ei[h] < 0) continue;
        int64_t part = k % tw - (int64_t)(c / K) * a.wpb;
        part = part < 0 ? 0 : part > a.wpb ? a.wpb : part;
        if ((k / tw) * a.wpb + part > K && es[h] > ms) { ms = es[h]; mi = 0; }
    }
    block_best(ms, mi, red_s, red_i, lane, wave);
    // G: K rounds of "the best entry strictly below the previous one"
    double gs = INFINITY;
    int64_t gi = INT64_MAX;
    for (int j = 0; j < K; j++) {
        double bs = -INFINITY;
        int64_t bi = -1;
#pragma unroll
        for (int h = 0; h < MAXH; h++)
            if (key_gt(gs, gi, es[h], ei[h]) && key_gt(es[h], ei[h], bs, bi)) { bs = es[h]; bi = ei[h]; }
        block_best(bs, bi, red_s, red_i, lane, wave);
        gs = bs; gi = bi;
    }
    double thr = gs - 2.0 * a.E;
    thr -= fabs(thr) * 0x1p-51;   // at least one ulp below the rounded difference: R can only grow, the certificate can only fail
    const bool ok = mi < 0 || ms < thr;
#pragma unroll
    for (int h = 0; h < MAXH; h++)
        if (ei[h] >= 0 && es[h] >= thr) {
            const int at = atomicAdd(&n_cand, 1);
            if (at < kRescoreCap) { chip_topk_entry t; t.score = es[h]; t.idx = ei[h]; cand[at] = t; }
        }
    __syncthreads();
    const int nc = n_cand < kRescoreCap ? n_cand : kRescoreCap;
    // exact scores: one wave per candidate row
    const float *qrow = static_cast<const float *>(a.q[3 * tick + q]);
    for (int j = wave; j < nc; j += 8) {
        const int64_t r = cand[j].idx;
        const float *row[1] = {static_cast<const float *>(a.seg_table[r >> a.seg_shift]) + (r & a.seg_mask) * (int64_t)a.D};
        double acc[1][1];
        rows_dot<float, 1, 4, true, 1, 1>(row, qrow, a.D, lane, acc);
        const double s = butterfly_sum(acc[0][0]);
        if (lane == 0) cand[j].score = s;
    }
    __syncthreads();
    if (wave == 0) {
        static_assert(kRescoreCap <= 64, "one lane per candidate");
        chip_topk_entry *out = a.out + (int64_t)(3 * tick + q) * K;
        chip_topk_entry me;
        me.score = -INFINITY; me.idx = -1;
        if (lane < nc) me = cand[lane];
        int rank = 0;
        for (int j = 0; j < nc; j++) {
            const chip_topk_entry o = cand[j];
            rank += key_gt(o.score, o.idx, me.score, me.idx) ? 1 : 0;
        }
        if (lane < nc && rank < K) out[rank] = me;
        if (lane >= nc && lane < K) out[lane] = me;   // fewer candidates than K: the list ends in empty entries
        if (lane == 0) a.cert[tick][q] = ok && n_cand <= kRescoreCap ? 1u : 2u;
    }
}

// ------------------------------------------------------------------------------------------------ bulk ticks: exact records from a many-query group
// bulk_tick_finish: ONE launch per group of chip_loop_ticks_bulk (batch.hip), one workgroup of four waves per tick, behind the group's
// topk_merge_batch.  Query 3 t + i of the group is row l_t - 1 - i against rows [0, k_t); its sorted list of KL fp32 fmaf-chain scores is read
// in place.  Per query (wave i, lane = list slot):  G = the topk-th score (-inf where that slot is unused),  M = the KL-th score if that
// slot is used (else the GEMM dropped nothing),  thr = G - 2E lowered as tick_rescore lowers it,  R = the entries with score >= thr -- a
// prefix of the list, at most KL rows.  Certificate: nothing dropped, or M < thr.  The rows of R are scored one wave per row
// by rows_dot + butterfly_sum -- the bits of every other scan kernel -- with the query row read in place, ranked by key_gt, and the
// topk best written; thread 0 then writes the tick's record with tick_decision.  A workgroup reads its own tick's lists and rows only.
template <bool FULL>
__global__ __launch_bounds__(256) void bulk_tick_finish(BulkFinishArgs a)
{
    __shared__ chip_topk_entry cand[3][CHIP_MAX_TOPK];
    __shared__ chip_topk_entry tops[3];
    __shared__ int n_cand[3], cert[3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tick = blockIdx.x, KL = a.KL, K = a.K;
    if (wave < 3) {
        const int q = wave;
        chip_topk_entry e;
        e.score = -INFINITY; e.idx = -1;
        if (lane < KL) e = a.lists[((int64_t)3 * tick + q) * KL + lane];
        const double gs = readlane_f64(e.score, K - 1);                 // (an unused slot carries -inf)
        const double ms = readlane_f64(e.score, KL - 1);
        const bool dropped = readlane_i64(e.idx, KL - 1) >= 0;
        double thr = gs - 2.0 * a.E;
        thr -= fabs(thr) * 0x1p-51;   // as tick_rescore: R can only grow, the certificate can only fail
        const bool in_r = e.idx >= 0 && e.score >= thr;
        const unsigned long long mask = __ballot(in_r);
        if (in_r) cand[q][__popcll(mask & ((1ull << lane) - 1ull))] = e;
        if (lane == 0) { n_cand[q] = __popcll(mask); cert[q] = !dropped || ms < thr ? 1 : 0; }
    }
    __syncthreads();
    for (int j = wave; j < 3 * KL; j += 4) {   // exact scores: one wave per row of R
        const int q = j / KL, i = j - q * KL;
        if (i >= n_cand[q]) continue;
        const int64_t r = cand[q][i].idx, qr = a.rows[(int64_t)3 * tick + q];
        const float *row[1] = {static_cast<const float *>(a.seg_table[r >> a.seg_shift]) + (r & a.seg_mask) * (int64_t)a.D};
        const float *qrow = static_cast<const float *>(a.seg_table[qr >> a.seg_shift]) + (qr & a.seg_mask) * (int64_t)a.D;
        double acc[1][1];
        rows_dot<float, 1, 4, FULL, 1, 1>(row, qrow, a.D, lane, acc);
        const double s = butterfly_sum(acc[0][0]);
        if (lane == 0) cand[q][i].score = s;
    }
    __syncthreads();
    if (wave < 3) {
        const int q = wave, nc = n_cand[q];
        chip_topk_entry *out = a.out + ((int64_t)3 * tick + q) * K;
        chip_topk_entry me;
        me.score = -INFINITY; me.idx = -1;
        if (lane < nc) me = cand[q][lane];
        int rank = 0;
        for (int j = 0; j < nc; j++) {
            const chip_topk_entry o = cand[q][j];
            rank += key_gt(o.score, o.idx, me.score, me.idx) ? 1 : 0;
        }
        if (lane < nc && rank < K) out[rank] = me;
        if (lane >= nc && lane < K) out[lane] = me;   // fewer rows than topk: the list ends in empty entries
        if (lane < nc && rank == 0) tops[q] = me;
        if (lane == 0 && nc == 0) tops[q] = me;
    }
    __syncthreads();
    if (tid == 0) {
        a.rec[tick] = tick_decision<3>(tops, false, a.rows[(int64_t)3 * tick] + 1, a.locality, a.thresh);
        a.words[2 * tick] = cert[0] && cert[1] && cert[2] ? 1u : 2u;
        a.words[2 * tick + 1] = (uint32_t)(n_cand[0] + n_cand[1] + n_cand[2]);
    }
}

int launch_bulk_finish(Ctx *c, hipStream_t s, const BulkFinishArgs &a, int n_ticks)
{
    if (n_ticks < 1 || a.KL < 1 || a.KL > CHIP_MAX_TOPK || a.K < 1 || a.K > a.KL || a.D % 4 != 0) return CHIP_ERR_UNSUPPORTED;
    if (a.D % 1024 == 0) hipLaunchKernelGGL(bulk_tick_finish<true>, dim3(n_ticks), dim3(256), 0, s, a);    // whole 4 KiB batches
    else hipLaunchKernelGGL(bulk_tick_finish<false>, dim3(n_ticks), dim3(256), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ K1, wide double rows
// Double rows whose NQ query descriptors do not fit the 160 KiB of LDS (the reference's default D = 8192, src/Cerebro.cpp:1021, as a
// MatrixXd of genuine float64 values: 3 x 8192 x 8 B = 192 KiB).  The first NQ - NG queries are staged as usual; the last NG are read
// from global memory next to the row -- every wave of the launch reads the same D x 8 bytes, so they come out of the L2 -- with the
// same per-lane element order as rows_dot (lane L: elements j*128 + 2L + c, j ascending, fma; then the xor butterfly), hence the
// same bits as the staged form and as the oracle (orc_dot_tree_f64).  A rare configuration: plain compiler-scheduled loads.
template <int NQ, int NG, bool FULL>
__global__ __launch_bounds__(1024) void db_scan_topk_wide(ScanArgs a)
{
    static_assert(NG >= 1 && NG < NQ, "at least one query staged, at least one read in place");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *qs = reinterpret_cast<double *>(smem);  // [NQ - NG][D]
    constexpr int NL = NQ - NG, U = 4, CH = 128;
    const int D = a.D, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpb = blockDim.x >> 6;
    stage_queries<double, NL>(a, qs, tid, blockDim.x);
    __syncthreads();
    const double *qg[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) qg[g] = static_cast<const double *>(a.q[NL + g]);

    double my_s[NQ], thr_s[NQ];
    int64_t my_i[NQ], thr_i[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) { my_s[q] = -INFINITY; my_i[q] = -1; thr_s[q] = -INFINITY; thr_i[q] = -1; }
    const int e0 = lane * 2;
    const int64_t tw = (int64_t)gridDim.x * wpb;
    for (int64_t r = (int64_t)blockIdx.x * wpb + wave; r < a.n_rows; r += tw) {
        const double *row = row_base<double>(a, r);
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[q] = 0.0;
        for (int base = 0; base < D; base += CH * U) {
            f64x2 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = base + u * CH + e0;
                if (FULL || e < D) v[u] = __builtin_nontemporal_load(as_global(reinterpret_cast<const f64x2 *>(row + e)));
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = base + u * CH + e0;
                if (FULL || e < D) {
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        const f64x2 w = q < NL ? *reinterpret_cast<const f64x2 *>(qs + q * D + e)
                                               : *as_global(reinterpret_cast<const f64x2 *>(qg[q < NL ? 0 : q - NL] + e));
                        acc[q] = __builtin_fma(w[0], v[u][0], acc[q]);
                        acc[q] = __builtin_fma(w[1], v[u][1], acc[q]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[q] = butterfly_sum(acc[q]);
        const int64_t gi = r * a.idx_mul + a.idx_add;
#pragma unroll
        for (int q = 0; q < NQ; q++) wave_topk_offer(acc[q], gi, K, lane, my_s[q], my_i[q], thr_s[q], thr_i[q]);
    }
    block_merge_store<NQ>(smem, my_s, my_i, K, lane, wave, wpb, [&](int q) { return a.partial + ((int64_t)blockIdx.x * NQ + q) * K; });
}

// ------------------------------------------------------------------------------------------------ K1, row-batched form
// The same scan with R rows per wave in flight at once and the loads issued as ONE continuous stream (round 3): a wave walks
// the (pass, 4 KiB batch, load slot u) sequence of its rows and re-issues slot u for the NEXT batch as soon as the fmas that
// read slot u of the current batch have been issued, so R x 4 KiB per wave stay in flight for the whole scan instead of
// draining to zero at every batch (db_scan_topk above).  Three things follow for SHORT prefixes (BASELINE config 2: 10 003 rows
// over 4096 waves = 2.4 rows per wave, which the one-row kernel walks as 12 dependent 4 KiB batches per wave):
//   * R = 3 turns a wave's whole share into one pass of 4 batches with 12 KiB in flight;
//   * the queries are staged by LDS-DMA (global_load_lds_dwordx4, no staging VGPRs), issued BEFORE the first row loads and
//     waited for with a counted vmcnt, so the first 12 KiB of DB rows are already on their way while the queries land;
//   * each query element is converted to fp64 once per R rows (R = 3: 20 instead of 28 VALU instructions per KiB of DB).
// Arithmetic and order per (row, query) are those of rows_dot: lane L accumulates elements j*CH + N*L + c, j ascending, into
// one fp64 accumulator by fma, then the xor butterfly -- bit-identical scores, same (score desc, index desc) lists.
// Loads use the SGPR-base form (row base in an SGPR pair, one shared 32-bit lane offset), immediate offsets u * 1 KiB.
// Requires whole 4 KiB batches (D * sizeof(T) % 4096 == 0) and queries that are 16-B aligned rows of D elements.
__device__ __forceinline__ uint32_t lds_byte_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
// 16 bytes per lane, global -> LDS at (wave-uniform LDS base in M0) + lane * 16; M0 is saved and restored around the load
__device__ __forceinline__ void glds16_q(const void *gsrc_lane, uint32_t lds_base_wave_uniform)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc_lane), "s"(lds_base_wave_uniform)
                 : "memory");
}

// Block merge over the LDS lists: wpb sorted lists of K per query -> one sorted list of K per query in a.partial[blockIdx.x].
// device-coherent 16-byte entry store / load (agent-scope relaxed atomics: write-through `sc1` stores and loads, no cache-wide fence)
__device__ __forceinline__ void store_entry_agent(chip_topk_entry *p, double s, int64_t i)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(&p->score), (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(&p->idx), (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ chip_topk_entry load_entry_agent(const chip_topk_entry *p)
{
    chip_topk_entry e;
    e.score = __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(&p->score), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    e.idx = (int64_t)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(&p->idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return e;
}

template <int NQ>
__device__ __forceinline__ void block_merge_lists(const ScanArgs &a, const chip_topk_entry *lists, int K, int lane, int wave, int wpb, bool coherent = false)
{
    __syncthreads();
    for (int q = wave; q < NQ; q += wpb) {
        const int ncand = wpb * K;  // <= 16 waves * 16 = 256 -> at most 4 per lane
        double cs[4];
        int64_t ci[4];
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const int c = lane + 64 * h;
            if (c < ncand) {
                const chip_topk_entry t = lists[((c / K) * NQ + q) * CHIP_MAX_TOPK + (c % K)];
                cs[h] = t.score;
                ci[h] = t.idx;
            } else { cs[h] = -INFINITY; ci[h] = -1; }
        }
        chip_topk_entry *outp = a.partial + ((int64_t)blockIdx.x * NQ + q) * K;
        for (int j = 0; j < K; j++) {
            double bs = cs[0];
            int64_t bi = ci[0];
#pragma unroll
            for (int h = 1; h < 4; h++)
                if (key_gt(cs[h], ci[h], bs, bi)) { bs = cs[h]; bi = ci[h]; }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double os = __shfl_xor(bs, m, 64);
                const int64_t oi = __shfl_xor(bi, m, 64);
                if (key_gt(os, oi, bs, bi)) { bs = os; bi = oi; }
            }
#pragma unroll
            for (int h = 0; h < 4; h++)
                if (ci[h] == bi && cs[h] == bs) { cs[h] = -INFINITY; ci[h] = -1; }
            if (lane == 0) {
                if (coherent) store_entry_agent(outp + j, bs, bi);
                else { chip_topk_entry t; t.score = bs; t.idx = bi; outp[j] = t; }
            }
        }
    }
}

// Load targets of db_scan_topk_rows.  The loads are issued from inline asm and consumed behind counted s_waitcnt -- a register
// that the compiler believed "defined" at the load statement could be copied or spilled by it BEFORE the wait (it happened: the
// first version of this kernel, with "=v" outputs, got v_mov copies of in-flight registers at a control-flow merge).  So the
// targets are PHYSICAL registers the compiler does not own: the kernel is compiled with amdgpu_num_vgpr(kRowsVgprBase / 2) -- on
// gfx950's unified VGPR/AGPR file hipcc (ROCm 7.2) takes that attribute as HALF the ArchVGPR budget (measured: 24 -> 48, 32 -> 64,
// 40 -> 80 registers, spilling beyond) -- which leaves v[kRowsVgprBase ..] to the asm statements; a load names its target
// literally, and the statement that waits for it also moves the data (converted to fp64 for float rows) into compiler-owned
// outputs -- wait and first read are one asm block.  tests/test_codeobj_registers.py disassembles the built library and checks
// the partition: nothing but these loads writes v[80..127], nothing but the take statements reads them.
constexpr int kRowsVgprBase = 80;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "db_scan_topk_rows names physical VGPRs and uses global_load_lds_dwordx4: gfx950 (MI355X) only -- build with --offload-arch=gfx950"
#endif
#define CHIP_ROWS_CLOBBERS                                                                                                      \
    "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97",   \
    "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", \
    "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127"

// slot (u, rr) of an R-row batch -> v[base : base + 3]
template <int R> __host__ __device__ constexpr int rows_slot_reg(int u, int rr) { return kRowsVgprBase + 4 * (u * R + rr); }

template <bool NTL, int REG, int OFF>
__device__ __forceinline__ void rows_issue(uint32_t voff, const void *row_uniform)
{
    if constexpr (NTL)   // non-temporal: a stream that is read once (prefixes beyond the Infinity Cache)
        asm volatile("global_load_dwordx4 v[%2:%3], %0, %1 offset:%4 nt" ::"v"(voff), "s"(row_uniform), "n"(REG), "n"(REG + 3), "n"(OFF) : "memory");
    else                 // temporal: a prefix that fits the 256 MiB Infinity Cache is re-read by every tick
        asm volatile("global_load_dwordx4 v[%2:%3], %0, %1 offset:%4" ::"v"(voff), "s"(row_uniform), "n"(REG), "n"(REG + 3), "n"(OFF) : "memory");
}

// wait until at most CNT vector-memory operations are outstanding, then hand one 8-byte HALF (H = 0, 1) of the slot's 16 bytes
// to the compiler as fp64: two elements of a float row, one of a double row (halves keep the compiler-side live set small)
template <int REG, int CNT, int H>
__device__ __forceinline__ void rows_take(double (&d)[2], float)
{
    asm volatile("s_waitcnt vmcnt(%2)\n\tv_cvt_f64_f32 %0, v[%3]\n\tv_cvt_f64_f32 %1, v[%4]"
                 : "=&v"(d[0]), "=&v"(d[1])
                 : "n"(CNT), "n"(REG + 2 * H), "n"(REG + 2 * H + 1)
                 : "memory");
}
template <int REG, int CNT, int H>
__device__ __forceinline__ void rows_take(double (&d)[2], double)
{
    asm volatile("s_waitcnt vmcnt(%1)\n\tv_mov_b64 %0, v[%2:%3]" : "=&v"(d[0]) : "n"(CNT), "n"(REG + 2 * H), "n"(REG + 2 * H + 1) : "memory");
    d[1] = 0.0;
}

// Fused tick: the decision of Cerebro.cpp:1035-1056 needs the BEST entry per query only (chip_tick_result carries argmax / maxv, no
// lists), and the best of the whole prefix is the best of the per-workgroup bests under the same total order (score desc, index
// desc).  So a tick runs the scan with K = 1 and the last workgroup to arrive (device-scope ticket) reduces the <= 512 per-workgroup
// entries -- one per thread, wave butterfly, eight waves through LDS -- applies the accept rule and stores the 64-byte record straight
// into the pinned host slot: no K2 launch, no launch gap, no second kernel's ramp (a 10k-row tick spent ~15 us of its stream's time in
// the one-workgroup merge and ~6 us in front of it, profiles/r03_tick_timeline_10k.md).  Hand-off: write-through stores + completion
// wait + device-scope ticket on the writers' side, L2-bypassing loads on the last workgroup's side (no cache-wide fences).
// What one pass of the row-batched scan is asked to do -- the fields of ScanArgs that differ from pass to pass.  A launch takes them from
// its kernel arguments; the resident instance from the command it was sent (they then live in SGPRs: no arrays, nothing indexed).
struct RowsPass {
    int64_t n_rows;
    const void *q0, *q1, *q2, *q3;
    int32_t dyn_claim;
    chip_tick_result *fused_result;
    unsigned long long *fused_seq;
    unsigned long long fused_seq_val;
    int64_t tick_l;
    int32_t locality;
    double thresh;
};
__device__ __forceinline__ RowsPass rows_pass_of(const ScanArgs &a)
{
    RowsPass t;
    t.n_rows = a.n_rows;
    t.q0 = a.q[0]; t.q1 = a.q[1]; t.q2 = a.q[2]; t.q3 = a.q[3];
    t.dyn_claim = a.dyn_claim;
    t.fused_result = a.fused_result;
    t.fused_seq = a.fused_seq;
    t.fused_seq_val = a.fused_seq_val;
    t.tick_l = a.tick_l;
    t.locality = a.locality;
    t.thresh = a.thresh;
    return t;
}

template <int NQ, bool TOGETHER, bool XSTAMP>
__device__ __forceinline__ void fused_tick_finish(const ScanArgs &a, const RowsPass &t, char *smem, int K, int tid, int lane, int wave, int wpb)
{
    int *last = reinterpret_cast<int *>(smem);                                  // LDS is free again: the lists have been consumed
    chip_topk_entry *wbest = reinterpret_cast<chip_topk_entry *>(smem + 64);    // [wpb][NQ]
    // This workgroup's entries went out as write-through (agent-scope) stores; once they have completed (vmcnt(0)) they are visible
    // device-wide, and the ticket may be taken.  No __threadfence(): an agent-scope release fence writes back this XCD's L2 -- with
    // 256-512 workgroups doing it the tick took 120 us instead of 25 (measured; it is also why round 2's fused merge lost).
    //   Writers (every workgroup): what stands in for the release is an ISA property of gfx942 / gfx950, not the HIP memory model --
    //   an sc1 (agent-scope) store is written THROUGH its XCD's L2 to the fabric, and its vmcnt slot is only returned when the
    //   write has been acknowledged there; "s_waitcnt vmcnt(0)" + the workgroup barrier therefore order this workgroup's entries
    //   before its ticket increment for every agent-scope observer.  The code object is gfx950-only (chip_create refuses anything
    //   else), and tests/test_scan_gpu.py::test_fused_tick_handoff_stress compares >= 200k fused ticks with the two-launch path.
    //   Reader (ONE workgroup): a real agent-scope ACQUIRE after the ticket is won -- it invalidates this XCD's non-coherent L2
    //   lines and the CU's vector L1 (buffer_inv sc1), so no entry of the launch that used this list buffer 64 ticks ago can be
    //   served from a cache; one workgroup per tick pays it, which is free (the 120 us were 256-512 workgroups RELEASING).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *last = __hip_atomic_fetch_add(a.fused_ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!*last) return;
    unsigned long long *xstamp = nullptr;   // tuning only (the resident instance with CHIP_SCAN_STAMPS=1): pass-wide stamps behind the waves'
    if constexpr (XSTAMP) xstamp = a.stamps ? a.stamps + (size_t)gridDim.x * wpb * 4 : nullptr;
    if (xstamp && tid == 0) xstamp[5] = (unsigned long long)wall_clock64();
    // (The resident instance leaves the fence out: everything this workgroup reads from memory from here on is read by agent-scope loads,
    //  which are coherent at that scope by themselves -- 0.84 us of the pass, measured; tests/test_resident_gpu.py compares every record
    //  of tens of thousands of consecutive, different commands.  The launched kernels keep it: belt and braces.)
    if constexpr (!XSTAMP) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (xstamp && tid == 0) xstamp[2] = (unsigned long long)wall_clock64();
    // One entry per workgroup of the launch and query; grid-stride, so a block smaller than the grid (CHIP_SCAN_BLOCK=256) drops
    // nothing.  TOGETHER (the R = 1 kernels, which have the registers for it): the NQ loads of a workgroup's entries are issued
    // before the first compare -- one round trip to memory instead of NQ; the others reduce one query at a time.
    auto reduce_store = [&](double s, int64_t i, int q) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double os = __shfl_xor(s, m, 64);
            const int64_t oi = __shfl_xor(i, m, 64);
            if (key_gt(os, oi, s, i)) { s = os; i = oi; }
        }
        if (lane == 0) { chip_topk_entry e; e.score = s; e.idx = i; wbest[wave * NQ + q] = e; }
    };
    if constexpr (TOGETHER) {
        double bs[NQ];
        int64_t bi[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) { bs[q] = -INFINITY; bi[q] = -1; }
        for (int wg = tid; wg < (int)gridDim.x; wg += (int)blockDim.x) {
            chip_topk_entry e[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++) e[q] = load_entry_agent(a.partial + ((int64_t)wg * NQ + q) * K);   // bypasses this XCD's L2
#pragma unroll
            for (int q = 0; q < NQ; q++)
                if (key_gt(e[q].score, e[q].idx, bs[q], bi[q])) { bs[q] = e[q].score; bi[q] = e[q].idx; }
        }
#pragma unroll
        for (int q = 0; q < NQ; q++) reduce_store(bs[q], bi[q], q);
    } else {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            double bs = -INFINITY;
            int64_t bi = -1;
            for (int wg = tid; wg < (int)gridDim.x; wg += (int)blockDim.x) {
                const chip_topk_entry e = load_entry_agent(a.partial + ((int64_t)wg * NQ + q) * K);   // bypasses this XCD's L2
                if (key_gt(e.score, e.idx, bs, bi)) { bs = e.score; bi = e.idx; }
            }
            reduce_store(bs, bi, q);
        }
    }
    if (xstamp && tid == 0) xstamp[6] = (unsigned long long)wall_clock64();
    __syncthreads();
    if (wave != 0) return;
    if (xstamp && tid == 0) xstamp[7] = (unsigned long long)wall_clock64();
    // the waves' bests -> the launch's best per query.  TOGETHER: lane 16 q + w takes wave w's entry of query q and a four-step
    // butterfly inside each group of 16 lanes finishes it (a max under a total order: the same entry whatever the order); the others
    // keep the serial loop of one lane (1.8 us of a 10k-row tick, measured -- but no extra registers).
    double maxv[3] = {-INFINITY, -INFINITY, -INFINITY};
    int64_t argmax[3] = {-1, -1, -1};
    if constexpr (TOGETHER) {
        const int q = lane >> 4, w = lane & 15;
        double sc = -INFINITY;
        int64_t ix = -1;
        if (q < NQ && w < wpb) { const chip_topk_entry e = wbest[w * NQ + q]; sc = e.score; ix = e.idx; }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const double os = __shfl_xor(sc, m, 64);
            const int64_t oi = __shfl_xor(ix, m, 64);
            if (key_gt(os, oi, sc, ix)) { sc = os; ix = oi; }
        }
#pragma unroll
        for (int qq = 0; qq < 3; qq++)
            if (qq < NQ) { maxv[qq] = readlane_f64(sc, 16 * qq); argmax[qq] = readlane_i64(ix, 16 * qq); }
    } else {
        for (int q = 0; q < 3; q++)
            if (q < NQ)
                for (int w = 0; w < wpb; w++) {
                    const chip_topk_entry e = wbest[w * NQ + q];
                    if (key_gt(e.score, e.idx, maxv[q], argmax[q])) { maxv[q] = e.score; argmax[q] = e.idx; }
                }
    }
    if (lane == 0) {
        chip_tick_result res;
        res.status = CHIP_TICK_SCANNED;
        res.found = 0;
        res.idx_curr = -1;
        res.idx_prev = -1;
        res.score = 0.0;
        for (int q = 0; q < 3; q++) { res.argmax[q] = argmax[q]; res.maxv[q] = maxv[q]; }
        if (NQ >= 3 && res.argmax[0] >= 0 && res.argmax[1] >= 0 && res.argmax[2] >= 0) {
            // Cerebro.cpp:1056  abs(u_argmax-um_argmax) < LOCALITY && abs(u_argmax-umm_argmax) < LOCALITY && u_max > THRESH
            int64_t d1 = res.argmax[0] - res.argmax[1];
            int64_t d2 = res.argmax[0] - res.argmax[2];
            if (d1 < 0) d1 = -d1;
            if (d2 < 0) d2 = -d2;
            if (d1 < t.locality && d2 < t.locality && res.maxv[0] > t.thresh) {
                res.found = 1;
                res.idx_curr = t.tick_l - 1;  // Cerebro.cpp:1080
                res.idx_prev = res.argmax[0];
                res.score = res.maxv[0];
            }
        }
        *t.fused_result = res;
        // ready for the pass that reuses this list buffer: a launch is ordered behind this one by its event; a command to the resident
        // instance arrives with no kernel boundary in between, so the reset is written THROUGH like the entries (agent-scope store)
        __hip_atomic_store(a.fused_ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (xstamp) xstamp[3] = (unsigned long long)wall_clock64();
        // completion word of the tick's slot (pinned host memory), system-scope RELEASE: a host polling it (acquire) sees the record above.
        // (The release is needed as it stands: the record's stores to host memory are held in this XCD's L2 until it is written back --
        //  with a completed-stores wait and a relaxed store of the word instead, the host read the PREVIOUS tick's record, every time.)
        if (t.fused_seq) __hip_atomic_store(t.fused_seq, t.fused_seq_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (xstamp) xstamp[4] = (unsigned long long)wall_clock64();
    }
}

// -DCHIP_NO_ROWS_FORM leaves the row-batched kernel out of the build: it rests on how THIS hipcc maps amdgpu_num_vgpr to an ArchVGPR
// budget (above), which `make verify` checks on the built code object -- a toolchain that allocates differently gets a library without
// the rows form (every scan takes the one-row kernel, same bits, short prefixes ~10-25 % slower) instead of no library at all;
// chip_get_info().scan_forms says which build this is.
#ifndef CHIP_NO_ROWS_FORM
// The body of the row-batched scan: one pass of the hot path over a prefix for the workgroup that runs it.  Two kernels inline it:
// db_scan_topk_rows (one launch per scan) and db_scan_resident (below: a kernel that stays on the chip and runs it once per command).
template <typename T, int NQ, int R, bool NTL, bool RESIDENT = false>
__device__ __forceinline__ void scan_rows_body(const ScanArgs &a, const RowsPass &t, char *smem)
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N, CH = 64 * N, U = 4;
    static_assert(kRowsVgprBase + 16 * R <= 128, "load targets beyond the 128 VGPRs of a 16-waves-per-CU kernel");
    const T *qs = reinterpret_cast<const T *>(smem);  // [NQ][D]
    const int D = a.D;
    const int K = a.K;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpb = blockDim.x >> 6;
    const int64_t tw = (int64_t)gridDim.x * wpb;
    const int64_t g = (int64_t)blockIdx.x * wpb + wave;           // this wave's first row (same row -> wave map as db_scan_topk)
    const int nb = D / (CH * U);                                   // 4 KiB batches per row
    const int64_t rbase = g, rstep = tw, rlim = t.n_rows;        // this wave's rows: rbase + i * rstep < rlim (the same row -> wave map as db_scan_topk)
    const int npass = rbase < rlim ? (int)((rlim - 1 - rbase) / (R * rstep)) + 1 : 0;
    const int total = npass * nb;                                  // batches this wave consumes (wave-uniform)

    unsigned long long *stamp = a.stamps ? a.stamps + (size_t)g * 4 : nullptr;   // tuning only
    if (stamp && lane == 0) stamp[0] = wall_clock64();
    // ---- queries -> LDS by LDS-DMA, 1 KiB per wave-instruction, chunks dealt round robin to the waves ----
    {
        const int cpq = (int)((size_t)D * sizeof(T) / 1024);
        const uint32_t lds0 = lds_byte_addr(smem);
        // the query bases as opaque SGPR values, SELECTED below, not indexed: the resident instance holds the pass in registers, and
        // a select between loads of neighbouring fields would be turned back into an indexed load of a stack copy
        uint64_t qb0 = (uint64_t)(uintptr_t)t.q0, qb1 = (uint64_t)(uintptr_t)t.q1, qb2 = (uint64_t)(uintptr_t)t.q2, qb3 = (uint64_t)(uintptr_t)t.q3;
        asm volatile("" : "+s"(qb0), "+s"(qb1), "+s"(qb2), "+s"(qb3));
        for (int i = wave; i < NQ * cpq; i += wpb) {
            const int q = i / cpq, ch = i - q * cpq;
            uint64_t qp = qb0;
            if (NQ > 1 && q == 1) qp = qb1;
            if (NQ > 2 && q == 2) qp = qb2;
            if (NQ > 3 && q == 3) qp = qb3;
            glds16_q(reinterpret_cast<const char *>((uintptr_t)qp) + (size_t)ch * 1024 + lane * 16, lds0 + (uint32_t)i * 1024u);
        }
    }

    const T *row[R];                                               // bases of the rows the NEXT issue reads (wave-uniform, SGPRs)
    const uint32_t lane_off = (uint32_t)(lane * 16);
    auto set_rows = [&](int pass) {
        const int64_t r0 = rbase + (int64_t)pass * R * rstep;
#pragma unroll
        for (int rr = 0; rr < R; rr++) {
            const int64_t r = r0 + rr * rstep;
            row[rr] = uniform_ptr(row_base_uniform<T>(a, r < rlim ? r : r0));   // a missing row re-reads the pass's first row; its result is dropped
        }
    };
    // load slot u of every row of the batch at byte offset byte_off of the rows
#define CHIP_ROWS_ISSUE_SLOT(u, byte_off)                                                                               \
    do {                                                                                                                \
        const uint32_t vo_ = (byte_off) + lane_off;                                                                     \
        rows_issue<NTL, rows_slot_reg<R>(u, 0), (u) * 1024>(vo_, row[0]);                                               \
        if constexpr (R > 1) rows_issue<NTL, rows_slot_reg<R>(u, R > 1 ? 1 : 0), (u) * 1024>(vo_, row[R > 1 ? 1 : 0]);  \
        if constexpr (R > 2) rows_issue<NTL, rows_slot_reg<R>(u, R > 2 ? 2 : 0), (u) * 1024>(vo_, row[R > 2 ? 2 : 0]);  \
    } while (0)

    if constexpr (R == 1) if (t.dyn_claim && tid == 0)   // the claim counter: units 0 .. wpb-1 are the waves' first rows (set before the barrier below)
        *reinterpret_cast<uint32_t *>(smem + (size_t)NQ * D * sizeof(T) + (size_t)wpb * NQ * CHIP_MAX_TOPK * sizeof(chip_topk_entry)) = (uint32_t)wpb;
    if (total > 0) {
        set_rows(0);
        CHIP_ROWS_ISSUE_SLOT(0, 0u); CHIP_ROWS_ISSUE_SLOT(1, 0u); CHIP_ROWS_ISSUE_SLOT(2, 0u); CHIP_ROWS_ISSUE_SLOT(3, 0u);
        // the LDS-DMA loads are older than the R*U row loads: "at most R*U outstanding" == the queries have landed
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(R * U) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }

    if (stamp && lane == 0) stamp[1] = wall_clock64();
    // running top-K lists: LDS behind the queries (this wave's NQ lists are touched by this wave only)
    chip_topk_entry *lists = reinterpret_cast<chip_topk_entry *>(smem + (size_t)NQ * D * sizeof(T));
    chip_topk_entry *mylists = lists + (size_t)wave * NQ * CHIP_MAX_TOPK;
    double thr_s[NQ];
    int64_t thr_i[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        thr_s[q] = -INFINITY; thr_i[q] = -1;
        if (lane < CHIP_MAX_TOPK) { chip_topk_entry t; t.score = -INFINITY; t.idx = -1; mylists[q * CHIP_MAX_TOPK + lane] = t; }
    }

    double acc[R][NQ];
#pragma unroll
    for (int rr = 0; rr < R; rr++)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[rr][q] = 0.0;

    // Slot u of the current batch: wait for its R loads (CNT0 + R-1-rr operations may stay outstanding behind row rr's), take the
    // data as fp64 and run the fmas of elements base + u*CH + N*lane + c against the staged queries.  Element-major, so one
    // query element is converted once and used by every row; per (row, query) the order is c ascending -- rows_dot's order.
#define CHIP_ROWS_FMA_HALF(u, h, CNT0)                                                                                   \
    do {                                                                                                                \
        double vd_[R][2];                                                                                               \
        rows_take<rows_slot_reg<R>(u, 0), (CNT0) + R - 1, h>(vd_[0], T());                                              \
        if constexpr (R > 1) rows_take<rows_slot_reg<R>(u, R > 1 ? 1 : 0), (CNT0) + R - 2, h>(vd_[R > 1 ? 1 : 0], T()); \
        if constexpr (R > 2) rows_take<rows_slot_reg<R>(u, R > 2 ? 2 : 0), (CNT0) + R - 3, h>(vd_[R > 2 ? 2 : 0], T()); \
        _Pragma("unroll") for (int c = 0; c < N / 2; c++) {                                                             \
            double wd_[NQ];                                                                                             \
            _Pragma("unroll") for (int q = 0; q < NQ; q++) wd_[q] = (double)w_[q][(h) * (N / 2) + c];                   \
            _Pragma("unroll") for (int rr = 0; rr < R; rr++)                                                            \
                _Pragma("unroll") for (int q = 0; q < NQ; q++) acc[rr][q] = __builtin_fma(wd_[q], vd_[rr][c], acc[rr][q]); \
        }                                                                                                               \
    } while (0)
#define CHIP_ROWS_FMA_SLOT(u, base, CNT0)                                                                               \
    do {                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        const int e_ = (base) + (u) * CH + lane * N;                                                                    \
        V w_[NQ];                                                                                                       \
        _Pragma("unroll") for (int q = 0; q < NQ; q++) w_[q] = *reinterpret_cast<const V *>(qs + q * D + e_);           \
        CHIP_ROWS_FMA_HALF(u, 0, CNT0);                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        CHIP_ROWS_FMA_HALF(u, 1, CNT0);                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)

    int pass = 0, b = 0;
    bool dyn = false;
    if constexpr (R == 1) dyn = t.dyn_claim != 0;
    if (dyn) {
      if constexpr (R == 1) {
        // ---- rows CLAIMED within the workgroup (round 5) -------------------------------------------------------------------------
        // Which wave scores which row is free: a row's dot products are one wave's fixed per-lane chain whoever that wave is, and the
        // lists merge under a total order.  The static map (wave g: rows g, g + tw, ...) makes every wave finish its LAST row when
        // its own speed says so -- and the speeds differ by the wave's age on its SIMD (stamps: 61 / 65 / 70 / 74 us at 29k rows).
        // Here the workgroup's rows -- unit u = row (u / wpb) * tw + blockIdx * wpb + u % wpb, the same set as before -- are handed
        // out by an LDS counter: a wave claims its next unit while it starts on the current one (the ds_add_rtn has a whole row,
        // ~8 us, to come back), so the waves of a workgroup run dry within one row of each other.
        // (Deeper streams, early re-issue at raised priority and rows claimed by workgroup pairs were tried and measured neutral or
        //  negative: profiles/r06_short_scan.md §2; the code was last carried by commit af4232e.)
        uint32_t *ctr = reinterpret_cast<uint32_t *>(smem + (size_t)NQ * D * sizeof(T) + (size_t)wpb * NQ * CHIP_MAX_TOPK * sizeof(chip_topk_entry));
        const int64_t wg0 = (int64_t)blockIdx.x * wpb;
        int n_units = 0;
        if (t.n_rows > wg0) {
            const int64_t span = t.n_rows - wg0, pf = span / tw, rem = span - pf * tw;
            n_units = (int)(pf * wpb + (rem < wpb ? rem : wpb));
        }
        auto unit_row = [&](int u) { return (int64_t)(u / wpb) * tw + wg0 + (u % wpb); };
        // (the counter was set to wpb by wave 0 before the staging barrier; unit `wave` is this wave's first, loaded above)
        int cur = wave;
        while (cur < n_units) {
            uint32_t nxt_v = 0;                                 // next unit, claimed by lane 0 alone: needed at this row's last batch
            if (lane == 0) nxt_v = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            int nxt = 0;
            bool more = false;
            for (b = 0; b < nb; b++) {
                const int base = b * (CH * U);
                bool next_batch = true;
                int nbase = base + CH * U;
                if (b + 1 == nb) {
                    nxt = __builtin_amdgcn_readfirstlane((int)nxt_v);
                    more = nxt < n_units;
                    next_batch = more;
                    nbase = 0;
                    if (more) row[0] = uniform_ptr(row_base_uniform<T>(a, unit_row(nxt)));
                }
                if (next_batch) {
                    const uint32_t noff = (uint32_t)nbase * (uint32_t)sizeof(T);
                    CHIP_ROWS_FMA_SLOT(0, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(0, noff);
                    CHIP_ROWS_FMA_SLOT(1, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(1, noff);
                    CHIP_ROWS_FMA_SLOT(2, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(2, noff);
                    CHIP_ROWS_FMA_SLOT(3, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(3, noff);
                } else {
                    CHIP_ROWS_FMA_SLOT(0, base, 3 * R);
                    CHIP_ROWS_FMA_SLOT(1, base, 2 * R);
                    CHIP_ROWS_FMA_SLOT(2, base, 1 * R);
                    CHIP_ROWS_FMA_SLOT(3, base, 0);
                }
            }
            const int64_t r = unit_row(cur);
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const double s = butterfly_sum(acc[0][q]);
                acc[0][q] = 0.0;
                wave_topk_offer_lds(s, r * a.idx_mul + a.idx_add, K, lane, mylists + q * CHIP_MAX_TOPK, thr_s[q], thr_i[q]);
            }
            cur = more ? nxt : n_units;
        }
      }
    } else
    for (int t = 0; t < total; t++) {
        const int base = b * (CH * U);
        if (t + 1 < total) {
            // steady state: slot (u, rr) has (U-1)*R + (R-1-rr) younger loads behind it whatever u is (the slots of the next
            // batch issued so far take the place of the slots of this batch already consumed)
            int nbase = base + CH * U;
            if (b + 1 == nb) { nbase = 0; set_rows(pass + 1); }
            const uint32_t noff = (uint32_t)nbase * (uint32_t)sizeof(T);
            CHIP_ROWS_FMA_SLOT(0, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(0, noff);
            CHIP_ROWS_FMA_SLOT(1, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(1, noff);
            CHIP_ROWS_FMA_SLOT(2, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(2, noff);
            CHIP_ROWS_FMA_SLOT(3, base, (U - 1) * R); CHIP_ROWS_ISSUE_SLOT(3, noff);
        } else {
            // the wave's last batch: nothing is re-issued, the loads behind slot (u, rr) are the rest of this batch
            CHIP_ROWS_FMA_SLOT(0, base, 3 * R);
            CHIP_ROWS_FMA_SLOT(1, base, 2 * R);
            CHIP_ROWS_FMA_SLOT(2, base, 1 * R);
            CHIP_ROWS_FMA_SLOT(3, base, 0);
        }
        if (++b == nb) {   // the rows of this pass are complete: butterfly, offer, next pass
            const int64_t r0 = rbase + (int64_t)pass * R * rstep;
#pragma unroll
            for (int rr = 0; rr < R; rr++) {
                const int64_t r = r0 + rr * rstep;
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const double s = butterfly_sum(acc[rr][q]);
                    acc[rr][q] = 0.0;
                    if (r < rlim) wave_topk_offer_lds(s, r * a.idx_mul + a.idx_add, K, lane, mylists + q * CHIP_MAX_TOPK, thr_s[q], thr_i[q]);
                }
            }
            b = 0;
            pass++;
        }
    }
#undef CHIP_ROWS_FMA_SLOT
#undef CHIP_ROWS_FMA_HALF
#undef CHIP_ROWS_ISSUE_SLOT
    if (stamp && lane == 0) stamp[2] = wall_clock64();
    block_merge_lists<NQ>(a, lists, K, lane, wave, wpb, t.fused_result != nullptr);
    if (t.fused_result != nullptr) fused_tick_finish<NQ, R == 1, RESIDENT>(a, t, smem, K, tid, lane, wave, wpb);
    if (stamp && lane == 0) stamp[3] = wall_clock64();
}

template <typename T, int NQ, int R, bool NTL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_num_vgpr(kRowsVgprBase / 2))) void db_scan_topk_rows(ScanArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    asm volatile("" ::: CHIP_ROWS_CLOBBERS);                       // makes the code object allocate the asm-owned registers
    scan_rows_body<T, NQ, R, NTL>(a, rows_pass_of(a), smem);
}

template <typename T, int NQ, int R, bool NTL>
static int launch_scan_rows(Ctx *c, hipStream_t s, const ScanArgs &a, int grid, size_t lds, int block)
{
    if (lds > 65536) CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_topk_rows<T, NQ, R, NTL>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((db_scan_topk_rows<T, NQ, R, NTL>), dim3(grid), dim3(block), lds, s, a);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// ---- the resident instance of the row-batched scan (opt-in, chip_internal.h ResidentCmd / ResidentArgs) ----
// One workgroup per CU stays on the chip and runs scan_rows_body<T, 3, 1, temporal> once per command -- the fused tick with nothing
// launched: no packet, no dispatch, no ramp of workgroup starts.  Wave 0 of workgroup 0 polls the host's 64-byte command line
// (system-scope loads over PCIe, 16 lanes = the whole line in one request; a line is accepted when head == tail) and copies it into
// every other workgroup's OWN line in device memory (one 64-byte write-through store each); wave 0 of the others polls its line
// (agent-scope loads: 256 pollers on 256 different lines, no hot spot).  The command reaches the waves of a workgroup through LDS.
// What the instance may read without a cache invalidation per command: published DB rows are immutable and a row is first read after
// it has been published, so no cache ever holds an older copy of one; the SEGMENT TABLE does change when the DB opens a new segment,
// so the host retires the instance before it touches the table (resident.hip resident_stop) and the next tick launches a new one.
// Every wait has a way out: workgroup 0 leaves (and sends the others home) after lease_ticks without a command, the others after four
// times that without a go word, so a host that died -- or a workgroup that never became resident -- cannot hold the chip.
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v); }
__device__ __forceinline__ unsigned long long uni_clock() { return uni64((uint64_t)wall_clock64()); }   // (the compiler takes the clock for a per-lane value)

template <typename T>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_num_vgpr(kRowsVgprBase / 2))) void db_scan_resident(ResidentArgs ra)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t cmd_s[16];
    asm volatile("" ::: CHIP_ROWS_CLOBBERS);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t done = ra.done;
    unsigned long long t_last = uni_clock();
    unsigned long long *xstamp = ra.base.stamps ? ra.base.stamps + (size_t)gridDim.x * (blockDim.x >> 6) * 4 : nullptr;   // tuning only
    for (;;) {
        if (wave == 0) {
            // lanes 16 k .. 16 k + 15 hold the 16 words of a line; a line is accepted when head == tail, is not the last one run, is not 0
            uint32_t v = 0, head = 0;
            bool leave = false;
            auto fresh = [&](uint32_t x) {
                head = (uint32_t)__builtin_amdgcn_readlane((int)x, 0);
                return head == (uint32_t)__builtin_amdgcn_readlane((int)x, 15) && head != done && head != 0u;
            };
            if (blockIdx.x == 0) {
                // The host's line, over PCIe: FOUR loads in flight, a quarter of a round trip apart (each is re-issued when it returns, so
                // the spacing holds) -- a command waits for the next load to leave, then for that load's round trip: 1.125 instead of 1.5.
                const uint32_t *line = ra.cmd_host + (lane & 15);
#define CHIP_POLL_HOST() __hip_atomic_load(line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
#define CHIP_POLL_STEP(P)                                                         \
    if (fresh(P)) { v = P; break; }                                               \
    if (uni_clock() - t_last > ra.lease_ticks) { leave = true; break; }           \
    P = CHIP_POLL_HOST();
                uint32_t p0 = CHIP_POLL_HOST();
                __builtin_amdgcn_s_sleep(10);
                uint32_t p1 = CHIP_POLL_HOST();
                __builtin_amdgcn_s_sleep(10);
                uint32_t p2 = CHIP_POLL_HOST();
                __builtin_amdgcn_s_sleep(10);
                uint32_t p3 = CHIP_POLL_HOST();
                for (;;) {
                    CHIP_POLL_STEP(p0)
                    CHIP_POLL_STEP(p1)
                    CHIP_POLL_STEP(p2)
                    CHIP_POLL_STEP(p3)
                }
#undef CHIP_POLL_STEP
#undef CHIP_POLL_HOST
            } else {
                const uint32_t *line = ra.cmd_dev + (size_t)blockIdx.x * 16 + (lane & 15);
                for (;;) {
                    v = __hip_atomic_load(line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (written by workgroup 0, or by the host through the BAR)
                    if (fresh(v)) break;
                    if (uni_clock() - t_last > 4 * ra.lease_ticks) { leave = true; break; }
                    __builtin_amdgcn_s_sleep(2);
                }
            }
            if (!leave) leave = __builtin_amdgcn_readlane((int)v, 3) < 0;   // n_rows < 0 (words 2, 3): the host retires the instance
            if (leave) {   // the line every workgroup acts on: n_rows = -1 under the leave mark
                v = (lane & 15) == 0 || (lane & 15) == 15 ? kResidentLeave : ((lane & 15) == 2 || (lane & 15) == 3 ? 0xffffffffu : 0u);
            }
            if (xstamp && blockIdx.x == 0 && lane == 0 && !leave) xstamp[0] = (unsigned long long)wall_clock64();
            if (lane < 16) cmd_s[lane] = v;
        }
        __syncthreads();
        if (blockIdx.x == 0 && (!ra.direct || cmd_s[0] == kResidentLeave)) {
            // the relay, by ALL waves of workgroup 0 (one wave alone issues a write-through store instruction every ~60 ns: 3.9 us for
            // 64 of them, measured): one 64-byte store per workgroup, four workgroups per instruction -- a line arrives whole
            const uint32_t w = cmd_s[lane & 15];
            for (int j = tid >> 4; j < (int)gridDim.x; j += (int)(blockDim.x >> 4))
                if (j > 0) __hip_atomic_store(ra.cmd_dev + (size_t)j * 16 + (lane & 15), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (xstamp && tid == 0 && cmd_s[0] != kResidentLeave) xstamp[1] = (unsigned long long)wall_clock64();
        }
        const ResidentCmd *cm = reinterpret_cast<const ResidentCmd *>(cmd_s);
        const int64_t n_rows = (int64_t)uni64((uint64_t)cm->n_rows);
        if (n_rows < 0) {
            if (blockIdx.x == 0 && tid == 0) __hip_atomic_store(ra.exit_host, ra.instance, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        const ScanArgs &a = ra.base;      // K = 1 and the fused-tick fields that do not change (ticket, list buffer) are set by the host
        RowsPass t;
        t.n_rows = n_rows;
        t.tick_l = (int64_t)uni64((uint64_t)cm->tick_l);
        t.locality = (int32_t)uni32((uint32_t)cm->locality);
        t.thresh = __longlong_as_double((long long)uni64((uint64_t)__double_as_longlong(cm->thresh)));
        t.fused_result = reinterpret_cast<chip_tick_result *>((uintptr_t)uni64(cm->result));
        t.fused_seq = reinterpret_cast<unsigned long long *>((uintptr_t)uni64(cm->seq_ptr));
        t.fused_seq_val = uni64(cm->seq_val);
        t.dyn_claim = (int32_t)uni32(cm->dyn_claim);
        const uint32_t number = uni32(cm->head);
        t.q0 = row_base_uniform<T>(a, t.tick_l - 1);   // v, vm, vmm (Cerebro.cpp:987-989)
        t.q1 = row_base_uniform<T>(a, t.tick_l - 2);
        t.q2 = row_base_uniform<T>(a, t.tick_l - 3);
        t.q3 = nullptr;
        scan_rows_body<T, 3, 1, false, true>(a, t, smem);
        done = number;
        t_last = uni_clock();
        __syncthreads();   // cmd_s and the lists are free again
    }
}

template <typename T>
static int launch_resident_T(Ctx *c, hipStream_t s, const ResidentArgs &ra, int grid, size_t lds, int block)
{
    if (lds > 65536) CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_resident<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((db_scan_resident<T>), dim3(grid), dim3(block), lds, s, ra);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}
#endif  // CHIP_NO_ROWS_FORM

template <typename T, int NQ, int U, bool FULL, int NT, int R>
static int launch_scan_k(Ctx *c, hipStream_t s, const ScanArgs &a, int grid, size_t lds, int block)
{
    if (lds > 65536) CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_topk<T, NQ, U, FULL, NT, R>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((db_scan_topk<T, NQ, U, FULL, NT, R>), dim3(grid), dim3(block), lds, s, a);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// Load path of K1.  Production (scan_variant 0): 4 x 16-B non-temporal loads per lane issued back to back from inline asm and
// consumed behind counted waits (rows_dot, NT == 6) -- with compiler-scheduled loads (variant 1, the round-1 kernel: U = 8
// builtin loads) hipcc sinks each load next to its use and a wave runs with 1-2 KiB in flight at 110 VGPRs; the asm form
// keeps 4 KiB per wave in flight at 66 VGPRs (short scans +5-7 %, 1M rows equal: profiles/r02_scan_load_path.txt).  Rows
// of whole 2 KiB batches use 2 loads per batch (D = 1536: +6 %); anything else (D * elem % 2048 != 0) takes the builtin path.
// The choice itself is scan_select() below; this launches the instantiation a record names -- one that does not exist is an error.
template <typename T, int NQ>
static int launch_scan_q(Ctx *c, hipStream_t s, const ScanArgs &a, const chip_debug_scan_launch &f)
{
    const int grid = f.grid, block = f.block;
    const size_t lds = (size_t)f.lds_bytes;
    if (f.family == CHIP_SCAN_FAMILY_ROWS) {   // scan_rows_form() said so: whole 4 KiB batches, R rows per wave in one continuous load stream
#ifndef CHIP_NO_ROWS_FORM
        const bool ntl = f.NTL != 0;
        if constexpr (NQ <= 3) {   // (four queries x R > 1 rows of accumulators do not fit the compiler's 80 registers: R = 1 only)
            if (f.R == 3) return ntl ? launch_scan_rows<T, NQ, 3, true>(c, s, a, grid, lds, block) : launch_scan_rows<T, NQ, 3, false>(c, s, a, grid, lds, block);
            if (f.R == 2) return ntl ? launch_scan_rows<T, NQ, 2, true>(c, s, a, grid, lds, block) : launch_scan_rows<T, NQ, 2, false>(c, s, a, grid, lds, block);
        }
        if (f.R == 1) return ntl ? launch_scan_rows<T, NQ, 1, true>(c, s, a, grid, lds, block) : launch_scan_rows<T, NQ, 1, false>(c, s, a, grid, lds, block);
#endif
        return CHIP_ERR_UNSUPPORTED;
    }
    if (f.family != CHIP_SCAN_FAMILY_ONE_ROW) return CHIP_ERR_UNSUPPORTED;
    const bool full = f.FULL != 0;
    if constexpr (sizeof(T) == 4) {
        if (f.U == 4 && f.NT == 8 && full) return launch_scan_k<T, NQ, 4, true, 8, 1>(c, s, a, grid, lds, block);   // scan_q64() said so (float rows only)
    }
    if (f.U == 4 && f.NT == 6 && full) return launch_scan_k<T, NQ, 4, true, 6, 1>(c, s, a, grid, lds, block);
    if (f.U == 2 && f.NT == 6 && full) return launch_scan_k<T, NQ, 2, true, 6, 1>(c, s, a, grid, lds, block);
    if (f.U == 8 && f.NT == 1) return full ? launch_scan_k<T, NQ, 8, true, 1, 1>(c, s, a, grid, lds, block) : launch_scan_k<T, NQ, 8, false, 1, 1>(c, s, a, grid, lds, block);
    return CHIP_ERR_UNSUPPORTED;
}

// Workgroup shape of K1.  The nq query descriptors sit in LDS (nq*D*elem bytes per workgroup), so the shape follows D:
// 2 workgroups x 512 threads per CU while two copies fit in the 160 KiB (D = 4096 fp32: 48 KiB each), else 1 x 1024 threads
// (D = 8192 fp32, the reference's default model, or D = 4096 fp64: 96 KiB) -- the same 16 waves per CU either way
// (measured: 6.7 TB/s vs 5.5 with 512 x 1).  CHIP_SCAN_BLOCK / CHIP_SCAN_BPC override (tuning only).
// Double rows: how many of the nq queries are NOT staged in LDS but read in place (db_scan_topk_wide); 0 = all of them fit.
int scan_wide_ng(const Ctx *c, int nq)
{
    if (c->elem != 8 || (size_t)nq * c->D * 8 <= 160 * 1024) return 0;
    const int fit = (int)((160 * 1024) / ((size_t)c->D * 8));
    return nq - (fit < 1 ? 1 : fit);
}

static size_t scan_lds_bytes(const Ctx *c, int nq, int K, int block, bool q64, bool rows_form = false)
{
    if (rows_form) return (size_t)nq * c->D * c->elem + (size_t)(block / 64) * nq * CHIP_MAX_TOPK * sizeof(chip_topk_entry) + 16;   // queries + running lists + the claim counter
    const size_t lds_q = (size_t)(q64 ? nq : nq - scan_wide_ng(c, nq)) * c->D * (q64 ? 8 : c->elem);   // the staged queries
    const size_t lds_m = (size_t)(block / 64) * nq * K * sizeof(chip_topk_entry);
    return lds_q > lds_m ? lds_q : lds_m;
}

static void scan_shape(const Ctx *c, int nq, bool q64, int *block, int *bpc)
{
    if (c->scan_block > 0) { *block = c->scan_block; *bpc = c->scan_blocks_per_cu; return; }
    const bool two_fit = 2 * (scan_lds_bytes(c, nq, CHIP_MAX_TOPK, 512, q64) + 1024) <= 160 * 1024;
    *block = two_fit ? 512 : 1024;
    *bpc = two_fit ? 2 : 1;
}

// Queries staged in LDS as fp64 (NT == 8: no per-row conversion of the query side, 21 instead of 34 VALU instructions per KiB
// of DB) for LONG scans of float rows: 8 bytes per query element make it one 1024-thread workgroup per CU, whose per-launch
// cost (96 KiB of staging per workgroup) only pays off on launches long enough to run alone on the scan stream -- measured
// +1.0-1.1 % at 750k / 1M rows, -0.5 .. -6 % at 500k .. 100k rows.  Same arithmetic, same bits.  CHIP_SCAN_VARIANT=1 / 7 disable it.
bool scan_q64(const Ctx *c, int nq, bool long_scan)
{
    return long_scan && c->elem == 4 && c->scan_variant != 1 && c->scan_variant != 7 && (int64_t)c->D * 4 % 4096 == 0 &&
           (size_t)nq * c->D * 8 <= 150 * 1024;
}

// Row-batched form of K1 (db_scan_topk_rows): R rows per wave in flight.  Returns R (1..3), or 0 for the one-row kernel.
// CHIP_SCAN_ROWS forces R for every scan (1..3) or disables the form (-1).
int scan_forms_built()
{
#ifdef CHIP_NO_ROWS_FORM
    return CHIP_SCAN_FORM_ONE_ROW;
#else
    return CHIP_SCAN_FORM_ONE_ROW | CHIP_SCAN_FORM_ROWS;
#endif
}

int scan_rows_form(const Ctx *c, int64_t n_rows, int nq, int grid, bool q64, bool sync_tick)
{
#ifdef CHIP_NO_ROWS_FORM
    (void)c; (void)n_rows; (void)nq; (void)grid; (void)q64; (void)sync_tick;
    return 0;
#endif
    if (q64 || c->scan_rows < 0 || c->scan_variant == 1 || (int64_t)c->D * c->elem % 4096 != 0) return 0;
    int block, bpc;
    scan_shape(c, nq, false, &block, &bpc);
    if ((size_t)bpc * scan_lds_bytes(c, nq, CHIP_MAX_TOPK, block, false, true) > 160 * 1024) return 0;   // queries + LDS lists must fit
    const int64_t waves = (int64_t)grid * (block / 64);
    const int64_t rpw = (n_rows + waves - 1) / waves;
    const int rmax = nq >= 4 ? 1 : 3;
    if (c->scan_rows > 0) return c->scan_rows > rmax ? rmax : c->scan_rows;
    (void)rpw;
    // Default policy, from A/B runs on one box (us per tick, 4096-D; profiles/r03_short_scan_ab_2.txt, r03_mid_scan_ab.txt):
    //   10k rows (164 MB): rows form R = 1 / 2 / 3 at half occupancy 25.1 / 26.5 / 27.7, one-row kernel 30.0;
    //   29k rows (475 MB, the reference's own capacity, Cerebro.cpp:946): rows form R = 1 with temporal loads 66.4, one-row kernel
    //   71.7, rows form with non-temporal loads R = 1 / 2 / 3 75.6 / 75.1 / 83.8;   60k rows (983 MB): 142.1 vs 141.3;
    //   100k / 1M rows: one-row kernel 232 / 2355 vs 245 / 2353.
    // => prefixes up to scan_plain_bytes (768 MiB: a good part of them survives in the 256 MiB Infinity Cache from tick to tick) take
    //    the rows form with R = 1 and temporal loads; longer ones the one-row kernel with non-temporal loads.
    // Round 6, beyond 768 MiB (non-temporal loads either way; us: isolated kernel / pipelined step / SYNCHRONOUS tick, two boxes,
    // profiles/r06_scan_rows_policy_ab.txt, r06_shape_ab_8192.txt):
    //   4096-D x  60k (0.98 GB): one-row 167 / 155 / 188   rows R = 1 165 / 149 / 162   R = 2 169 / 149 / 171
    //   4096-D x 100k (1.64 GB): one-row 257 / 245 / 282   rows R = 1 257 / 268 / 259   R = 2 264 / 256 / 274
    //   8192-D x  29k (0.95 GB, the reference's default model at its own capacity, Cerebro.cpp:946,1021):
    //                            one-row 180 / 166 / 207   rows R = 1 180 / 154 / 182   R = 2 168-172 / 153-157 / 170-178
    // => a SYNCHRONOUS tick (chip_loop_tick: what the reference's 10 Hz thread issues) takes the rows form -- fused, ONE launch, no
    //    merge kernel behind the scan -- up to scan_sync_plain_bytes (4 GiB; beyond that the 25 us are < 1 % of the tick); rows of
    //    32 KiB and more (8192-D floats) with two rows per wave in flight there, pipelined ticks of such rows likewise up to 2 GiB.
    const double bytes = (double)n_rows * c->D * c->elem;
    if (bytes <= c->scan_plain_bytes) return 1;
    const bool wide_rows = (int64_t)c->D * c->elem >= 32768 && nq < 4;
    if (sync_tick && bytes <= c->scan_sync_plain_bytes) return wide_rows ? 2 : 1;
    if (wide_rows && bytes <= 2048.0 * 1024 * 1024) return 2;
    return 0;
}

int scan_grid_for(const Ctx *c, int64_t n_rows, int nq, bool q64)
{
    int block, bpc;
    scan_shape(c, nq, q64, &block, &bpc);
    const int wpb = block / 64;
    int64_t want = (n_rows + wpb - 1) / wpb;
    // scan_reserve leaves workgroup slots free for the small kernels.  With the round-1 load path a full grid held every
    // CU's registers (2 x 8 waves x 110 VGPRs), so a merge (or the RCCL all-gather kernel) launched underneath a running scan
    // waited for a scan workgroup to retire -- and grid-stride workgroups retire only at the END of the scan: reserving 4 slots
    // cut the merge's wait from ~1.7 ms to ~30 us at 1M rows.  At 66 VGPRs and 96 of 160 KiB LDS per CU our own merges fit
    // next to a full grid (reserve 0 and 4 measure the same at 125k rows); the reserve stays on where an exchange is attached
    // because the collective's kernel is not ours to size.  Default: 0 on a plain ctx, 4 on a sharded ctx / group
    // sub-context.  CHIP_SCAN_RESERVE overrides.
    int64_t cap = (int64_t)c->n_cus * bpc - c->scan_reserve;
    // Cache-sized prefixes (BASELINE config 2: 164 MB at 10k rows) are ticked over faster than a launch can ramp up and drain:
    // per-wave stamps of a 10k-row launch show ~20 us of streaming at the memory system's limit inside a 33-40 us launch (spread of
    // the wave starts, query staging, the workgroups' tails).  A launch that takes only HALF of every CU's workgroup slots lets the
    // launches of consecutive ticks (alternating scan streams) be resident TOGETHER, so one tick streams while its neighbours ramp
    // up / finish; 8 waves x 12 KiB in flight per CU already saturate the memory system.
    if (bpc > 1 && c->scan_short_bpc > 0 && c->scan_short_bpc < bpc && (double)n_rows * c->D * c->elem <= c->scan_half_bytes)
        cap = (int64_t)c->n_cus * c->scan_short_bpc - c->scan_reserve;
    if (cap > c->max_grid) cap = c->max_grid;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    return (int)want;
}

template <typename T>
static int launch_scan_T(Ctx *c, hipStream_t s, const ScanArgs &a, const chip_debug_scan_launch &f)
{
    switch (f.nq) {
        case 1: return launch_scan_q<T, 1>(c, s, a, f);
        case 2: return launch_scan_q<T, 2>(c, s, a, f);
        case 3: return launch_scan_q<T, 3>(c, s, a, f);
        case 4: return launch_scan_q<T, 4>(c, s, a, f);
    }
    return CHIP_ERR_UNSUPPORTED;
}

template <int NQ, int NG>
static int launch_scan_wide(Ctx *c, hipStream_t s, const ScanArgs &a, const chip_debug_scan_launch &f)
{
    const int grid = f.grid, block = f.block, lds = f.lds_bytes;
    if (f.FULL) {
        CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_topk_wide<NQ, NG, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL((db_scan_topk_wide<NQ, NG, true>), dim3(grid), dim3(block), lds, s, a);
    } else {
        CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_topk_wide<NQ, NG, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL((db_scan_topk_wide<NQ, NG, false>), dim3(grid), dim3(block), lds, s, a);
    }
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// WHICH kernel a launch of K1 is: family, template arguments, shape and LDS, from the ctx (knobs, D, storage type), the per-launch
// policy already in `a` (q64, rows_form, plain_loads, dyn_claim, K, the fused tick) and the grid.  Needs no device.
int scan_select(const Ctx *c, const ScanArgs &a, int nq, int grid, chip_debug_scan_launch *f)
{
    *f = chip_debug_scan_launch{};
    if (nq < 1 || nq > CHIP_MAX_NQ) return CHIP_ERR_UNSUPPORTED;
    int block, bpc;
    scan_shape(c, nq, a.q64 != 0, &block, &bpc);
    const size_t lds = scan_lds_bytes(c, nq, a.K, block, a.q64 != 0, a.rows_form > 0);
    if (lds > 160 * 1024 || grid > 512) return CHIP_ERR_UNSUPPORTED;  // K2 holds one partial list per thread
    f->elem = c->elem;
    f->nq = nq;
    f->K = a.K;
    f->q64 = a.q64 != 0;
    f->fused = a.fused_result != nullptr;
    f->grid = grid;
    f->block = block;
    f->wg_per_cu = bpc;
    f->lds_bytes = (int32_t)lds;
    f->n_rows = a.n_rows;
    const int64_t row_bytes = (int64_t)c->D * c->elem;
    if (const int ng = scan_wide_ng(c, nq); ng > 0 && !a.q64 && a.rows_form == 0) {   // double rows wider than the LDS holds nq queries of
        if (!((nq == 3 && ng == 1) || (nq == 4 && (ng == 1 || ng == 2)))) return CHIP_ERR_UNSUPPORTED;   // chip_create bounds D so that two double queries always fit
        f->family = CHIP_SCAN_FAMILY_WIDE;
        f->NG = ng;
        f->FULL = c->D % 512 == 0;
        return CHIP_OK;
    }
    f->family = CHIP_SCAN_FAMILY_ONE_ROW;
    f->R = 1;
    if (c->elem == 4 && a.q64) { f->U = 4; f->NT = 8; f->FULL = 1; return CHIP_OK; }   // scan_q64() said so (float rows only)
#ifndef CHIP_NO_ROWS_FORM
    if (a.rows_form > 0) {   // scan_rows_form() said so: whole 4 KiB batches, R rows per wave in one continuous load stream
        f->family = CHIP_SCAN_FAMILY_ROWS;
        f->R = nq <= 3 ? (a.rows_form >= 3 ? 3 : a.rows_form) : 1;   // (four queries: R = 1 only, launch_scan_q)
        f->NTL = a.plain_loads == 0;
        f->claimed = a.dyn_claim != 0;
        return CHIP_OK;
    }
#endif
    f->FULL = 1;
    if (c->scan_variant != 1) {   // rows of whole 4 KiB / 2 KiB batches (one load per batch measured slower than the builtin path)
        if (row_bytes % 4096 == 0) { f->U = 4; f->NT = 6; return CHIP_OK; }
        if (row_bytes % 2048 == 0) { f->U = 2; f->NT = 6; return CHIP_OK; }
    }
    f->U = 8;   // the builtin path: 8 x 16 B per lane and step, the last step of a row guarded unless rows are whole steps
    f->NT = 1;
    f->FULL = row_bytes % 8192 == 0;
    return CHIP_OK;
}

int launch_scan(Ctx *c, hipStream_t s, const ScanArgs &a, int nq, int grid)
{
    chip_debug_scan_launch f;
    int rc = scan_select(c, a, nq, grid, &f);
    if (rc != CHIP_OK) return rc;
    if (f.family == CHIP_SCAN_FAMILY_WIDE) {
        if (nq == 3 && f.NG == 1) rc = launch_scan_wide<3, 1>(c, s, a, f);
        else if (nq == 4 && f.NG == 1) rc = launch_scan_wide<4, 1>(c, s, a, f);
        else if (nq == 4 && f.NG == 2) rc = launch_scan_wide<4, 2>(c, s, a, f);
        else rc = CHIP_ERR_UNSUPPORTED;
    } else {
        rc = c->elem == 8 ? launch_scan_T<double>(c, s, a, f) : launch_scan_T<float>(c, s, a, f);
    }
    if (rc != CHIP_OK) return rc;
    f.launches = c->last_scan.launches + 1;
    c->last_scan = f;
    return CHIP_OK;
}

// The shared passes (db_scan_topk_multi / db_scan_shared_f64: family MULTI; db_scan_prefilter: family PREFILTER).  The ONE place that sizes such
// a pass: which queries are staged and how much LDS the launch asks for, from D, the storage type, the ticks and K alone -- launch_pass
// launches what this says, scan_multi_max_ticks / scan_prefilter_usable ask it what a ctx can be served with, chip_debug_multi_plan and
// chip_debug_prefilter_plan hand it out without a device.  Rows of whole 4 KiB batches; as many of the 3 T queries staged in the rows' type
// as fit the LDS next to the lists, the other NG read in place where an instantiation exists for that NG:
//   MULTI, float rows : T = 2, 3; NG = 0 only (D = 4096: T <= 3; D = 8192: none);
//   MULTI, double rows: T = 2; NG <= 2 (D <= 3072: NG = 0; D = 3584: 1; D = 4096, 4608: 2; wider rows: no such form);
//   PREFILTER         : float rows, T = 4; NG = 0 (D <= 3072) or 3 (D = 4096); wider rows, K = 16 at D = 4096 and double rows have no such pass;
//   HALFQ             : float rows, T = 5; every query staged as fp16 (2 bytes per element), NG = 0 only: D <= 4096.
static int pass_plan(int family, int D, int elem, int n_ticks, int K, int grid, chip_debug_scan_launch *f)
{
    *f = chip_debug_scan_launch{};
    const bool prefilter = family == CHIP_SCAN_FAMILY_PREFILTER, halfq = family == CHIP_SCAN_FAMILY_HALFQ;
    if (D < 1 || (elem != 4 && elem != 8) || K < 1 || K > CHIP_MAX_TOPK || grid < 1 || grid > 512 || (int64_t)D * elem % 4096 != 0) return CHIP_ERR_UNSUPPORTED;
    if (prefilter || halfq ? elem != 4 : n_ticks < 2 || n_ticks > (elem == 8 ? kSharedF64MaxTicks : kMultiMaxTicks)) return CHIP_ERR_UNSUPPORTED;
    const int nq = 3 * n_ticks;
    const size_t kLds = 160 * 1024, lists = (size_t)(kMultiBlock / 64) * nq * K * sizeof(chip_topk_entry);   // [wave][3T][K] behind the queries
    const int max_ng = prefilter ? kPrefilterMaxNG : elem == 8 ? kSharedMaxNG : 0;
    const size_t staged_elem = halfq ? sizeof(_Float16) : (size_t)elem;
    const size_t fit = max_ng > 0 ? (kLds - lists) / ((size_t)D * staged_elem) : (size_t)nq;
    const int staged = fit < (size_t)nq ? (int)fit : nq, ng = nq - staged;
    if (prefilter ? ng != 0 && ng != kPrefilterMaxNG : ng > max_ng) return CHIP_ERR_UNSUPPORTED;   // an NG no instantiation exists for
    const size_t lds = (size_t)staged * D * staged_elem + lists;
    if (lds > kLds) return CHIP_ERR_UNSUPPORTED;
    f->family = family;
    f->elem = elem;
    f->nq = nq;
    f->K = K;
    f->U = kMultiU;
    f->FULL = 1;
    f->R = kMultiR;
    f->NTL = 1;
    f->ticks = n_ticks;
    f->q64 = elem == 8 ? staged : 0;   // queries staged as fp64 (float rows stage fp32)
    f->NG = ng;
    f->grid = grid;
    f->block = kMultiBlock;
    f->wg_per_cu = 1;
    f->lds_bytes = (int32_t)lds;
    return CHIP_OK;
}
int scan_multi_plan(int D, int elem, int n_ticks, int K, int grid, chip_debug_scan_launch *f) { return pass_plan(CHIP_SCAN_FAMILY_MULTI, D, elem, n_ticks, K, grid, f); }
int scan_prefilter_plan(int D, int elem, int K, int grid, chip_debug_scan_launch *f) { return pass_plan(CHIP_SCAN_FAMILY_PREFILTER, D, elem, kPrefilterTicks, K, grid, f); }

int scan_halfq_plan(int D, int elem, int K, int grid, chip_debug_scan_launch *f) { return pass_plan(CHIP_SCAN_FAMILY_HALFQ, D, elem, kHalfqTicks, K, grid, f); }

int scan_multi_grid(const Ctx *c) { return c->n_cus < c->max_grid ? c->n_cus : c->max_grid; }   // one 8-wave workgroup per CU

// How many ticks one pass can serve on this ctx, with the K the tick path asks for: 0 when there is no such form.
int scan_multi_max_ticks(const Ctx *c)
{
    if (c->nranks != 1 || c->scan_variant != 0 || c->scan_rows > 0) return 0;
    chip_debug_scan_launch f;
    for (int t = kMultiMaxTicks; t >= 2; t--)
        if (scan_multi_plan(c->D, c->elem, t, CHIP_DEFAULT_TOPK, scan_multi_grid(c), &f) == CHIP_OK) return t;
    return 0;
}

// E of DESIGN.md 3: (gamma_32 + gamma_64) N^2 + D 2^-148 with gamma_32 = 2 D u / (1 - 2 D u), u = 2^-24, gamma_64 = (D + 8) 2^-53 / (1 - (D + 8) 2^-53),
// evaluated in fp64 and rounded up (a handful of roundings, each below 2^-52 relative: the factor 1 + 2^-40 covers them).
double prefilter_error_bound(int D, double row_norm_max)
{
    const double u32 = 2.0 * D * std::ldexp(1.0, -24), u64 = (D + 8.0) * std::ldexp(1.0, -53);
    const double g = u32 / (1.0 - u32) + u64 / (1.0 - u64);
    return (g * row_norm_max * row_norm_max + D * std::ldexp(1.0, -148)) * (1.0 + std::ldexp(1.0, -40));
}

bool scan_prefilter_usable(const Ctx *c)
{
    if (c->elem != 4 || c->nranks != 1 || c->scan_variant != 0 || c->scan_rows > 0) return false;
    chip_debug_scan_launch f;
    if (scan_prefilter_plan(c->D, c->elem, CHIP_DEFAULT_TOPK, scan_multi_grid(c), &f) != CHIP_OK) return false;
    double n;
    { std::lock_guard<std::mutex> lk(c->mu); n = c->row_norm_max; }
    return n * n <= std::ldexp(1.0, 120) && 2.0 * c->D * std::ldexp(1.0, -24) < 0.5;   // no overflow of an fp32 partial sum (false for NaN as well)
}

// The five-tick pass.  e: the largest exponent with 2^e N <= 2^15 for the row-norm bound N -- an element of a published row is
// at most N in magnitude, so no staged half overflows (fp16 holds up to 65504) -- kept inside [-100, 100] so that 2^e and 2^-e are
// normal floats whatever N is (a smaller e than the largest is always safe; halfq_error_bound is evaluated with the e that is used).
int halfq_exponent(double row_norm_max)
{
    int x = 0;
    if (row_norm_max > 0.0 && std::isfinite(row_norm_max) && std::frexp(row_norm_max, &x) == 0.5) x--;   // N = m 2^x, 1/2 <= m < 1: N <= 2^x (a power of two: N = 2^(x-1))
    const int e = 15 - x;
    return e > 100 ? 100 : e < -100 ? -100 : e;
}

// E_h of DESIGN.md 3: gamma_64 N^2 + (gamma_32 (1 + 2^-11) + 2^-11) N^2 + (1 + gamma_32) N sqrt(D) 2^(-25-e) + D 2^(-149-e), gamma_32 and gamma_64
// as in prefilter_error_bound, evaluated in fp64 and rounded up.
double halfq_error_bound(int D, double row_norm_max, int e)
{
    const double u32 = 2.0 * D * std::ldexp(1.0, -24), u64 = (D + 8.0) * std::ldexp(1.0, -53);
    const double g32 = u32 / (1.0 - u32), g64 = u64 / (1.0 - u64), h = std::ldexp(1.0, -11), n2 = row_norm_max * row_norm_max;
    const double E = g64 * n2 + (g32 * (1.0 + h) + h) * n2 + (1.0 + g32) * row_norm_max * std::sqrt((double)D) * std::ldexp(1.0, -25 - e) +
                     D * std::ldexp(1.0, -149 - e);
    return E * (1.0 + std::ldexp(1.0, -40));
}

// N < 2^105: then e >= -90 and 2^e N^2 (1 + 2^-11) <= 2^121 bounds every fp32 partial sum of the scaled pass (false for NaN as well)
bool scan_halfq_usable(const Ctx *c)
{
    if (c->elem != 4 || c->nranks != 1 || c->scan_variant != 0 || c->scan_rows > 0) return false;
    chip_debug_scan_launch f;
    if (scan_halfq_plan(c->D, c->elem, CHIP_DEFAULT_TOPK, scan_multi_grid(c), &f) != CHIP_OK) return false;
    double n;
    { std::lock_guard<std::mutex> lk(c->mu); n = c->row_norm_max; }
    return n < std::ldexp(1.0, 105) && 2.0 * c->D * std::ldexp(1.0, -24) < 0.5;
}

// a shared pass as planned: the launch and the record of it (Ctx::last_scan)
template <class Kernel>
static int launch_pass(Ctx *c, hipStream_t s, Kernel kernel, const PassArgs &a, chip_debug_scan_launch f)
{
    CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, f.lds_bytes));
    hipLaunchKernelGGL(kernel, dim3(f.grid), dim3(kMultiBlock), f.lds_bytes, s, a);
    CHIP_HIP(c, hipGetLastError());
    f.n_rows = a.n_rows;
    f.launches = c->last_scan.launches + 1;
    c->last_scan = f;
    return CHIP_OK;
}

int launch_scan_multi(Ctx *c, hipStream_t s, const PassArgs &a, int n_ticks, int grid)
{
    chip_debug_scan_launch f;
    if (n_ticks > scan_multi_max_ticks(c) || grid > c->max_grid || scan_multi_plan(c->D, c->elem, n_ticks, a.K, grid, &f) != CHIP_OK)
        return CHIP_ERR_UNSUPPORTED;
    if (c->elem == 4) return n_ticks == 2 ? launch_pass(c, s, db_scan_topk_multi<2>, a, f) : launch_pass(c, s, db_scan_topk_multi<3>, a, f);
    static_assert(kSharedF64MaxTicks == 2 && kSharedMaxNG == 2, "the instantiations below");
    if (f.NG == 0) return launch_pass(c, s, db_scan_shared_f64<2, 0>, a, f);
    if (f.NG == 1) return launch_pass(c, s, db_scan_shared_f64<2, 1>, a, f);
    return launch_pass(c, s, db_scan_shared_f64<2, 2>, a, f);
}

int launch_scan_prefilter(Ctx *c, hipStream_t s, const PassArgs &a, int grid)
{
    chip_debug_scan_launch f;
    if (grid > c->max_grid || scan_prefilter_plan(c->D, c->elem, a.K, grid, &f) != CHIP_OK) return CHIP_ERR_UNSUPPORTED;
    return f.NG == 0 ? launch_pass(c, s, db_scan_prefilter<0>, a, f) : launch_pass(c, s, db_scan_prefilter<kPrefilterMaxNG>, a, f);
}

int launch_scan_halfq(Ctx *c, hipStream_t s, const PassArgs &a, int grid)
{
    chip_debug_scan_launch f;
    if (grid > c->max_grid || scan_halfq_plan(c->D, c->elem, a.K, grid, &f) != CHIP_OK || !(a.q_up > 0.0f)) return CHIP_ERR_UNSUPPORTED;
    return launch_pass(c, s, db_scan_halfq, a, f);
}

int launch_rescore(Ctx *c, hipStream_t s, const RescoreArgs &a, int n_ticks)
{
    if (a.n_lists > 512 || a.K > CHIP_MAX_TOPK || n_ticks < 1 || n_ticks > kPassMaxTicks) return CHIP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tick_rescore, dim3(3 * n_ticks), dim3(512), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

int launch_resident(Ctx *c, hipStream_t s, const ResidentArgs &ra, int grid)
{
#ifdef CHIP_NO_ROWS_FORM
    (void)c; (void)s; (void)ra; (void)grid;
    return CHIP_ERR_UNSUPPORTED;
#else
    int block, bpc;
    scan_shape(c, 3, false, &block, &bpc);
    const size_t lds = scan_lds_bytes(c, 3, 1, block, false, true);
    if (lds + 64 > 160 * 1024 || grid > 512) return CHIP_ERR_UNSUPPORTED;
    return c->elem == 8 ? launch_resident_T<double>(c, s, ra, grid, lds, block) : launch_resident_T<float>(c, s, ra, grid, lds, block);
#endif
}

// ------------------------------------------------------------------------------------------------ K1s
// The whole score vector u = v^T * M.leftCols(k) of ONE query (src/Cerebro.cpp:1026; the reference's debug plot consumes all
// of u, :1047-1052): same per-row arithmetic as K1 (rows_dot + butterfly => the same bits), one wave per row, out[local row].
template <typename T, bool FULL>
__global__ __launch_bounds__(512) void db_scan_scores(ScanArgs a, double *out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *qs = reinterpret_cast<T *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpb = blockDim.x >> 6;
    stage_queries<T, 1>(a, qs, tid, blockDim.x);
    __syncthreads();
    const int64_t tw = (int64_t)gridDim.x * wpb;
    for (int64_t r = (int64_t)blockIdx.x * wpb + wave; r < a.n_rows; r += tw) {
        const T *row[1] = {row_base<T>(a, r)};
        double acc[1][1];
        rows_dot<T, 1, 4, FULL, FULL ? 6 : 1, 1>(row, qs, a.D, lane, acc);   // whole 4 KiB batches: the asm load path of K1
        const double s = butterfly_sum(acc[0][0]);
        if (lane == 0) out[r] = s;
    }
}

int launch_scores(Ctx *c, hipStream_t s, const ScanArgs &a, double *out_dev)
{
    const size_t lds = (size_t)c->D * c->elem;
    int64_t grid = (a.n_rows + 7) / 8;
    if (grid > (int64_t)c->n_cus * 4) grid = (int64_t)c->n_cus * 4;
    if (grid < 1) grid = 1;
    const int chunk = 64 * (16 / c->elem) * 4;
    const bool full = a.D % chunk == 0;
    if (c->elem == 8) {
        if (lds > 65536) {
            CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_scores<double, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(db_scan_scores<double, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        if (full) hipLaunchKernelGGL((db_scan_scores<double, true>), dim3((int)grid), dim3(512), lds, s, a, out_dev);
        else hipLaunchKernelGGL((db_scan_scores<double, false>), dim3((int)grid), dim3(512), lds, s, a, out_dev);
    } else {
        if (full) hipLaunchKernelGGL((db_scan_scores<float, true>), dim3((int)grid), dim3(512), lds, s, a, out_dev);
        else hipLaunchKernelGGL((db_scan_scores<float, false>), dim3((int)grid), dim3(512), lds, s, a, out_dev);
    }
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ K2
// Merge (+ decision) of the per-workgroup lists of a scan, or of the per-GPU lists after the RCCL all-gather: one
// workgroup of 512 threads.
template <int NQ>
__global__ __launch_bounds__(512) void topk_merge(MergeArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[kMergeSmem];
    merge_sorted_lists<NQ>(a.in, a.n_lists, NQ, 0, a.K, a.out, a.result, a.l, a.locality, a.thresh, smem);
}

int launch_merge(Ctx *c, hipStream_t s, const MergeArgs &a, int nq)
{
    if (a.n_lists > 512) return CHIP_ERR_UNSUPPORTED;
    switch (nq) {
        case 1: hipLaunchKernelGGL(topk_merge<1>, dim3(1), dim3(512), 0, s, a); break;
        case 2: hipLaunchKernelGGL(topk_merge<2>, dim3(1), dim3(512), 0, s, a); break;
        case 3: hipLaunchKernelGGL(topk_merge<3>, dim3(1), dim3(512), 0, s, a); break;
        case 4: hipLaunchKernelGGL(topk_merge<4>, dim3(1), dim3(512), 0, s, a); break;
        default: return CHIP_ERR_UNSUPPORTED;
    }
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ K3
struct StoreArgs {
    void *const *seg_table;
    int32_t seg_shift;
    int64_t seg_mask;
    void *ring;
    int32_t D;
    int32_t rank, nranks;
    int64_t first_global;
    int64_t row_stride;  // staged row r is global row first_global + r * row_stride (1: a contiguous batch; G: one shard's rows only)
    int64_t n;
    int64_t ring_from;   // only global rows >= ring_from are mirrored into the ring (the newest CHIP_RING_ROWS)
    uint32_t *flags;
};

// four consecutive elements of global row g, starting at element e, into the DB (if this rank owns the row) and the ring
template <typename T>
__device__ __forceinline__ void store_row4(const StoreArgs &a, int64_t g, int e, const T (&v)[4])
{
    typedef typename Vec16<T>::type V;
    constexpr int N = Vec16<T>::N;
    V pk[4 / N];
#pragma unroll
    for (int c = 0; c < 4; c++) pk[c / N][c % N] = v[c];
    if (a.nranks == 1 || (g % a.nranks) == a.rank) {
        const int64_t loc = a.nranks == 1 ? g : g / a.nranks;
        T *dst = static_cast<T *>(a.seg_table[loc >> a.seg_shift]) + (loc & a.seg_mask) * (int64_t)a.D + e;
#pragma unroll
        for (int h = 0; h < 4 / N; h++) reinterpret_cast<V *>(dst)[h] = pk[h];
    }
    if (a.ring && g >= a.ring_from) {
        T *dst = static_cast<T *>(a.ring) + (g % CHIP_RING_ROWS) * (int64_t)a.D + e;
#pragma unroll
        for (int h = 0; h < 4 / N; h++) reinterpret_cast<V *>(dst)[h] = pk[h];
    }
}

// 4u (flag bit2) if the float a finite double narrowed to is +-Inf: exponent field 0xff, by integer arithmetic on the bits (no compare: the
// kernel keeps the registers recorded in profiles/project.md)
__device__ __forceinline__ uint32_t inf_bit2(float v) { return (((__float_as_uint(v) & 0x7fffffffu) + 0x00800000u) >> 31) << 2; }
__device__ __forceinline__ uint32_t inf_bit2(double) { return 0u; }

// M.col(_s) = desc (Cerebro.cpp:1005-1006): wire type S (float64[] of the .srv, or float) -> storage type T.
//   double -> float : round-to-nearest-even, flag bit0 unless (double)(float)x == x (lossless narrowing is the contract)
//   float  -> double, same -> same : exact.        NaN / Inf in any combination: flag bit1.
//   double -> float of a finite |x| >= 0x1.ffffffp+127: the float is +-Inf; bit0 and bit2 (ctx_append: refused with or without the flag)
template <typename S, typename T>
__global__ __launch_bounds__(256) void convert_rows(StoreArgs a, const S *__restrict__ src)
{
    const int64_t per_row = a.D / 4;
    const int64_t total = a.n * per_row;
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int e = (int)(i - r * per_row) * 4;
        S x[4];
        if constexpr (sizeof(S) == 8) {
            const f64x2 lo = *reinterpret_cast<const f64x2 *>(src + r * a.D + e);
            const f64x2 hi = *reinterpret_cast<const f64x2 *>(src + r * a.D + e + 2);
            x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
        } else {
            const f32x4 w = *reinterpret_cast<const f32x4 *>(src + r * a.D + e);
            x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
        }
        T v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            v[c] = (T)x[c];
            if (!(fabs((double)x[c]) <= 1.79769313486231570e308)) bad |= 2u;   // NaN / Inf
            else if (sizeof(T) < sizeof(S) && (S)v[c] != x[c]) bad |= 1u | inf_bit2(v[c]);   // not fp32-representable (incl. overflow)
        }
        store_row4<T>(a, a.first_global + r * a.row_stride, e, v);
    }
    if (bad) atomicOr(a.flags, bad);
}

// Row-norm bound of a float-row DB (Ctx::row_norm_max, what the prefilter's error bound E is made of): one wave per row just stored, its
// sum of squares in fp64 (the squares of fp32 values are exact), combined over rows by an atomic max on the bits of a non-negative double.
__global__ __launch_bounds__(256) void rows_norm2_max(StoreArgs a, unsigned long long *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.n; r += nw) {
        const int64_t g = a.first_global + r * a.row_stride;
        if (a.nranks != 1 && (g % a.nranks) != a.rank) continue;
        const int64_t loc = a.nranks == 1 ? g : g / a.nranks;
        const float *row = static_cast<const float *>(a.seg_table[loc >> a.seg_shift]) + (loc & a.seg_mask) * (int64_t)a.D;
        double ss = 0.0;
        for (int e = lane * 4; e < a.D; e += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(row + e);
#pragma unroll
            for (int c = 0; c < 4; c++) ss = __builtin_fma((double)v[c], (double)v[c], ss);
        }
        ss = butterfly_sum(ss);
        if (lane == 0 && ss > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(ss));   // (NaN: refused by the append's own check)
    }
}

static int launch_norm2(Ctx *c, hipStream_t s, const StoreArgs &a)
{
    if (c->elem != 4 || !c->norm2_dev.get() || a.n <= 0) return CHIP_OK;
    const int64_t blocks = (a.n + 3) / 4, cap = (int64_t)c->n_cus * 8;
    hipLaunchKernelGGL(rows_norm2_max, dim3((int)(blocks < cap ? blocks : cap)), dim3(256), 0, s, a, c->norm2_dev.get());
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

static StoreArgs make_store_args(Ctx *c, int64_t first_global, int64_t n, uint32_t *flags, bool write_ring = true)
{
    StoreArgs a;
    a.seg_table = c->seg_table_dev;
    a.seg_shift = c->seg_shift;
    a.seg_mask = c->seg_rows - 1;
    a.ring = write_ring ? c->ring_dev : nullptr;
    a.D = c->D;
    a.rank = c->rank;
    a.nranks = c->nranks;
    a.first_global = first_global;
    a.row_stride = 1;
    a.n = n;
    a.ring_from = first_global + n - CHIP_RING_ROWS;
    a.flags = flags;
    return a;
}

static int grid_for_elems(const Ctx *c, int64_t total_threads)
{
    int64_t g = (total_threads + 255) / 256;
    int64_t cap = (int64_t)c->n_cus * 8;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// src_elem: 8 = float64 rows (the wire type), 4 = float rows; the destination type is the ctx's storage type
int launch_store_rows(Ctx *c, hipStream_t s, const void *src, int src_elem, int64_t n, int64_t first_global, uint32_t *flags_dev, bool write_ring,
                      int64_t row_stride)
{
    StoreArgs a = make_store_args(c, first_global, n, flags_dev, write_ring);
    a.row_stride = row_stride;
    const dim3 grid(grid_for_elems(c, n * (c->D / 4))), block(256);
    if (src_elem == 8 && c->elem == 4) hipLaunchKernelGGL((convert_rows<double, float>), grid, block, 0, s, a, static_cast<const double *>(src));
    else if (src_elem == 8) hipLaunchKernelGGL((convert_rows<double, double>), grid, block, 0, s, a, static_cast<const double *>(src));
    else if (c->elem == 4) hipLaunchKernelGGL((convert_rows<float, float>), grid, block, 0, s, a, static_cast<const float *>(src));
    else hipLaunchKernelGGL((convert_rows<float, double>), grid, block, 0, s, a, static_cast<const float *>(src));
    CHIP_HIP(c, hipGetLastError());
    return write_ring ? CHIP_OK : launch_norm2(c, s, a);   // (the ring pass stores rows the DB pass has stored, and measured, already)
}

// ------------------------------------------------------------------------------------------------ synth
// Spec: oracle/dot_scan.c (orc_splitmix64 / orc_synth_row_f32).  Integer domain + one exact int->float
// conversion + one float multiply => bit-identical to the CPU generator.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t synth_rowkey(uint64_t seed, int64_t row)
{
    return splitmix64(seed + 0x632BE59BD9B4E019ULL * (uint64_t)row);
}
__device__ __forceinline__ int32_t synth_from_key(uint64_t key, int32_t e)
{
    const uint64_t h = splitmix64(key + (uint64_t)(uint32_t)e);
    const int32_t s = (int32_t)(h & 0xFFFF) + (int32_t)((h >> 16) & 0xFFFF) + (int32_t)((h >> 32) & 0xFFFF) + (int32_t)(h >> 48);
    return s - 131070;
}

struct SynthArgs {
    StoreArgs st;
    uint64_t seed;
    float scale, scale_planted;
    const int64_t *plant_dst, *plant_src;
    const int32_t *plant_kind;
    int64_t n_plant;
};

template <typename T>
__global__ __launch_bounds__(256) void synth_rows(SynthArgs a)
{
    const int64_t per_row = a.st.D / 4;
    const int64_t total = a.st.n * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int e = (int)(i - r * per_row) * 4;
        const int64_t g = a.st.first_global + r;
        // planted? (binary search over the sorted dst list)
        int32_t kind = 0;
        int64_t src = -1;
        int64_t lo = 0, hi = a.n_plant;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.plant_dst[mid] < g) lo = mid + 1; else hi = mid;
        }
        if (lo < a.n_plant && a.plant_dst[lo] == g) { kind = a.plant_kind[lo]; src = a.plant_src[lo]; }
        const uint64_t key = synth_rowkey(a.seed, g);
        const uint64_t skey = kind ? synth_rowkey(a.seed, src) : 0;
        T v[4];   // the generator is defined in float; a double-storage DB holds the same values widened
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (kind == 0) v[c] = (T)((float)synth_from_key(key, e + c) * a.scale);
            else if (kind == 2) v[c] = (T)((float)synth_from_key(skey, e + c) * a.scale);
            else v[c] = (T)((float)(5 * synth_from_key(skey, e + c) + synth_from_key(key, e + c)) * a.scale_planted);
        }
        store_row4<T>(a.st, g, e, v);
    }
}

// Unit-L2 form of the generator (spec: oracle/dot_scan.c orc_synth_row_unit_f32; SURVEY.md 8d "rows = unit-L2-norm"): the row's integers
// v_e as above, S = sum v_e^2 EXACTLY (64-bit integers: any summation order gives the same S), inv = 1 / sqrt((double)S) (two correctly
// rounded fp64 operations), element = (float)((double)v_e * inv) -- one correctly rounded multiply, one conversion.  So the rows are
// unit vectors to fp32 rounding (| |row| - 1 | ~ 1e-8) AND bit-identical to the CPU generator.  One workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void synth_rows_unit(SynthArgs a)
{
    __shared__ unsigned long long part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_row = a.st.D / 4;
    for (int64_t r = blockIdx.x; r < a.st.n; r += gridDim.x) {
        const int64_t g = a.st.first_global + r;
        int32_t kind = 0;
        int64_t src = -1;
        int64_t lo = 0, hi = a.n_plant;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.plant_dst[mid] < g) lo = mid + 1; else hi = mid;
        }
        if (lo < a.n_plant && a.plant_dst[lo] == g) { kind = a.plant_kind[lo]; src = a.plant_src[lo]; }
        const uint64_t key = synth_rowkey(a.seed, g);
        const uint64_t skey = kind ? synth_rowkey(a.seed, src) : 0;
        auto value = [&](int e) -> int64_t {
            if (kind == 0) return (int64_t)synth_from_key(key, e);
            if (kind == 2) return (int64_t)synth_from_key(skey, e);
            return 5 * (int64_t)synth_from_key(skey, e) + (int64_t)synth_from_key(key, e);
        };
        unsigned long long ss = 0;   // |v| <= 6 * 131070: v^2 < 2^40, a row of 8192 of them < 2^53
        for (int ch = tid; ch < per_row; ch += 256)
#pragma unroll
            for (int c = 0; c < 4; c++) { const int64_t v = value(4 * ch + c); ss += (unsigned long long)(v * v); }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        __syncthreads();   // (part[] of the previous row has been read by everybody)
        if (lane == 0) part[wave] = ss;
        __syncthreads();
        const unsigned long long S = part[0] + part[1] + part[2] + part[3];
        const double inv = S ? 1.0 / sqrt((double)S) : 0.0;
        for (int ch = tid; ch < per_row; ch += 256) {
            T v[4];
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = (T)(float)((double)value(4 * ch + c) * inv);
            store_row4<T>(a.st, g, 4 * ch, v);
        }
    }
}

int launch_synth(Ctx *c, hipStream_t s, int64_t first_global, int64_t n, uint64_t seed,
                 const int64_t *plant_dst_dev, const int64_t *plant_src_dev, const int32_t *plant_kind_dev, int64_t n_plant, int unit)
{
    SynthArgs a;
    a.st = make_store_args(c, first_global, n, nullptr);
    a.seed = seed;
    const double var = 1431655765.0;  // 4 * (65536^2 - 1) / 12
    a.scale = (float)(1.0 / std::sqrt((double)c->D * var));
    a.scale_planted = (float)(1.0 / std::sqrt((double)c->D * var * 26.0));
    a.plant_dst = plant_dst_dev;
    a.plant_src = plant_src_dev;
    a.plant_kind = plant_kind_dev;
    a.n_plant = n_plant;
    if (unit) {
        const int grid = (int)(n < (int64_t)c->n_cus * 32 ? n : (int64_t)c->n_cus * 32);
        if (c->elem == 8) hipLaunchKernelGGL(synth_rows_unit<double>, dim3(grid), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(synth_rows_unit<float>, dim3(grid), dim3(256), 0, s, a);
    } else if (c->elem == 8) hipLaunchKernelGGL(synth_rows<double>, dim3(grid_for_elems(c, n * (c->D / 4))), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(synth_rows<float>, dim3(grid_for_elems(c, n * (c->D / 4))), dim3(256), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    return launch_norm2(c, s, a.st);   // generated rows and plants alike
}

}  // namespace chip
