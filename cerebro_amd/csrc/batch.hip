// batch.hip -- many-query batched mode (BASELINE north_star: "MFMA used only for the batched
// descriptor x database GEMM where it is genuinely a dense fp32 contraction").
//
// Semantics: the fp32 inner-product search of the reference's compiled-out faiss variants (faiss::IndexFlatIP on
// X.cast<float>(), top-k labels; /root/reference/src/Cerebro.cpp:390,422,455-472) for Q queries at once:
//   score(q, row) = one k-ordered fp32 fmaf chain over the D elements   (oracle: orc_dot_fmaf_f32)
//   top-k per query ordered (score desc, index desc).
// With Q >= ~40 queries per DB pass the arithmetic intensity (Q/2 flop/B) crosses the 19.7 flop/B ridge, so the work
// belongs on the matrix cores: v_mfma_f32_32x32x2_f32 is exact fp32 (bit-for-bit a k-ordered fmaf chain,
// cdna_hip_programming.md 3) at the 157 TFLOP/s vector rate.
//
// K_B db_gemm_topk<KC, WN, KL> : grid (P workgroups) x (query tiles).  Tile = 64 WN queries x 64 WN DB rows on 2 x WN waves,
//   each wave owning WN x 2 MFMA 32x32 accumulators (64 WN queries x 64 DB rows):
//     WN = 4: 256 x 256 on 8 waves, one workgroup per CU -- 16 MFMAs per 6 fragment reads, one workgroup barrier per 128 MFMAs,
//             the DB streamed once per 256 queries; used when the padded query count is a multiple of 256 (0.84 of the fp32
//             matrix peak at Q = 256 x 1M rows);
//     WN = 2: 128 x 128 on 4 waves, two workgroups per CU (0.78), for everything else.
//   K is streamed in chunks of 32 through a two-stage LDS ring filled by LDS-DMA (see "LDS-DMA tile staging" below).  DB tiles
//   are claimed from a counter (one atomic per ~1 ms tile).  After the K loop of a tile its scores go through the same LDS, 128
//   DB rows per pass, and ALL threads scan them against register-resident sorted top-K lists (thread = query x 64-column half;
//   KL = list capacity, 8 or 16).  One sorted list per workgroup and query is written; topk_merge_batch (the shared
//   merge_sorted_lists) merges them.
#include "chip_internal.h"
#include "topk_merge.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>

namespace chip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int BM = 128;              // queries are padded to a multiple of the small tile
constexpr int CT_LD = 128 + 1;      // score tile in LDS [tile queries][129]: 128 DB rows per epilogue pass
// DB tile of one stage in LDS: 16 blocks of 8 rows x 32 floats (one LDS-DMA instruction each: 1 KiB, lane-linear), block b
// placed at b * kBBlock + (b & 3) floats -- rotated by 0..3 floats, which the LDS-DMA honours (its destination base only needs
// 4-byte alignment: scripts/probes/glds_align_probe.hip) -- 4 floats of padding per block keep the rotated blocks apart.
constexpr int kBBlock = 8 * 32 + 4;
constexpr int NST = 2;              // stages of the LDS ring a tile's K chunks go through (four at one workgroup per CU measured slower)
constexpr int kMaxQTiles = 4096;    // query tiles per call (grid.y); 4096 x 128 queries
__device__ __forceinline__ constexpr int b_row_off(int row) { return (row >> 3) * kBBlock + ((row >> 3) & 3) + (row & 7) * 32; }

struct BatchArgs {
    const void *const *seg_table;   // rows of the ctx's storage type: float, or double (the cast form of the kernel)
    int32_t seg_shift;
    int64_t seg_mask;
    int64_t n_rows;         // local rows [0, n_rows)
    int32_t D;
    const float *Q;         // [Qpad][D] device, rows >= Q are zero
    const float *Qt;        // the same queries as K-chunk-major transposed tiles: [Qpad/128][D/32][32][128]
    int32_t Qpad;
    int32_t K;
    uint32_t *tile_ctr;     // [query tiles] next unclaimed DB tile (zeroed before the launch)
    int64_t idx_mul, idx_add;
    chip_topk_entry *partial;  // [P][Qpad][K]
};

__device__ __forceinline__ bool fkey_gt(float s, int32_t i, float s2, int32_t i2) { return s > s2 || (s == s2 && i > i2); }

template <int KL>
struct TopList {  // sorted (score desc, local row desc); empty slots (-inf, -1); KL = capacity (8 or CHIP_MAX_TOPK): the
    float s[KL];  // lists live in registers across the whole K loop, next to 64..128 accumulator registers
    int32_t r[KL];
};

template <int KL>
__device__ __forceinline__ void list_init(TopList<KL> &L)
{
#pragma unroll
    for (int j = 0; j < KL; j++) { L.s[j] = -INFINITY; L.r[j] = -1; }
}
template <int KL>
__device__ __forceinline__ void list_push(TopList<KL> &L, int K, float s, int32_t row)
{
    // caller checked fkey_gt(s,row, L.s[K-1], L.r[K-1]); static-index insertion (no dynamic register indexing)
#pragma unroll
    for (int j = KL - 1; j >= 1; j--) {
        if (j < K) {
            const bool above = fkey_gt(s, row, L.s[j - 1], L.r[j - 1]);       // new entry belongs above slot j-1
            const bool here = fkey_gt(s, row, L.s[j], L.r[j]) && !above;       // exactly at slot j
            if (above) { L.s[j] = L.s[j - 1]; L.r[j] = L.r[j - 1]; }
            else if (here) { L.s[j] = s; L.r[j] = row; }
        }
    }
    if (fkey_gt(s, row, L.s[0], L.r[0])) { L.s[0] = s; L.r[0] = row; }
}
// the current K-th best of a list (K <= KL, run-time)
template <int KL>
__device__ __forceinline__ void list_kth(const TopList<KL> &L, int K, float &ts, int32_t &tr)
{
    ts = L.s[0]; tr = L.r[0];
#pragma unroll
    for (int j = 1; j < KL; j++)
        if (j < K) { ts = L.s[j]; tr = L.r[j]; }
}

// LDS-DMA tile staging (cdna_hip_programming.md 3, rule 21): global_load_lds_dwordx4 copies 16 bytes per lane straight from
// global memory to LDS at (wave-uniform base + lane * 16) -- no staging VGPRs, no ds_write pass.  The MFMA loop must also be
// free of VALU work: measured on this chip (scripts/probes/mfma_probe.hip, one wave per SIMD) a v_mfma_f32_32x32x2_f32 stream
// runs at 0.96 of peak with its fragments read as plain ds_read_b32, but at 0.80 when every operand needs one v_cndmask (16-B
// fragment reads + select) -- VALU instructions do not hide under this MFMA.  So both LDS images are laid out such that a lane
// reads exactly the floats it feeds to the matrix core:
//   A (queries)  : the host side keeps a K-CHUNK-MAJOR, TRANSPOSED image of the query tile in global memory
//                  (Qt[qtile][chunk][k 0..31][row 0..127], written once per call by transpose_queries), so the DMA is a linear
//                  16 KiB copy per chunk and lane (fr, fk) reads A[R + fr][2 kk + fk] at float (2 kk + fk) * 128 + R + fr:
//                  32 consecutive floats per half-wave -- conflict-free ds_read_b32, two k-steps per ds_read2st64_b32.
//   B (DB rows)  : row-major in global memory (fixed): per stage 16 blocks of [8 rows][8 slots of 16 B], one LDS-DMA
//                  instruction each (the destination is lane-linear), slots XOR-swizzled on both sides (slot p of row r holds
//                  floats [4 k4, 4 k4 + 4) with k4 = p ^ (r & 7): the loader picks its SOURCE address accordingly) and block
//                  b ROTATED by b & 3 floats (b_row_off).  Lane (fr, fk) reads floats [fk] and [2 + fk] of its row's slot with
//                  ONE ds_read2_b32; the 32 rows of a half-wave are 4 blocks x 8 rows = 4 rotations x 8 swizzled slots = 32
//                  distinct banks.  (Without the rotation a column read over 128-B rows is 4-way bank-conflicted whatever the
//                  slot swizzle -- 32 rows, 8 slots, one float offset: round 2 ran that way until the probe showed the
//                  destination base of an LDS-DMA may be any multiple of 4 bytes.)
// The LDS-DMA is issued from inline asm ON PURPOSE: hipcc tracks the builtin form and, not knowing which stage a load fills,
// drains ALL of them (s_waitcnt vmcnt(0)) at every barrier.  Untracked, the loads of the next chunk stay in flight
// underneath this chunk's MFMAs and the loop waits for them itself, once, at the barrier that ends the chunk.
// M0 (the wave-uniform LDS destination base) is written in the same statement that uses it (cdna_hip_programming.md, asm notes).
__device__ __forceinline__ void glds16(const float *gsrc, uint32_t lds_byte_addr_wave_uniform)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_byte_addr_wave_uniform)
                 : "memory");
}
// the same load addressed as wave-uniform base + 32-bit byte offset per lane (the prefix forms: no 64-bit pointer per lane and load)
__device__ __forceinline__ void glds16_s(const void *base_wave_uniform, uint32_t byte_off, uint32_t lds_byte_addr_wave_uniform)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(byte_off), "s"(base_wave_uniform), "s"(lds_byte_addr_wave_uniform)
                 : "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
// every LDS-DMA load has landed, own LDS reads done, workgroup barrier
__device__ __forceinline__ void wait_loads_and_barrier()
{
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// the lane number, read anew where it is called (the prefix forms: see db_gemm_body.inc)
__device__ __forceinline__ int lane_now()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// Double rows (chip_query_batch_cast_f32): the B side of the same LDS image, filled through registers.  The reference's faiss variants
// index X.cast<float>() of its MatrixXd DB (Cerebro.cpp:422,569,807), so a double-row DB enters this GEMM as (float)x per element
// (v_cvt_f32_f64, round to nearest even) and everything behind the loader -- image, fragment reads, MFMA order, epilogue -- is the float
// kernel's, hence the same fmaf chain.  LDS-DMA cannot convert, and a raw double tile (64 KiB per stage at 256 rows) does not fit
// beside the A ring, so a thread loads the 32 source bytes of each 16-byte slot its lane's DMA would have filled (2 x
// global_load_dwordx4), converts and stores the slot.  The slot's address is lane-linear in a block ROTATED by (wave & 3) floats:
// 16-byte aligned on waves 0 and 4 only, 8-byte on rotation 2, 4-byte on the odd ones -- and a DS access wider than 4 bytes off its
// natural alignment is replayed (tens of cycles per wave instruction).  The rotation is wave-uniform, so a scalar branch picks
// the widest store the wave's rotation allows: one ds_write_b128, two ds_write_b64, or two ds_write2_b32 (each 12-13 LDS cycles
// per wave instruction; no replay).
template <int ALIGN>
__device__ __forceinline__ void lds_store_slot(float *d, float x, float y, float z, float w)
{
    if constexpr (ALIGN == 16) {
        *reinterpret_cast<f32x4 *>(__builtin_assume_aligned(d, 16)) = f32x4{x, y, z, w};
    } else if constexpr (ALIGN == 8) {
        f32x2 *d2 = reinterpret_cast<f32x2 *>(__builtin_assume_aligned(d, 8));
        d2[0] = f32x2{x, y};
        d2[1] = f32x2{z, w};
    } else {
        d[0] = x; d[1] = y; d[2] = z; d[3] = w;
    }
}

// Qt[qtile][chunk][k][row] <- Q[qtile * TM + row][chunk * KC + k], TM = rows of a query tile (128 or 256)
// (one thread per element; Q is a few MB at most)
__global__ __launch_bounds__(256) void transpose_queries(const float *__restrict__ Q, float *__restrict__ Qt, int Qpad, int D, int tm_shift)
{
    constexpr int KC = 32;
    const int64_t n = (int64_t)Qpad * D;
    const int TM = 1 << tm_shift;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int row = (int)(i & (TM - 1));
        const int k = (int)((i >> tm_shift) & (KC - 1));
        const int64_t t = i >> (tm_shift + 5);           // (qtile, chunk) flattened: chunk fastest
        const int chunk = (int)(t % (D / KC)), qt = (int)(t / (D / KC));
        Qt[i] = Q[(int64_t)(qt * TM + row) * D + chunk * KC + k];
    }
}

// The same image made on the device from DB rows (chip_query_batch_rows_f32: the queries of a causal self-join ARE rows of the DB):
// Qt[qtile][chunk][k][q] <- row rows[qtile * TM + q], elements [chunk * 32 + k], straight through the segment table -- no Q image, no
// memset, no second launch.  One workgroup per (chunk, query tile): a row's 32 elements of the chunk are read as whole 16-byte vectors
// along D (8 per float row, 16 per double row), turned through LDS, and written out TM floats per k (coalesced).  Double rows are
// narrowed with v_cvt_f32_f64, the cast loader's own conversion, so a query row and a DB row round alike.  rows[q] < 0: a padded
// query, written as zeros.
struct GatherArgs {
    const void *const *seg_table;
    int32_t seg_shift;
    int64_t seg_mask;
    int32_t D;
    const int64_t *rows;    // [Qpad] local rows, -1 for padded queries
    float *Qt;
};
template <typename ROW, int TM>
__global__ __launch_bounds__(256) void gather_query_tiles(GatherArgs g)
{
    constexpr int KC = 32;
    constexpr bool DBL = std::is_same<ROW, double>::value;
    static_assert(DBL || std::is_same<ROW, float>::value, "float or double rows");
    constexpr int VPR = DBL ? 16 : 8;    // 16-byte vectors per row and chunk
    constexpr int EPV = KC / VPR;        // elements per vector
    __shared__ float T[KC][TM + 1];
    const int chunk = blockIdx.x, qt = blockIdx.y, n_chunks = g.D / KC;
    for (int i = threadIdx.x; i < TM * VPR; i += 256) {
        const int q = i / VPR, v = i % VPR;
        const int64_t r = g.rows[(int64_t)qt * TM + q];
        float x[EPV];
#pragma unroll
        for (int e = 0; e < EPV; e++) x[e] = 0.0f;
        if (r >= 0) {
            const ROW *src = reinterpret_cast<const ROW *const *>(g.seg_table)[r >> g.seg_shift] + (r & g.seg_mask) * (int64_t)g.D + chunk * KC + v * EPV;
            if constexpr (DBL) {
                const f64x2 d = *reinterpret_cast<const f64x2 *>(src);
                x[0] = (float)d[0]; x[1] = (float)d[1];
            } else {
                const f32x4 f = *reinterpret_cast<const f32x4 *>(src);
                x[0] = f[0]; x[1] = f[1]; x[2] = f[2]; x[3] = f[3];
            }
        }
#pragma unroll
        for (int e = 0; e < EPV; e++) T[v * EPV + e][q] = x[e];
    }
    __syncthreads();
    float *dst = g.Qt + ((int64_t)qt * n_chunks + chunk) * (KC * TM);
    for (int i = threadIdx.x; i < KC * TM; i += 256) dst[i] = T[i / TM][i % TM];
}

// WN = waves along the DB rows of a tile (2 or 4); a wave owns WN x 2 MFMA 32x32 blocks (64 WN queries x 64 DB rows), the
// workgroup tile is 64 WN x 64 WN (128 x 128 with 4 waves, 256 x 256 with 8), 2 x WN waves, 8 LDS-DMA per wave per chunk either way.
// ROW = float: DB rows by LDS-DMA; ROW = double: rows narrowed to float on their way into the same image (see above).
//
// The body is stated once, for two kernels.  db_gemm_topk (PREFIX = false) scans rows [0, a.n_rows) for every query.  db_gemm_prefixed
// (PREFIX = true: chip_query_batch_rows_f32 / chip_query_batch_prefix_f32) gives every query a prefix of its own: the tile walk of a query
// tile ends at lim.tile_limit[blockIdx.y], the largest limit among its queries (0: nothing is walked, the lists stay empty), and the
// epilogue clips the columns a thread scans by its own query's lim.q_limit.  The K loop, the staging and the lists do not know.
struct PrefixLimits {
    const int32_t *q_limit;      // [Qpad] local row limit of each query (0 for padded queries)
    const int32_t *tile_limit;   // [query tiles] max of q_limit over the tile
    uint32_t *done;              // [query tiles] work done, in half tiles (zeroed before the launch): what the kernel really walked
};
struct PrefixArgs {
    BatchArgs b;
    PrefixLimits lim;
};
template <int KC, int WN, int KL, typename ROW>
__global__ __launch_bounds__(128 * WN) void db_gemm_topk(BatchArgs a)
{
    constexpr bool PREFIX = false;
    const PrefixLimits lim{};   // (never read)
#include "db_gemm_body.inc"
}
template <int KC, int WN, int KL, typename ROW>
__global__ __launch_bounds__(128 * WN) void db_gemm_prefixed(PrefixArgs pa)
{
    constexpr bool PREFIX = true;
    const BatchArgs &a = pa.b;
    const PrefixLimits lim = pa.lim;
#include "db_gemm_body.inc"
}

// one workgroup per 4 queries: merge the P partition lists
struct BatchMergeArgs {
    const chip_topk_entry *in;  // [P][Qpad][K]
    int32_t n_lists, Qpad, K;
    chip_topk_entry *out;       // [Qpad][K]
};
__global__ __launch_bounds__(512) void topk_merge_batch(BatchMergeArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[kMergeSmem];
    merge_sorted_lists<4>(a.in, a.n_lists, a.Qpad, 4 * (int)blockIdx.x, a.K, a.out + (int64_t)4 * blockIdx.x * a.K, nullptr, 0, 0, 0.0, smem);
}

struct BatchState {
    DevBuf<float> Q, Qt;
    DevBuf<uint32_t> tile_ctr;        // one counter per query tile (kMaxQTiles)
    DevBuf<chip_topk_entry> partial, out;
    PinnedBuf<chip_topk_entry> h_out;
    // sharded DBs (chip_multi.hip): every shard's [Qpad][K] list side by side, and the merged result of the whole DB
    DevBuf<chip_topk_entry> gathered, merged;
    // chip_debug_merge_lists: the caller's lists, the merged lists, the record
    DevBuf<chip_topk_entry> dbg_in, dbg_out;
    DevBuf<chip_tick_result> dbg_rec;
    // prefix calls (query_batch_prefix): a group's query rows and limits (built in pinned memory, one upload), the sorted host vectors of
    // a group, the kernel's work counters and their copy, what the last call did
    PinnedBuf<char> h_prefix_in;
    DevBuf<char> prefix_in;
    PinnedBuf<float> h_q;
    DevBuf<uint32_t> prefix_done;
    PinnedBuf<uint32_t> h_prefix_done;
    chip_query_prefix_last prefix_last = {};
    // chip_loop_ticks_bulk: a group's records, exact lists and words (one block, one copy back), the record of an exact rerun (pinned), what
    // the last call did
    DevBuf<char> bulk_out;
    PinnedBuf<char> h_bulk_out;
    PinnedBuf<chip_tick_result> bulk_rec;
    chip_bulk_ticks_last bulk_last = {};
    hipEvent_t ev_done = nullptr;    // this shard's list is complete (recorded on its scan stream)
};

void batch_destroy(Ctx *c)
{
    BatchState *st = c->batch_state;
    if (!st) return;
    if (st->ev_done) (void)hipEventDestroy(st->ev_done);
    delete st;
    c->batch_state = nullptr;
}

int32_t batch_qpad(int32_t Q) { return (Q + BM - 1) / BM * BM; }
// the tile shape rule of both modes (see batch_local_enqueue)
static bool batch_wide(int32_t Qpad, int elem, int topk) { return Qpad % 256 == 0 && !(elem == 8 && topk > 8); }

// This ctx's share of a many-query call, enqueued on its scan stream: Q queries (host, Q x D fp32) against its LOCAL rows of the global
// prefix [0, k) -- the whole prefix on a plain ctx, rows i % G == rank of it on a shard -- leaving one sorted [Qpad][topk] list of
// (score, GLOBAL index) entries in device memory (*out_dev).  No host synchronisation.  Caller: query lock held, device current.
// The ctx's storage type picks the kernel: float rows by LDS-DMA, double rows narrowed to float in the loader -- the caller has
// checked that its entry point allows that (chip_query_batch_cast_f32).
int batch_local_enqueue(Ctx *c, int64_t k, const float *queries, int32_t Q, int32_t topk, chip_topk_entry **out_dev, int32_t *Qpad_out)
{
    if (!c->batch_state) {
        c->batch_state = new (std::nothrow) BatchState();
        if (!c->batch_state) return CHIP_ERR_OOM;
    }
    BatchState *st = c->batch_state;
    ResidentPause paused(c);   // the many-query scan fills every CU (and may free / allocate): no resident scan instance until it returns
    const int D = c->D;
    const int Qpad = batch_qpad(Q);
    const int64_t n_rows = local_count(c, k);
    // Tile shape: 256 x 256 with 8 waves (one workgroup per CU: 16 MFMAs per 6 fragment reads, one barrier per 128 MFMAs, the DB
    // streamed once per 256 queries) when the padded query count is a multiple of 256, else 128 x 128 with 4 waves.
    // Double rows with the long lists (topk > 8) keep to the small tile: next to 128 accumulator registers, 32 list registers and
    // the staging of the cast loader the 256 x 256 form does not fit 256 registers per wave (it would spill inside the tile loop).
    const bool wide = batch_wide(Qpad, c->elem, topk);
    const int TM = wide ? 256 : BM, TN = TM;
    const int qtiles = Qpad / TM;
    const int wgs = wide ? 1 : 2;            // workgroups per CU
    int64_t tiles = (n_rows + TN - 1) / TN;
    if (tiles < 1) tiles = 1;
    int64_t P = (wgs * (int64_t)c->n_cus + qtiles - 1) / qtiles;   // workgroups per query tile (each ends with one list per query): at most 512
    if (P > tiles) P = tiles;
    if (P > 512) P = 512;
    const int cap_wgs = env_int("CHIP_BATCH_WGS", 0);   // diagnosis / tests: fewer workgroups, i.e. many claimed tiles each
    if (cap_wgs > 0 && P > cap_wgs) P = cap_wgs;
    if (P < 1) P = 1;

    hipStream_t s = c->s_scan;
    int rc = st->Q.reserve(c, (size_t)Qpad * D);
    if (rc == CHIP_OK) rc = st->Qt.reserve(c, (size_t)Qpad * D);
    if (rc == CHIP_OK) rc = st->partial.reserve(c, (size_t)(P * Qpad * topk));
    if (rc == CHIP_OK) rc = st->out.reserve(c, (size_t)Qpad * topk);
    if (rc == CHIP_OK) rc = st->h_out.reserve(c, (size_t)Qpad * topk);
    if (rc == CHIP_OK) rc = st->tile_ctr.reserve(c, kMaxQTiles);
    if (rc != CHIP_OK) return rc;
    if (qtiles > kMaxQTiles) return CHIP_ERR_UNSUPPORTED;
    CHIP_HIP(c, hipMemsetAsync(st->tile_ctr, 0, sizeof(uint32_t) * kMaxQTiles, s));
    CHIP_HIP(c, hipMemsetAsync(st->Q, 0, sizeof(float) * (size_t)Qpad * D, s));
    CHIP_HIP(c, hipMemcpyAsync(st->Q, queries, sizeof(float) * (size_t)Q * D, hipMemcpyHostToDevice, s));
    {   // K-chunk-major transposed image of the query tiles (what the A-side LDS-DMA copies linearly)
        int64_t g = ((int64_t)Qpad * D + 255) / 256;
        if (g > (int64_t)c->n_cus * 8) g = (int64_t)c->n_cus * 8;
        hipLaunchKernelGGL(transpose_queries, dim3((unsigned)g), dim3(256), 0, s, st->Q, st->Qt, Qpad, D, wide ? 8 : 7);
        CHIP_HIP(c, hipGetLastError());
    }

    BatchArgs a;
    a.seg_table = reinterpret_cast<const void *const *>(c->seg_table_dev.get()); a.seg_shift = c->seg_shift; a.seg_mask = c->seg_rows - 1;
    a.n_rows = n_rows; a.D = D; a.Q = st->Q; a.Qt = st->Qt; a.Qpad = Qpad; a.K = topk; a.tile_ctr = st->tile_ctr;
    a.idx_mul = c->nranks; a.idx_add = c->nranks == 1 ? 0 : c->rank; a.partial = st->partial;
    constexpr int KCsel = 32;
    const size_t lds_gemm = sizeof(float) * NST * ((size_t)TM * KCsel + (size_t)(TN / 8) * kBBlock) /* stages x (A + B) */;
    const size_t lds_ct = sizeof(float) * (size_t)TM * CT_LD;
    const size_t lds = lds_gemm > lds_ct ? lds_gemm : lds_ct;
    hipEvent_t e1 = nullptr;
    if (c->prof_on) {
        const int prc = prof_begin(c, s, (double)n_rows * D * c->elem * qtiles, &e1);   // the DB is streamed once per query tile
        if (prc != CHIP_OK) return prc;
    }
    auto launch = [&](auto kernel, int threads) -> int {
        CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)P, (unsigned)qtiles), dim3(threads), lds, s, a);
        return CHIP_OK;
    };
    int lrc;
    if (c->elem == 8) {
        if (c->seg_rows % TN != 0) return CHIP_ERR_UNSUPPORTED;   // the cast loader addresses a tile within ONE segment (never the case: segments are >= 8192 rows)
        if (topk <= 8) lrc = wide ? launch(db_gemm_topk<KCsel, 4, 8, double>, 512) : launch(db_gemm_topk<KCsel, 2, 8, double>, 256);
        else lrc = launch(db_gemm_topk<KCsel, 2, CHIP_MAX_TOPK, double>, 256);
    } else if (topk <= 8) lrc = wide ? launch(db_gemm_topk<KCsel, 4, 8, float>, 512) : launch(db_gemm_topk<KCsel, 2, 8, float>, 256);
    else lrc = wide ? launch(db_gemm_topk<KCsel, 4, CHIP_MAX_TOPK, float>, 512) : launch(db_gemm_topk<KCsel, 2, CHIP_MAX_TOPK, float>, 256);
    if (lrc != CHIP_OK) return lrc;
    CHIP_HIP(c, hipGetLastError());
    if (e1) CHIP_HIP(c, hipEventRecord(e1, s));
    BatchMergeArgs m;
    m.in = st->partial; m.n_lists = (int)P; m.Qpad = Qpad; m.K = topk; m.out = st->out;
    hipLaunchKernelGGL(topk_merge_batch, dim3((Q + 3) / 4), dim3(512), 0, s, m);
    CHIP_HIP(c, hipGetLastError());
    *out_dev = st->out;
    *Qpad_out = Qpad;
    return CHIP_OK;
}

// D2H of a finished [Q][topk] list on the ctx's scan stream + conversion to the caller's arrays (synchronises that stream)
int batch_deliver(Ctx *c, const chip_topk_entry *list_dev, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    chip_topk_entry *const h_out = c->batch_state->h_out.host();
    hipStream_t s = c->s_scan;
    CHIP_HIP(c, hipMemcpyAsync(h_out, list_dev, sizeof(chip_topk_entry) * (size_t)Q * topk, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    if (h_out[0].idx == kFailedShardIdx) return CHIP_ERR_SHARD_FAILED;   // a shard took part with the failure mark (chip_multi.hip)
    for (int64_t i = 0; i < (int64_t)Q * topk; i++) {
        if (scores) scores[i] = (float)h_out[i].score;
        if (idx) idx[i] = h_out[i].idx;
    }
    return CHIP_OK;
}

// ---- a prefix per query (chip_query_batch_rows_f32, chip_query_batch_prefix_f32 and their cast forms)
// The walk order of a call: the queries stable-sorted by k ascending, so that the queries of a tile have limits close to each other
// and the tile walk of a query tile ends at the largest of them.
// (No exception leaves through the C ABI: an allocation that fails is CHIP_ERR_OOM.)
static int prefix_order(const int64_t *k, int32_t Q, std::vector<int32_t> &order)
{
    try {
        order.resize((size_t)Q);
        for (int32_t i = 0; i < Q; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [k](int32_t x, int32_t y) { return k[x] < k[y]; });
    } catch (const std::bad_alloc &) {
        return CHIP_ERR_OOM;
    }
    return CHIP_OK;
}
// One group of the sorted list, queries [first, first + count): its padding and tile shape by the rule of chip_query_batch_f32, and per
// query tile the largest limit -- the last real query's, the list being sorted (tile_limit, qtiles entries, may be NULL).  The ONE
// place that decides them: the call and chip_query_prefix_plan both come here.
struct PrefixGroup {
    int32_t first, count, Qpad, TM, qtiles;
    int64_t units;   // DB tiles the group walks: sum over its query tiles of ceil(tile limit / TM)
};
static PrefixGroup prefix_group(const int64_t *k, const int32_t *order, int32_t first, int32_t count, int elem, int topk, int32_t *tile_limit)
{
    PrefixGroup g;
    g.first = first; g.count = count; g.Qpad = batch_qpad(count);
    g.TM = batch_wide(g.Qpad, elem, topk) ? 256 : BM;
    g.qtiles = g.Qpad / g.TM;
    g.units = 0;
    for (int32_t t = 0; t < g.qtiles; t++) {
        const int32_t end = (t + 1) * g.TM < count ? (t + 1) * g.TM : count;   // (every tile holds a real query: Qpad - count < 128 <= TM)
        const int64_t lim = k[order[first + end - 1]];
        if (tile_limit) tile_limit[t] = (int32_t)lim;
        g.units += (lim + g.TM - 1) / g.TM;
    }
    return g;
}

static void prefix_plan(const int64_t *k, int32_t Q, int elem, int topk, const int32_t *order, chip_query_prefix_plan_out *f)
{
    f->group_size = CHIP_QUERY_PREFIX_GROUP; f->groups = 0; f->tile_full = 0; f->tile_last = 0;
    f->qtiles = 0; f->units = 0; f->units_rect = 0;
    const int64_t kmax = k[order[Q - 1]];
    for (int32_t first = 0; first < Q; first += CHIP_QUERY_PREFIX_GROUP) {
        const int32_t count = Q - first < CHIP_QUERY_PREFIX_GROUP ? Q - first : CHIP_QUERY_PREFIX_GROUP;
        const PrefixGroup g = prefix_group(k, order, first, count, elem, topk, nullptr);
        f->groups++;
        if (count == CHIP_QUERY_PREFIX_GROUP) f->tile_full = g.TM;
        f->tile_last = g.TM;
        f->qtiles += g.qtiles;
        f->units += g.units;
        f->units_rect += g.qtiles * ((kmax + g.TM - 1) / g.TM);
    }
}

// One group of a prefix call enqueued on the ctx's scan stream: one gather launch (or memset + upload + transpose_queries for host vectors),
// one GEMM launch, one merge launch -- the group's sorted [Qpad][topk] lists are then in st->out on the device, its input image (int64
// rows[Qpad] | int32 q_limit[Qpad] | int32 tile_limit[qtiles]) in st->prefix_in, the kernel's work counters in st->prefix_done.  No host
// wait.  Caller: arguments checked, query lock held, device current, resident scan paused.  query_rows (or, where NULL, queries): the
// caller's rows or vectors, in the CALLER's order.
static int prefix_group_enqueue(Ctx *c, BatchState *st, const PrefixGroup &g, const int32_t *tile_limit, const int64_t *k, const int32_t *order,
                                const int64_t *query_rows, const float *queries, int32_t topk)
{
    const int D = c->D, Qpad = g.Qpad, TM = g.TM, TN = TM, qtiles = g.qtiles;
    const bool wide = TM == 256, from_rows = query_rows != nullptr;
    // the group's input image: int64 rows[Qpad] | int32 q_limit[Qpad] | int32 tile_limit[qtiles]
    const size_t in_bytes = (size_t)Qpad * 12 + (size_t)qtiles * 4;
    int rc = st->h_prefix_in.reserve(c, in_bytes);
    if (rc == CHIP_OK) rc = st->prefix_in.reserve(c, in_bytes);
    if (rc == CHIP_OK) rc = st->Qt.reserve(c, (size_t)Qpad * D);
    if (rc == CHIP_OK && !from_rows) rc = st->Q.reserve(c, (size_t)Qpad * D);
    if (rc == CHIP_OK && !from_rows) rc = st->h_q.reserve(c, (size_t)g.count * D);
    if (rc == CHIP_OK) rc = st->tile_ctr.reserve(c, kMaxQTiles);
    if (rc == CHIP_OK) rc = st->prefix_done.reserve(c, kMaxQTiles);
    if (rc == CHIP_OK) rc = st->h_prefix_done.reserve(c, kMaxQTiles);
    if (rc != CHIP_OK) return rc;
    int64_t *const h_rows = reinterpret_cast<int64_t *>(st->h_prefix_in.host());
    int32_t *const h_qlim = reinterpret_cast<int32_t *>(h_rows + Qpad), *const h_tlim = h_qlim + Qpad;
    for (int32_t i = 0; i < Qpad; i++) {
        const bool real = i < g.count;
        const int32_t j = real ? order[g.first + i] : 0;
        h_rows[i] = real && from_rows ? query_rows[j] : -1;      // (a plain ctx: local row = global row)
        h_qlim[i] = real ? (int32_t)k[j] : 0;                    // padded queries: limit 0
    }
    memcpy(h_tlim, tile_limit, sizeof(int32_t) * (size_t)qtiles);
    int64_t tiles = (h_tlim[qtiles - 1] + TN - 1) / TN;          // of the group's largest prefix
    if (tiles < 1) tiles = 1;
    // workgroups per query tile, as batch_local_enqueue sizes them
    int64_t P = ((wide ? 1 : 2) * (int64_t)c->n_cus + qtiles - 1) / qtiles;
    if (P > tiles) P = tiles;
    if (P > 512) P = 512;
    const int cap_wgs = env_int("CHIP_BATCH_WGS", 0);
    if (cap_wgs > 0 && P > cap_wgs) P = cap_wgs;
    if (P < 1) P = 1;
    rc = st->partial.reserve(c, (size_t)(P * Qpad * topk));
    if (rc == CHIP_OK) rc = st->out.reserve(c, (size_t)Qpad * topk);
    if (rc == CHIP_OK) rc = st->h_out.reserve(c, (size_t)Qpad * topk);
    if (rc != CHIP_OK) return rc;

    hipStream_t s = c->s_scan;
    char *const in_dev = st->prefix_in;
    CHIP_HIP(c, hipMemcpyAsync(in_dev, st->h_prefix_in.host(), in_bytes, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemsetAsync(st->tile_ctr, 0, sizeof(uint32_t) * qtiles, s));
    CHIP_HIP(c, hipMemsetAsync(st->prefix_done, 0, sizeof(uint32_t) * qtiles, s));
    const void *const *seg_table = reinterpret_cast<const void *const *>(c->seg_table_dev.get());
    if (from_rows) {
        GatherArgs ga;
        ga.seg_table = seg_table; ga.seg_shift = c->seg_shift; ga.seg_mask = c->seg_rows - 1; ga.D = D;
        ga.rows = reinterpret_cast<const int64_t *>(in_dev); ga.Qt = st->Qt;
        const dim3 grid((unsigned)(D / 32), (unsigned)qtiles);
        if (c->elem == 8) {
            if (wide) hipLaunchKernelGGL((gather_query_tiles<double, 256>), grid, dim3(256), 0, s, ga);
            else hipLaunchKernelGGL((gather_query_tiles<double, 128>), grid, dim3(256), 0, s, ga);
        } else {
            if (wide) hipLaunchKernelGGL((gather_query_tiles<float, 256>), grid, dim3(256), 0, s, ga);
            else hipLaunchKernelGGL((gather_query_tiles<float, 128>), grid, dim3(256), 0, s, ga);
        }
        CHIP_HIP(c, hipGetLastError());
    } else {
        float *const h_q = st->h_q.host();
        for (int32_t i = 0; i < g.count; i++) memcpy(h_q + (size_t)i * D, queries + (size_t)order[g.first + i] * D, sizeof(float) * (size_t)D);
        if (Qpad > g.count) CHIP_HIP(c, hipMemsetAsync(st->Q + (size_t)g.count * D, 0, sizeof(float) * (size_t)(Qpad - g.count) * D, s));
        CHIP_HIP(c, hipMemcpyAsync(st->Q, h_q, sizeof(float) * (size_t)g.count * D, hipMemcpyHostToDevice, s));
        int64_t blocks = ((int64_t)Qpad * D + 255) / 256;
        if (blocks > (int64_t)c->n_cus * 8) blocks = (int64_t)c->n_cus * 8;
        hipLaunchKernelGGL(transpose_queries, dim3((unsigned)blocks), dim3(256), 0, s, st->Q, st->Qt, Qpad, D, wide ? 8 : 7);
        CHIP_HIP(c, hipGetLastError());
    }

    PrefixArgs a;
    a.b.seg_table = seg_table; a.b.seg_shift = c->seg_shift; a.b.seg_mask = c->seg_rows - 1;
    a.b.n_rows = 0 /* unused: the limits say */; a.b.D = D; a.b.Q = nullptr; a.b.Qt = st->Qt; a.b.Qpad = Qpad; a.b.K = topk; a.b.tile_ctr = st->tile_ctr;
    a.b.idx_mul = 1; a.b.idx_add = 0; a.b.partial = st->partial;
    a.lim.q_limit = reinterpret_cast<const int32_t *>(in_dev + (size_t)Qpad * 8);
    a.lim.tile_limit = a.lim.q_limit + Qpad;
    a.lim.done = st->prefix_done;
    const size_t lds_gemm = sizeof(float) * NST * ((size_t)TM * 32 + (size_t)(TN / 8) * kBBlock);
    const size_t lds_ct = sizeof(float) * (size_t)TM * CT_LD;
    const size_t lds = lds_gemm > lds_ct ? lds_gemm : lds_ct;
    auto launch = [&](auto kernel, int threads) -> int {
        CHIP_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)P, (unsigned)qtiles), dim3(threads), lds, s, a);
        return CHIP_OK;
    };
    int lrc;
    if (c->elem == 8) {
        if (topk <= 8) lrc = wide ? launch(db_gemm_prefixed<32, 4, 8, double>, 512) : launch(db_gemm_prefixed<32, 2, 8, double>, 256);
        else lrc = launch(db_gemm_prefixed<32, 2, CHIP_MAX_TOPK, double>, 256);   // (batch_wide: never the wide tile)
    } else if (topk <= 8) lrc = wide ? launch(db_gemm_prefixed<32, 4, 8, float>, 512) : launch(db_gemm_prefixed<32, 2, 8, float>, 256);
    else lrc = wide ? launch(db_gemm_prefixed<32, 4, CHIP_MAX_TOPK, float>, 512) : launch(db_gemm_prefixed<32, 2, CHIP_MAX_TOPK, float>, 256);
    if (lrc != CHIP_OK) return lrc;
    CHIP_HIP(c, hipGetLastError());
    BatchMergeArgs m;
    m.in = st->partial; m.n_lists = (int)P; m.Qpad = Qpad; m.K = topk; m.out = st->out;
    hipLaunchKernelGGL(topk_merge_batch, dim3((g.count + 3) / 4), dim3(512), 0, s, m);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// The same group to the caller's arrays: prefix_group_enqueue, one copy back, one host wait.
static int prefix_group_run(Ctx *c, BatchState *st, const PrefixGroup &g, const int32_t *tile_limit, const int64_t *k, const int32_t *order,
                            const int64_t *query_rows, const float *queries, int32_t topk, float *scores, int64_t *idx)
{
    const int rc = prefix_group_enqueue(c, st, g, tile_limit, k, order, query_rows, queries, topk);
    if (rc != CHIP_OK) return rc;
    const int qtiles = g.qtiles;
    hipStream_t s = c->s_scan;
    chip_topk_entry *const h_out = st->h_out.host();
    uint32_t *const h_done = st->h_prefix_done.host();
    CHIP_HIP(c, hipMemcpyAsync(h_out, st->out, sizeof(chip_topk_entry) * (size_t)g.count * topk, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipMemcpyAsync(h_done, st->prefix_done, sizeof(uint32_t) * qtiles, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    for (int32_t i = 0; i < g.count; i++) {
        const size_t to = (size_t)order[g.first + i] * topk, from = (size_t)i * topk;
        for (int32_t j = 0; j < topk; j++) {
            scores[to + j] = (float)h_out[from + j].score;
            idx[to + j] = h_out[from + j].idx;
        }
    }
    chip_query_prefix_last &last = st->prefix_last;
    last.groups++; last.launches += 3; last.waits++;
    last.units_planned += g.units;
    int64_t half_tiles = 0;                                   // the kernel counts half tiles (a query half of a tile is a unit of its own;
    for (int32_t t = 0; t < qtiles; t++) half_tiles += h_done[t];   // both halves of a tile are walked: the sum of a query tile is even)
    last.units_claimed += half_tiles / 2;
    return CHIP_OK;
}

// buffers of the cross-shard merge on the ctx that merges: gathered [n_lists][Qpad][topk], merged [Qpad][topk]
int batch_exchange_buffers(Ctx *c, int n_lists, int32_t Qpad, int32_t topk, chip_topk_entry **gathered, chip_topk_entry **merged, hipEvent_t *ev_done)
{
    if (!c->batch_state) {
        c->batch_state = new (std::nothrow) BatchState();
        if (!c->batch_state) return CHIP_ERR_OOM;
    }
    BatchState *st = c->batch_state;
    int rc = st->gathered.reserve(c, (size_t)n_lists * Qpad * topk);
    if (rc == CHIP_OK) rc = st->merged.reserve(c, (size_t)Qpad * topk);
    if (rc != CHIP_OK) return rc;
    if (!st->ev_done) CHIP_HIP(c, hipEventCreateWithFlags(&st->ev_done, hipEventDisableTiming));
    if (gathered) *gathered = st->gathered;
    if (merged) *merged = st->merged;
    if (ev_done) *ev_done = st->ev_done;
    return CHIP_OK;
}

// merge of n_lists per-shard lists [n_lists][Qpad][topk] -> out [Qpad][topk] on stream s (the same exact selection as within a device)
int batch_merge_lists(Ctx *c, hipStream_t s, const chip_topk_entry *in, int n_lists, int32_t Qpad, int32_t Q, int32_t topk, chip_topk_entry *out)
{
    BatchMergeArgs m;
    m.in = in; m.n_lists = n_lists; m.Qpad = Qpad; m.K = topk; m.out = out;
    hipLaunchKernelGGL(topk_merge_batch, dim3((Q + 3) / 4), dim3(512), 0, s, m);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// chip_debug_merge_lists: host lists [n_lists][nq][K] through the merge kernel of `form` exactly as the product paths launch it (launch_merge
// for topk_merge<nq>, batch_merge_lists for topk_merge_batch with Qpad = Q = nq), result to the host.  Caller: arguments checked, query lock
// held, device current.  `out` and the record are filled with a byte pattern first, so that an entry the kernel does not write is no entry at all.
int debug_merge_lists(Ctx *c, int form, const chip_topk_entry *lists, int32_t n_lists, int32_t nq, int32_t K, chip_topk_entry *out, int64_t l,
                      const chip_dot_params *p, chip_tick_result *result)
{
    if (!c->batch_state) {
        c->batch_state = new (std::nothrow) BatchState();
        if (!c->batch_state) return CHIP_ERR_OOM;
    }
    BatchState *st = c->batch_state;
    const size_t n_in = (size_t)n_lists * nq * K, n_out = (size_t)nq * K;
    {
        // one pause over the group: hipFree waits for the whole device, no resident scan instance on it until the last allocation is done
        ResidentPause paused(c, n_in > st->dbg_in.capacity() || n_out > st->dbg_out.capacity() || !st->dbg_rec.capacity());
        int rc = st->dbg_in.reserve(c, n_in);
        if (rc == CHIP_OK) rc = st->dbg_out.reserve(c, n_out);
        if (rc == CHIP_OK) rc = st->dbg_rec.reserve(c, 1);
        if (rc != CHIP_OK) return rc;
    }
    hipStream_t s = c->s_query;
    CHIP_HIP(c, hipMemcpyAsync(st->dbg_in, lists, sizeof(chip_topk_entry) * n_in, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemsetAsync(st->dbg_out, 0xA5, sizeof(chip_topk_entry) * n_out, s));
    CHIP_HIP(c, hipMemsetAsync(st->dbg_rec, 0xA5, sizeof(chip_tick_result), s));
    int rc;
    if (form == 0) rc = launch_merge(c, s, merge_args(st->dbg_in, n_lists, K, st->dbg_out, result ? st->dbg_rec.get() : nullptr, l, p), nq);
    else rc = batch_merge_lists(c, s, st->dbg_in, n_lists, nq, nq, K, st->dbg_out);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemcpyAsync(out, st->dbg_out, sizeof(chip_topk_entry) * n_out, hipMemcpyDeviceToHost, s));
    if (result) CHIP_HIP(c, hipMemcpyAsync(result, st->dbg_rec, sizeof(chip_tick_result), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

}  // namespace chip

using namespace chip;

// cast_rows: the caller came through chip_query_batch_cast_f32 and accepts double rows narrowed to float
static int query_batch(chip_ctx *c, int64_t k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx, bool cast_rows)
{
    if (!c || !queries || Q < 1) return CHIP_ERR_INVALID_ARG;
    if (topk < 1 || topk > CHIP_MAX_TOPK || c->D % 32 != 0) return CHIP_ERR_UNSUPPORTED;
    if ((int64_t)(Q + BM - 1) / BM > kMaxQTiles) return CHIP_ERR_UNSUPPORTED;
    if (c->group) return group_query_batch(c, k, queries, Q, topk, scores, idx, cast_rows);   // G per-device passes -> one merge on devices[0]
    if (c->elem != 4 && !cast_rows) return CHIP_ERR_UNSUPPORTED;   // fp32 GEMM over float rows; the cast of double rows (faiss: Cerebro.cpp:422) is opt-in
    int64_t n_global;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        n_global = c->rows_global;
    }
    if (k < 0) return CHIP_ERR_RANGE;
    const bool collective = c->xchg != nullptr;      // sharded ctx with an in-library exchange: every rank makes the same call
    if (k > n_global && !collective) return CHIP_ERR_RANGE;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    if (collective) return xchg_query_batch(c, k, queries, Q, topk, scores, idx, k > n_global, cast_rows);
    chip_topk_entry *out = nullptr;
    int32_t Qpad = 0;
    const int rc = batch_local_enqueue(c, k, queries, Q, topk, &out, &Qpad);
    if (rc != CHIP_OK) return rc;
    return batch_deliver(c, out, Q, topk, scores, idx);
}

extern "C" int chip_query_batch_f32(chip_ctx *c, int64_t k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    return query_batch(c, k, queries, Q, topk, scores, idx, false);
}

extern "C" int chip_query_batch_cast_f32(chip_ctx *c, int64_t k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    return query_batch(c, k, queries, Q, topk, scores, idx, true);
}

// ---- a prefix per query (header: "The same mode with a prefix PER QUERY")
static int query_batch_prefix(chip_ctx *c, const int64_t *query_rows, const float *queries, bool from_rows, const int64_t *k, int32_t Q, int32_t topk,
                              float *scores, int64_t *idx, bool cast_rows)
{
    if (!c || !k || !scores || !idx || Q < 1 || (from_rows ? !query_rows : !queries)) return CHIP_ERR_INVALID_ARG;
    if (topk < 1 || topk > CHIP_MAX_TOPK || c->D % 32 != 0) return CHIP_ERR_UNSUPPORTED;
    if (c->group || c->nranks != 1) return CHIP_ERR_UNSUPPORTED;    // a query row of a sharded DB lives on one rank only: not in this interface yet
    if (c->elem != 4 && !cast_rows) return CHIP_ERR_UNSUPPORTED;
    int64_t n_global;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        n_global = c->rows_global;
    }
    for (int32_t j = 0; j < Q; j++) {
        if (k[j] < 0 || k[j] > n_global) return CHIP_ERR_RANGE;
        if (from_rows && (query_rows[j] < 0 || query_rows[j] >= n_global)) return CHIP_ERR_RANGE;
    }
    if (n_global > INT32_MAX) return CHIP_ERR_UNSUPPORTED;          // the limits travel as int32, like the rows of a list
    // both loaders of db_gemm_prefixed address a DB tile through ONE segment base and 32-bit offsets: a tile (256 rows at most) must lie
    // within a segment, whatever the storage type (never otherwise: segments hold at least 8192 rows)
    if (c->seg_rows % 256 != 0) return CHIP_ERR_UNSUPPORTED;
    std::vector<int32_t> order;
    const int orc = prefix_order(k, Q, order);
    if (orc != CHIP_OK) return orc;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    if (!c->batch_state) {
        c->batch_state = new (std::nothrow) BatchState();
        if (!c->batch_state) return CHIP_ERR_OOM;
    }
    BatchState *st = c->batch_state;
    ResidentPause paused(c);   // as batch_local_enqueue: the scan fills every CU (and may free / allocate)
    st->prefix_last = chip_query_prefix_last{};
    int32_t tile_limit[CHIP_QUERY_PREFIX_GROUP / BM];
    for (int32_t first = 0; first < Q; first += CHIP_QUERY_PREFIX_GROUP) {
        const int32_t count = Q - first < CHIP_QUERY_PREFIX_GROUP ? Q - first : CHIP_QUERY_PREFIX_GROUP;
        const PrefixGroup g = prefix_group(k, order.data(), first, count, c->elem, topk, tile_limit);
        const int rc = prefix_group_run(c, st, g, tile_limit, k, order.data(), from_rows ? query_rows : nullptr, queries, topk, scores, idx);
        if (rc != CHIP_OK) return rc;
    }
    return CHIP_OK;
}

extern "C" int chip_build_has_query_prefix(void) { return 1; }

extern "C" int chip_query_batch_rows_f32(chip_ctx *c, const int64_t *query_rows, const int64_t *k, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    return query_batch_prefix(c, query_rows, nullptr, true, k, Q, topk, scores, idx, false);
}

extern "C" int chip_query_batch_rows_cast_f32(chip_ctx *c, const int64_t *query_rows, const int64_t *k, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    return query_batch_prefix(c, query_rows, nullptr, true, k, Q, topk, scores, idx, true);
}

extern "C" int chip_query_batch_prefix_f32(chip_ctx *c, const int64_t *k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    return query_batch_prefix(c, nullptr, queries, false, k, Q, topk, scores, idx, false);
}

extern "C" int chip_query_batch_prefix_cast_f32(chip_ctx *c, const int64_t *k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx)
{
    return query_batch_prefix(c, nullptr, queries, false, k, Q, topk, scores, idx, true);
}

// ---- bulk ticks (header: "Bulk ticks"): a many-query group over the tick queries + bulk_tick_finish (kernels.hip) = the ticks' exact records
// KL, the length of the fp32 lists the certificate works from: M is the KL-th score, up to KL rows per query are scored exactly.  Runs of
// near-identical neighbouring keyframes put several rows within 2E of the best, so the longest list the GEMM keeps (profiles/bulk_ticks.md).
#ifndef CHIP_BULK_LIST_LEN
#define CHIP_BULK_LIST_LEN CHIP_MAX_TOPK   // (8 builds the other list length the GEMM has, for the comparison in the profile note)
#endif
constexpr int kBulkListLen = CHIP_BULK_LIST_LEN;
static_assert(kBulkListLen == 8 || kBulkListLen == CHIP_MAX_TOPK, "the list lengths db_gemm_prefixed is built for");
static_assert(3 * CHIP_BULK_TICKS_GROUP <= CHIP_QUERY_PREFIX_GROUP && CHIP_BULK_TICKS_MAX_TOPK <= kBulkListLen, "a tick's queries stay in one group");

// The sequence rule: what chip_loop_tick, called for l[0], l[1], ... from the loop state last_l, would say of each tick (tick_prepare is the
// tick's own function) and the loop state afterwards.  k[t] = 0 where the tick is not scanned.
static int bulk_sequence(const int64_t *l, int32_t T, const chip_dot_params *p, int64_t last_l, int64_t n_rows, int32_t *status, int64_t *k, int64_t *last_l_out)
{
    for (int32_t t = 0; t < T; t++) {
        int32_t s = 0;
        int64_t kt = 0;
        const int rc = tick_prepare(n_rows, last_l, l[t], p, &s, &kt);
        if (rc != CHIP_OK) return rc;
        // one refusal of the bulk call's own (header): a prefix that is no prefix of the DB -- a negative lag, or a min_k below -lag -- which the
        // tick itself does not check; the many-query pass cannot walk it
        if (s == CHIP_TICK_SCANNED && (kt < 0 || kt > n_rows)) return CHIP_ERR_RANGE;
        status[t] = s;
        k[t] = s == CHIP_TICK_SCANNED ? kt : 0;
        if (s != CHIP_TICK_SKIPPED) last_l = l[t];   // :1098, and the else-branch of :1022
    }
    *last_l_out = last_l;
    return CHIP_OK;
}

// The walk order: the scanned ticks stable-sorted by k ascending.
static int bulk_order(const int32_t *status, const int64_t *k, int32_t T, std::vector<int32_t> &ticks)
{
    try {
        for (int32_t t = 0; t < T; t++)
            if (status[t] == CHIP_TICK_SCANNED) ticks.push_back(t);
        std::stable_sort(ticks.begin(), ticks.end(), [k](int32_t x, int32_t y) { return k[x] < k[y]; });
    } catch (const std::bad_alloc &) {
        return CHIP_ERR_OOM;
    }
    return CHIP_OK;
}

// One group: ticks[0 .. nt) as 3 nt queries in walk order (query 3 i + j: row l - 1 - j against [0, k)), and its shape by prefix_group.
struct BulkGroup {
    std::vector<int64_t> rows, k;
    std::vector<int32_t> ident;
    PrefixGroup g;
};
static int bulk_group(const int64_t *l, const int64_t *k, const int32_t *ticks, int32_t nt, int32_t *tile_limit, BulkGroup *b)
{
    try {
        b->rows.resize((size_t)3 * nt); b->k.resize((size_t)3 * nt); b->ident.resize((size_t)3 * nt);
    } catch (const std::bad_alloc &) {
        return CHIP_ERR_OOM;
    }
    for (int32_t i = 0; i < nt; i++)
        for (int j = 0; j < 3; j++) {
            b->rows[(size_t)3 * i + j] = l[ticks[i]] - 1 - j;
            b->k[(size_t)3 * i + j] = k[ticks[i]];
            b->ident[(size_t)3 * i + j] = 3 * i + j;
        }
    b->g = prefix_group(b->k.data(), b->ident.data(), 0, 3 * nt, 4, kBulkListLen, tile_limit);
    return CHIP_OK;
}

// A group on the device: gather + db_gemm_prefixed + topk_merge_batch with lists of KL entries, bulk_tick_finish on them, ONE copy back of
// records, exact lists and words, one host wait.  Ticks whose certificate does not hold are appended to `rerun`.
static int bulk_group_run(Ctx *c, BatchState *st, const int64_t *l, const int64_t *k, const int32_t *ticks, int32_t nt, const chip_dot_params *p,
                          int32_t topk, double E, chip_tick_result *out, double *scores, int64_t *idx, std::vector<int32_t> &rerun)
{
    int32_t tile_limit[CHIP_QUERY_PREFIX_GROUP / BM];
    BulkGroup b;
    int rc = bulk_group(l, k, ticks, nt, tile_limit, &b);
    if (rc != CHIP_OK) return rc;
    const size_t rec_bytes = sizeof(chip_tick_result) * (size_t)nt, list_bytes = sizeof(chip_topk_entry) * (size_t)nt * 3 * topk;
    const size_t bytes = rec_bytes + list_bytes + sizeof(uint32_t) * 2 * (size_t)nt;
    rc = st->bulk_out.reserve(c, bytes);
    if (rc == CHIP_OK) rc = st->h_bulk_out.reserve(c, bytes);
    if (rc == CHIP_OK) rc = prefix_group_enqueue(c, st, b.g, tile_limit, b.k.data(), b.ident.data(), b.rows.data(), nullptr, kBulkListLen);
    if (rc != CHIP_OK) return rc;
    hipStream_t s = c->s_scan;
    char *const dev = st->bulk_out;
    BulkFinishArgs a;
    a.seg_table = reinterpret_cast<const void *const *>(c->seg_table_dev.get()); a.seg_shift = c->seg_shift; a.seg_mask = c->seg_rows - 1;
    a.D = c->D; a.KL = kBulkListLen; a.K = topk;
    a.lists = st->out; a.rows = reinterpret_cast<const int64_t *>(st->prefix_in.get());
    a.E = E; a.locality = p->locality; a.thresh = p->thresh;
    a.rec = reinterpret_cast<chip_tick_result *>(dev);
    a.out = reinterpret_cast<chip_topk_entry *>(dev + rec_bytes);
    a.words = reinterpret_cast<uint32_t *>(dev + rec_bytes + list_bytes);
    rc = launch_bulk_finish(c, s, a, nt);
    if (rc != CHIP_OK) return rc;
    const char *const h = st->h_bulk_out.host();
    CHIP_HIP(c, hipMemcpyAsync(st->h_bulk_out.host(), dev, bytes, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    const chip_tick_result *const h_rec = reinterpret_cast<const chip_tick_result *>(h);
    const chip_topk_entry *const h_list = reinterpret_cast<const chip_topk_entry *>(h + rec_bytes);
    const uint32_t *const h_words = reinterpret_cast<const uint32_t *>(h + rec_bytes + list_bytes);
    chip_bulk_ticks_last &last = st->bulk_last;
    last.groups++; last.launches += 4; last.waits++;
    for (int32_t i = 0; i < nt; i++) {
        const int32_t t = ticks[i];
        last.rescored_rows += h_words[2 * i + 1];
        if (h_words[2 * i] != 1u) {
            last.uncertified++;
            try { rerun.push_back(t); } catch (const std::bad_alloc &) { return CHIP_ERR_OOM; }
            continue;
        }
        last.certified++;
        out[t] = h_rec[i];
        for (int32_t j = 0; j < 3 * topk; j++) {
            if (scores) scores[(size_t)t * 3 * topk + j] = h_list[(size_t)i * 3 * topk + j].score;
            if (idx) idx[(size_t)t * 3 * topk + j] = h_list[(size_t)i * 3 * topk + j].idx;
        }
    }
    return CHIP_OK;
}

// One tick alone through the exact path -- the scan over [0, k) with its three query rows, then the merge with the decision: what
// chip_scan_local + chip_merge_decide run, without a slot and without the loop state.
static int bulk_exact_tick(Ctx *c, BatchState *st, int64_t l, int64_t k, const chip_dot_params *p, int32_t topk, chip_tick_result *out, double *scores, int64_t *idx)
{
    const int64_t rows[3] = {l - 1, l - 2, l - 3};
    const void *q[3];
    RingGuard rg(c);
    int rc = query_row_ptrs(c, rows, 3, l, q);
    if (rc != CHIP_OK) return rc;
    ScanRequest rq;
    rq.k = k; rq.q = q; rq.nq = 3; rq.K = topk; rq.out = c->topk.dev(); rq.res = st->bulk_rec.dev(); rq.l = l; rq.p = p;
    rc = enqueue_scan_merge(c, rq);
    if (rc != CHIP_OK) return rc;
    rc = sync_topk_out(c, 3, topk, scores, idx);   // (waits for the merge: the record is in pinned memory by then)
    if (rc != CHIP_OK) return rc;
    *out = *st->bulk_rec.host();
    return CHIP_OK;
}

extern "C" int chip_build_has_bulk_ticks(void) { return 1; }

extern "C" int chip_loop_ticks_bulk(chip_ctx *c, const int64_t *l, int32_t T, const chip_dot_params *p, int64_t last_l, int32_t topk, chip_tick_result *out,
                                    double *scores, int64_t *idx, int64_t *last_l_out)
{
    if (!c || !l || !out || T < 1) return CHIP_ERR_INVALID_ARG;
    if (topk < 1 || topk > CHIP_BULK_TICKS_MAX_TOPK || c->D % 32 != 0 || c->elem != 4) return CHIP_ERR_UNSUPPORTED;
    if (c->group || c->parent || c->nranks != 1 || c->xchg) return CHIP_ERR_UNSUPPORTED;
    chip_dot_params dflt;
    if (!p) { chip_dot_params_default(&dflt); p = &dflt; }
    int64_t n_global;
    double nrm;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        n_global = c->rows_global;
        nrm = c->row_norm_max;
    }
    if (n_global > INT32_MAX || c->seg_rows % 256 != 0) return CHIP_ERR_UNSUPPORTED;   // as query_batch_prefix
    std::vector<int32_t> status, ticks, rerun;
    std::vector<int64_t> k;
    try {
        status.resize((size_t)T); k.resize((size_t)T);
    } catch (const std::bad_alloc &) {
        return CHIP_ERR_OOM;
    }
    int64_t last_after = last_l;
    int rc = bulk_sequence(l, T, p, last_l, n_global, status.data(), k.data(), &last_after);
    if (rc == CHIP_OK) rc = bulk_order(status.data(), k.data(), T, ticks);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    (void)coalesce_flush(c);
    CHIP_HIP(c, hipSetDevice(c->device));
    if (!c->batch_state) {
        c->batch_state = new (std::nothrow) BatchState();
        if (!c->batch_state) return CHIP_ERR_OOM;
    }
    BatchState *st = c->batch_state;
    ResidentPause paused(c);   // as query_batch_prefix
    rc = st->bulk_rec.reserve(c, 1);
    if (rc != CHIP_OK) return rc;
    // no fp32 partial sum overflows (scan_prefilter_usable's condition; false for NaN as well) -- else every tick takes the exact path
    const bool norm_ok = nrm * nrm <= std::ldexp(1.0, 120) && 2.0 * c->D * std::ldexp(1.0, -24) < 0.5;
    const double E = norm_ok ? prefilter_error_bound(c->D, nrm) : 0.0;
    st->bulk_last = chip_bulk_ticks_last{};
    st->bulk_last.list_len = kBulkListLen;
    st->bulk_last.E = E;
    for (int32_t t = 0; t < T; t++) {
        fill_immediate(out + t, status[(size_t)t]);
        for (int32_t j = 0; j < 3 * topk; j++) {
            if (scores) scores[(size_t)t * 3 * topk + j] = -INFINITY;
            if (idx) idx[(size_t)t * 3 * topk + j] = -1;
        }
    }
    const int32_t n_scan = (int32_t)ticks.size();
    if (norm_ok) {
        for (int32_t first = 0; first < n_scan; first += CHIP_BULK_TICKS_GROUP) {
            const int32_t nt = n_scan - first < CHIP_BULK_TICKS_GROUP ? n_scan - first : CHIP_BULK_TICKS_GROUP;
            rc = bulk_group_run(c, st, l, k.data(), ticks.data() + first, nt, p, topk, E, out, scores, idx, rerun);
            if (rc != CHIP_OK) return rc;
        }
    } else {
        rerun.swap(ticks);
    }
    for (const int32_t t : rerun) {
        const size_t at = (size_t)t * 3 * topk;
        rc = bulk_exact_tick(c, st, l[t], k[(size_t)t], p, topk, out + t, scores ? scores + at : nullptr, idx ? idx + at : nullptr);
        if (rc != CHIP_OK) return rc;
        st->bulk_last.exact_reruns++;
    }
    if (last_l_out) *last_l_out = last_after;
    return CHIP_OK;
}

extern "C" int chip_bulk_ticks_plan(const int64_t *l, int32_t T, const chip_dot_params *p, int64_t last_l, int64_t n_rows, int32_t *status, int64_t *k,
                                    chip_bulk_ticks_plan_out *out)
{
    if (!l || !status || !k || !out || T < 1 || n_rows < 0) return CHIP_ERR_INVALID_ARG;
    chip_dot_params dflt;
    if (!p) { chip_dot_params_default(&dflt); p = &dflt; }
    chip_bulk_ticks_plan_out f = {};
    f.group_ticks = CHIP_BULK_TICKS_GROUP;
    std::vector<int32_t> st, ticks;
    std::vector<int64_t> kk;
    try {
        st.resize((size_t)T); kk.resize((size_t)T);
    } catch (const std::bad_alloc &) {
        return CHIP_ERR_OOM;
    }
    int rc = bulk_sequence(l, T, p, last_l, n_rows, st.data(), kk.data(), &f.last_l);
    if (rc == CHIP_OK) rc = bulk_order(st.data(), kk.data(), T, ticks);
    if (rc != CHIP_OK) return rc;
    for (int32_t t = 0; t < T; t++) {
        if (st[(size_t)t] == CHIP_TICK_SKIPPED) f.ticks_skipped++;
        else if (st[(size_t)t] == CHIP_TICK_TOO_SHORT) f.ticks_too_short++;
    }
    const int32_t n_scan = (int32_t)ticks.size();
    f.ticks_scanned = n_scan;
    const int64_t kmax = n_scan ? kk[(size_t)ticks[(size_t)n_scan - 1]] : 0;
    for (int32_t first = 0; first < n_scan; first += CHIP_BULK_TICKS_GROUP) {
        const int32_t nt = n_scan - first < CHIP_BULK_TICKS_GROUP ? n_scan - first : CHIP_BULK_TICKS_GROUP;
        BulkGroup b;
        rc = bulk_group(l, kk.data(), ticks.data() + first, nt, nullptr, &b);
        if (rc != CHIP_OK) return rc;
        f.groups++;
        if (nt == CHIP_BULK_TICKS_GROUP) f.tile_full = b.g.TM;
        f.tile_last = b.g.TM;
        f.units += b.g.units;
        f.units_rect += b.g.qtiles * ((kmax + b.g.TM - 1) / b.g.TM);
    }
    memcpy(status, st.data(), sizeof(int32_t) * (size_t)T);
    memcpy(k, kk.data(), sizeof(int64_t) * (size_t)T);
    *out = f;
    return CHIP_OK;
}

extern "C" int chip_debug_bulk_ticks_last(chip_ctx *c, chip_bulk_ticks_last *out)
{
    if (!c || !out) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    *out = c->batch_state ? c->batch_state->bulk_last : chip_bulk_ticks_last{};
    out->list_len = kBulkListLen;   // (a property of the build: said before the first call as well)
    return CHIP_OK;
}

extern "C" int chip_query_prefix_plan(const int64_t *k, int32_t Q, int32_t elem, int32_t topk, int32_t *order, chip_query_prefix_plan_out *out)
{
    if (!k || !out || Q < 1) return CHIP_ERR_INVALID_ARG;
    if ((elem != 4 && elem != 8) || topk < 1 || topk > CHIP_MAX_TOPK) return CHIP_ERR_UNSUPPORTED;
    for (int32_t j = 0; j < Q; j++)
        if (k[j] < 0) return CHIP_ERR_RANGE;
    std::vector<int32_t> ord;
    const int orc = prefix_order(k, Q, ord);
    if (orc != CHIP_OK) return orc;
    prefix_plan(k, Q, elem, topk, ord.data(), out);
    if (order) memcpy(order, ord.data(), sizeof(int32_t) * (size_t)Q);
    return CHIP_OK;
}

extern "C" int chip_debug_query_prefix_last(chip_ctx *c, chip_query_prefix_last *out)
{
    if (!c || !out) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    *out = c->batch_state ? c->batch_state->prefix_last : chip_query_prefix_last{};
    return CHIP_OK;
}
