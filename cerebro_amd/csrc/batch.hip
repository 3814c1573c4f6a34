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
#include <cmath>
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
__device__ __forceinline__ uint32_t lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
// every LDS-DMA load has landed, own LDS reads done, workgroup barrier
__device__ __forceinline__ void wait_loads_and_barrier()
{
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
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

// WN = waves along the DB rows of a tile (2 or 4); a wave owns WN x 2 MFMA 32x32 blocks (64 WN queries x 64 DB rows), the
// workgroup tile is 64 WN x 64 WN (128 x 128 with 4 waves, 256 x 256 with 8), 2 x WN waves, 8 LDS-DMA per wave per chunk either way.
// ROW = float: DB rows by LDS-DMA; ROW = double: rows narrowed to float on their way into the same image (see above).
template <int KC, int WN, int KL, typename ROW>
__global__ __launch_bounds__(128 * WN) void db_gemm_topk(BatchArgs a)
{
    constexpr bool CAST = std::is_same<ROW, double>::value;
    static_assert(CAST || std::is_same<ROW, float>::value, "float or double rows");
    static_assert(KC == 32, "one K-chunk = 8 slots of 4 floats per DB row");
    static_assert(WN == 2 || WN == 4, "tile 128 x 128 or 256 x 256");
    constexpr int TM = 64 * WN, TN = 64 * WN;            // tile: queries x DB rows
    constexpr int NT = 128 * WN, WAVES = 2 * WN;          // threads, waves
    constexpr int TILE = TM * KC;                         // floats of the A tile of one stage
    constexpr int BTILE = (TN / 8) * kBBlock;             // DB tile: TN / 8 blocks of 8 rows, kBBlock floats apart
    constexpr int STAGE = TILE + BTILE;                   // A tile then B tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *S0 = reinterpret_cast<float *>(smem);        // stage s: A = S0 + s*STAGE, B = A + TILE
    float *Ct = reinterpret_cast<float *>(smem);         // [TM][CT_LD] (aliases the stages after the K loop)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int D = a.D, K = a.K;
    const int q0 = blockIdx.y * TM;
    // DB tiles are handed out dynamically: workgroup x of a query tile starts on DB tile x and then takes the next unclaimed one
    // from a counter (one atomic per tile, ~1 ms of work; fetched at the start of the tile, read at its end).  With a static
    // split 3907 tiles over 256 workgroups cost 16 tile times on every CU; claimed tiles cost 15.26.  The lists a workgroup
    // keeps do not care which tiles fed them: the merged top-K is the same set whatever the assignment.
    __shared__ unsigned next_tile_slot;
    const int64_t n_tiles = (a.n_rows + TN - 1) / TN;

    // Top-k of the tile scores: ALL threads take part -- thread t owns query q0 + (t % TM) over the 64-column half (t / TM)
    // of every 128-column epilogue pass, with its sorted list in registers; the two lists of a query are folded at the end.
    // (Round 1 had 64 owner threads scan 2 x 128 columns while the other three waves -- and, in lockstep, the other workgroup
    // of the CU -- waited.)
    const int oq = tid & (TM - 1), och = tid / TM;
    TopList<KL> L;
    list_init(L);

    const int n_chunks = D / KC;
    // A loader: the chunk image is contiguous (TM * 128 B): pass u, wave w copies bytes [(u * WAVES + w) * 1024, + 1024)
    const float *const a_src = a.Qt + ((int64_t)blockIdx.y * n_chunks) * TILE + (wave * 64 + lane) * 4;
    // B loader: pass u, wave w, lane i -> 8-row block u * WAVES + w, row i >> 3 of it, slot p = i & 7,
    // source floats [4 k4, 4 k4 + 4), k4 = p ^ (row & 7)
    const int l_row = wave * 8 + (lane >> 3), l_p = lane & 7;
    const int l_k4 = (l_p ^ (lane >> 3)) * 4;
    // fragment map
    const int fr = lane & 31, fk = lane >> 5;
    const int rb0 = wn * 64 + fr, rb1 = rb0 + 32;
    const int b_off0 = TILE + b_row_off(rb0) + fk, b_off1 = TILE + b_row_off(rb1) + fk, sw0 = rb0 & 7, sw1 = rb1 & 7;
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(S0));

    // Units of work: the first n_full = floor(n_tiles / P) * P tiles are whole tiles (P = workgroups of this query tile: full
    // rounds in which every CU is busy); what remains -- r < P tiles, the round that would leave P - r CUs idle -- is cut
    // into query halves when 2 r <= P (each wave then owns WN / 2 x 2 blocks and the unit takes half a tile time: 15.5 instead of
    // 16 tile times for 3907 tiles on 256 CUs).
    const int64_t n_full = n_tiles / gridDim.x * gridDim.x;
    const bool halves = 2 * (n_tiles - n_full) <= (int64_t)gridDim.x;
    const int64_t n_units = halves ? n_full + 2 * (n_tiles - n_full) : n_tiles;
    for (int64_t unit = blockIdx.x; unit < n_units;) {
        const bool half_unit = halves && unit >= n_full;
        const int64_t tile = half_unit ? n_full + ((unit - n_full) >> 1) : unit;
        const int qhalf = half_unit ? (int)((unit - n_full) & 1) : 0;
        const int nrb = half_unit ? WN / 2 : WN;                                      // 32-query row blocks per wave in this unit
        const int qrow0 = half_unit ? qhalf * (TM / 2) + wm * (16 * WN) : wm * (32 * WN);   // first query row of this wave
        const int a_off = fk * TM + qrow0 + fr;                        // + kk * 2 TM per k-step, + 32 i for row block i
        const int64_t n0 = tile * TN;
        unsigned claimed = 0;
        if (tid == 0) claimed = __hip_atomic_fetch_add(a.tile_ctr + blockIdx.y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float *brow[4];
        // double rows: a tile lies within one segment (seg_rows is a multiple of TN: batch_local_enqueue), so its rows are a
        // workgroup-uniform base plus 32-bit byte offsets (segments are at most 1 GiB); rows past the end read the tile's first row
        const char *seg = nullptr;
        uint32_t boff[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t br = n0 + u * (8 * WAVES) + l_row;
            if constexpr (CAST) {
                const int64_t brc = br < a.n_rows ? br : n0;
                boff[u] = (uint32_t)(((brc & a.seg_mask) * (int64_t)D + l_k4) * 8);
            } else {
                const int64_t brc = br < a.n_rows ? br : 0;   // rows past the end: any valid row (their columns are never scanned)
                brow[u] = reinterpret_cast<const float *const *>(a.seg_table)[brc >> a.seg_shift] + (brc & a.seg_mask) * (int64_t)D + l_k4;
            }
        }
        if constexpr (CAST) {
            const uint64_t sp = (uint64_t)reinterpret_cast<const char *const *>(a.seg_table)[n0 >> a.seg_shift];
            // (readfirstlane returns int: each half goes through uint32_t, or a low word with bit 31 set would sign-extend over the high one)
            const uint32_t sp_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sp >> 32)), sp_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sp);
            seg = (const char *)(((uint64_t)sp_hi << 32) | sp_lo);
        }
        f32x16 acc[WN][2];
#pragma unroll
        for (int i = 0; i < WN; i++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;

        // chunk c -> stage c % NST: 8 LDS-DMA instructions per wave, number j = 2 u + (0: A, 1: B)
        auto stage_load_one = [&](int c, int j) {
            const uint32_t st = lds_base + (uint32_t)((c % NST) * STAGE) * 4u;
            const int u = j >> 1;
            if (j & 1) {
                if constexpr (!CAST) glds16(brow[u] + c * KC, st + (uint32_t)(TILE + b_row_off((u * WAVES + wave) * 8)) * 4u);
            } else glds16(a_src + (int64_t)c * TILE + u * (WAVES * 256), st + (uint32_t)((u * WAVES + wave) * 256) * 4u);
        };
        auto stage_load = [&](int c) {
#pragma unroll
            for (int j = 0; j < 8; j++) stage_load_one(c, j);
        };
        // double rows: slot u of chunk c through registers (the slots of a thread are lane-linear in block u * WAVES + wave)
        auto cast_load = [&](int c, int u, f64x2 *r) {
            if constexpr (CAST) {
                const auto *chunk = (const __attribute__((address_space(1))) char *)seg + (int64_t)c * (KC * 8);
                const auto *p = (const __attribute__((address_space(1))) f64x2 *)(chunk + boff[u]);
                r[0] = p[0];
                r[1] = p[1];
            }
        };
        auto cast_store = [&](int c, int u, const f64x2 *r) {
            if constexpr (CAST) {
                float *d = S0 + (c % NST) * STAGE + TILE + b_row_off((u * WAVES + wave) * 8) + lane * 4;
                const float x = (float)r[0][0], y = (float)r[0][1], z = (float)r[1][0], w = (float)r[1][1];
                if ((wave & 3) == 0) lds_store_slot<16>(d, x, y, z, w);
                else if ((wave & 3) == 2) lds_store_slot<8>(d, x, y, z, w);
                else lds_store_slot<4>(d, x, y, z, w);
            }
        };
        if (n_chunks > 0) {
            stage_load(0);
            if constexpr (CAST) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    f64x2 r[2];
                    cast_load(0, u, r);
                    cast_store(0, u, r);
                }
            }
        }
        wait_loads_and_barrier();   // chunk 0 has landed
        // the K loop, instantiated for whole tiles (NRB = WN row blocks per wave) and for query halves (NRB = WN / 2)
        auto k_loop = [&](auto nrb_tag) {
            constexpr int NRB = decltype(nrb_tag)::value;
            for (int c = 0; c < n_chunks; c++) {
                const float *St = S0 + (c % NST) * STAGE;
                // chunk c + 1 goes to the stage last read in iteration c-1 (barrier since).  When its 8 LDS-DMA instructions are
                // issued matters (a burst keeps a wave from issuing MFMAs for ~300 cycles; a late load is waited for at the barrier):
                //   128 tile  all 8 at once at the top (the other workgroup's wave fills the gap: 119.4 TF vs 114.8 spread);
                //   256 tile  two in front of each of MFMA groups 1..4 (both waves of a SIMD belong to this workgroup and burst
                //             together: 0.814 of peak vs 0.792 for the burst, 0.805 for groups 0..3, 0.76 for one per group).
                //   double rows, both tiles: a thread's four slots in two halves through 16 staging registers -- slots 0, 1 loaded in
                //             front of group 0 and stored in front of group 3, where slots 2, 3 are loaded, stored in front of group 7;
                //             the A-side DMA in front of groups 0 and 1 (a store waits for every load issued before it: all of them
                //             are two groups old by then).
                const bool prefetch = c + 1 < n_chunks;
                if (!CAST && WN == 2 && prefetch) stage_load(c + 1);
                f64x2 raw[2][2];
                // fragments of k-steps (2 k4, 2 k4 + 1) in f[k4 & 1]: [2 i + t] = A row block i, [2 WN + 2 j + t] = B block j;
                // the next pair is read before this pair's 4 WN MFMAs are issued
                float f[2][2 * WN + 4];
                auto rd = [&](int k4, float *d) {
#pragma unroll
                    for (int i = 0; i < NRB; i++) {
                        d[2 * i] = St[a_off + 32 * i + (2 * k4) * (2 * TM)];
                        d[2 * i + 1] = St[a_off + 32 * i + (2 * k4 + 1) * (2 * TM)];
                    }
                    const int p0 = (k4 ^ sw0) << 2, p1 = (k4 ^ sw1) << 2;
                    d[2 * WN] = St[b_off0 + p0];     d[2 * WN + 1] = St[b_off0 + p0 + 2];
                    d[2 * WN + 2] = St[b_off1 + p1]; d[2 * WN + 3] = St[b_off1 + p1 + 2];
                };
                rd(0, f[0]);
                __builtin_amdgcn_sched_group_barrier(0x100, NRB + 2, 0);  // the reads of the first pair
#pragma unroll
                for (int k4 = 0; k4 < KC / 4; k4++) {
                    if (!CAST && WN == 4 && prefetch && k4 >= 1 && k4 <= 4) { stage_load_one(c + 1, 2 * k4 - 2); stage_load_one(c + 1, 2 * k4 - 1); }
                    if (CAST && prefetch && k4 == 0) { cast_load(c + 1, 0, raw[0]); cast_load(c + 1, 1, raw[1]); }
                    if (CAST && prefetch && k4 <= 1) { stage_load_one(c + 1, 4 * k4); stage_load_one(c + 1, 4 * k4 + 2); }
                    if (CAST && prefetch && k4 == 3) {
                        cast_store(c + 1, 0, raw[0]); cast_store(c + 1, 1, raw[1]);
                        cast_load(c + 1, 2, raw[0]); cast_load(c + 1, 3, raw[1]);
                    }
                    if (CAST && prefetch && k4 == 7) { cast_store(c + 1, 2, raw[0]); cast_store(c + 1, 3, raw[1]); }
                    if (k4 + 1 < KC / 4) rd(k4 + 1, f[(k4 + 1) & 1]);
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const float b0 = f[k4 & 1][2 * WN + t], b1 = f[k4 & 1][2 * WN + 2 + t];
#pragma unroll
                        for (int i = 0; i < NRB; i++) {
                            const float av = f[k4 & 1][2 * i + t];
                            acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[i][0], 0, 0, 0);
                            acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[i][1], 0, 0, 0);
                        }
                    }
                    // keep the order "reads of the next pair, then this pair's MFMAs" through the scheduler
                    __builtin_amdgcn_sched_group_barrier(0x100, NRB + 2, 0);   // DS reads (ds_read2)
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NRB, 0);   // MFMA
                }
                // chunk c+1 has landed (no chunk behind it has been issued), every wave is done reading stage c % NST
                wait_loads_and_barrier();
            }
        };
        if (half_unit) k_loop(std::integral_constant<int, WN / 2>{});
        else k_loop(std::integral_constant<int, WN>{});
        // ---- epilogue: the score tile through LDS, 128 DB rows (two of the WN wave columns) per pass (the stages are free:
        // the K loop ended with a barrier); C/D layout of the MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
        const int ncols = (a.n_rows - n0) < TN ? (int)(a.n_rows - n0) : TN;
        // double rows: the epilogue's addresses are recomputed per tile from an opaque copy of the lane -- hoisted out of the tile loop
        // they would sit in registers the staging needs through the K loop (and spill)
        int elane = lane, eoq = oq;
        if constexpr (CAST) asm volatile("" : "+v"(elane), "+v"(eoq));
#pragma unroll
        for (int h = 0; h < WN / 2; h++) {
            if (h > 0) __syncthreads();   // the previous pass's scan is done with Ct
            if ((wn >> 1) == h) {
#pragma unroll
                for (int it = 0; it < WN; it++) {
                    if (it >= nrb) continue;   // a query half: the upper row blocks hold nothing
#pragma unroll
                    for (int jt = 0; jt < 2; jt++)
#pragma unroll
                        for (int e = 0; e < 16; e++) {
                            const int row = qrow0 + it * 32 + (e & 3) + 8 * (e >> 2) + 4 * (elane >> 5);   // query within the tile
                            const int col = (wn & 1) * 64 + jt * 32 + (elane & 31);                                  // DB row within the pass
                            Ct[row * CT_LD + col] = acc[it][jt][e];
                        }
                }
            }
            __syncthreads();
            float ts;
            int32_t tr;
            list_kth(L, K, ts, tr);
            const int pass_cols = ncols - h * 128;         // columns of this pass that exist
            const bool mine = !half_unit || (eoq >= qhalf * (TM / 2) && eoq < (qhalf + 1) * (TM / 2));   // a query half: only its queries have scores
            const int c_hi = !mine ? 0 : pass_cols < (och + 1) * 64 ? pass_cols : (och + 1) * 64;
            for (int c = och * 64; c < c_hi; c++) {
                const float s = Ct[eoq * CT_LD + c];
                const int32_t row = (int32_t)(n0 + h * 128 + c);
                if (fkey_gt(s, row, ts, tr)) {   // NaN never enters
                    list_push(L, K, s, row);
                    list_kth(L, K, ts, tr);
                }
            }
        }
        // next tile: published by thread 0, read by everyone after the barrier that also ends this tile's use of Ct
        if (tid == 0) next_tile_slot = gridDim.x + claimed;
        __syncthreads();
        if constexpr (CAST) unit = __builtin_amdgcn_readfirstlane(next_tile_slot);   // (registers: the tile's bookkeeping stays scalar)
        else unit = next_tile_slot;
    }
    // fold the two column-half lists of a query into one (through LDS, once per workgroup): one list per (partition, query)
    __syncthreads();
    float *const Ls = reinterpret_cast<float *>(smem);                 // [TM][KL]
    int32_t *const Lr = reinterpret_cast<int32_t *>(Ls + TM * KL);
    if (och == 1) {
#pragma unroll
        for (int j = 0; j < KL; j++) { Ls[oq * KL + j] = L.s[j]; Lr[oq * KL + j] = L.r[j]; }
    }
    __syncthreads();
    if (och == 0) {
        for (int j = 0; j < K; j++) {
            const float s = Ls[oq * KL + j];
            const int32_t row = Lr[oq * KL + j];
            float ts;
            int32_t tr;
            list_kth(L, K, ts, tr);
            if (row >= 0 && fkey_gt(s, row, ts, tr)) list_push(L, K, s, row);
        }
        chip_topk_entry *dst = a.partial + ((int64_t)blockIdx.x * a.Qpad + q0 + oq) * K;
#pragma unroll
        for (int j = 0; j < KL; j++)
            if (j < K) {
                chip_topk_entry e;
                e.score = (double)L.s[j];
                e.idx = L.r[j] >= 0 ? (int64_t)L.r[j] * a.idx_mul + a.idx_add : -1;
                dst[j] = e;
            }
    }
    (void)NT;
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
    hipEvent_t ev_done = nullptr;     // this shard's list is complete (recorded on its scan stream)
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
    const bool wide = Qpad % 256 == 0 && !(c->elem == 8 && topk > 8);
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
