// match.hip -- the candidate verification front end on gfx950: what the reference's loop-candidate consumer runs per candidate between
// the descriptor scan and the three pose solves (include/cerebro_hip.h, "candidate verification front end", has the definitions):
//
//   hamming_match_split : cv::BFMatcher(NORM_HAMMING).match(d1, d2) (src/utils/PointFeatureMatching.cpp:38-41).  One query descriptor per
//                     lane in 8 VGPRs, one tile of 1024 train descriptors (32 KiB) staged through LDS per workgroup; every lane of a wave
//                     reads the SAME LDS address (a broadcast, conflict-free), xor + popcount, running (distance, index) per lane; the
//                     scan goes in index order with a strict <, and the tiles of a candidate meet in one 64-bit unsigned atomic minimum
//                     of distance << 32 | index, so ties keep the lowest train index.  Grid: query blocks of 256 x train tiles x candidates.
//   gms_filter      : gms_matcher::GetInlierMask(.., false, false) (src/utils/GMSMatcher/gms_matcher.cpp:9-15 -> run(1), :150-181) in ONE
//                     workgroup: per grid type 1..4 (:158) the 400 x 400 motion-statistics table (global scratch of the ctx; integer
//                     atomicAdd, order-independent) and the per-left-cell counts (LDS) of AssignMatchPairs (:73-98), then
//                     VerifyCellPairs (:100-148, rotation pattern 1 = identity) with one wave per table row for the first-maximum
//                     search and one lane per left cell for the 3 x 3 score against 6 * sqrt(mean count), then the inlier marks (:169-177).
//   gms_batch       : the same pass (gms_pass) with one workgroup per (grid type, candidate), on the matcher's keys.
//   gms_grid_modes  : GetInlierMask(.., WithScale, WithRotation) (gms_matcher.cpp:17-68), the optional form (modes != 0): one workgroup per
//                     (scale, grid type, candidate) builds table and column search once and scores the 400 x 8 (left cell, rotation) items;
//   gms_mode_select : one workgroup per candidate counts the up to 40 hypotheses, applies the choice and writes the winner's mask where
//                     gms_batch writes its planes.  Both also serve chip_gms_filter_modes (B = 1, the explicit list).
//   pose_sets_batch : MiscUtils::dmatch_2_eigen (src/utils/MiscUtils.cpp:121-143) + the two make_3d_2d_collection__ calls and
//                     make_3d_3d_collection__using__pfmatches_and_disparity (PointFeatureMatching.cpp:95-195) as ONE ordered stream
//                     compaction per candidate (ballot + prefix popcount per wave, scan across the 16 waves): outputs are in match
//                     order, in the layout pnp.hip / icp.hip take.
//
// There is ONE device pipeline, match_run: one query frame against B <= 16 candidates through hamming_match_split, gms_batch and
// pose_sets_batch.  chip_match_batch is that; chip_match_pair is a batch of one; chip_orb_match is the first kernel alone with one
// candidate and keys of its own.  gms_filter serves chip_gms_filter alone (an arbitrary match list, which the keys cannot express).
// chip_match_pairs_stored runs the same pipeline on a LIST of (query, candidate) pairs of stored frames, every pair with a query frame
// of its own: hamming_match_pairs, pairs_gms (with GMS modes pairs_grid_modes + pairs_mode_select) and pose_sets_stored_pairs are the
// bodies of the kernels above -- each stated once as a __device__ function -- with the pair's query frame taken from a second table in
// the kernel arguments, and with a count (the pair's own keypoints) apart from the stride of the rows (the widest query of the list).
// The frame store that the _stored entries read, and everything that fills it, is frames.hip: a run reaches a stored frame through
// FrameStore::rows (frame_store.h) and reads its point records (RecordPoints) where a run on host frames reads the 3-D images.
//
// Nothing here rounds twice: float division / multiplication, the float -> double widenings, fp64 add / multiply / divide / sqrt are
// single IEEE operations (-ffp-contract=off), the rest is integer.  tests/np_mirror_match.py restates all of it in numpy and
// tests/test_match_gpu.py compares byte for byte.
#include "chip_internal.h"
#include "frame_store.h"
#include "ransac_common.h"
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

namespace chip {

constexpr int kBfThreads = 256;
constexpr int kBfTile = 1024;            // train descriptors per LDS tile: 1024 x 32 B = 32 KiB
constexpr int kGrid = 20;                // mGridSizeLeft = Size(20, 20) (gms_matcher.h:62); right grid = left x the scale ratio of index 0 = 1.0 (:46, :230-231)
constexpr int kCells = kGrid * kGrid;    // 400
constexpr int kOneWg = 1024;             // the GMS and set-building kernels: one workgroup of 16 waves

// ------------------------------------------------------------------------------------------------ gms_filter
struct GmsArgs {
    const float2 *kp1, *kp2;
    int32_t w1, h1, w2, h2;
    const int32_t *qidx, *tidx; // match i is (qidx[i], tidx[i])
    int32_t n;
    int32_t *table;             // [400][400] motion statistics (mMotionStatistics, gms_matcher.h:93)
    uint8_t *inlier;            // [n]
    int32_t *n_inliers;
};

// floor of a grid coordinate as the reference evaluates it: pt.x * width is Point2f x int = a FLOAT product; "+ 0.5" promotes to double
// (gms_matcher.h:147-148,155,164,172-173).  Coordinates that are not finite or absurdly large have no cell.
constexpr double kCoordLim = 1.0e6;
__device__ __forceinline__ bool gms_coord(float p, bool shifted, int *out)
{
    const float f = p * (float)kGrid;
    const double v = shifted ? floor((double)f + 0.5) : (double)floorf(f);
    if (!(v >= -kCoordLim && v <= kCoordLim)) return false;
    *out = (int)v;
    return true;
}
// GetGridIndexLeft (gms_matcher.h:143-182); -1 also for an index outside [0, 400) (the reference would index out of bounds)
__device__ __forceinline__ int gms_cell_left(float px, float py, int type)
{
    const bool sx = type == 2 || type == 4, sy = type == 3 || type == 4;
    int x, y;
    if (!gms_coord(px, sx, &x) || !gms_coord(py, sy, &y)) return -1;
    if (type == 1 && (y >= kGrid || x >= kGrid)) return -1;   // :150
    if (sx && (x >= kGrid || x < 1)) return -1;               // :158, :176
    if (sy && (y >= kGrid || y < 1)) return -1;               // :167, :176
    const int idx = x + y * kGrid;
    return idx >= 0 && idx < kCells ? idx : -1;
}
// GetGridIndexRight (gms_matcher.h:184-189): no range check there; outside [0, 400) the match has no right cell
__device__ __forceinline__ int gms_cell_right(float px, float py)
{
    int x, y;
    if (!gms_coord(px, false, &x) || !gms_coord(py, false, &y)) return -1;
    const int idx = x + y * kGrid;
    return idx >= 0 && idx < kCells ? idx : -1;
}
// table entries are written by atomics (performed in L2) and read back by other lanes of the workgroup: read them at agent scope too
__device__ __forceinline__ int32_t table_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One grid type of gms_matcher::run (gms_matcher.cpp:161-177) by ONE workgroup of kOneWg threads: match(i, &lp, &rp) fetches the keypoints of
// match i, mark(i, hit) receives whether its cell pair is the accepted pair of its left cell.  gms_filter runs the four types one after
// another on one table, gms_batch one type per workgroup on a table of its own.
template <class Match, class Mark>
__device__ __forceinline__ void gms_pass(int type, int n, int32_t *table, float fw1, float fh1, float fw2, float fh2, Match match, Mark mark)
{
    __shared__ int32_t cnt[kCells];      // mNumberPointsInPerCellLeft
    __shared__ int32_t pair[kCells];     // mCellPairs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- :161-163
    for (int e = tid; e < kCells * kCells / 4; e += kOneWg) reinterpret_cast<int4 *>(table)[e] = make_int4(0, 0, 0, 0);
    for (int e = tid; e < kCells; e += kOneWg) { cnt[e] = 0; pair[e] = -1; }
    __threadfence();
    __syncthreads();
    // ---- AssignMatchPairs (:73-98); NormalizePoints (gms_matcher.h:126-139): float / int -> one float division
    for (int i = tid; i < n; i += kOneWg) {
        float2 lp, rp;
        match(i, &lp, &rp);
        const int l = gms_cell_left(__fdiv_rn(lp.x, fw1), __fdiv_rn(lp.y, fh1), type);
        const int r = gms_cell_right(__fdiv_rn(rp.x, fw2), __fdiv_rn(rp.y, fh2));
        if (l < 0 || r < 0) continue;                     // :92
        atomicAdd(&table[l * kCells + r], 1);             // :94
        atomicAdd(&cnt[l], 1);                            // :95
    }
    __threadfence();
    __syncthreads();
    // ---- VerifyCellPairs, first half (:106-121): per non-empty row the first column of maximal count.  One wave per row.
    for (int row = wave; row < kCells; row += kOneWg / 64) {
        if (cnt[row] == 0) continue;                      // sum(row) == 0 (:106): every increment of the row also counted in cnt
        int bv = 0, bj = INT_MAX;
        for (int j = lane; j < kCells; j += 64) {
            const int v = table_load(&table[row * kCells + j]);
            if (v > bv) { bv = v; bj = j; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const int ov = __shfl_xor(bv, m, 64), oj = __shfl_xor(bj, m, 64);
            if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
        if (lane == 0) pair[row] = bj;
    }
    __syncthreads();
    // ---- second half (:123-146): 3 x 3 neighbourhood score (GetNB9, gms_matcher.h:197-217; rotation pattern 1: same offset both sides)
    if (tid < kCells && pair[tid] >= 0) {
        const int lx = tid % kGrid, ly = tid / kGrid, rx = pair[tid] % kGrid, ry = pair[tid] / kGrid;
        int score = 0, tsum = 0, numpair = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int llx = lx + dx, lly = ly + dy, rrx = rx + dx, rry = ry + dy;
                if (llx < 0 || llx >= kGrid || lly < 0 || lly >= kGrid || rrx < 0 || rrx >= kGrid || rry < 0 || rry >= kGrid) continue;   // :136
                const int ll = llx + lly * kGrid, rr = rrx + rry * kGrid;
                score += table_load(&table[ll * kCells + rr]);
                tsum += cnt[ll];
                numpair++;
            }
        const double thresh = 6.0 * sqrt((double)tsum / (double)numpair);   // THRESH_FACTOR (gms_matcher.h:9), :143
        if ((double)score < thresh) pair[tid] = -2;                            // :145-146 (only this lane reads pair[tid] before the barrier)
    }
    __syncthreads();
    // ---- mark (:169-177)
    for (int i = tid; i < n; i += kOneWg) {
        float2 lp, rp;
        match(i, &lp, &rp);
        const int l = gms_cell_left(__fdiv_rn(lp.x, fw1), __fdiv_rn(lp.y, fh1), type);
        const int r = gms_cell_right(__fdiv_rn(rp.x, fw2), __fdiv_rn(rp.y, fh2));
        mark(i, l >= 0 && r >= 0 && pair[l] == r);
    }
    __syncthreads();                                      // pair / cnt are rewritten by the next pass
}

// chip_gms_filter alone: the four grid types on an explicit (qidx, tidx) list, which the pipeline's keys (match i = query i) cannot express
__global__ __launch_bounds__(kOneWg) void gms_filter(GmsArgs a)
{
    __shared__ int32_t total;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) total = 0;
    for (int i = tid; i < a.n; i += kOneWg) a.inlier[i] = 0;   // mvbInlierMask.assign(false) (gms_matcher.cpp:152); own bytes, same lane later
    for (int type = 1; type <= 4; type++)                     // :158
        gms_pass(type, a.n, a.table, (float)a.w1, (float)a.h1, (float)a.w2, (float)a.h2,
                 [&](int i, float2 *lp, float2 *rp) { *lp = a.kp1[a.qidx[i]]; *rp = a.kp2[a.tidx[i]]; },
                 [&](int i, bool hit) { if (hit) a.inlier[i] = 1; });
    int mine = 0;
    for (int i = tid; i < a.n; i += kOneWg) mine += a.inlier[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    if (lane == 0) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) *a.n_inliers = total;                       // :179
}

// ------------------------------------------------------------------------------------------------ the correspondence sets
enum { kSetUv = 0, kSetAb = 1, kSetBa = 2, kSet33 = 3, kSetOut = 4, kNSets = 5 };
struct SetsArgs {
    const float2 *kp1, *kp2;
    int32_t n;
    double Kinv[9];               // row-major
    double *uv, *uv_d, *X_ab, *uvn_ab, *X_ba, *uvn_ba, *A, *B;
    int32_t *mq, *mt;
    int32_t *counts;              // [kNSets]: n_matches_gms, n_3d2d_ab, n_3d2d_ba, n_3d3d, n_out_of_image
};

// (pixel_of, the pixel of a keypoint as the reference indexes the 3-D image, is in frame_store.h: frame_gather uses it too)
// the depth gate of :122 / :182: "z < 0.1 || z > 25." with the float z widened to double
__device__ __forceinline__ bool depth_ok(float z) { return !((double)z < 0.1 || (double)z > 25.); }

// Where a keypoint's 3-D point comes from.  in_a(i, p, &r) / in_b(t, p, &r): keypoint i of frame a / t of frame b at p has a pixel in its
// image, r then refers to its point; a(r, k) / b(r, k): coordinate k of that point.
// ImagePoints: the frames' 3-D images (H x W x 3), r = the pixel's offset.
struct ImagePoints {
    const float *xyz_a, *xyz_b;
    int32_t w1, h1, w2, h2;
    typedef size_t Ref;
    __device__ __forceinline__ bool in_a(int, float2 p, Ref *r) const
    {
        int x, y;
        if (!pixel_of(p, w1, h1, &x, &y)) return false;
        *r = 3 * ((size_t)y * w1 + x);
        return true;
    }
    __device__ __forceinline__ bool in_b(int, float2 p, Ref *r) const
    {
        int x, y;
        if (!pixel_of(p, w2, h2, &x, &y)) return false;
        *r = 3 * ((size_t)y * w2 + x);
        return true;
    }
    __device__ __forceinline__ float a(Ref r, int k) const { return xyz_a[r + k]; }
    __device__ __forceinline__ float b(Ref r, int k) const { return xyz_b[r + k]; }
};
// RecordPoints: the frame store's point records, one float4 per keypoint (frame_gather, frames.hip): (x, y, z, 1.0f) copied from the image at put
// time, or (0, 0, 0, 0.0f) for a keypoint outside it; r = the record.
struct RecordPoints {
    const float4 *rec_a, *rec_b;
    typedef float4 Ref;
    __device__ __forceinline__ bool in_a(int i, float2, Ref *r) const { *r = rec_a[i]; return r->w != 0.0f; }
    __device__ __forceinline__ bool in_b(int t, float2, Ref *r) const { *r = rec_b[t]; return r->w != 0.0f; }
    __device__ __forceinline__ float a(const Ref &r, int k) const { return k == 0 ? r.x : k == 1 ? r.y : r.z; }
    __device__ __forceinline__ float b(const Ref &r, int k) const { return a(r, k); }
};

// The ordered compaction by ONE workgroup of kOneWg threads; inlier(i) / train(i): the GMS mark and the train index of match i
// (the four planes of gms_batch and the merged keys); pts: ImagePoints (pose_sets_batch) or RecordPoints (pose_sets_stored_batch)
template <class Inlier, class Train, class Points>
__device__ __forceinline__ void pose_sets_body(const SetsArgs &a, Inlier inlier, Train train, const Points &pts)
{
    __shared__ int32_t wtot[kNSets][kOneWg / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run[kNSets] = {0, 0, 0, 0, 0};
    for (int base = 0; base < a.n; base += kOneWg) {
        const int i = base + tid;
        bool f[kNSets] = {false, false, false, false, false};
        float2 pa = make_float2(0.f, 0.f), pb = pa;
        int t = 0;
        typename Points::Ref oa{}, ob{};
        if (i < a.n && inlier(i)) {
            t = train(i);
            pa = a.kp1[i]; pb = a.kp2[t];
            const bool in_a = pts.in_a(i, pa, &oa), in_b = pts.in_b(t, pb, &ob);
            bool za = false, zb = false;
            if (in_a) za = depth_ok(pts.a(oa, 2));
            if (in_b) zb = depth_ok(pts.b(ob, 2));
            f[kSetUv] = true; f[kSetAb] = za; f[kSetBa] = zb; f[kSet33] = za && zb; f[kSetOut] = !in_a || !in_b;
        }
        int pos[kNSets];
#pragma unroll
        for (int s = 0; s < kNSets; s++) {
            const unsigned long long m = __ballot(f[s]);
            pos[s] = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wtot[s][wave] = __popcll(m);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kNSets; s++) {
            int before = 0, all = 0;
            for (int w = 0; w < kOneWg / 64; w++) { const int c = wtot[s][w]; all += c; if (w < wave) before += c; }
            pos[s] += run[s] + before;
            run[s] += all;
        }
        __syncthreads();                                      // wtot is rewritten by the next chunk
        const double ua = (double)pa.x, va = (double)pa.y, ub = (double)pb.x, vb = (double)pb.y;
        if (f[kSetUv]) {                                      // dmatch_2_eigen (MiscUtils.cpp:132-142)
            const int o = pos[kSetUv];
            a.uv[2 * o] = ua; a.uv[2 * o + 1] = va; a.uv_d[2 * o] = ub; a.uv_d[2 * o + 1] = vb;
            a.mq[o] = i; a.mt[o] = t;
        }
        // K.inverse() * uv (PointFeatureMatching.cpp:114-115), rows 0 and 1 of the 3 x 3 by 3 x 1 product, left to right
        if (f[kSetAb]) {                                      // make_3d_2d(uv, a_3dImage, uv_d) (Cerebro.cpp:1512): a's point, b's normalised pixel
            const int o = pos[kSetAb];
            for (int k = 0; k < 3; k++) a.X_ab[3 * o + k] = (double)pts.a(oa, k);
            a.uvn_ab[2 * o] = (a.Kinv[0] * ub + a.Kinv[1] * vb) + a.Kinv[2];
            a.uvn_ab[2 * o + 1] = (a.Kinv[3] * ub + a.Kinv[4] * vb) + a.Kinv[5];
        }
        if (f[kSetBa]) {                                      // make_3d_2d(uv_d, b_3dImage, uv) (Cerebro.cpp:1566)
            const int o = pos[kSetBa];
            for (int k = 0; k < 3; k++) a.X_ba[3 * o + k] = (double)pts.b(ob, k);
            a.uvn_ba[2 * o] = (a.Kinv[0] * ua + a.Kinv[1] * va) + a.Kinv[2];
            a.uvn_ba[2 * o + 1] = (a.Kinv[3] * ua + a.Kinv[4] * va) + a.Kinv[5];
        }
        if (f[kSet33]) {                                      // make_3d_3d (Cerebro.cpp:1624)
            const int o = pos[kSet33];
            for (int k = 0; k < 3; k++) { a.A[3 * o + k] = (double)pts.a(oa, k); a.B[3 * o + k] = (double)pts.b(ob, k); }
        }
    }
    if (tid < kNSets) a.counts[tid] = run[tid];
}

// ------------------------------------------------------------------------------------------------ one query frame, B candidates
// The three kernels of the pipeline have a candidate dimension in the grid.  Candidate j's descriptors, keypoints, 3-D image and sizes
// travel in the kernel arguments; all B pairs read ONE device copy of the query frame.
constexpr int kMaxBatch = CHIP_MATCH_MAX_BATCH;
struct BatchCand {
    const uint4 *desc;            // n x 2
    const float2 *kp;             // n
    const float *xyz;             // h x w x 3
    int32_t n, w, h, pad_;
};
struct BatchCands { BatchCand c[kMaxBatch]; };

// A partial minimum as ONE unsigned 64-bit key, distance << 32 | train index: the unsigned minimum over the tiles of a (query, candidate)
// is the smallest distance and, among equal distances, the LOWEST index -- BFMatcher's tie rule, whichever tile arrives first.
// All ones (the preset) decodes to index -1, distance -1: no train descriptors.
__device__ __forceinline__ int32_t key_train(unsigned long long k) { return (int32_t)(uint32_t)k; }

// One workgroup of kBfThreads: query block blockIdx.x of the n1 >= 1 query descriptors against train tile blockIdx.y of the n2 train
// descriptors, merged into keys[0 .. n1), the row of this (query frame, candidate); a tile past n2 leaves at once
__device__ __forceinline__ void hamming_tile(const uint4 *__restrict__ query, int n1, const uint4 *__restrict__ train, int n2,
                                             unsigned long long *__restrict__ keys)
{
    __shared__ uint4 tile[2 * kBfTile];
    const int base = blockIdx.y * kBfTile;
    if (base >= n2) return;                                   // workgroup-uniform
    const int cnt = n2 - base < kBfTile ? n2 - base : kBfTile;
    const int i = blockIdx.x * kBfThreads + threadIdx.x;
    const int qi = i < n1 ? i : n1 - 1;                       // n1 >= 1: the tail lanes scan a valid descriptor and store nothing
    const uint4 q0 = query[2 * (size_t)qi], q1 = query[2 * (size_t)qi + 1];
    for (int e = threadIdx.x; e < 2 * cnt; e += kBfThreads) tile[e] = train[2 * (size_t)base + e];
    __syncthreads();
    int best = INT_MAX, bidx = -1;
#pragma unroll 4
    for (int j = 0; j < cnt; j++) {
        const uint4 a = tile[2 * j], b = tile[2 * j + 1];      // wave-uniform address: one broadcast read
        const int d = __popc(q0.x ^ a.x) + __popc(q0.y ^ a.y) + __popc(q0.z ^ a.z) + __popc(q0.w ^ a.w) +
                      __popc(q1.x ^ b.x) + __popc(q1.y ^ b.y) + __popc(q1.z ^ b.z) + __popc(q1.w ^ b.w);
        if (d < best) { best = d; bidx = base + j; }          // strict: the first minimum of the tile stays
    }
    if (i < n1)                                               // cnt >= 1: bidx >= 0.  One native 64-bit unsigned minimum per lane and tile
        __hip_atomic_fetch_min(&keys[i], ((unsigned long long)(uint32_t)best << 32) | (uint32_t)bidx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (query blocks of 256, train tiles of 1024, B): one workgroup scans ONE tile; a tile past the candidate's n leaves at once
__global__ __launch_bounds__(kBfThreads) void hamming_match_split(const uint4 *__restrict__ query, int n1, BatchCands cands,
                                                                  unsigned long long *__restrict__ keys /* [B][n1] */)
{
    const int z = blockIdx.z;
    hamming_tile(query, n1, cands.c[z].desc, cands.c[z].n, keys + (size_t)z * n1);
}

// ---- a list of (query, candidate) pairs: pair z carries its query frame next to its candidate, a second table in the kernel arguments
// read through wave-uniform loads like the first.  Keys, planes and slabs are rows of `stride` = the largest query of the list per pair;
// pair z uses the first q[z].n of its row.  A pair with an empty frame on either side has n = 0 in BOTH tables and takes no part.
struct PairQuery {
    const uint4 *desc;            // n x 2
    const float2 *kp;             // n
    const float4 *rec;            // n: the point records (frame_gather)
    int32_t n, w, h, pad_;
};
struct PairQueries { PairQuery q[kMaxBatch]; };

// grid (query blocks of 256 over the stride, train tiles of 1024, P): a workgroup whose query block starts at or beyond its own pair's
// n1, or whose tile starts beyond its n2, leaves at once -- both tests are workgroup-uniform and come before the barrier
__global__ __launch_bounds__(kBfThreads) void hamming_match_pairs(PairQueries qs, BatchCands cands, int stride,
                                                                  unsigned long long *__restrict__ keys /* [P][stride] */)
{
    const int z = blockIdx.z, n1 = qs.q[z].n;
    if ((int)(blockIdx.x * kBfThreads) >= n1) return;
    hamming_tile(qs.q[z].desc, n1, cands.c[z].desc, cands.c[z].n, keys + (size_t)z * stride);
}

struct GmsBatchArgs {
    const float2 *kp1;                    // the query frame's keypoints; match i of candidate j = (i, train index of keys[j][i])
    int32_t n1, w1, h1;
    const unsigned long long *keys;       // [B][n1]
    int32_t *table;                       // [B][4][400][400]
    uint8_t *plane;                       // [B][4][n1]: the marks of ONE grid type each (pose_sets_batch takes their OR)
    BatchCands cands;
};
// grid (4 grid types, B): gms_filter's pass, one workgroup per (type, candidate) on its own table, writing its own byte plane
__global__ __launch_bounds__(kOneWg) void gms_batch(GmsBatchArgs a)
{
    const int type = blockIdx.x + 1, z = blockIdx.y;
    if (a.cands.c[z].n == 0) return;                          // no matches: pose_sets_batch does not read this candidate's planes
    const float2 *kp2 = a.cands.c[z].kp;
    const unsigned long long *keys = a.keys + (size_t)z * a.n1;
    uint8_t *plane = a.plane + ((size_t)z * 4 + blockIdx.x) * a.n1;
    gms_pass(type, a.n1, a.table + ((size_t)z * 4 + blockIdx.x) * (kCells * kCells), (float)a.w1, (float)a.h1, (float)a.cands.c[z].w,
             (float)a.cands.c[z].h, [&](int i, float2 *lp, float2 *rp) { *lp = a.kp1[i]; *rp = kp2[key_train(keys[i])]; },
             [&](int i, bool hit) { plane[i] = hit ? 1 : 0; });
}

struct GmsPairsArgs {
    const unsigned long long *keys;       // [P][stride]
    int32_t *table;                       // [P][4][400][400]
    uint8_t *plane;                       // [P][4][stride]
    int32_t stride;
    PairQueries qs;
    BatchCands cands;
};
// grid (4 grid types, P): gms_batch with the pair's own query keypoints, count and image size
__global__ __launch_bounds__(kOneWg) void pairs_gms(GmsPairsArgs a)
{
    const int type = blockIdx.x + 1, z = blockIdx.y;
    if (a.cands.c[z].n == 0) return;                          // no matches: pose_sets_stored_pairs does not read this pair's planes
    const float2 *kp1 = a.qs.q[z].kp, *kp2 = a.cands.c[z].kp;
    const unsigned long long *keys = a.keys + (size_t)z * a.stride;
    uint8_t *plane = a.plane + ((size_t)z * 4 + blockIdx.x) * a.stride;
    gms_pass(type, a.qs.q[z].n, a.table + ((size_t)z * 4 + blockIdx.x) * (kCells * kCells), (float)a.qs.q[z].w, (float)a.qs.q[z].h,
             (float)a.cands.c[z].w, (float)a.cands.c[z].h, [&](int i, float2 *lp, float2 *rp) { *lp = kp1[i]; *rp = kp2[key_train(keys[i])]; },
             [&](int i, bool hit) { plane[i] = hit ? 1 : 0; });
}

struct SetsBatchArgs {
    const float2 *kp1;
    const float *xyz_a;
    int32_t n1, w1, h1;
    const unsigned long long *keys;       // [B][n1]
    const uint8_t *plane;                 // [B][4][n1]
    double Kinv[9];
    double *uv, *uv_d, *X_ab, *uvn_ab, *X_ba, *uvn_ba, *A, *B;   // slabs of n1 rows per candidate
    int32_t *mq, *mt;
    int32_t *counts;                      // [B][kNSets]
    BatchCands cands;
};
// the sets of candidate z, inlier = the OR of its four planes, outputs into its slabs: n matches of the query keypoints kp1 in rows of
// `stride` (one query frame: n = stride = b.n1; a pair list: the pair's own n and kp1)
template <class Points>
__device__ __forceinline__ void pose_sets_rows(const SetsBatchArgs &b, int z, const float2 *kp1, int n, size_t stride, const Points &pts)
{
    const size_t row = (size_t)z * stride;
    SetsArgs a;
    a.kp1 = kp1; a.kp2 = b.cands.c[z].kp; a.n = n;
    for (int k = 0; k < 9; k++) a.Kinv[k] = b.Kinv[k];
    a.uv = b.uv + 2 * row; a.uv_d = b.uv_d + 2 * row; a.X_ab = b.X_ab + 3 * row; a.uvn_ab = b.uvn_ab + 2 * row;
    a.X_ba = b.X_ba + 3 * row; a.uvn_ba = b.uvn_ba + 2 * row; a.A = b.A + 3 * row; a.B = b.B + 3 * row;
    a.mq = b.mq + row; a.mt = b.mt + row; a.counts = b.counts + z * kNSets;
    const unsigned long long *keys = b.keys + row;
    const uint8_t *p = b.plane + 4 * row;
    pose_sets_body(a, [&](int i) { return (p[i] | p[stride + i] | p[2 * stride + i] | p[3 * stride + i]) != 0; },
                   [&](int i) { return key_train(keys[i]); }, pts);
}
template <class Points>
__device__ __forceinline__ void pose_sets_candidate(const SetsBatchArgs &b, int z, const Points &pts)
{
    pose_sets_rows(b, z, b.kp1, b.n1, (size_t)b.n1, pts);
}
// grid B: candidate blockIdx.x on the 3-D images of the two frames
__global__ __launch_bounds__(kOneWg) void pose_sets_batch(SetsBatchArgs b)
{
    const int z = blockIdx.x;
    if (b.cands.c[z].n == 0) {
        if (threadIdx.x < kNSets) b.counts[z * kNSets + threadIdx.x] = 0;
        return;
    }
    pose_sets_candidate(b, z, ImagePoints{b.xyz_a, b.cands.c[z].xyz, b.w1, b.h1, b.cands.c[z].w, b.cands.c[z].h});
}

// ------------------------------------------------------------------------------------------------ frames kept on the device
// pose_sets_batch on stored frames: the candidates' descriptors and keypoints (b.cands) point into the store, b.xyz_a and the candidates'
// xyz are null, the points are the records.  The argument block of pose_sets_batch is b unchanged.
struct SetsStoredArgs {
    SetsBatchArgs b;
    const float4 *rec_a;
    const float4 *rec[kMaxBatch];
};
__global__ __launch_bounds__(kOneWg) void pose_sets_stored_batch(SetsStoredArgs s)
{
    const int z = blockIdx.x;
    if (s.b.cands.c[z].n == 0) {
        if (threadIdx.x < kNSets) s.b.counts[z * kNSets + threadIdx.x] = 0;
        return;
    }
    pose_sets_candidate(s.b, z, RecordPoints{s.rec_a, s.rec[z]});
}
// the same for a pair list: s.b.n1 is the stride, s.b.kp1 and s.rec_a are not read, pair z has its query in qs.q[z]
struct SetsPairsArgs {
    SetsStoredArgs s;
    PairQueries qs;
};
__global__ __launch_bounds__(kOneWg) void pose_sets_stored_pairs(SetsPairsArgs p)
{
    const int z = blockIdx.x;
    if (p.s.b.cands.c[z].n == 0) {
        if (threadIdx.x < kNSets) p.s.b.counts[z * kNSets + threadIdx.x] = 0;
        return;
    }
    pose_sets_rows(p.s.b, z, p.qs.q[z].kp, p.qs.q[z].n, (size_t)p.s.b.n1, RecordPoints{p.qs.q[z].rec, p.s.rec[z]});
}

// ------------------------------------------------------------------------------------------------ GMS with scale and rotation
// gms_matcher::GetInlierMask(.., WithScale, WithRotation) (gms_matcher.cpp:17-68): run(RotationType) under SetScale(Scale) for up to
// 5 x 8 hypotheses, of which the first with the strictly largest inlier count stays.  The table and the first-maximum column search of a
// (scale, grid type) do not depend on the rotation -- only the 3 x 3 score does -- so ONE workgroup per (scale, grid type, candidate)
// builds them once and scores all eight rotations; a second kernel counts the hypotheses and applies the choice.
constexpr int kScales = 5, kRotations = 8;
// right grid side at scale index s: (int)(20 * ratio), ratios 1, 1/2, 1/sqrt(2), sqrt(2), 2 in double (gms_matcher.h:47, :230-234)
__host__ __device__ constexpr int mode_side(int s) { return s == 0 ? 20 : s == 1 ? 10 : s == 2 ? 14 : s == 3 ? 28 : 40; }
// table columns of the scales before s: the prefix sums of side^2 = 400, 100, 196, 784, 1600
__host__ __device__ constexpr int mode_cols_before(int s) { return s == 0 ? 0 : s == 1 ? 400 : s == 2 ? 500 : s == 3 ? 696 : s == 4 ? 1480 : 3080; }
// the eight outer positions of a row-major 3 x 3 neighbourhood, clockwise from the top-left, one per nibble (ring position 0 lowest):
// 0, 1, 2, 5, 8, 7, 6, 3.  Rotation type r pairs the left neighbour at ring position k with the right one at (k - (r - 1)) mod 8
// (the eight patterns of gms_matcher.h:12-44 restated), centre with centre.
constexpr uint32_t kRing = 0x36785210u;

// GetGridIndexRight under SetScale (gms_matcher.h:184-189, :230-234): floorf(p * (float)side) per axis, x + y * side, no range check on
// x or y; outside [0, side^2) the match has no right cell
__device__ __forceinline__ int mode_cell_right(float px, float py, int side)
{
    const double x = (double)floorf(px * (float)side), y = (double)floorf(py * (float)side);
    if (!(x >= -kCoordLim && x <= kCoordLim) || !(y >= -kCoordLim && y <= kCoordLim)) return -1;
    const int idx = (int)x + (int)y * side;
    return idx >= 0 && idx < side * side ? idx : -1;
}

struct GmsModesArgs {
    const float2 *kp1;
    int32_t n, w1, h1;                    // n matches per candidate
    const unsigned long long *keys;       // [B][n]: match i of candidate j = (i, train index of keys[j][i]) ...
    const int32_t *qidx, *tidx;           // ... or, when not null (B = 1), match i = (qidx[i], tidx[i])
    int32_t *table;                       // [B][S][4][400][N_s]
    uint8_t *plane;                       // [B][S][4][n]: per match the accepted-rotation bits (bit r - 1 = rotation r) of ONE (scale, grid type)
    int32_t n_scales, n_rot;              // 1 or 5, 1 or 8
    BatchCands cands;                     // kp, n, w, h of the candidates
};
// One workgroup of kOneWg threads: (scale, grid type) blockIdx.x of candidate blockIdx.y on n matches of the query keypoints kp1 (image
// w1 x h1), planes and keys in rows of `stride` (one query frame: a's own kp1, n = stride = a.n, w1, h1; a pair list: the pair's)
__device__ __forceinline__ void gms_grid_modes_body(const GmsModesArgs &a, const float2 *kp1, int n, size_t stride, int w1, int h1)
{
    __shared__ int32_t cnt[kCells];      // mNumberPointsInPerCellLeft
    __shared__ int32_t pair[kCells];     // mCellPairs before the threshold: the first column of maximal count, -1 for an empty row
    __shared__ int32_t acc[kCells];      // per left cell: bit r - 1 set iff rotation r accepts its pair
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x >> 2, type = (blockIdx.x & 3) + 1, z = blockIdx.y;
    if (a.cands.c[z].n == 0) return;                          // no matches: gms_mode_select does not read this candidate's planes
    const int side = mode_side(s), N = side * side;
    const size_t per_cand = (size_t)4 * kCells * mode_cols_before(a.n_scales);
    int32_t *table = a.table + (size_t)z * per_cand + (size_t)4 * kCells * mode_cols_before(s) + (size_t)(type - 1) * kCells * N;
    uint8_t *plane = a.plane + (((size_t)z * a.n_scales + s) * 4 + (type - 1)) * stride;
    const float2 *kp2 = a.cands.c[z].kp;
    const unsigned long long *keys = a.keys ? a.keys + (size_t)z * stride : nullptr;
    const float fw1 = (float)w1, fh1 = (float)h1, fw2 = (float)a.cands.c[z].w, fh2 = (float)a.cands.c[z].h;
    const bool listed = a.qidx != nullptr;                    // uniform
    // the cell pair of match i under this (scale, grid type); NormalizePoints (gms_matcher.h:126-139): one float division per coordinate
    const auto cells = [&](int i, int *l, int *r) {
        const float2 lp = kp1[listed ? a.qidx[i] : i], rp = kp2[listed ? a.tidx[i] : key_train(keys[i])];
        *l = gms_cell_left(__fdiv_rn(lp.x, fw1), __fdiv_rn(lp.y, fh1), type);
        *r = mode_cell_right(__fdiv_rn(rp.x, fw2), __fdiv_rn(rp.y, fh2), side);
    };
    // ---- gms_matcher.cpp:161-163 (N is a multiple of 4 and so is every table offset)
    for (int e = tid; e < kCells * N / 4; e += kOneWg) reinterpret_cast<int4 *>(table)[e] = make_int4(0, 0, 0, 0);
    for (int e = tid; e < kCells; e += kOneWg) { cnt[e] = 0; pair[e] = -1; }
    __threadfence();
    __syncthreads();
    // ---- AssignMatchPairs (:73-98)
    for (int i = tid; i < n; i += kOneWg) {
        int l, r;
        cells(i, &l, &r);
        if (l < 0 || r < 0) continue;                         // :92
        atomicAdd(&table[l * N + r], 1);                      // :94
        atomicAdd(&cnt[l], 1);                                // :95
    }
    __threadfence();
    __syncthreads();
    // ---- VerifyCellPairs, first half (:106-121), shared by the eight rotations: one wave per row over N columns
    for (int row = wave; row < kCells; row += kOneWg / 64) {
        if (cnt[row] == 0) continue;
        int bv = 0, bj = INT_MAX;
        for (int j = lane; j < N; j += 64) {
            const int v = table_load(&table[row * N + j]);
            if (v > bv) { bv = v; bj = j; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const int ov = __shfl_xor(bv, m, 64), oj = __shfl_xor(bj, m, 64);
            if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
        if (lane == 0) pair[row] = bj;
    }
    __syncthreads();
    // ---- second half (:123-146) for every (left cell, rotation) as one work item: 8 adjacent lanes hold the rotations of a cell
    for (int item = tid; item < kCells * kRotations; item += kOneWg) {   // 3200 = 3 x 1024 + 128: whole waves enter every round
        const int cell = item >> 3, rot = item & 7, pr = pair[cell];
        bool ok = false;
        if (pr >= 0 && rot < a.n_rot) {
            const int lx = cell % kGrid, ly = cell / kGrid, rx = pr % side, ry = pr / side;
            int score = table_load(&table[cell * N + pr]), tsum = cnt[cell], numpair = 1;   // centre with centre
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int lp = (int)(kRing >> (4 * k)) & 15, rp = (int)(kRing >> (4 * ((k - rot) & 7))) & 15;
                const int llx = lx + lp % 3 - 1, lly = ly + lp / 3 - 1, rrx = rx + rp % 3 - 1, rry = ry + rp / 3 - 1;
                if (llx < 0 || llx >= kGrid || lly < 0 || lly >= kGrid || rrx < 0 || rrx >= side || rry < 0 || rry >= side) continue;   // :136
                const int ll = llx + lly * kGrid;
                score += table_load(&table[ll * N + rrx + rry * side]);
                tsum += cnt[ll];
                numpair++;
            }
            const double thresh = 6.0 * sqrt((double)tsum / (double)numpair);   // :143, over the pairs that remain
            ok = !((double)score < thresh);                                       // :145-146
        }
        const unsigned long long m = __ballot(ok);
        if (rot == 0) acc[cell] = (int32_t)((m >> (lane & 56)) & 0xffull);
    }
    __syncthreads();
    // ---- mark (:169-177), for the eight rotations at once
    for (int i = tid; i < n; i += kOneWg) {
        int l, r;
        cells(i, &l, &r);
        plane[i] = l >= 0 && r >= 0 && pair[l] == r ? (uint8_t)acc[l] : (uint8_t)0;
    }
}
// grid (4 grid types x S scales, B)
__global__ __launch_bounds__(kOneWg) void gms_grid_modes(GmsModesArgs a)
{
    gms_grid_modes_body(a, a.kp1, a.n, (size_t)a.n, a.w1, a.h1);
}
// grid (4 grid types x S scales, P) on a pair list: a.n is the stride, a.kp1 / w1 / h1 are not read, a.qidx / tidx are null
struct GmsModesPairsArgs {
    GmsModesArgs a;
    PairQueries qs;
};
__global__ __launch_bounds__(kOneWg) void pairs_grid_modes(GmsModesPairsArgs p)
{
    const PairQuery &q = p.qs.q[blockIdx.y];
    gms_grid_modes_body(p.a, q.kp, q.n, (size_t)p.a.n, q.w, q.h);
}

struct GmsSelectArgs {
    const uint8_t *plane;                 // [B][S][4][n] of gms_grid_modes
    int32_t n, n_scales, n_rot;
    uint8_t *mask;                        // candidate z: n bytes (0 / 1) at mask + z * mask_stride ...
    size_t mask_stride;
    int32_t zero_slots;                   // ... followed by 3 x n zero bytes: the [B][4][n] planes pose_sets_batch ORs
    chip_gms_choice *choice;              // [B]
    int32_t live[kMaxBatch];              // 0: an empty candidate, nothing to read or write but the choice
};
// One workgroup of kOneWg threads: the counts of the S x R hypotheses of candidate blockIdx.x over its n matches, the choice
// (gms_matcher.cpp:19-33,38-48,54-66) and the winner's mask; the planes and the zeroed slots are rows of `stride` (a pair list: n is
// the pair's own count, otherwise n = stride = a.n)
__device__ __forceinline__ void gms_mode_select_body(const GmsSelectArgs &a, int n, size_t stride)
{
    __shared__ int32_t counts[kScales * kRotations];
    __shared__ int32_t win[2];
    const int tid = threadIdx.x, lane = tid & 63, z = blockIdx.x;
    const bool live = a.live[z] != 0;                        // uniform
    if (tid < kScales * kRotations) counts[tid] = (tid >> 3) < a.n_scales && (tid & 7) < a.n_rot ? 0 : -1;
    __syncthreads();
    const uint8_t *planes = a.plane + (size_t)z * a.n_scales * 4 * stride;
    for (int s = 0; live && s < a.n_scales; s++) {
        const uint8_t *p = planes + (size_t)s * 4 * stride;
        int mine[kRotations] = {0, 0, 0, 0, 0, 0, 0, 0};    // wave-uniform
        for (int base = 0; base < n; base += kOneWg) {
            const int i = base + tid;
            const int b = i < n ? p[i] | p[stride + i] | p[2 * stride + i] | p[3 * stride + i] : 0;
#pragma unroll
            for (int r = 0; r < kRotations; r++) mine[r] += __popcll(__ballot((b >> r) & 1));
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < kRotations; r++)
                if (r < a.n_rot) atomicAdd(&counts[s * kRotations + r], mine[r]);
        }
    }
    __syncthreads();
    chip_gms_choice *ch = a.choice + z;
    if (tid == 0) {                                           // scales ascending, rotations inside: the first strictly larger count stays
        int best = 0, bs = -1, br = 0;
        for (int s = 0; s < a.n_scales; s++)
            for (int r = 0; r < a.n_rot; r++)
                if (counts[s * kRotations + r] > best) { best = counts[s * kRotations + r]; bs = s; br = r + 1; }
        win[0] = bs; win[1] = br;
        ch->scale = bs; ch->rotation = br; ch->n_inliers = best;
    }
    if (tid < kScales * kRotations) ch->counts[tid >> 3][tid & 7] = counts[tid];
    __syncthreads();
    if (!live) return;
    uint8_t *out = a.mask + (size_t)z * a.mask_stride;
    const int ws = win[0], shift = ws >= 0 ? win[1] - 1 : 0;
    const uint8_t *p = planes + (size_t)(ws < 0 ? 0 : ws) * 4 * stride;
    for (int i = tid; i < n; i += kOneWg) {
        const int b = p[i] | p[stride + i] | p[2 * stride + i] | p[3 * stride + i];
        out[i] = ws >= 0 ? (uint8_t)((b >> shift) & 1) : (uint8_t)0;   // no choice: the mask is all zero
        if (a.zero_slots) out[stride + i] = out[2 * stride + i] = out[3 * stride + i] = 0;
    }
}
// grid B
__global__ __launch_bounds__(kOneWg) void gms_mode_select(GmsSelectArgs a)
{
    gms_mode_select_body(a, a.n, (size_t)a.n);
}
// grid P on a pair list: a.n is the stride, n[z] the count of pair z
struct GmsSelectPairsArgs {
    GmsSelectArgs a;
    int32_t n[kMaxBatch];
};
__global__ __launch_bounds__(kOneWg) void pairs_mode_select(GmsSelectPairsArgs p)
{
    gms_mode_select_body(p.a, p.n[blockIdx.x], (size_t)p.a.n);
}

// ------------------------------------------------------------------------------------------------ host side
struct MatchState {
    // the stand-alone calls, sized for kMatchMax keypoints once; d1 / kp1 also hold the query frame of a pipeline run, and nothing that
    // a run leaves for later calls (keys, sets, summaries) is in this group
    DevBuf<uint8_t> d1, d2;                     // d2: chip_orb_match's train descriptors
    DevBuf<unsigned long long> orb_keys;        // chip_orb_match's own keys, never the slab of a run
    DevBuf<float2> kp1, kp2;                    // kp2, qidx, tidx, inlier: chip_gms_filter's
    DevBuf<int32_t> qidx, tidx;
    DevBuf<uint8_t> inlier;
    DevBuf<int32_t> counts;                     // [kMaxBatch][kNSets] of a run; chip_gms_filter's inlier count borrows [0]
    PinnedBuf<int32_t> h_counts;
    // a pipeline run: the frames, the merged keys, one table and one plane per (candidate, grid type) and the five sets in slabs of n1
    // rows per candidate; all grown on demand (batch_reserve)
    DevBuf<float> xyz_a;
    DevBuf<uint8_t> desc;                       // candidate j at desc + 32 * (n of the candidates before it), kp alike
    DevBuf<float2> kp;
    DevBuf<float> xyz;
    DevBuf<unsigned long long> keys;
    DevBuf<int32_t> table;                      // match_state() reserves the one table of chip_gms_filter
    DevBuf<uint8_t> plane;
    DevBuf<double> uv, uv_d, X_ab, uvn_ab, X_ba, uvn_ba, A, B;
    DevBuf<int32_t> mq, mt;
    std::vector<unsigned long long> h_keys;     // fetch_matches: keys on their way out
    // GMS with scale / rotation: nothing of this exists before the first call with modes != 0 (modes_reserve)
    DevBuf<int32_t> mode_table;                 // [B][S][4][400][N_s]
    DevBuf<uint8_t> mode_plane;                 // [B][S][4][n]
    DevBuf<chip_gms_choice> mode_choice;        // [kMaxBatch]
    PinnedBuf<chip_gms_choice> h_choice;
    // (the frames a run on stored frames reads are the FrameStore's, frame_store.h)
    hipEvent_t ev[5] = {};                      // tuning only (CHIP_MATCH_BATCH_TIMING=1): around the three (with GMS modes: four) launches of a run
    // what the last run left: n_cand candidates of a query frame of n1 keypoints, of which ONE is selected -- the pointers and counts
    // chip_match_read_sets and the _matched solvers work on
    struct Sets { double *uv, *uv_d, *X_ab, *uvn_ab, *X_ba, *uvn_ba, *A, *B; int32_t *mq, *mt; };
    bool have_sets = false;
    bool keys_readable = false;                 // API behaviour, not a buffer selector: chip_match_batch_read_matches answers only after a
                                                // chip_match_batch, CHIP_ERR_BUSY after a chip_match_pair
    int32_t n_cand = 0, n1 = 0;                 // n1: the rows of a candidate's slab = the query frame's keypoints (a pair list: the most)
    int32_t cand_n1[CHIP_MATCH_MAX_BATCH] = {}; // the query keypoints of candidate j: n1, on a pair list the pair's own
    chip_match_summary cand_sm[CHIP_MATCH_MAX_BATCH] = {};
    chip_gms_choice cand_choice[CHIP_MATCH_MAX_BATCH] = {};   // of the last run, whatever its modes
    Sets cur{};
    chip_match_summary last{};                  // the selected candidate's summary

    void select(int32_t j)                      // 0 <= j < n_cand
    {
        const size_t r = (size_t)j * (size_t)n1;
        cur = Sets{uv + 2 * r, uv_d + 2 * r, X_ab + 3 * r, uvn_ab + 2 * r, X_ba + 3 * r, uvn_ba + 2 * r, A + 3 * r, B + 3 * r, mq + r, mt + r};
        last = cand_sm[j];
    }
};

void match_destroy(Ctx *c)
{
    if (c->match_state)
        for (hipEvent_t e : c->match_state->ev)
            if (e) (void)hipEventDestroy(e);
    delete c->match_state;
    c->match_state = nullptr;
}

int match_state(Ctx *c, MatchState **out)
{
    if (!c->match_state) {
        c->match_state = new (std::nothrow) MatchState();
        if (!c->match_state) return CHIP_ERR_OOM;
    }
    MatchState *st = c->match_state;
    *out = st;
    if (st->h_counts.capacity()) return CHIP_OK;   // reserved last: everything below exists
    ResidentPause paused(c);   // one pause over the group (as pnp_reserve); a call after a failure keeps what the failed one obtained
    const size_t n = kMatchMax;
    int rc = st->d1.reserve(c, n * CHIP_ORB_DESC_BYTES);
    if (rc == CHIP_OK) rc = st->d2.reserve(c, n * CHIP_ORB_DESC_BYTES);
    if (rc == CHIP_OK) rc = st->orb_keys.reserve(c, n);
    if (rc == CHIP_OK) rc = st->kp1.reserve(c, n);
    if (rc == CHIP_OK) rc = st->kp2.reserve(c, n);
    if (rc == CHIP_OK) rc = st->qidx.reserve(c, n);
    if (rc == CHIP_OK) rc = st->tidx.reserve(c, n);
    if (rc == CHIP_OK) rc = st->inlier.reserve(c, n);
    if (rc == CHIP_OK) rc = st->table.reserve(c, (size_t)kCells * kCells);
    if (rc == CHIP_OK) rc = st->counts.reserve(c, kMaxBatch * kNSets);
    if (rc == CHIP_OK) rc = st->h_counts.reserve(c, kMaxBatch * kNSets);
    return rc;
}

hipStream_t match_stream(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->query_mu);   // chip_set_stream swaps the ctx stream under this lock
    return c->s_query;
}

// n1 >= 1 queries against B candidates of at most max_n2 >= 1 train descriptors; keys [B][n1] preset to all ones
static int launch_matcher(Ctx *c, hipStream_t s, const uint8_t *query, int n1, const BatchCands &cands, int max_n2, int B, unsigned long long *keys)
{
    hipLaunchKernelGGL(hamming_match_split, dim3((n1 + kBfThreads - 1) / kBfThreads, (max_n2 + kBfTile - 1) / kBfTile, B), dim3(kBfThreads), 0, s,
                       reinterpret_cast<const uint4 *>(query), n1, cands, keys);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// n keys off the device as BFMatcher's (trainIdx, distance); all ones -> -1 / -1: no train descriptors
static int fetch_matches(Ctx *c, hipStream_t s, MatchState *st, const unsigned long long *keys, size_t n, int32_t *train_idx, int32_t *distance)
{
    st->h_keys.resize(n);
    CHIP_HIP(c, hipMemcpyAsync(st->h_keys.data(), keys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) {
        train_idx[i] = (int32_t)(uint32_t)st->h_keys[i];
        distance[i] = (int32_t)(uint32_t)(st->h_keys[i] >> 32);
    }
    return CHIP_OK;
}

int check_frame(const uint8_t *desc, const float *kp_xy, int32_t n, int32_t width, int32_t height, const void *image)
{
    if (n < 0 || width <= 0 || height <= 0 || !image) return CHIP_ERR_INVALID_ARG;
    if (n > 0 && (!desc || !kp_xy)) return CHIP_ERR_INVALID_ARG;
    if (n > kMatchMax || width > kMaxImageSide || height > kMaxImageSide) return CHIP_ERR_UNSUPPORTED;
    return CHIP_OK;
}
int check_frame(const chip_match_frame *f)
{
    return f ? check_frame(f->desc, f->kp_xy, f->n, f->width, f->height, f->xyz) : CHIP_ERR_INVALID_ARG;
}

// The buffers of a run for B candidates of a query frame of n1 keypoints; with uploads, the frames as well: tot_n keypoints and tot_px
// pixels over all candidates (a run on stored frames uploads nothing and has no such buffers).  Whatever has to grow grows inside ONE
// pause (as match_state).
static int batch_reserve(Ctx *c, MatchState *st, size_t B, size_t n1, bool uploads, size_t tot_n, size_t tot_px, size_t px_a)
{
    const size_t rows = B * n1;
    const bool frames_fit = !uploads || (st->xyz_a.capacity() >= 3 * px_a && st->desc.capacity() >= tot_n * CHIP_ORB_DESC_BYTES &&
                                         st->kp.capacity() >= tot_n && st->xyz.capacity() >= 3 * tot_px);
    const bool fits = frames_fit && st->keys.capacity() >= rows && st->table.capacity() >= B * 4 * kCells * kCells &&
                      st->plane.capacity() >= 4 * rows && st->uv.capacity() >= 2 * rows;
    if (fits) return CHIP_OK;   // the set buffers grow together with uv
    ResidentPause paused(c);
    int rc = CHIP_OK;
    if (uploads) {
        rc = st->xyz_a.reserve(c, 3 * px_a);
        if (rc == CHIP_OK) rc = st->desc.reserve(c, tot_n * CHIP_ORB_DESC_BYTES);
        if (rc == CHIP_OK) rc = st->kp.reserve(c, tot_n);
        if (rc == CHIP_OK) rc = st->xyz.reserve(c, 3 * tot_px);
    }
    if (rc == CHIP_OK) rc = st->keys.reserve(c, rows);
    if (rc == CHIP_OK) rc = st->table.reserve(c, B * 4 * kCells * kCells);
    if (rc == CHIP_OK) rc = st->plane.reserve(c, 4 * rows);
    if (rc == CHIP_OK) rc = st->uv_d.reserve(c, 2 * rows);
    if (rc == CHIP_OK) rc = st->X_ab.reserve(c, 3 * rows);
    if (rc == CHIP_OK) rc = st->uvn_ab.reserve(c, 2 * rows);
    if (rc == CHIP_OK) rc = st->X_ba.reserve(c, 3 * rows);
    if (rc == CHIP_OK) rc = st->uvn_ba.reserve(c, 2 * rows);
    if (rc == CHIP_OK) rc = st->A.reserve(c, 3 * rows);
    if (rc == CHIP_OK) rc = st->B.reserve(c, 3 * rows);
    if (rc == CHIP_OK) rc = st->mq.reserve(c, rows);
    if (rc == CHIP_OK) rc = st->mt.reserve(c, rows);
    if (rc == CHIP_OK) rc = st->uv.reserve(c, 2 * rows);   // last: its capacity stands for the whole group of set buffers
    return rc;
}

// A run's frames as the kernels see them, once their device pointers are known: uploaded host frames (xyz_a and cands.c[j].xyz, the
// image policy) or slots of the frame store (rec_a and rec[j], the record policy).  A candidate with n == 0 takes no part.
struct RunFrames {
    const uint8_t *desc_a = nullptr;
    const float2 *kp_a = nullptr;
    int32_t n1 = 0, w1 = 0, h1 = 0;
    const float *xyz_a = nullptr;
    const float4 *rec_a = nullptr;
    bool stored = false;
    BatchCands cands;
    const float4 *rec[kMaxBatch];
    int32_t max_n2 = 0;
    // a pair list (stored frames only): n1 is the stride, desc_a / kp_a / rec_a / w1 / h1 are unused and pair j has its query in qs.q[j]
    bool pairs = false;
    PairQueries qs;
    RunFrames() { std::memset(&cands, 0, sizeof cands); std::memset(rec, 0, sizeof rec); std::memset(&qs, 0, sizeof qs); }
};

// tuning only (CHIP_MATCH_BATCH_TIMING=1): device time of each kernel of a run by events, averaged, printed at process exit; runs on
// host frames, runs on stored frames and runs with GMS modes (four kernels) are kept apart
struct KernelTiming {
    const char *what;
    const char *name[4];
    int k;
    double acc[4] = {0, 0, 0, 0}; long n = 0; bool on = std::getenv("CHIP_MATCH_BATCH_TIMING") != nullptr;
    KernelTiming(const char *w, const char *sets) : what(w), name{"hamming_match_split", "gms_batch", sets, nullptr}, k(3) {}
    KernelTiming(const char *w, const char *sets, bool) : what(w), name{"hamming_match_split", "gms_grid_modes", "gms_mode_select", sets}, k(4) {}
    KernelTiming(const char *w, const char *n0, const char *n1, const char *n2, const char *n3) : what(w), name{n0, n1, n2, n3}, k(n3 ? 4 : 3) {}
    ~KernelTiming()
    {
        if (!on || !n) return;
        std::fprintf(stderr, "%s kernel timing over %ld calls (us):", what, n);
        for (int i = 0; i < k; i++) std::fprintf(stderr, "%s %s %.1f", i ? "," : "", name[i], 1e3 * acc[i] / n);
        std::fprintf(stderr, "\n");
    }
};

// What a call with no hypothesis to choose from reports (no matches at all): nothing chosen, 0 for the combinations the modes try
static void choice_none(chip_gms_choice *ch, uint32_t modes)
{
    ch->scale = -1; ch->rotation = 0; ch->n_inliers = 0;
    const int S = modes & CHIP_GMS_WITH_SCALE ? kScales : 1, R = modes & CHIP_GMS_WITH_ROTATION ? kRotations : 1;
    for (int s = 0; s < kScales; s++)
        for (int r = 0; r < kRotations; r++) ch->counts[s][r] = s < S && r < R ? 0 : -1;
}
// modes == 0: the one hypothesis (scale 0, rotation 1) with the plain count
static void choice_plain(chip_gms_choice *ch, int32_t n_inliers)
{
    choice_none(ch, 0);
    ch->scale = 0; ch->rotation = 1; ch->n_inliers = ch->counts[0][0] = n_inliers;
}

// The tables, planes and choice records of a call with modes != 0: B candidates, S scales, n matches each.  Whatever has to grow grows
// inside ONE pause (as batch_reserve); a process that never passes modes != 0 never comes here.
static int modes_reserve(Ctx *c, MatchState *st, size_t B, int S, size_t n)
{
    const size_t tab = B * 4 * kCells * (size_t)mode_cols_before(S), pl = B * (size_t)S * 4 * n;
    if (st->mode_table.capacity() >= tab && st->mode_plane.capacity() >= pl && st->h_choice.capacity()) return CHIP_OK;
    ResidentPause paused(c);
    int rc = st->mode_table.reserve(c, tab);
    if (rc == CHIP_OK) rc = st->mode_plane.reserve(c, pl);
    if (rc == CHIP_OK) rc = st->mode_choice.reserve(c, kMaxBatch);
    if (rc == CHIP_OK) rc = st->h_choice.reserve(c, kMaxBatch);
    return rc;
}
// the two launches of the mode on B candidates of n matches: ga filled but for table / plane / n_scales / n_rot.  qs: a pair list, ga.n
// is then the stride and pair j has qs->q[j].n matches
static int launch_modes(Ctx *c, MatchState *st, hipStream_t s, GmsModesArgs &ga, int B, uint32_t modes, uint8_t *mask, size_t mask_stride,
                        bool zero_slots, hipEvent_t between, const PairQueries *qs = nullptr)
{
    ga.n_scales = modes & CHIP_GMS_WITH_SCALE ? kScales : 1;
    ga.n_rot = modes & CHIP_GMS_WITH_ROTATION ? kRotations : 1;
    ga.table = st->mode_table; ga.plane = st->mode_plane;
    if (qs) {
        GmsModesPairsArgs gp;
        gp.a = ga; gp.qs = *qs;
        hipLaunchKernelGGL(pairs_grid_modes, dim3(4 * ga.n_scales, B), dim3(kOneWg), 0, s, gp);
    } else {
        hipLaunchKernelGGL(gms_grid_modes, dim3(4 * ga.n_scales, B), dim3(kOneWg), 0, s, ga);
    }
    CHIP_HIP(c, hipGetLastError());
    if (between) CHIP_HIP(c, hipEventRecord(between, s));
    GmsSelectArgs sa;
    sa.plane = st->mode_plane; sa.n = ga.n; sa.n_scales = ga.n_scales; sa.n_rot = ga.n_rot;
    sa.mask = mask; sa.mask_stride = mask_stride; sa.zero_slots = zero_slots ? 1 : 0; sa.choice = st->mode_choice;
    for (int j = 0; j < kMaxBatch; j++) sa.live[j] = j < B && ga.cands.c[j].n > 0;
    if (qs) {
        GmsSelectPairsArgs sp;
        sp.a = sa;
        for (int j = 0; j < kMaxBatch; j++) sp.n[j] = qs->q[j].n;
        hipLaunchKernelGGL(pairs_mode_select, dim3(B), dim3(kOneWg), 0, s, sp);
    } else {
        hipLaunchKernelGGL(gms_mode_select, dim3(B), dim3(kOneWg), 0, s, sa);
    }
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

// The device part of a run, for both kinds of frames (f.n1 >= 1, the slabs reserved): the keys preset, three launches (with GMS modes
// four: gms_grid_modes + gms_mode_select in the place of gms_batch), the counts back, cand_sm[0 .. B) and cand_choice[0 .. B) filled.
// A pair list (f.pairs) takes the _pairs form of every kernel: the same launches, f.n1 the stride of the rows.
static int match_launch(Ctx *c, MatchState *st, hipStream_t s, const RunFrames &f, int B, const double Kinv[9], uint32_t modes)
{
    const int n1 = f.n1;
    if (modes && f.max_n2 > 0) {
        const int rc = modes_reserve(c, st, (size_t)B, modes & CHIP_GMS_WITH_SCALE ? kScales : 1, (size_t)n1);
        if (rc != CHIP_OK) return rc;
    }
    CHIP_HIP(c, hipMemsetAsync(st->keys, 0xff, (size_t)B * n1 * sizeof(unsigned long long), s));   // all ones: no match yet
    if (f.max_n2 > 0) {
        static KernelTiming kt_host("match batch", "pose_sets_batch"), kt_stored("match batch stored", "pose_sets_stored_batch");
        static KernelTiming km_host("match batch modes", "pose_sets_batch", true), km_stored("match batch stored modes", "pose_sets_stored_batch", true);
        static KernelTiming kt_pairs("match pairs stored", "hamming_match_pairs", "pairs_gms", "pose_sets_stored_pairs", nullptr);
        static KernelTiming km_pairs("match pairs stored modes", "hamming_match_pairs", "pairs_grid_modes", "pairs_mode_select", "pose_sets_stored_pairs");
        KernelTiming &kt = f.pairs ? (modes ? km_pairs : kt_pairs) : modes ? (f.stored ? km_stored : km_host) : (f.stored ? kt_stored : kt_host);
        const int last = kt.k;                   // ev[last]: after the sets kernel
        if (kt.on)
            for (hipEvent_t &e : st->ev)
                if (!e) CHIP_HIP(c, hipEventCreate(&e));
        if (kt.on) CHIP_HIP(c, hipEventRecord(st->ev[0], s));
        int rc = CHIP_OK;
        if (f.pairs) {
            hipLaunchKernelGGL(hamming_match_pairs, dim3((n1 + kBfThreads - 1) / kBfThreads, (f.max_n2 + kBfTile - 1) / kBfTile, B), dim3(kBfThreads), 0,
                               s, f.qs, f.cands, n1, st->keys.get());
            CHIP_HIP(c, hipGetLastError());
        } else {
            rc = launch_matcher(c, s, f.desc_a, n1, f.cands, f.max_n2, B, st->keys);
            if (rc != CHIP_OK) return rc;
        }
        if (kt.on) CHIP_HIP(c, hipEventRecord(st->ev[1], s));
        if (modes) {                             // the winner's mask goes where gms_batch's planes go: slot 0 the mask, slots 1-3 zero
            GmsModesArgs ma;
            ma.kp1 = f.kp_a; ma.n = n1; ma.w1 = f.w1; ma.h1 = f.h1; ma.keys = st->keys; ma.qidx = ma.tidx = nullptr; ma.cands = f.cands;
            rc = launch_modes(c, st, s, ma, B, modes, st->plane, 4 * (size_t)n1, true, kt.on ? st->ev[2] : nullptr, f.pairs ? &f.qs : nullptr);
            if (rc != CHIP_OK) return rc;
        } else if (f.pairs) {
            GmsPairsArgs ga;
            ga.keys = st->keys; ga.table = st->table; ga.plane = st->plane; ga.stride = n1; ga.qs = f.qs; ga.cands = f.cands;
            hipLaunchKernelGGL(pairs_gms, dim3(4, B), dim3(kOneWg), 0, s, ga);
            CHIP_HIP(c, hipGetLastError());
        } else {
            GmsBatchArgs ga;
            ga.kp1 = f.kp_a; ga.n1 = n1; ga.w1 = f.w1; ga.h1 = f.h1; ga.keys = st->keys; ga.table = st->table; ga.plane = st->plane;
            ga.cands = f.cands;
            hipLaunchKernelGGL(gms_batch, dim3(4, B), dim3(kOneWg), 0, s, ga);
            CHIP_HIP(c, hipGetLastError());
        }
        if (kt.on) CHIP_HIP(c, hipEventRecord(st->ev[last - 1], s));
        SetsStoredArgs ss;
        SetsBatchArgs &sa = ss.b;
        sa.kp1 = f.kp_a; sa.xyz_a = f.xyz_a; sa.n1 = n1; sa.w1 = f.w1; sa.h1 = f.h1; sa.keys = st->keys; sa.plane = st->plane;
        for (int i = 0; i < 9; i++) sa.Kinv[i] = Kinv[i];
        sa.uv = st->uv; sa.uv_d = st->uv_d; sa.X_ab = st->X_ab; sa.uvn_ab = st->uvn_ab; sa.X_ba = st->X_ba; sa.uvn_ba = st->uvn_ba;
        sa.A = st->A; sa.B = st->B; sa.mq = st->mq; sa.mt = st->mt; sa.counts = st->counts; sa.cands = f.cands;
        if (f.stored) {
            ss.rec_a = f.rec_a;
            for (int j = 0; j < kMaxBatch; j++) ss.rec[j] = f.rec[j];
            if (f.pairs) {
                SetsPairsArgs sp;
                sp.s = ss; sp.qs = f.qs;
                hipLaunchKernelGGL(pose_sets_stored_pairs, dim3(B), dim3(kOneWg), 0, s, sp);
            } else {
                hipLaunchKernelGGL(pose_sets_stored_batch, dim3(B), dim3(kOneWg), 0, s, ss);
            }
        } else {
            hipLaunchKernelGGL(pose_sets_batch, dim3(B), dim3(kOneWg), 0, s, sa);
        }
        CHIP_HIP(c, hipGetLastError());
        if (kt.on) CHIP_HIP(c, hipEventRecord(st->ev[last], s));
        CHIP_HIP(c, hipMemcpyAsync(st->h_counts.host(), st->counts, (size_t)B * kNSets * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (modes) CHIP_HIP(c, hipMemcpyAsync(st->h_choice.host(), st->mode_choice, (size_t)B * sizeof(chip_gms_choice), hipMemcpyDeviceToHost, s));
        CHIP_HIP(c, hipStreamSynchronize(s));
        for (int k = 0; k < last && kt.on; k++) {
            float ms = 0.f;
            CHIP_HIP(c, hipEventElapsedTime(&ms, st->ev[k], st->ev[k + 1]));
            kt.acc[k] += ms;
        }
        kt.n += kt.on;
    }
    CHIP_HIP(c, hipStreamSynchronize(s));
    for (int j = 0; j < B && f.max_n2 > 0; j++) {
        if (f.cands.c[j].n == 0) continue;
        const int32_t *h = st->h_counts.host() + j * kNSets;
        if (modes) st->cand_choice[j] = st->h_choice.host()[j];
        else choice_plain(&st->cand_choice[j], h[kSetUv]);
        chip_match_summary &sm = st->cand_sm[j];
        sm.n_matches_all = f.pairs ? f.qs.q[j].n : n1;
        sm.n_matches_gms = h[kSetUv]; sm.n_3d2d_ab = h[kSetAb]; sm.n_3d2d_ba = h[kSetBa]; sm.n_3d3d = h[kSet33]; sm.n_out_of_image = h[kSetOut];
    }
    return CHIP_OK;
}

// what every run leaves: B candidates of a query frame of n1 keypoints, candidate 0 selected
static void match_finish(MatchState *st, int B, int n1)
{
    st->n_cand = B;
    st->n1 = n1;
    for (int j = 0; j < B; j++) st->cand_n1[j] = n1;
    st->select(0);
    st->have_sets = true;
}

// The pipeline on host frames: frame a against the candidates b[0 .. B) -- uploads, three launches, the counts back -- leaves the keys and
// the five sets of every candidate in its slab, cand_sm[0 .. B) filled and candidate 0 selected.  match_mu held, the arguments checked,
// have_sets false.
static int match_run(Ctx *c, MatchState *st, const chip_match_frame *a, const chip_match_frame *b, int B, const double Kinv[9], uint32_t modes = 0)
{
    int rc0 = icp_wait_matched(c);               // a pending matched ICP batch reads the slabs this run rewrites
    if (rc0 != CHIP_OK) return rc0;
    const int n1 = a->n;
    RunFrames f;
    size_t tot_n = 0, tot_px = 0;
    for (int j = 0; j < B; j++) {
        if (b[j].n == 0) continue;               // an empty candidate is not uploaded: no matches (BFMatcher on an empty descriptor matrix)
        f.max_n2 = b[j].n > f.max_n2 ? b[j].n : f.max_n2;
        tot_n += (size_t)b[j].n;
        tot_px += (size_t)b[j].width * b[j].height;
    }
    for (int j = 0; j < B; j++) {
        std::memset(&st->cand_sm[j], 0, sizeof(chip_match_summary));
        choice_none(&st->cand_choice[j], modes);   // what an empty query frame or candidate keeps
    }
    if (n1 > 0) {
        const size_t px_a = (size_t)a->width * a->height;
        int rc = batch_reserve(c, st, (size_t)B, (size_t)n1, true, tot_n, tot_px, px_a);
        if (rc != CHIP_OK) return rc;
        hipStream_t s = match_stream(c);
        if (f.max_n2 > 0) {
            CHIP_HIP(c, hipMemcpyAsync(st->d1, a->desc, (size_t)n1 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
            CHIP_HIP(c, hipMemcpyAsync(st->kp1, a->kp_xy, (size_t)n1 * sizeof(float2), hipMemcpyHostToDevice, s));
            CHIP_HIP(c, hipMemcpyAsync(st->xyz_a, a->xyz, 3 * px_a * sizeof(float), hipMemcpyHostToDevice, s));
            size_t off_n = 0, off_px = 0;
            for (int j = 0; j < B; j++) {
                const int n2 = b[j].n;
                if (n2 == 0) continue;
                const size_t px = (size_t)b[j].width * b[j].height;
                uint8_t *dd = st->desc + off_n * CHIP_ORB_DESC_BYTES;
                float2 *dk = st->kp + off_n;
                float *dx = st->xyz + 3 * off_px;
                CHIP_HIP(c, hipMemcpyAsync(dd, b[j].desc, (size_t)n2 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
                CHIP_HIP(c, hipMemcpyAsync(dk, b[j].kp_xy, (size_t)n2 * sizeof(float2), hipMemcpyHostToDevice, s));
                CHIP_HIP(c, hipMemcpyAsync(dx, b[j].xyz, 3 * px * sizeof(float), hipMemcpyHostToDevice, s));
                f.cands.c[j] = BatchCand{reinterpret_cast<const uint4 *>(dd), dk, dx, n2, b[j].width, b[j].height, 0};
                off_n += (size_t)n2; off_px += px;
            }
        }
        f.desc_a = st->d1; f.kp_a = st->kp1; f.n1 = n1; f.w1 = a->width; f.h1 = a->height; f.xyz_a = st->xyz_a;
        rc = match_launch(c, st, s, f, B, Kinv, modes);
        if (rc != CHIP_OK) return rc;
    }
    match_finish(st, B, n1);
    return CHIP_OK;
}

// The pipeline on stored frames: slot sa against the slots sb[0 .. B), nothing uploaded.  Same state afterwards as match_run.
static int match_run_stored(Ctx *c, MatchState *st, const FrameStore *fs, int32_t sa, const int32_t *sb, int B, const double Kinv[9], uint32_t modes)
{
    int rc0 = icp_wait_matched(c);               // as match_run
    if (rc0 != CHIP_OK) return rc0;
    const FrameStore::Rows a = fs->rows(sa);
    RunFrames f;
    f.stored = true;
    for (int j = 0; j < B; j++) {
        const FrameStore::Rows b = fs->rows(sb[j]);
        std::memset(&st->cand_sm[j], 0, sizeof(chip_match_summary));
        choice_none(&st->cand_choice[j], modes);
        if (b.n == 0) continue;
        f.max_n2 = b.n > f.max_n2 ? b.n : f.max_n2;
        f.cands.c[j] = BatchCand{reinterpret_cast<const uint4 *>(b.desc), b.kp, nullptr, b.n, b.w, b.h, 0};
        f.rec[j] = b.rec;
    }
    if (a.n > 0) {
        int rc = batch_reserve(c, st, (size_t)B, (size_t)a.n, false, 0, 0, 0);
        if (rc != CHIP_OK) return rc;
        f.desc_a = a.desc; f.kp_a = a.kp; f.rec_a = a.rec;
        f.n1 = a.n; f.w1 = a.w; f.h1 = a.h;
        rc = match_launch(c, st, match_stream(c), f, B, Kinv, modes);
        if (rc != CHIP_OK) return rc;
    }
    match_finish(st, B, a.n);
    return CHIP_OK;
}

// The pipeline on a list of stored pairs: slot sa[j] against slot sb[j], every pair with a query frame of its own, in the same three
// (four) launches.  The rows of keys, planes and slabs have the stride of the widest query frame; a pair with an empty frame on either
// side takes no part.  Same state afterwards as match_run, with the pair index in the place of the candidate's.
static int match_run_pairs_stored(Ctx *c, MatchState *st, const FrameStore *fs, const int32_t *sa, const int32_t *sb, int P, const double Kinv[9],
                                  uint32_t modes)
{
    int rc0 = icp_wait_matched(c);               // as match_run
    if (rc0 != CHIP_OK) return rc0;
    RunFrames f;
    f.stored = f.pairs = true;
    int32_t n_a[kMaxBatch];
    for (int j = 0; j < P; j++) {
        const FrameStore::Rows a = fs->rows(sa[j]), b = fs->rows(sb[j]);
        std::memset(&st->cand_sm[j], 0, sizeof(chip_match_summary));
        choice_none(&st->cand_choice[j], modes);
        n_a[j] = a.n;
        f.n1 = a.n > f.n1 ? a.n : f.n1;          // the stride counts an empty candidate's query too: its keys are readable (all -1)
        if (a.n == 0 || b.n == 0) continue;
        f.max_n2 = b.n > f.max_n2 ? b.n : f.max_n2;
        f.qs.q[j] = PairQuery{reinterpret_cast<const uint4 *>(a.desc), a.kp, a.rec, a.n, a.w, a.h, 0};
        f.cands.c[j] = BatchCand{reinterpret_cast<const uint4 *>(b.desc), b.kp, nullptr, b.n, b.w, b.h, 0};
        f.rec[j] = b.rec;
    }
    if (f.n1 > 0) {
        int rc = batch_reserve(c, st, (size_t)P, (size_t)f.n1, false, 0, 0, 0);
        if (rc != CHIP_OK) return rc;
        rc = match_launch(c, st, match_stream(c), f, P, Kinv, modes);
        if (rc != CHIP_OK) return rc;
    }
    match_finish(st, P, f.n1);
    for (int j = 0; j < P; j++) st->cand_n1[j] = n_a[j];
    return CHIP_OK;
}

}  // namespace chip

using namespace chip;

extern "C" int chip_build_has_match(void) { return 1; }

extern "C" int chip_orb_match(chip_ctx *c, const uint8_t *d1, int32_t n1, const uint8_t *d2, int32_t n2, int32_t *train_idx, int32_t *distance)
{
    if (!c || n1 < 0 || n2 < 0 || (n1 > 0 && (!d1 || !train_idx || !distance)) || (n2 > 0 && !d2)) return CHIP_ERR_INVALID_ARG;
    if (c->group || n1 > kMatchMax || n2 > kMatchMax) return CHIP_ERR_UNSUPPORTED;
    if (n1 == 0) return CHIP_OK;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    MatchState *st = nullptr;
    int rc = match_state(c, &st);
    if (rc != CHIP_OK) return rc;
    hipStream_t s = match_stream(c);
    CHIP_HIP(c, hipMemsetAsync(st->orb_keys, 0xff, (size_t)n1 * sizeof(unsigned long long), s));   // all ones: no match yet
    if (n2 > 0) {
        CHIP_HIP(c, hipMemcpyAsync(st->d1, d1, (size_t)n1 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(st->d2, d2, (size_t)n2 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
        BatchCands one;                        // the matcher reads desc and n of a candidate only
        std::memset(&one, 0, sizeof one);
        one.c[0].desc = reinterpret_cast<const uint4 *>(st->d2.get());
        one.c[0].n = n2;
        rc = launch_matcher(c, s, st->d1, n1, one, n2, 1, st->orb_keys);
        if (rc != CHIP_OK) return rc;
    }
    return fetch_matches(c, s, st, st->orb_keys, (size_t)n1, train_idx, distance);
}

// chip_gms_filter (modes == 0: gms_filter, one launch) and chip_gms_filter_modes (the two kernels of the mode with B = 1 on the list)
static int gms_filter_call(chip_ctx *c, const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1, const float *kp2_xy, int32_t n2, int32_t w2,
                           int32_t h2, const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches, uint32_t modes, uint8_t *inlier,
                           int32_t *n_inliers, chip_gms_choice *choice)
{
    if (modes & ~(uint32_t)(CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION)) return CHIP_ERR_INVALID_ARG;
    if (!c || n1 < 0 || n2 < 0 || n_matches < 0 || w1 <= 0 || h1 <= 0 || w2 <= 0 || h2 <= 0 || !n_inliers) return CHIP_ERR_INVALID_ARG;
    if ((n1 > 0 && !kp1_xy) || (n2 > 0 && !kp2_xy) || (n_matches > 0 && (!query_idx || !train_idx || !inlier))) return CHIP_ERR_INVALID_ARG;
    if (c->group || n1 > kMatchMax || n2 > kMatchMax || n_matches > kMatchMax) return CHIP_ERR_UNSUPPORTED;
    for (int32_t i = 0; i < n_matches; i++)   // the kernel indexes the keypoints with these
        if (query_idx[i] < 0 || query_idx[i] >= n1 || train_idx[i] < 0 || train_idx[i] >= n2) return CHIP_ERR_RANGE;
    *n_inliers = 0;
    if (choice) choice_none(choice, modes);
    if (n_matches == 0) return CHIP_OK;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    MatchState *st = nullptr;
    int rc = match_state(c, &st);
    if (rc != CHIP_OK) return rc;
    hipStream_t s = match_stream(c);
    CHIP_HIP(c, hipMemcpyAsync(st->kp1, kp1_xy, (size_t)n1 * sizeof(float2), hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemcpyAsync(st->kp2, kp2_xy, (size_t)n2 * sizeof(float2), hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemcpyAsync(st->qidx, query_idx, (size_t)n_matches * sizeof(int32_t), hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemcpyAsync(st->tidx, train_idx, (size_t)n_matches * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (modes) {
        rc = modes_reserve(c, st, 1, modes & CHIP_GMS_WITH_SCALE ? kScales : 1, (size_t)n_matches);
        if (rc != CHIP_OK) return rc;
        GmsModesArgs ma;
        std::memset(&ma.cands, 0, sizeof ma.cands);
        ma.kp1 = st->kp1; ma.n = n_matches; ma.w1 = w1; ma.h1 = h1; ma.keys = nullptr; ma.qidx = st->qidx; ma.tidx = st->tidx;
        ma.cands.c[0].kp = st->kp2; ma.cands.c[0].n = n2; ma.cands.c[0].w = w2; ma.cands.c[0].h = h2;   // n2 >= 1: there is a match
        rc = launch_modes(c, st, s, ma, 1, modes, st->inlier, 0, false, nullptr);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipMemcpyAsync(inlier, st->inlier, (size_t)n_matches, hipMemcpyDeviceToHost, s));
        CHIP_HIP(c, hipMemcpyAsync(st->h_choice.host(), st->mode_choice, sizeof(chip_gms_choice), hipMemcpyDeviceToHost, s));
        CHIP_HIP(c, hipStreamSynchronize(s));
        *n_inliers = st->h_choice.host()[0].n_inliers;
        if (choice) *choice = st->h_choice.host()[0];
        return CHIP_OK;
    }
    GmsArgs g;
    g.kp1 = st->kp1; g.kp2 = st->kp2; g.w1 = w1; g.h1 = h1; g.w2 = w2; g.h2 = h2;
    g.qidx = st->qidx; g.tidx = st->tidx; g.n = n_matches;
    g.table = st->table; g.inlier = st->inlier; g.n_inliers = st->counts;
    hipLaunchKernelGGL(gms_filter, dim3(1), dim3(kOneWg), 0, s, g);
    CHIP_HIP(c, hipGetLastError());
    CHIP_HIP(c, hipMemcpyAsync(inlier, st->inlier, (size_t)n_matches, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipMemcpyAsync(st->h_counts.host(), st->counts, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    *n_inliers = st->h_counts.host()[0];
    if (choice) choice_plain(choice, *n_inliers);
    return CHIP_OK;
}

extern "C" int chip_gms_filter(chip_ctx *c, const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1, const float *kp2_xy, int32_t n2, int32_t w2,
                               int32_t h2, const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches, uint8_t *inlier, int32_t *n_inliers)
{
    return gms_filter_call(c, kp1_xy, n1, w1, h1, kp2_xy, n2, w2, h2, query_idx, train_idx, n_matches, 0, inlier, n_inliers, nullptr);
}

extern "C" int chip_build_has_gms_modes(void) { return 1; }

extern "C" int chip_gms_filter_modes(chip_ctx *c, const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1, const float *kp2_xy, int32_t n2,
                                     int32_t w2, int32_t h2, const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches, uint32_t modes,
                                     uint8_t *inlier, int32_t *n_inliers, chip_gms_choice *choice)
{
    return gms_filter_call(c, kp1_xy, n1, w1, h1, kp2_xy, n2, w2, h2, query_idx, train_idx, n_matches, modes, inlier, n_inliers, choice);
}

// a batch of one
extern "C" int chip_match_pair(chip_ctx *c, const chip_match_frame *a, const chip_match_frame *b, const double Kinv[9], chip_match_summary *summary)
{
    if (!c || !Kinv || !summary) return CHIP_ERR_INVALID_ARG;
    int rc = check_frame(a);
    if (rc == CHIP_OK) rc = check_frame(b);
    if (rc != CHIP_OK) return rc;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    MatchState *st = nullptr;
    rc = match_state(c, &st);
    if (rc != CHIP_OK) return rc;
    st->have_sets = false;
    rc = match_run(c, st, a, b, 1, Kinv);
    if (rc != CHIP_OK) return rc;
    st->keys_readable = false;
    *summary = st->cand_sm[0];
    return CHIP_OK;
}

extern "C" int chip_match_read_sets(chip_ctx *c, chip_match_sets_out *out)
{
    if (!c || !out) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    CHIP_HIP(c, hipSetDevice(c->device));
    hipStream_t s = match_stream(c);
    const chip_match_summary &m = st->last;
    const auto fetch = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    const size_t g = (size_t)m.n_matches_gms, ab = (size_t)m.n_3d2d_ab, ba = (size_t)m.n_3d2d_ba, dd = (size_t)m.n_3d3d;
    CHIP_HIP(c, fetch(out->uv, st->cur.uv, g * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->uv_d, st->cur.uv_d, g * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->X_ab, st->cur.X_ab, ab * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->uvn_ab, st->cur.uvn_ab, ab * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->X_ba, st->cur.X_ba, ba * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->uvn_ba, st->cur.uvn_ba, ba * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->A_3d3d, st->cur.A, dd * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->B_3d3d, st->cur.B, dd * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->match_query_idx, st->cur.mq, g * sizeof(int32_t)));
    CHIP_HIP(c, fetch(out->match_train_idx, st->cur.mt, g * sizeof(int32_t)));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

extern "C" int chip_pnp_ransac_matched(chip_ctx *c, int32_t which, const chip_ransac_params *p, double T_colmajor[16], float *confidence,
                                       uint8_t *inlier_mask, chip_ransac_summary *summary)
{
    if (!c || !p || !T_colmajor || !confidence || (which != CHIP_SET_AB && which != CHIP_SET_BA)) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    if (which == CHIP_SET_AB) return pnp_ransac_device(c, st->cur.X_ab, st->cur.uvn_ab, st->last.n_3d2d_ab, p, T_colmajor, confidence, inlier_mask, summary);
    return pnp_ransac_device(c, st->cur.X_ba, st->cur.uvn_ba, st->last.n_3d2d_ba, p, T_colmajor, confidence, inlier_mask, summary);
}

extern "C" int chip_icp_ransac_matched(chip_ctx *c, const chip_ransac_params *p, double T_colmajor[16], float *confidence, uint8_t *inlier_mask,
                                       chip_ransac_summary *summary)
{
    if (!c || !p || !T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    return icp_ransac_device(c, st->cur.A, st->cur.B, st->last.n_3d3d, p, T_colmajor, confidence, inlier_mask, summary);
}

// ------------------------------------------------------------------------------------------------ one query frame against B candidates
extern "C" int chip_build_has_match_batch(void) { return 1; }

static int match_batch_call(chip_ctx *c, const chip_match_frame *a, const chip_match_frame *b, int32_t B, const double Kinv[9], uint32_t modes,
                            chip_match_summary *summary, chip_gms_choice *choice)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    if (c->match_state) c->match_state->have_sets = false;   // a failed call, refused arguments included, leaves nothing selected
    if (!a || !b || !Kinv || !summary || B < 1 || (modes & ~(uint32_t)(CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION))) return CHIP_ERR_INVALID_ARG;
    if (B > kMaxBatch) return CHIP_ERR_UNSUPPORTED;
    int rc = check_frame(a);
    for (int j = 0; j < B && rc == CHIP_OK; j++) rc = check_frame(&b[j]);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipSetDevice(c->device));
    MatchState *st = nullptr;
    rc = match_state(c, &st);
    if (rc != CHIP_OK) return rc;
    st->have_sets = false;
    rc = match_run(c, st, a, b, B, Kinv, modes);
    if (rc != CHIP_OK) return rc;
    st->keys_readable = true;
    for (int j = 0; j < B; j++) summary[j] = st->cand_sm[j];
    for (int j = 0; j < B && choice; j++) choice[j] = st->cand_choice[j];
    return CHIP_OK;
}

extern "C" int chip_match_batch(chip_ctx *c, const chip_match_frame *a, const chip_match_frame *b, int32_t B, const double Kinv[9],
                                chip_match_summary *summary)
{
    return match_batch_call(c, a, b, B, Kinv, 0, summary, nullptr);
}

extern "C" int chip_match_batch_modes(chip_ctx *c, const chip_match_frame *a, const chip_match_frame *b, int32_t B, const double Kinv[9],
                                      uint32_t modes, chip_match_summary *summary, chip_gms_choice *choice)
{
    return match_batch_call(c, a, b, B, Kinv, modes, summary, choice);
}

extern "C" int chip_match_select(chip_ctx *c, int32_t j)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    if (j < 0 || j >= st->n_cand) return CHIP_ERR_RANGE;
    st->select(j);
    return CHIP_OK;
}

extern "C" int chip_match_batch_read_matches(chip_ctx *c, int32_t j, int32_t *train_idx, int32_t *distance)
{
    if (!c || !train_idx || !distance) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets || !st->keys_readable) return CHIP_ERR_BUSY;   // not after a chip_match_pair
    if (j < 0 || j >= st->n_cand) return CHIP_ERR_RANGE;
    const size_t n = (size_t)st->cand_n1[j];    // of the row's st->n1
    if (n == 0) return CHIP_OK;
    CHIP_HIP(c, hipSetDevice(c->device));
    return fetch_matches(c, match_stream(c), st, st->keys + (size_t)j * (size_t)st->n1, n, train_idx, distance);
}

extern "C" int chip_pnp_ransac_matched_batch(chip_ctx *c, int32_t P, const int32_t *cand, const int32_t *which, const chip_ransac_params *p,
                                             const uint64_t *seeds, double *T_colmajor, float *confidence, uint8_t *const *inlier_mask,
                                             chip_ransac_summary *summary, int32_t *status)
{
    if (!c || P < 0 || !p || (P > 0 && (!cand || !which || !T_colmajor || !confidence || !status))) return CHIP_ERR_INVALID_ARG;
    for (int i = 0; i < P; i++)
        if (which[i] != CHIP_SET_AB && which[i] != CHIP_SET_BA) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    for (int i = 0; i < P; i++)
        if (cand[i] < 0 || cand[i] >= st->n_cand) return CHIP_ERR_RANGE;
    // the runnable problems, gathered: their slab pointers, seeds and masks; the others are answered here
    std::vector<const double *> X, uv;
    std::vector<int32_t> N, at;
    std::vector<uint64_t> sd;
    std::vector<uint8_t *> masks;
    const MatchState::Sets keep = st->cur;
    const chip_match_summary keep_sm = st->last;
    for (int i = 0; i < P; i++) {
        st->select(cand[i]);
        const bool ab = which[i] == CHIP_SET_AB;
        const int32_t n = ab ? st->last.n_3d2d_ab : st->last.n_3d2d_ba;
        status[i] = ransac_check_params(p, n);
        if (status[i] != CHIP_OK) {
            for (int k = 0; k < 16; k++) T_colmajor[16 * (size_t)i + k] = NAN;
            confidence[i] = -1.f;
            if (summary) { std::memset(&summary[i], 0, sizeof summary[i]); summary[i].best_hypothesis = -1; }
            continue;
        }
        X.push_back(ab ? st->cur.X_ab : st->cur.X_ba);
        uv.push_back(ab ? st->cur.uvn_ab : st->cur.uvn_ba);
        N.push_back(n); at.push_back(i);
        sd.push_back(seeds ? seeds[i] : p->seed);
        masks.push_back(inlier_mask ? inlier_mask[i] : nullptr);
    }
    st->cur = keep; st->last = keep_sm;          // the selection is chip_match_select's alone
    const int R = (int)at.size();
    if (R == 0) return CHIP_OK;
    std::vector<double> T(16 * (size_t)R);
    std::vector<float> conf((size_t)R);
    std::vector<chip_ransac_summary> summ((size_t)R);
    const int rc = pnp_ransac_device_batch(c, R, X.data(), uv.data(), N.data(), p, sd.data(), T.data(), conf.data(), masks.data(), summ.data());
    if (rc != CHIP_OK) return rc;
    for (int r = 0; r < R; r++) {
        std::memcpy(T_colmajor + 16 * (size_t)at[r], T.data() + 16 * (size_t)r, 16 * sizeof(double));
        confidence[at[r]] = conf[r];
        if (summary) summary[at[r]] = summ[r];
    }
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ ICP on the sets of several candidates
extern "C" int chip_icp_ransac_matched_batch_enqueue(chip_ctx *c, int32_t P, const int32_t *cand, const chip_ransac_params *p, const uint64_t *seeds,
                                                     int32_t *status)
{
    if (!c || P < 1 || !cand || !p || !status) return CHIP_ERR_INVALID_ARG;
    if (P > CHIP_ICP_MAX_BATCH) return CHIP_ERR_UNSUPPORTED;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    for (int i = 0; i < P; i++)
        if (cand[i] < 0 || cand[i] >= st->n_cand) return CHIP_ERR_RANGE;
    // the runnable problems, gathered: their slab pointers, counts and seeds, read in place; the selection is not touched
    const double *A[CHIP_ICP_MAX_BATCH], *B[CHIP_ICP_MAX_BATCH];
    int32_t N[CHIP_ICP_MAX_BATCH], at[CHIP_ICP_MAX_BATCH];
    uint64_t sd[CHIP_ICP_MAX_BATCH];
    int R = 0;
    for (int i = 0; i < P; i++) {
        const int32_t n = st->cand_sm[cand[i]].n_3d3d;
        status[i] = ransac_check_params(p, n);
        if (status[i] != CHIP_OK) continue;       // left out of the launch; the collect gives it the left-out answer
        const size_t r = (size_t)cand[i] * (size_t)st->n1;
        A[R] = st->A + 3 * r; B[R] = st->B + 3 * r;
        N[R] = n; at[R] = i; sd[R] = seeds ? seeds[i] : p->seed;
        R++;
    }
    return icp_enqueue_device_batch(c, R, A, B, N, p, sd, P, at);
}

extern "C" int chip_icp_ransac_matched_batch(chip_ctx *c, int32_t P, const int32_t *cand, const chip_ransac_params *p, const uint64_t *seeds,
                                             double *T_colmajor, float *confidence, uint8_t *const *inlier_mask, chip_ransac_summary *summary,
                                             int32_t *status)
{
    if (!T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    const int rc = chip_icp_ransac_matched_batch_enqueue(c, P, cand, p, seeds, status);
    if (rc != CHIP_OK) return rc;
    return chip_icp_ransac_matched_batch_collect(c, T_colmajor, confidence, inlier_mask, summary);
}

// ------------------------------------------------------------------------------------------------ one stored frame against B stored candidates
// (the store itself -- reserve, the puts, drop, read -- is frames.hip; chip_frame_store_reserve creates the match state with it)
static int match_batch_stored_call(chip_ctx *c, int64_t a_id, const int64_t *b_ids, int32_t B, const double Kinv[9], uint32_t modes,
                                   chip_match_summary *summary, chip_gms_choice *choice)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    const FrameStore *fs = c->frame_store;
    if (st) st->have_sets = false;           // a failed call, refused arguments included, leaves nothing selected
    if (!b_ids || !Kinv || !summary || B < 1 || (modes & ~(uint32_t)(CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION))) return CHIP_ERR_INVALID_ARG;
    if (B > kMaxBatch) return CHIP_ERR_UNSUPPORTED;
    if (!st || !fs || fs->n_slots == 0) return CHIP_ERR_BUSY;
    int32_t sb[kMaxBatch];
    const auto fa = fs->slot_of.find(a_id);
    if (fa == fs->slot_of.end()) return CHIP_ERR_RANGE;
    for (int j = 0; j < B; j++) {
        const auto fb = fs->slot_of.find(b_ids[j]);
        if (fb == fs->slot_of.end()) return CHIP_ERR_RANGE;
        sb[j] = fb->second;
    }
    CHIP_HIP(c, hipSetDevice(c->device));
    const int rc = match_run_stored(c, st, fs, fa->second, sb, B, Kinv, modes);
    if (rc != CHIP_OK) return rc;
    st->keys_readable = true;
    for (int j = 0; j < B; j++) summary[j] = st->cand_sm[j];
    for (int j = 0; j < B && choice; j++) choice[j] = st->cand_choice[j];
    return CHIP_OK;
}

extern "C" int chip_match_batch_stored(chip_ctx *c, int64_t a_id, const int64_t *b_ids, int32_t B, const double Kinv[9], chip_match_summary *summary)
{
    return match_batch_stored_call(c, a_id, b_ids, B, Kinv, 0, summary, nullptr);
}

extern "C" int chip_match_batch_stored_modes(chip_ctx *c, int64_t a_id, const int64_t *b_ids, int32_t B, const double Kinv[9], uint32_t modes,
                                             chip_match_summary *summary, chip_gms_choice *choice)
{
    return match_batch_stored_call(c, a_id, b_ids, B, Kinv, modes, summary, choice);
}

// ------------------------------------------------------------------------------------------------ a list of stored pairs
extern "C" int chip_build_has_match_pairs(void) { return 1; }

extern "C" int chip_match_pairs_stored(chip_ctx *c, const int64_t *a_ids, const int64_t *b_ids, int32_t P, const double Kinv[9], uint32_t modes,
                                       chip_match_summary *summary, chip_gms_choice *choice)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    const FrameStore *fs = c->frame_store;
    if (st) st->have_sets = false;           // a failed call, refused arguments included, leaves nothing selected
    if (!a_ids || !b_ids || !Kinv || !summary || P < 1 || (modes & ~(uint32_t)(CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION))) return CHIP_ERR_INVALID_ARG;
    if (P > CHIP_MATCH_MAX_PAIRS) return CHIP_ERR_UNSUPPORTED;
    if (!st || !fs || fs->n_slots == 0) return CHIP_ERR_BUSY;
    int32_t sa[kMaxBatch], sb[kMaxBatch];
    for (int j = 0; j < P; j++) {
        const auto fa = fs->slot_of.find(a_ids[j]), fb = fs->slot_of.find(b_ids[j]);
        if (fa == fs->slot_of.end() || fb == fs->slot_of.end()) return CHIP_ERR_RANGE;
        sa[j] = fa->second; sb[j] = fb->second;
    }
    CHIP_HIP(c, hipSetDevice(c->device));
    const int rc = match_run_pairs_stored(c, st, fs, sa, sb, P, Kinv, modes);
    if (rc != CHIP_OK) return rc;
    st->keys_readable = true;
    for (int j = 0; j < P; j++) summary[j] = st->cand_sm[j];
    for (int j = 0; j < P && choice; j++) choice[j] = st->cand_choice[j];
    return CHIP_OK;
}
