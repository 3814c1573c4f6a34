// match.hip -- the candidate verification front end on gfx950: what the reference's loop-candidate consumer runs per candidate between
// the descriptor scan and the three pose solves (include/cerebro_hip.h, "candidate verification front end", has the definitions):
//
//   orb_bf_match    : cv::BFMatcher(NORM_HAMMING).match(d1, d2) (src/utils/PointFeatureMatching.cpp:38-41).  One query descriptor per
//                     lane in 8 VGPRs, the train descriptors staged through LDS in tiles of 1024 (32 KiB); every lane of a wave reads the
//                     SAME LDS address (a broadcast, conflict-free), xor + popcount, running (distance, index) per lane; the scan goes
//                     in index order with a strict <, so ties keep the lowest train index.  One launch, ceil(n1 / 256) workgroups.
//   gms_filter      : gms_matcher::GetInlierMask(.., false, false) (src/utils/GMSMatcher/gms_matcher.cpp:9-15 -> run(1), :150-181) in ONE
//                     workgroup: per grid type 1..4 (:158) the 400 x 400 motion-statistics table (global scratch of the ctx; integer
//                     atomicAdd, order-independent) and the per-left-cell counts (LDS) of AssignMatchPairs (:73-98), then
//                     VerifyCellPairs (:100-148, rotation pattern 1 = identity) with one wave per table row for the first-maximum
//                     search and one lane per left cell for the 3 x 3 score against 6 * sqrt(mean count), then the inlier marks (:169-177).
//   pose_sets_build : MiscUtils::dmatch_2_eigen (src/utils/MiscUtils.cpp:121-143) + the two make_3d_2d_collection__ calls and
//                     make_3d_3d_collection__using__pfmatches_and_disparity (PointFeatureMatching.cpp:95-195) as ONE ordered stream
//                     compaction (ballot + prefix popcount per wave, scan across the 16 waves): outputs are in match order, in the
//                     layout pnp.hip / icp.hip take.
//
// Nothing here rounds twice: float division / multiplication, the float -> double widenings, fp64 add / multiply / divide / sqrt are
// single IEEE operations (-ffp-contract=off), the rest is integer.  tests/np_mirror_match.py restates all of it in numpy and
// tests/test_match_gpu.py compares byte for byte.
#include "chip_internal.h"
#include <climits>
#include <cstring>
#include <new>

namespace chip {

constexpr int kMatchMax = CHIP_MATCH_MAX_KEYPOINTS;
constexpr int kBfThreads = 256;
constexpr int kBfTile = 1024;            // train descriptors per LDS tile: 1024 x 32 B = 32 KiB
constexpr int kGrid = 20;                // mGridSizeLeft = Size(20, 20) (gms_matcher.h:62); right grid = left x the scale ratio of index 0 = 1.0 (:46, :230-231)
constexpr int kCells = kGrid * kGrid;    // 400
constexpr int kOneWg = 1024;             // gms_filter / pose_sets_build: one workgroup of 16 waves
constexpr int kMaxImageSide = 16384;

// ------------------------------------------------------------------------------------------------ orb_bf_match
__global__ __launch_bounds__(kBfThreads) void orb_bf_match(const uint4 *__restrict__ query, int n1, const uint4 *__restrict__ train, int n2,
                                                           int32_t *__restrict__ train_idx, int32_t *__restrict__ distance)
{
    __shared__ uint4 tile[2 * kBfTile];
    const int i = blockIdx.x * kBfThreads + threadIdx.x;
    const int qi = i < n1 ? i : n1 - 1;                       // n1 >= 1: the tail lanes scan a valid descriptor and store nothing
    const uint4 q0 = query[2 * (size_t)qi], q1 = query[2 * (size_t)qi + 1];
    int best = INT_MAX, bidx = -1;
    for (int base = 0; base < n2; base += kBfTile) {
        const int cnt = n2 - base < kBfTile ? n2 - base : kBfTile;
        __syncthreads();                                      // the previous tile has been read by every wave
        for (int e = threadIdx.x; e < 2 * cnt; e += kBfThreads) tile[e] = train[2 * (size_t)base + e];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const uint4 a = tile[2 * j], b = tile[2 * j + 1];  // wave-uniform address: one broadcast read
            const int d = __popc(q0.x ^ a.x) + __popc(q0.y ^ a.y) + __popc(q0.z ^ a.z) + __popc(q0.w ^ a.w) +
                          __popc(q1.x ^ b.x) + __popc(q1.y ^ b.y) + __popc(q1.z ^ b.z) + __popc(q1.w ^ b.w);
            if (d < best) { best = d; bidx = base + j; }      // strict: the first minimum stays
        }
    }
    if (i < n1) { train_idx[i] = bidx; distance[i] = bidx >= 0 ? best : -1; }
}

// ------------------------------------------------------------------------------------------------ gms_filter
struct GmsArgs {
    const float2 *kp1, *kp2;
    int32_t w1, h1, w2, h2;
    const int32_t *qidx;        // nullptr: match i is (i, tidx[i]) -- the output of orb_bf_match
    const int32_t *tidx;
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

__global__ __launch_bounds__(kOneWg) void gms_filter(GmsArgs a)
{
    __shared__ int32_t cnt[kCells];      // mNumberPointsInPerCellLeft
    __shared__ int32_t pair[kCells];     // mCellPairs
    __shared__ int32_t total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float fw1 = (float)a.w1, fh1 = (float)a.h1, fw2 = (float)a.w2, fh2 = (float)a.h2;
    if (tid == 0) total = 0;
    for (int i = tid; i < a.n; i += kOneWg) a.inlier[i] = 0;   // mvbInlierMask.assign(false) (gms_matcher.cpp:152); own bytes, same lane later
    for (int type = 1; type <= 4; type++) {                   // :158
        // ---- :161-163
        for (int e = tid; e < kCells * kCells / 4; e += kOneWg) reinterpret_cast<int4 *>(a.table)[e] = make_int4(0, 0, 0, 0);
        for (int e = tid; e < kCells; e += kOneWg) { cnt[e] = 0; pair[e] = -1; }
        __threadfence();
        __syncthreads();
        // ---- AssignMatchPairs (:73-98); NormalizePoints (gms_matcher.h:126-139): float / int -> one float division
        for (int i = tid; i < a.n; i += kOneWg) {
            const float2 lp = a.kp1[a.qidx ? a.qidx[i] : i], rp = a.kp2[a.tidx[i]];
            const int l = gms_cell_left(__fdiv_rn(lp.x, fw1), __fdiv_rn(lp.y, fh1), type);
            const int r = gms_cell_right(__fdiv_rn(rp.x, fw2), __fdiv_rn(rp.y, fh2));
            if (l < 0 || r < 0) continue;                     // :92
            atomicAdd(&a.table[l * kCells + r], 1);           // :94
            atomicAdd(&cnt[l], 1);                            // :95
        }
        __threadfence();
        __syncthreads();
        // ---- VerifyCellPairs, first half (:106-121): per non-empty row the first column of maximal count.  One wave per row.
        for (int row = wave; row < kCells; row += kOneWg / 64) {
            if (cnt[row] == 0) continue;                      // sum(row) == 0 (:106): every increment of the row also counted in cnt
            int bv = 0, bj = INT_MAX;
            for (int j = lane; j < kCells; j += 64) {
                const int v = table_load(&a.table[row * kCells + j]);
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
                    score += table_load(&a.table[ll * kCells + rr]);
                    tsum += cnt[ll];
                    numpair++;
                }
            const double thresh = 6.0 * sqrt((double)tsum / (double)numpair);   // THRESH_FACTOR (gms_matcher.h:9), :143
            if ((double)score < thresh) pair[tid] = -2;                            // :145-146 (only this lane reads pair[tid] before the barrier)
        }
        __syncthreads();
        // ---- mark (:169-177)
        for (int i = tid; i < a.n; i += kOneWg) {
            const float2 lp = a.kp1[a.qidx ? a.qidx[i] : i], rp = a.kp2[a.tidx[i]];
            const int l = gms_cell_left(__fdiv_rn(lp.x, fw1), __fdiv_rn(lp.y, fh1), type);
            const int r = gms_cell_right(__fdiv_rn(rp.x, fw2), __fdiv_rn(rp.y, fh2));
            if (l >= 0 && r >= 0 && pair[l] == r) a.inlier[i] = 1;
        }
        __syncthreads();                                      // pair / cnt are rewritten by the next pass
    }
    int mine = 0;
    for (int i = tid; i < a.n; i += kOneWg) mine += a.inlier[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    if (lane == 0) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) *a.n_inliers = total;                       // :179
}

// ------------------------------------------------------------------------------------------------ pose_sets_build
enum { kSetUv = 0, kSetAb = 1, kSetBa = 2, kSet33 = 3, kSetOut = 4, kNSets = 5 };
struct SetsArgs {
    const float2 *kp1, *kp2;
    const int32_t *tidx;          // match i = (i, tidx[i])
    const uint8_t *inlier;
    int32_t n;
    const float *xyz_a, *xyz_b;   // H x W x 3
    int32_t w1, h1, w2, h2;
    double Kinv[9];               // row-major
    double *uv, *uv_d, *X_ab, *uvn_ab, *X_ba, *uvn_ba, *A, *B;
    int32_t *mq, *mt;
    int32_t *counts;              // [kNSets]: n_matches_gms, n_3d2d_ab, n_3d2d_ba, n_3d3d, n_out_of_image
};

// pixel of a keypoint as the reference indexes the 3-D image: (int)uv(1,k), (int)uv(0,k) (PointFeatureMatching.cpp:121,180) -- truncation
// of the float keypoint (exact as a double).  (-1, w) truncates into [0, w - 1]; anything else (NaN too) is outside the image.
__device__ __forceinline__ bool pixel_of(float2 p, int w, int h, int *x, int *y)
{
    if (!(p.x > -1.0f && p.x < (float)w && p.y > -1.0f && p.y < (float)h)) return false;
    *x = (int)p.x; *y = (int)p.y;
    return true;
}
// the depth gate of :122 / :182: "z < 0.1 || z > 25." with the float z widened to double
__device__ __forceinline__ bool depth_ok(float z) { return !((double)z < 0.1 || (double)z > 25.); }

__global__ __launch_bounds__(kOneWg) void pose_sets_build(SetsArgs a)
{
    __shared__ int32_t wtot[kNSets][kOneWg / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run[kNSets] = {0, 0, 0, 0, 0};
    for (int base = 0; base < a.n; base += kOneWg) {
        const int i = base + tid;
        bool f[kNSets] = {false, false, false, false, false};
        float2 pa = make_float2(0.f, 0.f), pb = pa;
        int t = 0;
        size_t oa = 0, ob = 0;
        if (i < a.n && a.inlier[i]) {
            t = a.tidx[i];
            pa = a.kp1[i]; pb = a.kp2[t];
            int xa, ya, xb, yb;
            const bool in_a = pixel_of(pa, a.w1, a.h1, &xa, &ya), in_b = pixel_of(pb, a.w2, a.h2, &xb, &yb);
            bool za = false, zb = false;
            if (in_a) { oa = 3 * ((size_t)ya * a.w1 + xa); za = depth_ok(a.xyz_a[oa + 2]); }
            if (in_b) { ob = 3 * ((size_t)yb * a.w2 + xb); zb = depth_ok(a.xyz_b[ob + 2]); }
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
            for (int k = 0; k < 3; k++) a.X_ab[3 * o + k] = (double)a.xyz_a[oa + k];
            a.uvn_ab[2 * o] = (a.Kinv[0] * ub + a.Kinv[1] * vb) + a.Kinv[2];
            a.uvn_ab[2 * o + 1] = (a.Kinv[3] * ub + a.Kinv[4] * vb) + a.Kinv[5];
        }
        if (f[kSetBa]) {                                      // make_3d_2d(uv_d, b_3dImage, uv) (Cerebro.cpp:1566)
            const int o = pos[kSetBa];
            for (int k = 0; k < 3; k++) a.X_ba[3 * o + k] = (double)a.xyz_b[ob + k];
            a.uvn_ba[2 * o] = (a.Kinv[0] * ua + a.Kinv[1] * va) + a.Kinv[2];
            a.uvn_ba[2 * o + 1] = (a.Kinv[3] * ua + a.Kinv[4] * va) + a.Kinv[5];
        }
        if (f[kSet33]) {                                      // make_3d_3d (Cerebro.cpp:1624)
            const int o = pos[kSet33];
            for (int k = 0; k < 3; k++) { a.A[3 * o + k] = (double)a.xyz_a[oa + k]; a.B[3 * o + k] = (double)a.xyz_b[ob + k]; }
        }
    }
    if (tid < kNSets) a.counts[tid] = run[tid];
}

// ------------------------------------------------------------------------------------------------ host side
struct MatchState {
    // inputs / intermediates, sized for kMatchMax keypoints once
    DevBuf<uint8_t> d1, d2;
    DevBuf<float2> kp1, kp2;
    DevBuf<int32_t> qidx, tidx, dist, table, counts;
    DevBuf<uint8_t> inlier;
    // the five sets chip_match_pair leaves on the device
    DevBuf<double> uv, uv_d, X_ab, uvn_ab, X_ba, uvn_ba, A, B;
    DevBuf<int32_t> mq, mt;
    DevBuf<float> xyz_a, xyz_b;                 // grown on demand
    PinnedBuf<int32_t> h_counts;
    bool have_sets = false;
    chip_match_summary last{};
};

void match_destroy(Ctx *c)
{
    delete c->match_state;
    c->match_state = nullptr;
}

static int match_state(Ctx *c, MatchState **out)
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
    if (rc == CHIP_OK) rc = st->kp1.reserve(c, n);
    if (rc == CHIP_OK) rc = st->kp2.reserve(c, n);
    if (rc == CHIP_OK) rc = st->qidx.reserve(c, n);
    if (rc == CHIP_OK) rc = st->tidx.reserve(c, n);
    if (rc == CHIP_OK) rc = st->dist.reserve(c, n);
    if (rc == CHIP_OK) rc = st->table.reserve(c, (size_t)kCells * kCells);
    if (rc == CHIP_OK) rc = st->counts.reserve(c, 8);
    if (rc == CHIP_OK) rc = st->inlier.reserve(c, n);
    if (rc == CHIP_OK) rc = st->uv.reserve(c, n * 2);
    if (rc == CHIP_OK) rc = st->uv_d.reserve(c, n * 2);
    if (rc == CHIP_OK) rc = st->X_ab.reserve(c, n * 3);
    if (rc == CHIP_OK) rc = st->uvn_ab.reserve(c, n * 2);
    if (rc == CHIP_OK) rc = st->X_ba.reserve(c, n * 3);
    if (rc == CHIP_OK) rc = st->uvn_ba.reserve(c, n * 2);
    if (rc == CHIP_OK) rc = st->A.reserve(c, n * 3);
    if (rc == CHIP_OK) rc = st->B.reserve(c, n * 3);
    if (rc == CHIP_OK) rc = st->mq.reserve(c, n);
    if (rc == CHIP_OK) rc = st->mt.reserve(c, n);
    if (rc == CHIP_OK) rc = st->h_counts.reserve(c, 8);
    return rc;
}

static hipStream_t match_stream(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->query_mu);   // chip_set_stream swaps the ctx stream under this lock
    return c->s_query;
}

static int launch_bf(Ctx *c, hipStream_t s, MatchState *st, int n1, int n2)
{
    hipLaunchKernelGGL(orb_bf_match, dim3((n1 + kBfThreads - 1) / kBfThreads), dim3(kBfThreads), 0, s,
                       reinterpret_cast<const uint4 *>(st->d1.get()), n1, reinterpret_cast<const uint4 *>(st->d2.get()), n2, st->tidx.get(), st->dist.get());
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

static int launch_gms(Ctx *c, hipStream_t s, MatchState *st, bool identity_queries, int n, int w1, int h1, int w2, int h2)
{
    GmsArgs g;
    g.kp1 = st->kp1; g.kp2 = st->kp2; g.w1 = w1; g.h1 = h1; g.w2 = w2; g.h2 = h2;
    g.qidx = identity_queries ? nullptr : st->qidx; g.tidx = st->tidx; g.n = n;
    g.table = st->table; g.inlier = st->inlier; g.n_inliers = st->counts + 7;
    hipLaunchKernelGGL(gms_filter, dim3(1), dim3(kOneWg), 0, s, g);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

static int check_frame(const chip_match_frame *f)
{
    if (!f || f->n < 0 || f->width <= 0 || f->height <= 0 || !f->xyz) return CHIP_ERR_INVALID_ARG;
    if (f->n > 0 && (!f->desc || !f->kp_xy)) return CHIP_ERR_INVALID_ARG;
    if (f->n > kMatchMax || f->width > kMaxImageSide || f->height > kMaxImageSide) return CHIP_ERR_UNSUPPORTED;
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
    CHIP_HIP(c, hipMemcpyAsync(st->d1, d1, (size_t)n1 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
    if (n2 > 0) CHIP_HIP(c, hipMemcpyAsync(st->d2, d2, (size_t)n2 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
    rc = launch_bf(c, s, st, n1, n2);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemcpyAsync(train_idx, st->tidx, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipMemcpyAsync(distance, st->dist, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

extern "C" int chip_gms_filter(chip_ctx *c, const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1, const float *kp2_xy, int32_t n2, int32_t w2,
                               int32_t h2, const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches, uint8_t *inlier, int32_t *n_inliers)
{
    if (!c || n1 < 0 || n2 < 0 || n_matches < 0 || w1 <= 0 || h1 <= 0 || w2 <= 0 || h2 <= 0 || !n_inliers) return CHIP_ERR_INVALID_ARG;
    if ((n1 > 0 && !kp1_xy) || (n2 > 0 && !kp2_xy) || (n_matches > 0 && (!query_idx || !train_idx || !inlier))) return CHIP_ERR_INVALID_ARG;
    if (c->group || n1 > kMatchMax || n2 > kMatchMax || n_matches > kMatchMax) return CHIP_ERR_UNSUPPORTED;
    for (int32_t i = 0; i < n_matches; i++)   // the kernel indexes the keypoints with these
        if (query_idx[i] < 0 || query_idx[i] >= n1 || train_idx[i] < 0 || train_idx[i] >= n2) return CHIP_ERR_RANGE;
    *n_inliers = 0;
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
    rc = launch_gms(c, s, st, false, n_matches, w1, h1, w2, h2);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemcpyAsync(inlier, st->inlier, (size_t)n_matches, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipMemcpyAsync(st->h_counts.host(), st->counts + 7, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    *n_inliers = st->h_counts.host()[0];
    return CHIP_OK;
}

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
    chip_match_summary sm;
    std::memset(&sm, 0, sizeof sm);
    const int n1 = a->n, n2 = b->n;
    if (n1 > 0 && n2 > 0) {                    // an empty train set gives no matches (BFMatcher on an empty descriptor matrix)
        const size_t fa = 3 * (size_t)a->width * a->height, fb = 3 * (size_t)b->width * b->height;
        rc = st->xyz_a.reserve(c, fa);
        if (rc == CHIP_OK) rc = st->xyz_b.reserve(c, fb);
        if (rc != CHIP_OK) return rc;
        hipStream_t s = match_stream(c);
        CHIP_HIP(c, hipMemcpyAsync(st->d1, a->desc, (size_t)n1 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(st->d2, b->desc, (size_t)n2 * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(st->kp1, a->kp_xy, (size_t)n1 * sizeof(float2), hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(st->kp2, b->kp_xy, (size_t)n2 * sizeof(float2), hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(st->xyz_a, a->xyz, fa * sizeof(float), hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(st->xyz_b, b->xyz, fb * sizeof(float), hipMemcpyHostToDevice, s));
        rc = launch_bf(c, s, st, n1, n2);
        if (rc == CHIP_OK) rc = launch_gms(c, s, st, true, n1, a->width, a->height, b->width, b->height);
        if (rc != CHIP_OK) return rc;
        SetsArgs sa;
        sa.kp1 = st->kp1; sa.kp2 = st->kp2; sa.tidx = st->tidx; sa.inlier = st->inlier; sa.n = n1;
        sa.xyz_a = st->xyz_a; sa.xyz_b = st->xyz_b; sa.w1 = a->width; sa.h1 = a->height; sa.w2 = b->width; sa.h2 = b->height;
        for (int i = 0; i < 9; i++) sa.Kinv[i] = Kinv[i];
        sa.uv = st->uv; sa.uv_d = st->uv_d; sa.X_ab = st->X_ab; sa.uvn_ab = st->uvn_ab; sa.X_ba = st->X_ba; sa.uvn_ba = st->uvn_ba;
        sa.A = st->A; sa.B = st->B; sa.mq = st->mq; sa.mt = st->mt; sa.counts = st->counts;
        hipLaunchKernelGGL(pose_sets_build, dim3(1), dim3(kOneWg), 0, s, sa);
        CHIP_HIP(c, hipGetLastError());
        CHIP_HIP(c, hipMemcpyAsync(st->h_counts.host(), st->counts, kNSets * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CHIP_HIP(c, hipStreamSynchronize(s));
        sm.n_matches_all = n1;
        sm.n_matches_gms = st->h_counts.host()[kSetUv];
        sm.n_3d2d_ab = st->h_counts.host()[kSetAb];
        sm.n_3d2d_ba = st->h_counts.host()[kSetBa];
        sm.n_3d3d = st->h_counts.host()[kSet33];
        sm.n_out_of_image = st->h_counts.host()[kSetOut];
    }
    st->last = sm;
    st->have_sets = true;
    *summary = sm;
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
    CHIP_HIP(c, fetch(out->uv, st->uv, g * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->uv_d, st->uv_d, g * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->X_ab, st->X_ab, ab * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->uvn_ab, st->uvn_ab, ab * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->X_ba, st->X_ba, ba * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->uvn_ba, st->uvn_ba, ba * 2 * sizeof(double)));
    CHIP_HIP(c, fetch(out->A_3d3d, st->A, dd * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->B_3d3d, st->B, dd * 3 * sizeof(double)));
    CHIP_HIP(c, fetch(out->match_query_idx, st->mq, g * sizeof(int32_t)));
    CHIP_HIP(c, fetch(out->match_train_idx, st->mt, g * sizeof(int32_t)));
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
    if (which == CHIP_SET_AB) return pnp_ransac_device(c, st->X_ab, st->uvn_ab, st->last.n_3d2d_ab, p, T_colmajor, confidence, inlier_mask, summary);
    return pnp_ransac_device(c, st->X_ba, st->uvn_ba, st->last.n_3d2d_ba, p, T_colmajor, confidence, inlier_mask, summary);
}

extern "C" int chip_icp_ransac_matched(chip_ctx *c, const chip_ransac_params *p, double T_colmajor[16], float *confidence, uint8_t *inlier_mask,
                                       chip_ransac_summary *summary)
{
    if (!c || !p || !T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    MatchState *st = c->match_state;
    if (!st || !st->have_sets) return CHIP_ERR_BUSY;
    return icp_ransac_device(c, st->A, st->B, st->last.n_3d3d, p, T_colmajor, confidence, inlier_mask, summary);
}
