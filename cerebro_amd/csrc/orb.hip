// orb.hip -- the detector half of ORB on gfx950: what cv::ORB::create(5000) with setFastThreshold(0) does before it describes
// (src/utils/PointFeatureMatching.cpp:16-22).  include/cerebro_hip.h, "ORB keypoint detection on the device", has the definition; it is
// this project's own, all-integer, and restated in tests/np_mirror_orb_detect.py, which the device equals bit for bit.
//
//   orb_pyramid    : level l from level l - 1, fixed-point bilinear at pixel centres.  One launch per level above 0 (a level needs the one
//                    before); a thread makes four pixels of a row and stores one dword.
//   orb_fast_score : all levels in one launch (level = blockIdx.z).  A workgroup stages 22 rows x 136 bytes (a tile of 128 x 16 pixels with
//                    its halo of 3, rows as whole dwords) in LDS; a thread reads 7 rows x 4 dwords, makes the score of eight pixels (16
//                    differences, the nine-wide cyclic minimum and maximum by doubling: 2, 4, 8, 8 + 1) and stores them as one 16-byte store.
//   orb_candidates : all levels (blockIdx.y).  A workgroup owns a strip of two rows of the detection rectangle: threshold and 3 x 3 strict
//                    maximum, ordered compaction (ballot + prefix popcount, running base across the waves) of the survivors' raster
//                    indices into LDS, then the 7 x 7 Harris sums for the survivors only, one per thread.  A strip holds at most one strict
//                    maximum per 2 x 2 block, which bounds its segment of the level's candidate list; the strip's count goes next to it.
//   orb_select     : one workgroup per level.  Scan of the strip counts, the segments closed up in place into one list in raster order (a
//                    bisection in LDS per candidate, once), radix select of the quota-th largest R (8 bits a pass, LDS histogram, four
//                    loads in flight), then one ordered pass that keeps R > R* and the first ties in raster order.  Writes the kept list
//                    at the level's quota prefix and the kept count.
//   orb_moments    : one wave per kept keypoint over all levels: the level of output i from the eight kept counts, the 31 rows of the
//                    patch as aligned dwords, one wave reduction, two 16-byte stores per record.
//
//
// ... and the descriptor half ("ORB descriptors on the device" in the header; tests/np_mirror_orb_describe.py), after orb_moments on the
// same stream, only in a describing call (chip_orb_detect_describe, chip_frame_put_orb_stereo):
//   orb_blur       : all levels in one launch (level = blockIdx.z).  A workgroup stages 38 rows x 136 bytes (a tile of 128 x 32 pixels with
//                    its halo of 3, rows as whole dwords, the clamps applied while staging) in LDS, makes the 16-bit horizontal sums of
//                    the 38 rows into a second LDS plane, then a thread sums seven rows for 16 pixels and stores them as one 16-byte store
//                    (the blurred planes have a pitch of their own, a multiple of 16).
//   orb_describe   : one wave per kept keypoint: the bin from the record's moments (lanes 0 .. 31 one int64 product sum each, one wave
//                    reduction), the lane's four steered pairs in one 16-byte load, eight byte gathers, four ballots, two 16-byte stores.
//
// Every kernel has a batch entry fb_<stage> for the batched frame puts (frames.hip put_orb_stereo_batch): the same body on the bases of
// one of up to 16 frames, the frame taken from the grid, its scratch at frame x stride in the same buffers (orb_batch_enqueue).
//
// Nothing returns to the host between the stages; the records and the eight counts leave in ONE copy at the end (the descriptors of
// chip_orb_detect_describe in one more).
#include "chip_internal.h"
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

namespace chip {

constexpr int kOrbLevels = CHIP_ORB_MAX_LEVELS;
constexpr int kOrbMaxSide = CHIP_ORB_MAX_SIDE;
constexpr int kOrbThreads = 256;
constexpr int kScoreTileW = 128, kScoreTileH = 16;       // pixels of a score tile: 16 x 16 threads of eight pixels in a row each
constexpr int kScoreLdsRows = kScoreTileH + 6;           // 22
constexpr int kScoreLdsPairs = (kScoreTileW + 8) / 8;    // 17 uint2 a row: the tile's columns - 4 .. + 131
constexpr int kStripRows = 2;
constexpr int kStripMaxCand = (kOrbMaxSide - 32 + 1) / 2;   // 2032: one strict maximum per 2 x 2 block, border >= 16
constexpr int kMaxStrips = (kOrbMaxSide - 32 + 1) / 2;      // 2032 strips of two rows
constexpr int kSelectThreads = 1024;
static_assert(kMaxStrips <= 2 * kSelectThreads, "orb_select scans two strips a thread");
constexpr int kOutHeader = 32;                           // bytes: the eight kept counts in front of the records

struct OrbLevel {
    int32_t w, h, pitch, spitch;       // image row pitch in bytes (a multiple of 4), score row pitch in elements (a multiple of 8)
    int32_t x0, y0, x1, y1;            // detection rectangle, empty: x1 < x0
    int32_t quota, qprefix;            // kept list of the level: [qprefix, qprefix + quota)
    int32_t cap, nstrips;              // candidate segment of a strip, strips of the level
    uint32_t img_off, score_off, cand_off, strip_off;   // into the ctx's buffers, in elements
    double scale;
};
struct OrbTable {
    int32_t n_levels, n_features, threshold, pad;
    OrbLevel l[kOrbLevels];
};
struct OrbCand { long long R; int32_t raster, pad; };    // 16 bytes
struct OrbArgs {
    uint8_t *img;
    int16_t *score;
    OrbCand *cand;
    int32_t *strip_count;
    OrbCand *kept;
    uint8_t *out;                      // kOutHeader bytes of counts, then the records
    OrbTable t;
};
// The frame axis of a batched put (chip_frame_put_orb_stereo_batch): frame f of a group has its scratch at f * stride behind frame 0's, in
// elements of each buffer.  The element offsets of OrbLevel stay per frame.
constexpr int kOrbGroup = kFramePutGroup;
struct OrbStrides { size_t img, score, cand, strip, kept, out; };
struct OrbBatchArgs { OrbArgs a; OrbStrides f; };

// ------------------------------------------------------------------------------------------------ orb_pyramid
__device__ __forceinline__ void orb_axis(int x, int n_src, int n_dst, int *i0, int *i1, uint32_t *frac)
{
    long long X = ((long long)(2 * x + 1) * n_src * 1024) / n_dst - 1024;
    const long long hi = (long long)(n_src - 1) * 2048;
    X = X < 0 ? 0 : (X > hi ? hi : X);
    *i0 = (int)(X >> 11);
    *frac = (uint32_t)(X & 2047);
    *i1 = min(*i0 + 1, n_src - 1);
}
// Every stage has ONE body, a __device__ function on the bases of its frame, and two entries: the single call's kernel (frame 0) and the
// batched put's (fb_*: the frame from the grid, its bases at frame x stride).
__device__ __forceinline__ void pyramid_frame(const OrbTable &t, uint8_t *img, int lv)
{
    const OrbLevel &d = t.l[lv], &s = t.l[lv - 1];
    const int xq = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (4 * xq >= d.w || y >= d.h) return;
    const uint8_t *src = img + s.img_off;
    int y0, y1;
    uint32_t b;
    orb_axis(y, s.h, d.h, &y0, &y1, &b);
    const uint8_t *r0 = src + (size_t)y0 * s.pitch, *r1 = src + (size_t)y1 * s.pitch;
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = min(4 * xq + i, d.w - 1);           // the pad bytes of a row repeat its last pixel
        int x0, x1;
        uint32_t f;
        orb_axis(x, s.w, d.w, &x0, &x1, &f);
        const uint32_t v = (r0[x0] * (2048u - f) * (2048u - b) + r0[x1] * f * (2048u - b) + r1[x0] * (2048u - f) * b + r1[x1] * f * b +
                            (1u << 21)) >> 22;
        packed |= v << (8 * i);
    }
    *reinterpret_cast<uint32_t *>(img + d.img_off + (size_t)y * d.pitch + 4 * xq) = packed;
}
// grid (ceil(pitch / 4 / 64), ceil(h / 4)), block (64, 4): level lv from level lv - 1
__global__ __launch_bounds__(kOrbThreads) void orb_pyramid(OrbArgs a, int lv) { pyramid_frame(a.t, a.img, lv); }
// the same grid x frames (blockIdx.z)
__global__ __launch_bounds__(kOrbThreads) void fb_pyramid(OrbBatchArgs g, int lv) { pyramid_frame(g.a.t, g.a.img + blockIdx.z * g.f.img, lv); }

// ------------------------------------------------------------------------------------------------ orb_fast_score
// byte c (0 .. 15) of the four dwords of a row
#define ORB_BYTE(r, c) (int)(((r)[(c) >> 2] >> (8 * ((c) & 3))) & 255u)
__device__ __forceinline__ void fast_score_frame(const OrbTable &t, const uint8_t *img0, int16_t *score, int lv)
{
    __shared__ uint2 tile[kScoreLdsRows][kScoreLdsPairs];
    const OrbLevel &L = t.l[lv];
    const int tx0 = blockIdx.x * kScoreTileW, ty0 = blockIdx.y * kScoreTileH;
    if (tx0 >= L.spitch || ty0 >= L.h) return;            // wave-uniform: the whole workgroup leaves
    const uint8_t *img = img0 + L.img_off;
    uint32_t *flat = reinterpret_cast<uint32_t *>(&tile[0][0]);
    for (int i = threadIdx.x; i < kScoreLdsRows * 2 * kScoreLdsPairs; i += kOrbThreads) {
        const int r = i / (2 * kScoreLdsPairs), cq = i - r * (2 * kScoreLdsPairs);
        const int gy = ty0 - 3 + r, gx = tx0 - 4 + 4 * cq;
        uint32_t v = 0;
        if (gy >= 0 && gy < L.h && gx >= 0 && gx < L.pitch) v = *reinterpret_cast<const uint32_t *>(img + (size_t)gy * L.pitch + gx);
        flat[i] = v;
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = tx0 + 8 * lx, y = ty0 + ly;
    if (x >= L.spitch || y >= L.h) return;
    uint32_t rows[7][4];                                  // rows y - 3 .. y + 3, columns x - 4 .. x + 11
#pragma unroll
    for (int r = 0; r < 7; r++) {
        const uint2 p = tile[ly + r][lx], q = tile[ly + r][lx + 1];
        rows[r][0] = p.x; rows[r][1] = p.y; rows[r][2] = q.x; rows[r][3] = q.y;
    }
    constexpr int ring_dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int ring_dy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    uint32_t packed[4];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int ip = ORB_BYTE(rows[3], 4 + i);
        int d[16], lo[16], hi[16], t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = ORB_BYTE(rows[3 + ring_dy[k]], 4 + i + ring_dx[k]) - ip;
        // minimum and maximum over the nine ring pixels k .. k + 8, for every k: windows of 2, 4, 8, then the ninth
#pragma unroll
        for (int k = 0; k < 16; k++) { lo[k] = min(d[k], d[(k + 1) & 15]); hi[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = min(lo[k], lo[(k + 2) & 15]);
#pragma unroll
        for (int k = 0; k < 16; k++) lo[k] = min(t[k], t[(k + 4) & 15]);
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = max(hi[k], hi[(k + 2) & 15]);
#pragma unroll
        for (int k = 0; k < 16; k++) hi[k] = max(t[k], t[(k + 4) & 15]);
        int b = -256, dk = 256;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            b = max(b, min(lo[k], d[(k + 8) & 15]));      // brighter: the largest arc minimum of I_k - I_p
            dk = min(dk, max(hi[k], d[(k + 8) & 15]));    // darker: I_p - I_k, so minus the smallest arc maximum
        }
        int S = max(b, -dk) - 1;
        const int px = x + i;
        if (px < 3 || px > L.w - 4 || y < 3 || y > L.h - 4) S = -256;
        const uint32_t s16 = (uint32_t)S & 0xffffu;
        if (i & 1) packed[i >> 1] |= s16 << 16; else packed[i >> 1] = s16;
    }
    *reinterpret_cast<uint4 *>(score + L.score_off + (size_t)y * L.spitch + x) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
}
// grid (tiles in x of the widest level, tiles in y of the tallest, n_levels), block 256
__global__ __launch_bounds__(kOrbThreads) void orb_fast_score(OrbArgs a) { fast_score_frame(a.t, a.img, a.score, blockIdx.z); }
// grid z = level + n_levels * frame
__global__ __launch_bounds__(kOrbThreads) void fb_fast_score(OrbBatchArgs g)
{
    const int f = blockIdx.z / g.a.t.n_levels;
    fast_score_frame(g.a.t, g.a.img + f * g.f.img, g.a.score + f * g.f.score, blockIdx.z - f * g.a.t.n_levels);
}

// ------------------------------------------------------------------------------------------------ orb_candidates
__device__ __forceinline__ long long orb_harris(const uint8_t *img, int pitch, int x, int y)
{
    int a = 0, bb = 0, c = 0;
    for (int dy = -3; dy <= 3; dy++) {
        const uint8_t *m = img + (size_t)(y + dy) * pitch + x, *u = m - pitch, *d = m + pitch;
        for (int dx = -3; dx <= 3; dx++) {
            const int ul = u[dx - 1], uc = u[dx], ur = u[dx + 1], ml = m[dx - 1], mr = m[dx + 1], dl = d[dx - 1], dc = d[dx], dr = d[dx + 1];
            const int ix = 2 * (mr - ml) + (ur - ul) + (dr - dl);
            const int iy = 2 * (dc - uc) + (dl - ul) + (dr - ur);
            a += ix * ix; bb += iy * iy; c += ix * iy;
        }
    }
    const long long A = a, B = bb, C = c;
    return 25 * (A * B - C * C) - (A + B) * (A + B);
}
// grid (strips of the level with the most, n_levels), block 256.  The body is orb_candidates_body.inc (see there why it is text).
__global__ __launch_bounds__(kOrbThreads) void orb_candidates(OrbArgs a)
{
#define ORB_FRAME(p, which) (p)
#include "orb_candidates_body.inc"
#undef ORB_FRAME
}
// the same grid x frames (blockIdx.z)
__global__ __launch_bounds__(kOrbThreads) void fb_candidates(OrbBatchArgs g)
{
    const OrbArgs &a = g.a;
#define ORB_FRAME(p, which) ((p) + (size_t)blockIdx.z * g.f.which)
#include "orb_candidates_body.inc"
#undef ORB_FRAME
}

// ------------------------------------------------------------------------------------------------ orb_select
// exclusive sum of v over the threads of the workgroup in thread order, and the total; scratch: one int per wave
__device__ __forceinline__ int orb_block_excl(int v, int32_t *scratch, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(inc, off); if (lane >= off) inc += t; }
    __syncthreads();                                      // the scratch of the call before has been read
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kSelectThreads / 64; w++) { const int n = scratch[w]; all += n; if (w < wave) before += n; }
    *total = all;
    return before + inc - v;
}
__device__ __forceinline__ void select_frame(const OrbTable &t, OrbCand *cand0, const int32_t *strip_count, OrbCand *kept0, uint8_t *out)
{
    __shared__ int32_t start[2 * kSelectThreads + 1];     // start[s]: candidates of the level before strip s (kMaxStrips <= 2048)
    __shared__ __align__(16) int32_t hist[256];
    __shared__ int32_t scratch[kSelectThreads / 64];
    __shared__ unsigned long long sel_prefix;
    __shared__ int32_t sel_k;
    const int lv = blockIdx.x, tid = threadIdx.x;
    const OrbLevel &L = t.l[lv];
    int32_t *counts_out = reinterpret_cast<int32_t *>(out);
    if (lv >= t.n_levels) { if (tid == 0) counts_out[lv] = 0; return; }
    const int32_t *sn = strip_count + L.strip_off;
    int C;
    {   // scan of the strip counts, two strips a thread
        const int s = 2 * tid;
        const int c0 = s < L.nstrips ? sn[s] : 0, c1 = s + 1 < L.nstrips ? sn[s + 1] : 0;
        const int e = orb_block_excl(c0 + c1, scratch, &C);
        start[s] = e;
        start[s + 1] = e + c0;
        if (tid == kSelectThreads - 1) start[2 * kSelectThreads] = C;
        __syncthreads();
    }
    OrbCand *cand = cand0 + L.cand_off;
    uint4 *flat = reinterpret_cast<uint4 *>(cand);
    // The segments close up in place, so that candidate g of the level in raster order is entry g: 1024 at a time, each found by a
    // bisection over the strip ranges, read, and after a barrier written.  Entry g never lies behind its source, a chunk writes
    // [g0, g0 + 1024) and the sources of every later chunk lie at or behind g0 + 1024, so nothing unread is overwritten.
    for (int g0 = 0; g0 < C; g0 += kSelectThreads) {
        const int g = g0 + tid;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (g < C) {
            int lo = 0, hi = L.nstrips;                   // start[lo] <= g < start[hi]
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (start[mid] <= g) lo = mid; else hi = mid; }
            raw = flat[(size_t)lo * L.cap + (g - start[lo])];
        }
        __syncthreads();
        if (g < C) flat[g] = raw;
    }
    __syncthreads();
    const bool all = C <= L.quota;
    unsigned long long star = 0;                          // key of R*: R with the sign bit flipped, so that unsigned order is R's
    int need = 0;                                         // ties of R* to keep
    if (!all) {
        if (tid == 0) { sel_prefix = 0; sel_k = L.quota; }
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned long long prefix = sel_prefix;
            for (int g = tid; g < C; g += 4 * kSelectThreads) {           // four loads in flight
                unsigned long long key[4];
#pragma unroll
                for (int j = 0; j < 4; j++) key[j] = (unsigned long long)cand[min(g + j * kSelectThreads, C - 1)].R ^ 0x8000000000000000ull;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (g + j * kSelectThreads < C && (shift == 56 || (key[j] >> (shift + 8)) == (prefix >> (shift + 8))))
                        atomicAdd(&hist[(int)((key[j] >> shift) & 255)], 1);
            }
            __syncthreads();
            if (tid < 64) {                               // the bin of the k-th largest among the keys that share the prefix: four bins a lane
                const int4 h = *reinterpret_cast<const int4 *>(&hist[4 * tid]);
                const int mine = h.x + h.y + h.z + h.w, k = sel_k;
                int from_here = mine;                     // keys in the bins of this lane and of the lanes above
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_down(from_here, off); if (tid + off < 64) from_here += t; }
                const int above = from_here - mine;
                const bool holds = above < k && k <= from_here;
                if (__ballot(holds) == 0ull) {            // k == 0 (a quota of 0): nothing is kept, whatever the bin
                    if (tid == 0) sel_prefix = prefix | (255ull << shift);
                } else if (holds) {
                    int kk = k - above, bin = 3;
                    if (h.w < kk) { kk -= h.w; bin = 2; if (h.z < kk) { kk -= h.z; bin = 1; if (h.y < kk) { kk -= h.y; bin = 0; } } }
                    sel_prefix = prefix | ((unsigned long long)(4 * tid + bin) << shift);
                    sel_k = kk;
                }
            }
            __syncthreads();
        }
        star = sel_prefix;
        need = sel_k;
    }
    uint4 *kept = reinterpret_cast<uint4 *>(kept0 + L.qprefix);
    int n_kept = 0, n_ties = 0;
    for (int g0 = 0; g0 < C; g0 += kSelectThreads) {
        const int g = g0 + tid;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        bool keep = false, tie = false;
        if (g < C) {
            raw = flat[g];
            const unsigned long long key = (((unsigned long long)raw.y << 32) | raw.x) ^ 0x8000000000000000ull;
            keep = all || key > star;
            tie = !all && key == star;
        }
        int ties_here, kept_here;
        const int tie_rank = orb_block_excl(tie ? 1 : 0, scratch, &ties_here);
        if (tie && n_ties + tie_rank < need) keep = true;
        const int pos = orb_block_excl(keep ? 1 : 0, scratch, &kept_here);
        if (keep && n_kept + pos < L.quota) kept[n_kept + pos] = raw;
        n_ties += ties_here;
        n_kept += kept_here;
    }
    if (tid == 0) counts_out[lv] = min(n_kept, L.quota);
}
// grid CHIP_ORB_MAX_LEVELS, block 1024
__global__ __launch_bounds__(kSelectThreads) void orb_select(OrbArgs a) { select_frame(a.t, a.cand, a.strip_count, a.kept, a.out); }
// grid (CHIP_ORB_MAX_LEVELS, frames): still one workgroup per (level, frame)
__global__ __launch_bounds__(kSelectThreads) void fb_select(OrbBatchArgs g)
{
    const size_t f = blockIdx.y;
    select_frame(g.a.t, g.a.cand + f * g.f.cand, g.a.strip_count + f * g.f.strip, g.a.kept + f * g.f.kept, g.a.out + f * g.f.out);
}

// ------------------------------------------------------------------------------------------------ orb_moments
__device__ __forceinline__ void moments_frame(const OrbTable &t, const uint8_t *img0, const OrbCand *kept, uint8_t *out)
{
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kOrbThreads / 64) + (threadIdx.x >> 6)));
    const int32_t *counts = reinterpret_cast<const int32_t *>(out);
    int lv = -1, j = i;
#pragma unroll
    for (int l = 0; l < kOrbLevels; l++) {
        const int n = counts[l];
        if (lv < 0) { if (j < n) lv = l; else j -= n; }
    }
    if (lv < 0) return;                                   // wave-uniform
    const OrbLevel &L = t.l[lv];
    const uint4 c = *reinterpret_cast<const uint4 *>(kept + L.qprefix + j);   // R low, R high, raster
    const int y = (int)c.z / L.w, x = (int)c.z - y * L.w;
    const uint8_t *img = img0 + L.img_off;
    const int xa = (x - 15) & ~3;                         // the aligned dword that holds column x - 15; nine dwords cover the row at most
    const unsigned long long umax = 0x3689abcddeeeffffull;   // umax[|v|] = nibble |v|
    int m10 = 0, m01 = 0;
    for (int it = lane; it < 31 * 9; it += 64) {
        const int r = it / 9, q = it - 9 * r, v = r - 15, col = xa + 4 * q;
        if (col > x + 15) continue;
        const uint32_t w = *reinterpret_cast<const uint32_t *>(img + (size_t)(y + v) * L.pitch + col);
        const int um = (int)((umax >> (4 * (v < 0 ? -v : v))) & 15ull);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int u = col + b - x, I = (int)((w >> (8 * b)) & 255u);
            if (u >= -um && u <= um) { m10 += u * I; m01 += v * I; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m10 += __shfl_xor(m10, off); m01 += __shfl_xor(m01, off); }
    if (lane == 0) {
        const float fx = (float)((double)x * L.scale), fy = (float)((double)y * L.scale);
        uint4 *rec = reinterpret_cast<uint4 *>(out + kOutHeader + (size_t)i * sizeof(chip_orb_keypoint));
        rec[0] = make_uint4(c.x, c.y, __float_as_uint(fx), __float_as_uint(fy));
        rec[1] = make_uint4((uint32_t)m10, (uint32_t)m01, (uint32_t)x | ((uint32_t)y << 16), (uint32_t)lv);
    }
}
// grid ceil(n_features / 4), block 256: wave i makes record i
__global__ __launch_bounds__(kOrbThreads) void orb_moments(OrbArgs a) { moments_frame(a.t, a.img, a.kept, a.out); }
// the same grid x frames (blockIdx.y)
__global__ __launch_bounds__(kOrbThreads) void fb_moments(OrbBatchArgs g)
{
    const size_t f = blockIdx.y;
    moments_frame(g.a.t, g.a.img + f * g.f.img, g.a.kept + f * g.f.kept, g.a.out + f * g.f.out);
}

// ------------------------------------------------------------------------------------------------ orb_blur
constexpr int kBlurTileW = 128, kBlurTileH = 32;         // pixels of a blur tile: 8 x 32 threads of sixteen pixels in a row each
constexpr int kBlurRows = kBlurTileH + 6;                // 38
constexpr int kBlurDwords = (kBlurTileW + 8) / 4;        // 34 dwords a row: the tile's columns - 4 .. + 131
constexpr int kBlurHPitch = kBlurTileW + 8;              // uint16 a row of horizontal sums; + 8: rows start 16 bytes apart in the banks
constexpr int kDescWaves = kOrbThreads / 64;
constexpr int kOrbTabHeader = 256;                       // bytes: C[32], S[32] as int32 in front of the steered table
struct OrbBlurLevel { int32_t w, h, pitch, bpitch; uint32_t img_off, blur_off; };   // bpitch: a multiple of 16; the offsets in bytes
struct OrbBlurArgs {
    const uint8_t *img;
    uint8_t *blur;
    OrbBlurLevel l[kOrbLevels];
};
struct OrbBlurBatchArgs { OrbBlurArgs a; size_t img_stride, blur_stride; int32_t n_levels; };
// the dword of row `row` (pitch bytes, w pixels) at columns gx .. gx + 3 with the column clamped into the row; gx is a multiple of 4
__device__ __forceinline__ uint32_t orb_clamped_dword(const uint8_t *row, int gx, int w)
{
    const int last_at = (w - 1) & ~3;
    const uint32_t d = *reinterpret_cast<const uint32_t *>(row + min(max(gx, 0), last_at));
    if (gx < 0) return (d & 255u) * 0x01010101u;
    if (gx + 3 < w) return d;
    const uint32_t last = (*reinterpret_cast<const uint32_t *>(row + last_at) >> (8 * ((w - 1) & 3))) & 255u;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= (gx + b < w ? (d >> (8 * b)) & 255u : last) << (8 * b);
    return v;
}
// grid (tiles in x of the widest level, tiles in y of the tallest, n_levels), block 256.  The body is orb_blur_body.inc (see there why it is text).
__global__ __launch_bounds__(kOrbThreads) void orb_blur(OrbBlurArgs a)
{
#define ORB_FRAME(p, stride) (p)
#define ORB_BLUR_LEVEL blockIdx.z
#include "orb_blur_body.inc"
#undef ORB_BLUR_LEVEL
#undef ORB_FRAME
}
// grid z = level + n_levels * frame
__global__ __launch_bounds__(kOrbThreads) void fb_blur(OrbBlurBatchArgs batch)
{
    const OrbBlurArgs &a = batch.a;
    const unsigned frame = blockIdx.z / (unsigned)batch.n_levels;
#define ORB_FRAME(p, stride) ((p) + (size_t)frame * batch.stride)
#define ORB_BLUR_LEVEL (blockIdx.z - frame * (unsigned)batch.n_levels)
#include "orb_blur_body.inc"
#undef ORB_BLUR_LEVEL
#undef ORB_FRAME
}

// ------------------------------------------------------------------------------------------------ orb_describe
struct OrbDescArgs {
    const uint8_t *blur;
    const uint8_t *out;                // the eight kept counts and the records, as orb_moments left them
    const uint8_t *tab;                // kOrbTabHeader bytes of C and S, then the steered table [bin][lane][pairs lane, 64 + lane, 128 + lane, 192 + lane][4]
    uint8_t *desc;                     // 32 bytes per keypoint: the call's buffer or a slot of the frame store
    float2 *kp;                        // (x, y) per keypoint in a slot of the frame store, or null
    int32_t bpitch[kOrbLevels];
    uint32_t blur_off[kOrbLevels];
};
// desc / kp of the batch form: the rows of slot 0 of the frame store; frame f writes the rows of slot[f]
struct OrbDescBatchArgs { OrbDescArgs a; size_t blur_stride, out_stride; int32_t slot_kp; uint32_t slot[kOrbGroup]; };
// row_at: the first row of the frame's slot behind a.desc / a.kp
__device__ __forceinline__ void describe_frame(const OrbDescArgs &a, size_t blur_at, size_t out_at, size_t row_at)
{
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kDescWaves + (threadIdx.x >> 6)));
    const int32_t *counts = reinterpret_cast<const int32_t *>(a.out + out_at);
    int total = 0;
#pragma unroll
    for (int l = 0; l < kOrbLevels; l++) total += counts[l];
    if (i >= total) return;                               // wave-uniform
    const uint4 *rec = reinterpret_cast<const uint4 *>(a.out + out_at + kOutHeader + (size_t)i * sizeof(chip_orb_keypoint));
    const uint4 m = rec[1];                               // m10, m01, x | y << 16, level
    const int x = (int)(m.z & 0xffffu), y = (int)(m.z >> 16), lv = (int)(m.w & 7u);
    const int32_t *cs = reinterpret_cast<const int32_t *>(a.tab);
    const int k = lane & 31;
    long long v = (long long)(int32_t)m.x * cs[k] + (long long)(int32_t)m.y * cs[32 + k];
    int best = k;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {              // the largest sum, the lowest bin among equals; lanes 32 .. 63 repeat 0 .. 31
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(unsigned long long)v, off), hi = (uint32_t)__shfl_xor((int)((unsigned long long)v >> 32), off);
        const long long ov = (long long)(((unsigned long long)hi << 32) | lo);
        const int ob = __shfl_xor(best, off);
        if (ov > v || (ov == v && ob < best)) { v = ov; best = ob; }
    }
    best = __builtin_amdgcn_readfirstlane(best);
    const uint4 t = *reinterpret_cast<const uint4 *>(a.tab + kOrbTabHeader + ((size_t)best * 64 + lane) * 16);
    const uint8_t *B = a.blur + blur_at + a.blur_off[lv] + (size_t)y * a.bpitch[lv] + x;
    const int bp = a.bpitch[lv];
    const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
    unsigned long long bits[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int rx1 = (int8_t)(tw[j] & 255u), ry1 = (int8_t)((tw[j] >> 8) & 255u), rx2 = (int8_t)((tw[j] >> 16) & 255u), ry2 = (int8_t)(tw[j] >> 24);
        const int p = B[ry1 * bp + rx1], q = B[ry2 * bp + rx2];
        bits[j] = __ballot(p < q);                        // bit `lane` is pair 64 j + lane: bytes 8 j .. 8 j + 7, LSB first
    }
    if (lane == 0) {
        uint4 *d = reinterpret_cast<uint4 *>(a.desc + (row_at + (size_t)i) * CHIP_ORB_DESC_BYTES);
        d[0] = make_uint4((uint32_t)bits[0], (uint32_t)(bits[0] >> 32), (uint32_t)bits[1], (uint32_t)(bits[1] >> 32));
        d[1] = make_uint4((uint32_t)bits[2], (uint32_t)(bits[2] >> 32), (uint32_t)bits[3], (uint32_t)(bits[3] >> 32));
        if (a.kp) a.kp[row_at + (size_t)i] = make_float2(__uint_as_float(rec[0].z), __uint_as_float(rec[0].w));
    }
}
// grid ceil(n_features / 4), block 256: wave i makes descriptor i
__global__ __launch_bounds__(kOrbThreads) void orb_describe(OrbDescArgs a) { describe_frame(a, 0, 0, 0); }
// the same grid x frames (blockIdx.y): straight into the frame's slot
__global__ __launch_bounds__(kOrbThreads) void fb_describe(OrbDescBatchArgs g)
{
    const size_t f = blockIdx.y, at = (size_t)g.slot[f] * (size_t)g.slot_kp;
    describe_frame(g.a, f * g.blur_stride, f * g.out_stride, at);
}

// ------------------------------------------------------------------------------------------------ host side
struct OrbState {
    DevBuf<uint8_t> img;               // the levels, rows of pitch bytes
    DevBuf<int16_t> score;             // the score planes, rows of spitch elements
    DevBuf<OrbCand> cand;              // per level nstrips segments of cap candidates
    DevBuf<int32_t> strip_count;
    DevBuf<OrbCand> kept;              // CHIP_MATCH_MAX_KEYPOINTS
    DevBuf<uint8_t> out;               // kOutHeader + CHIP_MATCH_MAX_KEYPOINTS records
    PinnedBuf<uint8_t> h_out;
    PinnedBuf<uint8_t> h_img;          // level 0 with its row pitch, for widths that are no multiple of 4
    // the descriptor half: nothing of this exists before the first describing call
    DevBuf<uint8_t> blur;              // the blurred levels, rows of bpitch bytes
    DevBuf<uint8_t> tab;               // C, S and the steered table in the lanes' order, uploaded once
    DevBuf<uint8_t> desc;              // CHIP_MATCH_MAX_KEYPOINTS descriptors of chip_orb_detect_describe on their way out
    PinnedBuf<uint8_t> h_desc;
    bool tab_loaded = false;
    bool have = false;                 // a detect has finished: t describes what the buffers hold
    bool have_blur = false;            // ... and it was a describing one: bl describes the blurred planes
    OrbTable t{};
    OrbBlurLevel bl[kOrbLevels] = {};
};

void orb_destroy(Ctx *c)
{
    delete c->orb_state;
    c->orb_state = nullptr;
}

// ---- the descriptor's tables, made once on the host from the generator of the header
constexpr int kOrbPairs = 256;
static const int32_t kOrbQuarter[9] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0};   // C[0 .. 8]; S[k] = C[8 - k]
struct OrbTables {
    int32_t C[CHIP_ORB_BINS], S[CHIP_ORB_BINS];
    int8_t pattern[kOrbPairs][4];                        // x1, y1, x2, y2
    int8_t steered[CHIP_ORB_BINS][kOrbPairs][4];         // rx1, ry1, rx2, ry2
    std::vector<uint8_t> device;                         // what orb_describe reads: kOrbTabHeader bytes of C, S, then [bin][lane][4 pairs][4]
};
static const OrbTables &orb_tables()
{
    static OrbTables T;
    static std::once_flag once;
    std::call_once(once, [] {
        for (int k = 0; k <= 8; k++) { T.C[k] = kOrbQuarter[k]; T.S[k] = kOrbQuarter[8 - k]; }
        for (int k = 0; k + 8 < CHIP_ORB_BINS; k++) { T.C[k + 8] = -T.S[k]; T.S[k + 8] = T.C[k]; }
        uint64_t s = 0x4F52425F42524945ull;
        auto draw = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (int)((s >> 33) % 11u) - 5; };
        auto coord = [&draw]() { const int a = draw(), b = draw(), c = draw(); return a + b + c; };
        int n = 0;
        while (n < kOrbPairs) {
            const int x1 = coord(), y1 = coord(), x2 = coord(), y2 = coord();   // always twelve draws, in this order
            if (x1 * x1 + y1 * y1 > 169 || x2 * x2 + y2 * y2 > 169) continue;
            if ((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) < 9) continue;
            bool seen = false;
            for (int j = 0; j < n && !seen; j++) {
                const int8_t *q = T.pattern[j];
                seen = (q[0] == x1 && q[1] == y1 && q[2] == x2 && q[3] == y2) || (q[0] == x2 && q[1] == y2 && q[2] == x1 && q[3] == y1);
            }
            if (seen) continue;
            T.pattern[n][0] = (int8_t)x1; T.pattern[n][1] = (int8_t)y1; T.pattern[n][2] = (int8_t)x2; T.pattern[n][3] = (int8_t)y2;
            n++;
        }
        for (int k = 0; k < CHIP_ORB_BINS; k++)
            for (int p = 0; p < kOrbPairs; p++)
                for (int e = 0; e < 4; e += 2) {
                    const int x = T.pattern[p][e], y = T.pattern[p][e + 1];
                    T.steered[k][p][e] = (int8_t)((x * T.C[k] - y * T.S[k] + 8192) >> 14);       // arithmetic shifts
                    T.steered[k][p][e + 1] = (int8_t)((x * T.S[k] + y * T.C[k] + 8192) >> 14);
                }
        T.device.assign(kOrbTabHeader + sizeof T.steered, 0);
        std::memcpy(T.device.data(), T.C, sizeof T.C);
        std::memcpy(T.device.data() + sizeof T.C, T.S, sizeof T.S);
        for (int k = 0; k < CHIP_ORB_BINS; k++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 4; j++)
                    std::memcpy(T.device.data() + kOrbTabHeader + (((size_t)k * 64 + lane) * 4 + j) * 4, T.steered[k][64 * j + lane], 4);
    });
    return T;
}
static_assert(kOrbTabHeader == 2 * CHIP_ORB_BINS * sizeof(int32_t), "C and S in front of the steered table");

static int orb_bin_of(int32_t m10, int32_t m01)
{
    const OrbTables &T = orb_tables();
    int best = 0;
    long long top = 0;
    for (int k = 0; k < CHIP_ORB_BINS; k++) {
        const long long v = (long long)m10 * T.C[k] + (long long)m01 * T.S[k];
        if (k == 0 || v > top) { top = v; best = k; }
    }
    return best;
}

static int orb_params(const chip_orb_params *p, chip_orb_params *d)
{
    chip_orb_params_default(d);
    if (p) *d = *p;
    if (d->n_features < 1 || d->n_features > CHIP_MATCH_MAX_KEYPOINTS || d->n_levels < 1 || d->n_levels > kOrbLevels) return CHIP_ERR_UNSUPPORTED;
    if (d->fast_threshold < 0 || d->fast_threshold > 255 || d->border < 16 || d->border > 64) return CHIP_ERR_UNSUPPORTED;
    return CHIP_OK;
}

// the table of the header; the one place that decides sizes, quotas and rectangles
static void orb_plan(int32_t width, int32_t height, const chip_orb_params &p, chip_orb_level lv[kOrbLevels])
{
    std::memset(lv, 0, sizeof(chip_orb_level) * kOrbLevels);
    const double f = 1.0 / 1.2;
    double g = 1.0;
    for (int l = 0; l < p.n_levels; l++) g *= f;
    double nd = (double)p.n_features * (1.0 - f) / (1.0 - g), s = 1.0;
    int sum = 0;
    for (int l = 0; l < p.n_levels; l++) {
        if (l > 0) s *= 1.2;
        chip_orb_level &L = lv[l];
        L.scale = s;
        L.width = (int32_t)std::floor((double)width / s + 0.5);
        L.height = (int32_t)std::floor((double)height / s + 0.5);
        if (l < p.n_levels - 1) {
            L.quota = (int32_t)std::floor(nd + 0.5);
            if (L.quota > p.n_features - sum) L.quota = p.n_features - sum;   // the rounded quotas never exceed n_features together
            sum += L.quota;
            nd *= f;
        } else {
            L.quota = p.n_features - sum > 0 ? p.n_features - sum : 0;
        }
        L.x0 = L.y0 = p.border; L.x1 = L.width - 1 - p.border; L.y1 = L.height - 1 - p.border;
        if (L.x1 < L.x0 || L.y1 < L.y0) { L.x0 = L.y0 = 0; L.x1 = L.y1 = -1; }
    }
}

static hipStream_t orb_stream(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->query_mu);   // chip_set_stream swaps the ctx stream under this lock
    return c->s_query;
}

static int orb_check_size(int32_t width, int32_t height, const chip_orb_params *p, chip_orb_params *d)
{
    if (width < 1 || height < 1) return CHIP_ERR_INVALID_ARG;
    const int rc = orb_params(p, d);
    if (rc != CHIP_OK) return rc;
    if (width > kOrbMaxSide || height > kOrbMaxSide) return CHIP_ERR_UNSUPPORTED;
    return CHIP_OK;
}

int orb_check(int32_t width, int32_t height, const chip_orb_params *p, chip_orb_params *d) { return orb_check_size(width, height, p, d); }

// The detector and, if describe, the descriptor of one image, enqueued on s up to the copy of the first `back` bytes of the output (the
// eight counts, then the records) into h_out; nothing is waited for.  The image is `image` (host) or `image_dev` (device), dense rows.
// desc_dev / kp_dev: where orb_describe writes (desc_dev null: the state's own buffer; kp_dev may be null).  The caller holds match_mu,
// has selected the device, and calls orb_finished once the stream has drained.
// the launch table: where every level of ONE frame lives in the ctx's buffers, the elements a frame takes of each, and what sizes the grids
struct OrbLayout {
    OrbTable t{};
    OrbBlurLevel bl[kOrbLevels] = {};
    size_t img_n = 0, score_n = 0, cand_n = 0, strip_n = 0, blur_n = 0;
    int max_w = 0, max_h = 0, max_strips = 0, max_bw = 0;
};
static void orb_layout(int32_t width, int32_t height, const chip_orb_params &d, OrbLayout *lay)
{
    chip_orb_level plan[kOrbLevels];
    orb_plan(width, height, d, plan);
    OrbTable &t = lay->t;
    OrbBlurLevel *bl = lay->bl;
    t.n_levels = d.n_levels; t.n_features = d.n_features; t.threshold = d.fast_threshold;
    size_t &img_n = lay->img_n, &score_n = lay->score_n, &cand_n = lay->cand_n, &strip_n = lay->strip_n, &blur_n = lay->blur_n;
    int qprefix = 0, &max_w = lay->max_w, &max_h = lay->max_h, &max_strips = lay->max_strips, &max_bw = lay->max_bw;
    for (int l = 0; l < d.n_levels; l++) {
        OrbLevel &L = t.l[l];
        L.w = plan[l].width; L.h = plan[l].height; L.scale = plan[l].scale;
        L.pitch = (L.w + 3) & ~3; L.spitch = (L.w + 7) & ~7;
        L.x0 = plan[l].x0; L.y0 = plan[l].y0; L.x1 = plan[l].x1; L.y1 = plan[l].y1;
        L.quota = plan[l].quota; L.qprefix = qprefix; qprefix += L.quota;
        const bool area = L.x1 >= L.x0;
        L.cap = area ? (L.x1 - L.x0 + 2) / 2 : 0;
        L.nstrips = area ? (L.y1 - L.y0 + kStripRows) / kStripRows : 0;
        L.img_off = (uint32_t)img_n; L.score_off = (uint32_t)score_n; L.cand_off = (uint32_t)cand_n; L.strip_off = (uint32_t)strip_n;
        bl[l] = OrbBlurLevel{L.w, L.h, L.pitch, (L.w + 15) & ~15, L.img_off, (uint32_t)blur_n};
        img_n += ((size_t)L.pitch * L.h + 15) & ~(size_t)15;
        score_n += (size_t)L.spitch * L.h;               // a multiple of 8 elements: every plane starts on 16 bytes
        cand_n += (size_t)L.cap * L.nstrips;
        strip_n += (size_t)L.nstrips;
        blur_n += (size_t)bl[l].bpitch * L.h;             // a multiple of 16 bytes
        max_w = L.spitch > max_w ? L.spitch : max_w; max_h = L.h > max_h ? L.h : max_h;
        max_strips = L.nstrips > max_strips ? L.nstrips : max_strips;
        max_bw = bl[l].bpitch > max_bw ? bl[l].bpitch : max_bw;
    }
}

int orb_enqueue(Ctx *c, hipStream_t s, const uint8_t *image, const uint8_t *image_dev, int32_t width, int32_t height, const chip_orb_params &d,
                bool describe, uint8_t *desc_dev, float2 *kp_dev, size_t back)
{
    OrbLayout lay;
    orb_layout(width, height, d, &lay);
    const OrbTable &t = lay.t;
    const OrbBlurLevel *bl = lay.bl;
    const size_t img_n = lay.img_n, score_n = lay.score_n, cand_n = lay.cand_n, strip_n = lay.strip_n, blur_n = lay.blur_n;
    const int max_w = lay.max_w, max_h = lay.max_h, max_strips = lay.max_strips, max_bw = lay.max_bw;
    if (!c->orb_state) {
        c->orb_state = new (std::nothrow) OrbState();
        if (!c->orb_state) return CHIP_ERR_OOM;
    }
    OrbState *st = c->orb_state;
    st->have = st->have_blur = false;
    int rc = CHIP_OK;
    const size_t out_bytes = kOutHeader + (size_t)CHIP_MATCH_MAX_KEYPOINTS * sizeof(chip_orb_keypoint);
    const size_t h_img_n = !image || t.l[0].pitch == t.l[0].w ? 0 : (size_t)t.l[0].pitch * t.l[0].h;   // a host image whose width is no multiple of 4
    if (st->img.capacity() < img_n || st->score.capacity() < score_n || st->cand.capacity() < cand_n + 1 || st->strip_count.capacity() < strip_n + 1 ||
        !st->h_out.capacity() || st->h_img.capacity() < h_img_n) {
        ResidentPause paused(c);   // one pause over the group, as the GMS mode tables
        rc = st->img.reserve(c, img_n);
        if (rc == CHIP_OK) rc = st->score.reserve(c, score_n);
        if (rc == CHIP_OK) rc = st->cand.reserve(c, cand_n + 1);
        if (rc == CHIP_OK) rc = st->strip_count.reserve(c, strip_n + 1);
        if (rc == CHIP_OK) rc = st->kept.reserve(c, CHIP_MATCH_MAX_KEYPOINTS);
        if (rc == CHIP_OK) rc = st->out.reserve(c, out_bytes);
        if (rc == CHIP_OK) rc = st->h_out.reserve(c, out_bytes);
        if (rc == CHIP_OK) rc = st->h_img.reserve(c, h_img_n);
        if (rc != CHIP_OK) return rc;
    }
    const OrbTables &tables = orb_tables();
    const size_t desc_bytes = (size_t)CHIP_MATCH_MAX_KEYPOINTS * CHIP_ORB_DESC_BYTES;
    if (describe && (st->blur.capacity() < blur_n + 1 || !st->h_desc.capacity())) {
        ResidentPause paused(c);
        rc = st->blur.reserve(c, blur_n + 1);
        if (rc == CHIP_OK) rc = st->tab.reserve(c, tables.device.size());
        if (rc == CHIP_OK) rc = st->desc.reserve(c, desc_bytes);
        if (rc == CHIP_OK) rc = st->h_desc.reserve(c, desc_bytes);
        if (rc != CHIP_OK) return rc;
    }
    OrbArgs a;
    a.img = st->img; a.score = st->score; a.cand = st->cand; a.strip_count = st->strip_count; a.kept = st->kept; a.out = st->out; a.t = t;
    const OrbLevel &L0 = t.l[0];
    if (image_dev) {
        CHIP_HIP(c, hipMemcpy2DAsync(a.img, (size_t)L0.pitch, image_dev, (size_t)width, (size_t)width, (size_t)height, hipMemcpyDeviceToDevice, s));
    } else if (L0.pitch == L0.w) {
        CHIP_HIP(c, hipMemcpyAsync(a.img, image, (size_t)width * height, hipMemcpyHostToDevice, s));
    } else {   // rows of pitch bytes are made on the host, in pinned memory (the previous call has finished: every call ends in a wait)
        uint8_t *rows = st->h_img.host();
        for (int y = 0; y < height; y++) std::memcpy(rows + (size_t)y * L0.pitch, image + (size_t)y * width, (size_t)width);
        CHIP_HIP(c, hipMemcpyAsync(a.img, rows, (size_t)L0.pitch * height, hipMemcpyHostToDevice, s));
    }
    if (describe && !st->tab_loaded) {                    // the tables outlive the copy: they are static
        CHIP_HIP(c, hipMemcpyAsync(st->tab, tables.device.data(), tables.device.size(), hipMemcpyHostToDevice, s));
        st->tab_loaded = true;
    }
    for (int l = 1; l < d.n_levels; l++) {
        const OrbLevel &L = t.l[l];
        if (L.w < 1 || L.h < 1) break;                    // sizes only shrink: nothing above either
        hipLaunchKernelGGL(orb_pyramid, dim3((L.pitch / 4 + 63) / 64, (L.h + 3) / 4), dim3(64, 4), 0, s, a, l);
        CHIP_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(orb_fast_score, dim3((max_w + kScoreTileW - 1) / kScoreTileW, (max_h + kScoreTileH - 1) / kScoreTileH, d.n_levels),
                       dim3(kOrbThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    if (max_strips > 0) {
        hipLaunchKernelGGL(orb_candidates, dim3(max_strips, d.n_levels), dim3(kOrbThreads), 0, s, a);
        CHIP_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(orb_select, dim3(kOrbLevels), dim3(kSelectThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    const dim3 per_keypoint((d.n_features + kOrbThreads / 64 - 1) / (kOrbThreads / 64));
    hipLaunchKernelGGL(orb_moments, per_keypoint, dim3(kOrbThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    if (describe) {
        OrbBlurArgs b;
        b.img = st->img; b.blur = st->blur;
        OrbDescArgs g;
        g.blur = st->blur; g.out = st->out; g.tab = st->tab; g.desc = desc_dev ? desc_dev : st->desc.get(); g.kp = kp_dev;
        for (int l = 0; l < kOrbLevels; l++) { b.l[l] = bl[l]; g.bpitch[l] = bl[l].bpitch; g.blur_off[l] = bl[l].blur_off; }
        if (max_bw > 0 && max_h > 0) {
            hipLaunchKernelGGL(orb_blur, dim3((max_bw + kBlurTileW - 1) / kBlurTileW, (max_h + kBlurTileH - 1) / kBlurTileH, d.n_levels),
                               dim3(kOrbThreads), 0, s, b);
            CHIP_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(orb_describe, per_keypoint, dim3(kOrbThreads), 0, s, g);
        CHIP_HIP(c, hipGetLastError());
    }
    CHIP_HIP(c, hipMemcpyAsync(st->h_out.host(), a.out, back, hipMemcpyDeviceToHost, s));
    st->t = t;
    for (int l = 0; l < kOrbLevels; l++) st->bl[l] = bl[l];
    return CHIP_OK;
}

constexpr size_t kOrbOutBytes = kOutHeader + (size_t)CHIP_MATCH_MAX_KEYPOINTS * sizeof(chip_orb_keypoint);   // header and records of one frame
constexpr size_t kOrbKeptStride = CHIP_MATCH_MAX_KEYPOINTS;

int orb_batch_reserve(Ctx *c, int32_t G, int32_t width, int32_t height, const chip_orb_params &d, bool probe)
{
    if (G < 1 || G > kOrbGroup) return CHIP_ERR_INVALID_ARG;
    OrbLayout lay;
    orb_layout(width, height, d, &lay);
    if (!c->orb_state) {
        if (probe) return 1;
        c->orb_state = new (std::nothrow) OrbState();
        if (!c->orb_state) return CHIP_ERR_OOM;
    }
    OrbState *st = c->orb_state;
    const size_t g = (size_t)G;
    const size_t desc_bytes = (size_t)CHIP_MATCH_MAX_KEYPOINTS * CHIP_ORB_DESC_BYTES;
    const OrbTables &tables = orb_tables();
    const bool fits = st->img.capacity() >= g * lay.img_n && st->score.capacity() >= g * lay.score_n && st->cand.capacity() >= g * lay.cand_n + 1 &&
                      st->strip_count.capacity() >= g * lay.strip_n + 1 && st->kept.capacity() >= g * kOrbKeptStride &&
                      st->out.capacity() >= g * kOrbOutBytes && st->h_out.capacity() && st->blur.capacity() >= g * lay.blur_n + 1 &&
                      st->h_desc.capacity();
    if (probe) return fits ? 0 : 1;
    if (fits) return CHIP_OK;
    ResidentPause paused(c);   // one pause over everything a group needs
    int rc = st->img.reserve(c, g * lay.img_n);
    if (rc == CHIP_OK) rc = st->score.reserve(c, g * lay.score_n);
    if (rc == CHIP_OK) rc = st->cand.reserve(c, g * lay.cand_n + 1);
    if (rc == CHIP_OK) rc = st->strip_count.reserve(c, g * lay.strip_n + 1);
    if (rc == CHIP_OK) rc = st->kept.reserve(c, g * kOrbKeptStride);
    if (rc == CHIP_OK) rc = st->out.reserve(c, g * kOrbOutBytes);
    if (rc == CHIP_OK) rc = st->h_out.reserve(c, kOrbOutBytes);
    if (rc == CHIP_OK) rc = st->blur.reserve(c, g * lay.blur_n + 1);
    if (rc == CHIP_OK) rc = st->tab.reserve(c, tables.device.size());
    if (rc == CHIP_OK) rc = st->desc.reserve(c, desc_bytes);
    if (rc == CHIP_OK) rc = st->h_desc.reserve(c, desc_bytes);
    return rc;
}

// The detector and the descriptor of the G <= kOrbGroup left images of a batched put, ONE launch per stage (the pyramid: per level) over
// all frames.  The rectified pairs lie in device memory, pair f at pairs_dev + f * pair_stride, dense rows, left first.  Frame f's scratch
// lies at f x the single call's size behind frame 0's, in the same buffers, grown inside one pause; orb_describe's batch entry writes the
// rows of slot[f] of the store (desc_base, kp_base: slot 0, slot_kp rows a slot).  Nothing is waited for and nothing is copied back: the
// kept counts of frame f stay at *out_dev + f * *out_stride (eight int32) for the block matcher's batch entry and orb_batch_counts.
// *launches grows by the launches made.  The caller holds match_mu and has selected the device.
int orb_batch_enqueue(Ctx *c, hipStream_t s, const uint8_t *pairs_dev, size_t pair_stride, int32_t G, int32_t width, int32_t height,
                      const chip_orb_params &d, uint8_t *desc_base, float2 *kp_base, int32_t slot_kp, const int32_t *slot, int32_t *launches,
                      const uint8_t **out_dev, size_t *out_stride)
{
    int rc = orb_batch_reserve(c, G, width, height, d, false);   // (the caller has done it: nothing grows here)
    if (rc != CHIP_OK) return rc;
    OrbLayout lay;
    orb_layout(width, height, d, &lay);
    OrbState *st = c->orb_state;
    st->have = st->have_blur = false;                     // the debug calls read a single call's buffers
    const size_t g = (size_t)G, out_bytes = kOrbOutBytes, kept_n = kOrbKeptStride;
    const OrbTables &tables = orb_tables();
    OrbBatchArgs a;
    a.a.img = st->img; a.a.score = st->score; a.a.cand = st->cand; a.a.strip_count = st->strip_count; a.a.kept = st->kept; a.a.out = st->out;
    a.a.t = lay.t;
    a.f = OrbStrides{lay.img_n, lay.score_n, lay.cand_n, lay.strip_n, kept_n, out_bytes};
    const OrbTable &t = lay.t;
    const OrbLevel &L0 = t.l[0];
    const size_t px = (size_t)width * height;
    if (L0.pitch == L0.w) {        // a level 0 is its dense image: the left images of all frames in ONE strided copy, a row a frame
        CHIP_HIP(c, hipMemcpy2DAsync(a.a.img, lay.img_n, pairs_dev, pair_stride, px, g, hipMemcpyDeviceToDevice, s));
    } else {
        for (size_t f = 0; f < g; f++)
            CHIP_HIP(c, hipMemcpy2DAsync(a.a.img + f * lay.img_n, (size_t)L0.pitch, pairs_dev + f * pair_stride, (size_t)width, (size_t)width,
                                         (size_t)height, hipMemcpyDeviceToDevice, s));
    }
    if (!st->tab_loaded) {
        CHIP_HIP(c, hipMemcpyAsync(st->tab, tables.device.data(), tables.device.size(), hipMemcpyHostToDevice, s));
        st->tab_loaded = true;
    }
    const unsigned frames = (unsigned)G;
    for (int l = 1; l < d.n_levels; l++) {
        const OrbLevel &L = t.l[l];
        if (L.w < 1 || L.h < 1) break;
        hipLaunchKernelGGL(fb_pyramid, dim3((L.pitch / 4 + 63) / 64, (L.h + 3) / 4, frames), dim3(64, 4), 0, s, a, l);
        CHIP_HIP(c, hipGetLastError());
        ++*launches;
    }
    hipLaunchKernelGGL(fb_fast_score, dim3((lay.max_w + kScoreTileW - 1) / kScoreTileW, (lay.max_h + kScoreTileH - 1) / kScoreTileH, d.n_levels * frames),
                       dim3(kOrbThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    ++*launches;
    if (lay.max_strips > 0) {
        hipLaunchKernelGGL(fb_candidates, dim3(lay.max_strips, d.n_levels, frames), dim3(kOrbThreads), 0, s, a);
        CHIP_HIP(c, hipGetLastError());
        ++*launches;
    }
    hipLaunchKernelGGL(fb_select, dim3(kOrbLevels, frames), dim3(kSelectThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    ++*launches;
    const dim3 per_keypoint((d.n_features + kOrbThreads / 64 - 1) / (kOrbThreads / 64), frames);
    hipLaunchKernelGGL(fb_moments, per_keypoint, dim3(kOrbThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    ++*launches;
    OrbBlurBatchArgs b;
    b.a.img = st->img; b.a.blur = st->blur; b.img_stride = lay.img_n; b.blur_stride = lay.blur_n; b.n_levels = d.n_levels;
    OrbDescBatchArgs e;
    e.a.blur = st->blur; e.a.out = st->out; e.a.tab = st->tab; e.a.desc = desc_base; e.a.kp = kp_base;
    e.blur_stride = lay.blur_n; e.out_stride = out_bytes; e.slot_kp = slot_kp;
    for (int l = 0; l < kOrbLevels; l++) { b.a.l[l] = lay.bl[l]; e.a.bpitch[l] = lay.bl[l].bpitch; e.a.blur_off[l] = lay.bl[l].blur_off; }
    for (int f = 0; f < kOrbGroup; f++) e.slot[f] = (uint32_t)slot[f < G ? f : 0];
    if (lay.max_bw > 0 && lay.max_h > 0) {
        hipLaunchKernelGGL(fb_blur, dim3((lay.max_bw + kBlurTileW - 1) / kBlurTileW, (lay.max_h + kBlurTileH - 1) / kBlurTileH, d.n_levels * frames),
                           dim3(kOrbThreads), 0, s, b);
        CHIP_HIP(c, hipGetLastError());
        ++*launches;
    }
    hipLaunchKernelGGL(fb_describe, per_keypoint, dim3(kOrbThreads), 0, s, e);
    CHIP_HIP(c, hipGetLastError());
    ++*launches;
    *out_dev = st->out;
    *out_stride = out_bytes;
    return CHIP_OK;
}

// the eight kept counts of each of the G frames of the group enqueued last, in ONE strided copy into pinned memory; *counts (G x 8) is
// valid once s has drained
int orb_batch_counts(Ctx *c, hipStream_t s, int32_t G, const int32_t **counts)
{
    OrbState *st = c->orb_state;
    const size_t out_bytes = kOrbOutBytes;
    CHIP_HIP(c, hipMemcpy2DAsync(st->h_out.host(), kOutHeader, st->out, out_bytes, kOutHeader, (size_t)G, hipMemcpyDeviceToHost, s));
    *counts = reinterpret_cast<const int32_t *>(st->h_out.host());
    return CHIP_OK;
}

// the stream has drained after an orb_enqueue: the counts (checked against n_features) and what the debug calls may read
int orb_finished(Ctx *c, bool describe, int32_t n_features, int32_t *total_out, int32_t level_counts[8])
{
    OrbState *st = c->orb_state;
    const int32_t *counts = reinterpret_cast<const int32_t *>(st->h_out.host());
    int32_t total = 0;
    for (int l = 0; l < kOrbLevels; l++) {
        total += counts[l];
        if (level_counts) level_counts[l] = counts[l];
    }
    if (total < 0 || total > n_features) return CHIP_ERR_HIP;   // cannot happen: the kept lists are bounded by the quotas
    *total_out = total;
    st->have = true;
    st->have_blur = describe;
    return CHIP_OK;
}

}  // namespace chip

using namespace chip;

extern "C" int chip_build_has_orb_detect(void) { return 1; }

extern "C" void chip_orb_params_default(chip_orb_params *p)
{
    if (p) *p = chip_orb_params{5000, 8, 0, 31};   // cv::ORB::create(5000), setFastThreshold(0)
}

extern "C" int chip_orb_plan(int32_t width, int32_t height, const chip_orb_params *p, chip_orb_level levels[8])
{
    if (!levels) return CHIP_ERR_INVALID_ARG;
    chip_orb_params d;
    const int rc = orb_check_size(width, height, p, &d);
    if (rc != CHIP_OK) return rc;
    orb_plan(width, height, d, levels);
    return CHIP_OK;
}

// chip_orb_detect and chip_orb_detect_describe: desc null is the former
static int orb_detect_call(chip_ctx *c, const uint8_t *image, int32_t width, int32_t height, const chip_orb_params *p, chip_orb_keypoint *kp,
                           int32_t capacity, int32_t *n, int32_t level_counts[8], uint8_t *desc)
{
    chip_orb_params d;
    int rc = orb_check_size(width, height, p, &d);
    if (rc != CHIP_OK) return rc;
    if (capacity < d.n_features) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    hipStream_t s = orb_stream(c);
    const size_t back = kOutHeader + (size_t)d.n_features * sizeof(chip_orb_keypoint);
    rc = orb_enqueue(c, s, image, nullptr, width, height, d, desc != nullptr, nullptr, nullptr, back);
    if (rc != CHIP_OK) return rc;
    OrbState *st = c->orb_state;
    if (desc) CHIP_HIP(c, hipMemcpyAsync(st->h_desc.host(), st->desc, (size_t)d.n_features * CHIP_ORB_DESC_BYTES, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    int32_t total = 0;
    rc = orb_finished(c, desc != nullptr, d.n_features, &total, level_counts);
    if (rc != CHIP_OK) return rc;
    std::memcpy(kp, st->h_out.host() + kOutHeader, (size_t)total * sizeof(chip_orb_keypoint));
    if (desc) std::memcpy(desc, st->h_desc.host(), (size_t)total * CHIP_ORB_DESC_BYTES);
    *n = total;
    return CHIP_OK;
}

extern "C" int chip_orb_detect(chip_ctx *c, const uint8_t *image, int32_t width, int32_t height, const chip_orb_params *p,
                               chip_orb_keypoint *kp, int32_t capacity, int32_t *n, int32_t level_counts[8])
{
    if (!c || !image || !kp || !n) return CHIP_ERR_INVALID_ARG;
    return orb_detect_call(c, image, width, height, p, kp, capacity, n, level_counts, nullptr);
}

// ------------------------------------------------------------------------------------------------ the descriptor half
extern "C" int chip_build_has_orb_describe(void) { return 1; }

extern "C" int chip_orb_bin(int32_t m10, int32_t m01) { return orb_bin_of(m10, m01); }

extern "C" int chip_orb_pattern(int8_t pattern[1024], int8_t steered[32768])
{
    if (!pattern && !steered) return CHIP_ERR_INVALID_ARG;
    const OrbTables &T = orb_tables();
    if (pattern) std::memcpy(pattern, T.pattern, sizeof T.pattern);
    if (steered) std::memcpy(steered, T.steered, sizeof T.steered);
    return CHIP_OK;
}

extern "C" int chip_orb_detect_describe(chip_ctx *c, const uint8_t *image, int32_t width, int32_t height, const chip_orb_params *p,
                                        chip_orb_keypoint *kp, int32_t capacity, int32_t *n, int32_t level_counts[8], uint8_t *desc)
{
    if (!c || !image || !kp || !n || !desc) return CHIP_ERR_INVALID_ARG;
    return orb_detect_call(c, image, width, height, p, kp, capacity, n, level_counts, desc);
}

extern "C" int chip_debug_orb_blur(chip_ctx *c, int32_t level, uint8_t *out)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    OrbState *st = c->orb_state;
    if (!st || !st->have || !st->have_blur) return CHIP_ERR_BUSY;
    if (level < 0 || level >= st->t.n_levels) return CHIP_ERR_RANGE;
    const OrbBlurLevel &L = st->bl[level];
    if (L.w < 1 || L.h < 1 || !out) return CHIP_OK;       // an empty level: nothing to deliver
    CHIP_HIP(c, hipSetDevice(c->device));
    hipStream_t s = orb_stream(c);
    CHIP_HIP(c, hipMemcpy2DAsync(out, (size_t)L.w, st->blur.get() + L.blur_off, (size_t)L.bpitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

extern "C" int chip_debug_orb_level(chip_ctx *c, int32_t level, uint8_t *image_out, int16_t *score_out)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    OrbState *st = c->orb_state;
    if (!st || !st->have) return CHIP_ERR_BUSY;
    if (level < 0 || level >= st->t.n_levels) return CHIP_ERR_RANGE;
    const OrbLevel &L = st->t.l[level];
    if (L.w < 1 || L.h < 1) return CHIP_OK;               // an empty level: nothing to deliver
    CHIP_HIP(c, hipSetDevice(c->device));
    hipStream_t s = orb_stream(c);
    if (image_out)
        CHIP_HIP(c, hipMemcpy2DAsync(image_out, (size_t)L.w, st->img.get() + L.img_off, (size_t)L.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost, s));
    if (score_out)
        CHIP_HIP(c, hipMemcpy2DAsync(score_out, (size_t)L.w * 2, st->score.get() + L.score_off, (size_t)L.spitch * 2, (size_t)L.w * 2, (size_t)L.h,
                                     hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}
