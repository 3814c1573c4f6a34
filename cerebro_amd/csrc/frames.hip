// frames.hip -- the device-resident frame store on gfx950 and everything that fills it (include/cerebro_hip.h has the definitions:
// "frames kept on the device", "a frame from its disparity map", "... its rectified stereo pair", "... its raw stereo pair").  The match
// stage that reads stored frames is match.hip; the detector and the descriptor that the ORB puts run are orb.hip.
//
//   frame_gather     : a frame's point records at put time, one thread per keypoint: (x, y, z, 1.0f) copied from the staged 3-D image at
//                      the keypoint's pixel (pixel_of, frame_store.h), (0, 0, 0, 0.0f) outside it.  A match reads records only.
//   disparity_gather : the same for a frame that arrives as its disparity map: the record from the ONE value at the keypoint's pixel
//                      (point_of_disparity: StereoGeometry::disparity_to_3DPoints restated).
//   disparity_to_xyz : the dense out3D of the same function (chip_disparity_to_xyz), four consecutive pixels of a row per thread.
//   bm_prefilter     : the x-Sobel prefilter of the block matcher, both images of the pair in one launch, four pixels per thread.
//   bm_keypoints     : disparity_gather for a frame that arrives as its rectified pair -- one wave per keypoint computes the disparity at
//                      the keypoint's pixel (bm_pixel: lane = disparity, v_sad_u8 on window rows read in place), lane 0 writes the record.
//   bm_dense         : the same body at every pixel (chip_stereo_bm; the definition made callable, not a hot path).
//   rectify_pair     : both eyes and both stages of the rectification in one launch, on maps the host has quantised to 1/32 pixel.
//   fb_rectify, fb_prefilter, fb_keypoints : the batch entries of rectify_pair, bm_prefilter and bm_keypoints for the batched puts
//                      (chip_frame_put_orb_stereo_batch, chip_frame_put_raw_orb_stereo_batch): the frame is a grid axis, the body is the
//                      single kernel's (a __device__ function on the frame's bases; rectify_pair's an included text).  fb_keypoints reads each frame's kept count in
//                      device memory and writes the records of its slot through a slot table in the arguments.
//
// The host side has ONE slot transaction (SlotPut) around per-source record writers: chip_frame_put, _disparity and _stereo upload the
// caller's rows and state what they stage and which kernel writes the records (put_frame); the two ORB puts make the rows on the device
// (put_orb_stereo; put_orb_stereo_batch: many pairs per call in groups of one launch per stage, chip_frame_put_records: the rows back from
// a checkpoint).  The state is FrameStore (frame_store.h), guarded by match_mu; the dense calls and the rectification create it alone.
// Nothing here rounds twice (-ffp-contract=off); tests/np_mirror_{frame_store,disparity,stereo_bm,rectify}.py restate it in numpy.
#include "frame_store.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace chip {

// ------------------------------------------------------------------------------------------------ frames kept on the device
// frame_gather: a frame's point records at put time, one thread per keypoint; afterwards the staged image is not needed again
struct GatherArgs {
    const float2 *kp;             // n, in the frame's slot
    const float *xyz;             // h x w x 3, staged
    float4 *rec;                  // n, in the frame's slot
    int32_t n, w, h;
};
constexpr int kGatherThreads = 256;
__global__ __launch_bounds__(kGatherThreads) void frame_gather(GatherArgs g)
{
    const int i = blockIdx.x * kGatherThreads + threadIdx.x;
    if (i >= g.n) return;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    int x, y;
    if (pixel_of(g.kp[i], g.w, g.h, &x, &y)) {
        const size_t o = 3 * ((size_t)y * g.w + x);
        r = make_float4(g.xyz[o], g.xyz[o + 1], g.xyz[o + 2], 1.0f);
    }
    g.rec[i] = r;
}

// A pixel's 3-D point from its disparity: StereoGeometry::disparity_to_3DPoints (src/utils/CameraGeometry.cpp:485-523) restated.  The
// five floats are Q(0,3), (1,3), (2,3), (3,2), (3,3) narrowed on the host (:494-498); d is the disparity as a float, 16 x pixels.
// pw: every operation in fp64 in the reference's order, an IEEE divide, one narrowing (:511); d / 16 * Q32 is exact, the two additions
// and the divide round.  x, y, z: fp32 products (:520-522); the file is compiled with -ffp-contract=off, nothing here may fuse.
struct DispQ { float q03, q13, q23, q32, q33; };
__device__ __forceinline__ float3 point_of_disparity(float d, int j, int i, const DispQ &q)
{
    const float pw = (float)(1.0 / ((((double)d / 16.0) * (double)q.q32 + (double)q.q33) + 1e-6));
    return make_float3(((float)j + q.q03) * pw, ((float)i + q.q13) * pw, q.q23 * pw);
}

// disparity_gather: frame_gather for a frame that arrives as its disparity map -- the record of a keypoint is computed from the ONE
// disparity value at its pixel
struct GatherDispArgs {
    const float2 *kp;             // n, in the frame's slot
    const void *disp;             // h x w, staged: int16 (CHIP_DISP_S16) or float (CHIP_DISP_F32)
    float4 *rec;                  // n, in the frame's slot
    int32_t n, w, h, type;
    DispQ q;
};
__global__ __launch_bounds__(kGatherThreads) void disparity_gather(GatherDispArgs g)
{
    const int i = blockIdx.x * kGatherThreads + threadIdx.x;
    if (i >= g.n) return;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    int x, y;
    if (pixel_of(g.kp[i], g.w, g.h, &x, &y)) {
        const size_t o = (size_t)y * g.w + x;
        const float d = g.type == CHIP_DISP_S16 ? (float)static_cast<const int16_t *>(g.disp)[o] : static_cast<const float *>(g.disp)[o];
        const float3 p = point_of_disparity(d, x, y, g.q);
        r = make_float4(p.x, p.y, p.z, 1.0f);
    }
    g.rec[i] = r;
}

// disparity_to_xyz: the dense out3D (:482-524).  A thread takes four consecutive pixels of a row: where the four are inside the row and
// their first is a multiple of four in the image (the rows of a width that is none start anywhere) with both pointers 16-byte aligned,
// ONE load of 8 (int16) or 16 (float) bytes and three 16-byte stores for the 48 contiguous bytes; otherwise pixel by pixel.
struct DenseDispArgs {
    const void *disp;             // h x w
    float *xyz;                   // h x w x 3
    int32_t w, h, type, quads;    // quads: (w + 3) / 4 threads per row
    DispQ q;
};
constexpr int kDenseThreads = 256;
__global__ __launch_bounds__(kDenseThreads) void disparity_to_xyz(DenseDispArgs a)
{
    const size_t t = (size_t)blockIdx.x * kDenseThreads + threadIdx.x;
    const int i = (int)(t / (size_t)a.quads), j0 = 4 * (int)(t % (size_t)a.quads);
    if (i >= a.h) return;
    const size_t p0 = (size_t)i * a.w + j0;
    const int16_t *s16 = static_cast<const int16_t *>(a.disp);
    const float *f32 = static_cast<const float *>(a.disp);
    const bool aligned = (((uintptr_t)a.disp | (uintptr_t)a.xyz) & 15) == 0;
    if (j0 + 4 <= a.w && (p0 & 3) == 0 && aligned) {
        float d[4];
        if (a.type == CHIP_DISP_S16) {
            const short4 v = *reinterpret_cast<const short4 *>(s16 + p0);
            d[0] = (float)v.x; d[1] = (float)v.y; d[2] = (float)v.z; d[3] = (float)v.w;
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(f32 + p0);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        float3 p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = point_of_disparity(d[k], j0 + k, i, a.q);
        float4 *o = reinterpret_cast<float4 *>(a.xyz + 3 * p0);
        o[0] = make_float4(p[0].x, p[0].y, p[0].z, p[1].x);
        o[1] = make_float4(p[1].y, p[1].z, p[2].x, p[2].y);
        o[2] = make_float4(p[2].z, p[3].x, p[3].y, p[3].z);
        return;
    }
    for (int j = j0; j < j0 + 4 && j < a.w; j++) {
        const size_t p = (size_t)i * a.w + j;
        const float3 v = point_of_disparity(a.type == CHIP_DISP_S16 ? (float)s16[p] : f32[p], j, i, a.q);
        a.xyz[3 * p] = v.x; a.xyz[3 * p + 1] = v.y; a.xyz[3 * p + 2] = v.z;
    }
}

// ------------------------------------------------------------------------------------------------ the block matcher
// The definition is in include/cerebro_hip.h ("a frame from its rectified stereo pair"): this project's own, modelled on cv::StereoBM
// with PREFILTER_XSOBEL, all in int32.  r = block_size / 2.
struct BmParams { int32_t nd, r, cap, tex, ratio; };
constexpr int kBmInvalid = -16;        // (minDisparity - 1) * 16
constexpr int kBmRowDwords = 6;        // a window row: at most 21 bytes, padded to whole dwords
constexpr int kBmPad = 16;             // bytes behind the prefiltered pair: a row read in whole dwords ends at most 7 bytes behind its window
constexpr int kBmThreads = 256;
constexpr int kBmWaves = kBmThreads / 64;

// bm_prefilter: both images in one launch -- the staged pair is 2 h rows of w bytes, the prefiltered pair the same.  A thread takes four
// consecutive pixels of a row: the column sums s(x) = I[y-][x] + 2 I[y][x] + I[y+][x] at the six columns around them (v = s(x + 1) -
// s(x - 1), exact in int32), then ONE 32-bit store where the four are inside the row and their address is a multiple of four (a width
// that is none shifts every row), byte by byte otherwise.
struct PrefilterArgs {
    const uint8_t *img;           // 2 h x w: left, right
    uint8_t *pre;                 // 2 h x w
    int32_t w, h, quads, cap;     // quads: (w + 3) / 4 threads per row
};
// One body per stage and two entries, as in orb.hip: the single call's kernel and the batched put's (fb_*), whose frame comes from the grid
// and whose bases lie at frame x stride.
__device__ __forceinline__ void prefilter_frame(const PrefilterArgs &a)
{
    const size_t t = (size_t)blockIdx.x * kBmThreads + threadIdx.x;
    const size_t row = t / (size_t)a.quads;                          // of the pair
    const int x0 = 4 * (int)(t % (size_t)a.quads);
    if (row >= 2 * (size_t)a.h) return;
    const int y = (int)(row % (size_t)a.h);                          // of its image
    const uint8_t *I = a.img + (row - (size_t)y) * (size_t)a.w;
    const int ym = y > 0 ? y - 1 : (a.h > 1 ? 1 : 0), yp = y + 1 < a.h ? y + 1 : (a.h > 1 ? a.h - 2 : 0);   // reflected rows
    const uint8_t *r0 = I + (size_t)ym * a.w, *r1 = I + (size_t)y * a.w, *r2 = I + (size_t)yp * a.w;
    int s[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int x = x0 - 1 + k;
        s[k] = x >= 0 && x < a.w ? (int)r0[x] + 2 * (int)r1[x] + (int)r2[x] : 0;
    }
    uint32_t out[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x0 + k;
        out[k] = x == 0 || x >= a.w - 1 ? (uint32_t)a.cap : (uint32_t)(min(max(s[k + 2] - s[k], -a.cap), a.cap) + a.cap);
    }
    const size_t o = row * (size_t)a.w + (size_t)x0;                 // a.pre is aligned: the offset decides
    if (x0 + 4 <= a.w && (o & 3) == 0) {
        *reinterpret_cast<uint32_t *>(a.pre + o) = out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24;
        return;
    }
    for (int k = 0; k < 4 && x0 + k < a.w; k++) a.pre[o + k] = (uint8_t)out[k];
}
__global__ __launch_bounds__(kBmThreads) void bm_prefilter(PrefilterArgs a) { prefilter_frame(a); }
// the same grid x frames (blockIdx.y); both strides are multiples of 16 bytes
struct PrefilterBatchArgs { PrefilterArgs a; size_t img_stride, pre_stride; };
__global__ __launch_bounds__(kBmThreads) void fb_prefilter(PrefilterBatchArgs g)
{
    PrefilterArgs a = g.a;
    a.img += blockIdx.y * g.img_stride;
    a.pre += blockIdx.y * g.pre_stride;
    prefilter_frame(a);
}

__device__ __forceinline__ bool bm_defined(int x, int y, int w, int h, const BmParams &b)
{
    return y >= b.r && y <= h - 1 - b.r && x >= b.nd - 1 + b.r && x <= w - 1 - b.r;
}

// The nw <= 6 dwords of a window row that starts at byte o (any alignment) of the prefiltered pair: nw + 1 aligned dword loads, each
// dword of the row formed from two neighbours with v_alignbyte_b32.  The last load ends at most 7 bytes behind the row (kBmPad).
__device__ __forceinline__ void bm_row(const uint32_t *pre, size_t o, int nw, uint32_t row[kBmRowDwords])
{
    const uint32_t *a = pre + (o >> 2);
    const uint32_t sh = (uint32_t)o & 3;
    uint32_t wd[kBmRowDwords + 1];
#pragma unroll
    for (int k = 0; k <= kBmRowDwords; k++) wd[k] = k <= nw ? a[k] : 0u;
#pragma unroll
    for (int k = 0; k < kBmRowDwords; k++) row[k] = __builtin_amdgcn_alignbyte(wd[k + 1], wd[k], sh);
}

// bm_pixel: the disparity of the defined pixel (x, y), by one wave; lane = disparity d, every lane returns the value.  Per window row the
// left segment is the same for all lanes and lane d's right segment starts one byte below lane d - 1's; both are read in place (the
// strip of a wave is (2r + 1) x (nd + 2r) bytes, it stays in the cache).  The (2r + 1)-byte row is padded to whole dwords with zero bytes
// on both sides, so v_sad_u8 sums four absolute differences at a time; T comes from the same left dwords against cap in every byte.
// The minimum with its tie rule is one wave reduction on SAD << 8 | (63 - d): smallest SAD, then largest d (SAD <= 441 * 126 < 2^16).
// Lanes >= nd read what lane nd - 1 reads and carry the largest key.
__device__ __forceinline__ int bm_pixel(const uint8_t *pre8, size_t px, int w, int x, int y, const BmParams &b, int lane)
{
    const uint32_t *pre = reinterpret_cast<const uint32_t *>(pre8);
    const int nb = 2 * b.r + 1, nw = (nb + 3) >> 2;
    const uint32_t tail = 0xffffffffu >> (8 * (4 * nw - nb));        // nb is odd: one or three bytes of the last dword count
    const uint32_t capw = (uint32_t)b.cap * 0x01010101u;
    const int d = min(lane, b.nd - 1);
    uint32_t sad = 0, T = 0;
    for (int dy = -b.r; dy <= b.r; dy++) {
        const size_t ol = (size_t)(y + dy) * (size_t)w + (size_t)(x - b.r);
        uint32_t L[kBmRowDwords], R[kBmRowDwords];
        bm_row(pre, ol, nw, L);
        bm_row(pre, px + ol - (size_t)d, nw, R);
#pragma unroll
        for (int k = 0; k < kBmRowDwords; k++) {
            if (k >= nw) break;
            const uint32_t mask = k == nw - 1 ? tail : 0xffffffffu;
            const uint32_t l = L[k] & mask;
            sad = __builtin_amdgcn_sad_u8(l, R[k] & mask, sad);
            T = __builtin_amdgcn_sad_u8(l, capw & mask, T);
        }
    }
    uint32_t key = lane < b.nd ? sad << 8 | (uint32_t)(63 - lane) : 0xffffffffu;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o));
    key = __builtin_amdgcn_readfirstlane(key);
    const int m = (int)(key >> 8), D = 63 - (int)(key & 255u);
    if ((int)T < b.tex) return kBmInvalid;
    if (b.ratio > 0) {
        const int thresh = m + m * b.ratio / 100;                     // m * ratio <= 55 566 * 100
        if (__ballot(lane < b.nd && abs(lane - D) > 1 && (int)sad <= thresh) != 0) return kBmInvalid;
    }
    const int at_p = D == 0 ? 1 : D == b.nd - 1 ? b.nd - 2 : D - 1, at_n = D == 0 ? 1 : D == b.nd - 1 ? b.nd - 2 : D + 1;
    const int p = (int)__builtin_amdgcn_readlane(sad, at_p), n = (int)__builtin_amdgcn_readlane(sad, at_n);
    const int q = p + n - 2 * m + abs(p - n);
    return (D * 256 + (q != 0 ? (p - n) * 256 / q : 0) + 15) >> 4;    // `/` truncates toward zero; the sum is never negative
}

// bm_keypoints: disparity_gather for a frame that arrives as its rectified pair -- one wave per keypoint computes the disparity at the
// keypoint's pixel, lane 0 writes the record
struct BmKeypointArgs {
    const float2 *kp;             // n, in the frame's slot
    const uint8_t *pre;           // 2 h x w: the prefiltered pair
    float4 *rec;                  // n, in the frame's slot
    int32_t n, w, h;
    BmParams b;
    DispQ q;
};
__device__ __forceinline__ void keypoints_frame(const BmKeypointArgs &g)
{
    const int i = blockIdx.x * kBmWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= g.n) return;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    int x, y;
    if (pixel_of(g.kp[i], g.w, g.h, &x, &y)) {
        int v = kBmInvalid;
        if (bm_defined(x, y, g.w, g.h, g.b)) v = bm_pixel(g.pre, (size_t)g.w * g.h, g.w, x, y, g.b, lane);
        const float3 p = point_of_disparity((float)v, x, y, g.q);
        r = make_float4(p.x, p.y, p.z, 1.0f);
    }
    if (lane == 0) g.rec[i] = r;
}
__global__ __launch_bounds__(kBmThreads) void bm_keypoints(BmKeypointArgs g) { keypoints_frame(g); }
// The grid of the largest possible frame x frames (blockIdx.y).  kp / rec: the rows of slot 0 of the store, frame f has those of slot[f];
// its keypoint count is the sum of the eight kept counts the detector left at out + f * out_stride, read here, so no count travels to the
// host in mid-call.  A wave beyond the count leaves at once.
struct BmKeypointBatchArgs { BmKeypointArgs a; const uint8_t *out; size_t pre_stride, out_stride; int32_t slot_kp; uint32_t slot[kFramePutGroup]; };
__global__ __launch_bounds__(kBmThreads) void fb_keypoints(BmKeypointBatchArgs g)
{
    const size_t f = blockIdx.y, at = (size_t)g.slot[f] * (size_t)g.slot_kp;
    const int32_t *counts = reinterpret_cast<const int32_t *>(g.out + f * g.out_stride);
    BmKeypointArgs a = g.a;
    a.n = 0;
#pragma unroll
    for (int l = 0; l < CHIP_ORB_MAX_LEVELS; l++) a.n += counts[l];
    a.kp += at; a.rec += at; a.pre += f * g.pre_stride;
    keypoints_frame(a);
}

// bm_dense: the same body at every pixel, one wave per pixel (the definition made callable: chip_stereo_bm; not a hot path)
struct BmDenseArgs {
    const uint8_t *pre;           // 2 h x w
    int16_t *disp;                // h x w
    int32_t w, h;
    BmParams b;
};
__global__ __launch_bounds__(kBmThreads) void bm_dense(BmDenseArgs g)
{
    const size_t px = (size_t)g.w * g.h;
    const size_t i = (size_t)blockIdx.x * kBmWaves + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= px) return;
    const int y = (int)(i / (size_t)g.w), x = (int)(i % (size_t)g.w);
    int v = kBmInvalid;
    if (bm_defined(x, y, g.w, g.h, g.b)) v = bm_pixel(g.pre, px, g.w, x, y, g.b, lane);
    if (lane == 0) g.disp[i] = (int16_t)v;
}

// ------------------------------------------------------------------------------------------------ rectification
// The definition is in include/cerebro_hip.h ("a frame from its raw stereo pair"): this project's own, modelled on cv::remap with
// INTER_LINEAR, float maps and BORDER_CONSTANT 0; all in int32 once the host has quantised the maps to 1/32 pixel.
constexpr int kRectPix = 4;            // consecutive pixels of a row per thread: one 32-bit store
constexpr int kRectLanes = 64;         // threads along a row: a workgroup spans kRectLanes * kRectPix = 256 pixels of a row ...
constexpr int kRectRows = 4;           // ... on four rows
constexpr int kRectThreads = kRectLanes * kRectRows;

// S(I, qx, qy) of the header: four bytes, each 0 outside the image, weighed in 1/32 and rounded half up
__device__ __forceinline__ int rect_sample(const uint8_t *I, int w, int h, int qx, int qy)
{
    const int x0 = qx >> 5, a = qx & 31, y0 = qy >> 5, b = qy & 31;
    const bool xi0 = (unsigned)x0 < (unsigned)w, xi1 = (unsigned)(x0 + 1) < (unsigned)w;
    const bool yi0 = (unsigned)y0 < (unsigned)h, yi1 = (unsigned)(y0 + 1) < (unsigned)h;
    const uint8_t *r0 = I + ((ptrdiff_t)y0 * w + x0), *r1 = r0 + w;     // dereferenced only where the tap is inside
    const int p00 = yi0 && xi0 ? (int)r0[0] : 0, p01 = yi0 && xi1 ? (int)r0[1] : 0;
    const int p10 = yi1 && xi0 ? (int)r1[0] : 0, p11 = yi1 && xi1 ? (int)r1[1] : 0;
    return (p00 * (32 - a) * (32 - b) + p01 * a * (32 - b) + p10 * (32 - a) * b + p11 * a * b + 512) >> 10;
}

// rectify_pair: both eyes (grid z) and both stages in one launch.  The quantised maps lie interleaved, (qx, qy) per pixel: eye e has
// `stages` planes of w h entries at q + e * stages * w h, stage 1 first.  With two stages an output pixel reads its stage-2 entry and
// makes each of its four taps of the undistorted image U -- never written anywhere -- from that tap's stage-1 entry and four raw bytes,
// rounded to a byte as the two-pass form rounds it, so the result is the two-pass result bit for bit.  A thread makes kRectPix pixels
// and stores them as bm_prefilter does: one dword where they are inside the row and the address allows, bytes otherwise.
struct RectifyArgs {
    const uint8_t *raw;           // eyes x h x w
    uint8_t *out;                 // eyes x h x w
    const int2 *q;                // eyes x stages x h x w
    int32_t w, h, stages;
};
// the body is rectify_pair_body.inc (see there why it is text)
__global__ __launch_bounds__(kRectThreads) void rectify_pair(RectifyArgs g)
{
#define RECT_EYE blockIdx.z
#define RECT_FRAME(p) (p)
#include "rectify_pair_body.inc"
#undef RECT_FRAME
#undef RECT_EYE
}
// grid z = eye + 2 * frame: the pairs of all frames through the one set of maps; the stride (both pairs' alike) is a multiple of 16 bytes
struct RectifyBatchArgs { RectifyArgs a; size_t stride; };
__global__ __launch_bounds__(kRectThreads) void fb_rectify(RectifyBatchArgs batch)
{
    const RectifyArgs &g = batch.a;
#define RECT_EYE (blockIdx.z & 1)
#define RECT_FRAME(p) ((p) + (size_t)(blockIdx.z >> 1) * batch.stride)
#include "rectify_pair_body.inc"
#undef RECT_FRAME
#undef RECT_EYE
}

// ------------------------------------------------------------------------------------------------ host side
void frame_store_destroy(Ctx *c)
{
    delete c->frame_store;
    c->frame_store = nullptr;
}

// the ctx's FrameStore, created empty on first use (as orb_state): no device memory before a call needs it.  Null: CHIP_ERR_OOM
static FrameStore *frame_store(Ctx *c)
{
    if (!c->frame_store) c->frame_store = new (std::nothrow) FrameStore();
    return c->frame_store;
}

// the prefilter of the pair staged in fs->stage into bm_pre (reserved by the caller)
static hipError_t launch_bm_prefilter(FrameStore *fs, hipStream_t s, int32_t w, int32_t h, const BmParams &b)
{
    const PrefilterArgs a{fs->stage, fs->bm_pre, w, h, (w + 3) / 4, b.cap};
    const size_t threads = 2 * (size_t)h * (size_t)a.quads;
    hipLaunchKernelGGL(bm_prefilter, dim3((unsigned)((threads + kBmThreads - 1) / kBmThreads)), dim3(kBmThreads), 0, s, a);
    return hipGetLastError();
}

// the records of the n >= 1 keypoints in the slot rows at `at`, from the prefiltered pair in bm_pre
static hipError_t launch_bm_keypoints(FrameStore *fs, hipStream_t s, size_t at, int32_t n, int32_t w, int32_t h, const BmParams &b, const DispQ &q)
{
    const BmKeypointArgs g{fs->store_kp + at, fs->bm_pre, fs->store_rec + at, n, w, h, b, q};
    hipLaunchKernelGGL(bm_keypoints, dim3((n + kBmWaves - 1) / kBmWaves), dim3(kBmThreads), 0, s, g);
    return hipGetLastError();
}

static hipError_t launch_rectify(hipStream_t s, const uint8_t *raw, uint8_t *out, const int2 *q, int32_t w, int32_t h, int32_t stages, int32_t eyes)
{
    const RectifyArgs a{raw, out, q, w, h, stages};
    const dim3 grid((unsigned)((w + kRectLanes * kRectPix - 1) / (kRectLanes * kRectPix)), (unsigned)((h + kRectRows - 1) / kRectRows), (unsigned)eyes);
    hipLaunchKernelGGL(rectify_pair, grid, dim3(kRectThreads), 0, s, a);
    return hipGetLastError();
}

// The slot transaction of a put: the slot of a known id (replace), else the first free one; rows at `at`.  Nothing of the store changes
// before commit() or abandon().  match_mu held.
struct SlotPut {
    FrameStore *fs;
    int64_t id;
    int32_t k = -1;               // -1: the store is full
    bool replace = false;
    size_t at = 0;
    // cursor (the puts of one group, none of them committed yet): a new id takes the first free slot at or behind *cursor and moves it on
    SlotPut(FrameStore *store, int64_t frame_id, int32_t *cursor = nullptr) : fs(store), id(frame_id)
    {
        const auto known = fs->slot_of.find(id);
        replace = known != fs->slot_of.end();
        if (replace) k = known->second;
        for (int32_t j = cursor ? *cursor : 0; k < 0 && j < fs->n_slots; j++)
            if (!fs->slots[(size_t)j].used) k = j;
        if (cursor && !replace && k >= 0) *cursor = k + 1;
        if (k >= 0) at = (size_t)k * (size_t)fs->slot_kp;
    }
    void commit(int32_t n, int32_t w, int32_t h)
    {
        fs->slots[(size_t)k] = FrameStore::StoredFrame{id, n, w, h, true};
        if (!replace) { fs->slot_of[id] = k; fs->n_frames++; }
    }
    void abandon()                // the device work failed part-way: the rows of a replaced id are undefined now, and the id leaves the store
    {
        if (replace) { fs->slots[(size_t)k] = FrameStore::StoredFrame(); fs->slot_of.erase(id); fs->n_frames--; }
    }
};

// Q(0,3), (1,3), (2,3), (3,2), (3,3) of the row-major 4 x 4, each narrowed to float as CameraGeometry.cpp:494-498 does
static DispQ disp_q(const double Q[16])
{
    return DispQ{(float)Q[3], (float)Q[7], (float)Q[11], (float)Q[14], (float)Q[15]};
}

// the parameter table of the header; p null: the defaults
static int bm_params(const chip_stereo_bm_params *p, BmParams *b)
{
    chip_stereo_bm_params d;
    chip_stereo_bm_params_default(&d);
    if (p) d = *p;
    if (d.num_disparities != 16 && d.num_disparities != 32 && d.num_disparities != 48 && d.num_disparities != 64) return CHIP_ERR_UNSUPPORTED;
    if (d.block_size < 5 || d.block_size > 4 * kBmRowDwords - 3 || d.block_size % 2 == 0) return CHIP_ERR_UNSUPPORTED;
    if (d.prefilter_cap < 1 || d.prefilter_cap > 63 || d.texture_threshold < 0) return CHIP_ERR_UNSUPPORTED;
    if (d.uniqueness_ratio < 0 || d.uniqueness_ratio > 100) return CHIP_ERR_UNSUPPORTED;
    *b = BmParams{d.num_disparities, d.block_size / 2, d.prefilter_cap, d.texture_threshold, d.uniqueness_ratio};
    return CHIP_OK;
}

// The put of a frame whose descriptors and keypoints come from the host (chip_frame_put, chip_frame_put_disparity,
// chip_frame_put_stereo), the arguments checked: the slot, the staging buffer of stage_bytes (pre_bytes != 0: the prefiltered pair as
// well), the two row uploads, then records(fs, s, at) -- which stages what the frame arrives as and launches the kernels that write the
// slot's records -- and the wait.  A frame of no keypoints is committed without touching the device.
struct PutRows { const uint8_t *desc; const float *kp_xy; int32_t n, w, h; };
template <class Records>
static int put_frame(chip_ctx *c, int64_t id, const PutRows &f, size_t stage_bytes, size_t pre_bytes, Records records)
{
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    FrameStore *fs = c->frame_store;
    if (!fs || fs->n_slots == 0) return CHIP_ERR_BUSY;
    if (f.n > fs->slot_kp) return CHIP_ERR_UNSUPPORTED;
    SlotPut put(fs, id);
    if (put.k < 0) return CHIP_ERR_OOM;
    CHIP_HIP(c, hipSetDevice(c->device));
    if (f.n > 0) {
        int rc = fs->stage.reserve(c, stage_bytes);                  // the last step that can fail before the slot is written
        if (rc == CHIP_OK && pre_bytes) rc = fs->bm_pre.reserve(c, pre_bytes);   // (a regrow pauses the resident scan by itself)
        if (rc != CHIP_OK) return rc;
        hipStream_t s = match_stream(c);
        hipError_t e = hipMemcpyAsync(fs->store_desc + put.at * CHIP_ORB_DESC_BYTES, f.desc, (size_t)f.n * CHIP_ORB_DESC_BYTES, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(fs->store_kp + put.at, f.kp_xy, (size_t)f.n * sizeof(float2), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = records(fs, s, put.at);
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // the caller's arrays are free again; a later match is ordered behind the put anyway
        if (e != hipSuccess) {
            put.abandon();
            CHIP_HIP(c, e);
        }
    }
    put.commit(f.n, f.w, f.h);
    return CHIP_OK;
}

// A frame from its rectified pair and nothing else: the detector and the descriptor (orb.hip) run on the left image where the pair is
// staged, orb_describe writes the slot's descriptor and keypoint rows, and the block matcher makes the records as in
// chip_frame_put_stereo.  What comes back is the eight kept counts.  raw: the pair is the cameras' own (chip_frame_put_raw_orb_stereo)
// -- it is staged behind the place of the rectified pair, rectify_pair writes that pair through the ctx's maps, and the rest is the same.
static int put_orb_stereo(chip_ctx *c, int64_t id, int32_t width, int32_t height, const uint8_t *left, const uint8_t *right,
                          const chip_orb_params *orb, const chip_stereo_bm_params *bm, const double Q_rowmajor[16], int32_t *n, bool raw)
{
    if (!c || !left || !right || !Q_rowmajor || !n) return CHIP_ERR_INVALID_ARG;
    chip_orb_params d;
    int rc = orb_check(width, height, orb, &d);
    if (rc != CHIP_OK) return rc;
    BmParams b;
    rc = bm_params(bm, &b);
    if (rc != CHIP_OK) return rc;
    const DispQ q = disp_q(Q_rowmajor);
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    FrameStore *fs = c->frame_store;
    if (!fs || fs->n_slots == 0) return CHIP_ERR_BUSY;
    if (raw && fs->rect_stages == 0) return CHIP_ERR_BUSY;         // no maps
    if (raw && (width != fs->rect_w || height != fs->rect_h)) return CHIP_ERR_INVALID_ARG;
    if (d.n_features > fs->slot_kp) return CHIP_ERR_UNSUPPORTED;   // the slot must hold whatever the detector keeps
    SlotPut put(fs, id);
    if (put.k < 0) return CHIP_ERR_OOM;
    CHIP_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    rc = fs->stage.reserve(c, (raw ? 4 : 2) * px);
    if (rc == CHIP_OK) rc = fs->bm_pre.reserve(c, 2 * px + kBmPad);
    if (rc != CHIP_OK) return rc;
    hipStream_t s = match_stream(c);
    uint8_t *stage = fs->stage;
    uint8_t *in = raw ? stage + 2 * px : stage;                    // where the caller's pair goes
    int32_t total = 0;
    const auto run = [&]() -> int {
        CHIP_HIP(c, hipMemcpyAsync(in, left, px, hipMemcpyHostToDevice, s));
        CHIP_HIP(c, hipMemcpyAsync(in + px, right, px, hipMemcpyHostToDevice, s));
        if (raw) CHIP_HIP(c, launch_rectify(s, in, stage, fs->rect_maps, width, height, fs->rect_stages, 2));
        const int e = orb_enqueue(c, s, nullptr, stage, width, height, d, true, fs->store_desc + put.at * CHIP_ORB_DESC_BYTES, fs->store_kp + put.at,
                                  8 * sizeof(int32_t));
        if (e != CHIP_OK) return e;
        CHIP_HIP(c, launch_bm_prefilter(fs, s, width, height, b));   // runs while the counts travel
        CHIP_HIP(c, hipStreamSynchronize(s));
        const int f = orb_finished(c, true, d.n_features, &total, nullptr);
        if (f != CHIP_OK || total == 0) return f;
        CHIP_HIP(c, launch_bm_keypoints(fs, s, put.at, total, width, height, b, q));
        CHIP_HIP(c, hipStreamSynchronize(s));
        return CHIP_OK;
    };
    rc = run();
    if (rc != CHIP_OK) {
        // CHIP_ERR_OOM: a buffer of the detector could not grow, which is decided before its first launch -- the slot is as it was
        if (rc != CHIP_ERR_OOM) put.abandon();
        return rc;
    }
    put.commit(total, width, height);
    *n = total;
    return CHIP_OK;
}

// ---- the batched put: F pairs of one rig, walked in groups of put_group() frames -- ONE launch per stage and ONE wait per group
static int32_t put_group(int32_t width, int32_t height)
{
    const size_t g = ((size_t)1 << 23) / ((size_t)width * (size_t)height);   // level-0 pixels of a group <= 2^23
    return g < 1 ? 1 : g > (size_t)kFramePutGroup ? kFramePutGroup : (int32_t)g;
}

// the checks of the batched calls that need neither a ctx nor the pairs: F and the parameters
static int put_batch_check(int32_t width, int32_t height, const chip_orb_params *orb, int32_t F, chip_orb_params *d)
{
    if (F < 1) return CHIP_ERR_INVALID_ARG;
    if (F > CHIP_FRAME_MAX_PUT) return CHIP_ERR_UNSUPPORTED;
    return orb_check(width, height, orb, d);
}

// A group of G frames in flight: pair f is staged at f * pair_stride (a multiple of 16 bytes: every frame's rows keep the alignment the
// kernels' wide stores ask of frame 0), the raw pairs behind the places of all the rectified ones, the prefiltered pairs likewise at
// f * pre_stride.  The detector's batch entries write the descriptor and keypoint rows of each frame's slot, fb_keypoints the records
// from the kept counts it reads in device memory; the G x 8 counts come back in one copy in front of the one wait.
static int put_orb_stereo_batch(chip_ctx *c, const int64_t *ids, int32_t F, int32_t width, int32_t height, const uint8_t *const *left,
                                const uint8_t *const *right, const chip_orb_params *orb, const chip_stereo_bm_params *bm,
                                const double Q_rowmajor[16], int32_t *n, bool raw)
{
    if (!c || !ids || !left || !right || !Q_rowmajor || !n || F < 1) return CHIP_ERR_INVALID_ARG;
    {
        std::vector<int64_t> sorted;
        const int32_t look = F > CHIP_FRAME_MAX_PUT ? CHIP_FRAME_MAX_PUT : F;       // (a longer call is refused below whatever it holds)
        try { sorted.assign(ids, ids + look); } catch (const std::bad_alloc &) { return CHIP_ERR_OOM; }
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return CHIP_ERR_INVALID_ARG;
        for (int32_t f = 0; f < look; f++)
            if (!left[f] || !right[f]) return CHIP_ERR_INVALID_ARG;
    }
    chip_orb_params d;
    int rc = put_batch_check(width, height, orb, F, &d);
    if (rc != CHIP_OK) return rc;
    BmParams b;
    rc = bm_params(bm, &b);
    if (rc != CHIP_OK) return rc;
    const DispQ q = disp_q(Q_rowmajor);
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    FrameStore *fs = c->frame_store;
    if (fs && fs->n_slots > 0 && d.n_features > fs->slot_kp) return CHIP_ERR_UNSUPPORTED;   // a slot must hold whatever the detector keeps
    if (!fs || fs->n_slots == 0) return CHIP_ERR_BUSY;
    if (raw && fs->rect_stages == 0) return CHIP_ERR_BUSY;         // no maps
    if (raw && (width != fs->rect_w || height != fs->rect_h)) return CHIP_ERR_INVALID_ARG;
    int32_t fresh = 0;
    for (int32_t f = 0; f < F; f++) fresh += fs->slot_of.find(ids[f]) == fs->slot_of.end();
    if (fresh > fs->n_slots - fs->n_frames) return CHIP_ERR_OOM;   // all or nothing: the store is as it was
    CHIP_HIP(c, hipSetDevice(c->device));
    const int32_t group = put_group(width, height), widest = F < group ? F : group;
    const size_t px = (size_t)width * height;
    const size_t pair_stride = (2 * px + 15) & ~(size_t)15, pre_stride = (2 * px + kBmPad + 15) & ~(size_t)15;
    const size_t stage_bytes = (raw ? 2 : 1) * (size_t)widest * pair_stride, pre_bytes = (size_t)widest * pre_stride;
    {   // everything a group needs, the detector's scratch included, inside one pause
        const bool grow = fs->stage.capacity() < stage_bytes || fs->bm_pre.capacity() < pre_bytes || orb_batch_reserve(c, widest, width, height, d, true) != 0;
        ResidentPause paused(c, grow);
        rc = fs->stage.reserve(c, stage_bytes);
        if (rc == CHIP_OK) rc = fs->bm_pre.reserve(c, pre_bytes);
        if (rc == CHIP_OK) rc = orb_batch_reserve(c, widest, width, height, d, false);
        if (rc != CHIP_OK) return rc;
    }
    hipStream_t s = match_stream(c);
    uint8_t *stage = fs->stage;
    uint8_t *in = raw ? stage + (size_t)widest * pair_stride : stage;   // where the callers' pairs go
    fs->last_groups = fs->last_launches = fs->last_waits = 0;
    for (int32_t f = 0; f < F; f++) n[f] = -1;
    for (int32_t g0 = 0; g0 < F; g0 += group) {
        const int32_t G = F - g0 < group ? F - g0 : group;
        std::vector<SlotPut> puts;
        try { puts.reserve((size_t)G); } catch (const std::bad_alloc &) { return CHIP_ERR_OOM; }   // (this group and the later ones are untouched)
        int32_t slot[kFramePutGroup] = {}, cursor = 0;
        for (int32_t f = 0; f < G; f++) {
            puts.emplace_back(fs, ids[g0 + f], &cursor);
            if (puts.back().k < 0) return CHIP_ERR_OOM;               // cannot happen: the free slots were counted above
            slot[f] = puts.back().k;
        }
        const int32_t *counts = nullptr;
        fs->last_groups++;
        const auto run = [&]() -> int {
            for (int32_t f = 0; f < G; f++) {
                CHIP_HIP(c, hipMemcpyAsync(in + (size_t)f * pair_stride, left[g0 + f], px, hipMemcpyHostToDevice, s));
                CHIP_HIP(c, hipMemcpyAsync(in + (size_t)f * pair_stride + px, right[g0 + f], px, hipMemcpyHostToDevice, s));
            }
            if (raw) {
                const RectifyBatchArgs a{RectifyArgs{in, stage, fs->rect_maps, width, height, fs->rect_stages}, pair_stride};
                const dim3 grid((unsigned)((width + kRectLanes * kRectPix - 1) / (kRectLanes * kRectPix)), (unsigned)((height + kRectRows - 1) / kRectRows),
                                2u * (unsigned)G);
                hipLaunchKernelGGL(fb_rectify, grid, dim3(kRectThreads), 0, s, a);
                CHIP_HIP(c, hipGetLastError());
                fs->last_launches++;
            }
            const uint8_t *out = nullptr;
            size_t out_stride = 0;
            const int e = orb_batch_enqueue(c, s, stage, pair_stride, G, width, height, d, fs->store_desc, fs->store_kp, fs->slot_kp, slot,
                                            &fs->last_launches, &out, &out_stride);
            if (e != CHIP_OK) return e;
            {
                const PrefilterBatchArgs a{PrefilterArgs{stage, fs->bm_pre, width, height, (width + 3) / 4, b.cap}, pair_stride, pre_stride};
                const size_t threads = 2 * (size_t)height * (size_t)a.a.quads;
                hipLaunchKernelGGL(fb_prefilter, dim3((unsigned)((threads + kBmThreads - 1) / kBmThreads), (unsigned)G), dim3(kBmThreads), 0, s, a);
                CHIP_HIP(c, hipGetLastError());
                fs->last_launches++;
            }
            {
                BmKeypointBatchArgs a{BmKeypointArgs{fs->store_kp, fs->bm_pre, fs->store_rec, 0, width, height, b, q}, out, pre_stride, out_stride,
                                      fs->slot_kp, {}};
                for (int f = 0; f < kFramePutGroup; f++) a.slot[f] = (uint32_t)slot[f < G ? f : 0];
                hipLaunchKernelGGL(fb_keypoints, dim3((unsigned)((d.n_features + kBmWaves - 1) / kBmWaves), (unsigned)G), dim3(kBmThreads), 0, s, a);
                CHIP_HIP(c, hipGetLastError());
                fs->last_launches++;
            }
            const int k = orb_batch_counts(c, s, G, &counts);
            if (k != CHIP_OK) return k;
            fs->last_waits++;
            CHIP_HIP(c, hipStreamSynchronize(s));
            for (int32_t f = 0; f < G; f++) {
                int32_t total = 0;
                for (int l = 0; l < CHIP_ORB_MAX_LEVELS; l++) total += counts[8 * f + l];
                if (total < 0 || total > d.n_features) return CHIP_ERR_HIP;   // cannot happen: the kept lists are bounded by the quotas
            }
            return CHIP_OK;
        };
        rc = run();
        if (rc != CHIP_OK) {                  // the groups before this one stay; this one's ids leave the store; the later ones are untouched
            for (SlotPut &p : puts) p.abandon();
            return rc;
        }
        for (int32_t f = 0; f < G; f++) {
            int32_t total = 0;
            for (int l = 0; l < CHIP_ORB_MAX_LEVELS; l++) total += counts[8 * f + l];
            puts[(size_t)f].commit(total, width, height);
            n[g0 + f] = total;
        }
    }
    return CHIP_OK;
}

// Q of the header: a map value in 1/32 pixel.  The product is exact in float; rintf rounds to nearest, ties to even (the default mode)
static inline int32_t rect_quantize(float m)
{
    if (m != m) return -64;
    return (int32_t)rintf(32.0f * fminf(fmaxf(m, -2.0f), 32768.0f));
}

static void rect_quantize_plane(const float *mx, const float *my, size_t px, int2 *q)
{
    for (size_t i = 0; i < px; i++) q[i] = make_int2(rect_quantize(mx[i]), rect_quantize(my[i]));
}

}  // namespace chip

using namespace chip;

// ------------------------------------------------------------------------------------------------ the frame store
extern "C" int chip_build_has_frame_store(void) { return 1; }

extern "C" int chip_frame_store_reserve(chip_ctx *c, int32_t n_slots, int32_t slot_keypoints)
{
    if (!c || n_slots < 1 || slot_keypoints < 1 || slot_keypoints > kMatchMax) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    MatchState *ms = nullptr;
    int rc = match_state(c, &ms);            // a store means matches on it: the runs on stored frames find the match state in place
    if (rc != CHIP_OK) return rc;
    FrameStore *fs = frame_store(c);
    if (!fs) return CHIP_ERR_OOM;
    if (fs->n_slots == n_slots && fs->slot_kp == slot_keypoints) return CHIP_OK;
    if (fs->n_frames > 0) return CHIP_ERR_BUSY;
    ResidentPause paused(c);                 // the frees and the three allocations inside one pause
    CHIP_HIP(c, hipStreamSynchronize(match_stream(c)));
    fs->store_desc.release(); fs->store_kp.release(); fs->store_rec.release();
    fs->n_slots = fs->slot_kp = 0;
    fs->slots.clear();
    const size_t rows = (size_t)n_slots * (size_t)slot_keypoints;
    rc = fs->store_desc.alloc(c, rows * CHIP_ORB_DESC_BYTES);
    if (rc == CHIP_OK) rc = fs->store_kp.alloc(c, rows);
    if (rc == CHIP_OK) rc = fs->store_rec.alloc(c, rows);
    if (rc != CHIP_OK) {                     // no store rather than part of one
        fs->store_desc.release(); fs->store_kp.release(); fs->store_rec.release();
        return rc;
    }
    fs->slots.assign((size_t)n_slots, FrameStore::StoredFrame());
    fs->n_slots = n_slots; fs->slot_kp = slot_keypoints;
    return CHIP_OK;
}

extern "C" int chip_frame_store_info(chip_ctx *c, int32_t *n_slots, int32_t *slot_keypoints, int32_t *n_frames)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    const FrameStore *fs = c->frame_store;
    if (n_slots) *n_slots = fs ? fs->n_slots : 0;
    if (slot_keypoints) *slot_keypoints = fs ? fs->slot_kp : 0;
    if (n_frames) *n_frames = fs ? fs->n_frames : 0;
    return CHIP_OK;
}

extern "C" int chip_frame_drop(chip_ctx *c, int64_t id)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    FrameStore *fs = c->frame_store;
    if (!fs) return CHIP_ERR_RANGE;
    const auto known = fs->slot_of.find(id);
    if (known == fs->slot_of.end()) return CHIP_ERR_RANGE;
    fs->slots[(size_t)known->second] = FrameStore::StoredFrame();
    fs->slot_of.erase(known);
    fs->n_frames--;
    return CHIP_OK;
}

extern "C" int chip_frame_read(chip_ctx *c, int64_t id, int32_t *n, int32_t *width, int32_t *height, uint8_t *desc, float *kp_xy, float *pts)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    FrameStore *fs = c->frame_store;
    if (!fs || fs->n_slots == 0) return CHIP_ERR_BUSY;
    const auto known = fs->slot_of.find(id);
    if (known == fs->slot_of.end()) return CHIP_ERR_RANGE;
    const FrameStore::Rows r = fs->rows(known->second);
    if (n) *n = r.n;
    if (width) *width = r.w;
    if (height) *height = r.h;
    if (r.n == 0 || (!desc && !kp_xy && !pts)) return CHIP_OK;
    CHIP_HIP(c, hipSetDevice(c->device));
    hipStream_t s = match_stream(c);
    const size_t m = (size_t)r.n;
    if (desc) CHIP_HIP(c, hipMemcpyAsync(desc, r.desc, m * CHIP_ORB_DESC_BYTES, hipMemcpyDeviceToHost, s));
    if (kp_xy) CHIP_HIP(c, hipMemcpyAsync(kp_xy, r.kp, m * sizeof(float2), hipMemcpyDeviceToHost, s));
    if (pts) CHIP_HIP(c, hipMemcpyAsync(pts, r.rec, m * sizeof(float4), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ frames from their 3-D images
// stages the image; frame_gather copies the records out of it
extern "C" int chip_frame_put(chip_ctx *c, int64_t id, const chip_match_frame *f)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_frame(f);
    if (rc != CHIP_OK) return rc;
    const size_t bytes = 3 * (size_t)f->width * f->height * sizeof(float);
    return put_frame(c, id, PutRows{f->desc, f->kp_xy, f->n, f->width, f->height}, bytes, 0, [&](FrameStore *fs, hipStream_t s, size_t at) {
        const hipError_t e = hipMemcpyAsync(fs->stage, f->xyz, bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        const GatherArgs g{fs->store_kp + at, reinterpret_cast<const float *>(fs->stage.get()), fs->store_rec + at, f->n, f->width, f->height};
        hipLaunchKernelGGL(frame_gather, dim3((f->n + kGatherThreads - 1) / kGatherThreads), dim3(kGatherThreads), 0, s, g);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------------------------------------ frames from their disparity maps
extern "C" int chip_build_has_disparity(void) { return 1; }

// stages the map; disparity_gather computes each record from the one value at the keypoint's pixel
extern "C" int chip_frame_put_disparity(chip_ctx *c, int64_t id, const uint8_t *desc, const float *kp_xy, int32_t n, int32_t width, int32_t height,
                                        const void *disparity, int32_t disp_type, const double Q_rowmajor[16])
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_frame(desc, kp_xy, n, width, height, disparity);   // the frame rules, on the disparity
    if (rc != CHIP_OK) return rc;
    if ((disp_type != CHIP_DISP_S16 && disp_type != CHIP_DISP_F32) || !Q_rowmajor) return CHIP_ERR_INVALID_ARG;
    const DispQ q = disp_q(Q_rowmajor);
    const size_t bytes = (size_t)width * height * (disp_type == CHIP_DISP_S16 ? sizeof(int16_t) : sizeof(float));
    return put_frame(c, id, PutRows{desc, kp_xy, n, width, height}, bytes, 0, [&](FrameStore *fs, hipStream_t s, size_t at) {
        const hipError_t e = hipMemcpyAsync(fs->stage, disparity, bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        const GatherDispArgs g{fs->store_kp + at, fs->stage, fs->store_rec + at, n, width, height, disp_type, q};
        hipLaunchKernelGGL(disparity_gather, dim3((n + kGatherThreads - 1) / kGatherThreads), dim3(kGatherThreads), 0, s, g);
        return hipGetLastError();
    });
}

extern "C" int chip_disparity_to_xyz(chip_ctx *c, const void *disparity, int32_t disp_type, int32_t width, int32_t height,
                                     const double Q_rowmajor[16], float *xyz)
{
    if (!c || !disparity || !Q_rowmajor || !xyz || width <= 0 || height <= 0) return CHIP_ERR_INVALID_ARG;
    if (disp_type != CHIP_DISP_S16 && disp_type != CHIP_DISP_F32) return CHIP_ERR_INVALID_ARG;
    if (width > kMaxImageSide || height > kMaxImageSide) return CHIP_ERR_UNSUPPORTED;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    FrameStore *fs = frame_store(c);
    if (!fs) return CHIP_ERR_OOM;
    const size_t px = (size_t)width * height;
    const size_t bytes = disp_type == CHIP_DISP_S16 ? px * sizeof(int16_t) : px * sizeof(float);
    int rc = fs->stage.reserve(c, bytes);
    if (rc == CHIP_OK) rc = fs->dense.reserve(c, 3 * px * sizeof(float));
    if (rc != CHIP_OK) return rc;
    hipStream_t s = match_stream(c);
    const DenseDispArgs a{fs->stage, reinterpret_cast<float *>(fs->dense.get()), width, height, disp_type, (width + 3) / 4, disp_q(Q_rowmajor)};
    const size_t threads = (size_t)height * (size_t)a.quads;
    CHIP_HIP(c, hipMemcpyAsync(fs->stage, disparity, bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(disparity_to_xyz, dim3((unsigned)((threads + kDenseThreads - 1) / kDenseThreads)), dim3(kDenseThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    CHIP_HIP(c, hipMemcpyAsync(xyz, fs->dense, 3 * px * sizeof(float), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ frames from their rectified pairs
extern "C" int chip_build_has_stereo_bm(void) { return 1; }

extern "C" void chip_stereo_bm_params_default(chip_stereo_bm_params *p)
{
    if (p) *p = chip_stereo_bm_params{64, 21, 31, 10, 15};           // cv::StereoBM::create(64, 21)
}

// stages the pair, left first; bm_prefilter and bm_keypoints compute each record from the disparity at the keypoint's pixel
extern "C" int chip_frame_put_stereo(chip_ctx *c, int64_t id, const uint8_t *desc, const float *kp_xy, int32_t n, int32_t width, int32_t height,
                                     const uint8_t *left, const uint8_t *right, const chip_stereo_bm_params *p, const double Q_rowmajor[16])
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    int rc = check_frame(desc, kp_xy, n, width, height, left);   // the frame rules, on the left image
    if (rc != CHIP_OK) return rc;
    if (!right || !Q_rowmajor) return CHIP_ERR_INVALID_ARG;
    BmParams b;
    rc = bm_params(p, &b);
    if (rc != CHIP_OK) return rc;
    const DispQ q = disp_q(Q_rowmajor);
    const size_t px = (size_t)width * height;
    return put_frame(c, id, PutRows{desc, kp_xy, n, width, height}, 2 * px, 2 * px + kBmPad, [&](FrameStore *fs, hipStream_t s, size_t at) {
        hipError_t e = hipMemcpyAsync(fs->stage, left, px, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(fs->stage + px, right, px, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = launch_bm_prefilter(fs, s, width, height, b);
        if (e == hipSuccess) e = launch_bm_keypoints(fs, s, at, n, width, height, b, q);
        return e;
    });
}

extern "C" int chip_stereo_bm(chip_ctx *c, const uint8_t *left, const uint8_t *right, int32_t width, int32_t height,
                              const chip_stereo_bm_params *p, int16_t *disparity)
{
    if (!c || !left || !right || !disparity || width <= 0 || height <= 0) return CHIP_ERR_INVALID_ARG;
    if (width > kMaxImageSide || height > kMaxImageSide) return CHIP_ERR_UNSUPPORTED;
    BmParams b;
    int rc = bm_params(p, &b);
    if (rc != CHIP_OK) return rc;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    FrameStore *fs = frame_store(c);
    if (!fs) return CHIP_ERR_OOM;
    const size_t px = (size_t)width * height;
    rc = fs->stage.reserve(c, 2 * px);
    if (rc == CHIP_OK) rc = fs->bm_pre.reserve(c, 2 * px + kBmPad);
    if (rc == CHIP_OK) rc = fs->dense.reserve(c, px * sizeof(int16_t));
    if (rc != CHIP_OK) return rc;
    hipStream_t s = match_stream(c);
    const BmDenseArgs a{fs->bm_pre, reinterpret_cast<int16_t *>(fs->dense.get()), width, height, b};
    CHIP_HIP(c, hipMemcpyAsync(fs->stage, left, px, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemcpyAsync(fs->stage + px, right, px, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, launch_bm_prefilter(fs, s, width, height, b));
    hipLaunchKernelGGL(bm_dense, dim3((unsigned)((px + kBmWaves - 1) / kBmWaves)), dim3(kBmThreads), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    CHIP_HIP(c, hipMemcpyAsync(disparity, a.disp, px * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

extern "C" int chip_frame_put_orb_stereo(chip_ctx *c, int64_t id, int32_t width, int32_t height, const uint8_t *left, const uint8_t *right,
                                         const chip_orb_params *orb, const chip_stereo_bm_params *bm, const double Q_rowmajor[16], int32_t *n)
{
    return put_orb_stereo(c, id, width, height, left, right, orb, bm, Q_rowmajor, n, false);
}

// ------------------------------------------------------------------------------------------------ frames from their raw pairs
extern "C" int chip_build_has_rectify(void) { return 1; }

extern "C" int chip_rectify_quantize(const float *map, int64_t count, int32_t *q)
{
    if (!map || !q || count < 0) return CHIP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < count; i++) q[i] = rect_quantize(map[i]);
    return CHIP_OK;
}

extern "C" int chip_remap(chip_ctx *c, const uint8_t *image, int32_t width, int32_t height, const float *map_x, const float *map_y, uint8_t *out)
{
    if (!c || !image || !map_x || !map_y || !out || width < 1 || height < 1) return CHIP_ERR_INVALID_ARG;
    if (width > kMaxImageSide || height > kMaxImageSide) return CHIP_ERR_UNSUPPORTED;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    FrameStore *fs = frame_store(c);
    if (!fs) return CHIP_ERR_OOM;
    const size_t px = (size_t)width * height;
    int rc = fs->stage.reserve(c, 2 * px);   // the result, the image behind it
    if (rc == CHIP_OK) rc = fs->remap_q.reserve(c, px);
    if (rc != CHIP_OK) return rc;
    try { fs->h_rect.resize(px); } catch (const std::bad_alloc &) { return CHIP_ERR_OOM; }
    rect_quantize_plane(map_x, map_y, px, fs->h_rect.data());
    hipStream_t s = match_stream(c);
    uint8_t *stage = fs->stage;
    CHIP_HIP(c, hipMemcpyAsync(fs->remap_q, fs->h_rect.data(), px * sizeof(int2), hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemcpyAsync(stage + px, image, px, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, launch_rectify(s, stage + px, stage, fs->remap_q, width, height, 1, 1));
    CHIP_HIP(c, hipMemcpyAsync(out, stage, px, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

extern "C" int chip_rectify_set_maps(chip_ctx *c, int32_t width, int32_t height, const float *lx1, const float *ly1, const float *lx2,
                                     const float *ly2, const float *rx1, const float *ry1, const float *rx2, const float *ry2)
{
    if (!c || !lx1 || !ly1 || !rx1 || !ry1 || width < 1 || height < 1) return CHIP_ERR_INVALID_ARG;
    const int n2 = (lx2 != nullptr) + (ly2 != nullptr) + (rx2 != nullptr) + (ry2 != nullptr);
    if (n2 != 0 && n2 != 4) return CHIP_ERR_INVALID_ARG;
    if (width > CHIP_ORB_MAX_SIDE || height > CHIP_ORB_MAX_SIDE) return CHIP_ERR_UNSUPPORTED;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    FrameStore *fs = frame_store(c);
    if (!fs) return CHIP_ERR_OOM;
    const int32_t stages = n2 ? 2 : 1;
    const size_t px = (size_t)width * height, entries = 2 * (size_t)stages * px;
    try { fs->h_rect.resize(entries); } catch (const std::bad_alloc &) { return CHIP_ERR_OOM; }
    fs->rect_stages = 0;                     // from here on the old maps are gone, whatever happens
    const int rc = fs->rect_maps.reserve(c, entries);   // (a regrow pauses the resident scan by itself)
    if (rc != CHIP_OK) return rc;
    int2 *q = fs->h_rect.data();
    rect_quantize_plane(lx1, ly1, px, q);
    if (n2) rect_quantize_plane(lx2, ly2, px, q + px);
    rect_quantize_plane(rx1, ry1, px, q + (size_t)stages * px);
    if (n2) rect_quantize_plane(rx2, ry2, px, q + (size_t)stages * px + px);
    hipStream_t s = match_stream(c);
    CHIP_HIP(c, hipMemcpyAsync(fs->rect_maps, q, entries * sizeof(int2), hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    fs->rect_w = width; fs->rect_h = height; fs->rect_stages = stages;
    return CHIP_OK;
}

extern "C" int chip_rectify_pair(chip_ctx *c, const uint8_t *left_raw, const uint8_t *right_raw, int32_t width, int32_t height,
                                 uint8_t *left_out, uint8_t *right_out)
{
    if (!c || !left_raw || !right_raw || !left_out || !right_out || width < 1 || height < 1) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    FrameStore *fs = c->frame_store;
    if (!fs || fs->rect_stages == 0) return CHIP_ERR_BUSY;
    if (width != fs->rect_w || height != fs->rect_h) return CHIP_ERR_INVALID_ARG;
    CHIP_HIP(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    const int rc = fs->stage.reserve(c, 4 * px);   // the rectified pair, the raw one behind it
    if (rc != CHIP_OK) return rc;
    hipStream_t s = match_stream(c);
    uint8_t *stage = fs->stage;
    CHIP_HIP(c, hipMemcpyAsync(stage + 2 * px, left_raw, px, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, hipMemcpyAsync(stage + 3 * px, right_raw, px, hipMemcpyHostToDevice, s));
    CHIP_HIP(c, launch_rectify(s, stage + 2 * px, stage, fs->rect_maps, width, height, fs->rect_stages, 2));
    CHIP_HIP(c, hipMemcpyAsync(left_out, stage, px, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipMemcpyAsync(right_out, stage + px, px, hipMemcpyDeviceToHost, s));
    CHIP_HIP(c, hipStreamSynchronize(s));
    return CHIP_OK;
}

extern "C" int chip_frame_put_raw_orb_stereo(chip_ctx *c, int64_t id, int32_t width, int32_t height, const uint8_t *left_raw,
                                             const uint8_t *right_raw, const chip_orb_params *orb, const chip_stereo_bm_params *bm,
                                             const double Q_rowmajor[16], int32_t *n)
{
    return put_orb_stereo(c, id, width, height, left_raw, right_raw, orb, bm, Q_rowmajor, n, true);
}

// ------------------------------------------------------------------------------------------------ many pairs per call
extern "C" int chip_build_has_frame_put_batch(void) { return 1; }

extern "C" int chip_frame_put_plan(int32_t width, int32_t height, const chip_orb_params *orb, int32_t raw, int32_t F, int32_t *group, int32_t *n_groups)
{
    if (!group || !n_groups || (raw != 0 && raw != 1)) return CHIP_ERR_INVALID_ARG;
    chip_orb_params d;
    const int rc = put_batch_check(width, height, orb, F, &d);
    if (rc != CHIP_OK) return rc;
    *group = put_group(width, height);
    *n_groups = (F + *group - 1) / *group;
    return CHIP_OK;
}

extern "C" int chip_frame_put_orb_stereo_batch(chip_ctx *c, const int64_t *ids, int32_t F, int32_t width, int32_t height, const uint8_t *const *left,
                                               const uint8_t *const *right, const chip_orb_params *orb, const chip_stereo_bm_params *bm,
                                               const double Q_rowmajor[16], int32_t *n)
{
    return put_orb_stereo_batch(c, ids, F, width, height, left, right, orb, bm, Q_rowmajor, n, false);
}

extern "C" int chip_frame_put_raw_orb_stereo_batch(chip_ctx *c, const int64_t *ids, int32_t F, int32_t width, int32_t height,
                                                   const uint8_t *const *left_raw, const uint8_t *const *right_raw, const chip_orb_params *orb,
                                                   const chip_stereo_bm_params *bm, const double Q_rowmajor[16], int32_t *n)
{
    return put_orb_stereo_batch(c, ids, F, width, height, left_raw, right_raw, orb, bm, Q_rowmajor, n, true);
}

extern "C" int chip_debug_frame_put_last(chip_ctx *c, int32_t *groups, int32_t *launches, int32_t *waits)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->match_mu);
    const FrameStore *fs = c->frame_store;
    if (groups) *groups = fs ? fs->last_groups : 0;
    if (launches) *launches = fs ? fs->last_launches : 0;
    if (waits) *waits = fs ? fs->last_waits : 0;
    return CHIP_OK;
}

// the rows chip_frame_read gave, back into a slot: three uploads, no kernel
extern "C" int chip_frame_put_records(chip_ctx *c, int64_t id, const uint8_t *desc, const float *kp_xy, const float *pts, int32_t n, int32_t width,
                                      int32_t height)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    const int rc = check_frame(desc, kp_xy, n, width, height, pts);   // the frame rules, on the records
    if (rc != CHIP_OK) return rc;
    for (int32_t i = 0; i < n; i++) {       // the fourth float is what the gather kernels write: 0.0f (no point) or 1.0f, bit for bit
        uint32_t w;
        std::memcpy(&w, pts + 4 * (size_t)i + 3, sizeof w);
        if (w != 0u && w != 0x3f800000u) return CHIP_ERR_INVALID_ARG;
    }
    return put_frame(c, id, PutRows{desc, kp_xy, n, width, height}, 0, 0, [&](FrameStore *fs, hipStream_t s, size_t at) {
        return hipMemcpyAsync(fs->store_rec + at, pts, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, s);
    });
}
