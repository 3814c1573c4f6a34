// frame_store.h -- what frames.hip (the frame store and everything that fills it) and match.hip (the match stage, which reads stored
// frames) share.  Internal: included by those two files only.
#pragma once
#include "chip_internal.h"
#include <unordered_map>
#include <vector>

namespace chip {

constexpr int kMatchMax = CHIP_MATCH_MAX_KEYPOINTS;
constexpr int kMaxImageSide = 16384;

// pixel of a keypoint as the reference indexes the 3-D image: (int)uv(1,k), (int)uv(0,k) (PointFeatureMatching.cpp:121,180) -- truncation
// of the float keypoint (exact as a double).  (-1, w) truncates into [0, w - 1]; anything else (NaN too) is outside the image.
__device__ __forceinline__ bool pixel_of(float2 p, int w, int h, int *x, int *y)
{
    if (!(p.x > -1.0f && p.x < (float)w && p.y > -1.0f && p.y < (float)h)) return false;
    *x = (int)p.x; *y = (int)p.y;
    return true;
}

// The frame store (chip_frame_store_reserve): n_slots slots of slot_kp keypoints each, 56 bytes per keypoint; rows never move after the
// reserve.  With it, the buffers that only frame calls use, grown on demand.  Ctx::frame_store, created on first use, under match_mu.
struct FrameStore {
    struct StoredFrame { int64_t id = 0; int32_t n = 0, w = 0, h = 0; bool used = false; };
    DevBuf<uint8_t> store_desc;
    DevBuf<float2> store_kp;
    DevBuf<float4> store_rec;
    int32_t n_slots = 0, slot_kp = 0, n_frames = 0;
    std::vector<StoredFrame> slots;
    std::unordered_map<int64_t, int32_t> slot_of;   // id -> slot
    // stage: the bytes of the call in flight -- the image of a put, or its disparity, or its rectified pair (a raw pair behind it); also
    // the input of the dense calls, whose 3-D image / int16 map is `dense` until it is copied out
    DevBuf<uint8_t> stage, dense;
    DevBuf<uint8_t> bm_pre;                     // the prefiltered pair of the stereo put (or of chip_stereo_bm) in flight, kBmPad bytes behind it
    // rectification: the quantised maps of chip_rectify_set_maps, [eye][stage][h][w] entries (qx, qy), and the one plane of the
    // chip_remap in flight.  Nothing of this exists before the first of those calls.
    DevBuf<int2> rect_maps, remap_q;
    std::vector<int2> h_rect;                   // the maps on their way up
    int32_t rect_w = 0, rect_h = 0, rect_stages = 0;   // rect_stages == 0: no maps
    int32_t last_groups = 0, last_launches = 0, last_waits = 0;   // what the last batched put did (chip_debug_frame_put_last)

    // slot k as a match or a read sees it: its rows and its frame (n == 0: an empty frame)
    struct Rows { const uint8_t *desc; const float2 *kp; const float4 *rec; int32_t n, w, h; };
    Rows rows(int32_t k) const
    {
        const size_t at = (size_t)k * (size_t)slot_kp;
        return Rows{store_desc + at * CHIP_ORB_DESC_BYTES, store_kp + at, store_rec + at, slots[(size_t)k].n, slots[(size_t)k].w, slots[(size_t)k].h};
    }
};

// defined in match.hip
int match_state(Ctx *c, MatchState **out);         // the match state, created and its fixed buffers reserved on first use
hipStream_t match_stream(Ctx *c);                  // the stream of the match and frame calls (the ctx's query stream)
// the frame rules: on a frame, or on its parts with what the frame arrives as (3-D image, disparity, left image) as `image`
int check_frame(const uint8_t *desc, const float *kp_xy, int32_t n, int32_t width, int32_t height, const void *image);
int check_frame(const chip_match_frame *f);

}  // namespace chip
