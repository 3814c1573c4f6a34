// The reference's GMS matcher with its scale / rotation variants as a compiled checker: a C ABI around
// src/utils/GMSMatcher/gms_matcher.{h,cpp} of the reference tree, which `make ref_modes` compiles BY PATH next to this file against the
// stand-in oracle/ref_gms/opencv2/opencv.hpp (no reference source is in this repository).  It is oracle/ref_gms/gms_ref.cc plus the two
// booleans of GetInlierMask(mask, WithScale, WithRotation) (src/utils/PointFeatureMatching.cpp:52-53), and it reports the size of the
// mask vector: when no hypothesis has an inlier the reference leaves the caller's vector untouched (gms_matcher.cpp:26-30), i.e. empty.
// tests/gms_modes_ref_lib.py loads it; tests/test_gms_modes_mirror.py compares tests/np_mirror_gms_modes.py with it.
#include "gms_matcher.h"

#include <cstdint>

namespace ref_gms {
int out_of_bounds = 0;
}

enum { kRefOk = 0, kRefBadArgument = -1 };
// *flag: 0 = the reference ran inside its tables; 1 = it indexed a matrix out of bounds (stopped there, the mask is all zero);
//        2 = not run: a keypoint is not finite or so large that the reference's float -> int conversion would be undefined
enum { kFlagNone = 0, kFlagOutOfBounds = 1, kFlagNotRun = 2 };

extern "C" int gms_ref_modes_run(const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1, const float *kp2_xy, int32_t n2, int32_t w2, int32_t h2,
                                 const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches, int32_t with_scale, int32_t with_rotation,
                                 uint8_t *inlier, int32_t *n_inliers, int32_t *mask_size, int32_t *flag)
{
    if (n1 < 0 || n2 < 0 || n_matches < 0 || w1 <= 0 || h1 <= 0 || w2 <= 0 || h2 <= 0 || !n_inliers || !mask_size || !flag) return kRefBadArgument;
    if ((n1 > 0 && !kp1_xy) || (n2 > 0 && !kp2_xy) || (n_matches > 0 && (!query_idx || !train_idx || !inlier))) return kRefBadArgument;
    for (int32_t i = 0; i < n_matches; i++)   // the reference indexes its point vectors with these
        if (query_idx[i] < 0 || query_idx[i] >= n1 || train_idx[i] < 0 || train_idx[i] >= n2) return kRefBadArgument;
    *n_inliers = 0;
    *mask_size = 0;
    *flag = kFlagNone;
    for (int32_t i = 0; i < n_matches; i++) inlier[i] = 0;
    const float lim = 1.0e6f;
    for (int32_t i = 0; i < 2 * n1; i++)
        if (!(kp1_xy[i] >= -lim && kp1_xy[i] <= lim)) { *flag = kFlagNotRun; return kRefOk; }
    for (int32_t i = 0; i < 2 * n2; i++)
        if (!(kp2_xy[i] >= -lim && kp2_xy[i] <= lim)) { *flag = kFlagNotRun; return kRefOk; }

    std::vector<KeyPoint> kp1((size_t)n1), kp2((size_t)n2);
    for (int32_t i = 0; i < n1; i++) { kp1[i].pt.x = kp1_xy[2 * i]; kp1[i].pt.y = kp1_xy[2 * i + 1]; }
    for (int32_t i = 0; i < n2; i++) { kp2[i].pt.x = kp2_xy[2 * i]; kp2[i].pt.y = kp2_xy[2 * i + 1]; }
    std::vector<DMatch> matches_all((size_t)n_matches);
    for (int32_t i = 0; i < n_matches; i++) { matches_all[i].queryIdx = query_idx[i]; matches_all[i].trainIdx = train_idx[i]; }

    ref_gms::out_of_bounds = 0;
    try {
        std::vector<bool> vbInliers;
        gms_matcher gms(kp1, Size(w1, h1), kp2, Size(w2, h2), matches_all);
        const int num_inliers = gms.GetInlierMask(vbInliers, with_scale != 0, with_rotation != 0);
        *mask_size = (int32_t)vbInliers.size();
        if (*mask_size != n_matches && *mask_size != 0) return kRefBadArgument;   // the whole mask, or the untouched (empty) vector
        for (int32_t i = 0; i < *mask_size; i++) inlier[i] = vbInliers[i] ? 1 : 0;
        *n_inliers = num_inliers;
    } catch (const ref_gms::OutOfBounds &) {
        *flag = kFlagOutOfBounds;
    }
    return kRefOk;
}
