// examples/frame_put_raw_stereo.cc -- keyframes handed over as what the camera driver delivers: the RAW 8-bit stereo pair.  The
// reference makes the rectified pair on a host core (StereoGeometry::do_stereo_rectification_of_raw_images,
// src/utils/CameraGeometry.cpp:387-402: four cv::remap per pair); here the maps go to the device once (chip_rectify_set_maps) and
// every frame of the pair backlog of examples/orb_frame_put.cc -- each scene warped into a "raw" pair by a synthetic distortion -- is
// put TWICE: once straight from the raw pair (chip_frame_put_raw_orb_stereo: rectification, detector, descriptor and block matcher on
// the device, one count back) and once through the plain C++ restatement of the definition below (include/cerebro_hip.h, "a frame
// from its raw stereo pair") followed by chip_frame_put_orb_stereo.  Every stored row must have the same bits; verify_pairs_stored
// then runs on both id sets and every summary, GMS choice, accept flag, pose and goodness must have the same bits as well.
// The maps are made in plain C++: a radial-tangential pinhole model for stage 1 (undistortion), the homography of a small rotation
// for stage 2 (rectification); an integrator takes them from the calibration instead.
// The definition is this project's own; the host restatement is a plain loop, NOT OpenCV's implementation.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   frame_put_raw_stereo [n_features] [P] [reps]   defaults 3000, 6, 0.  Prints one line per pair with its match and survivor counts; exit
//                                       code 0 iff the two ways of putting agree in everything.  With reps > 0 the two ways, the host
//                                       restatement alone, chip_rectify_pair and chip_frame_put_orb_stereo on the rectified pair are
//                                       timed on query frame 0, alternating (medians of reps runs).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../cerebro_amd/host/cerebro_host.h"

using namespace cerebro_hip;

struct Maps {
    std::vector<float> x1, y1, x2, y2;   // stage 1: raw -> undistorted; stage 2: undistorted -> rectified
};

// Q of the header: 1/32 pixel, NaN -> -64, ties to even (rintf in the default rounding mode)
static int32_t quantize(float m)
{
    if (m != m) return -64;
    return (int32_t)rintf(32.0f * std::min(std::max(m, -2.0f), 32768.0f));
}

// S of the header on every pixel: one stage
static void remap_host(const uint8_t *I, int w, int h, const float *mx, const float *my, uint8_t *out)
{
    const auto at = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h ? (int)I[(size_t)y * w + x] : 0; };
    for (size_t i = 0; i < (size_t)w * h; i++) {
        const int32_t qx = quantize(mx[i]), qy = quantize(my[i]);
        const int x0 = qx >> 5, a = qx & 31, y0 = qy >> 5, b = qy & 31;
        out[i] = (uint8_t)((at(x0, y0) * (32 - a) * (32 - b) + at(x0 + 1, y0) * a * (32 - b) + at(x0, y0 + 1) * (32 - a) * b +
                            at(x0 + 1, y0 + 1) * a * b + 512) >> 10);
    }
}

// two stages: the undistorted image is a uint8 image of its own, as in the reference
static void rectify_host(const uint8_t *raw, int w, int h, const Maps &m, std::vector<uint8_t> &u, uint8_t *out)
{
    u.resize((size_t)w * h);
    remap_host(raw, w, h, m.x1.data(), m.y1.data(), u.data());
    remap_host(u.data(), w, h, m.x2.data(), m.y2.data(), out);
}

// stage 1: where in the distorted image the ideal pixel (x, y) of the same pinhole camera comes from
static void radtan_maps(int w, int h, double f, double cx, double cy, double k1, double k2, double p1, double p2, std::vector<float> &mx,
                        std::vector<float> &my)
{
    mx.resize((size_t)w * h);
    my.resize((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const double xn = (x - cx) / f, yn = (y - cy) / f, r2 = xn * xn + yn * yn, rad = 1 + k1 * r2 + k2 * r2 * r2;
            mx[(size_t)y * w + x] = (float)(f * (xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)) + cx);
            my[(size_t)y * w + x] = (float)(f * (yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn) + cy);
        }
}

// stage 2: the homography K R K^-1 of a small rotation (first order in the angles)
static void rotation_maps(int w, int h, double f, double cx, double cy, double rx, double ry, double rz, std::vector<float> &mx,
                          std::vector<float> &my)
{
    mx.resize((size_t)w * h);
    my.resize((size_t)w * h);
    const double R[9] = {1, -rz, ry, rz, 1, -rx, -ry, rx, 1};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const double xn = (x - cx) / f, yn = (y - cy) / f;
            const double X = R[0] * xn + R[1] * yn + R[2], Y = R[3] * xn + R[4] * yn + R[5], Z = R[6] * xn + R[7] * yn + R[8];
            mx[(size_t)y * w + x] = (float)(f * X / Z + cx);
            my[(size_t)y * w + x] = (float)(f * Y / Z + cy);
        }
}

// a first-order inverse of a map near the identity: 2 (x, y) - map
static void mirror_maps(int w, int h, const std::vector<float> &mx, const std::vector<float> &my, std::vector<float> &ix, std::vector<float> &iy)
{
    ix.resize(mx.size());
    iy.resize(my.size());
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            ix[(size_t)y * w + x] = 2.0f * (float)x - mx[(size_t)y * w + x];
            iy[(size_t)y * w + x] = 2.0f * (float)y - my[(size_t)y * w + x];
        }
}

struct Frame {
    std::vector<uint8_t> left, right;
};

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 3000;
    const int P = argc > 2 ? std::atoi(argv[2]) : 6;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
    if (n < 1 || n > CHIP_MATCH_MAX_KEYPOINTS || P < 3 || P > CHIP_MATCH_MAX_PAIRS || reps < 0) {
        std::fprintf(stderr, "usage: frame_put_raw_stereo [n_features in 1..%d] [P in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_PAIRS);
        return 2;
    }
    const int W = 752, H = 480, TILE = 94, PAD = 64, CELL = 6;
    const double f = 458.654, cx = 367.215803962, cy = 248.375340610, baseline = 0.110073808127;
    const double Kinv[9] = {1.0 / f, 0.0, -cx / f, 0.0, 1.0 / f, -cy / f, 0.0, 0.0, 1.0};
    const double Q[16] = {1.0, 0.0, 0.0, -cx, 0.0, 1.0, 0.0, -cy, 0.0, 0.0, 0.0, f, 0.0, 0.0, 1.0 / baseline, 0.0};   // cv::stereoRectify
    chip_stereo_bm_params bm;
    chip_stereo_bm_params_default(&bm);
    chip_orb_params orb;
    chip_orb_params_default(&orb);
    orb.n_features = n;

    // the calibration: each eye its own distortion and its own small rotation
    Maps ml, mr;
    radtan_maps(W, H, f, cx, cy, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, ml.x1, ml.y1);
    radtan_maps(W, H, 457.587, 379.999, 255.238, -0.28368365, 0.07451284, -0.00010473, -3.55590700e-05, mr.x1, mr.y1);
    rotation_maps(W, H, f, cx, cy, 0.004, -0.007, 0.009, ml.x2, ml.y2);
    rotation_maps(W, H, f, cx, cy, -0.005, 0.006, -0.004, mr.x2, mr.y2);

    // a rectified pair of a scene (examples/orb_frame_put.cc): blocks of CELL pixels of random brightness under pixel noise, the left
    // image the right one shifted by its tile's disparity ...
    const auto make_pair = [&](Frame &fr, uint64_t scene_seed, uint64_t tiles_seed, int dx) {
        const int BW = W + PAD + 2;
        std::mt19937_64 rng(scene_seed);
        std::vector<uint8_t> cells((size_t)((BW + CELL - 1) / CELL) * ((H + CELL - 1) / CELL)), base((size_t)BW * H);
        for (auto &v : cells) v = (uint8_t)(40 + rng() % 176);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < BW; x++)
                base[(size_t)y * BW + x] = (uint8_t)((int)cells[(size_t)(y / CELL) * ((BW + CELL - 1) / CELL) + x / CELL] + (int)(rng() % 31) - 15);
        std::mt19937_64 tr(tiles_seed);
        const int tw = (W + TILE - 1) / TILE, th = (H + TILE - 1) / TILE;
        std::vector<int> shift((size_t)tw * th);
        for (auto &s : shift) s = 8 + (int)(tr() % 33);
        fr.left.resize((size_t)W * H);
        fr.right.resize((size_t)W * H);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                fr.right[(size_t)y * W + x] = base[(size_t)y * BW + x + PAD + dx];
                fr.left[(size_t)y * W + x] = base[(size_t)y * BW + x + PAD + dx - shift[(size_t)(y / TILE) * tw + x / TILE]];
            }
    };
    // ... warped into the pair the cameras would have seen: through the mirrored maps, rectification first.  What comes back through
    // the calibration is the scene up to the interpolation; the test below is about the two ways of putting, not about the scene
    Maps wl, wr;
    mirror_maps(W, H, ml.x2, ml.y2, wl.x1, wl.y1);
    mirror_maps(W, H, ml.x1, ml.y1, wl.x2, wl.y2);
    mirror_maps(W, H, mr.x2, mr.y2, wr.x1, wr.y1);
    mirror_maps(W, H, mr.x1, mr.y1, wr.x2, wr.y2);
    std::vector<uint8_t> u;
    const auto make_raw = [&](Frame &raw, uint64_t scene_seed, uint64_t tiles_seed, int dx) {
        Frame fr;
        make_pair(fr, scene_seed, tiles_seed, dx);
        raw.left.resize(fr.left.size());
        raw.right.resize(fr.right.size());
        rectify_host(fr.left.data(), W, H, wl, u, raw.left.data());
        rectify_host(fr.right.data(), W, H, wr, u, raw.right.data());
    };
    std::vector<Frame> qs((size_t)P), cs((size_t)P);
    for (int k = 0; k < P; k++) {
        make_raw(qs[(size_t)k], 42 + (uint64_t)k, 100 + (uint64_t)k, 0);
        make_raw(cs[(size_t)k], 42 + (uint64_t)k, 100 + (uint64_t)k, 2);     // the same scene two pixels on
    }
    Frame empty;                                                             // a black pair: nothing is kept
    empty.left.assign((size_t)W * H, 0);
    empty.right.assign((size_t)W * H, 0);

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    chip_ctx *ctx = cer.ctx();
    int rc = chip_rectify_set_maps(ctx, W, H, ml.x1.data(), ml.y1.data(), ml.x2.data(), ml.y2.data(), mr.x1.data(), mr.y1.data(), mr.x2.data(),
                                   mr.y2.data());
    if (rc != CHIP_OK) { std::fprintf(stderr, "chip_rectify_set_maps -> %s\n", chip_strerror(rc)); return 1; }
    // keyframe arrival.  Straight from the raw pair: ids 1000 + k (query k), k (its second view), -1 (empty); rectified on the host: the same + 5000
    const int64_t via_host = 5000;
    Frame rect;
    rect.left.resize((size_t)W * H);
    rect.right.resize((size_t)W * H);
    const auto rectify_on_host = [&](const Frame &raw) {
        rectify_host(raw.left.data(), W, H, ml, u, rect.left.data());
        rectify_host(raw.right.data(), W, H, mr, u, rect.right.data());
    };
    const auto put_via_host = [&](int64_t id, const Frame &raw, int32_t *m) {
        rectify_on_host(raw);
        return chip_frame_put_orb_stereo(ctx, id, W, H, rect.left.data(), rect.right.data(), &orb, &bm, Q, m);
    };
    const auto put_both = [&](int64_t id, const Frame &raw) {
        int32_t m = -1, kept = -2;
        int r = chip_frame_put_raw_orb_stereo(ctx, id, W, H, raw.left.data(), raw.right.data(), &orb, &bm, Q, &m);
        if (r == CHIP_OK) r = put_via_host(id + via_host, raw, &kept);
        if (r == CHIP_OK && m != kept) { std::printf("frame %lld: the kept count DIFFERS (%d, %d)\n", (long long)id, m, kept); return (int)CHIP_ERR_HIP; }
        return r;
    };
    rc = chip_frame_store_reserve(ctx, 2 * (2 * P + 1), n);
    for (int k = 0; k < P && rc == CHIP_OK; k++) {
        rc = put_both(1000 + k, qs[(size_t)k]);
        if (rc == CHIP_OK) rc = put_both(k, cs[(size_t)k]);
    }
    if (rc == CHIP_OK) rc = put_both(-1, empty);
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }

    int differ = 0;
    // the rectified pair itself: chip_rectify_pair against the restatement, on query frame 0
    Frame dev;
    dev.left.resize((size_t)W * H);
    dev.right.resize((size_t)W * H);
    if (chip_rectify_pair(ctx, qs[0].left.data(), qs[0].right.data(), W, H, dev.left.data(), dev.right.data()) != CHIP_OK) return 1;
    rectify_on_host(qs[0]);
    const bool same_pair = dev.left == rect.left && dev.right == rect.right;
    std::printf("query frame 0: the rectified pair of chip_rectify_pair %s\n", same_pair ? "== the host restatement" : "DIFFERS from the host restatement");
    differ += !same_pair;

    // the stored rows themselves, frame by frame
    std::vector<uint8_t> d_s((size_t)n * CHIP_ORB_DESC_BYTES), d_h(d_s.size());
    std::vector<float> k_s(2 * (size_t)n), k_h(k_s.size()), r_s(4 * (size_t)n), r_h(r_s.size());
    size_t with_depth = 0, keypoints = 0;
    for (int k = 0; k <= 2 * P; k++) {
        const int64_t id = k == 2 * P ? -1 : k < P ? 1000 + k : k - P;
        int32_t ns = 0, nh = 0;
        if (chip_frame_read(ctx, id, &ns, nullptr, nullptr, d_s.data(), k_s.data(), r_s.data()) != CHIP_OK ||
            chip_frame_read(ctx, id + via_host, &nh, nullptr, nullptr, d_h.data(), k_h.data(), r_h.data()) != CHIP_OK) return 1;
        if (ns != nh || std::memcmp(d_s.data(), d_h.data(), 32 * (size_t)ns) != 0 || std::memcmp(k_s.data(), k_h.data(), 8 * (size_t)ns) != 0 ||
            std::memcmp(r_s.data(), r_h.data(), 16 * (size_t)ns) != 0) {
            std::printf("frame %lld: the stored rows DIFFER\n", (long long)id);
            differ++;
        }
        keypoints += (size_t)ns;
        for (int32_t i = 0; i < ns; i++) with_depth += r_s[4 * (size_t)i + 2] > 0.1f;
    }
    std::printf("%zu keypoints in %d frames, %zu of them with a depth\n", keypoints, 2 * P + 1, with_depth);
    if (with_depth == 0) { std::printf("no keypoint has a depth: the comparison DIFFERS from a meaningful one\n"); differ++; }

    // the backlog: pair k = (query k, its second view), but the last two: an unrelated pair and an empty candidate
    std::vector<int64_t> a_ids, b_ids, a_host, b_host;
    std::vector<uint64_t> seeds;
    for (int k = 0; k < P; k++) {
        a_ids.push_back(1000 + k);
        b_ids.push_back(k == P - 1 ? -1 : k == P - 2 ? 0 : k);
        a_host.push_back(a_ids.back() + via_host);
        b_host.push_back(b_ids.back() + via_host);
        seeds.push_back(7 + 10 * (uint64_t)k);
    }
    const auto fresh = [&](std::vector<ProcessedLoopCandidate> &pc) {
        pc.assign((size_t)P, ProcessedLoopCandidate());
        for (int j = 0; j < P; j++) { pc[(size_t)j].t_node_1 = Time{100 + (uint32_t)j, 0}; pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
    };
    std::vector<ProcessedLoopCandidate> from_raw, from_host;
    bool ok_s[CHIP_MATCH_MAX_PAIRS] = {}, ok_h[CHIP_MATCH_MAX_PAIRS] = {};
    chip_match_summary sm_s[CHIP_MATCH_MAX_PAIRS] = {}, sm_h[CHIP_MATCH_MAX_PAIRS] = {};
    chip_gms_choice ch_s[CHIP_MATCH_MAX_PAIRS] = {}, ch_h[CHIP_MATCH_MAX_PAIRS] = {};
    fresh(from_raw);
    fresh(from_host);
    if (!verify_pairs_stored(ctx, a_ids.data(), b_ids.data(), P, Kinv, from_raw.data(), ok_s, seeds.data(), sm_s, 0, ch_s) ||
        !verify_pairs_stored(ctx, a_host.data(), b_host.data(), P, Kinv, from_host.data(), ok_h, seeds.data(), sm_h, 0, ch_h)) {
        std::fprintf(stderr, "frame_put_raw_stereo: a library call failed\n");
        return 1;
    }
    int survivors = 0;
    for (int j = 0; j < P; j++) {
        const ProcessedLoopCandidate &p = from_raw[(size_t)j], &q = from_host[(size_t)j];
        bool same = ok_s[j] == ok_h[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size() && std::memcmp(&sm_s[j], &sm_h[j], sizeof(chip_match_summary)) == 0 &&
                    std::memcmp(&ch_s[j], &ch_h[j], sizeof(chip_gms_choice)) == 0;
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        std::printf("pair %2d (%lld, %lld): matches=%d gms=%d 3d3d=%d  %s  %s\n", j, (long long)a_ids[(size_t)j], (long long)b_ids[(size_t)j],
                    sm_s[j].n_matches_all, sm_s[j].n_matches_gms, sm_s[j].n_3d3d, ok_s[j] ? "three poses" : "rejected",
                    same ? "== the same frames rectified on the host" : "DIFFERS from the same frames rectified on the host");
        differ += !same;
        survivors += ok_s[j];
    }
    std::printf("%d of %d pairs survive with three poses\n", survivors, P);

    if (reps > 0) {
        const auto now = [] { return std::chrono::steady_clock::now(); };
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        const Frame &raw = qs[0];
        Frame pre;                                            // the rectified pair of query frame 0, made before the clock starts
        rectify_on_host(raw);
        pre = rect;
        std::vector<double> t_raw, t_via_host, t_host, t_pair, t_rectified;
        for (int r = 0; r < reps + 3; r++) {                  // the variants alternate; three warm-up rounds
            int32_t m = 0;
            auto t0 = now();
            if (chip_frame_put_raw_orb_stereo(ctx, 1000, W, H, raw.left.data(), raw.right.data(), &orb, &bm, Q, &m) != CHIP_OK) return 1;
            const double a = ms(t0, now());
            t0 = now();
            if (put_via_host(1000 + via_host, raw, &m) != CHIP_OK) return 1;
            const double b = ms(t0, now());
            t0 = now();
            rectify_on_host(raw);
            const double c = ms(t0, now());
            t0 = now();
            if (chip_rectify_pair(ctx, raw.left.data(), raw.right.data(), W, H, dev.left.data(), dev.right.data()) != CHIP_OK) return 1;
            const double d = ms(t0, now());
            t0 = now();
            if (chip_frame_put_orb_stereo(ctx, 1000 + via_host, W, H, pre.left.data(), pre.right.data(), &orb, &bm, Q, &m) != CHIP_OK) return 1;
            const double e = ms(t0, now());
            if (r >= 3) { t_raw.push_back(a); t_via_host.push_back(b); t_host.push_back(c); t_pair.push_back(d); t_rectified.push_back(e); }
        }
        std::printf("timing %dx%d n=%d reps=%d (medians, ms): chip_frame_put_raw_orb_stereo %.3f, chip_frame_put_orb_stereo on the rectified pair "
                    "%.3f, host restatement + chip_frame_put_orb_stereo %.3f; host restatement of the rectification alone (a plain loop, not "
                    "OpenCV's implementation) %.3f; chip_rectify_pair %.3f\n", W, H, n, reps, median(t_raw), median(t_rectified), median(t_via_host),
                    median(t_host), median(t_pair));
    }
    return differ == 0 ? 0 : 1;
}
