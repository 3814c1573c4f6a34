// examples/orb_frame_put.cc -- keyframes handed over as their rectified 8-bit stereo pair and NOTHING else: no keypoints, no descriptors
// (src/utils/PointFeatureMatching.cpp:16-22 runs detectAndCompute on a host core).  Every frame of the pair backlog of
// examples/frame_put_stereo.cc -- here the views of a place are the same textured scene two pixels apart, so that the detector finds
// the same corners -- is put TWICE: once straight from the pair (chip_frame_put_orb_stereo: detector, descriptor and block matcher
// on the device, one count back) and once composed on the host from single calls (chip_orb_detect_describe, then
// chip_frame_put_stereo with the records' (x, y)).  Every stored row must have the same bits; verify_pairs_stored then runs on both id
// sets and every summary, GMS choice, accept flag, pose and goodness must have the same bits as well.  The descriptors of query frame 0
// are also made by the plain C++ restatement of the definition below (include/cerebro_hip.h, "ORB descriptors on the device") from the
// pyramid levels and the records the device left; they must equal the device's.
// The definition is this project's own; the host restatement is a plain loop, NOT OpenCV's implementation.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   orb_frame_put [n_features] [P] [reps]   defaults 3000, 6, 0.  Prints one line per pair with its match and survivor counts; exit code 0
//                                       iff the two ways of putting agree in everything.  With reps > 0 the two ways and the host
//                                       restatement of the descriptor are timed on query frame 0, alternating (medians of reps runs).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../cerebro_amd/host/cerebro_host.h"

using namespace cerebro_hip;

static void blur_host(const uint8_t *I, int w, int h, uint8_t *B)
{
    static const int g[7] = {9, 17, 24, 28, 24, 17, 9};
    std::vector<int> Hs((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int s = 0;
            for (int i = -3; i <= 3; i++) s += g[i + 3] * I[(size_t)y * w + std::min(std::max(x + i, 0), w - 1)];
            Hs[(size_t)y * w + x] = s;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int s = 8192;
            for (int j = -3; j <= 3; j++) s += g[j + 3] * Hs[(size_t)std::min(std::max(y + j, 0), h - 1) * w + x];
            B[(size_t)y * w + x] = (uint8_t)(s >> 14);
        }
}

// the descriptors of n records from the blurred levels; the pattern's steered table comes from the library (chip_orb_pattern), the bin
// is computed here
static void describe_host(const std::vector<std::vector<uint8_t>> &blurred, const chip_orb_level *lv, const chip_orb_keypoint *kp, int n,
                          const int8_t *steered, uint8_t *desc)
{
    static const int quarter[9] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0};
    long long C[CHIP_ORB_BINS], S[CHIP_ORB_BINS];
    for (int k = 0; k <= 8; k++) { C[k] = quarter[k]; S[k] = quarter[8 - k]; }
    for (int k = 0; k + 8 < CHIP_ORB_BINS; k++) { C[k + 8] = -S[k]; S[k + 8] = C[k]; }
    std::memset(desc, 0, (size_t)n * CHIP_ORB_DESC_BYTES);
    for (int i = 0; i < n; i++) {
        int bin = 0;
        long long top = 0;
        for (int k = 0; k < CHIP_ORB_BINS; k++) {
            const long long v = kp[i].m10 * C[k] + kp[i].m01 * S[k];
            if (k == 0 || v > top) { top = v; bin = k; }
        }
        const int w = lv[kp[i].level].width, x = kp[i].x_level, y = kp[i].y_level;
        const uint8_t *B = blurred[kp[i].level].data();
        const int8_t *T = steered + (size_t)bin * 256 * 4;
        for (int p = 0; p < 256; p++)
            if (B[(size_t)(y + T[4 * p + 1]) * w + x + T[4 * p]] < B[(size_t)(y + T[4 * p + 3]) * w + x + T[4 * p + 2]])
                desc[(size_t)i * CHIP_ORB_DESC_BYTES + (p >> 3)] |= (uint8_t)(1u << (p & 7));
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
        std::fprintf(stderr, "usage: orb_frame_put [n_features in 1..%d] [P in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_PAIRS);
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

    // a rectified pair of a scene: blocks of CELL pixels of random brightness under pixel noise (corners at every scale), PAD + 2 columns
    // wider than the image; the right image starts dx columns into it, the left image is the same shifted by the tile's disparity
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
    std::vector<Frame> qs((size_t)P), cs((size_t)P);
    for (int k = 0; k < P; k++) {
        make_pair(qs[(size_t)k], 42 + (uint64_t)k, 100 + (uint64_t)k, 0);
        make_pair(cs[(size_t)k], 42 + (uint64_t)k, 100 + (uint64_t)k, 2);    // the same scene two pixels on
    }
    Frame empty;                                                             // a flat pair: nothing is kept
    empty.left.assign((size_t)W * H, 90);
    empty.right.assign((size_t)W * H, 90);

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    chip_ctx *ctx = cer.ctx();
    // keyframe arrival.  Straight from the pair: ids 1000 + k (query k), k (its second view), -1 (empty); composed on the host: the same + 5000
    const int64_t via_host = 5000;
    std::vector<chip_orb_keypoint> kp((size_t)n);
    std::vector<uint8_t> desc((size_t)n * CHIP_ORB_DESC_BYTES);
    std::vector<float> xy(2 * (size_t)n);
    int32_t kept = 0;
    const auto put_composed = [&](int64_t id, const Frame &fr) {
        int rc = chip_orb_detect_describe(ctx, fr.left.data(), W, H, &orb, kp.data(), n, &kept, nullptr, desc.data());
        if (rc != CHIP_OK) return rc;
        for (int32_t i = 0; i < kept; i++) { xy[2 * (size_t)i] = kp[(size_t)i].x; xy[2 * (size_t)i + 1] = kp[(size_t)i].y; }
        return chip_frame_put_stereo(ctx, id, desc.data(), xy.data(), kept, W, H, fr.left.data(), fr.right.data(), &bm, Q);
    };
    const auto put_both = [&](int64_t id, const Frame &fr) {
        int32_t m = -1;
        int rc = chip_frame_put_orb_stereo(ctx, id, W, H, fr.left.data(), fr.right.data(), &orb, &bm, Q, &m);
        if (rc == CHIP_OK) rc = put_composed(id + via_host, fr);
        if (rc == CHIP_OK && m != kept) { std::printf("frame %lld: the kept count DIFFERS (%d, %d)\n", (long long)id, m, kept); return (int)CHIP_ERR_HIP; }
        return rc;
    };
    int rc = chip_frame_store_reserve(ctx, 2 * (2 * P + 1), n);
    for (int k = 0; k < P && rc == CHIP_OK; k++) {
        rc = put_both(1000 + k, qs[(size_t)k]);
        if (rc == CHIP_OK) rc = put_both(k, cs[(size_t)k]);
    }
    if (rc == CHIP_OK) rc = put_both(-1, empty);
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }

    int differ = 0;
    // the stored rows themselves, frame by frame
    std::vector<uint8_t> d_s(desc.size()), d_h(desc.size());
    std::vector<float> k_s(xy.size()), k_h(xy.size()), r_s(4 * (size_t)n), r_h(r_s.size());
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

    // the descriptor restated on the host, on query frame 0 (the levels and records are the device's)
    int8_t steered[CHIP_ORB_BINS * 256 * 4];
    chip_orb_level lv[CHIP_ORB_MAX_LEVELS];
    if (chip_orb_pattern(nullptr, steered) != CHIP_OK || chip_orb_plan(W, H, &orb, lv) != CHIP_OK) return 1;
    if (chip_orb_detect_describe(ctx, qs[0].left.data(), W, H, &orb, kp.data(), n, &kept, nullptr, desc.data()) != CHIP_OK) return 1;
    std::vector<std::vector<uint8_t>> level((size_t)orb.n_levels), blurred((size_t)orb.n_levels);
    for (int l = 0; l < orb.n_levels; l++) {
        level[(size_t)l].resize((size_t)lv[l].width * lv[l].height);
        blurred[(size_t)l].resize(level[(size_t)l].size());
        if (chip_debug_orb_level(ctx, l, level[(size_t)l].data(), nullptr) != CHIP_OK) return 1;
    }
    std::vector<uint8_t> host_desc(desc.size());
    const auto describe_on_host = [&] {
        for (int l = 0; l < orb.n_levels; l++) blur_host(level[(size_t)l].data(), lv[l].width, lv[l].height, blurred[(size_t)l].data());
        describe_host(blurred, lv, kp.data(), kept, steered, host_desc.data());
    };
    describe_on_host();
    const bool same_desc = std::memcmp(host_desc.data(), desc.data(), (size_t)kept * CHIP_ORB_DESC_BYTES) == 0;
    std::printf("query frame 0: %d descriptors %s\n", kept, same_desc ? "== the host restatement" : "DIFFER from the host restatement");
    differ += !same_desc;

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
    std::vector<ProcessedLoopCandidate> from_pair, from_host;
    bool ok_s[CHIP_MATCH_MAX_PAIRS] = {}, ok_h[CHIP_MATCH_MAX_PAIRS] = {};
    chip_match_summary sm_s[CHIP_MATCH_MAX_PAIRS] = {}, sm_h[CHIP_MATCH_MAX_PAIRS] = {};
    chip_gms_choice ch_s[CHIP_MATCH_MAX_PAIRS] = {}, ch_h[CHIP_MATCH_MAX_PAIRS] = {};
    fresh(from_pair);
    fresh(from_host);
    if (!verify_pairs_stored(ctx, a_ids.data(), b_ids.data(), P, Kinv, from_pair.data(), ok_s, seeds.data(), sm_s, 0, ch_s) ||
        !verify_pairs_stored(ctx, a_host.data(), b_host.data(), P, Kinv, from_host.data(), ok_h, seeds.data(), sm_h, 0, ch_h)) {
        std::fprintf(stderr, "orb_frame_put: a library call failed\n");
        return 1;
    }
    int survivors = 0;
    for (int j = 0; j < P; j++) {
        const ProcessedLoopCandidate &p = from_pair[(size_t)j], &q = from_host[(size_t)j];
        bool same = ok_s[j] == ok_h[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size() && std::memcmp(&sm_s[j], &sm_h[j], sizeof(chip_match_summary)) == 0 &&
                    std::memcmp(&ch_s[j], &ch_h[j], sizeof(chip_gms_choice)) == 0;
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        std::printf("pair %2d (%lld, %lld): matches=%d gms=%d 3d3d=%d  %s  %s\n", j, (long long)a_ids[(size_t)j], (long long)b_ids[(size_t)j],
                    sm_s[j].n_matches_all, sm_s[j].n_matches_gms, sm_s[j].n_3d3d, ok_s[j] ? "three poses" : "rejected",
                    same ? "== the same frames composed on the host" : "DIFFERS from the same frames composed on the host");
        differ += !same;
        survivors += ok_s[j];
    }
    std::printf("%d of %d pairs survive with three poses\n", survivors, P);

    if (reps > 0) {
        const auto now = [] { return std::chrono::steady_clock::now(); };
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        const Frame &fr = qs[0];
        std::vector<double> t_pair, t_composed, t_host;
        for (int r = 0; r < reps + 3; r++) {                  // the variants alternate; three warm-up rounds
            int32_t m = 0;
            auto t0 = now();
            if (chip_frame_put_orb_stereo(ctx, 1000, W, H, fr.left.data(), fr.right.data(), &orb, &bm, Q, &m) != CHIP_OK) return 1;
            const double a = ms(t0, now());
            t0 = now();
            if (put_composed(1000 + via_host, fr) != CHIP_OK) return 1;
            const double b = ms(t0, now());
            t0 = now();
            describe_on_host();
            const double c = ms(t0, now());
            if (r >= 3) { t_pair.push_back(a); t_composed.push_back(b); t_host.push_back(c); }
        }
        std::printf("timing %dx%d n=%d reps=%d (medians, ms): chip_frame_put_orb_stereo %.3f, chip_orb_detect_describe + chip_frame_put_stereo %.3f; "
                    "host restatement of blur + descriptor (a plain loop, not OpenCV) %.3f\n", W, H, kept, reps, median(t_pair), median(t_composed),
                    median(t_host));
    }
    return differ == 0 ? 0 : 1;
}
