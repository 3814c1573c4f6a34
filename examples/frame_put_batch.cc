// examples/frame_put_batch.cc -- keyframes put in bulk, as a restarted node, an offline replay or a consumer thread with a backlog puts
// them.  The backlog of examples/frame_put_raw_stereo.cc (raw stereo pairs of scenes seen twice, and a black pair) goes into the store
// TWICE under two id sets: by ONE chip_frame_put_raw_orb_stereo_batch (every stage one launch per group of 16 frames, one host wait per
// group) and by the loop of chip_frame_put_raw_orb_stereo.  Every stored row must have the same bits; verify_pairs_stored then runs on
// both id sets and every summary, GMS choice, accept flag, pose and goodness must have the same bits as well.  Then the checkpoint
// path: every frame of the batch is read (chip_frame_read), dropped and put back from its records alone (chip_frame_put_records: no
// image, no kernel), and the same match must come out again.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   frame_put_batch [n_features] [P] [reps]   defaults 3000, 6, 0.  Prints one line per pair and, if everything agrees, a line with
//                                       "all equal"; exit code 0 iff it does.  With reps > 0 the batch call and the loop are timed on the
//                                       2 P + 1 frames, alternating (medians of reps runs), with the rectified form next to the raw one.
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
        std::fprintf(stderr, "usage: frame_put_batch [n_features in 1..%d] [P in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_PAIRS);
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

    // the arrival order: query k (id 1000 + k), its second view (id k), ..., the black pair (id -1) in the middle; the loop's ids + 5000
    const int64_t via_loop = 5000;
    const int F = 2 * P + 1;
    std::vector<int64_t> ids, loop_ids;
    std::vector<const uint8_t *> lefts, rights;
    const auto arrive = [&](int64_t id, const Frame &fr) {
        ids.push_back(id);
        loop_ids.push_back(id + via_loop);
        lefts.push_back(fr.left.data());
        rights.push_back(fr.right.data());
    };
    for (int k = 0; k < P; k++) {
        if (k == P / 2) arrive(-1, empty);
        arrive(1000 + k, qs[(size_t)k]);
        arrive(k, cs[(size_t)k]);
    }
    int32_t group = 0, n_groups = 0;
    rc = chip_frame_put_plan(W, H, &orb, 1, F, &group, &n_groups);
    if (rc == CHIP_OK) rc = chip_frame_store_reserve(ctx, 2 * F, n);
    std::vector<int32_t> kept((size_t)F, -2), kept_loop((size_t)F, -2);
    if (rc == CHIP_OK) rc = chip_frame_put_raw_orb_stereo_batch(ctx, ids.data(), F, W, H, lefts.data(), rights.data(), &orb, &bm, Q, kept.data());
    int32_t did_groups = 0, launches = 0, waits = 0;
    if (rc == CHIP_OK) rc = chip_debug_frame_put_last(ctx, &did_groups, &launches, &waits);
    for (int f = 0; f < F && rc == CHIP_OK; f++)
        rc = chip_frame_put_raw_orb_stereo(ctx, loop_ids[(size_t)f], W, H, lefts[(size_t)f], rights[(size_t)f], &orb, &bm, Q, &kept_loop[(size_t)f]);
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }
    int differ = 0;
    std::printf("%d frames in one call: %d groups of up to %d, %d launches, %d host waits (the loop: about %d launches, %d waits)\n", F, did_groups,
                group, launches, waits, 16 * F, 2 * F);
    if (did_groups != n_groups || waits != did_groups || launches > 16 * did_groups) { std::printf("the call DIFFERS from its plan\n"); differ++; }

    // the stored rows themselves, frame by frame
    struct Rows { int32_t n = 0, w = 0, h = 0; std::vector<uint8_t> d; std::vector<float> k, r; };
    const auto read = [&](int64_t id, Rows &o) {
        o.d.assign((size_t)n * CHIP_ORB_DESC_BYTES, 0); o.k.assign(2 * (size_t)n, 0.f); o.r.assign(4 * (size_t)n, 0.f);
        return chip_frame_read(ctx, id, &o.n, &o.w, &o.h, o.d.data(), o.k.data(), o.r.data()) == CHIP_OK;
    };
    const auto same_rows = [](const Rows &a, const Rows &b) {
        return a.n == b.n && a.w == b.w && a.h == b.h && std::memcmp(a.d.data(), b.d.data(), 32 * (size_t)a.n) == 0 &&
               std::memcmp(a.k.data(), b.k.data(), 8 * (size_t)a.n) == 0 && std::memcmp(a.r.data(), b.r.data(), 16 * (size_t)a.n) == 0;
    };
    std::vector<Rows> saved((size_t)F);
    size_t with_depth = 0, keypoints = 0;
    for (int f = 0; f < F; f++) {
        Rows loop;
        if (!read(ids[(size_t)f], saved[(size_t)f]) || !read(loop_ids[(size_t)f], loop)) return 1;
        if (!same_rows(saved[(size_t)f], loop) || kept[(size_t)f] != kept_loop[(size_t)f] || kept[(size_t)f] != loop.n) {
            std::printf("frame %lld: the stored rows DIFFER\n", (long long)ids[(size_t)f]);
            differ++;
        }
        keypoints += (size_t)loop.n;
        for (int32_t i = 0; i < loop.n; i++) with_depth += loop.r[4 * (size_t)i + 2] > 0.1f;
    }
    std::printf("%zu keypoints in %d frames, %zu of them with a depth\n", keypoints, F, with_depth);
    if (with_depth == 0) { std::printf("no keypoint has a depth: the comparison DIFFERS from a meaningful one\n"); differ++; }

    // the backlog: pair k = (query k, its second view), but the last two: an unrelated pair and an empty candidate
    std::vector<int64_t> a_ids, b_ids, a_loop, b_loop;
    std::vector<uint64_t> seeds;
    for (int k = 0; k < P; k++) {
        a_ids.push_back(1000 + k);
        b_ids.push_back(k == P - 1 ? -1 : k == P - 2 ? 0 : k);
        a_loop.push_back(a_ids.back() + via_loop);
        b_loop.push_back(b_ids.back() + via_loop);
        seeds.push_back(7 + 10 * (uint64_t)k);
    }
    struct Verdict {
        std::vector<ProcessedLoopCandidate> pc;
        bool ok[CHIP_MATCH_MAX_PAIRS] = {};
        chip_match_summary sm[CHIP_MATCH_MAX_PAIRS] = {};
        chip_gms_choice ch[CHIP_MATCH_MAX_PAIRS] = {};
    };
    const auto verify = [&](const std::vector<int64_t> &a, const std::vector<int64_t> &b, Verdict &v) {
        v.pc.assign((size_t)P, ProcessedLoopCandidate());
        for (int j = 0; j < P; j++) { v.pc[(size_t)j].t_node_1 = Time{100 + (uint32_t)j, 0}; v.pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
        return verify_pairs_stored(ctx, a.data(), b.data(), P, Kinv, v.pc.data(), v.ok, seeds.data(), v.sm, 0, v.ch);
    };
    const auto same_verdict = [&](const Verdict &x, const Verdict &y, int j) {
        const ProcessedLoopCandidate &p = x.pc[(size_t)j], &q = y.pc[(size_t)j];
        bool same = x.ok[j] == y.ok[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size() && std::memcmp(&x.sm[j], &y.sm[j], sizeof(chip_match_summary)) == 0 &&
                    std::memcmp(&x.ch[j], &y.ch[j], sizeof(chip_gms_choice)) == 0;
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        return same;
    };
    Verdict from_batch, from_loop, from_records;
    if (!verify(a_ids, b_ids, from_batch) || !verify(a_loop, b_loop, from_loop)) { std::fprintf(stderr, "frame_put_batch: a library call failed\n"); return 1; }

    // the checkpoint path: records out, frames dropped, records back in (in the other order: other slots), the same match again
    for (int f = 0; f < F; f++)
        if (chip_frame_drop(ctx, ids[(size_t)f]) != CHIP_OK) return 1;
    for (int f = F - 1; f >= 0; f--) {
        const Rows &s = saved[(size_t)f];
        rc = chip_frame_put_records(ctx, ids[(size_t)f], s.d.data(), s.k.data(), s.r.data(), s.n, s.w, s.h);
        if (rc != CHIP_OK) { std::fprintf(stderr, "chip_frame_put_records -> %s\n", chip_strerror(rc)); return 1; }
    }
    for (int f = 0; f < F; f++) {
        Rows back;
        if (!read(ids[(size_t)f], back)) return 1;
        if (!same_rows(back, saved[(size_t)f])) { std::printf("frame %lld: the restored rows DIFFER\n", (long long)ids[(size_t)f]); differ++; }
    }
    if (!verify(a_ids, b_ids, from_records)) { std::fprintf(stderr, "frame_put_batch: a library call failed\n"); return 1; }
    int survivors = 0;
    for (int j = 0; j < P; j++) {
        const bool s1 = same_verdict(from_batch, from_loop, j), s2 = same_verdict(from_batch, from_records, j);
        std::printf("pair %2d (%lld, %lld): matches=%d gms=%d 3d3d=%d  %s  %s, %s\n", j, (long long)a_ids[(size_t)j], (long long)b_ids[(size_t)j],
                    from_batch.sm[j].n_matches_all, from_batch.sm[j].n_matches_gms, from_batch.sm[j].n_3d3d, from_batch.ok[j] ? "three poses" : "rejected",
                    s1 ? "== the loop of single puts" : "DIFFERS from the loop of single puts",
                    s2 ? "== the frames restored from their records" : "DIFFERS from the frames restored from their records");
        differ += !s1 + !s2;
        survivors += from_batch.ok[j];
    }
    std::printf("%d of %d pairs survive with three poses\n", survivors, P);
    if (differ == 0) std::printf("all equal: %d frames, %d pairs, one batch call == %d single calls == the records put back\n", F, P, F);

    if (reps > 0) {
        const auto now = [] { return std::chrono::steady_clock::now(); };
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        std::vector<double> t_batch, t_loop, t_rbatch, t_rloop, t_records;
        std::vector<int32_t> m((size_t)F);
        for (int r = 0; r < reps + 3; r++) {                  // the variants alternate; three warm-up rounds
            auto t0 = now();
            if (chip_frame_put_raw_orb_stereo_batch(ctx, ids.data(), F, W, H, lefts.data(), rights.data(), &orb, &bm, Q, m.data()) != CHIP_OK) return 1;
            const double a = ms(t0, now());
            t0 = now();
            for (int f = 0; f < F; f++)
                if (chip_frame_put_raw_orb_stereo(ctx, loop_ids[(size_t)f], W, H, lefts[(size_t)f], rights[(size_t)f], &orb, &bm, Q, &m[(size_t)f]) != CHIP_OK) return 1;
            const double b = ms(t0, now());
            t0 = now();                                       // (the raw pairs stand in for rectified ones: the time does not depend on the content much)
            if (chip_frame_put_orb_stereo_batch(ctx, ids.data(), F, W, H, lefts.data(), rights.data(), &orb, &bm, Q, m.data()) != CHIP_OK) return 1;
            const double c = ms(t0, now());
            t0 = now();
            for (int f = 0; f < F; f++)
                if (chip_frame_put_orb_stereo(ctx, loop_ids[(size_t)f], W, H, lefts[(size_t)f], rights[(size_t)f], &orb, &bm, Q, &m[(size_t)f]) != CHIP_OK) return 1;
            const double d = ms(t0, now());
            t0 = now();
            for (int f = 0; f < F; f++) {
                const Rows &s = saved[(size_t)f];
                if (chip_frame_put_records(ctx, ids[(size_t)f], s.d.data(), s.k.data(), s.r.data(), s.n, s.w, s.h) != CHIP_OK) return 1;
            }
            const double e = ms(t0, now());
            if (r >= 3) { t_batch.push_back(a); t_loop.push_back(b); t_rbatch.push_back(c); t_rloop.push_back(d); t_records.push_back(e); }
        }
        std::printf("timing %dx%d n=%d F=%d reps=%d (medians, ms for all F frames): raw pairs in one batch call %.3f, in the loop of single calls "
                    "%.3f; rectified pairs in one batch call %.3f, in the loop %.3f; from their records %.3f\n", W, H, n, F, reps, median(t_batch),
                    median(t_loop), median(t_rbatch), median(t_rloop), median(t_records));
    }
    return differ == 0 ? 0 : 1;
}
