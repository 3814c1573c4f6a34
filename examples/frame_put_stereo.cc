// examples/frame_put_stereo.cc -- keyframes handed over as their rectified 8-bit stereo pair instead of the disparity map that
// cv::StereoBM::create(64, 21) makes of it on a host core (src/utils/CameraGeometry.cpp:81,416).  Every frame of a
// small pair backlog carries a synthetic pair -- a random texture, smoothed once, the left image the right one shifted by a
// piecewise-constant integer disparity -- and is put TWICE: once from the pair (chip_frame_put_stereo: the block matcher runs on the
// device, at the keypoints) and once through chip_frame_put_disparity with the int16 map that the plain C++ restatement of the
// definition below (include/cerebro_hip.h, "a frame from its rectified stereo pair") makes on the host.  verify_pairs_stored then runs on
// both id sets; every record, summary, GMS choice, accept flag, pose and goodness must have the same bits.
// The definition is this project's own, modelled on StereoBM; the host restatement is a plain loop, NOT OpenCV's implementation.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   frame_put_stereo [n_points] [P] [reps]   defaults 3000, 6, 0.  P places, each with a query frame of its own and a second view of it;
//                                        the last two pairs are an unrelated pair and a pair with an empty candidate.  Prints one line
//                                        per pair; exit code 0 iff the two ways of putting agree in everything.  With reps > 0 the three
//                                        puts (pair, int16 map, 3-D image), the host restatement and chip_stereo_bm are timed on query
//                                        frame 0, alternating (medians of reps runs).
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

static void prefilter_host(const uint8_t *I, int w, int h, int cap, uint8_t *P)
{
    for (int y = 0; y < h; y++) {
        const uint8_t *r0 = I + (size_t)(y > 0 ? y - 1 : h > 1 ? 1 : 0) * w, *r1 = I + (size_t)y * w, *r2 = I + (size_t)(y + 1 < h ? y + 1 : h > 1 ? h - 2 : 0) * w;
        for (int x = 0; x < w; x++) {
            if (x == 0 || x == w - 1) { P[(size_t)y * w + x] = (uint8_t)cap; continue; }
            const int v = (r0[x + 1] - r0[x - 1]) + 2 * (r1[x + 1] - r1[x - 1]) + (r2[x + 1] - r2[x - 1]);
            P[(size_t)y * w + x] = (uint8_t)(std::min(std::max(v, -cap), cap) + cap);
        }
    }
}

// The definition, with the window sums taken as running sums: per disparity, column sums over the 2r + 1 rows of the window (one row
// enters, one leaves) and a sliding sum of 2r + 1 of them.  sad[d] holds SAD(d) of every defined pixel; T likewise.
static void stereo_bm_host(const uint8_t *L, const uint8_t *R, int w, int h, const chip_stereo_bm_params &p, int16_t *out)
{
    const int nd = p.num_disparities, r = p.block_size / 2, cap = p.prefilter_cap;
    std::fill(out, out + (size_t)w * h, (int16_t)-16);
    const int y0 = r, y1 = h - 1 - r, x0 = nd - 1 + r, x1 = w - 1 - r;
    if (y1 < y0 || x1 < x0) return;
    std::vector<uint8_t> PL((size_t)w * h), PR((size_t)w * h);
    prefilter_host(L, w, h, cap, PL.data());
    prefilter_host(R, w, h, cap, PR.data());
    const int Wd = x1 - x0 + 1, Hd = y1 - y0 + 1;
    const size_t plane = (size_t)Wd * Hd;
    std::vector<int32_t> sad((size_t)nd * plane), T(plane), col((size_t)w);
    // |a - b| of row y at column x for plane d (d == nd: the texture plane, against cap)
    const auto diff = [&](int d, int y, int x) {
        const int a = PL[(size_t)y * w + x], b = d == nd ? cap : PR[(size_t)y * w + x - d];
        return a > b ? a - b : b - a;
    };
    for (int d = 0; d <= nd; d++) {
        int32_t *dst = d == nd ? T.data() : sad.data() + (size_t)d * plane;
        for (int x = nd - 1; x < w; x++) {
            col[(size_t)x] = 0;
            for (int y = 0; y <= 2 * r; y++) col[(size_t)x] += diff(d, y, x);
        }
        for (int y = y0; y <= y1; y++) {
            if (y > y0)
                for (int x = nd - 1; x < w; x++) col[(size_t)x] += diff(d, y + r, x) - diff(d, y - r - 1, x);
            int32_t s = 0;
            for (int x = x0 - r; x <= x0 + r; x++) s += col[(size_t)x];
            for (int x = x0; x <= x1; x++) {
                if (x > x0) s += col[(size_t)(x + r)] - col[(size_t)(x - r - 1)];
                dst[(size_t)(y - y0) * Wd + (x - x0)] = s;
            }
        }
    }
    for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++) {
            const size_t at = (size_t)(y - y0) * Wd + (x - x0);
            const auto S = [&](int d) { return sad[(size_t)d * plane + at]; };
            int32_t m = S(0);
            int D = 0;
            for (int d = 1; d < nd; d++)
                if (S(d) <= m) { m = S(d); D = d; }              // the LARGEST d with the smallest SAD
            if (T[at] < p.texture_threshold) continue;
            if (p.uniqueness_ratio > 0) {
                const int32_t thresh = m + m * p.uniqueness_ratio / 100;
                bool unique = true;
                for (int d = 0; d < nd && unique; d++) unique = !(std::abs(d - D) > 1 && S(d) <= thresh);
                if (!unique) continue;
            }
            const int32_t pp = D == 0 ? S(1) : D == nd - 1 ? S(nd - 2) : S(D - 1), nn = D == 0 ? S(1) : D == nd - 1 ? S(nd - 2) : S(D + 1);
            const int32_t q = pp + nn - 2 * m + std::abs(pp - nn);
            out[(size_t)y * w + x] = (int16_t)((D * 256 + (q != 0 ? (pp - nn) * 256 / q : 0) + 15) >> 4);
        }
}

// CameraGeometry.cpp:485-523, for the timing of chip_frame_put with the 3-D image (built with -ffp-contract=off)
static void disparity_to_xyz_host(const int16_t *disp, int W, int H, const double Q[16], float *xyz)
{
    const float Q03 = (float)Q[3], Q13 = (float)Q[7], Q23 = (float)Q[11], Q32 = (float)Q[14], Q33 = (float)Q[15];
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const float d = (float)disp[(size_t)i * W + j];
            const float pw = (float)(1.0 / ((((double)d / 16.0) * (double)Q32 + (double)Q33) + 1e-6));
            float *p = xyz + 3 * ((size_t)i * W + j);
            p[0] = ((float)j + Q03) * pw;
            p[1] = ((float)i + Q13) * pw;
            p[2] = Q23 * pw;
        }
}

struct Frame {
    std::vector<float> kp;
    std::vector<uint8_t> desc, left, right;
    std::vector<int16_t> disp;                               // the host restatement's map of (left, right)
    int32_t n() const { return (int32_t)(kp.size() / 2); }
};

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 3000;
    const int P = argc > 2 ? std::atoi(argv[2]) : 6;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
    if (n < 1 || n > CHIP_MATCH_MAX_KEYPOINTS || P < 3 || P > CHIP_MATCH_MAX_PAIRS || reps < 0) {
        std::fprintf(stderr, "usage: frame_put_stereo [n_points in 1..%d] [P in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_PAIRS);
        return 2;
    }
    const int W = 752, H = 480, TILE = 94, PAD = 64;
    const double f = 458.654, cx = 367.215803962, cy = 248.375340610, baseline = 0.110073808127;
    const double Kinv[9] = {1.0 / f, 0.0, -cx / f, 0.0, 1.0 / f, -cy / f, 0.0, 0.0, 1.0};
    const double Q[16] = {1.0, 0.0, 0.0, -cx, 0.0, 1.0, 0.0, -cy, 0.0, 0.0, 0.0, f, 0.0, 0.0, 1.0 / baseline, 0.0};   // cv::stereoRectify
    chip_stereo_bm_params bm;
    chip_stereo_bm_params_default(&bm);

    // a rectified pair: a random texture PAD columns wider than the image, smoothed once (3 x 3 box); the right image is its last W columns,
    // the left image the same shifted by the tile's disparity (8 .. 40 pixels: 1.3 .. 6.3 m)
    std::mt19937_64 rng(42);
    const auto make_pair = [&](Frame &fr, uint64_t tiles_seed) {
        const int BW = W + PAD;
        std::vector<uint8_t> raw((size_t)BW * H), base((size_t)BW * H);
        for (auto &v : raw) v = (uint8_t)(rng() & 0xff);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < BW; x++) {
                int s = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) s += raw[(size_t)std::min(std::max(y + dy, 0), H - 1) * BW + std::min(std::max(x + dx, 0), BW - 1)];
                base[(size_t)y * BW + x] = (uint8_t)((s + 4) / 9);
            }
        std::mt19937_64 tr(tiles_seed);
        const int tw = (W + TILE - 1) / TILE, th = (H + TILE - 1) / TILE;
        std::vector<int> shift((size_t)tw * th);
        for (auto &s : shift) s = 8 + (int)(tr() % 33);
        fr.left.resize((size_t)W * H);
        fr.right.resize((size_t)W * H);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                fr.right[(size_t)y * W + x] = base[(size_t)y * BW + x + PAD];
                fr.left[(size_t)y * W + x] = base[(size_t)y * BW + x + PAD - shift[(size_t)(y / TILE) * tw + x / TILE]];
            }
        fr.disp.resize((size_t)W * H);
        stereo_bm_host(fr.left.data(), fr.right.data(), W, H, bm, fr.disp.data());
    };

    // P places: query view k has random keypoints (the later the place, the fewer), its second view sees them two pixels on under the same
    // tiling of disparities (4 % of the descriptor bits differ)
    std::uniform_real_distribution<double> ux(90.0, W - 14.0), uy(12.0, H - 12.0), u01(0.0, 1.0);
    std::vector<Frame> qs((size_t)P), cs((size_t)P);
    for (int k = 0; k < P; k++) {
        Frame &a = qs[(size_t)k], &b = cs[(size_t)k];
        const int want = std::max(1, n - (n / 20) * k);
        for (int i = 0; i < want; i++) {
            const float u = (float)ux(rng), v = (float)uy(rng);
            a.kp.push_back(u); a.kp.push_back(v);
            b.kp.push_back(u + 2.0f); b.kp.push_back(v);
            for (int d = 0; d < CHIP_ORB_DESC_BYTES; d++) {
                const uint8_t byte = (uint8_t)(rng() & 0xff);
                uint8_t flip = 0;
                for (int bit = 0; bit < 8; bit++) flip |= (uint8_t)((u01(rng) < 0.04) << bit);
                a.desc.push_back(byte);
                b.desc.push_back(byte ^ flip);
            }
        }
        make_pair(a, 100 + (uint64_t)k);
        make_pair(b, 100 + (uint64_t)k);
    }
    Frame empty;
    make_pair(empty, 99);

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    chip_ctx *ctx = cer.ctx();
    // keyframe arrival.  From the pair: ids 1000 + k (query k), k (its second view), -1 (empty); through the host restatement's map: the
    // same + 5000
    const int64_t via_map = 5000;
    const auto put_both = [&](int64_t id, const Frame &fr) {
        const int rc = chip_frame_put_stereo(ctx, id, fr.desc.data(), fr.kp.data(), fr.n(), W, H, fr.left.data(), fr.right.data(), &bm, Q);
        if (rc != CHIP_OK) return rc;
        return chip_frame_put_disparity(ctx, id + via_map, fr.desc.data(), fr.kp.data(), fr.n(), W, H, fr.disp.data(), CHIP_DISP_S16, Q);
    };
    int rc = chip_frame_store_reserve(ctx, 2 * (2 * P + 1), qs[0].n());
    for (int k = 0; k < P && rc == CHIP_OK; k++) {
        rc = put_both(1000 + k, qs[(size_t)k]);
        if (rc == CHIP_OK) rc = put_both(k, cs[(size_t)k]);
    }
    if (rc == CHIP_OK) rc = put_both(-1, empty);
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }

    // the backlog: pair k = (query k, its second view), but the last two: an unrelated pair and an empty candidate
    std::vector<int64_t> a_ids, b_ids, a_map, b_map;
    std::vector<uint64_t> seeds;
    for (int k = 0; k < P; k++) {
        a_ids.push_back(1000 + k);
        b_ids.push_back(k == P - 1 ? -1 : k == P - 2 ? 0 : k);
        a_map.push_back(a_ids.back() + via_map);
        b_map.push_back(b_ids.back() + via_map);
        seeds.push_back(7 + 10 * (uint64_t)k);
    }
    int differ = 0;
    // the records themselves, frame by frame
    std::vector<float> rec_s(4 * (size_t)qs[0].n()), rec_m(rec_s.size());
    size_t with_depth = 0;
    for (int k = 0; k < 2 * P; k++) {
        const int64_t id = k < P ? 1000 + k : k - P;
        int32_t ns = 0, nm = 0;
        if (chip_frame_read(ctx, id, &ns, nullptr, nullptr, nullptr, nullptr, rec_s.data()) != CHIP_OK ||
            chip_frame_read(ctx, id + via_map, &nm, nullptr, nullptr, nullptr, nullptr, rec_m.data()) != CHIP_OK) return 1;
        if (ns != nm || std::memcmp(rec_s.data(), rec_m.data(), 16 * (size_t)ns) != 0) {
            std::printf("frame %lld: the records DIFFER\n", (long long)id);
            differ++;
        }
        for (int32_t i = 0; i < ns; i++) with_depth += rec_s[4 * (size_t)i + 2] > 0.1f;
    }
    std::printf("%zu keypoints of %d frames have a depth\n", with_depth, 2 * P);
    if (with_depth == 0) { std::printf("no keypoint has a depth: the comparison DIFFERS from a meaningful one\n"); differ++; }

    const auto fresh = [&](std::vector<ProcessedLoopCandidate> &pc) {
        pc.assign((size_t)P, ProcessedLoopCandidate());
        for (int j = 0; j < P; j++) { pc[(size_t)j].t_node_1 = Time{100 + (uint32_t)j, 0}; pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
    };
    std::vector<ProcessedLoopCandidate> from_pair, from_map;
    bool ok_s[CHIP_MATCH_MAX_PAIRS] = {}, ok_m[CHIP_MATCH_MAX_PAIRS] = {};
    chip_match_summary sm_s[CHIP_MATCH_MAX_PAIRS] = {}, sm_m[CHIP_MATCH_MAX_PAIRS] = {};
    chip_gms_choice ch_s[CHIP_MATCH_MAX_PAIRS] = {}, ch_m[CHIP_MATCH_MAX_PAIRS] = {};
    fresh(from_pair);
    fresh(from_map);
    if (!verify_pairs_stored(ctx, a_ids.data(), b_ids.data(), P, Kinv, from_pair.data(), ok_s, seeds.data(), sm_s, 0, ch_s) ||
        !verify_pairs_stored(ctx, a_map.data(), b_map.data(), P, Kinv, from_map.data(), ok_m, seeds.data(), sm_m, 0, ch_m)) {
        std::fprintf(stderr, "frame_put_stereo: a library call failed\n");
        return 1;
    }
    for (int j = 0; j < P; j++) {
        const ProcessedLoopCandidate &p = from_pair[(size_t)j], &q = from_map[(size_t)j];
        bool same = ok_s[j] == ok_m[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size() && std::memcmp(&sm_s[j], &sm_m[j], sizeof(chip_match_summary)) == 0 &&
                    std::memcmp(&ch_s[j], &ch_m[j], sizeof(chip_gms_choice)) == 0;
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        std::printf("pair %2d (%lld, %lld): n1=%d gms=%d 3d3d=%d  %s  %s\n", j, (long long)a_ids[(size_t)j], (long long)b_ids[(size_t)j], sm_s[j].n_matches_all,
                    sm_s[j].n_matches_gms, sm_s[j].n_3d3d, ok_s[j] ? "three poses" : "rejected",
                    same ? "== the same frames put through chip_frame_put_disparity" : "DIFFERS from the same frames put through chip_frame_put_disparity");
        differ += !same;
    }

    if (reps > 0) {
        const auto now = [] { return std::chrono::steady_clock::now(); };
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        const Frame &fr = qs[0];
        std::vector<float> xyz((size_t)W * H * 3);
        std::vector<int16_t> dense((size_t)W * H), host((size_t)W * H);
        disparity_to_xyz_host(fr.disp.data(), W, H, Q, xyz.data());
        const chip_match_frame mf{fr.desc.data(), fr.kp.data(), fr.n(), W, H, xyz.data()};
        std::vector<double> t_img, t_s16, t_pair, t_host, t_dense;
        for (int r = 0; r < reps + 3; r++) {                  // the variants alternate; three warm-up rounds
            auto t0 = now();
            if (chip_frame_put(ctx, 1000 + via_map, &mf) != CHIP_OK) return 1;
            const double a = ms(t0, now());
            t0 = now();
            if (chip_frame_put_disparity(ctx, 1000 + via_map, fr.desc.data(), fr.kp.data(), fr.n(), W, H, fr.disp.data(), CHIP_DISP_S16, Q) != CHIP_OK) return 1;
            const double b = ms(t0, now());
            t0 = now();
            if (chip_frame_put_stereo(ctx, 1000, fr.desc.data(), fr.kp.data(), fr.n(), W, H, fr.left.data(), fr.right.data(), &bm, Q) != CHIP_OK) return 1;
            const double c = ms(t0, now());
            t0 = now();
            stereo_bm_host(fr.left.data(), fr.right.data(), W, H, bm, host.data());
            const double d = ms(t0, now());
            t0 = now();
            if (chip_stereo_bm(ctx, fr.left.data(), fr.right.data(), W, H, &bm, dense.data()) != CHIP_OK) return 1;
            const double e = ms(t0, now());
            if (r >= 3) { t_img.push_back(a); t_s16.push_back(b); t_pair.push_back(c); t_host.push_back(d); t_dense.push_back(e); }
        }
        if (dense != host) { std::printf("chip_stereo_bm DIFFERS from the host restatement\n"); differ++; }
        std::printf("timing %dx%d n=%d reps=%d (medians, ms): chip_frame_put %.3f, chip_frame_put_disparity S16 %.3f, chip_frame_put_stereo %.3f; "
                    "host restatement (a plain loop, not OpenCV) %.3f, chip_stereo_bm %.3f\n", W, H, fr.n(), reps, median(t_img), median(t_s16),
                    median(t_pair), median(t_host), median(t_dense));
    }
    return differ == 0 ? 0 : 1;
}
