// examples/frame_put_disparity.cc -- keyframes handed over as what cv::StereoBM delivers, the CV_16SC1 disparity map, instead of the
// CV_32FC3 3-D image the reference makes from it on the host (StereoGeometry::disparity_to_3DPoints, src/utils/CameraGeometry.cpp:459-524,
// over all w x h pixels).  Every frame of a small pair backlog is put TWICE: once from its disparity
// (chip_frame_put_disparity: the 3-D points are computed on the device, at the keypoints) and once through chip_frame_put with the 3-D
// image computed by the plain C++ loop below, the reference's loop restated.  verify_pairs_stored then runs on both id sets; every
// record, summary, GMS choice, accept flag, pose and goodness must have the same bits.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   frame_put_disparity [n_points] [P] [reps]   defaults 3000, 6, 0.  P places, each with a query frame of its own and a second view of
//                                        it; the last two pairs are an unrelated pair and a pair with an empty candidate.  Prints one
//                                        line per pair; exit code 0 iff the two ways of putting agree in everything.  With reps > 0 the
//                                        two puts (and the put of a float disparity), the host loop and chip_disparity_to_xyz are timed
//                                        on query frame 0, alternating (medians of reps runs).
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

// CameraGeometry.cpp:485-523: five entries of Q narrowed to float, pw in double with ONE narrowing, three float products.  Built
// without FMA contraction (the Makefile passes -ffp-contract=off), as the reference is.
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
    std::vector<uint8_t> desc;
    std::vector<int16_t> disp;
    int32_t n() const { return (int32_t)(kp.size() / 2); }
};

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 3000;
    const int P = argc > 2 ? std::atoi(argv[2]) : 6;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
    if (n < 1 || n > CHIP_MATCH_MAX_KEYPOINTS || P < 3 || P > CHIP_MATCH_MAX_PAIRS || reps < 0) {
        std::fprintf(stderr, "usage: frame_put_disparity [n_points in 1..%d] [P in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_PAIRS);
        return 2;
    }
    const int W = 752, H = 480;
    const double f = 458.654, cx = 367.215803962, cy = 248.375340610, baseline = 0.110073808127;
    const double Kinv[9] = {1.0 / f, 0.0, -cx / f, 0.0, 1.0 / f, -cy / f, 0.0, 0.0, 1.0};
    const double Q[16] = {1.0, 0.0, 0.0, -cx, 0.0, 1.0, 0.0, -cy, 0.0, 0.0, 0.0, f, 0.0, 0.0, 1.0 / baseline, 0.0};   // cv::stereoRectify
    const int16_t invalid = -16;                             // StereoBM's (minDisparity - 1) * 16: z < 0, dropped by the depth gate
    const auto raw_of = [&](double z) { return (int16_t)std::lround(16.0 * f * baseline / z); };

    // P places: query view k sees a point per keypoint (the later the place, the fewer keypoints), and what the frame carries of it is the
    // raw disparity at that pixel; a second view of the same cloud (4 % of the descriptor bits differ)
    std::mt19937_64 rng(42);
    std::uniform_real_distribution<double> ux(1.0, W - 2.0), uy(1.0, H - 2.0), uz(2.0, 6.0), u01(0.0, 1.0);
    std::vector<Frame> qs((size_t)P), cs((size_t)P);
    for (int k = 0; k < P; k++) {
        Frame &a = qs[(size_t)k], &b = cs[(size_t)k];
        a.disp.assign((size_t)W * H, invalid);
        b.disp.assign((size_t)W * H, invalid);
        const int want = std::max(1, n - (n / 20) * k);
        std::vector<double> Xa;
        std::vector<uint8_t> taken((size_t)W * H, 0);
        for (int i = 0; i < want; i++) {
            const float u = (float)ux(rng), v = (float)uy(rng);
            const double z = uz(rng);
            const size_t px = (size_t)(int)v * W + (size_t)(int)u;
            if (taken[px]) continue;
            taken[px] = 1;
            a.disp[px] = raw_of(z);
            const double X[3] = {z * ((double)u - cx) / f, z * ((double)v - cy) / f, z};
            for (int r = 0; r < 3; r++) Xa.push_back(X[r]);
            a.kp.push_back(u); a.kp.push_back(v);
            for (int d = 0; d < CHIP_ORB_DESC_BYTES; d++) a.desc.push_back((uint8_t)(rng() & 0xff));
        }
        const int m = a.n();
        const double yaw = (k % 2 ? -1.0 : 1.0) * (1.0 + k % 5) * M_PI / 180.0, t[3] = {0.15 - 0.05 * (k % 5), 0.02, 0.05 + 0.02 * (k % 5)};   // b_T_a
        const double R[9] = {std::cos(yaw), 0.0, std::sin(yaw), 0.0, 1.0, 0.0, -std::sin(yaw), 0.0, std::cos(yaw)};
        std::fill(taken.begin(), taken.end(), 0);
        for (int i = 0; i < m; i++) {
            double Xb[3];
            for (int r = 0; r < 3; r++) Xb[r] = R[3 * r] * Xa[3 * (size_t)i] + R[3 * r + 1] * Xa[3 * (size_t)i + 1] + R[3 * r + 2] * Xa[3 * (size_t)i + 2] + t[r];
            const float ub = (float)(f * Xb[0] / Xb[2] + cx), vb = (float)(f * Xb[1] / Xb[2] + cy);
            if (!(ub >= 0.f && ub < (float)W && vb >= 0.f && vb < (float)H)) continue;
            const size_t px = (size_t)(int)vb * W + (size_t)(int)ub;
            if (taken[px]) continue;
            taken[px] = 1;
            b.disp[px] = raw_of(Xb[2]);
            b.kp.push_back(ub); b.kp.push_back(vb);
            for (int d = 0; d < CHIP_ORB_DESC_BYTES; d++) {
                uint8_t flip = 0;
                for (int bit = 0; bit < 8; bit++) flip |= (uint8_t)((u01(rng) < 0.04) << bit);
                b.desc.push_back(a.desc[(size_t)i * CHIP_ORB_DESC_BYTES + d] ^ flip);
            }
        }
    }
    Frame empty;
    empty.disp.assign((size_t)W * H, invalid);

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    chip_ctx *ctx = cer.ctx();
    // keyframe arrival.  From the disparity: ids 1000 + k (query k), k (its second view), -1 (empty); through the host loop and the 3-D
    // image: the same + 5000
    const int64_t via_image = 5000;
    std::vector<float> xyz((size_t)W * H * 3);
    const auto put_both = [&](int64_t id, const Frame &fr) {
        int rc = chip_frame_put_disparity(ctx, id, fr.desc.data(), fr.kp.data(), fr.n(), W, H, fr.disp.data(), CHIP_DISP_S16, Q);
        if (rc != CHIP_OK) return rc;
        disparity_to_xyz_host(fr.disp.data(), W, H, Q, xyz.data());
        const chip_match_frame mf{fr.desc.data(), fr.kp.data(), fr.n(), W, H, xyz.data()};
        return chip_frame_put(ctx, id + via_image, &mf);
    };
    int rc = chip_frame_store_reserve(ctx, 2 * (2 * P + 1), qs[0].n());
    for (int k = 0; k < P && rc == CHIP_OK; k++) {
        rc = put_both(1000 + k, qs[(size_t)k]);
        if (rc == CHIP_OK) rc = put_both(k, cs[(size_t)k]);
    }
    if (rc == CHIP_OK) rc = put_both(-1, empty);
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }

    // the backlog: pair k = (query k, its second view), but the last two: an unrelated pair and an empty candidate
    std::vector<int64_t> a_ids, b_ids, a_img, b_img;
    std::vector<uint64_t> seeds;
    for (int k = 0; k < P; k++) {
        a_ids.push_back(1000 + k);
        b_ids.push_back(k == P - 1 ? -1 : k == P - 2 ? 0 : k);
        a_img.push_back(a_ids.back() + via_image);
        b_img.push_back(b_ids.back() + via_image);
        seeds.push_back(7 + 10 * (uint64_t)k);
    }
    int differ = 0;
    // the records themselves, frame by frame
    std::vector<float> rec_d(4 * (size_t)qs[0].n()), rec_i(rec_d.size());
    for (int k = 0; k < 2 * P; k++) {
        const int64_t id = k < P ? 1000 + k : k - P;
        int32_t nd = 0, ni = 0;
        if (chip_frame_read(ctx, id, &nd, nullptr, nullptr, nullptr, nullptr, rec_d.data()) != CHIP_OK ||
            chip_frame_read(ctx, id + via_image, &ni, nullptr, nullptr, nullptr, nullptr, rec_i.data()) != CHIP_OK) return 1;
        if (nd != ni || std::memcmp(rec_d.data(), rec_i.data(), 16 * (size_t)nd) != 0) {
            std::printf("frame %lld: the records DIFFER\n", (long long)id);
            differ++;
        }
    }

    const auto fresh = [&](std::vector<ProcessedLoopCandidate> &pc) {
        pc.assign((size_t)P, ProcessedLoopCandidate());
        for (int j = 0; j < P; j++) { pc[(size_t)j].t_node_1 = Time{100 + (uint32_t)j, 0}; pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
    };
    std::vector<ProcessedLoopCandidate> from_disp, from_img;
    bool ok_d[CHIP_MATCH_MAX_PAIRS] = {}, ok_i[CHIP_MATCH_MAX_PAIRS] = {};
    chip_match_summary sm_d[CHIP_MATCH_MAX_PAIRS] = {}, sm_i[CHIP_MATCH_MAX_PAIRS] = {};
    chip_gms_choice ch_d[CHIP_MATCH_MAX_PAIRS] = {}, ch_i[CHIP_MATCH_MAX_PAIRS] = {};
    fresh(from_disp);
    fresh(from_img);
    if (!verify_pairs_stored(ctx, a_ids.data(), b_ids.data(), P, Kinv, from_disp.data(), ok_d, seeds.data(), sm_d, 0, ch_d) ||
        !verify_pairs_stored(ctx, a_img.data(), b_img.data(), P, Kinv, from_img.data(), ok_i, seeds.data(), sm_i, 0, ch_i)) {
        std::fprintf(stderr, "frame_put_disparity: a library call failed\n");
        return 1;
    }
    for (int j = 0; j < P; j++) {
        const ProcessedLoopCandidate &p = from_disp[(size_t)j], &q = from_img[(size_t)j];
        bool same = ok_d[j] == ok_i[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size() && std::memcmp(&sm_d[j], &sm_i[j], sizeof(chip_match_summary)) == 0 &&
                    std::memcmp(&ch_d[j], &ch_i[j], sizeof(chip_gms_choice)) == 0;
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        std::printf("pair %2d (%lld, %lld): n1=%d gms=%d 3d3d=%d  %s  %s\n", j, (long long)a_ids[(size_t)j], (long long)b_ids[(size_t)j], sm_d[j].n_matches_all,
                    sm_d[j].n_matches_gms, sm_d[j].n_3d3d, ok_d[j] ? "three poses" : "rejected",
                    same ? "== the same frames put through chip_frame_put" : "DIFFERS from the same frames put through chip_frame_put");
        differ += !same;
    }

    if (reps > 0) {
        const auto now = [] { return std::chrono::steady_clock::now(); };
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        const Frame &fr = qs[0];
        std::vector<float> dispf(fr.disp.begin(), fr.disp.end()), dense((size_t)W * H * 3);
        disparity_to_xyz_host(fr.disp.data(), W, H, Q, xyz.data());
        const chip_match_frame mf{fr.desc.data(), fr.kp.data(), fr.n(), W, H, xyz.data()};
        std::vector<double> t_img, t_s16, t_f32, t_host, t_dense;
        for (int r = 0; r < reps + 3; r++) {                  // the variants alternate; three warm-up rounds
            auto t0 = now();
            if (chip_frame_put(ctx, 1000 + via_image, &mf) != CHIP_OK) return 1;
            const double a = ms(t0, now());
            t0 = now();
            if (chip_frame_put_disparity(ctx, 1000, fr.desc.data(), fr.kp.data(), fr.n(), W, H, fr.disp.data(), CHIP_DISP_S16, Q) != CHIP_OK) return 1;
            const double b = ms(t0, now());
            t0 = now();
            if (chip_frame_put_disparity(ctx, 1000, fr.desc.data(), fr.kp.data(), fr.n(), W, H, dispf.data(), CHIP_DISP_F32, Q) != CHIP_OK) return 1;
            const double c = ms(t0, now());
            t0 = now();
            disparity_to_xyz_host(fr.disp.data(), W, H, Q, dense.data());
            const double d = ms(t0, now());
            t0 = now();
            if (chip_disparity_to_xyz(ctx, fr.disp.data(), CHIP_DISP_S16, W, H, Q, dense.data()) != CHIP_OK) return 1;
            const double e = ms(t0, now());
            if (r >= 3) { t_img.push_back(a); t_s16.push_back(b); t_f32.push_back(c); t_host.push_back(d); t_dense.push_back(e); }
        }
        if (std::memcmp(dense.data(), xyz.data(), dense.size() * sizeof(float)) != 0) { std::printf("chip_disparity_to_xyz DIFFERS from the host loop\n"); differ++; }
        std::printf("timing %dx%d n=%d reps=%d (medians, ms): chip_frame_put %.3f, chip_frame_put_disparity S16 %.3f, F32 %.3f; host loop %.3f, "
                    "chip_disparity_to_xyz %.3f\n", W, H, fr.n(), reps, median(t_img), median(t_s16), median(t_f32), median(t_host), median(t_dense));
    }
    return differ == 0 ? 0 : 1;
}
