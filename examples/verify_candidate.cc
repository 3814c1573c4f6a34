// examples/verify_candidate.cc -- one loop candidate through the candidate verification front end and the three poses, as the patched
// Cerebro::process_loop_candidate_imagepair_consistent_pose_compute does: keypoints + descriptors + 3-D images
// in, LoopEdge out.  No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   verify_candidate [n_points]      default 3000.  Two synthetic views of one random point cloud with a known relative pose; with a few
//                                    thousand points the candidate passes the consistency gate and a LoopEdge is printed, with ~100 it is
//                                    rejected by the "< 150 matches" rule (Cerebro.cpp:1487).  Exit code 0 iff the outcome is the expected one.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../cerebro_amd/host/cerebro_host.h"

using namespace cerebro_hip;

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 3000;
    if (n < 1 || n > CHIP_MATCH_MAX_KEYPOINTS) { std::fprintf(stderr, "n_points must be in [1, %d]\n", CHIP_MATCH_MAX_KEYPOINTS); return 2; }
    const int W = 752, H = 480;
    const double f = 458.0, cx = W / 2.0, cy = H / 2.0;
    const double Kinv[9] = {1.0 / f, 0.0, -cx / f, 0.0, 1.0 / f, -cy / f, 0.0, 0.0, 1.0};
    const double yaw = 2.0 * M_PI / 180.0, t[3] = {0.15, 0.02, 0.05};                  // b_T_a
    const double R[9] = {std::cos(yaw), 0.0, std::sin(yaw), 0.0, 1.0, 0.0, -std::sin(yaw), 0.0, std::cos(yaw)};

    std::mt19937_64 rng(42);
    std::uniform_real_distribution<double> ux(1.0, W - 2.0), uy(1.0, H - 2.0), uz(3.0, 12.0), u01(0.0, 1.0);
    std::vector<float> kp_a, kp_b, xyz_a((size_t)W * H * 3, 0.f), xyz_b((size_t)W * H * 3, 0.f);
    std::vector<uint8_t> d_a, d_b, taken_a((size_t)W * H, 0), taken_b((size_t)W * H, 0);
    for (int i = 0; i < n; i++) {
        const float u = (float)ux(rng), v = (float)uy(rng);
        const double z = uz(rng);
        // the point of keypoint (u, v) at depth z, as the CV_32FC3 3-D image stores it
        const float Xa[3] = {(float)(z * ((double)u - cx) / f), (float)(z * ((double)v - cy) / f), (float)z};
        double Xb[3];
        for (int r = 0; r < 3; r++) Xb[r] = R[3 * r] * Xa[0] + R[3 * r + 1] * Xa[1] + R[3 * r + 2] * Xa[2] + t[r];
        const float ub = (float)(f * Xb[0] / Xb[2] + cx), vb = (float)(f * Xb[1] / Xb[2] + cy);
        if (!(ub >= 0.f && ub < (float)W && vb >= 0.f && vb < (float)H)) continue;
        const size_t pa = (size_t)(int)v * W + (size_t)(int)u, pb = (size_t)(int)vb * W + (size_t)(int)ub;
        if (taken_a[pa] || taken_b[pb]) continue;                                       // one 3-D point per pixel
        taken_a[pa] = taken_b[pb] = 1;
        for (int r = 0; r < 3; r++) { xyz_a[3 * pa + r] = Xa[r]; xyz_b[3 * pb + r] = (float)Xb[r]; }
        kp_a.push_back(u); kp_a.push_back(v); kp_b.push_back(ub); kp_b.push_back(vb);
        for (int k = 0; k < CHIP_ORB_DESC_BYTES; k++) {
            const uint8_t byte = (uint8_t)(rng() & 0xff);
            uint8_t flip = 0;
            for (int bit = 0; bit < 8; bit++) flip |= (uint8_t)((u01(rng) < 0.04) << bit);   // 4 % of the bits differ in the other view
            d_a.push_back(byte); d_b.push_back(byte ^ flip);
        }
    }
    const int m = (int)(kp_a.size() / 2);
    chip_match_frame fa{d_a.data(), kp_a.data(), m, W, H, xyz_a.data()}, fb{d_b.data(), kp_b.data(), m, W, H, xyz_b.data()};

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    ProcessedLoopCandidate pc;
    pc.t_node_1 = Time{100, 0}; pc.t_node_2 = Time{160, 0};                             // a minute apart (the gate wants >= 10 s)
    pc.idx_from_datamanager_1 = 1000; pc.idx_from_datamanager_2 = 1600;
    chip_match_summary sm{};
    bool posed = verify_candidate(cer.ctx(), fa, fb, Kinv, pc, 7, &sm);                 // first call: allocations, code objects
    const auto t0 = std::chrono::steady_clock::now();
    posed = verify_candidate(cer.ctx(), fa, fb, Kinv, pc, 7, &sm);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("keypoints %d / %d: matches_all=%d pf_matches=%d 3d2d_ab=%d 3d2d_ba=%d 3d3d=%d out_of_image=%d  verify_candidate %.3f ms (second call, one run)\n",
                m, m, sm.n_matches_all, sm.n_matches_gms, sm.n_3d2d_ab, sm.n_3d2d_ba, sm.n_3d3d, sm.n_out_of_image, ms);
    const bool expect_edge = n >= 2000;
    if (!posed) {
        std::printf("candidate rejected before the poses (%s)\n", sm.n_matches_gms < 150 ? "fewer than 150 GMS matches" : "no consistent pose");
        return expect_edge ? 1 : 0;
    }
    LoopEdgePOD msg;
    if (!pc.makeLoopEdgeMsgWithConsistencyCheck(msg)) {
        std::printf("candidate rejected by the consistency gate\n");
        return expect_edge ? 1 : 0;
    }
    double err = 0.0;                                                                    // b_T_a against the generator's
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) err = std::fmax(err, std::fabs(pc._3d2d__2T1[4 * c + r] - R[3 * r + c]));
        err = std::fmax(err, std::fabs(pc._3d2d__2T1[12 + r] - t[r]));
    }
    std::printf("LoopEdge %u.%09u -> %u.%09u  position (%.6f, %.6f, %.6f)  weight %.4f  |b_T_a - truth|_max = %.2e\n", msg.timestamp0.sec,
                msg.timestamp0.nsec, msg.timestamp1.sec, msg.timestamp1.nsec, msg.position[0], msg.position[1], msg.position[2], msg.weight, err);
    return expect_edge && err < 1e-3 ? 0 : 1;
}
