// examples/verify_candidates_stored.cc -- all loop candidates of one keyframe verified on frames KEPT ON THE DEVICE:
// the query and the B candidates are put into the frame store once (chip_frame_put), then verify_candidates_stored
// (chip_match_batch_stored + chip_pnp_ransac_matched_batch + ICP per survivor: no upload) runs against verify_candidates on the same
// host frames.  No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   verify_candidates_stored [n_points] [B] [reps]   defaults 3000, 6, 0.  The scene of examples/verify_candidates.cc: B - 2 views of a
//                                              random point cloud, one UNRELATED frame and one EMPTY frame.  Prints one line per
//                                              candidate; exit code 0 iff both paths agree in every ProcessedLoopCandidate field and
//                                              every summary.  With reps > 0 both paths are then timed (median of reps runs).
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

struct Frame {
    std::vector<float> kp, xyz;
    std::vector<uint8_t> desc;
    chip_match_frame view(int W, int H) const { return chip_match_frame{desc.data(), kp.data(), (int32_t)(kp.size() / 2), W, H, xyz.data()}; }
};

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 3000;
    const int B = argc > 2 ? std::atoi(argv[2]) : 6;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
    if (n < 1 || n > CHIP_MATCH_MAX_KEYPOINTS || B < 3 || B > CHIP_MATCH_MAX_BATCH || reps < 0) {
        std::fprintf(stderr, "usage: verify_candidates_stored [n_points in 1..%d] [B in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_BATCH);
        return 2;
    }
    const int W = 752, H = 480;
    const double f = 458.0, cx = W / 2.0, cy = H / 2.0;
    const double Kinv[9] = {1.0 / f, 0.0, -cx / f, 0.0, 1.0 / f, -cy / f, 0.0, 0.0, 1.0};

    // the query view: one 3-D point per pixel, as the CV_32FC3 3-D image stores it
    std::mt19937_64 rng(42);
    std::uniform_real_distribution<double> ux(1.0, W - 2.0), uy(1.0, H - 2.0), uz(3.0, 12.0), u01(0.0, 1.0);
    Frame a;
    a.xyz.assign((size_t)W * H * 3, 0.f);
    std::vector<float> Xa;
    {
        std::vector<uint8_t> taken((size_t)W * H, 0);
        for (int i = 0; i < n; i++) {
            const float u = (float)ux(rng), v = (float)uy(rng);
            const double z = uz(rng);
            const size_t px = (size_t)(int)v * W + (size_t)(int)u;
            if (taken[px]) continue;
            taken[px] = 1;
            const float X[3] = {(float)(z * ((double)u - cx) / f), (float)(z * ((double)v - cy) / f), (float)z};
            for (int r = 0; r < 3; r++) { a.xyz[3 * px + r] = X[r]; Xa.push_back(X[r]); }
            a.kp.push_back(u); a.kp.push_back(v);
            for (int k = 0; k < CHIP_ORB_DESC_BYTES; k++) a.desc.push_back((uint8_t)(rng() & 0xff));
        }
    }
    const int m = (int)(a.kp.size() / 2);

    // the candidates: views of the same cloud (4 % of the descriptor bits differ), an unrelated frame, an empty frame
    std::vector<Frame> cands((size_t)B);
    for (int j = 0; j < B; j++) {
        Frame &b = cands[(size_t)j];
        b.xyz.assign((size_t)W * H * 3, 0.f);
        if (j == B - 1) continue;                                                         // empty
        if (j == B - 2) {                                                                 // unrelated
            for (int i = 0; i < m; i++) {
                b.kp.push_back((float)ux(rng)); b.kp.push_back((float)uy(rng));
                for (int k = 0; k < CHIP_ORB_DESC_BYTES; k++) b.desc.push_back((uint8_t)(rng() & 0xff));
            }
            continue;
        }
        const double yaw = (j % 2 ? -1.0 : 1.0) * (1.0 + j) * M_PI / 180.0, t[3] = {0.15 - 0.05 * j, 0.02, 0.05 + 0.02 * j};   // b_T_a
        const double R[9] = {std::cos(yaw), 0.0, std::sin(yaw), 0.0, 1.0, 0.0, -std::sin(yaw), 0.0, std::cos(yaw)};
        std::vector<uint8_t> taken((size_t)W * H, 0);
        for (int i = 0; i < m; i++) {
            double Xb[3];
            for (int r = 0; r < 3; r++) Xb[r] = R[3 * r] * Xa[3 * i] + R[3 * r + 1] * Xa[3 * i + 1] + R[3 * r + 2] * Xa[3 * i + 2] + t[r];
            const float ub = (float)(f * Xb[0] / Xb[2] + cx), vb = (float)(f * Xb[1] / Xb[2] + cy);
            if (!(ub >= 0.f && ub < (float)W && vb >= 0.f && vb < (float)H)) continue;
            const size_t px = (size_t)(int)vb * W + (size_t)(int)ub;
            if (taken[px]) continue;
            taken[px] = 1;
            for (int r = 0; r < 3; r++) b.xyz[3 * px + r] = (float)Xb[r];
            b.kp.push_back(ub); b.kp.push_back(vb);
            for (int k = 0; k < CHIP_ORB_DESC_BYTES; k++) {
                uint8_t flip = 0;
                for (int bit = 0; bit < 8; bit++) flip |= (uint8_t)((u01(rng) < 0.04) << bit);
                b.desc.push_back(a.desc[(size_t)i * CHIP_ORB_DESC_BYTES + k] ^ flip);
            }
        }
    }
    const chip_match_frame fa = a.view(W, H);
    std::vector<chip_match_frame> fb;
    std::vector<uint64_t> seeds;
    for (int j = 0; j < B; j++) { fb.push_back(cands[(size_t)j].view(W, H)); seeds.push_back(7 + 10 * (uint64_t)j); }

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    // keyframe arrival: every frame is put once; the ids are the integrator's (here 1000 for the query, j for candidate j)
    int rc = chip_frame_store_reserve(cer.ctx(), B + 1, m);
    if (rc == CHIP_OK) rc = chip_frame_put(cer.ctx(), 1000, &fa);
    std::vector<int64_t> ids;
    for (int j = 0; j < B && rc == CHIP_OK; j++) { ids.push_back(j); rc = chip_frame_put(cer.ctx(), j, &fb[(size_t)j]); }
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }
    const auto fresh = [&](std::vector<ProcessedLoopCandidate> &pc) {
        pc.assign((size_t)B, ProcessedLoopCandidate());
        for (int j = 0; j < B; j++) { pc[(size_t)j].t_node_1 = Time{100, 0}; pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
    };
    std::vector<ProcessedLoopCandidate> host, stored;
    std::vector<chip_match_summary> sm_host((size_t)B), sm_stored((size_t)B);
    bool ok_host[CHIP_MATCH_MAX_BATCH] = {}, ok_stored[CHIP_MATCH_MAX_BATCH] = {};
    const auto run_host = [&] {
        fresh(host);
        return verify_candidates(cer.ctx(), fa, fb.data(), B, Kinv, host.data(), ok_host, seeds.data(), sm_host.data());
    };
    const auto run_stored = [&] {
        fresh(stored);
        return verify_candidates_stored(cer.ctx(), 1000, ids.data(), B, Kinv, stored.data(), ok_stored, seeds.data(), sm_stored.data());
    };
    if (!run_host() || !run_stored()) { std::fprintf(stderr, "verify_candidates_stored: a library call failed\n"); return 1; }

    int differ = 0;
    for (int j = 0; j < B; j++) {
        const ProcessedLoopCandidate &p = host[(size_t)j], &q = stored[(size_t)j];
        bool same = ok_host[j] == ok_stored[j] && p.pf_matches == q.pf_matches && p.t_node_1 == q.t_node_1 && p.t_node_2 == q.t_node_2 &&
                    p.idx_from_datamanager_1 == q.idx_from_datamanager_1 && p.idx_from_datamanager_2 == q.idx_from_datamanager_2 &&
                    p.isSet_3d2d__2T1 == q.isSet_3d2d__2T1 && std::memcmp(p._3d2d__2T1.data(), q._3d2d__2T1.data(), 16 * sizeof(double)) == 0 &&
                    std::memcmp(&p._3d2d__2T1__ransac_confidence, &q._3d2d__2T1__ransac_confidence, sizeof(float)) == 0 &&
                    std::memcmp(&sm_host[(size_t)j], &sm_stored[(size_t)j], sizeof(chip_match_summary)) == 0 &&
                    p.opX_b_T_a.size() == q.opX_b_T_a.size() && p.opX_goodness.size() == q.opX_goodness.size();
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        const chip_match_summary &s = sm_stored[(size_t)j];
        std::printf("candidate %2d: keypoints %d / %d matches_all=%d pf_matches=%d 3d2d_ab=%d 3d2d_ba=%d 3d3d=%d  %s  %s\n", j, m, fb[(size_t)j].n,
                    s.n_matches_all, s.n_matches_gms, s.n_3d2d_ab, s.n_3d2d_ba, s.n_3d3d,
                    ok_stored[j] ? "three poses" : (s.n_matches_gms < 150 ? "rejected: fewer than 150 GMS matches" : "rejected: no pose"),
                    same ? "== verify_candidates" : "DIFFERS from verify_candidates");
        differ += !same;
    }
    bool expected = !ok_stored[B - 1] && !ok_stored[B - 2];
    for (int j = 0; j < B - 2 && n >= 2000; j++) expected = expected && ok_stored[j];
    if (!expected) std::printf("unexpected outcome: which candidates passed is not what the scene was built for\n");

    if (reps > 0) {
        const auto median_ms = [&](const auto &fn) {
            std::vector<double> t;
            for (int r = 0; r < reps; r++) {
                const auto t0 = std::chrono::steady_clock::now();
                fn();
                t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(t.begin(), t.end());
            return t[t.size() / 2];
        };
        const double t_host = median_ms(run_host), t_stored = median_ms(run_stored);
        std::printf("timing B=%d n=%d reps=%d: verify_candidates %.3f ms, verify_candidates_stored %.3f ms (medians)\n", B, m, reps, t_host, t_stored);
    }
    return differ == 0 && expected ? 0 : 1;
}
