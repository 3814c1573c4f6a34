// examples/verify_candidates_composed.cc -- verify_candidates_stored against the same answer COMPOSED from the C ABI alone, one call at
// a time: chip_match_batch_stored, chip_pnp_ransac_matched_batch over the survivors, then per survivor
// chip_match_select + chip_icp_ransac_matched and the gates.  verify_candidates_stored runs the ICP of all survivors as ONE matched
// batch underneath the PnP call; the composition runs it as a loop of blocking calls after it.  Both must give the same bits.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   verify_candidates_composed [n_points] [B] [reps]   defaults 3000, 6, 0.  The scene of examples/verify_candidates_stored.cc.  Prints one
//                                              line per candidate; exit code 0 iff both paths agree bit for bit in every pose, goodness
//                                              and accept flag.  With reps > 0 both are then timed (median of reps runs), and the
//                                              composition is split into its match call, its PnP call and its ICP loop.
#include <algorithm>
#include <array>
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
        std::fprintf(stderr, "usage: verify_candidates_composed [n_points in 1..%d] [B in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_BATCH);
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
    std::vector<ProcessedLoopCandidate> stored, composed;
    bool ok_stored[CHIP_MATCH_MAX_BATCH] = {}, ok_composed[CHIP_MATCH_MAX_BATCH] = {};
    const auto run_stored = [&] {
        fresh(stored);
        return verify_candidates_stored(cer.ctx(), 1000, ids.data(), B, Kinv, stored.data(), ok_stored, seeds.data(), nullptr);
    };
    // the composition, one C call at a time; t[0..2]: wall time of the match call, the PnP call and the ICP loop (ms)
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto run_composed = [&](double *t) {
        fresh(composed);
        chip_ctx *ctx = cer.ctx();
        for (int j = 0; j < B; j++) ok_composed[j] = false;
        chip_match_summary sm[CHIP_MATCH_MAX_BATCH] = {};
        const auto t0 = now();
        if (chip_match_batch_stored(ctx, 1000, ids.data(), B, Kinv, sm) != CHIP_OK) return false;
        const auto t1 = now();
        chip_ransac_params pp, pi;
        chip_ransac_params_default(&pp);
        chip_icp_params_default(&pi);
        int32_t cand[2 * CHIP_MATCH_MAX_BATCH], which[2 * CHIP_MATCH_MAX_BATCH], status[2 * CHIP_MATCH_MAX_BATCH], slot[CHIP_MATCH_MAX_BATCH];
        uint64_t sd[2 * CHIP_MATCH_MAX_BATCH];
        double T[2 * CHIP_MATCH_MAX_BATCH * 16];
        float conf[2 * CHIP_MATCH_MAX_BATCH];
        int P = 0;
        for (int j = 0; j < B; j++) {
            slot[j] = -1;
            if (sm[j].n_matches_gms < 150) continue;
            composed[(size_t)j].pf_matches = sm[j].n_matches_gms;
            slot[j] = P;
            cand[P] = j; which[P] = CHIP_SET_AB; sd[P] = seeds[(size_t)j]; P++;
            cand[P] = j; which[P] = CHIP_SET_BA; sd[P] = seeds[(size_t)j] + 1; P++;
        }
        if (P > 0 && chip_pnp_ransac_matched_batch(ctx, P, cand, which, &pp, sd, T, conf, nullptr, nullptr, status) != CHIP_OK) return false;
        const auto t2 = now();
        for (int j = 0; j < B; j++) {
            if (slot[j] < 0) continue;
            const int k = slot[j];
            std::array<double, 16> op1{}, op2_a_T_b{}, op2{}, icp{};
            float g1 = -1.f, g2 = -1.f, g3 = -1.f;
            if (status[k] == CHIP_OK) { for (int i = 0; i < 16; i++) op1[i] = T[16 * k + i]; g1 = conf[k]; }
            if (status[k + 1] == CHIP_OK) { for (int i = 0; i < 16; i++) op2_a_T_b[i] = T[16 * (k + 1) + i]; g2 = conf[k + 1]; }
            matrix4_inverse_rigid(op2_a_T_b.data(), op2.data());
            pi.seed = seeds[(size_t)j] ^ 0x9E3779B97F4A7C15ull;
            if (chip_match_select(ctx, j) != CHIP_OK) return false;
            if (chip_icp_ransac_matched(ctx, &pi, icp.data(), &g3, nullptr, nullptr) != CHIP_OK) g3 = -1.f;
            bool nan = false;
            for (int i = 0; i < 16; i++)
                if (op1[i] != op1[i] || op2[i] != op2[i] || icp[i] != icp[i]) nan = true;
            if (nan || g1 < 0 || g2 < 0 || g3 < 0) continue;
            composed[(size_t)j].opX_b_T_a = {op1, op2, icp};
            composed[(size_t)j].opX_goodness = {g1, g2, g3};
            ok_composed[j] = true;
        }
        if (t) { t[0] = ms(t0, t1); t[1] = ms(t1, t2); t[2] = ms(t2, now()); }
        return true;
    };
    if (!run_stored() || !run_composed(nullptr)) { std::fprintf(stderr, "verify_candidates_composed: a library call failed\n"); return 1; }

    int differ = 0;
    for (int j = 0; j < B; j++) {
        const ProcessedLoopCandidate &p = stored[(size_t)j], &q = composed[(size_t)j];
        bool same = ok_stored[j] == ok_composed[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size();
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        std::printf("candidate %2d: pf_matches=%d  %s  %s\n", j, p.pf_matches, ok_stored[j] ? "three poses" : "rejected",
                    same ? "== the composition from single calls" : "DIFFERS from the composition from single calls");
        differ += !same;
    }
    bool expected = !ok_stored[B - 1] && !ok_stored[B - 2];
    for (int j = 0; j < B - 2 && n >= 2000; j++) expected = expected && ok_stored[j];
    if (!expected) std::printf("unexpected outcome: which candidates passed is not what the scene was built for\n");

    if (reps > 0) {
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        std::vector<double> ts, tc, part[3];
        for (int r = 0; r < reps; r++) {
            const auto t0 = now();
            run_stored();
            ts.push_back(ms(t0, now()));
        }
        for (int r = 0; r < reps; r++) {
            double t[3];
            const auto t0 = now();
            run_composed(t);
            tc.push_back(ms(t0, now()));
            for (int k = 0; k < 3; k++) part[k].push_back(t[k]);
        }
        std::printf("timing B=%d n=%d reps=%d: verify_candidates_stored %.3f ms, composed %.3f ms = match %.3f + pnp batch %.3f + icp loop %.3f (medians)\n",
                    B, m, reps, median(ts), median(tc), median(part[0]), median(part[1]), median(part[2]));
    }
    return differ == 0 && expected ? 0 : 1;
}
