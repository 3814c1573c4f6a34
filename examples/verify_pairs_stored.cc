// examples/verify_pairs_stored.cc -- a backlog of the loop-candidate consumer thread (src/Cerebro.cpp:1224-1232: foundLoops[prev .. new),
// every entry a pair (t_curr, t_prev) with a current frame of its own) verified in ONE call: the frames are put
// once, then verify_pairs_stored (chip_match_pairs_stored + one matched ICP batch underneath one matched PnP batch) runs against the
// loop it replaces, verify_candidates_stored with B = 1 per pair.  Both must give the same bits.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   verify_pairs_stored [n_points] [P] [reps]   defaults 3000, 6, 0.  P places, each with a query frame of its own (another cloud, another
//                                        keypoint count) and a second view of it; the last two pairs are an unrelated pair and a pair
//                                        with an empty candidate.  Prints one line per pair; exit code 0 iff both paths agree in every
//                                        pose, goodness, accept flag, summary and GMS choice.  With reps > 0 both are then timed (median
//                                        of reps runs), and each is also run as its match calls, its PnP calls and its ICP calls apart.
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
    const int P = argc > 2 ? std::atoi(argv[2]) : 6;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
    if (n < 1 || n > CHIP_MATCH_MAX_KEYPOINTS || P < 3 || P > CHIP_MATCH_MAX_PAIRS || reps < 0) {
        std::fprintf(stderr, "usage: verify_pairs_stored [n_points in 1..%d] [P in 3..%d] [reps >= 0]\n", CHIP_MATCH_MAX_KEYPOINTS, CHIP_MATCH_MAX_PAIRS);
        return 2;
    }
    const int W = 752, H = 480;
    const double f = 458.0, cx = W / 2.0, cy = H / 2.0;
    const double Kinv[9] = {1.0 / f, 0.0, -cx / f, 0.0, 1.0 / f, -cy / f, 0.0, 0.0, 1.0};

    // P places: query view k (one 3-D point per keypoint pixel, as the CV_32FC3 3-D image stores it; the later the place, the fewer
    // keypoints) and a second view of the same cloud (4 % of the descriptor bits differ)
    std::mt19937_64 rng(42);
    std::uniform_real_distribution<double> ux(1.0, W - 2.0), uy(1.0, H - 2.0), uz(3.0, 12.0), u01(0.0, 1.0);
    std::vector<Frame> qs((size_t)P), cs((size_t)P);
    for (int k = 0; k < P; k++) {
        Frame &a = qs[(size_t)k], &b = cs[(size_t)k];
        a.xyz.assign((size_t)W * H * 3, 0.f);
        b.xyz.assign((size_t)W * H * 3, 0.f);
        const int want = std::max(1, n - (n / 20) * k);
        std::vector<float> Xa;
        std::vector<uint8_t> taken((size_t)W * H, 0);
        for (int i = 0; i < want; i++) {
            const float u = (float)ux(rng), v = (float)uy(rng);
            const double z = uz(rng);
            const size_t px = (size_t)(int)v * W + (size_t)(int)u;
            if (taken[px]) continue;
            taken[px] = 1;
            const float X[3] = {(float)(z * ((double)u - cx) / f), (float)(z * ((double)v - cy) / f), (float)z};
            for (int r = 0; r < 3; r++) { a.xyz[3 * px + r] = X[r]; Xa.push_back(X[r]); }
            a.kp.push_back(u); a.kp.push_back(v);
            for (int d = 0; d < CHIP_ORB_DESC_BYTES; d++) a.desc.push_back((uint8_t)(rng() & 0xff));
        }
        const int m = (int)(a.kp.size() / 2);
        const double yaw = (k % 2 ? -1.0 : 1.0) * (1.0 + k % 5) * M_PI / 180.0, t[3] = {0.15 - 0.05 * (k % 5), 0.02, 0.05 + 0.02 * (k % 5)};   // b_T_a
        const double R[9] = {std::cos(yaw), 0.0, std::sin(yaw), 0.0, 1.0, 0.0, -std::sin(yaw), 0.0, std::cos(yaw)};
        std::fill(taken.begin(), taken.end(), 0);
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
            for (int d = 0; d < CHIP_ORB_DESC_BYTES; d++) {
                uint8_t flip = 0;
                for (int bit = 0; bit < 8; bit++) flip |= (uint8_t)((u01(rng) < 0.04) << bit);
                b.desc.push_back(a.desc[(size_t)i * CHIP_ORB_DESC_BYTES + d] ^ flip);
            }
        }
    }
    Frame empty;
    empty.xyz.assign((size_t)W * H * 3, 0.f);

    Cerebro cer(4096);
    if (!cer.ok()) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(cer.last_status())); return 2; }
    // keyframe arrival: every frame is put once; the ids are the integrator's (here 1000 + k for query k, k for its second view, -1 empty)
    int rc = chip_frame_store_reserve(cer.ctx(), 2 * P + 1, (int32_t)(qs[0].kp.size() / 2));
    for (int k = 0; k < P && rc == CHIP_OK; k++) {
        const chip_match_frame fa = qs[(size_t)k].view(W, H), fb = cs[(size_t)k].view(W, H);
        rc = chip_frame_put(cer.ctx(), 1000 + k, &fa);
        if (rc == CHIP_OK) rc = chip_frame_put(cer.ctx(), k, &fb);
    }
    if (rc == CHIP_OK) { const chip_match_frame fe = empty.view(W, H); rc = chip_frame_put(cer.ctx(), -1, &fe); }
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }
    // the backlog: pair k = (query k, its second view), but the last two: an unrelated pair and an empty candidate
    std::vector<int64_t> a_ids, b_ids;
    std::vector<uint64_t> seeds;
    for (int k = 0; k < P; k++) {
        a_ids.push_back(1000 + k);
        b_ids.push_back(k == P - 1 ? -1 : k == P - 2 ? 0 : k);
        seeds.push_back(7 + 10 * (uint64_t)k);
    }

    const auto fresh = [&](std::vector<ProcessedLoopCandidate> &pc) {
        pc.assign((size_t)P, ProcessedLoopCandidate());
        for (int j = 0; j < P; j++) { pc[(size_t)j].t_node_1 = Time{100 + (uint32_t)j, 0}; pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
    };
    std::vector<ProcessedLoopCandidate> listed, looped;
    bool ok_listed[CHIP_MATCH_MAX_PAIRS] = {}, ok_looped[CHIP_MATCH_MAX_PAIRS] = {};
    chip_match_summary sm_listed[CHIP_MATCH_MAX_PAIRS] = {}, sm_looped[CHIP_MATCH_MAX_PAIRS] = {};
    chip_gms_choice ch_listed[CHIP_MATCH_MAX_PAIRS] = {}, ch_looped[CHIP_MATCH_MAX_PAIRS] = {};
    const auto run_listed = [&] {
        fresh(listed);
        return verify_pairs_stored(cer.ctx(), a_ids.data(), b_ids.data(), P, Kinv, listed.data(), ok_listed, seeds.data(), sm_listed, 0, ch_listed);
    };
    const auto run_looped = [&] {
        fresh(looped);
        for (int j = 0; j < P; j++)
            if (!verify_candidates_stored(cer.ctx(), a_ids[(size_t)j], &b_ids[(size_t)j], 1, Kinv, &looped[(size_t)j], &ok_looped[j], &seeds[(size_t)j],
                                          &sm_looped[j], 0, &ch_looped[j]))
                return false;
        return true;
    };
    if (!run_listed() || !run_looped()) { std::fprintf(stderr, "verify_pairs_stored: a library call failed\n"); return 1; }

    int differ = 0;
    for (int j = 0; j < P; j++) {
        const ProcessedLoopCandidate &p = listed[(size_t)j], &q = looped[(size_t)j];
        bool same = ok_listed[j] == ok_looped[j] && p.pf_matches == q.pf_matches && p.opX_b_T_a.size() == q.opX_b_T_a.size() &&
                    p.opX_goodness.size() == q.opX_goodness.size() && std::memcmp(&sm_listed[j], &sm_looped[j], sizeof(chip_match_summary)) == 0 &&
                    std::memcmp(&ch_listed[j], &ch_looped[j], sizeof(chip_gms_choice)) == 0;
        for (size_t k = 0; same && k < p.opX_b_T_a.size(); k++)
            same = std::memcmp(p.opX_b_T_a[k].data(), q.opX_b_T_a[k].data(), 16 * sizeof(double)) == 0 &&
                   std::memcmp(&p.opX_goodness[k], &q.opX_goodness[k], sizeof(float)) == 0;
        std::printf("pair %2d (%lld, %lld): n1=%d gms=%d  %s  %s\n", j, (long long)a_ids[(size_t)j], (long long)b_ids[(size_t)j], sm_listed[j].n_matches_all,
                    sm_listed[j].n_matches_gms, ok_listed[j] ? "three poses" : "rejected",
                    same ? "== verify_candidates_stored with B = 1" : "DIFFERS from verify_candidates_stored with B = 1");
        differ += !same;
    }
    bool expected = !ok_listed[P - 1] && !ok_listed[P - 2];
    for (int j = 0; j < P - 2 && n >= 2000; j++) expected = expected && ok_listed[j];
    if (!expected) std::printf("unexpected outcome: which pairs passed is not what the scene was built for\n");

    if (reps > 0) {
        const auto now = [] { return std::chrono::steady_clock::now(); };
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto median = [](std::vector<double> t) { std::sort(t.begin(), t.end()); return t[t.size() / 2]; };
        // the stages apart, blocking, on the pairs [first, first + count): one match call (the pair list, or with count == 1 the batch
        // of one it replaces), one matched PnP batch and one matched ICP batch over the survivors; t[0..2] accumulate their wall time
        const auto stages = [&](int first, int count, double *t) {
            chip_ctx *ctx = cer.ctx();
            chip_match_summary sm[CHIP_MATCH_MAX_PAIRS] = {};
            const auto t0 = now();
            const int mrc = count == 1 ? chip_match_batch_stored(ctx, a_ids[(size_t)first], &b_ids[(size_t)first], 1, Kinv, sm)
                                       : chip_match_pairs_stored(ctx, &a_ids[(size_t)first], &b_ids[(size_t)first], count, Kinv, 0, sm, nullptr);
            if (mrc != CHIP_OK) return false;
            const auto t1 = now();
            chip_ransac_params pp, pi;
            chip_ransac_params_default(&pp);
            chip_icp_params_default(&pi);
            int32_t cand[2 * CHIP_MATCH_MAX_PAIRS], which[2 * CHIP_MATCH_MAX_PAIRS], status[2 * CHIP_MATCH_MAX_PAIRS], icp_cand[CHIP_MATCH_MAX_PAIRS];
            uint64_t sd[2 * CHIP_MATCH_MAX_PAIRS], icp_sd[CHIP_MATCH_MAX_PAIRS];
            double T[2 * CHIP_MATCH_MAX_PAIRS * 16];
            float conf[2 * CHIP_MATCH_MAX_PAIRS];
            int N = 0, Q = 0;
            for (int j = 0; j < count; j++) {
                if (sm[j].n_matches_gms < 150) continue;
                const uint64_t s0 = seeds[(size_t)(first + j)];
                cand[N] = j; which[N] = CHIP_SET_AB; sd[N] = s0; N++;
                cand[N] = j; which[N] = CHIP_SET_BA; sd[N] = s0 + 1; N++;
                icp_cand[Q] = j; icp_sd[Q] = s0 ^ 0x9E3779B97F4A7C15ull; Q++;
            }
            if (N > 0 && chip_pnp_ransac_matched_batch(ctx, N, cand, which, &pp, sd, T, conf, nullptr, nullptr, status) != CHIP_OK) return false;
            const auto t2 = now();
            if (Q > 0 && chip_icp_ransac_matched_batch(ctx, Q, icp_cand, &pi, icp_sd, T, conf, nullptr, nullptr, status) != CHIP_OK) return false;
            t[0] += ms(t0, t1); t[1] += ms(t1, t2); t[2] += ms(t2, now());
            return true;
        };
        std::vector<double> tl, to, pl[3], po[3];
        for (int r = 0; r < reps; r++) {                     // the variants alternate
            auto t0 = now();
            run_listed();
            tl.push_back(ms(t0, now()));
            t0 = now();
            run_looped();
            to.push_back(ms(t0, now()));
            double a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
            if (!stages(0, P, a)) return 1;
            for (int j = 0; j < P; j++)
                if (!stages(j, 1, b)) return 1;
            for (int k = 0; k < 3; k++) { pl[k].push_back(a[k]); po[k].push_back(b[k]); }
        }
        std::printf("timing P=%d n=%d reps=%d (medians, ms): verify_pairs_stored %.3f, loop of verify_candidates_stored(B=1) %.3f, ratio %.2f\n", P,
                    (int)(qs[0].kp.size() / 2), reps, median(tl), median(to), median(to) / median(tl));
        std::printf("stages apart, blocking: pair list = match %.3f + pnp batch %.3f + icp batch %.3f; loop = match %.3f + pnp %.3f + icp %.3f\n",
                    median(pl[0]), median(pl[1]), median(pl[2]), median(po[0]), median(po[1]), median(po[2]));
    }
    return differ == 0 && expected ? 0 : 1;
}
