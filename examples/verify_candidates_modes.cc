// examples/verify_candidates_modes.cc -- loop candidates seen under a ROLLED camera: GMS in its plain form
// (GetInlierMask(mask, false, false), the reference's call site) keeps nothing of such a candidate, so it never reaches PnP; with the
// scale / rotation variants (gms_modes = CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION) it does.  The query and the candidates are put
// into the frame store once, then verify_candidates_stored runs twice on the same ids: gms_modes = 0 and gms_modes = 3.
// No ROS, no Eigen, no OpenCV: libcerebro_host.so + libcerebro_hip.so only.
//
//   verify_candidates_modes [n_points]   default 3000.  Candidates: 0 an ordinary view, 1 the view ROLLED by 90 degrees about the optical
//                                        axis, 2 an ordinary view, 3 an unrelated frame.  Prints per candidate and mode the hypothesis
//                                        counts, the choice and the accept flag, and for the rolled candidate the largest deviation of
//                                        its PnP pose from the pose the scene was made with.  Exit code 0 iff the rolled candidate is
//                                        rejected with gms_modes = 0 and accepted with 3, the ordinary ones are accepted by both and the
//                                        unrelated one by neither.
#include <algorithm>
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
    const int B = 4, kRolled = 1;
    if (n < 2000 || n > CHIP_MATCH_MAX_KEYPOINTS) {
        std::fprintf(stderr, "usage: verify_candidates_modes [n_points in 2000..%d]\n", CHIP_MATCH_MAX_KEYPOINTS);
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

    // the candidates: views of the same cloud (4 % of the descriptor bits differ), one of them rolled, and an unrelated frame
    double R_rolled[9] = {}, t_rolled[3] = {};
    std::vector<Frame> cands((size_t)B);
    for (int j = 0; j < B; j++) {
        Frame &b = cands[(size_t)j];
        b.xyz.assign((size_t)W * H * 3, 0.f);
        if (j == B - 1) {                                                                 // unrelated
            for (int i = 0; i < m; i++) {
                b.kp.push_back((float)ux(rng)); b.kp.push_back((float)uy(rng));
                for (int k = 0; k < CHIP_ORB_DESC_BYTES; k++) b.desc.push_back((uint8_t)(rng() & 0xff));
            }
            continue;
        }
        const double yaw = (j % 2 ? -1.0 : 1.0) * (1.0 + j) * M_PI / 180.0, t[3] = {0.15 - 0.05 * j, 0.02, 0.05 + 0.02 * j};   // b_T_a
        const double roll = j == kRolled ? M_PI / 2 : 0.0, cy_ = std::cos(yaw), sy_ = std::sin(yaw), cr = std::cos(roll), sr = std::sin(roll);
        const double R[9] = {cy_ * cr, -cy_ * sr, sy_, sr, cr, 0.0, -sy_ * cr, sy_ * sr, cy_};   // Ry(yaw) . Rz(roll)
        if (j == kRolled) { std::memcpy(R_rolled, R, sizeof R); std::memcpy(t_rolled, t, sizeof t); }
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
    int rc = chip_frame_store_reserve(cer.ctx(), B + 1, m);
    if (rc == CHIP_OK) rc = chip_frame_put(cer.ctx(), 1000, &fa);
    std::vector<int64_t> ids;
    for (int j = 0; j < B && rc == CHIP_OK; j++) { ids.push_back(j); rc = chip_frame_put(cer.ctx(), j, &fb[(size_t)j]); }
    if (rc != CHIP_OK) { std::fprintf(stderr, "frame store -> %s\n", chip_strerror(rc)); return 1; }

    const uint32_t modes[2] = {0, CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION};
    bool ok[2][CHIP_MATCH_MAX_BATCH] = {};
    double rolled_err = -1.0;
    for (int k = 0; k < 2; k++) {
        std::vector<ProcessedLoopCandidate> pc((size_t)B);
        for (int j = 0; j < B; j++) { pc[(size_t)j].t_node_1 = Time{100, 0}; pc[(size_t)j].t_node_2 = Time{160 + (uint32_t)j, 0}; }
        chip_match_summary sm[CHIP_MATCH_MAX_BATCH] = {};
        chip_gms_choice ch[CHIP_MATCH_MAX_BATCH] = {};
        if (!verify_candidates_stored(cer.ctx(), 1000, ids.data(), B, Kinv, pc.data(), ok[k], seeds.data(), sm, modes[k], ch)) {
            std::fprintf(stderr, "verify_candidates_modes: a library call failed\n");
            return 1;
        }
        for (int j = 0; j < B; j++) {
            std::printf("gms_modes=%u candidate %d%s: matches_all=%d pf_matches=%d choice=(scale %d, rotation %d) accepted=%d counts=", modes[k], j,
                        j == kRolled ? " (rolled 90 deg)" : j == B - 1 ? " (unrelated)" : "", sm[j].n_matches_all, sm[j].n_matches_gms, ch[j].scale,
                        ch[j].rotation, ok[k][j] ? 1 : 0);
            for (int s = 0; s < 5; s++)
                for (int r = 0; r < 8; r++)
                    if (ch[j].counts[s][r] >= 0) std::printf("%s%d", s || r ? (r ? "," : " | ") : "", ch[j].counts[s][r]);
            std::printf("\n");
        }
        if (k == 1 && ok[1][kRolled]) {                      // op1 = b_T_a of the a -> b PnP (column-major) against the scene's pose
            const std::array<double, 16> &T = pc[(size_t)kRolled].opX_b_T_a[0];
            rolled_err = 0.0;
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) rolled_err = std::max(rolled_err, std::fabs(T[4 * c + r] - R_rolled[3 * r + c]));
                rolled_err = std::max(rolled_err, std::fabs(T[12 + r] - t_rolled[r]));
            }
        }
    }
    std::printf("rolled candidate: PnP pose deviates from the scene's pose by at most %.3e\n", rolled_err);
    const bool expected = !ok[0][kRolled] && ok[1][kRolled] && ok[0][0] && ok[1][0] && ok[0][2] && ok[1][2] && !ok[0][B - 1] && !ok[1][B - 1];
    std::printf("%s\n", expected ? "as expected: the rolled candidate is rejected with gms_modes=0 and accepted with gms_modes=3"
                                 : "UNEXPECTED outcome: which candidates passed is not what the scene was built for");
    return expected ? 0 : 1;
}
