// append_vlad.cc -- the NetVLAD pooling against a plain C++ restatement of its definition (include/cerebro_hip.h "NetVLAD pooling"):
// the same feature maps, with planted revisits, go into two DBs -- one through chip_db_append_vlad_f32, one through the restatement
// below followed by chip_db_append_f64 (direct route) or chip_db_append_projected_f32 (route through a projection) -- and every row read
// back and every tick record must have equal bits.  With an argument it also times the default model's shape (1410 x 512, K = 16,
// D = 8192): the pooled append, chip_vlad, chip_db_append_f64 of a ready row, and the restatement alone on one host core (NOT TF).
//   append_vlad          compare (direct: 130 x 64, K = 4 + 1 ghost, D 256; projected: 130 x 64, K = 8 -> 512 -> D 256; both layouts)
//   append_vlad time     compare, then time
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cerebro_hip.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform()   // (-1, 1)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(rng_state >> 11) / (double)(1ll << 52) - 1.0;
}

// ---- the definition, restated ------------------------------------------------------------------------------------------------
static double butterfly(double acc[64])
{
    for (int m = 32; m >= 1; m >>= 1) {
        double nxt[64];
        for (int L = 0; L < 64; L++) nxt[L] = acc[L] + acc[L ^ m];
        std::memcpy(acc, nxt, sizeof nxt);
    }
    return acc[0];
}
static double dot_tree_f32(const float *x, const float *row, int n)
{
    double acc[64] = {0.0};
    for (int base = 0; base < n; base += 256)
        for (int L = 0; L < 64; L++)
            for (int c = 0; c < 4; c++) {
                const int e = base + 4 * L + c;
                if (e < n) acc[L] = std::fma((double)x[e], (double)row[e], acc[L]);   // the product is exact: fma == multiply-then-add
            }
    return butterfly(acc);
}
static double dot_tree_f64(const double *x, const double *row, int n)
{
    double acc[64] = {0.0};
    for (int base = 0; base < n; base += 128)
        for (int L = 0; L < 64; L++)
            for (int c = 0; c < 2; c++) {
                const int e = base + 2 * L + c;
                if (e < n) acc[L] = std::fma(x[e], row[e], acc[L]);
            }
    return butterfly(acc);
}
static double vlad_exp(double t)
{
    const double LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
    if (t < -700.0) return 0.0;
    const double kf = std::nearbyint(t * LOG2E);   // the default rounding mode: ties to even
    const double r = (t - kf * LN2_HI) - kf * LN2_LO;
    double fact[14];
    fact[0] = 1.0;
    for (int i = 1; i < 14; i++) fact[i] = fact[i - 1] * (double)i;   // exact: 13! < 2^53
    double p = 1.0 / fact[13];
    for (int i = 12; i >= 0; i--) p = p * r + 1.0 / fact[i];
    const uint64_t bits = (uint64_t)(1023 + (int)kf) << 52;
    double scale;
    std::memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}
// x: N x C (n-major); Wt: (K+G) x C; bias: K+G; centres: K x C  ->  v: K*C floats
static void vlad_host(const float *x, int N, int C, int K, int G, const float *Wt, const float *bias, const float *centres, float *v)
{
    const int KG = K + G;
    std::vector<double> a((size_t)N * KG), s((size_t)KG), V((size_t)K * C, 0.0), A((size_t)K, 0.0), U((size_t)K * C);
    for (int n = 0; n < N; n++) {
        for (int k = 0; k < KG; k++) s[(size_t)k] = dot_tree_f32(x + (size_t)n * C, Wt + (size_t)k * C, C) + (double)bias[k];
        double m = s[0];
        for (int k = 1; k < KG; k++) if (s[(size_t)k] > m) m = s[(size_t)k];
        double Z = 0.0;
        for (int k = 0; k < KG; k++) { s[(size_t)k] = vlad_exp(s[(size_t)k] - m); Z = Z + s[(size_t)k]; }
        for (int k = 0; k < KG; k++) a[(size_t)n * KG + k] = s[(size_t)k] / Z;
    }
    for (int n0 = 0; n0 < N; n0 += CHIP_VLAD_BLOCK) {
        const int n1 = n0 + CHIP_VLAD_BLOCK < N ? n0 + CHIP_VLAD_BLOCK : N;
        for (int k = 0; k < K; k++) {
            double S = 0.0;
            for (int n = n0; n < n1; n++) S = S + a[(size_t)n * KG + k];
            A[(size_t)k] = A[(size_t)k] + S;
            for (int c = 0; c < C; c++) {
                double P = 0.0;
                for (int n = n0; n < n1; n++) P = P + (a[(size_t)n * KG + k] * (double)x[(size_t)n * C + c]);
                V[(size_t)k * C + c] = V[(size_t)k * C + c] + P;
            }
        }
    }
    for (int k = 0; k < K; k++) {
        double *w = U.data() + (size_t)k * C;
        for (int c = 0; c < C; c++) w[c] = V[(size_t)k * C + c] + (A[(size_t)k] * (double)centres[(size_t)k * C + c]);
        const double q = dot_tree_f64(w, w, C);
        const double r = std::sqrt(q > 1e-12 ? q : 1e-12);
        for (int c = 0; c < C; c++) w[c] = w[c] / r;
    }
    const double q = dot_tree_f64(U.data(), U.data(), K * C);
    const double r = std::sqrt(q > 1e-12 ? q : 1e-12);
    for (int e = 0; e < K * C; e++) v[e] = (float)(U[(size_t)e] / r);
}

#define CHK(call) do { const int _s = (call); if (_s != CHIP_OK) { std::printf("%s: status %d (%s)\n", #call, _s, chip_strerror(_s)); return 1; } } while (0)

struct Model {
    int C, K, G;
    std::vector<float> Wt, bias, centres;
    Model(int C_, int K_, int G_) : C(C_), K(K_), G(G_), Wt((size_t)(K_ + G_) * C_), bias((size_t)(K_ + G_)), centres((size_t)K_ * C_)
    {
        for (float &v : Wt) v = (float)uniform();
        for (float &v : bias) v = (float)(0.5 * uniform());
        for (float &v : centres) v = (float)(0.3 * uniform());
    }
};

// M maps of N positions, a post-ReLU look (half the values zero), with planted revisits: runs of six noisy copies of the maps 30 back
static std::vector<float> make_maps(int M, int N, int C)
{
    const size_t sz = (size_t)N * C;
    std::vector<float> maps((size_t)M * sz);
    for (float &v : maps) { const double u = uniform(); v = u > 0 ? (float)u : 0.f; }
    for (int i = 40; i < M; i++)
        if (i % 10 < 6)
            for (size_t e = 0; e < sz; e++) {
                const float base = maps[(size_t)(i - 30) * sz + e];
                maps[(size_t)i * sz + e] = base > 0 ? base + 0.02f * (float)uniform() : 0.f;
            }
    return maps;
}

static int compare(bool projected, const char *name)
{
    const int N = 130, D = 256, M = 80, in_dim = 512;
    const Model mdl = projected ? Model(64, 8, 0) : Model(64, 4, 1);
    const int C = mdl.C, KC = mdl.K * C;
    const std::vector<float> maps = make_maps(M, N, C);
    std::vector<float> Mt;
    chip_ctx *a = nullptr, *b = nullptr;
    CHK(chip_create(&a, D, 0, 0, 0, 1));
    CHK(chip_create(&b, D, 0, 0, 0, 1));
    CHK(chip_vlad_set(a, C, mdl.K, mdl.G, mdl.Wt.data(), mdl.bias.data(), mdl.centres.data()));
    if (projected) {
        Mt.resize((size_t)D * in_dim);
        for (float &v : Mt) v = (float)uniform();
        CHK(chip_project_set(a, in_dim, Mt.data(), CHIP_PROJ_F32, nullptr));
        CHK(chip_project_set(b, in_dim, Mt.data(), CHIP_PROJ_F32, nullptr));
    }
    int bad = 0;
    int64_t first = -1;
    std::vector<float> v((size_t)KC), t((size_t)N * C);
    std::vector<double> vd((size_t)KC);
    for (int i = 0; i < M; i++) {
        const float *map = maps.data() + (size_t)i * N * C;
        vlad_host(map, N, C, mdl.K, mdl.G, mdl.Wt.data(), mdl.bias.data(), mdl.centres.data(), v.data());
        if (i & 1) {   // every other map goes in as a torch trunk would hand it over: channels first
            for (int n = 0; n < N; n++)
                for (int c = 0; c < C; c++) t[(size_t)c * N + n] = map[(size_t)n * C + c];
            CHK(chip_db_append_vlad_f32(a, t.data(), N, CHIP_VLAD_NCHW, 0, &first));
        } else {
            CHK(chip_db_append_vlad_f32(a, map, N, CHIP_VLAD_NHWC, 0, &first));
        }
        if (first != i) { std::printf("%s: first_index %lld DIFFERS from %d\n", name, (long long)first, i); return 1; }
        if (projected) {
            CHK(chip_db_append_projected_f32(b, v.data(), 1, 0, &first));
        } else {
            for (int e = 0; e < KC; e++) vd[(size_t)e] = (double)v[(size_t)e];
            CHK(chip_db_append_f64(b, vd.data(), 1, 0, &first));
        }
    }
    chip_info ia, ib;
    CHK(chip_get_info(a, &ia));
    CHK(chip_get_info(b, &ib));
    if (ia.storage_bytes != ib.storage_bytes || ia.rows_global != M || ib.rows_global != M) { std::printf("%s: storage / size DIFFERS\n", name); bad++; }
    std::vector<int64_t> rows((size_t)M);
    for (int i = 0; i < M; i++) rows[(size_t)i] = i;
    std::vector<double> ra((size_t)M * D), rb((size_t)M * D);
    CHK(chip_db_read_rows_f64(a, rows.data(), M, ra.data()));
    CHK(chip_db_read_rows_f64(b, rows.data(), M, rb.data()));
    for (int i = 0; i < M; i++)
        if (std::memcmp(ra.data() + (size_t)i * D, rb.data() + (size_t)i * D, (size_t)D * 8) != 0) { std::printf("%s: row %d DIFFERS\n", name, i); bad++; }
    chip_dot_params p;
    chip_dot_params_default(&p);
    int found = 0, scanned = 0;
    for (int l = 1; l <= M; l++) {
        chip_tick_result ta, tb;
        std::memset(&ta, 0, sizeof ta);
        std::memset(&tb, 0, sizeof tb);
        CHK(chip_loop_tick(a, l, &p, &ta));
        CHK(chip_loop_tick(b, l, &p, &tb));
        if (std::memcmp(&ta, &tb, sizeof ta) != 0) { std::printf("%s: tick %d DIFFERS\n", name, l); bad++; }
        found += ta.found;
        scanned += ta.status == CHIP_TICK_SCANNED;
    }
    std::printf("%s route: %d rows and %d ticks (%d scanned, %d loop candidates) compared, %d differences\n", name, M, M, scanned, found, bad);
    chip_destroy(a);
    chip_destroy(b);
    return bad ? 1 : 0;
}

static double median_ms(std::vector<double> &v)
{
    for (size_t i = 1; i < v.size(); i++)
        for (size_t j = i; j > 0 && v[j] < v[j - 1]; j--) { const double t = v[j]; v[j] = v[j - 1]; v[j - 1] = t; }
    return v[v.size() / 2];
}
template <typename F> static double timed(int reps, F f)
{
    std::vector<double> ms;
    for (int r = 0; r < reps + 2; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 2) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());   // two warm-up calls
    }
    return median_ms(ms);
}

static int time_it()
{
    const int N = 1410, D = 8192;
    const Model mdl(512, 16, 0);
    const std::vector<float> map = make_maps(1, N, mdl.C);
    std::vector<float> v((size_t)D), vdev((size_t)D);
    std::vector<double> vd((size_t)D);
    chip_ctx *c = nullptr;
    CHK(chip_create(&c, D, 0, 0, 0, 1));
    CHK(chip_vlad_set(c, mdl.C, mdl.K, mdl.G, mdl.Wt.data(), mdl.bias.data(), mdl.centres.data()));
    int st = CHIP_OK;
    int64_t first;
    const double t_host = timed(3, [&] { vlad_host(map.data(), N, mdl.C, mdl.K, mdl.G, mdl.Wt.data(), mdl.bias.data(), mdl.centres.data(), v.data()); });
    for (int e = 0; e < D; e++) vd[(size_t)e] = (double)v[(size_t)e];
    const double t_vlad = timed(30, [&] { st |= chip_vlad(c, map.data(), N, CHIP_VLAD_NHWC, vdev.data()); });
    const double t_app = timed(30, [&] { st |= chip_db_append_vlad_f32(c, map.data(), N, CHIP_VLAD_NHWC, 0, &first); });
    const double t_f64 = timed(30, [&] { st |= chip_db_append_f64(c, vd.data(), 1, 0, &first); });
    CHK(st);
    const bool same = std::memcmp(v.data(), vdev.data(), (size_t)D * 4) == 0;
    std::printf("%d x %d, K = %d -> %d, medians: restatement on one host core (not TF) %.1f ms | chip_vlad %.3f ms | chip_db_append_vlad_f32 %.3f ms | "
                "chip_db_append_f64 of a ready row %.3f ms | device vector %s the restatement\n", N, mdl.C, mdl.K, D, t_host, t_vlad, t_app, t_f64,
                same ? "equals" : "DIFFERS from");
    chip_destroy(c);
    return same ? 0 : 1;
}

int main(int argc, char **)
{
    if (chip_build_has_vlad() != 1) { std::printf("this build has no pooling\n"); return 1; }
    int rc = compare(false, "direct");
    rc |= compare(true, "projected");
    if (argc > 1) rc |= time_it();
    return rc;
}
