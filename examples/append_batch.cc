// append_batch.cc -- batched ingest against the loop of single calls (include/cerebro_hip.h "batched ingest"): the same feature maps, with
// planted revisits, go into two DBs -- one through ONE chip_db_append_vlad_batch_f32, one through chip_db_append_vlad_f32 map by map --
// on the two routes of append_vlad.cc at the shapes of the reference's models: K = 16 straight to 8192-D, and K = 64 through a
// projection (32768 -> D).  Every row read back and every tick record over both DBs must have equal bits.  With an argument it also
// times both ways of filling, at 16 maps per call.
//   append_batch          compare (direct: 65 x 512, K = 16, D 8192; projected: 65 x 512, K = 64 -> 32768 -> D 256; both layouts)
//   append_batch time     compare, then time (direct: 1410 x 512; projected: 540 x 512 -> 32768 -> D 4096)
#include <chrono>
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

#define CHK(call) do { const int _s = (call); if (_s != CHIP_OK) { std::printf("%s: status %d (%s)\n", #call, _s, chip_strerror(_s)); return 1; } } while (0)

struct Model {
    int C, K, G;
    std::vector<float> Wt, bias, centres;
    Model(int C_, int K_, int G_) : C(C_), K(K_), G(G_), Wt((size_t)(K_ + G_) * C_), bias((size_t)(K_ + G_)), centres((size_t)K_ * C_)
    {
        for (float &v : Wt) v = (float)(uniform() * 0.1);
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

// channels first, map by map: what a torch trunk hands over as [B, C, H, W]
static std::vector<float> channels_first(const std::vector<float> &maps, int M, int N, int C)
{
    std::vector<float> t(maps.size());
    for (int m = 0; m < M; m++)
        for (int n = 0; n < N; n++)
            for (int c = 0; c < C; c++) t[((size_t)m * C + c) * N + n] = maps[((size_t)m * N + n) * C + c];
    return t;
}

static int set_up(chip_ctx *c, const Model &mdl, const std::vector<float> &Mt, int in_dim)
{
    CHK(chip_vlad_set(c, mdl.C, mdl.K, mdl.G, mdl.Wt.data(), mdl.bias.data(), mdl.centres.data()));
    if (!Mt.empty()) CHK(chip_project_set(c, in_dim, Mt.data(), CHIP_PROJ_F32, nullptr));
    return 0;
}

static int compare(bool projected, const char *name)
{
    const int N = 65, M = 61, C = 512;
    const Model mdl(C, projected ? 64 : 16, 0);
    const int KC = mdl.K * C, D = projected ? 256 : KC;
    const std::vector<float> maps = make_maps(M, N, C), maps_t = channels_first(maps, M, N, C);
    std::vector<float> Mt;
    if (projected) {
        Mt.resize((size_t)D * KC);
        for (float &v : Mt) v = (float)uniform();
    }
    chip_ctx *a = nullptr, *b = nullptr;
    CHK(chip_create(&a, D, 0, 0, 0, 1));
    CHK(chip_create(&b, D, 0, 0, 0, 1));
    if (set_up(a, mdl, Mt, KC) || set_up(b, mdl, Mt, KC)) return 1;
    int bad = 0;
    int64_t first = -1;
    // a: two batched calls, one per layout (40 maps as they lie, 21 channels first); b: the loop of single calls
    const int M0 = 40;
    CHK(chip_db_append_vlad_batch_f32(a, maps.data(), M0, N, CHIP_VLAD_NHWC, 0, &first));
    if (first != 0) { std::printf("%s: first_index %lld DIFFERS from 0\n", name, (long long)first); bad++; }
    CHK(chip_db_append_vlad_batch_f32(a, maps_t.data() + (size_t)M0 * N * C, M - M0, N, CHIP_VLAD_NCHW, 0, &first));
    if (first != M0) { std::printf("%s: first_index %lld DIFFERS from %d\n", name, (long long)first, M0); bad++; }
    if (projected) {
        int64_t passes[2], descs[2];
        int32_t width = 0;
        CHK(chip_debug_project_last(a, passes, descs, &width));
        chip_project_plan_out plan;
        CHK(chip_project_plan(KC, CHIP_PROJ_F32, M - M0, &plan));
        if (passes[0] != plan.shared_passes || passes[1] != plan.single_launches || descs[0] + descs[1] != M - M0) {
            std::printf("%s: the launches of the last call DIFFER from the plan\n", name);
            bad++;
        }
        std::printf("%s route: %d maps read the matrix %lld times (width %d)\n", name, M - M0, (long long)(passes[0] + passes[1]), width);
    }
    for (int i = 0; i < M; i++) {
        CHK(chip_db_append_vlad_f32(b, maps.data() + (size_t)i * N * C, N, CHIP_VLAD_NHWC, 0, &first));
        if (first != i) { std::printf("%s: first_index %lld DIFFERS from %d\n", name, (long long)first, i); return 1; }
    }
    chip_info ia, ib;
    CHK(chip_get_info(a, &ia));
    CHK(chip_get_info(b, &ib));
    if (ia.storage_bytes != ib.storage_bytes || ia.rows_global != M || ib.rows_global != M || ia.lossy_rows != ib.lossy_rows ||
        std::memcmp(&ia.row_norm_max, &ib.row_norm_max, sizeof ia.row_norm_max) != 0) {
        std::printf("%s: storage / size / norm DIFFERS\n", name);
        bad++;
    }
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

static int time_it(bool projected, const char *name)
{
    const int B = 16, C = 512, N = projected ? 540 : 1410;
    const Model mdl(C, projected ? 64 : 16, 0);
    const int KC = mdl.K * C, D = projected ? 4096 : KC;
    const std::vector<float> maps = make_maps(B, N, C);
    std::vector<float> Mt;
    if (projected) {
        Mt.resize((size_t)D * KC);
        for (float &v : Mt) v = (float)uniform();
    }
    chip_ctx *c = nullptr;
    CHK(chip_create(&c, D, 0, 0, 0, 1));
    if (set_up(c, mdl, Mt, KC)) return 1;
    int st = CHIP_OK;
    int64_t first;
    const double t_batch = timed(30, [&] { st |= chip_db_append_vlad_batch_f32(c, maps.data(), B, N, CHIP_VLAD_NHWC, 0, &first); });
    const double t_loop = timed(30, [&] {
        for (int i = 0; i < B; i++) st |= chip_db_append_vlad_f32(c, maps.data() + (size_t)i * N * C, N, CHIP_VLAD_NHWC, 0, &first);
    });
    CHK(st);
    std::printf("%s route, %d maps of %d x %d, K = %d -> D %d, medians of 30: one batched call %.3f ms | the loop of single calls %.3f ms\n", name, B, N, C,
                mdl.K, D, t_batch, t_loop);
    chip_destroy(c);
    return 0;
}

int main(int argc, char **)
{
    if (chip_build_has_vlad() != 1 || chip_build_has_project() != 1) { std::printf("this build has no pooling or no projection\n"); return 1; }
    int rc = compare(false, "direct");
    rc |= compare(true, "projected");
    if (argc > 1) {
        rc |= time_it(false, "direct");
        rc |= time_it(true, "projected");
    }
    return rc;
}
