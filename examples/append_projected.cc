// append_projected.cc -- the descriptor projection against a plain C++ restatement of its definition (include/cerebro_hip.h
// "descriptor projection"): the same raw descriptors, with planted revisits, go into two DBs -- one through
// chip_db_append_projected_f32, one through the restatement below followed by chip_db_append_f64 -- and every row read back and every
// tick record must have equal bits, for a float and for a double matrix.  With an argument it also times, at 32768 -> 4096: the two
// ways, chip_project, and the restatement alone (a plain loop on one host core; NOT numpy's order, see the header).
//   append_projected          compare (in_dim 512, D 256, 200 descriptors)
//   append_projected time     compare, then time
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
template <typename MT> static double dot_tree(const float *x, const MT *row, int n)
{
    constexpr int N = 16 / (int)sizeof(MT);   // elements per lane and chunk: 4 floats / 2 doubles
    double acc[64] = {0.0};
    for (int base = 0; base < n; base += 64 * N)
        for (int L = 0; L < 64; L++)
            for (int c = 0; c < N; c++) {
                const int e = base + N * L + c;
                acc[L] = std::fma((double)x[e], (double)row[e], acc[L]);   // float matrix: the product is exact, fma == multiply-then-add
            }
    return butterfly(acc);
}
template <typename MT> static void project_host(const float *x, const MT *Mt, const double *bias, int in_dim, int D, double *z)
{
    std::vector<double> y((size_t)D);
    for (int j = 0; j < D; j++) {
        const double t = dot_tree(x, Mt + (size_t)j * in_dim, in_dim);
        y[(size_t)j] = bias ? t + bias[j] : t;
    }
    double acc[64] = {0.0};
    for (int base = 0; base < D; base += 128)
        for (int L = 0; L < 64; L++)
            for (int c = 0; c < 2; c++) {
                const int e = base + 2 * L + c;
                if (e < D) acc[L] = std::fma(y[(size_t)e], y[(size_t)e], acc[L]);
            }
    const double r = std::sqrt(butterfly(acc));
    for (int j = 0; j < D; j++) z[j] = y[(size_t)j] / r;
}

#define CHK(call) do { const int _s = (call); if (_s != CHIP_OK) { std::printf("%s: status %d (%s)\n", #call, _s, chip_strerror(_s)); return 1; } } while (0)

template <typename MT> static int compare(int matrix_type, const char *name)
{
    const int in_dim = 512, D = 256, N = 200;
    std::vector<MT> Mt((size_t)D * in_dim);
    for (MT &v : Mt) v = (MT)uniform();
    std::vector<double> bias((size_t)D);
    for (double &v : bias) v = 0.1 * uniform();
    std::vector<float> raw((size_t)N * in_dim);
    for (float &v : raw) v = (float)uniform();
    for (int i = 80; i < N; i++)             // planted revisits: runs of six noisy copies of the descriptors 70 keyframes back
        if (i % 20 < 6)
            for (int e = 0; e < in_dim; e++) raw[(size_t)i * in_dim + e] = raw[(size_t)(i - 70) * in_dim + e] + 0.05f * (float)uniform();

    chip_ctx *a = nullptr, *b = nullptr;
    CHK(chip_create(&a, D, 0, 0, 0, 1));
    CHK(chip_create(&b, D, 0, 0, 0, 1));
    CHK(chip_project_set(a, in_dim, Mt.data(), matrix_type, bias.data()));
    std::vector<double> z((size_t)N * D);
    for (int i = 0; i < N; i++) project_host(raw.data() + (size_t)i * in_dim, Mt.data(), bias.data(), in_dim, D, z.data() + (size_t)i * D);
    int64_t first = -1;
    for (int i = 0; i < N; i += 50) {         // batches of 50, as a replay would send them
        CHK(chip_db_append_projected_f32(a, raw.data() + (size_t)i * in_dim, 50, 0, &first));
        if (first != i) { std::printf("%s: first_index %lld DIFFERS from %d\n", name, (long long)first, i); return 1; }
        CHK(chip_db_append_f64(b, z.data() + (size_t)i * D, 50, 0, &first));
    }
    chip_info ia, ib;
    CHK(chip_get_info(a, &ia));
    CHK(chip_get_info(b, &ib));
    int bad = 0;
    if (ia.storage_bytes != 8 || ib.storage_bytes != 8 || ia.rows_global != N || ib.rows_global != N) { std::printf("%s: storage / size DIFFERS\n", name); bad++; }
    std::vector<int64_t> rows((size_t)N);
    for (int i = 0; i < N; i++) rows[(size_t)i] = i;
    std::vector<double> ra((size_t)N * D), rb((size_t)N * D);
    CHK(chip_db_read_rows_f64(a, rows.data(), N, ra.data()));
    CHK(chip_db_read_rows_f64(b, rows.data(), N, rb.data()));
    for (int i = 0; i < N; i++)
        if (std::memcmp(ra.data() + (size_t)i * D, rb.data() + (size_t)i * D, (size_t)D * 8) != 0 ||
            std::memcmp(ra.data() + (size_t)i * D, z.data() + (size_t)i * D, (size_t)D * 8) != 0) { std::printf("%s: row %d DIFFERS\n", name, i); bad++; }
    chip_dot_params p;
    chip_dot_params_default(&p);
    int found = 0, scanned = 0;
    for (int l = 1; l <= N; l++) {
        chip_tick_result ta, tb;
        std::memset(&ta, 0, sizeof ta);
        std::memset(&tb, 0, sizeof tb);
        CHK(chip_loop_tick(a, l, &p, &ta));
        CHK(chip_loop_tick(b, l, &p, &tb));
        if (std::memcmp(&ta, &tb, sizeof ta) != 0) { std::printf("%s: tick %d DIFFERS\n", name, l); bad++; }
        found += ta.found;
        scanned += ta.status == CHIP_TICK_SCANNED;
    }
    if (found == 0) { std::printf("%s: no planted revisit was found: the comparison DIFFERS from what it is meant to be\n", name); bad++; }
    std::printf("%s matrix: %d rows and %d ticks (%d scanned, %d loop candidates) compared, %d differences\n", name, N, N, scanned, found, bad);
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

template <typename MT> static int time_it(int matrix_type, const char *name)
{
    const int in_dim = 32768, D = 4096;
    std::vector<MT> Mt((size_t)D * in_dim);
    for (MT &v : Mt) v = (MT)uniform();
    std::vector<double> bias((size_t)D);
    for (double &v : bias) v = 0.1 * uniform();
    std::vector<float> x((size_t)in_dim);
    for (float &v : x) v = (float)uniform();
    std::vector<double> z((size_t)D), zd((size_t)D);
    chip_ctx *c = nullptr;
    CHK(chip_create(&c, D, 0, 0, 0, 1));
    CHK(chip_project_set(c, in_dim, Mt.data(), matrix_type, bias.data()));
    int st = CHIP_OK;
    int64_t first;
    const double t_host = timed(3, [&] { project_host(x.data(), Mt.data(), bias.data(), in_dim, D, z.data()); });
    const double t_proj = timed(30, [&] { st |= chip_project(c, x.data(), 1, zd.data()); });
    const double t_app = timed(30, [&] { st |= chip_db_append_projected_f32(c, x.data(), 1, 0, &first); });
    const double t_f64 = timed(30, [&] { st |= chip_db_append_f64(c, z.data(), 1, 0, &first); });
    CHK(st);
    const bool same = std::memcmp(z.data(), zd.data(), (size_t)D * 8) == 0;
    std::printf("%s matrix, %d -> %d, medians: restatement on one host core %.1f ms | chip_project %.3f ms | chip_db_append_projected_f32 %.3f ms | "
                "chip_db_append_f64 of a ready row %.3f ms | device row %s the restatement\n", name, in_dim, D, t_host, t_proj, t_app, t_f64,
                same ? "equals" : "DIFFERS from");
    chip_destroy(c);
    return same ? 0 : 1;
}

int main(int argc, char **)
{
    if (chip_build_has_project() != 1) { std::printf("this build has no projection\n"); return 1; }
    int rc = compare<float>(CHIP_PROJ_F32, "float");
    rc |= compare<double>(CHIP_PROJ_F64, "double");
    if (argc > 1) {
        rc |= time_it<float>(CHIP_PROJ_F32, "float");
        rc |= time_it<double>(CHIP_PROJ_F64, "double");
    }
    return rc;
}
