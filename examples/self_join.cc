// self_join.cc -- the causal self-join of a DB in ONE call (include/cerebro_hip.h "a prefix PER QUERY") against the loop of single
// queries: a 256-D x 3000-row DB of unit rows with planted revisits; row i searches rows [0, i - 50) for its 5 best matches.
//   one call : chip_query_batch_rows_f32 over all 3000 rows (the queries are gathered from the DB on the device)
//   the loop : rows read back with chip_db_read_rows_f32, then chip_query_batch_f32 with Q = 1 per row
// Every score and every index must have equal bits.  With an argument it also times both.
//   self_join          compare
//   self_join time     compare, then time
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cerebro_hip.h"

#define CHK(call) do { const int _s = (call); if (_s != CHIP_OK) { std::printf("%s: status %d (%s)\n", #call, _s, chip_strerror(_s)); return 1; } } while (0)

int main(int argc, char **)
{
    if (chip_build_has_query_prefix() != 1) { std::printf("this build has no prefix-per-query mode\n"); return 1; }
    const int D = 256, N = 3000, LAG = 50, K = 5;
    // planted revisits: from row 400 on, runs of six rows are noisy copies of the (unplanted) rows 310 back
    std::vector<int64_t> dst, src;
    std::vector<int32_t> kind;
    for (int i = 400; i < N; i++)
        if (i % 20 < 6) { dst.push_back(i); src.push_back(i - 310); kind.push_back(1); }
    chip_ctx *c = nullptr;
    CHK(chip_create(&c, D, 0, 0, 0, 1));
    CHK(chip_db_append_synthetic_unit(c, N, 2024, dst.data(), src.data(), kind.data(), (int64_t)dst.size()));

    std::vector<int64_t> rows((size_t)N), k((size_t)N);
    for (int i = 0; i < N; i++) { rows[(size_t)i] = i; k[(size_t)i] = i > LAG ? i - LAG : 0; }
    std::vector<float> s_join((size_t)N * K), s_loop((size_t)N * K), q((size_t)N * D);
    std::vector<int64_t> i_join((size_t)N * K), i_loop((size_t)N * K);
    CHK(chip_query_batch_rows_f32(c, rows.data(), k.data(), N, K, s_join.data(), i_join.data()));
    chip_query_prefix_last last;
    CHK(chip_debug_query_prefix_last(c, &last));
    chip_query_prefix_plan_out plan;
    CHK(chip_query_prefix_plan(k.data(), N, 4, K, nullptr, &plan));

    CHK(chip_db_read_rows_f32(c, rows.data(), N, q.data()));
    auto loop = [&]() -> int {
        for (int i = 0; i < N; i++)
            CHK(chip_query_batch_f32(c, k[(size_t)i], q.data() + (size_t)i * D, 1, K, s_loop.data() + (size_t)i * K, i_loop.data() + (size_t)i * K));
        return 0;
    };
    if (loop()) return 1;
    int bad = 0, revisits = 0;
    for (int i = 0; i < N; i++) {
        if (std::memcmp(s_join.data() + (size_t)i * K, s_loop.data() + (size_t)i * K, sizeof(float) * K) != 0 ||
            std::memcmp(i_join.data() + (size_t)i * K, i_loop.data() + (size_t)i * K, sizeof(int64_t) * K) != 0) {
            if (bad++ < 5) std::printf("row %d DIFFERS: best %lld (%.9g) against %lld (%.9g)\n", i, (long long)i_join[(size_t)i * K], s_join[(size_t)i * K],
                                       (long long)i_loop[(size_t)i * K], s_loop[(size_t)i * K]);
        }
        revisits += i >= 400 && i % 20 < 6 && i_join[(size_t)i * K] == i - 310;
    }
    std::printf("%d rows, %d groups, %d launches, %d host waits; DB tiles walked %lld (planned %lld, one prefix for all: %lld); %d of %d planted revisits on top\n",
                N, last.groups, last.launches, last.waits, (long long)last.units_claimed, (long long)plan.units, (long long)plan.units_rect, revisits,
                (int)dst.size());
    if (last.units_claimed != plan.units || last.units_planned != plan.units) { std::printf("the tiles walked DIFFER from the plan\n"); bad++; }
    if (bad) { std::printf("%d differences\n", bad); return 1; }
    std::printf("%d lists of %d compared with the loop of single queries: all equal\n", N, K);

    if (argc > 1) {
        auto ms = [](auto f) {
            std::vector<double> v;
            for (int r = 0; r < 7; r++) {
                const auto t0 = std::chrono::steady_clock::now();
                f();
                v.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            for (size_t i = 1; i < v.size(); i++)
                for (size_t j = i; j > 0 && v[j] < v[j - 1]; j--) { const double t = v[j]; v[j] = v[j - 1]; v[j - 1] = t; }
            return v[v.size() / 2];
        };
        int st = CHIP_OK;
        const double t_join = ms([&] { st |= chip_query_batch_rows_f32(c, rows.data(), k.data(), N, K, s_join.data(), i_join.data()); });
        const double t_loop = ms([&] { st |= loop(); });
        CHK(st);
        std::printf("medians of 7: one call %.3f ms | the loop of %d single queries %.3f ms\n", t_join, N, t_loop);
    }
    chip_destroy(c);
    return 0;
}
