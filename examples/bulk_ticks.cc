// bulk_ticks.cc -- the tick records of a whole schedule in ONE call (include/cerebro_hip.h "Bulk ticks") against the loop of ticks: a
// 256-D x 3000-row DB of unit rows with planted revisits, walked at every l = 3 .. 3000 with the default parameters (so skipped, too-short
// and scanned ticks interleave).
//   one call : chip_loop_ticks_bulk over all the l (many-query groups, certificate, exact rescoring, the accept rule)
//   the loop : chip_loop_reset, then chip_loop_tick per l; chip_query_rows per scanned tick for the lists
// Every field of every record, every score and every index must have equal bits.  With an argument it also times both.
//   bulk_ticks          compare
//   bulk_ticks time     compare, then time
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cerebro_hip.h"

#define CHK(call) do { const int _s = (call); if (_s != CHIP_OK) { std::printf("%s: status %d (%s)\n", #call, _s, chip_strerror(_s)); return 1; } } while (0)

int main(int argc, char **)
{
    if (chip_build_has_bulk_ticks() != 1) { std::printf("this build has no bulk ticks\n"); return 1; }
    const int D = 256, N = 3000, K = 5;
    // planted revisits: from row 400 on, runs of six rows are noisy copies of the (unplanted) rows 310 back
    std::vector<int64_t> dst, src;
    std::vector<int32_t> kind;
    for (int i = 400; i < N; i++)
        if (i % 20 < 6) { dst.push_back(i); src.push_back(i - 310); kind.push_back(1); }
    chip_ctx *c = nullptr;
    CHK(chip_create(&c, D, 0, 0, 0, 1));
    CHK(chip_db_append_synthetic_unit(c, N, 2024, dst.data(), src.data(), kind.data(), (int64_t)dst.size()));
    chip_dot_params p;
    chip_dot_params_default(&p);

    std::vector<int64_t> l;
    for (int64_t i = 3; i <= N; i++) l.push_back(i);
    const int32_t T = (int32_t)l.size();
    std::vector<chip_tick_result> bulk((size_t)T), loop((size_t)T);
    std::vector<double> s_bulk((size_t)T * 3 * K), s_loop((size_t)T * 3 * K);
    std::vector<int64_t> i_bulk((size_t)T * 3 * K), i_loop((size_t)T * 3 * K);
    int64_t last_bulk = -1;
    CHK(chip_loop_ticks_bulk(c, l.data(), T, &p, 0, K, bulk.data(), s_bulk.data(), i_bulk.data(), &last_bulk));
    chip_bulk_ticks_last last;
    CHK(chip_debug_bulk_ticks_last(c, &last));

    auto run_loop = [&](bool lists) -> int {
        chip_loop_reset(c);
        for (int32_t t = 0; t < T; t++) {
            CHK(chip_loop_tick(c, l[(size_t)t], &p, &loop[(size_t)t]));
            if (!lists) continue;
            double *s = s_loop.data() + (size_t)t * 3 * K;
            int64_t *ix = i_loop.data() + (size_t)t * 3 * K;
            if (loop[(size_t)t].status == CHIP_TICK_SCANNED) {
                const int64_t rows[3] = {l[(size_t)t] - 1, l[(size_t)t] - 2, l[(size_t)t] - 3};
                CHK(chip_query_rows(c, l[(size_t)t] - p.lag, rows, 3, K, s, ix));
            } else {
                for (int j = 0; j < 3 * K; j++) { s[j] = -INFINITY; ix[j] = -1; }
            }
        }
        return 0;
    };
    if (run_loop(true)) return 1;
    int bad = 0, scanned = 0, found = 0;
    for (int32_t t = 0; t < T; t++) {
        const chip_tick_result &a = bulk[(size_t)t], &b = loop[(size_t)t];
        const bool same = a.status == b.status && a.found == b.found && a.idx_curr == b.idx_curr && a.idx_prev == b.idx_prev &&
                          std::memcmp(&a.score, &b.score, sizeof a.score) == 0 && std::memcmp(a.argmax, b.argmax, sizeof a.argmax) == 0 &&
                          std::memcmp(a.maxv, b.maxv, sizeof a.maxv) == 0 &&
                          std::memcmp(s_bulk.data() + (size_t)t * 3 * K, s_loop.data() + (size_t)t * 3 * K, sizeof(double) * 3 * K) == 0 &&
                          std::memcmp(i_bulk.data() + (size_t)t * 3 * K, i_loop.data() + (size_t)t * 3 * K, sizeof(int64_t) * 3 * K) == 0;
        if (!same && bad++ < 5)
            std::printf("tick at l = %lld DIFFERS: status %d found %d best %lld (%.17g) against status %d found %d best %lld (%.17g)\n", (long long)l[(size_t)t],
                        a.status, a.found, (long long)a.argmax[0], a.maxv[0], b.status, b.found, (long long)b.argmax[0], b.maxv[0]);
        scanned += a.status == CHIP_TICK_SCANNED;
        found += a.found;
    }
    if (last_bulk != chip_loop_last_l(c)) { std::printf("last_l DIFFERS: %lld against %lld\n", (long long)last_bulk, (long long)chip_loop_last_l(c)); bad++; }
    std::printf("%d ticks (%d scanned, %d loops found), %d groups, %d launches, %d host waits; certified %lld, uncertified %lld (run again exactly: %lld), "
                "%lld rows rescored, lists of %d, E = %.3g\n", T, scanned, found, last.groups, last.launches, last.waits, (long long)last.certified,
                (long long)last.uncertified, (long long)last.exact_reruns, (long long)last.rescored_rows, last.list_len, last.E);
    if (bad) { std::printf("%d differences\n", bad); return 1; }
    std::printf("%d records and %d lists of %d compared with the loop of ticks: all equal\n", T, 3 * T, K);

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
        const double t_bulk = ms([&] { st |= chip_loop_ticks_bulk(c, l.data(), T, &p, 0, 1, bulk.data(), nullptr, nullptr, nullptr); });
        const double t_loop = ms([&] { st |= run_loop(false); });
        CHK(st);
        std::printf("medians of 7: one call %.3f ms | the loop of %d ticks %.3f ms\n", t_bulk, T, t_loop);
    }
    chip_destroy(c);
    return 0;
}
