// ransac_common.h -- pieces shared by the batched RANSAC legs (pnp.hip, icp.hip): the counter-based RNG + sampler
// (device) and the host side of a call: parameter check, the per-hypothesis result block, theia::Ransac's sequential selection
// rule replayed on the host (K7), the report of its winner and the copy-out of the whole block (test aid).
#pragma once
#include "chip_internal.h"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace chip {

constexpr int kSampleMax = 16;   // DlsPnpWithRansac.h:45 uses 15, :118 uses 10

__device__ __forceinline__ uint64_t splitmix64_d(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t rng_draw(uint64_t seed, uint32_t hyp, uint32_t draw)
{
    return splitmix64_d(seed ^ ((uint64_t)hyp << 32) ^ (uint64_t)draw);
}

// theia::RandomSampler restated: partial Fisher-Yates over a VIRTUAL identity permutation of N: step i swaps positions i and
// j_i = i + draw_i % (N - i); only the <= 2S touched positions are materialised.  Executed by a WHOLE WAVE: the S draws and
// their 64-bit modulo are computed by lanes 0..S-1 at once, and the sparse permutation map lives in registers (lane e holds
// entry e) so that every lookup is a __ballot + v_readlane instead of a serial scan.  Returns sample i in lane i (< S).
__device__ __forceinline__ int ransac_sample_wave(uint64_t seed, int hyp, int N, int S, int lane)
{
    int jv = 0;
    if (lane < S) {
        const uint64_t x = rng_draw(seed, (uint32_t)hyp, (uint32_t)lane);
        jv = lane + (int)(x % (uint64_t)(N - lane));
    }
    int key = -1, val = 0, used = 0, mine = 0;
    for (int i = 0; i < S; i++) {
        const int j = __builtin_amdgcn_readlane(jv, i);
        const unsigned long long mi = __ballot(lane < used && key == i), mj = __ballot(lane < used && key == j);
        int vi = i, vj = j, pi = -1, pj = -1;
        if (mi) { pi = __builtin_ctzll(mi); vi = __builtin_amdgcn_readlane(val, pi); }
        if (mj) { pj = __builtin_ctzll(mj); vj = __builtin_amdgcn_readlane(val, pj); }
        if (pi < 0) { pi = used++; if (lane == pi) key = i; }   // idx[i] <- vj ; idx[j] <- vi
        if (lane == pi) val = vj;
        if (j != i) {
            if (pj < 0) { pj = used++; if (lane == pj) key = j; }
            if (lane == pj) val = vi;
        }
        if (lane == i) mine = vj;
    }
    return mine;
}

inline uint64_t splitmix64_h(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// CHIP_SAMPLER_THEIA_PERSISTENT: theia::RandomSampler as written -- Initialize() once (0..N-1), every Sample() continues on the
// permutation the previous one left (oracle/pnp_ransac.c orc_ransac_sample_persistent).  Inherently sequential over the
// hypotheses, S swaps each: done on the host, the kernels read the table (out[h * stride + i]).  `perm` is scratch (>= N).
inline void ransac_sample_table_persistent(uint64_t seed, int32_t H, int32_t N, int32_t S, int32_t stride, int32_t *perm, int32_t *out)
{
    for (int32_t i = 0; i < N; i++) perm[i] = i;
    for (int32_t h = 0; h < H; h++)
        for (int32_t i = 0; i < S; i++) {
            const uint64_t x = splitmix64_h(seed ^ ((uint64_t)(uint32_t)h << 32) ^ (uint64_t)(uint32_t)i);
            const int32_t j = i + (int32_t)(x % (uint64_t)(N - i));
            const int32_t t = perm[i]; perm[i] = perm[j]; perm[j] = t;
            out[(size_t)h * stride + i] = perm[i];
        }
}

// theia::SampleConsensusEstimator::ComputeMaxIterations
inline int32_t ransac_max_iterations(int32_t S, double ratio, double log_fail, int32_t min_it, int32_t max_it)
{
    if (ratio == 1.0) return min_it;
    const double log_prob = std::log(1.0 - std::pow(ratio, (double)S)) - DBL_EPSILON;
    const double itf = std::floor(log_fail / log_prob) + 1.0;
    int32_t it = (itf > 2.0e9) ? 2000000000 : (int32_t)itf;
    if (it < min_it) it = min_it;
    if (it > max_it) it = max_it;
    return it;
}

inline int32_t ransac_initial_iterations(const chip_ransac_params *p)
{
    if (p->n_hypotheses > 0) return p->n_hypotheses;
    int32_t max_it = p->max_iterations;
    if (p->min_inlier_ratio > 0)
        max_it = ransac_max_iterations(p->sample_size, p->min_inlier_ratio, std::log(p->failure_probability), p->min_iterations, p->max_iterations);
    return max_it;
}

// K7: theia::Ransac::Estimate's sequential rule (strict '<': first best wins; early termination unless benchmark mode)
// replayed over per-hypothesis results.  Returns the winner (-1: none); *num_it = iterations the reference would run.
inline int32_t ransac_select(const chip_ransac_params *p, int32_t N, int32_t H, const int32_t *valid, const double *cost,
                             const int32_t *nin, int32_t *num_it_out, int32_t *n_models_out, double *best_cost_out)
{
    const bool bench = p->n_hypotheses > 0;
    const int32_t S = p->sample_size;
    const double log_fail = std::log(p->failure_probability);
    double best_cost = DBL_MAX;
    int32_t best_h = -1, n_models = 0, num_it = 0, max_it = H;
    for (num_it = 0; num_it < max_it; num_it++) {
        if (!valid[num_it]) continue;   // EstimateModel returned false
        n_models++;
        if (cost[num_it] < best_cost) {
            best_cost = cost[num_it];
            best_h = num_it;
            if (!bench) {
                const double ratio = (double)nin[num_it] / (double)N;
                if (ratio < (double)S / (double)N) continue;
                const int32_t mi = ransac_max_iterations(S, ratio, log_fail, p->min_iterations, p->max_iterations);
                if (mi < max_it) max_it = mi;
            }
        }
    }
    *num_it_out = num_it;
    *n_models_out = n_models;
    *best_cost_out = best_cost;
    return best_h;
}

// What both entry points refuse, in the order they report it (the callers check their pointers first)
inline int ransac_check_params(const chip_ransac_params *p, int32_t N)
{
    if (N < 20) return CHIP_ERR_TOO_FEW_POINTS;  // DlsPnpWithRansac.cpp:136-139 (PnP) / :19-22 (ICP)
    const int32_t S = p->sample_size;
    if (S < 3 || S > kSampleMax || S > N || p->n_hypotheses < 0 || p->max_iterations < 1) return CHIP_ERR_UNSUPPORTED;
    if (p->sampler != CHIP_SAMPLER_FRESH && p->sampler != CHIP_SAMPLER_THEIA_PERSISTENT) return CHIP_ERR_UNSUPPORTED;
    return CHIP_OK;
}

// Per-hypothesis results live in pinned, device-mapped HOST memory: the scoring kernel stores them straight across PCIe (a few
// hundred KB per call, posted while the kernel runs), so a call needs no D2H copy and a single stream synchronisation.
struct RansacResults {
    PinnedBuf<double> cost, T;                 // [H], [H][16]
    PinnedBuf<int32_t> nin, valid;             // [H]
    PinnedBuf<unsigned long long> mask;        // [H][words]
    PinnedBuf<int32_t> sample_in;              // CHIP_SAMPLER_THEIA_PERSISTENT: the host-sequenced sample table [H][kSampleMax] ...
    std::vector<int32_t> perm;                 // ... and the permutation it is sequenced on
    int32_t cap_H = 0, cap_words = 0;
    bool fits(int H, int words) const { return H <= cap_H && words <= cap_words; }
    int reserve(Ctx *c, int H, int words)      // H and words never shrink; the caller holds one ResidentPause over its whole group
    {
        if (fits(H, words)) return CHIP_OK;
        const size_t nh = (size_t)(H > cap_H ? H : cap_H), nw = (size_t)(words > cap_words ? words : cap_words);
        cap_H = cap_words = 0;
        int rc = cost.reserve(c, nh);
        if (rc == CHIP_OK) rc = T.reserve(c, 16 * nh);
        if (rc == CHIP_OK) rc = nin.reserve(c, nh);
        if (rc == CHIP_OK) rc = valid.reserve(c, nh);
        if (rc == CHIP_OK) rc = mask.reserve(c, nh * nw);
        if (rc == CHIP_OK) rc = sample_in.reserve(c, kSampleMax * nh);
        if (rc != CHIP_OK) return rc;
        cap_H = (int32_t)nh; cap_words = (int32_t)nw;
        return CHIP_OK;
    }
};

// The end of a call: ransac_select over hypotheses [first_hyp, first_hyp + H) of r (rows of `words` mask words), then the winner's
// pose, inlier mask and confidence -- or, without one, the reference's uninitialised Matrix4d as 16 NaNs (the caller NaN-checks).
inline void ransac_report(const chip_ransac_params *p, int32_t N, int H, int words, const RansacResults &r, size_t first_hyp,
                          double *T_colmajor, float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary)
{
    double best_cost = DBL_MAX;
    int32_t n_models = 0, num_it = 0, nin = 0;
    const int32_t best_h = ransac_select(p, N, H, r.valid.host() + first_hyp, r.cost.host() + first_hyp, r.nin.host() + first_hyp, &num_it, &n_models, &best_cost);
    if (best_h >= 0) {
        const size_t h = first_hyp + (size_t)best_h;
        std::memcpy(T_colmajor, r.T.host() + 16 * h, sizeof(double) * 16);
        nin = r.nin.host()[h];
        const unsigned long long *hm = r.mask.host() + h * (size_t)words;
        if (inlier_mask)
            for (int i = 0; i < N; i++) inlier_mask[i] = (uint8_t)((hm[i >> 6] >> (i & 63)) & 1ull);
        const double ratio = (double)nin / (double)N;
        *confidence = (float)(1.0 - std::pow(1.0 - std::pow(ratio, (double)p->sample_size), (double)num_it));  // summary.confidence (DlsPnpWithRansac.cpp:240 / :121)
    } else {
        for (int i = 0; i < 16; i++) T_colmajor[i] = NAN;
        if (inlier_mask) std::memset(inlier_mask, 0, (size_t)N);
        *confidence = 0.0f;
    }
    if (summary) {
        summary->n_iterations = num_it;
        summary->n_inliers = nin;
        summary->best_hypothesis = best_h;
        summary->n_models = n_models;
        summary->best_cost = best_h >= 0 ? best_cost : INFINITY;
    }
}

// Test aid (chip_debug_ransac_record): hypotheses [first_hyp, first_hyp + H) of r, rows of `words` mask words, as a copy with defined
// content everywhere.  The kernels write neither T nor the mask row of a rejected hypothesis, nor the mask words beyond a problem's own
// ceil(N / 64) (a batched launch gives every row the stride of its widest problem): those slots hold what an earlier call left there.
// The copy has T = NaN and mask = 0 in them, so that whole arrays can be compared.  Every output may be null.
inline void ransac_record_copy(const RansacResults &r, size_t first_hyp, int H, int words, int32_t N, int32_t *valid, double *cost,
                               int32_t *nin, double *T, unsigned long long *mask)
{
    const int32_t *v = r.valid.host() + first_hyp;
    if (valid) std::memcpy(valid, v, sizeof(int32_t) * (size_t)H);
    if (cost) std::memcpy(cost, r.cost.host() + first_hyp, sizeof(double) * (size_t)H);
    if (nin) std::memcpy(nin, r.nin.host() + first_hyp, sizeof(int32_t) * (size_t)H);
    const int own = (N + 63) / 64;
    for (int h = 0; h < H; h++) {
        if (T)
            for (int e = 0; e < 16; e++) T[16 * (size_t)h + e] = v[h] ? r.T.host()[16 * (first_hyp + h) + e] : (double)NAN;
        if (mask)
            for (int w = 0; w < words; w++)
                mask[(size_t)h * words + w] = (v[h] && w < own) ? r.mask.host()[(first_hyp + h) * (size_t)words + w] : 0ull;
    }
}

}  // namespace chip
