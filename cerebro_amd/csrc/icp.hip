// icp.hip -- batched Umeyama-ICP-in-RANSAC on gfx950: replaces the RANSAC branch of
// StaticTheiaPoseCompute::P3P_ICP (/root/reference/src/DlsPnpWithRansac.cpp:65-121), i.e. theia::Ransac over the
// AlignPointCloudsUmeyamaWithRansac estimator (src/DlsPnpWithRansac.h:104-166).
//
//   icp_models    : ONE LANE per hypothesis (64 hypotheses per wave; round 5 -- rounds 1-4 ran one wave per hypothesis with all 64
//                   lanes computing the same 3x3 solve).  The lane draws its 10-point sample (the same counter-based partial
//                   Fisher-Yates as PnP, here with the sparse permutation map in the lane's own registers: step i's entry is
//                   (j_i, value), a lookup takes the LAST earlier entry with that key), gathers the sample points, and runs
//                   the Umeyama solve (means, covariance, fixed-sweep Jacobi SVD, S22 sign, scale: ~600 flops + 24 rotations
//                   with a division and two square roots each); accept iff min(s, 1/s) > 0.9 (:137); writes b_T_a + valid.
//   icp_score     : one wave per hypothesis: the L2 error of all N correspondences under that hypothesis's model, MLE cost in
//                   the fixed lane-strided + butterfly order, inlier words by __ballot.
//                   Both kernels keep the operation order of oracle/icp_ransac.c, so poses, costs and masks are the bits of
//                   rounds 1-4 (tests/test_icp_gpu.py); the model work per call drops 64-fold (8000 hypotheses: 168 -> see
//                   profiles/r05_icp.txt), the reference-mode call (<= 50 hypotheses = one wave of icp_models) keeps its latency.
//   The two bodies are stated once, icp_model_lane and icp_score_wave, on a row index and on A / B / N / seed / multipliers handed in.
//   Two entry pairs call them and differ only in where those per-problem values come from.  icp_models / icp_score: one estimation,
//   the values travel in the kernel argument block (no table, no copy), row = hypothesis.  icp_models_batch / icp_score_batch add a
//   PROBLEM dimension (blockIdx.y; ceil(H / 64) x P and H x P): up to CHIP_ICP_MAX_BATCH independent estimations -- the 3-D / 3-D sets
//   of all surviving candidates of a keyframe -- share one pair of launches, and a wave reads its problem's values from a table in
//   device memory (IcpProblem) through uniform loads.  The bits of a problem depend neither on P nor on its position nor on its
//   neighbours (tests/test_icp_batch_gpu.py).
//   K7 on the host: ransac_common.h (shared with PnP).
// fp64, -ffp-contract=off, same operation order as oracle/icp_ransac.c => bit-identical poses and masks.
#include "ransac_common.h"
#include <cstring>
#include <new>
#include <vector>

namespace chip {

// IcpLaunch: the per-hypothesis arrays and the parameters all problems of a launch share; problem p, hypothesis h has row p * H + h in
// every array (a single estimation is problem 0).
struct IcpLaunch {
    int32_t S, H;
    double thresh;
    int32_t use_mle;
    int32_t mask_words;              // row stride of mask: ceil(N / 64) of the launch's widest problem; a problem writes its own words only
    double *T_out;     // [P * H][16]
    double *cost;      // [P * H]
    int32_t *nin;      // [P * H]
    int32_t *valid;    // [P * H]
    unsigned long long *mask;  // [P * H][mask_words]
    const int32_t *sample_in;   // CHIP_SAMPLER_THEIA_PERSISTENT: [P * H][kSampleMax] sequenced by the host (pinned, device-mapped); else nullptr
    double *T_dev;     // [P * H][16] device copy of the models: the score kernel reads it (T_out is pinned HOST memory)
    int32_t *valid_dev;// [P * H]
};
// IcpProblem: what differs between the problems
struct IcpProblem {
    const double *A;   // N x 3 (frame a)
    const double *B;   // N x 3 (frame b)
    int32_t N, pad_;
    uint64_t seed;
    uint64_t magic[kSampleMax];   // floor(2^64 / (N - i)): the sampler's 64-bit modulo as a multiply-high (the divisors depend on i only)
};
// A single estimation (icp_models / icp_score): its problem travels in the kernel argument block
struct IcpArgs {
    IcpProblem pr;
    IcpLaunch l;
};
// A batched launch (icp_models_batch / icp_score_batch): one row per problem of a table in DEVICE memory (the enqueue copies it there
// in-stream); a wave reads its row, blockIdx.y, through uniform (scalar) loads
struct IcpBatchArgs {
    const IcpProblem *prob;          // [P]
    IcpLaunch l;
};

constexpr int kJacobiSweeps = 8;

#define JROT(p, q)                                                                             \
    do {                                                                                       \
        const double apq = Am[p][q];                                                           \
        if (apq != 0.0) {                                                                      \
            const double theta = (Am[q][q] - Am[p][p]) / (2.0 * apq);                          \
            const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)); \
            const double cc = 1.0 / sqrt(tt * tt + 1.0), ss = tt * cc;                         \
            for (int r = 0; r < 3; r++) {                                                      \
                const double arp = Am[r][p], arq = Am[r][q];                                   \
                Am[r][p] = cc * arp - ss * arq;                                                \
                Am[r][q] = ss * arp + cc * arq;                                                \
            }                                                                                  \
            for (int r = 0; r < 3; r++) {                                                      \
                const double apr = Am[p][r], aqr = Am[q][r];                                   \
                Am[p][r] = cc * apr - ss * aqr;                                                \
                Am[q][r] = ss * apr + cc * aqr;                                                \
            }                                                                                  \
            for (int r = 0; r < 3; r++) {                                                      \
                const double vrp = V[r][p], vrq = V[r][q];                                     \
                V[r][p] = cc * vrp - ss * vrq;                                                 \
                V[r][q] = ss * vrp + cc * vrq;                                                 \
            }                                                                                  \
        }                                                                                      \
    } while (0)

#define COLSWAP(i, j)                                                                          \
    do {                                                                                       \
        const double tw = w[i]; w[i] = w[j]; w[j] = tw;                                        \
        for (int r = 0; r < 3; r++) { const double tv = V[r][i]; V[r][i] = V[r][j]; V[r][j] = tv; } \
    } while (0)

// Sample of hypothesis `hyp` by ONE lane: theia::RandomSampler's partial Fisher-Yates over a virtual identity permutation
// (oracle/pnp_ransac.c orc_ransac_sample; ransac_common.h has the wave-cooperative form).  Step i swaps positions i and
// j_i = i + draw_i % (N - i).  Position i is final after step i and never read again, so only the j-targets need remembering:
// entry e = (key j_e, the value step e wrote there); the current value of a position is that of the LAST earlier entry with
// that key, else the position itself.  Fully unrolled, so keys / values stay in registers.
// x % d by Barrett reduction with the host's m = floor(2^64 / d): q = mulhi(x, m) underestimates x / d by at most 2, so the
// remainder needs at most two corrections -- the exact x % d of the oracle (hipcc's generic 64-bit division is ~150 instructions
// per draw and lane; the divisors N - i are the same for every hypothesis).
__device__ __forceinline__ uint64_t mod_magic(uint64_t x, uint64_t d, uint64_t m)
{
    uint64_t r = x - __umul64hi(x, m) * d;
    if (r >= d) r -= d;
    if (r >= d) r -= d;
    return r;
}

__device__ __forceinline__ void ransac_sample_lane(uint64_t seed, int hyp, int N, int S, const uint64_t *magic, int smp[kSampleMax])
{
    int key[kSampleMax], val[kSampleMax];
#pragma unroll
    for (int i = 0; i < kSampleMax; i++) {
        key[i] = -1; val[i] = 0; smp[i] = 0;
        if (i < S) {
            const uint64_t x = rng_draw(seed, (uint32_t)hyp, (uint32_t)i);
            const int j = i + (int)mod_magic(x, (uint64_t)(N - i), magic[i]);
            int vi = i, vj = j;
#pragma unroll
            for (int e = 0; e < i; e++) {
                if (key[e] == i) vi = val[e];
                if (key[e] == j) vj = val[e];
            }
            smp[i] = vj;          // idx[i] <- old idx[j]
            key[i] = j;           // idx[j] <- old idx[i]   (j == i: vj == vi, a no-op as in the reference)
            val[i] = vi;
        }
    }
}

// One hypothesis of one problem by ONE lane: sample, Umeyama, scale gate, pose -> row `row` of the launch's arrays.
__device__ __forceinline__ void icp_model_lane(const double *A, const double *B, int N, uint64_t seed, const uint64_t *magic, int hyp, size_t row,
                                               const IcpLaunch &a)
{
    const int n = a.S;
    int smp[kSampleMax];
    if (a.sample_in) {
#pragma unroll
        for (int i = 0; i < kSampleMax; i++) smp[i] = i < n ? a.sample_in[row * kSampleMax + i] : 0;
    } else {
        ransac_sample_lane(seed, hyp, N, n, magic, smp);
    }

    // ---- Umeyama on the sample ----
    double ma[3] = {0.0, 0.0, 0.0}, mb[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kSampleMax; i++)
        if (i < n)
            for (int k = 0; k < 3; k++) { ma[k] = ma[k] + A[3 * smp[i] + k]; mb[k] = mb[k] + B[3 * smp[i] + k]; }
    for (int k = 0; k < 3; k++) { ma[k] = ma[k] / (double)n; mb[k] = mb[k] / (double)n; }
    double Sg[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, var_a = 0.0;
#pragma unroll
    for (int i = 0; i < kSampleMax; i++)
        if (i < n) {
            double da[3], db[3];
            for (int k = 0; k < 3; k++) { da[k] = A[3 * smp[i] + k] - ma[k]; db[k] = B[3 * smp[i] + k] - mb[k]; }
            var_a = var_a + ((da[0] * da[0] + da[1] * da[1]) + da[2] * da[2]);
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) Sg[r][c] = Sg[r][c] + db[r] * da[c];
        }
    var_a = var_a / (double)n;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Sg[r][c] = Sg[r][c] / (double)n;
    double Am[3][3], V[3][3], w[3], sig[3], U[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            Am[r][c] = (Sg[0][r] * Sg[0][c] + Sg[1][r] * Sg[1][c]) + Sg[2][r] * Sg[2][c];
            V[r][c] = (r == c) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) { JROT(0, 1); JROT(0, 2); JROT(1, 2); }
    w[0] = Am[0][0]; w[1] = Am[1][1]; w[2] = Am[2][2];
    // descending selection sort (ties keep the lower index first), same comparisons as the oracle
    if (w[1] > w[0]) COLSWAP(0, 1);
    if (w[2] > w[0]) COLSWAP(0, 2);
    if (w[2] > w[1]) COLSWAP(1, 2);
    {
        const double det = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                           V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
        if (det < 0.0)
            for (int r = 0; r < 3; r++) V[r][2] = -V[r][2];
    }
    for (int k = 0; k < 3; k++) sig[k] = sqrt(w[k] > 0.0 ? w[k] : 0.0);
    bool ok = (sig[1] > 1e-6 * sig[0]) && (sig[0] > 0.0);
    double R[9], t[3], scale = 0.0;
    for (int e = 0; e < 9; e++) R[e] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (ok) {
        for (int k = 0; k < 2; k++)
            for (int r = 0; r < 3; r++) U[r][k] = ((Sg[r][0] * V[0][k] + Sg[r][1] * V[1][k]) + Sg[r][2] * V[2][k]) / sig[k];
        double S22 = 1.0;
        if (sig[2] > 1e-6 * sig[0]) {
            for (int r = 0; r < 3; r++) U[r][2] = ((Sg[r][0] * V[0][2] + Sg[r][1] * V[1][2]) + Sg[r][2] * V[2][2]) / sig[2];
            const double detU = U[0][0] * (U[1][1] * U[2][2] - U[1][2] * U[2][1]) - U[0][1] * (U[1][0] * U[2][2] - U[1][2] * U[2][0]) +
                                U[0][2] * (U[1][0] * U[2][1] - U[1][1] * U[2][0]);
            if (detU < 0.0) S22 = -1.0;
        } else {
            U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
            U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
            U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[3 * r + c] = (U[r][0] * V[c][0] + U[r][1] * V[c][1]) + (S22 * U[r][2]) * V[c][2];
        scale = ((sig[0] + sig[1]) + S22 * sig[2]) / var_a;
        for (int r = 0; r < 3; r++) t[r] = mb[r] - scale * ((R[3 * r] * ma[0] + R[3 * r + 1] * ma[1]) + R[3 * r + 2] * ma[2]);
        const double inv = 1.0 / scale;
        ok = (scale < inv ? scale : inv) > 0.9;   // DlsPnpWithRansac.h:137
    }
    a.valid_dev[row] = ok ? 1 : 0;
    if (!ok) { a.valid[row] = 0; a.nin[row] = 0; a.cost[row] = INFINITY; return; }
    double T[16];
    T[0] = R[0]; T[1] = R[3]; T[2] = R[6]; T[3] = 0.0;
    T[4] = R[1]; T[5] = R[4]; T[6] = R[7]; T[7] = 0.0;
    T[8] = R[2]; T[9] = R[5]; T[10] = R[8]; T[11] = 0.0;
    T[12] = t[0]; T[13] = t[1]; T[14] = t[2]; T[15] = 1.0;
    for (int e = 0; e < 16; e++) { a.T_dev[row * 16 + e] = T[e]; a.T_out[row * 16 + e] = T[e]; }
}

// One hypothesis of one problem by ONE wave: the error of all N correspondences under the model in row `row`
__device__ __forceinline__ void icp_score_wave(const double *A, const double *B, int N, size_t row, const IcpLaunch &a)
{
    const int lane = threadIdx.x;
    if (!a.valid_dev[row]) return;       // wave-uniform; icp_models has written valid / nin / cost of a rejected hypothesis
    double T[16];
    for (int e = 0; e < 16; e++) T[e] = a.T_dev[row * 16 + e];
    // ---- Error (L2, DlsPnpWithRansac.h:152-164) over all N + MLE cost ----
    double acc = 0.0;
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < N) {
            const double a0 = A[3 * i], a1 = A[3 * i + 1], a2 = A[3 * i + 2];
            const double x = ((T[0] * a0 + T[4] * a1) + T[8] * a2) + T[12];
            const double y = ((T[1] * a0 + T[5] * a1) + T[9] * a2) + T[13];
            const double z = ((T[2] * a0 + T[6] * a1) + T[10] * a2) + T[14];
            const double dx = x - B[3 * i], dy = y - B[3 * i + 1], dz = z - B[3 * i + 2];
            const double rr = sqrt((dx * dx + dy * dy) + dz * dz);
            in = rr < a.thresh;
            acc = acc + (in ? rr : a.thresh);
        }
        const unsigned long long bw = __ballot(in);
        cnt += __popcll(bw);
        if (lane == 0) a.mask[row * a.mask_words + (base >> 6)] = bw;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m, 64);
    if (lane == 0) {
        a.valid[row] = 1;
        a.nin[row] = cnt;
        a.cost[row] = a.use_mle ? acc : (double)(N - cnt);
    }
}

__global__ __launch_bounds__(64) void icp_models(IcpArgs a)
{
    const int hyp = blockIdx.x * 64 + threadIdx.x;
    if (hyp >= a.l.H) return;
    icp_model_lane(a.pr.A, a.pr.B, a.pr.N, a.pr.seed, a.pr.magic, hyp, (size_t)hyp, a.l);
}

__global__ __launch_bounds__(64) void icp_score(IcpArgs a)
{
    icp_score_wave(a.pr.A, a.pr.B, a.pr.N, (size_t)blockIdx.x, a.l);
}

__global__ __launch_bounds__(64) void icp_models_batch(IcpBatchArgs a)
{
    const IcpProblem &pr = a.prob[blockIdx.y];   // wave-uniform: everything read from it stays in scalar registers
    const double *const A = pr.A, *const B = pr.B;
    const int N = pr.N;
    const uint64_t seed = pr.seed;
    uint64_t magic[kSampleMax];
#pragma unroll
    for (int i = 0; i < kSampleMax; i++) magic[i] = pr.magic[i];
    const int hyp = blockIdx.x * 64 + threadIdx.x;
    if (hyp >= a.l.H) return;
    icp_model_lane(A, B, N, seed, magic, hyp, (size_t)blockIdx.y * (size_t)a.l.H + (size_t)hyp, a.l);
}

__global__ __launch_bounds__(64) void icp_score_batch(IcpBatchArgs a)
{
    const IcpProblem &pr = a.prob[blockIdx.y];   // wave-uniform
    icp_score_wave(pr.A, pr.B, pr.N, (size_t)blockIdx.y * (size_t)a.l.H + (size_t)blockIdx.x, a.l);
}

constexpr int kIcpMaxBatch = CHIP_ICP_MAX_BATCH;

// What is pending / was collected last
enum IcpKind { kIcpSingle = 0, kIcpMatchedBatch = 1 };

struct IcpState {
    DevBuf<double> A, B, T_dev;        // A / B: the staged points of all problems of a host-pointer call, problem after problem
    DevBuf<int32_t> valid_dev;
    PinnedBuf<IcpProblem> prob;        // a batched launch's problem table (kIcpMaxBatch rows) as the host writes it ...
    DevBuf<IcpProblem> prob_dev;       // ... and where the kernels read it: copied in-stream, ahead of the launches
    RansacResults res;                 // what icp_score leaves per hypothesis (as in pnp.hip: no D2H copies, one sync per call)
    hipStream_t stream = nullptr;      // the ICP stream (not the PnP stream: the two estimations may overlap)
    bool pending = false;              // an enqueued estimation awaits its collect
    bool collected = false;            // pend_* and res describe a finished launch (test aid: chip_debug_ransac_record)
    int pend_kind = kIcpSingle;
    int32_t pend_P = 0, pend_H = 0, pend_words = 0;   // the launch: its problems, hypotheses per problem, mask row stride
    int32_t pend_N[kIcpMaxBatch] = {};
    // a matched batch answers pend_total problems, of which pend_P ran: problem r of the launch is answer pend_at[r]
    int32_t pend_total = 0, pend_at[kIcpMaxBatch] = {};
    chip_ransac_params pend_params{};
};

void icp_destroy(Ctx *c)
{
    IcpState *st = c->icp_state;
    if (!st) return;
    if (st->stream) { (void)hipStreamSynchronize(st->stream); (void)hipStreamDestroy(st->stream); }
    delete st;
    c->icp_state = nullptr;
}

// Ntot: points to stage per side (0: the sets are read where they lie), PH: hypotheses of the whole launch
static int icp_reserve(Ctx *c, IcpState *st, size_t Ntot, size_t PH, int words)
{
    const size_t nN = 3 * Ntot;
    // one pause over the group: hipFree waits for the whole device, no resident scan instance on it until the last allocation is done
    ResidentPause paused(c, nN > st->A.capacity() || PH > st->valid_dev.capacity() || !st->res.fits((int)PH, words) || !st->prob.capacity());
    int rc = st->A.reserve(c, nN);
    if (rc == CHIP_OK) rc = st->B.reserve(c, nN);
    if (rc == CHIP_OK) rc = st->T_dev.reserve(c, 16 * PH);
    if (rc == CHIP_OK) rc = st->valid_dev.reserve(c, PH);
    if (rc == CHIP_OK) rc = st->res.reserve(c, (int)PH, words);
    if (rc == CHIP_OK) rc = st->prob_dev.reserve(c, kIcpMaxBatch);
    if (rc == CHIP_OK) rc = st->prob.reserve(c, kIcpMaxBatch);   // last: its capacity stands for the two tables
    return rc;
}

}  // namespace chip

using namespace chip;

extern "C" void chip_icp_params_default(chip_ransac_params *p)
{
    if (!p) return;
    chip_ransac_params_default(p);
    p->error_thresh = 0.1;  // DlsPnpWithRansac.cpp:89
    p->sample_size = 10;    // DlsPnpWithRansac.h:118
}

extern "C" int chip_build_has_icp_batch(void) { return 1; }

// The estimation is split in two so that it can run underneath something else (its kernels are tiny and the PnP kernels leave
// the GPU 92-95 % idle): enqueue = H2D of the points + ONE pair of launches for all P problems on the ICP stream, no
// synchronisation; collect = wait, replay theia's selection rule problem by problem, fetch the winners.  chip_icp_ransac is a batch
// of one, enqueue + collect.  P == 1 launches icp_models / icp_score, P >= 2 the batched pair behind an in-stream copy of the problem
// table.  P == 0 (a matched batch without a runnable problem) launches nothing.
static int icp_enqueue_locked(Ctx *c, int P, const double *const *A, const double *const *B, const int32_t *N, const chip_ransac_params *p,
                              const uint64_t *seeds, bool dev_in, int kind)
{
    CHIP_HIP(c, hipSetDevice(c->device));
    if (!c->icp_state) {
        c->icp_state = new (std::nothrow) IcpState();
        if (!c->icp_state) return CHIP_ERR_OOM;
    }
    IcpState *st = c->icp_state;
    if (st->pending) return CHIP_ERR_BUSY;
    st->collected = false;
    if (!st->stream) CHIP_HIP(c, hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    const int32_t S = p->sample_size;
    const int H = ransac_initial_iterations(p);
    size_t Ntot = 0;
    int words = 0;
    for (int i = 0; i < P; i++) { Ntot += (size_t)N[i]; const int w = (N[i] + 63) / 64; words = w > words ? w : words; }
    if (P > 0) {
        int rc = icp_reserve(c, st, dev_in ? 0 : Ntot, (size_t)P * (size_t)H, words);
        if (rc != CHIP_OK) return rc;
        hipStream_t s = st->stream;
        IcpProblem tab[kIcpMaxBatch];   // built here: a single estimation never touches the pinned table
        size_t off = 0;
        for (int i = 0; i < P; off += (size_t)N[i], i++) {
            IcpProblem &pr = tab[i];
            pr.N = N[i]; pr.pad_ = 0;
            pr.seed = seeds ? seeds[i] : p->seed;
            if (dev_in) {   // A[i] / B[i] ARE device memory (icp_ransac_device, the matched batch), read where they lie
                pr.A = A[i]; pr.B = B[i];
            } else {
                pr.A = st->A + 3 * off; pr.B = st->B + 3 * off;
                CHIP_HIP(c, hipMemcpyAsync(st->A + 3 * off, A[i], sizeof(double) * 3 * (size_t)N[i], hipMemcpyHostToDevice, s));
                CHIP_HIP(c, hipMemcpyAsync(st->B + 3 * off, B[i], sizeof(double) * 3 * (size_t)N[i], hipMemcpyHostToDevice, s));
            }
            for (int k = 0; k < kSampleMax; k++) {   // N - k >= 20 - 16 > 1 (ransac_check_params), so the quotient fits 64 bits
                const uint64_t d = (uint64_t)(N[i] - (k < S ? k : 0));
                pr.magic[k] = (uint64_t)((((unsigned __int128)1) << 64) / d);
            }
        }
        IcpLaunch l;
        l.S = S; l.H = H; l.thresh = p->error_thresh; l.use_mle = p->use_mle; l.mask_words = words;
        l.T_out = st->res.T.dev(); l.cost = st->res.cost.dev(); l.nin = st->res.nin.dev(); l.valid = st->res.valid.dev(); l.mask = st->res.mask.dev();
        l.T_dev = st->T_dev; l.valid_dev = st->valid_dev;
        l.sample_in = nullptr;
        if (p->sampler == CHIP_SAMPLER_THEIA_PERSISTENT) {   // one persistent permutation per problem, hypotheses 0..H-1 in order
            for (int i = 0; i < P; i++) {
                st->res.perm.resize((size_t)N[i]);
                ransac_sample_table_persistent(tab[i].seed, H, N[i], S, kSampleMax, st->res.perm.data(), st->res.sample_in.host() + (size_t)i * H * kSampleMax);
            }
            l.sample_in = st->res.sample_in.dev();
        }
        if (P == 1) {   // a single estimation: everything in the argument block, no table, no copy (which costs a call 3 - 4 us: profiles/icp_batch.md)
            IcpArgs a;
            a.pr = tab[0]; a.l = l;
            hipLaunchKernelGGL(icp_models, dim3((H + 63) / 64), dim3(64), 0, s, a);    // lane = hypothesis
            CHIP_HIP(c, hipGetLastError());
            hipLaunchKernelGGL(icp_score, dim3(H), dim3(64), 0, s, a);                 // wave = hypothesis
            CHIP_HIP(c, hipGetLastError());
        } else {
            std::memcpy(st->prob.host(), tab, sizeof(IcpProblem) * (size_t)P);   // pinned: the copy below reads it when the stream gets there
            CHIP_HIP(c, hipMemcpyAsync(st->prob_dev, st->prob.host(), sizeof(IcpProblem) * (size_t)P, hipMemcpyHostToDevice, s));
            IcpBatchArgs a;
            a.prob = st->prob_dev; a.l = l;
            hipLaunchKernelGGL(icp_models_batch, dim3((H + 63) / 64, P), dim3(64), 0, s, a);    // lane = hypothesis, blockIdx.y = problem
            CHIP_HIP(c, hipGetLastError());
            hipLaunchKernelGGL(icp_score_batch, dim3(H, P), dim3(64), 0, s, a);                 // wave = hypothesis
            CHIP_HIP(c, hipGetLastError());
        }
    }
    st->pending = true;
    st->pend_kind = kind;
    st->pend_P = P; st->pend_H = H; st->pend_words = words; st->pend_params = *p;
    for (int i = 0; i < P; i++) st->pend_N[i] = N[i];
    return CHIP_OK;
}

// waits for the pending launch and reports problem r of it into answer at[r] (null: r) of the caller's arrays
static int icp_collect_locked(Ctx *c, const int32_t *at, double *T_colmajor, float *confidence, uint8_t *const *inlier_mask, chip_ransac_summary *summary)
{
    IcpState *st = c->icp_state;
    CHIP_HIP(c, hipSetDevice(c->device));
    const hipError_t waited = st->pend_P > 0 ? hipStreamSynchronize(st->stream) : hipSuccess;
    st->pending = false;                 // also after a failed wait: the estimation is lost, the ctx takes the next one
    st->collected = st->pend_P > 0 && waited == hipSuccess;
    CHIP_HIP(c, waited);
    for (int r = 0; r < st->pend_P; r++) {
        const int i = at ? at[r] : r;
        ransac_report(&st->pend_params, st->pend_N[r], st->pend_H, st->pend_words, st->res, (size_t)r * st->pend_H, T_colmajor + 16 * (size_t)i,
                      confidence + i, inlier_mask ? inlier_mask[i] : nullptr, summary ? summary + i : nullptr);
    }
    return CHIP_OK;
}

static int icp_collect_single_locked(Ctx *c, double T_colmajor[16], float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary)
{
    IcpState *st = c->icp_state;
    if (!st || !st->pending || st->pend_kind != kIcpSingle) return CHIP_ERR_BUSY;
    uint8_t *masks[1] = {inlier_mask};
    return icp_collect_locked(c, nullptr, T_colmajor, confidence, masks, summary);
}

static int icp_check_args(const double *A, const double *B, int32_t N, const chip_ransac_params *p)
{
    if (!A || !B || !p) return CHIP_ERR_INVALID_ARG;
    return ransac_check_params(p, N);
}

extern "C" int chip_icp_ransac_enqueue(chip_ctx *c, const double *A, const double *B, int32_t N, const chip_ransac_params *p)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) c = static_cast<chip_ctx *>(chip::group_root(c));
    const int rc = icp_check_args(A, B, N, p);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> lk(c->icp_mu);
    return icp_enqueue_locked(c, 1, &A, &B, &N, p, nullptr, false, kIcpSingle);
}

extern "C" int chip_icp_ransac_collect(chip_ctx *c, double T_colmajor[16], float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary)
{
    if (!c || !T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    if (c->group) c = static_cast<chip_ctx *>(chip::group_root(c));
    std::lock_guard<std::mutex> lk(c->icp_mu);
    return icp_collect_single_locked(c, T_colmajor, confidence, inlier_mask, summary);
}

extern "C" int chip_icp_ransac_batch(chip_ctx *c, int32_t P, const double *const *A, const double *const *B, const int32_t *N,
                                     const chip_ransac_params *p, const uint64_t *seeds, double *T_colmajor, float *confidence,
                                     uint8_t *const *inlier_mask, chip_ransac_summary *summary)
{
    if (!c || P < 1 || !A || !B || !N || !p || !T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    if (P > kIcpMaxBatch) return CHIP_ERR_UNSUPPORTED;
    for (int i = 0; i < P; i++) {
        const int rc = icp_check_args(A[i], B[i], N[i], p);
        if (rc != CHIP_OK) return rc;
    }
    if (c->group) c = static_cast<chip_ctx *>(chip::group_root(c));
    std::lock_guard<std::mutex> lk(c->icp_mu);
    const int rc = icp_enqueue_locked(c, P, A, B, N, p, seeds, false, kIcpSingle);
    if (rc != CHIP_OK) return rc;
    return icp_collect_locked(c, nullptr, T_colmajor, confidence, inlier_mask, summary);
}

// a batch of one: the launch is the single pair
extern "C" int chip_icp_ransac(chip_ctx *c, const double *A, const double *B, int32_t N, const chip_ransac_params *p,
                               double T_colmajor[16], float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary)
{
    if (!c || !A || !B || !p || !T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    uint8_t *masks[1] = {inlier_mask};
    return chip_icp_ransac_batch(c, 1, &A, &B, &N, p, nullptr, T_colmajor, confidence, masks, summary);
}

// Test aid (cerebro_hip.h chip_debug_ransac_record, ICP leg): every hypothesis of problem `problem` of the last collected launch
int chip::icp_debug_record(Ctx *c, int32_t problem, chip_debug_ransac_shape *shape, int32_t *valid, double *cost, int32_t *nin, double *T_colmajor,
                           unsigned long long *mask)
{
    std::lock_guard<std::mutex> lk(c->icp_mu);
    IcpState *st = c->icp_state;
    if (!st || st->pending || !st->collected) return CHIP_ERR_BUSY;
    if (problem < 0 || problem >= st->pend_P) return CHIP_ERR_INVALID_ARG;
    CHIP_HIP(c, hipSetDevice(c->device));
    CHIP_HIP(c, hipStreamSynchronize(st->stream));
    const int32_t N = st->pend_N[problem];
    if (shape) { shape->P = st->pend_P; shape->H = st->pend_H; shape->N = N; shape->words = st->pend_words; shape->S = st->pend_params.sample_size; shape->sampler = st->pend_params.sampler; }
    ransac_record_copy(st->res, (size_t)problem * st->pend_H, st->pend_H, st->pend_words, N, valid, cost, nin, T_colmajor, mask);
    return CHIP_OK;
}

// chip_icp_ransac on sets that already are in device memory (match.hip): no staging copy, otherwise the same call
int chip::icp_ransac_device(Ctx *c, const double *A_dev, const double *B_dev, int32_t N, const chip_ransac_params *p, double *T_colmajor,
                            float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary)
{
    int rc = icp_check_args(A_dev, B_dev, N, p);
    if (rc != CHIP_OK) return rc;
    std::lock_guard<std::mutex> lk(c->icp_mu);
    rc = icp_enqueue_locked(c, 1, &A_dev, &B_dev, &N, p, nullptr, true, kIcpSingle);
    if (rc != CHIP_OK) return rc;
    return icp_collect_single_locked(c, T_colmajor, confidence, inlier_mask, summary);
}

// The enqueue half of chip_icp_ransac_matched_batch (match.hip, which holds match_mu and has answered the left-out problems'
// status): R validated problems on device-resident sets, one pair of launches; problem r is answer at[r] of the `total` the collect
// delivers.  R == 0 launches nothing.
int chip::icp_enqueue_device_batch(Ctx *c, int32_t R, const double *const *A_dev, const double *const *B_dev, const int32_t *N,
                                   const chip_ransac_params *p, const uint64_t *seeds, int32_t total, const int32_t *at)
{
    std::lock_guard<std::mutex> lk(c->icp_mu);
    const int rc = icp_enqueue_locked(c, R, A_dev, B_dev, N, p, seeds, true, kIcpMatchedBatch);
    if (rc != CHIP_OK) return rc;
    IcpState *st = c->icp_state;
    st->pend_total = total;
    for (int r = 0; r < R; r++) st->pend_at[r] = at[r];
    return CHIP_OK;
}

// A match call is about to rewrite the slabs: the kernels of a pending matched batch must have read them.  Its results are in pinned
// memory by then, so the batch stays collectable.  match_mu held (lock order match_mu -> icp_mu).
int chip::icp_wait_matched(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->icp_mu);
    IcpState *st = c->icp_state;
    if (!st || !st->pending || st->pend_kind != kIcpMatchedBatch || st->pend_P == 0) return CHIP_OK;
    CHIP_HIP(c, hipSetDevice(c->device));
    CHIP_HIP(c, hipStreamSynchronize(st->stream));
    return CHIP_OK;
}

extern "C" int chip_icp_ransac_matched_batch_collect(chip_ctx *c, double *T_colmajor, float *confidence, uint8_t *const *inlier_mask,
                                                     chip_ransac_summary *summary)
{
    if (!c || !T_colmajor || !confidence) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->icp_mu);
    IcpState *st = c->icp_state;
    if (!st || !st->pending || st->pend_kind != kIcpMatchedBatch) return CHIP_ERR_BUSY;
    // the left-out answer everywhere first; the problems that ran overwrite theirs (a left-out problem's mask is untouched)
    for (int i = 0; i < st->pend_total; i++) {
        for (int k = 0; k < 16; k++) T_colmajor[16 * (size_t)i + k] = NAN;
        confidence[i] = -1.f;
        if (summary) { std::memset(&summary[i], 0, sizeof summary[i]); summary[i].best_hypothesis = -1; }
    }
    return icp_collect_locked(c, st->pend_at, T_colmajor, confidence, inlier_mask, summary);
}
