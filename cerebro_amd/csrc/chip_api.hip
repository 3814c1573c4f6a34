// chip_api.hip -- C-ABI entry points of libcerebro_hip.so (see include/cerebro_hip.h for the contract and
// the reference lines each entry point replaces).  Host-side C++ over the HIP runtime; no torch, no CPU
// fallback: every compute entry point runs HIP kernels or fails with a CHIP_ERR_* status.
//
// This file holds the single-device context.  chip_multi.hip builds on its building blocks (declared in
// chip_internal.h): the in-library exchange of per-shard top-k lists over RCCL, and group contexts that drive the
// GPUs of one node from one process.  Entry points dispatch on ctx->group.
#include "chip_internal.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

using namespace chip;

extern "C" {

const char *chip_strerror(int status)
{
    switch (status) {
        case CHIP_OK: return "ok";
        case CHIP_ERR_INVALID_ARG: return "invalid argument";
        case CHIP_ERR_NO_DEVICE: return "no usable HIP device";
        case CHIP_ERR_HIP: return "HIP runtime error (see chip_last_hip_error)";
        case CHIP_ERR_OOM: return "out of device memory";
        case CHIP_ERR_NOT_F32: return "descriptor value not exactly representable as float32";
        case CHIP_ERR_NONFINITE: return "NaN/Inf in descriptor";
        case CHIP_ERR_RANGE: return "index / length out of range";
        case CHIP_ERR_UNSUPPORTED: return "unsupported configuration";
        case CHIP_ERR_TOO_FEW_POINTS: return "fewer than 20 correspondences";
        case CHIP_ERR_BUSY: return "async slot busy or empty";
        case CHIP_ERR_COMM: return "RCCL error (see chip_last_comm_error)";
        case CHIP_ERR_SHARD_FAILED: return "a shard could not take part in this tick / query (all ranks see this status); retry";
        case CHIP_ERR_GROUP_BROKEN: return "multi-GPU ctx is broken by an earlier partial failure; destroy it";
    }
    return "unknown status";
}

int chip_abi_version(void) { return CHIP_ABI_VERSION; }
int chip_build_scan_forms(void) { return scan_forms_built(); }
int chip_build_has_tick_coalesce(void) { return 1; }
int chip_build_test_hooks(void)
{
#ifdef CHIP_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
}

int chip_last_hip_error(const chip_ctx *ctx, const char **text)
{
    if (!ctx) return (int)hipErrorInvalidValue;
    const Ctx *c = ctx->group ? group_root(const_cast<chip_ctx *>(ctx)) : ctx;
    if (text) *text = hipGetErrorString(c->last_hip);
    return (int)c->last_hip;
}

void chip_dot_params_default(chip_dot_params *p)
{
    if (!p) return;
    p->locality = 12;                 // Cerebro.cpp:912
    p->thresh = (double)(float)0.85;  // Cerebro.cpp:913 (float) compared with double at :1056
    p->lag = 50;                      // Cerebro.cpp:914
    p->min_new = 3;                   // Cerebro.cpp:962
    p->min_k = 5;                     // Cerebro.cpp:1022
}

void chip_ransac_params_default(chip_ransac_params *p)
{
    if (!p) return;
    p->error_thresh = 0.03;        // DlsPnpWithRansac.cpp:208
    p->min_inlier_ratio = 0.7;     // :209
    p->max_iterations = 50;        // :210
    p->min_iterations = 5;         // :211
    p->use_mle = 1;                // :212
    p->sample_size = 15;           // DlsPnpWithRansac.h:45
    p->failure_probability = 0.01; // theia::RansacParameters default
    p->seed = 0x5EEDCE7EB80ULL;
    p->n_hypotheses = 0;
    p->sampler = CHIP_SAMPLER_FRESH;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ internals
namespace chip {

int env_int(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

static int ensure_capacity(Ctx *c, int64_t local_rows)
{
    // caller holds append_mu
    const int64_t need = (local_rows + c->seg_rows - 1) >> c->seg_shift;
    if (need > kMaxSegs) return CHIP_ERR_OOM;
    bool grew = false;
    // the segment table is about to change: no instance from here until the table is final (an instance reads the table through
    // caches nothing invalidates while it lives; rows of the new segment are published only after this function returns)
    ResidentPause paused(c, (int64_t)c->segs.size() < need);
    while ((int64_t)c->segs.size() < need) {
        void *p = nullptr;
        CHIP_HIP(c, hipMalloc(&p, (size_t)c->seg_rows * c->D * c->elem));
        {
            std::lock_guard<std::mutex> lk(c->mu);
            c->segs.push_back(p);
        }
        grew = true;
    }
    if (grew) {
        CHIP_HIP(c, hipMemcpyAsync(c->seg_table_dev, c->segs.data(), c->segs.size() * sizeof(void *), hipMemcpyHostToDevice, c->s_append));
        CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    }
    return CHIP_OK;
}

// (Re)allocate everything whose size depends on the storage type.  Only ever called on an EMPTY DB (create, or the automatic
// switch to double rows on the first append), with the append lock held or before the ctx is published.
static int configure_storage(Ctx *c, int elem)
{
    ResidentPause paused(c);
    for (void *p : c->segs) (void)hipFree(p);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->segs.clear();
    }
    c->ring_dev.release();
    c->qvec_dev.release();
    c->elem = elem;
    // segment geometry: power-of-two rows, ~512 MiB (float rows) / ~1 GiB (double rows) each
    int64_t rows = kSegBytesTarget / ((int64_t)c->D * 4);
    int shift = 0;
    while ((2ll << shift) <= rows) shift++;
    if (shift < 6) shift = 6;
    c->seg_shift = shift;
    c->seg_rows = 1ll << shift;
    CHIP_HIP(c, hipMemset(c->seg_table_dev, 0, kMaxSegs * sizeof(void *)));
    if (c->nranks > 1) {
        const int rc = c->ring_dev.reserve(c, (size_t)CHIP_RING_ROWS * c->D * elem);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipMemset(c->ring_dev, 0, (size_t)CHIP_RING_ROWS * c->D * elem));
    }
    return c->qvec_dev.reserve(c, (size_t)CHIP_MAX_NQ * c->D * elem);
}

// Drains the ctx, then destroys what is not memory.  The buffers the ctx owns (its DevBuf / PinnedBuf members) are freed by their destructors
// at the `delete c` at the end, the units' by their *_destroy: all of it after the drain and with the ctx's device still current, for every
// sub-context of a group as well (group_destroy comes here once per sub-context).
void ctx_destroy(chip_ctx *c)
{
    if (!c) return;
    if (c->group) { group_destroy(c); delete c; return; }
    (void)hipSetDevice(c->device);
    { std::lock_guard<std::mutex> qlk(c->query_mu); (void)coalesce_flush(c); }   // parked ticks run like every other enqueued tick
    resident_stop(c);
    (void)hipDeviceSynchronize();
    resident_destroy(c);
    exchange_destroy(c);
    pnp_destroy(c);
    icp_destroy(c);
    batch_destroy(c);
    match_destroy(c);
    frame_store_destroy(c);
    orb_destroy(c);
    for (void *p : c->segs) (void)hipFree(p);
    for (int i = 0; i < Ctx::kRing; i++) {
        if (c->ev_scan[i]) (void)hipEventDestroy(c->ev_scan[i]);
        if (c->ev_merged[i]) (void)hipEventDestroy(c->ev_merged[i]);
    }
    if (c->s_scan) (void)hipStreamDestroy(c->s_scan);
    if (c->s_scan2) (void)hipStreamDestroy(c->s_scan2);
    for (hipStream_t x : c->s_scan_x)
        if (x) (void)hipStreamDestroy(x);
    for (Slot &s : c->slots)
        if (s.done) (void)hipEventDestroy(s.done);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->own_query_stream && c->s_query) (void)hipStreamDestroy(c->s_query);
    if (c->s_append) (void)hipStreamDestroy(c->s_append);
    if (c->s_pnp) (void)hipStreamDestroy(c->s_pnp);
    delete c;
}

// Every variable that decides WHICH scan kernel a launch is, read in one place: chip_create and the device-free planner
// (chip_debug_scan_plan) both come here, so a plan is made under exactly the knobs a ctx created now would run under.
void scan_read_knobs(Ctx *c)
{
    c->scan_block = env_int("CHIP_SCAN_BLOCK", 0);   // 0 = chosen from D per launch (kernels.hip scan_shape)
    if (c->scan_block != 256 && c->scan_block != 512 && c->scan_block != 768 && c->scan_block != 1024) c->scan_block = 0;
    c->scan_blocks_per_cu = env_int("CHIP_SCAN_BPC", 2);
    if (c->scan_blocks_per_cu < 1) c->scan_blocks_per_cu = 1;
    c->scan_variant = env_int("CHIP_SCAN_VARIANT", 0);
    c->scan_rows = env_int("CHIP_SCAN_ROWS", 0);
    c->scan_claim = env_int("CHIP_SCAN_CLAIM", -1);   // -1 = auto (full-occupancy launches of the row-batched kernel), 0 = never, 1 = always
    c->tick_same_stream = env_int("CHIP_TICK_SAME_STREAM", 1) != 0;
    c->scan_short_bpc = env_int("CHIP_SCAN_SHORT_BPC", 1);
    c->scan_plain_bytes = (double)env_int("CHIP_SCAN_PLAIN_MIB", 768) * 1024 * 1024;
    c->scan_half_bytes = (double)env_int("CHIP_SCAN_HALF_MIB", 192) * 1024 * 1024;
    c->scan_sync_plain_bytes = (double)env_int("CHIP_SCAN_SYNC_PLAIN_MIB", 4096) * 1024 * 1024;
    c->scan_overlap_bytes = (double)env_int("CHIP_SCAN_OVERLAP_GIB", 8) * 1024 * 1024 * 1024;
    // a sharded ctx gets three small kernels per tick through its ctx stream underneath the scans: keep slots free for them
    c->scan_reserve = env_int("CHIP_SCAN_RESERVE", c->nranks > 1 ? 4 : 0);
    c->max_grid = 512;  // K2 (one 512-thread workgroup) keeps one partial list per thread
    c->scan_streams = env_int("CHIP_SCAN_STREAMS", c->nranks > 1 ? 2 : 4);   // tick streams (create_impl)
    c->tick_fused = env_int("CHIP_TICK_FUSED", 1) != 0;
}

static int create_impl(chip_ctx *c, int64_t capacity_hint, int elem)
{
    hipDeviceProp_t prop;
    CHIP_HIP(c, hipGetDeviceProperties(&prop, c->device));
    c->n_cus = prop.multiProcessorCount;
    std::strncpy(c->arch, prop.gcnArchName, sizeof(c->arch) - 1);
    if (std::strncmp(c->arch, "gfx950", 6) != 0 && !std::getenv("CHIP_ALLOW_ANY_ARCH")) return CHIP_ERR_NO_DEVICE;

    // The querier reads segs[] without c->mu (row_ptr_host) while the appender may open a new segment: reserve the whole
    // table (32 KiB) so that push_back never reallocates -- entries below the published length are immutable.
    c->segs.reserve(kMaxSegs);

    CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_query, hipStreamNonBlocking));
    CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_append, hipStreamNonBlocking));
    CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_pnp, hipStreamNonBlocking));
    int rc = c->seg_table_dev.alloc(c, kMaxSegs);
    if (rc == CHIP_OK) rc = configure_storage(c, elem);
    if (rc != CHIP_OK) return rc;
    c->stage_bytes = 64ull << 20;
    if (c->stage_bytes < (size_t)c->D * 8 * 64) c->stage_bytes = (size_t)c->D * 8 * 64;
    rc = c->stage_dev.alloc(c, c->stage_bytes);
    if (rc == CHIP_OK) rc = c->flags_dev.alloc(c, 1);
    if (rc == CHIP_OK) rc = c->flags_host.alloc(c, 1);
    if (rc == CHIP_OK) rc = c->norm2_dev.alloc(c, 1);
    if (rc == CHIP_OK) rc = c->norm2_host.alloc(c, 1);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemset(c->norm2_dev, 0, sizeof(unsigned long long)));
    *c->norm2_host.host() = 0;

    scan_read_knobs(c);
    CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_scan, hipStreamNonBlocking));
    {
        // Tick streams.  Short ticks of a plain ctx run scan + merge on ONE stream and rotate over up to four of them: a 10k-row tick
        // is ~37 us of scan, ~15 us of one-workgroup merge and ~12 us of launch / event gap per stream (rocprofv3 timeline,
        // profiles/r03_tick_timeline_10k.md), so two streams leave the memory system idle a third of the time.  Sharded / group
        // contexts (merge + exchange on the ctx stream) use the first two only.
        const int ns = c->scan_streams;
        if (ns >= 2) CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_scan2, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++)
            if (ns >= 3 + i) CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_scan_x[i], hipStreamNonBlocking));
    }
    for (int i = 0; i < Ctx::kRing; i++) {
        // [max_grid][CHIP_MAX_NQ][CHIP_MAX_TOPK] of one launch, or [ticks][max_grid][3][CHIP_MAX_TOPK] of a pass that serves several ticks (up to
        // kPassMaxTicks), and behind them the [kPassMaxTicks][3][CHIP_MAX_TOPK] exact lists tick_rescore leaves for the merge (coalesce_submit)
        constexpr size_t kListsPerGroup = 3 * kPassMaxTicks > CHIP_MAX_NQ ? 3 * kPassMaxTicks : CHIP_MAX_NQ;
        static_assert(kPassMaxTicks >= kMultiMaxTicks && kPassMaxTicks >= kPrefilterTicks, "the list buffers are sized for the deepest pass");
        rc = c->partial_dev[i].alloc(c, ((size_t)c->max_grid + 1) * kListsPerGroup * CHIP_MAX_TOPK);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipEventCreateWithFlags(&c->ev_scan[i], hipEventDisableTiming));
        CHIP_HIP(c, hipEventCreateWithFlags(&c->ev_merged[i], hipEventDisableTiming));
    }
    rc = c->tickets_dev.alloc(c, Ctx::kRing);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemset(c->tickets_dev, 0, Ctx::kRing * sizeof(int32_t)));
    // pipelined ticks that arrive while a long scan is running share one DB pass: at most this many per pass (0 = never; coalesce_* below)
    // (5 / 4: float rows whose shape has the fp16-query / the fp32 prefilter pass; every other ctx stops at what scan_multi_plan gives it)
    c->coalesce_max = env_int("CHIP_TICK_COALESCE", kPassMaxTicks);
    if (c->coalesce_max < 2) c->coalesce_max = 0;
    if (c->coalesce_max > kPassMaxTicks) c->coalesce_max = kPassMaxTicks;
    c->tick_poll = env_int("CHIP_TICK_POLL", 1) != 0;
    resident_read_knobs(c);
    rc = c->seq_all.alloc(c, CHIP_MAX_INFLIGHT);
    if (rc != CHIP_OK) return rc;
    std::memset(c->seq_all.host(), 0, sizeof(unsigned long long) * CHIP_MAX_INFLIGHT);
    rc = c->cert_all.alloc(c, CHIP_MAX_INFLIGHT * 4);
    if (rc != CHIP_OK) return rc;
    std::memset(c->cert_all.host(), 0, sizeof(uint32_t) * CHIP_MAX_INFLIGHT * 4);
    rc = c->topk.alloc(c, (size_t)CHIP_MAX_NQ * CHIP_MAX_TOPK);
    if (rc != CHIP_OK) return rc;
    for (Slot &s : c->slots) {
        CHIP_HIP(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        // pinned + mapped: the deciding workgroup stores the record here directly, no D2H copy kernel per tick
        rc = s.rec.alloc(c, 1);
        if (rc != CHIP_OK) return rc;
        s.seq_host = c->seq_all.host() + (&s - c->slots);
        s.seq_dev = c->seq_all.dev() + (&s - c->slots);
        s.cert_host = c->cert_all.host() + 4 * (&s - c->slots);
        s.cert_dev = c->cert_all.dev() + 4 * (&s - c->slots);
    }
    if (env_int("CHIP_SCAN_STAMPS", 0)) {
        rc = c->stamps_dev.alloc(c, (size_t)c->max_grid * 16 * 4 + 64);   // (+ 8 launch-wide stamps behind the waves')
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipMemset(c->stamps_dev, 0, ((size_t)c->max_grid * 16 * 4 + 64) * sizeof(unsigned long long)));
    }
    rc = pnp_create(c);
    if (rc != CHIP_OK) return rc;
    c->cap_hint = capacity_hint;
    if (capacity_hint > 0) {
        std::lock_guard<std::mutex> lk(c->append_mu);
        rc = ensure_capacity(c, local_count(c, capacity_hint));
        if (rc != CHIP_OK) return rc;
    }
    return CHIP_OK;
}

int ctx_create(chip_ctx **out, int32_t D, int64_t capacity_hint, int32_t device, int32_t shard_rank, int32_t shard_count, uint32_t flags)
{
    if (!out) return CHIP_ERR_INVALID_ARG;
    *out = nullptr;
    if (D <= 0 || shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count || capacity_hint < 0) return CHIP_ERR_INVALID_ARG;
    const uint32_t store = flags & kCreateStoreMask;
    if (store == kCreateStoreMask) return CHIP_ERR_INVALID_ARG;
    if (D % 4 != 0 || (size_t)D * 4 * CHIP_MAX_NQ > 160 * 1024) return CHIP_ERR_UNSUPPORTED;
    // double rows: two query descriptors (2 x D x 8 B) must fit the 160 KiB of LDS; further ones are read in place (db_scan_topk_wide).
    // D <= 10 240 for either storage type -- the reference's default 8192-D model included (Cerebro.cpp:1021)
    if (store == CHIP_CREATE_STORE_F64 && (size_t)D * 8 * 2 > 160 * 1024) return CHIP_ERR_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CHIP_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return CHIP_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return CHIP_ERR_NO_DEVICE;
    chip_ctx *c = new (std::nothrow) chip_ctx();
    if (!c) return CHIP_ERR_OOM;
    c->D = D;
    c->device = device;
    c->rank = shard_rank;
    c->nranks = shard_count;
    c->store_auto = store == 0;
    int rc = create_impl(c, capacity_hint, store == CHIP_CREATE_STORE_F64 ? 8 : 4);
    if (rc != CHIP_OK) { ctx_destroy(c); return rc; }
    *out = c;
    return CHIP_OK;
}

bool scan_policy(const Ctx *c, int64_t n_local, int nq, bool sync_tick, ScanArgs *a, int *grid)
{
    const double bytes = (double)n_local * c->D * c->elem;
    const bool short_scan = bytes <= c->scan_overlap_bytes;
    a->q64 = scan_q64(c, nq, !short_scan) ? 1 : 0;
    *grid = scan_grid_for(c, n_local, nq, a->q64 != 0);
    a->rows_form = scan_rows_form(c, n_local, nq, *grid, a->q64 != 0, sync_tick);
    a->plain_loads = bytes <= c->scan_plain_bytes ? 1 : 0;
    // rows claimed within the workgroup: measured -2 % on the synchronous 29k / 45k tick (two workgroups per CU), neutral at 10k (one
    // workgroup per CU: the launch is too short for the waves to drift apart) -- profiles/r05_short_scan.md
    a->dyn_claim = (a->rows_form == 1 && (c->scan_claim == 1 || (c->scan_claim < 0 && *grid > c->n_cus))) ? 1 : 0;
    return short_scan;
}

// fused tick: one launch (kernels.hip fused_tick_finish) -- same-stream short ticks through the row-batched kernel, decision wanted,
// no list output
bool scan_tick_fused(const Ctx *c, bool same_stream, const ScanArgs &a, bool decision_only, int nq)
{
    return same_stream && a.rows_form > 0 && c->tick_fused && decision_only && nq == 3;
}

bool tick_merge_on_scan_stream(const Ctx *c, bool tick, bool short_scan, bool second_tick_stream, bool caller_accepts)
{
    return tick && short_scan && !c->prof_on && c->nranks == 1 && !c->xchg && !c->parent && c->own_query_stream && second_tick_stream &&
           caller_accepts && c->tick_same_stream;
}

MergeArgs merge_args(const chip_topk_entry *in, int32_t n_lists, int32_t K, chip_topk_entry *out, chip_tick_result *result, int64_t l, const chip_dot_params *p)
{
    MergeArgs m;
    m.in = in;
    m.n_lists = n_lists;
    m.K = K;
    m.out = out;
    m.result = result;
    m.l = l;
    m.locality = p ? p->locality : 0;
    m.thresh = p ? p->thresh : 0.0;
    return m;
}

int prof_begin(Ctx *c, hipStream_t s, double bytes, hipEvent_t *stop)
{
    while (c->prof_used + 2 > c->prof_ev.size()) {
        hipEvent_t e;
        CHIP_HIP(c, hipEventCreate(&e));
        c->prof_ev.push_back(e);
    }
    hipEvent_t start = c->prof_ev[c->prof_used];
    *stop = c->prof_ev[c->prof_used + 1];
    c->prof_used += 2;
    c->prof_bytes_last = bytes;
    CHIP_HIP(c, hipEventRecord(start, s));
    return CHIP_OK;
}

// Enqueue K1 (scan + per-workgroup top-k, on s_scan) and K2 (cross-workgroup merge [+ accept decision], on the ctx
// stream behind an event) for rq.nq queries over the global prefix [0,rq.k).  rq.out (device or pinned host, optional) gets
// [nq][K]; rq.res (optional) the decision record of Cerebro.cpp:1056.  Consecutive calls pipeline: scans run back to
// back on s_scan while the previous merge (and whatever the caller enqueues after it on the ctx stream) proceeds.
int enqueue_scan_merge(Ctx *c, const ScanRequest &rq, ScanReceipt *rcpt)
{
    const int b = (int)(c->n_enqueued++ % Ctx::kRing);
    // Ticks (queries already resident) over a short prefix alternate between two scan streams so that the ramp-down of
    // one launch overlaps the ramp-up of the next (measured, 1 -> 2 streams: 10k rows 45 -> 38 us/tick, 60k 172 -> 153,
    // 125k 317 -> 308, 500k 1191 -> 1157; at 1M the gain is < 1 %, and launches that overlap would no longer have a
    // meaningful per-launch duration for the roofline, so long scans and profiled runs stay on one stream).  Anything that
    // uploads its queries on s_scan first stays on s_scan.
    ScanArgs a;
    int grid = 0;
    const int nq = rq.nq;
    const bool short_scan = scan_policy(c, local_count(c, rq.k), nq, rq.tick && rq.sync_tick, &a, &grid);
    hipStream_t s_scan = (rq.tick && short_scan && !c->prof_on && c->s_scan2 && (c->n_enqueued & 1)) ? c->s_scan2 : c->s_scan;
    // (same-stream short ticks rotate over all tick streams: see below)
    const bool same_stream = tick_merge_on_scan_stream(c, rq.tick, short_scan, c->s_scan2 != nullptr, rq.merge_on_scan_stream);
    if (same_stream) {
        hipStream_t ring[4] = {c->s_scan, c->s_scan2, c->s_scan_x[0], c->s_scan_x[1]};
        int ns = 2;
        while (ns < 4 && ring[ns]) ns++;
        s_scan = ring[c->n_same_stream++ % (uint64_t)ns];
    }
    scan_args_db(c, &a);
    a.n_rows = local_count(c, rq.k);
    a.K = rq.K;
    for (int i = 0; i < CHIP_MAX_NQ; i++) a.q[i] = i < nq ? rq.q[i] : nullptr;
    a.idx_mul = c->nranks;
    a.idx_add = c->nranks == 1 ? 0 : c->rank;
    a.partial = c->partial_dev[b];
    a.stamps = c->stamps_dev;
    const bool fused = scan_tick_fused(c, same_stream, a, rq.res != nullptr && rq.out == nullptr && rq.p != nullptr, nq);
    if (fused) {
        a.K = 1;
        a.fused_result = rq.res;
        a.fused_ticket = c->tickets_dev + b;
        a.tick_l = rq.l;
        a.locality = rq.p->locality;
        a.thresh = rq.p->thresh;
        a.fused_seq = rq.seq_dev;            // (nullptr unless the caller asked for a pollable completion)
        a.fused_seq_val = rq.seq_val;
    }

    // The merge that last read this buffer ran kRing ticks ago; only when it is not already complete (a stalled ctx
    // stream) does the scan stream need a barrier packet -- in steady state this costs nothing.
    if (hipEventQuery(c->ev_merged[b]) != hipSuccess) CHIP_HIP(c, hipStreamWaitEvent(s_scan, c->ev_merged[b], 0));
    hipEvent_t e1 = nullptr;
    int rc = c->prof_on ? prof_begin(c, s_scan, (double)a.n_rows * c->D * c->elem, &e1) : CHIP_OK;
    if (rc == CHIP_OK) rc = launch_scan(c, s_scan, a, nq, grid);
    if (rc != CHIP_OK) return rc;
    if (e1) CHIP_HIP(c, hipEventRecord(e1, s_scan));
    // Short ticks of a plain single-GPU ctx keep the merge on the scan's OWN stream: the tick is then two launches and two event
    // records on one stream (no cross-stream event pair), and because consecutive ticks alternate between the two scan streams,
    // merge(i) still overlaps scan(i+1).  At 10k rows the tick is host-enqueue-bound otherwise (round 2: 21-34 us of API calls per
    // tick against a ~20 us kernel).  Anything with an exchange, an external ctx stream or profiling keeps the ctx-stream merge.
    hipStream_t s_merge = same_stream ? s_scan : c->s_query;
    if (rcpt) { rcpt->merge_stream = s_merge; rcpt->fused = fused; rcpt->done_ev = same_stream ? c->ev_merged[b] : nullptr; }   // same-stream tick: the merge event (recorded below) IS the tick's completion event
    if (!same_stream) {
        CHIP_HIP(c, hipEventRecord(c->ev_scan[b], s_scan));
        if (rq.tick && !short_scan) { c->pass_ev = c->ev_scan[b]; c->pass_shared = false; c->pass_no++; }   // the scan later ticks may park behind (coalesce_*)
        if (c->ring_dev) c->last_scan_ev[s_scan == c->s_scan2 ? 1 : 0] = c->ev_scan[b];   // caller holds ring_mu (RingGuard)
        CHIP_HIP(c, hipStreamWaitEvent(c->s_query, c->ev_scan[b], 0));
    }

    if (fused) {   // the scan's last workgroup has written the decision record: the scan's end IS the tick's end
        CHIP_HIP(c, hipEventRecord(c->ev_merged[b], s_scan));
        return CHIP_OK;
    }
    rc = launch_merge(c, s_merge, merge_args(c->partial_dev[b], grid, rq.K, rq.out, rq.res, rq.l, rq.p), nq);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipEventRecord(c->ev_merged[b], s_merge));
    return CHIP_OK;
}

// Pointers of the query rows (device).  Single GPU: straight into the DB; sharded: the replicated ring.
// Sharded ctx: the query rows of a scan are read from the replicated ring, which the appender overwrites in place.  A
// querier holds ring_mu from the residency check until the scan's completion event is recorded (RingGuard); the appender
// announces the length its call will reach (rows_pending) and picks up the newest scan events under the same lock before it
// touches the ring, and its ring writes wait for those scans.  So a scan either was validated against the post-append
// length, or is ordered before the ring writes.
int query_row_ptrs(Ctx *c, const int64_t *rows, int nq, int64_t n_global, const void **q)
{
    int64_t total;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        total = c->rows_global;
    }
    for (int i = 0; i < nq; i++) {
        const int64_t g = rows[i];
        if (g < 0 || g >= n_global || g >= total) return CHIP_ERR_RANGE;
        if (c->nranks == 1) {
            q[i] = row_ptr_host(c, g);
        } else {
            // no longer in the replicated ring -- counting the rows of an append that is in flight right now
            const int64_t horizon = c->rows_pending > total ? c->rows_pending : total;
            if (g < horizon - CHIP_RING_ROWS) return CHIP_ERR_RANGE;
            q[i] = ring_ptr(c, g);
        }
    }
    return CHIP_OK;
}

// External query vectors -> qvec_dev in the storage type, on the scan stream: K1 reads them there (the previous synchronous
// call has fully drained, so no WAR hazard).  float <-> double conversion of a few rows is done on the host: widening is
// exact; narrowing double queries for a float DB must be lossless ((double)(float)x == x) or the call fails.
int upload_query_vectors(Ctx *c, const void *queries, int src_elem, int nq, const void **q)
{
    const size_t n = (size_t)nq * c->D;
    if (src_elem == c->elem) {
        CHIP_HIP(c, hipMemcpyAsync(c->qvec_dev, queries, n * c->elem, hipMemcpyHostToDevice, c->s_scan));
    } else {
        c->qconv.resize(n * c->elem);
        if (c->elem == 8) {
            double *d = reinterpret_cast<double *>(c->qconv.data());
            const float *s = static_cast<const float *>(queries);
            for (size_t i = 0; i < n; i++) d[i] = (double)s[i];
        } else {
            float *d = reinterpret_cast<float *>(c->qconv.data());
            const double *s = static_cast<const double *>(queries);
            for (size_t i = 0; i < n; i++) {
                d[i] = (float)s[i];
                if (!((double)d[i] == s[i])) return std::isfinite(s[i]) ? CHIP_ERR_NOT_F32 : CHIP_ERR_NONFINITE;
            }
        }
        CHIP_HIP(c, hipMemcpyAsync(c->qvec_dev, c->qconv.data(), n * c->elem, hipMemcpyHostToDevice, c->s_scan));
        CHIP_HIP(c, hipStreamSynchronize(c->s_scan));   // qconv is pageable and reused
    }
    for (int i = 0; i < nq; i++) q[i] = c->qvec_dev + (size_t)i * c->D * c->elem;
    return CHIP_OK;
}

// Host part of the tick (Cerebro.cpp:960-966, :1019-1022).  Returns CHIP_TICK_* in *status.  last_l is NOT written here:
// the caller commits it once the tick has actually been enqueued (or at once for TOO_SHORT), so a failed enqueue leaves the
// state as the reference's loop would (it only reaches :1098 at the end of an executed pass).
int tick_prepare(int64_t n, int64_t last_l, int64_t l, const chip_dot_params *p, int32_t *status, int64_t *k_out)
{
    if (l < 0 || l > n) return CHIP_ERR_RANGE;
    if (l - last_l < p->min_new) { *status = CHIP_TICK_SKIPPED; return CHIP_OK; }  // :962-966, last_l untouched
    if (l < 3) return CHIP_ERR_RANGE;  // needs descriptors l-1, l-2, l-3 (:987-989)
    const int64_t k = l - p->lag;      // :1019
    *k_out = k;
    *status = (k > p->min_k) ? CHIP_TICK_SCANNED : CHIP_TICK_TOO_SHORT;  // :1022
    return CHIP_OK;
}

void fill_immediate(chip_tick_result *r, int32_t status)
{
    std::memset(r, 0, sizeof *r);
    r->status = status;
    r->idx_curr = r->idx_prev = -1;
    for (int q = 0; q < 3; q++) { r->argmax[q] = -1; r->maxv[q] = -INFINITY; }
}

int64_t published_rows(const Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->mu);
    return c->rows_global;
}

int tick_begin(Slot &s, int64_t n_rows, int64_t *last_l, int64_t l, const chip_dot_params *p, int32_t *status, int64_t *k)
{
    if (s.state != SlotState::Free) return CHIP_ERR_BUSY;
    const int rc = tick_prepare(n_rows, *last_l, l, p, status, k);
    if (rc != CHIP_OK) return rc;
    s.prev_last_l = *last_l;
    s.prefilter = false;
    s.tick_l = l;
    s.last_l_ptr = last_l;
    if (*status != CHIP_TICK_SCANNED) {
        if (*status == CHIP_TICK_TOO_SHORT) *last_l = l;   // :1098 (the else-branch of :1022 still ends the pass)
        fill_immediate(s.rec.host(), *status);
        s.state = SlotState::Immediate;
    }
    return CHIP_OK;
}

// One tick as a pass of its own: scan (K1) + merge and decision (K2), the slot's completion event.  query_mu held.
static int tick_submit(Ctx *c, int64_t k, int64_t l, const chip_dot_params *p, const void *const *q, bool sync_tick, Slot &s)
{
    ScanRequest rq;
    rq.k = k; rq.q = q; rq.nq = 3; rq.K = CHIP_DEFAULT_TOPK;
    rq.res = s.rec.dev(); rq.l = l; rq.p = p;
    rq.tick = true; rq.sync_tick = sync_tick; rq.merge_on_scan_stream = true;
    if (c->tick_poll) { s.seq_want = ++c->tick_seq; rq.seq_dev = s.seq_dev; rq.seq_val = s.seq_want; }
    ScanReceipt done;
    const int rc = enqueue_scan_merge(c, rq, &done);
    if (rc != CHIP_OK) return rc;
    // a same-stream tick is complete when its merge is: one event record per tick (the list buffer's merge event; the buffer is
    // not reused before kRing = 64 further enqueues, and at most CHIP_MAX_INFLIGHT - 1 = 63 ticks are uncollected)
    if (done.done_ev) s.wait_ev = done.done_ev;
    else { CHIP_HIP(c, hipEventRecord(s.done, done.merge_stream)); s.wait_ev = s.done; }
    s.pass_no = c->pass_no;
    s.state = c->tick_poll && done.fused ? SlotState::Poll : SlotState::Event;   // the fused kernel stores the completion word itself
    return CHIP_OK;
}

// ---- several pipelined ticks per DB pass ----
// A caller that keeps ticks in flight (chip_loop_tick_enqueue ahead of chip_loop_tick_collect) has the library stream the same
// prefix once per tick.  Ticks do not depend on one another (status and last_l are settled at enqueue, the query rows are
// published rows), so T of them can share ONE pass with 3 T queries (kernels.hip db_scan_topk_multi): an enqueue that finds a
// scan of this ctx still running PARKS its tick instead of launching it, and parked ticks leave together.
//   * nothing running, nothing parked: the tick is launched at once, alone, exactly as before;
//   * a scan running: park; the T_max-th parked tick sends all of them off as one pass;
//   * nothing stays parked while its caller can no longer release it -- see coalesce_flush's callers (listed in cerebro_hip.h).
// Only long scans (beyond scan_overlap_bytes: the launches that run alone on the scan stream) of a plain single-GPU ctx on its
// own streams, float or double rows (scan_multi_plan says which D).  The synchronous tick, the fused / resident short ticks and the paced figures never come here.
int coalesce_decide(int n_parked, int t_max, bool scan_running)
{
    if (t_max < 2) return kCoalesceLaunch;
    if (!scan_running) return n_parked > 0 ? kCoalesceParkFlush : kCoalesceLaunch;   // the scan they parked behind has ended: leave with this one
    return n_parked + 1 >= t_max ? kCoalesceParkFlush : kCoalescePark;
}

// most ticks a pass over [0, k) may serve on this ctx; 0: the tick does not coalesce
static int coalesce_ticks_max(const Ctx *c, int64_t k, bool sync_tick)
{
    if (c->coalesce_max < 2 || sync_tick || c->nranks != 1 || c->xchg || c->parent || c->group || !c->own_query_stream) return 0;
    if ((double)k * c->D * c->elem <= c->scan_overlap_bytes) return 0;
    int fit = scan_multi_max_ticks(c);
    if (c->coalesce_max >= kPrefilterTicks && scan_prefilter_usable(c)) fit = kPrefilterTicks;   // four leave as one prefilter pass
    if (c->coalesce_max >= kHalfqTicks && scan_halfq_usable(c)) fit = kHalfqTicks;               // five: the same with fp16-staged queries
    const int t = fit < c->coalesce_max ? fit : c->coalesce_max;
    return t >= 2 ? t : 0;
}

// T >= 2 parked ticks as one pass: one launch of db_scan_topk_multi / db_scan_shared_f64 on the scan stream, then K2 once per tick on the ctx stream,
// each on its own block of lists and followed by its slot's completion event.
// T >= kPrefilterTicks: the pass is db_scan_prefilter (four) or db_scan_halfq (five), and on the ctx stream ONE launch of tick_rescore (certificate + exact scores of the
// proven candidates -> one list per tick and query) goes in front of the ticks' K2 launches; the slot remembers the tick, and a collect
// that finds a certificate word that does not say "holds" runs the tick again alone (tick_collect_slot).
static int coalesce_submit(Ctx *c, int first, int T)
{
    const Ctx::ParkedTick *parked = c->parked + first;   // the pass serves parked[first .. first + T)
    const int b = (int)(c->n_enqueued++ % Ctx::kRing);
    const int K = CHIP_DEFAULT_TOPK;
    const bool prefilter = T >= kPrefilterTicks, halfq = T == kHalfqTicks;
    static_assert(kPrefilterTicks > kMultiMaxTicks && kHalfqTicks == kPrefilterTicks + 1, "passes of four and five ticks are the prefilters'");
    PassArgs a{};
    scan_args_db(c, &a);
    a.K = K;
    a.partial = c->partial_dev[b];
    for (int t = 0; t < T; t++) {
        a.k[t] = parked[t].k;
        if (a.k[t] > a.n_rows) a.n_rows = a.k[t];
        for (int i = 0; i < 3; i++) a.q[3 * t + i] = parked[t].q[i];
    }
    const int grid = scan_multi_grid(c);
    double E = 0.0;
    int e = 0;
    if (prefilter) {
        std::lock_guard<std::mutex> lk(c->mu);
        if (halfq) {   // the scale of the staged queries and the bound that goes with it, from ONE reading of the norm bound
            e = halfq_exponent(c->row_norm_max);
            a.q_up = std::ldexp(1.0f, e);
            a.s_up = std::ldexp(1.0, e);
            a.s_down = std::ldexp(1.0, -e);
            E = halfq_error_bound(c->D, c->row_norm_max, e);
        } else {
            E = prefilter_error_bound(c->D, c->row_norm_max);
        }
    }
    if (hipEventQuery(c->ev_merged[b]) != hipSuccess) CHIP_HIP(c, hipStreamWaitEvent(c->s_scan, c->ev_merged[b], 0));
    hipEvent_t e1 = nullptr;   // one event pair per pass; a pass reads the prefix once
    int rc = c->prof_on ? prof_begin(c, c->s_scan, (double)a.n_rows * c->D * c->elem, &e1) : CHIP_OK;
    if (rc == CHIP_OK)
        rc = halfq ? launch_scan_halfq(c, c->s_scan, a, grid) : prefilter ? launch_scan_prefilter(c, c->s_scan, a, grid) : launch_scan_multi(c, c->s_scan, a, T, grid);
    if (rc != CHIP_OK) return rc;
    if (e1) CHIP_HIP(c, hipEventRecord(e1, c->s_scan));
    CHIP_HIP(c, hipEventRecord(c->ev_scan[b], c->s_scan));
    c->pass_ev = c->ev_scan[b];
    c->pass_shared = true;
    c->pass_no++;
    CHIP_HIP(c, hipStreamWaitEvent(c->s_query, c->ev_scan[b], 0));
    chip_topk_entry *exact = c->partial_dev[b] + (size_t)kPassMaxTicks * grid * 3 * K;   // [tick][3][K], behind the pass's lists
    if (prefilter) {
        RescoreArgs ra{};
        ra.seg_table = a.seg_table; ra.seg_shift = a.seg_shift; ra.seg_mask = a.seg_mask; ra.D = a.D; ra.K = K;
        ra.in = c->partial_dev[b]; ra.n_lists = grid; ra.wpb = 8;   // (kMultiBlock / 64 waves per workgroup)
        ra.E = E;
        ra.out = exact;
        for (int t = 0; t < T; t++) {
            const Ctx::ParkedTick &pt = parked[t];
            Slot &s = *pt.slot;
            ra.k[t] = pt.k;
            for (int i = 0; i < 3; i++) { ra.q[3 * t + i] = s.pf_q[i] = pt.q[i]; s.cert_host[i] = 0; }
            ra.cert[t] = s.cert_dev;
            s.prefilter = true; s.pf_k = pt.k; s.pf_p = pt.p;
        }
        rc = launch_rescore(c, c->s_query, ra, T);
        if (rc != CHIP_OK) return rc;
        Ctx::LastPass &lp = c->last_pass;   // what chip_debug_last_pass reads back
        lp.family = halfq ? CHIP_SCAN_FAMILY_HALFQ : CHIP_SCAN_FAMILY_PREFILTER;
        lp.ticks = T; lp.grid = grid; lp.wpb = ra.wpb; lp.K = K; lp.e = e; lp.ring = b; lp.E = E;
        for (int t = 0; t < T; t++) { lp.k[t] = parked[t].k; lp.cert[t] = parked[t].slot->cert_host; }
    }
    if (halfq) {   // one K2 launch for the five ticks (kernels.hip pass_merge): workgroup t is topk_merge<3> on tick t's lists
        PassMergeArgs m{};
        m.in = exact;
        m.K = K;
        for (int t = 0; t < T; t++) {
            const MergeArgs mt = merge_args(exact + (size_t)t * 3 * K, 1, K, nullptr, parked[t].slot->rec.dev(), parked[t].l, &parked[t].p);
            m.result[t] = mt.result; m.l[t] = mt.l; m.locality[t] = mt.locality; m.thresh[t] = mt.thresh;
        }
        rc = launch_pass_merge(c, c->s_query, m, T);
        if (rc != CHIP_OK) return rc;
    }
    for (int t = 0; t < T; t++) {
        const Ctx::ParkedTick &pt = parked[t];
        if (halfq) rc = CHIP_OK;
        else if (prefilter) rc = launch_merge(c, c->s_query, merge_args(exact + (size_t)t * 3 * K, 1, K, nullptr, pt.slot->rec.dev(), pt.l, &pt.p), 3);
        else rc = launch_merge(c, c->s_query, merge_args(c->partial_dev[b] + (size_t)t * grid * 3 * K, grid, K, nullptr, pt.slot->rec.dev(), pt.l, &pt.p), 3);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipEventRecord(pt.slot->done, c->s_query));
        pt.slot->wait_ev = pt.slot->done;
        pt.slot->state = SlotState::Event;
        pt.slot->pass_no = c->pass_no;
    }
    CHIP_HIP(c, hipEventRecord(c->ev_merged[b], c->s_query));
    c->coalesce_passes++;
    c->coalesce_ticks += T;
    if (prefilter) { c->prefilter_passes++; c->prefilter_ticks += T; }
    return CHIP_OK;
}

int coalesce_flush(Ctx *c)
{
    const int T = c->n_parked;
    if (T == 0) return CHIP_OK;
    c->n_parked = 0;
    const Ctx::ParkedTick &p0 = c->parked[0];
    int rc;
    if (T == kHalfqTicks && !scan_halfq_usable(c)) {           // a row appended since they parked took the norm bound out of range: three and two
        rc = coalesce_submit(c, 0, kMultiMaxTicks);
        if (rc == CHIP_OK) rc = coalesce_submit(c, kMultiMaxTicks, T - kMultiMaxTicks);
    } else if (T == kPrefilterTicks && !scan_prefilter_usable(c)) {   // likewise: three and one
        const Ctx::ParkedTick &pl = c->parked[T - 1];
        rc = coalesce_submit(c, 0, T - 1);
        if (rc == CHIP_OK) rc = tick_submit(c, pl.k, pl.l, &pl.p, pl.q, false, *pl.slot);
    } else {
        rc = T == 1 ? tick_submit(c, p0.k, p0.l, &p0.p, p0.q, false, *p0.slot) : coalesce_submit(c, 0, T);
    }
    for (int t = 0; t < T && rc != CHIP_OK; t++) {   // the enqueue has long returned: the tick's collect reports it
        c->parked[t].slot->state = SlotState::Failed;
        c->parked[t].slot->err = rc;
    }
    return rc;
}

static int tick_enqueue_slot(Ctx *c, int64_t l, const chip_dot_params *p, bool sync_tick, Slot &s)
{
    int32_t status = 0;
    int64_t k = 0;
    // With an exchange attached the ranks may see different published lengths (each has its own appender): l > n on THIS rank is
    // then not a reason to leave the collective call -- the rank takes part with the failure mark (xchg_tick_enqueue).
    const int64_t n_pub = published_rows(c);
    int rc = tick_begin(s, c->xchg ? INT64_MAX : n_pub, &c->last_l, l, p, &status, &k);
    if (rc != CHIP_OK || status != CHIP_TICK_SCANNED) return rc;
    if (c->xchg) {   // sharded ctx with its exchange inside the library: scan -> local merge -> all-gather -> merge + decision
        rc = xchg_tick_enqueue(c, l, k, p, sync_tick, s, l > n_pub);
        if (rc != CHIP_OK) return rc;
    } else {
        const int64_t rows[3] = {l - 1, l - 2, l - 3};  // v, vm, vmm (:987-989)
        const void *q[3];
        RingGuard rg(c);
        rc = query_row_ptrs(c, rows, 3, l, q);
        if (rc != CHIP_OK) return rc;
        if (resident_eligible(c, k)) {
            (void)coalesce_flush(c);
            rc = resident_tick_enqueue(c, k, l, p, s);
            if (rc == CHIP_OK) { c->last_l = l; return CHIP_OK; }   // :1098
            if (rc != CHIP_ERR_UNSUPPORTED && rc != kResidentPaused) return rc;   // (no resident form on this ctx, or paused: launch the tick)
        }
        int t_max = coalesce_ticks_max(c, k, sync_tick);
        // The pipeline fills behind a tick launched alone: the pass parked behind THAT scan takes four, five only behind a shared pass.  A
        // long run loses nothing by it (1 + 4 + 5 + 5 + ... is as many scans as 1 + 5 + 5 + ... + 4), and a burst of up to 17 ticks with 16 in
        // flight leaves as 1 + 4 + 5 + 5 + 2 and not as 1 + 5 + 5 + 5 + 1: its last tick shares a pass instead of reading the prefix alone,
        // and callers that count the passes of such a burst see what they saw with four per pass.
        if (t_max == kHalfqTicks && !c->pass_shared && !c->coalesce_force) t_max = kPrefilterTicks;
        const int act = t_max < 2 ? kCoalesceLaunch
                                  : coalesce_decide(c->n_parked, t_max, c->coalesce_force || (c->pass_ev && hipEventQuery(c->pass_ev) == hipErrorNotReady));
        if (act == kCoalesceLaunch) {
            (void)coalesce_flush(c);   // submission order stays call order (a failure is reported by the collects of the ticks it concerns)
            rc = tick_submit(c, k, l, p, q, sync_tick, s);
            if (rc != CHIP_OK) return rc;
        } else {
            Ctx::ParkedTick &pt = c->parked[c->n_parked++];
            pt.slot = &s; pt.k = k; pt.l = l; pt.p = *p;
            for (int i = 0; i < 3; i++) pt.q[i] = q[i];
            s.state = SlotState::Parked;
            if (act == kCoalesceParkFlush) (void)coalesce_flush(c);
        }
    }
    c->last_l = l;                     // :1098
    return CHIP_OK;
}

int tick_collect_slot(Ctx *c, Slot &s, chip_tick_result *out)
{
    // A parked tick leaves now (with whatever is parked next to it).  A collect that is about to block on the NEWEST pass submitted
    // sends the parked ticks off first: nothing is queued behind that pass, and the GPU would run dry until the caller returns.
    if (s.state == SlotState::Parked) (void)coalesce_flush(c);
    else if (c->n_parked > 0 && (s.state == SlotState::Event || s.state == SlotState::Poll) && s.pass_no == c->pass_no &&
             hipEventQuery(s.wait_ev) == hipErrorNotReady)
        (void)coalesce_flush(c);
    switch (s.state) {
    case SlotState::Free:
    case SlotState::Parked:      // (coalesce_flush leaves no slot parked)
        return CHIP_ERR_BUSY;
    case SlotState::Failed:      // the pass this tick was part of could not be submitted: as a tick whose enqueue had failed
        s.state = SlotState::Free;
        if (s.last_l_ptr && *s.last_l_ptr == s.tick_l) *s.last_l_ptr = s.prev_last_l;
        return s.err;
    case SlotState::Immediate:
        break;
    case SlotState::Resident: {
        const int rc = resident_collect(c, s);
        if (rc != CHIP_OK) { s.state = SlotState::Free; return rc; }
        break;
    }
    case SlotState::Poll: {
        // A fused tick's last workgroup writes the record into the slot's pinned host memory and THEN stores the slot's completion word
        // with a system-scope release: polling that word (acquire) hands the record over ~4-5 us before the stream's event would -- the
        // end-of-kernel cache maintenance, the event's barrier packet and its signal are off the synchronous tick's critical path.  The
        // event is still recorded (it orders the reuse of the list buffer); it is only waited for if the word does not arrive.
        bool done = false;
        const volatile unsigned long long *w = s.seq_host;
        for (long spin = 0; spin < (1L << 24) && !done; spin++) {
            done = __atomic_load_n(w, __ATOMIC_ACQUIRE) == s.seq_want;
            if (!done && (spin & 0x3fff) == 0x3fff && hipEventQuery(s.wait_ev) != hipErrorNotReady) break;   // finished or failed: let the event say which
        }
        if (done) break;
    }
        [[fallthrough]];   // the word did not arrive
    case SlotState::Event:
        CHIP_HIP(c, hipEventSynchronize(s.wait_ev));   // (a failure leaves the slot as it is)
        break;
    }
    if (s.prefilter) {
        // The tick left with a prefilter pass.  Its record stands if tick_rescore proved, for all three queries, that the rows it scored
        // exactly hold the exact top-K; if not (scores closer together than the fp32 error bound, or more candidates than it scores), the
        // tick runs again alone through the exact scan, and that record is the caller's.
        s.prefilter = false;
        if (s.cert_host[0] != 1u || s.cert_host[1] != 1u || s.cert_host[2] != 1u) {
            c->prefilter_uncertified++;
            (void)coalesce_flush(c);   // submission order stays call order
            const int rc = tick_submit(c, s.pf_k, s.tick_l, &s.pf_p, s.pf_q, false, s);
            if (rc != CHIP_OK) { s.state = SlotState::Free; return rc; }
            CHIP_HIP(c, hipEventSynchronize(s.wait_ev));
        }
    }
    *out = *s.rec.host();
    s.state = SlotState::Free;
    if (out->status == CHIP_TICK_FAILED) {   // a shard could not take part: the tick had no effect (:1098 was not reached)
        // Roll last_l back only while this tick is still the newest one enqueued.  With ticks pipelined, a later tick may have been
        // enqueued (and may succeed) meanwhile: its commit of last_l stands, exactly as if the reference's sequential loop had
        // skipped the failed pass and run the next one.
        if (s.last_l_ptr && *s.last_l_ptr == s.tick_l) *s.last_l_ptr = s.prev_last_l;
        else if (s.last_l_ptr) {
            // A newer tick was enqueued on top of this failed one.  Should IT fail too, it must not roll back to this tick's l (a pass
            // that never reached :1098): hand it this tick's predecessor instead, so that a run of failed ticks unwinds to the last_l
            // of the newest tick that did not fail.  The successor is the in-flight slot whose prev_last_l is this l.
            for (Slot &o : c->slots)
                if (&o != &s && o.state != SlotState::Free && o.last_l_ptr == s.last_l_ptr && o.prev_last_l == s.tick_l) o.prev_last_l = s.prev_last_l;
        }
        fill_immediate(out, CHIP_TICK_FAILED);
        return CHIP_ERR_SHARD_FAILED;
    }
    return CHIP_OK;
}

int sync_topk_out(Ctx *c, int nq, int K, double *scores, int64_t *idx)
{
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));  // the last block stored the list into pinned host memory
    if (c->topk.host()[0].idx == -2) return CHIP_ERR_SHARD_FAILED;   // kFailedShardIdx: a shard could not take part (every rank sees it)
    for (int i = 0; i < nq * K; i++) {
        if (scores) scores[i] = c->topk.host()[i].score;
        if (idx) idx[i] = c->topk.host()[i].idx;
    }
    return CHIP_OK;
}

// Announce an append to queriers of a sharded ctx and order its ring writes behind the scans already enqueued.
static int ring_begin_append(Ctx *c, int64_t new_total)
{
    if (!c->ring_dev) return CHIP_OK;
    hipEvent_t ev[2];
    {
        std::lock_guard<std::mutex> rl(c->ring_mu);
        c->rows_pending = new_total;        // queriers now validate ring residency against the length after this call
        ev[0] = c->last_scan_ev[0];
        ev[1] = c->last_scan_ev[1];
    }
    for (hipEvent_t e : ev)                 // scans already enqueued read their queries before the ring is overwritten
        if (e) CHIP_HIP(c, hipStreamWaitEvent(c->s_append, e, 0));
    return CHIP_OK;
}

// ---- append, in phases (see chip_internal.h).  The caller holds the append lock and has made the device current. ----
int append_reserve(Ctx *c, int64_t first, int64_t n) { return ensure_capacity(c, local_count(c, first + n)); }

// Upload rows [from, from + count) of the call (step > 1: every step-th row, i.e. one shard's rows) in staging-sized chunks and
// run K3 on them.  ring: mirror into the replicated ring as well.  A projected append (src.raw) makes each chunk's rows on the device
// instead of copying them: the raw descriptors are staged already (ctx_append), the rows are doubles.  A pooled append (src.fmap) makes
// the chunk's rows from the caller's feature maps the same way (vlad.hip vlad_chunk).
static int append_pass(Ctx *c, const AppendSrc &src, int64_t first, int64_t from, int64_t count, int64_t step, bool ring)
{
    const int src_elem = src.elem;
    const size_t row_bytes = (size_t)c->D * src_elem;
    const int64_t chunk_rows = (int64_t)(c->stage_bytes / row_bytes);
    for (int64_t done = 0; done < count; done += chunk_rows) {
        const int64_t m = (count - done) < chunk_rows ? (count - done) : chunk_rows;
        if (src.raw) {   // (plain single-GPU ctx: step == 1)
            const int r = project_chunk(c, from + done, m);
            if (r != CHIP_OK) return r;
        } else if (src.fmap) {   // (plain single-GPU ctx: step == 1)
            const int r = vlad_chunk(c, src, from + done, m);
            if (r != CHIP_OK) return r;
        } else {
            const char *host = static_cast<const char *>(src.desc) + (size_t)(from + done * step) * row_bytes;
            if (step == 1)
                CHIP_HIP(c, hipMemcpyAsync(c->stage_dev, host, (size_t)m * row_bytes, hipMemcpyHostToDevice, c->s_append));
            else   // one shard's rows: a strided gather out of the caller's batch, one row per pitch line
                CHIP_HIP(c, hipMemcpy2DAsync(c->stage_dev, row_bytes, host, (size_t)step * row_bytes, row_bytes, (size_t)m, hipMemcpyHostToDevice, c->s_append));
        }
        const int r = launch_store_rows(c, c->s_append, c->stage_dev, src_elem, m, first + from + done * step, c->flags_dev, ring, step);
        if (r != CHIP_OK) return r;
        // the staging buffer is reused by the next chunk: stream order serialises copy -> kernel -> copy
    }
    return CHIP_OK;
}

// DB rows only (rows past the published length are invisible to queries); *bad gets the validation bits of THIS ctx's share:
// bit0 = a value that is not float32-representable went into float rows, bit1 = NaN / Inf, bit2 (with bit0) = a finite value became +-Inf.
int append_store_db(Ctx *c, const AppendSrc &src, int64_t first, int64_t n, bool owner_only, uint32_t *bad)
{
    *c->flags_host.host() = 0;
    CHIP_HIP(c, hipMemsetAsync(c->flags_dev, 0, sizeof(uint32_t), c->s_append));
    CHIP_HIP(c, hipMemsetAsync(c->norm2_dev, 0, sizeof(unsigned long long), c->s_append));   // the rows of this call alone: append_publish folds them in
    int rc;
    if (owner_only && c->nranks > 1) {
        const int64_t G = c->nranks;
        const int64_t i0 = ((c->rank - first) % G + G) % G;               // first row of the batch this shard owns
        const int64_t cnt = n > i0 ? (n - i0 + G - 1) / G : 0;
        rc = append_pass(c, src, first, i0, cnt, G, false);
    } else {
        rc = append_pass(c, src, first, 0, n, 1, false);
    }
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemcpyAsync(c->flags_host.host(), c->flags_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_append));
    CHIP_HIP(c, hipMemcpyAsync(c->norm2_host.host(), c->norm2_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_append));
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    *bad = *c->flags_host.host();
    return CHIP_OK;
}

// Genuinely float64 descriptors (e.g. ReljaNetVLAD's numpy WPCA output, whole_image_desc_compute_server.py:148-149): an
// undecided, still EMPTY DB becomes a double-row DB -- as the reference's MatrixXd M (Cerebro.cpp:946).
bool append_can_switch_to_double(const Ctx *c, int64_t first) { return c->store_auto && first == 0 && (size_t)c->D * 8 * 2 <= 160 * 1024; }

int append_switch_to_double(Ctx *c, int64_t n)
{
    int rc = configure_storage(c, 8);
    if (rc != CHIP_OK) return rc;
    return ensure_capacity(c, local_count(c, c->cap_hint > n ? c->cap_hint : n));
}

void append_publish(Ctx *c, int64_t new_total, bool lossy, int64_t n)
{
    std::lock_guard<std::mutex> lk(c->mu);  // publish the new length only now (rows fully resident)
    c->rows_global = new_total;
    c->rows_local = local_count(c, c->rows_global);
    if (c->elem == 4 && c->norm2_host.host()) {   // the largest sum of squares among the rows this call stored (append_store_db / synth_generate waited for it)
        double ss;
        std::memcpy(&ss, c->norm2_host.host(), sizeof ss);
        const double nrm = std::sqrt(ss) * (1.0 + std::ldexp(1.0, -30));
        if (!(nrm <= c->row_norm_max)) c->row_norm_max = nrm;   // (a NaN would stick, and switch the prefilter off)
    }
    if (lossy) c->lossy_rows += n;   // upper bound: rows of this call
    c->store_auto = false;           // the storage type is final once the DB holds a row
}

int append_ring_publish(Ctx *c, const AppendSrc &src, int64_t first, int64_t n, bool lossy)
{
    if (c->ring_dev) {  // sharded: mirror the newest rows into the replicated ring (the DB store of owned rows is idempotent)
        int rc = ring_begin_append(c, first + n);
        if (rc != CHIP_OK) return rc;
        const int64_t m = n < CHIP_RING_ROWS ? n : CHIP_RING_ROWS;
        rc = append_pass(c, src, first, n - m, m, 1, true);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    }
    append_publish(c, first + n, lossy, n);
    return CHIP_OK;
}

int ctx_append(Ctx *c, const AppendSrc &src, int64_t n, uint32_t flags, int64_t *first_index)
{
    if (!c || !(src.raw ? (const void *)src.raw : src.fmap ? (const void *)src.fmap : src.desc) || n < 0) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> alk(c->append_mu);
    if (src.raw && !c->proj.in_dim) return CHIP_ERR_BUSY;   // a projected append without a projection
    if (src.fmap) {                                         // a pooled append: weights, then the pooled vector's length against what takes it
        if (!c->vlad.C) return CHIP_ERR_BUSY;
        if (c->vlad.K * c->vlad.C != (c->proj.in_dim ? c->proj.in_dim : c->D)) return CHIP_ERR_UNSUPPORTED;
    }
    CHIP_HIP(c, hipSetDevice(c->device));
    const int64_t first = published_rows(c);
    if (first_index) *first_index = first;
    if (n == 0) return CHIP_OK;
    // a projected append launches kernels that fill every CU and do not fit beside the resident scan instance (project.hip project_chunk)
    // (a pooled append: vlad.hip vlad_chunk says why it pauses too)
    ResidentPause paused(c, src.raw != nullptr || src.fmap != nullptr);
    int rc = append_reserve(c, first, n);
    if (rc == CHIP_OK && src.raw) rc = project_stage_input(c, src.raw, n);   // once: a retry below projects the staged descriptors again
    if (rc != CHIP_OK) return rc;
    // A ctx that is fed the whole stream by its own caller (single GPU, or one process per GPU) validates the WHOLE batch, so that
    // every rank takes the same storage-type / rejection decision without talking to the others.
    uint32_t bad = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (src.raw || src.fmap) project_count_reset(c);   // chip_debug_project_last: what THIS run of the call launches
        rc = append_store_db(c, src, first, n, false, &bad);
        if (rc != CHIP_OK) return rc;
        if (bad & 2u) return CHIP_ERR_NONFINITE;
        if (!(bad & 1u)) break;
        // CHIP_APPEND_ALLOW_ROUNDING is the caller saying "these ARE float32 descriptors, up to the precision they were printed / sent
        // with" (a state.json checkpoint holds 15-digit decimal text, RawFileIO.cpp:330-459): they are rounded to the float rows they
        // came from, also in an empty undecided DB.  Without the flag the data decides: an empty undecided DB takes values that are
        // not float32-representable as they are (double rows); anywhere else they are refused.
        // Rounding is to a float32 VALUE: a finite wire value beyond the float range (bit2) would be stored as +-Inf, and a DB never holds one.
        if (flags & CHIP_APPEND_ALLOW_ROUNDING) {
            if (bad & 4u) return CHIP_ERR_NONFINITE;
            break;
        }
        if (attempt == 0 && append_can_switch_to_double(c, first)) {
            rc = append_switch_to_double(c, n);
            if (rc != CHIP_OK) return rc;
            continue;
        }
        return CHIP_ERR_NOT_F32;
    }
    return append_ring_publish(c, src, first, n, (bad & 1u) != 0);
}

int synth_generate(Ctx *c, int64_t first, int64_t n, uint64_t seed, const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant, int unit)
{
    ResidentPause paused(c, n_plant > 0);   // declared first: the plant arrays below are freed before it resumes
    DevBuf<int64_t> pd, ps;
    DevBuf<int32_t> pk;
    if (n_plant > 0) {
        int rc = pd.reserve(c, (size_t)n_plant);
        if (rc == CHIP_OK) rc = ps.reserve(c, (size_t)n_plant);
        if (rc == CHIP_OK) rc = pk.reserve(c, (size_t)n_plant);
        if (rc != CHIP_OK) return rc;
        CHIP_HIP(c, hipMemcpyAsync(pd, plant_dst, n_plant * sizeof(int64_t), hipMemcpyHostToDevice, c->s_append));
        CHIP_HIP(c, hipMemcpyAsync(ps, plant_src, n_plant * sizeof(int64_t), hipMemcpyHostToDevice, c->s_append));
        CHIP_HIP(c, hipMemcpyAsync(pk, plant_kind, n_plant * sizeof(int32_t), hipMemcpyHostToDevice, c->s_append));
    }
    int rc = ring_begin_append(c, first + n);   // same ordering against in-flight scans as ctx_append
    hipError_t e0 = hipMemsetAsync(c->norm2_dev, 0, sizeof(unsigned long long), c->s_append);
    if (rc == CHIP_OK) rc = launch_synth(c, c->s_append, first, n, seed, pd, ps, pk, n_plant, unit);
    if (e0 == hipSuccess) e0 = hipMemcpyAsync(c->norm2_host.host(), c->norm2_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_append);
    hipError_t e = hipStreamSynchronize(c->s_append);   // before the plant arrays go
    if (e == hipSuccess) e = e0;
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, e);
    return CHIP_OK;
}

static int check_plants(int64_t first, int64_t n, const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant)
{
    for (int64_t i = 0; i < n_plant; i++) {
        if (plant_dst[i] < first || plant_dst[i] >= first + n || plant_src[i] < 0) return CHIP_ERR_RANGE;
        if (i > 0 && plant_dst[i] <= plant_dst[i - 1]) return CHIP_ERR_INVALID_ARG;
        if (plant_kind[i] != 1 && plant_kind[i] != 2) return CHIP_ERR_INVALID_ARG;
    }
    return CHIP_OK;
}

int ctx_append_synthetic(Ctx *c, int64_t n, uint64_t seed, const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant, int unit)
{
    if (!c || n < 0 || n_plant < 0 || (n_plant > 0 && (!plant_dst || !plant_src || !plant_kind))) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> alk(c->append_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    const int64_t first = published_rows(c);
    int rc = check_plants(first, n, plant_dst, plant_src, plant_kind, n_plant);
    if (rc != CHIP_OK) return rc;
    if (n == 0) return CHIP_OK;
    rc = append_reserve(c, first, n);
    if (rc != CHIP_OK) return rc;
    rc = synth_generate(c, first, n, seed, plant_dst, plant_src, plant_kind, n_plant, unit);
    if (rc != CHIP_OK) return rc;
    append_publish(c, first + n, false, n);
    return CHIP_OK;
}

// one row (storage type) to host memory, asynchronously on the ctx stream
int ctx_read_row(Ctx *c, int64_t g, int64_t total, void *out)
{
    const void *src;
    if (owns_row(c, g)) src = row_ptr_host(c, local_of(c, g));
    else if (c->ring_dev && g >= total - CHIP_RING_ROWS) src = ring_ptr(c, g);
    else return CHIP_ERR_RANGE;
    CHIP_HIP(c, hipMemcpyAsync(out, src, (size_t)c->D * c->elem, hipMemcpyDeviceToHost, c->s_query));
    return CHIP_OK;
}

static int read_rows(chip_ctx *c, const int64_t *rows, int64_t n, void *out, int out_elem)
{
    if (!c || !rows || !out || n < 0) return CHIP_ERR_INVALID_ARG;
    if (c->group) return group_read_rows(c, rows, n, out, out_elem);
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    if (out_elem < c->elem) return CHIP_ERR_NOT_F32;   // double rows do not fit a float buffer: chip_db_read_rows_f64
    const int64_t total = published_rows(c);
    const bool conv = out_elem != c->elem;             // float rows into a double buffer: widen on the host
    std::vector<float> tmp;
    if (conv) tmp.resize((size_t)n * c->D);
    for (int64_t i = 0; i < n; i++) {
        const int64_t g = rows[i];
        if (g < 0 || g >= total) return CHIP_ERR_RANGE;
        void *dst = conv ? (void *)(tmp.data() + (size_t)i * c->D) : (void *)(static_cast<char *>(out) + (size_t)i * c->D * out_elem);
        const int rc = ctx_read_row(c, g, total, dst);
        if (rc != CHIP_OK) return rc;
    }
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));
    if (conv)
        for (size_t i = 0; i < tmp.size(); i++) static_cast<double *>(out)[i] = (double)tmp[i];
    return CHIP_OK;
}

int merge_enqueue_slot(Ctx *c, int64_t l, const chip_dot_params *p, const void *dev_gathered, int32_t n_lists, int32_t topk, Slot &s)
{
    if (s.state != SlotState::Free) return CHIP_ERR_BUSY;
    // (the record goes to s.rec, pinned + mapped: no D2H copy)
    int rc = launch_merge(c, c->s_query, merge_args((const chip_topk_entry *)dev_gathered, n_lists, topk, nullptr, s.rec.dev(), l, p), 3);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipEventRecord(s.done, c->s_query));
    s.wait_ev = s.done;
    s.state = SlotState::Event;
    return CHIP_OK;
}

// merge of gathered [n_lists][nq][K] lists into out[nq][K] on the ctx stream, no decision
int merge_enqueue_out(Ctx *c, const void *dev_gathered, int32_t n_lists, int nq, int32_t topk, chip_topk_entry *out)
{
    return launch_merge(c, c->s_query, merge_args((const chip_topk_entry *)dev_gathered, n_lists, topk, out, nullptr, 0, nullptr), nq);
}

// All scores of one query over this ctx's share of the prefix [0,k): u_global[local * mul + add] = score (host buffer).
int ctx_scores_local(Ctx *c, int64_t k, const void *q, double *u_global, int64_t mul, int64_t add)
{
    const int64_t n_rows = local_count(c, k);
    if (n_rows == 0) return CHIP_OK;
    if ((size_t)n_rows > c->scores_dev.capacity()) {
        const int rc = c->scores_dev.reserve(c, (size_t)(n_rows + n_rows / 4 + 1024));
        if (rc != CHIP_OK) return rc;
    }
    ScanArgs a;
    scan_args_db(c, &a);
    a.n_rows = n_rows;
    a.K = 1;
    for (int i = 0; i < CHIP_MAX_NQ; i++) a.q[i] = i == 0 ? q : nullptr;
    a.idx_mul = mul;
    a.idx_add = add;
    a.partial = nullptr;
    int rc = launch_scores(c, c->s_scan, a, c->scores_dev);
    if (rc != CHIP_OK) return rc;
    if (mul == 1 && add == 0) {
        CHIP_HIP(c, hipMemcpyAsync(u_global, c->scores_dev, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->s_scan));
        CHIP_HIP(c, hipStreamSynchronize(c->s_scan));
    } else {
        std::vector<double> tmp((size_t)n_rows);
        CHIP_HIP(c, hipMemcpyAsync(tmp.data(), c->scores_dev, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->s_scan));
        CHIP_HIP(c, hipStreamSynchronize(c->s_scan));
        for (int64_t r = 0; r < n_rows; r++) u_global[r * mul + add] = tmp[(size_t)r];
    }
    return CHIP_OK;
}

}  // namespace chip

extern "C" {

// ------------------------------------------------------------------------------------------------ lifecycle
int chip_create(chip_ctx **out, int32_t D, int64_t capacity_hint, int32_t device, int32_t shard_rank, int32_t shard_count)
{
    return ctx_create(out, D, capacity_hint, device, shard_rank, shard_count, 0);
}

int chip_create_ex(chip_ctx **out, int32_t D, int64_t capacity_hint, int32_t device, int32_t shard_rank, int32_t shard_count, uint32_t flags)
{
    if (flags & ~kCreateStoreMask) return CHIP_ERR_INVALID_ARG;
    return ctx_create(out, D, capacity_hint, device, shard_rank, shard_count, flags);
}

void chip_destroy(chip_ctx *ctx) { ctx_destroy(ctx); }

int chip_set_stream(chip_ctx *c, void *hip_stream)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group || c->xchg) return CHIP_ERR_UNSUPPORTED;   // the library owns the exchange and its stream ordering
    std::lock_guard<std::mutex> lk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));
    resident_stop(c);                       // ticks of a ctx on a caller's stream are launched behind that stream's work
    if (c->own_query_stream) CHIP_HIP(c, hipStreamDestroy(c->s_query));
    c->s_query = (hipStream_t)hip_stream;   // may be 0: HIP's null stream is a valid external stream
    c->own_query_stream = false;
    return CHIP_OK;
}

int chip_reset_stream(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    if (c->own_query_stream) return CHIP_OK;
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));
    CHIP_HIP(c, hipStreamCreateWithFlags(&c->s_query, hipStreamNonBlocking));
    c->own_query_stream = true;
    return CHIP_OK;
}

int chip_synchronize(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return group_synchronize(c);
    CHIP_HIP(c, hipSetDevice(c->device));
    { std::lock_guard<std::mutex> qlk(c->query_mu); (void)coalesce_flush(c); }
    CHIP_HIP(c, hipStreamSynchronize(c->s_append));
    CHIP_HIP(c, hipStreamSynchronize(c->s_scan));
    if (c->s_scan2) CHIP_HIP(c, hipStreamSynchronize(c->s_scan2));
    for (hipStream_t x : c->s_scan_x)
        if (x) CHIP_HIP(c, hipStreamSynchronize(x));
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));
    CHIP_HIP(c, hipStreamSynchronize(c->s_pnp));
    resident_wait_command(c);
    return CHIP_OK;
}

// ------------------------------------------------------------------------------------------------ append
int chip_db_append_f64(chip_ctx *c, const double *desc, int64_t n, uint32_t flags, int64_t *first_index)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    return c->group ? group_append(c, desc, 8, n, flags, first_index) : ctx_append(c, AppendSrc{desc, 8}, n, flags, first_index);
}

// chip_db_append_f64 with the rows made on the device from raw descriptors (project.hip): the same phases, a second kind of source
int chip_db_append_projected_f32(chip_ctx *c, const float *x, int64_t n, uint32_t flags, int64_t *first_index)
{
    if (!c || !x || n < 0) return CHIP_ERR_INVALID_ARG;
    if (c->group || c->nranks > 1) return CHIP_ERR_UNSUPPORTED;
    return ctx_append(c, AppendSrc{nullptr, 8, x}, n, flags, first_index);
}

// chip_db_append_f64 of n_maps rows pooled on the device from feature maps (vlad.hip): a third kind of source
int chip_db_append_vlad_batch_f32(chip_ctx *c, const float *fmaps, int32_t n_maps, int32_t positions, int32_t layout, uint32_t flags, int64_t *first_index)
{
    if (!c || !fmaps || n_maps < 0) return CHIP_ERR_INVALID_ARG;
    if (positions < 1 || positions > CHIP_VLAD_MAX_POSITIONS || (layout != CHIP_VLAD_NHWC && layout != CHIP_VLAD_NCHW)) return CHIP_ERR_UNSUPPORTED;
    if (c->group || c->nranks > 1) return CHIP_ERR_UNSUPPORTED;
    AppendSrc src{nullptr, 8};
    src.fmap = fmaps;
    src.positions = positions;
    src.layout = layout;
    src.n_maps = n_maps;
    return ctx_append(c, src, n_maps, flags, first_index);
}

// the single call: a batch of one
int chip_db_append_vlad_f32(chip_ctx *c, const float *fmap, int32_t positions, int32_t layout, uint32_t flags, int64_t *first_index)
{
    return chip_db_append_vlad_batch_f32(c, fmap, 1, positions, layout, flags, first_index);
}

int chip_db_append_f32(chip_ctx *c, const float *desc, int64_t n, int64_t *first_index)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    return c->group ? group_append(c, desc, 4, n, 0, first_index) : ctx_append(c, AppendSrc{desc, 4}, n, 0, first_index);
}

int64_t chip_db_size(const chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    return published_rows(c);
}

int chip_db_read_rows_f32(chip_ctx *c, const int64_t *rows, int64_t n, float *out) { return read_rows(c, rows, n, out, 4); }
int chip_db_read_rows_f64(chip_ctx *c, const int64_t *rows, int64_t n, double *out) { return read_rows(c, rows, n, out, 8); }

int chip_db_append_synthetic(chip_ctx *c, int64_t n, uint64_t seed,
                             const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    return c->group ? group_append_synthetic(c, n, seed, plant_dst, plant_src, plant_kind, n_plant, 0)
                    : ctx_append_synthetic(c, n, seed, plant_dst, plant_src, plant_kind, n_plant, 0);
}

int chip_db_append_synthetic_unit(chip_ctx *c, int64_t n, uint64_t seed,
                                  const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    return c->group ? group_append_synthetic(c, n, seed, plant_dst, plant_src, plant_kind, n_plant, 1)
                    : ctx_append_synthetic(c, n, seed, plant_dst, plant_src, plant_kind, n_plant, 1);
}

// ------------------------------------------------------------------------------------------------ queries
static int check_query_args(chip_ctx *c, int64_t k, int32_t nq, int32_t topk, int64_t *n_global)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (nq < 1 || nq > CHIP_MAX_NQ || topk < 1 || topk > CHIP_MAX_TOPK) return CHIP_ERR_UNSUPPORTED;
    *n_global = published_rows(c);
    if (k < 0) return CHIP_ERR_RANGE;
    // with an exchange attached "k beyond what THIS rank has published" is a per-rank condition: the rank takes part in the
    // collective call with the failure mark (chip_multi.hip) instead of leaving it
    if (k > *n_global && !(c->xchg && !c->group)) return CHIP_ERR_RANGE;
    return CHIP_OK;
}

static int query_common(chip_ctx *c, int64_t k, const int64_t *query_rows, const void *vectors, int vec_elem, int32_t nq, int32_t topk,
                        double *scores, int64_t *idx)
{
    int64_t n = 0;
    int rc = check_query_args(c, k, nq, topk, &n);
    if (rc != CHIP_OK) return rc;
    if (!query_rows && !vectors) return CHIP_ERR_INVALID_ARG;
    if (c->group) return group_query(c, k, query_rows, vectors, vec_elem, nq, topk, scores, idx);
    std::lock_guard<std::mutex> qlk(c->query_mu);
    (void)coalesce_flush(c);
    CHIP_HIP(c, hipSetDevice(c->device));
    const void *q[CHIP_MAX_NQ];
    RingGuard rg(c);
    if (c->xchg) {   // collective: every rank makes the same call; per-rank conditions become the failure mark
        bool fail_local = k > n;
        rc = query_rows ? xchg_fetch_rows(c, query_rows, nq, n, q, &fail_local) : upload_query_vectors(c, vectors, vec_elem, nq, q);
        if (rc != CHIP_OK) return rc;
        return xchg_query(c, k, q, nq, topk, scores, idx, fail_local);
    }
    rc = query_rows ? query_row_ptrs(c, query_rows, nq, n, q) : upload_query_vectors(c, vectors, vec_elem, nq, q);
    if (rc != CHIP_OK) return rc;
    ScanRequest rq;
    rq.k = k; rq.q = q; rq.nq = nq; rq.K = topk; rq.out = c->topk.dev();
    rc = enqueue_scan_merge(c, rq);
    if (rc != CHIP_OK) return rc;
    return sync_topk_out(c, nq, topk, scores, idx);
}

int chip_query_rows(chip_ctx *c, int64_t k, const int64_t *query_rows, int32_t nq, int32_t topk, double *scores, int64_t *idx)
{
    if (!query_rows) return CHIP_ERR_INVALID_ARG;
    return query_common(c, k, query_rows, nullptr, 0, nq, topk, scores, idx);
}

int chip_query_vectors_f32(chip_ctx *c, int64_t k, const float *queries, int32_t nq, int32_t topk, double *scores, int64_t *idx)
{
    if (!queries) return CHIP_ERR_INVALID_ARG;
    return query_common(c, k, nullptr, queries, 4, nq, topk, scores, idx);
}

int chip_query_vectors_f64(chip_ctx *c, int64_t k, const double *queries, int32_t nq, int32_t topk, double *scores, int64_t *idx)
{
    if (!queries) return CHIP_ERR_INVALID_ARG;
    return query_common(c, k, nullptr, queries, 8, nq, topk, scores, idx);
}

int chip_query_scores(chip_ctx *c, int64_t k, int64_t query_row, double *u)
{
    if (!c || !u) return CHIP_ERR_INVALID_ARG;
    const int64_t n = published_rows(c);
    if (k < 0 || query_row < 0) return CHIP_ERR_RANGE;
    const bool collective = c->xchg && !c->group;
    const bool out_of_range = k > n || query_row >= n;          // per-rank conditions when the ranks append independently
    if (out_of_range && !collective) return CHIP_ERR_RANGE;
    if (c->group) return group_scores(c, k, query_row, u);
    std::lock_guard<std::mutex> qlk(c->query_mu);
    (void)coalesce_flush(c);
    CHIP_HIP(c, hipSetDevice(c->device));
    const void *q[1];
    RingGuard rg(c);
    int rc;
    if (collective) {   // the query row comes from its owner (any appended row); the broadcast is made by EVERY rank, also by one
                        // that then finds its own arguments out of range -- leaving before it would put the communicator out of step
        bool fail_local = false;
        rc = xchg_fetch_rows(c, &query_row, 1, n, q, &fail_local);
        if (rc == CHIP_OK && (fail_local || out_of_range)) rc = CHIP_ERR_RANGE;
    } else {
        rc = query_row_ptrs(c, &query_row, 1, n, q);
    }
    if (rc != CHIP_OK) return rc;
    // a sharded ctx fills only the entries of the rows it owns (u[i], i % shard_count == shard_rank)
    return ctx_scores_local(c, k, q[0], u, c->nranks, c->nranks == 1 ? 0 : c->rank);
}

// ------------------------------------------------------------------------------------------------ tick
int chip_loop_tick(chip_ctx *c, int64_t l, const chip_dot_params *p, chip_tick_result *out)
{
    if (!c || !p || !out) return CHIP_ERR_INVALID_ARG;
    if (c->group) {
        const int rc = group_tick_enqueue(c, l, p, CHIP_MAX_INFLIGHT - 1);
        return rc != CHIP_OK ? rc : group_tick_collect(c, CHIP_MAX_INFLIGHT - 1, out);
    }
    if (c->nranks != 1 && !c->xchg) return CHIP_ERR_UNSUPPORTED;  // host-driven exchange: chip_scan_local + chip_merge_decide
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    Slot &s = c->slots[CHIP_MAX_INFLIGHT - 1];
    int rc = tick_enqueue_slot(c, l, p, true, s);   // synchronous: the scan form of this tick is chosen for its latency (kernels.hip scan_rows_form)
    if (rc != CHIP_OK) return rc;
    return tick_collect_slot(c, s, out);
}

int chip_loop_tick_enqueue(chip_ctx *c, int64_t l, const chip_dot_params *p, int32_t slot)
{
    if (!c || !p || slot < 0 || slot >= CHIP_MAX_INFLIGHT - 1) return CHIP_ERR_INVALID_ARG;
    if (c->group) return group_tick_enqueue(c, l, p, slot);
    if (c->nranks != 1 && !c->xchg) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    return tick_enqueue_slot(c, l, p, false, c->slots[slot]);
}

int chip_loop_tick_collect(chip_ctx *c, int32_t slot, chip_tick_result *out)
{
    if (!c || !out || slot < 0 || slot >= CHIP_MAX_INFLIGHT - 1) return CHIP_ERR_INVALID_ARG;
    if (c->group) return group_tick_collect(c, slot, out);
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    return tick_collect_slot(c, c->slots[slot], out);
}

int64_t chip_loop_last_l(const chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    return c->last_l;
}

void chip_loop_reset(chip_ctx *c)
{
    if (!c) return;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    c->last_l = 0;
}

int chip_scan_local(chip_ctx *c, int64_t l, const chip_dot_params *p, int32_t topk, void *dev_out, int32_t *status)
{
    if (!c || !p || !dev_out || !status) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    if (topk < 1 || topk > CHIP_MAX_TOPK) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    int64_t k = 0;
    int rc = tick_prepare(published_rows(c), c->last_l, l, p, status, &k);
    if (rc == CHIP_OK && *status == CHIP_TICK_TOO_SHORT) c->last_l = l;
    if (rc != CHIP_OK || *status != CHIP_TICK_SCANNED) return rc;
    const int64_t rows[3] = {l - 1, l - 2, l - 3};
    const void *q[3];
    RingGuard rg(c);
    rc = query_row_ptrs(c, rows, 3, l, q);
    if (rc != CHIP_OK) return rc;
    // scan on s_scan, then (behind an event) the local merge on the ctx stream writes this rank's 3 x topk list to
    // dev_out: everything the caller enqueues next on the ctx stream (the all-gather) is ordered after it, while the
    // next tick's scan is free to start as soon as this scan ends.
    ScanRequest rq;
    rq.k = k; rq.q = q; rq.nq = 3; rq.K = topk; rq.out = (chip_topk_entry *)dev_out;
    rq.l = l; rq.tick = true;
    rc = enqueue_scan_merge(c, rq);
    if (rc == CHIP_OK) c->last_l = l;  // :1098
    return rc;
}

int chip_merge_decide(chip_ctx *c, int64_t l, const chip_dot_params *p, const void *dev_gathered, int32_t n_lists,
                      int32_t topk, chip_tick_result *out)
{
    if (!c || !p || !dev_gathered || !out || n_lists < 1) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    if (topk < 1 || topk > CHIP_MAX_TOPK) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    Slot &s = c->slots[CHIP_MAX_INFLIGHT - 1];
    int rc = merge_enqueue_slot(c, l, p, dev_gathered, n_lists, topk, s);
    if (rc != CHIP_OK) return rc;
    return tick_collect_slot(c, s, out);
}

int chip_merge_decide_enqueue(chip_ctx *c, int64_t l, const chip_dot_params *p, const void *dev_gathered, int32_t n_lists,
                              int32_t topk, int32_t slot)
{
    if (!c || !p || !dev_gathered || n_lists < 1 || slot < 0 || slot >= CHIP_MAX_INFLIGHT - 1) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    if (topk < 1 || topk > CHIP_MAX_TOPK) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    return merge_enqueue_slot(c, l, p, dev_gathered, n_lists, topk, c->slots[slot]);
}

// The two list-merge kernels alone, on the caller's lists (test aid; batch.hip debug_merge_lists).
int chip_debug_merge_lists(chip_ctx *c, int32_t form, const chip_topk_entry *lists, int32_t n_lists, int32_t nq, int32_t K, chip_topk_entry *out,
                           int64_t l, const chip_dot_params *p, chip_tick_result *result)
{
    if (!c || !lists || !out || n_lists < 1 || (result && !p)) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_ERR_UNSUPPORTED;
    if (K < 1 || K > CHIP_MAX_TOPK || n_lists > 512) return CHIP_ERR_UNSUPPORTED;
    const bool form_ok = form == 0 ? nq >= 1 && nq <= CHIP_MAX_NQ                          // topk_merge<nq>
                                   : form == 1 && nq >= 4 && nq % 4 == 0 && nq <= 4096 && !result;   // topk_merge_batch: four queries per workgroup, no record
    if (!form_ok) return CHIP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    return debug_merge_lists(c, form, lists, n_lists, nq, K, out, l, p, result);
}

// ------------------------------------------------------------------------------------------------ introspection
int chip_get_info(const chip_ctx *c, chip_info *info)
{
    if (!c || !info) return CHIP_ERR_INVALID_ARG;
    std::memset(info, 0, sizeof *info);
    const Ctx *r = c->group ? group_root(const_cast<chip_ctx *>(c)) : c;
    std::lock_guard<std::mutex> lk(r->mu);
    info->abi_version = CHIP_ABI_VERSION;
    info->D = r->D;
    info->device = r->device;
    info->shard_rank = r->rank;
    info->shard_count = r->nranks;
    info->n_cus = r->n_cus;
    info->rows_global = r->rows_global;
    info->rows_local = r->rows_local;
    info->capacity_local = (int64_t)r->segs.size() * r->seg_rows;
    info->lossy_rows = r->lossy_rows;
    std::strncpy(info->arch, r->arch, sizeof(info->arch) - 1);
    info->storage_bytes = r->elem;
    info->n_devices = c->group ? group_size(c) : 1;
    info->exchange = c->group ? c->group_transport : (c->xchg ? CHIP_EXCHANGE_RCCL : CHIP_EXCHANGE_NONE);
    info->comm_ranks = exchange_comm_ranks(c->group ? r : c);
    info->comm_init_abandoned = c->comm_init_abandoned;
    info->scan_forms = scan_forms_built();
    info->test_hooks = chip_build_test_hooks();
    info->row_norm_max = r->row_norm_max;
    return CHIP_OK;
}

// Several pipelined ticks per DB pass (coalesce_* above).  Passes that served more than one tick and the ticks they served, so that
// a test can see that ticks did share a pass; CHIP_ERR_INVALID_ARG on a group.
int chip_debug_coalesce_stats(chip_ctx *c, int64_t *passes, int64_t *ticks)
{
    if (!c || !passes || !ticks || c->group) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    *passes = c->coalesce_passes;
    *ticks = c->coalesce_ticks;
    return CHIP_OK;
}

// Prefilter passes of either kind (four ticks: db_scan_prefilter, five: db_scan_halfq; + tick_rescore), their ticks, and the ticks among them that a collect has run again alone
// because their certificate did not hold.
int chip_debug_prefilter_stats(chip_ctx *c, int64_t *passes, int64_t *ticks, int64_t *uncertified)
{
    if (!c || !passes || !ticks || !uncertified || c->group) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    *passes = c->prefilter_passes;
    *ticks = c->prefilter_ticks;
    *uncertified = c->prefilter_uncertified;
    return CHIP_OK;
}

// What the last prefilter pass of this ctx (four ticks or five) left in device memory, and what it was launched with.  Launches nothing and
// submits nothing (parked ticks stay parked): waits for the ctx's own streams, then copies.  The pass's list buffer is not reused before
// Ctx::kRing further enqueues, and a tick that runs again alone takes another buffer: valid after the collects of the pass's window.
int chip_debug_last_pass(chip_ctx *c, chip_debug_pass_info *info, chip_topk_entry *cand, chip_topk_entry *exact, uint32_t *cert)
{
    if (!c || c->group) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    const Ctx::LastPass &lp = c->last_pass;
    if (lp.family == 0) return CHIP_ERR_BUSY;
    CHIP_HIP(c, hipSetDevice(c->device));
    CHIP_HIP(c, hipStreamSynchronize(c->s_scan));
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->family = lp.family; info->ticks = lp.ticks; info->grid = lp.grid; info->wpb = lp.wpb; info->K = lp.K; info->e = lp.e; info->E = lp.E;
        for (int t = 0; t < lp.ticks; t++) info->k[t] = lp.k[t];
    }
    const chip_topk_entry *lists = c->partial_dev[lp.ring];
    const size_t n_cand = (size_t)lp.ticks * lp.grid * 3 * lp.K, n_exact = (size_t)lp.ticks * 3 * lp.K;
    if (cand) CHIP_HIP(c, hipMemcpy(cand, lists, n_cand * sizeof(chip_topk_entry), hipMemcpyDeviceToHost));
    if (exact) CHIP_HIP(c, hipMemcpy(exact, lists + (size_t)kPassMaxTicks * lp.grid * 3 * lp.K, n_exact * sizeof(chip_topk_entry), hipMemcpyDeviceToHost));
    if (cert)
        for (int t = 0; t < lp.ticks; t++)
            for (int i = 0; i < 3; i++) cert[3 * t + i] = lp.cert[t][i];
    return CHIP_OK;
}

// While on, a tick that may share a pass parks even when no scan of the ctx is running -- whether a small test scan is still running
// when the next enqueue arrives is a race the tests must not depend on.  Everything that releases parked ticks works as always;
// switching it off releases them.
int chip_debug_coalesce_force(chip_ctx *c, int32_t on)
{
    if (!c || c->group) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    c->coalesce_force = on != 0;
    if (!on) { (void)hipSetDevice(c->device); (void)coalesce_flush(c); }
    return CHIP_OK;
}

// The parking policy alone (no ctx, no device): kCoalesceLaunch / Park / ParkFlush for a tick that could share a pass.
int chip_debug_coalesce_decide(int32_t n_parked, int32_t t_max, int32_t scan_running) { return coalesce_decide(n_parked, t_max, scan_running != 0); }

// WHICH kernel the last top-k scan of this ctx was (launch_scan / launch_scan_multi keep the record where they choose the
// instantiation); parked ticks are submitted first, so that the record is the launch of the calls made so far.
int chip_debug_last_scan(chip_ctx *c, chip_debug_scan_launch *out)
{
    if (!c || !out || c->group) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    (void)hipSetDevice(c->device);
    (void)coalesce_flush(c);
    *out = c->last_scan;
    return CHIP_OK;
}

// The same record without a device: a ctx that exists on the host only (D, storage type, CU count, the knobs of the environment as
// chip_create reads them), then the functions the enqueue path runs -- scan_policy, tick_merge_on_scan_stream, scan_tick_fused, scan_select.  A plain
// single-GPU ctx on its own streams, profiling off, the resident instance off.
int chip_debug_scan_plan(int32_t D, int32_t elem, int32_t nq, int32_t K, int64_t n_rows, int32_t call, int32_t n_cus, chip_debug_scan_launch *out)
{
    if (!out || D <= 0 || (elem != 4 && elem != 8) || nq < 1 || nq > CHIP_MAX_NQ || K < 1 || K > CHIP_MAX_TOPK || n_rows < 0 || n_cus < 1 ||
        call < CHIP_SCAN_CALL_QUERY || call > CHIP_SCAN_CALL_TICK_SYNC)
        return CHIP_ERR_INVALID_ARG;
    // what chip_create refuses (ctx_create)
    if (D % 4 != 0 || (size_t)D * 4 * CHIP_MAX_NQ > 160 * 1024 || (elem == 8 && (size_t)D * 8 * 2 > 160 * 1024)) return CHIP_ERR_UNSUPPORTED;
    std::unique_ptr<Ctx> c(new (std::nothrow) Ctx());
    if (!c) return CHIP_ERR_OOM;
    c->D = D;
    c->elem = elem;
    c->n_cus = n_cus;
    scan_read_knobs(c.get());
    const bool tick = call != CHIP_SCAN_CALL_QUERY;
    ScanArgs a{};
    int grid = 0;
    const bool short_scan = scan_policy(c.get(), n_rows, nq, call == CHIP_SCAN_CALL_TICK_SYNC, &a, &grid);
    a.n_rows = n_rows;
    a.D = D;
    a.K = K;
    const bool same_stream = tick_merge_on_scan_stream(c.get(), tick, short_scan, c->scan_streams >= 2, tick);   // (every tick of the library accepts: tick_submit)
    chip_tick_result dummy;
    if (scan_tick_fused(c.get(), same_stream, a, tick, nq)) { a.K = 1; a.fused_result = &dummy; }
    return scan_select(c.get(), a, nq, grid, out);
}

// The shared pass of n_ticks pipelined ticks without a device: scan_multi_plan, the function launch_scan_multi sizes itself with, for a plain
// single-GPU ctx of n_cus compute units.
int chip_debug_multi_plan(int32_t D, int32_t elem, int32_t n_ticks, int32_t K, int32_t n_cus, chip_debug_scan_launch *out)
{
    if (!out || D <= 0 || (elem != 4 && elem != 8) || n_ticks < 1 || K < 1 || K > CHIP_MAX_TOPK || n_cus < 1) return CHIP_ERR_INVALID_ARG;
    if (D % 4 != 0 || (size_t)D * 4 * CHIP_MAX_NQ > 160 * 1024 || (elem == 8 && (size_t)D * 8 * 2 > 160 * 1024)) return CHIP_ERR_UNSUPPORTED;   // (ctx_create)
    return scan_multi_plan(D, elem, n_ticks, K, n_cus < 512 ? n_cus : 512, out);
}

// The prefilter pass without a device: scan_prefilter_plan, the function launch_scan_prefilter sizes itself with.
int chip_debug_prefilter_plan(int32_t D, int32_t elem, int32_t K, int32_t n_cus, chip_debug_scan_launch *out)
{
    if (!out || D <= 0 || (elem != 4 && elem != 8) || K < 1 || K > CHIP_MAX_TOPK || n_cus < 1) return CHIP_ERR_INVALID_ARG;
    if (D % 4 != 0 || (size_t)D * 4 * CHIP_MAX_NQ > 160 * 1024 || (elem == 8 && (size_t)D * 8 * 2 > 160 * 1024)) return CHIP_ERR_UNSUPPORTED;   // (ctx_create)
    return scan_prefilter_plan(D, elem, K, n_cus < 512 ? n_cus : 512, out);
}

// The five-tick pass without a device: scan_halfq_plan, the function launch_scan_halfq sizes itself with.
int chip_debug_halfq_plan(int32_t D, int32_t elem, int32_t K, int32_t n_cus, chip_debug_scan_launch *out)
{
    if (!out || D <= 0 || (elem != 4 && elem != 8) || K < 1 || K > CHIP_MAX_TOPK || n_cus < 1) return CHIP_ERR_INVALID_ARG;
    if (D % 4 != 0 || (size_t)D * 4 * CHIP_MAX_NQ > 160 * 1024 || (elem == 8 && (size_t)D * 8 * 2 > 160 * 1024)) return CHIP_ERR_UNSUPPORTED;   // (ctx_create)
    return scan_halfq_plan(D, elem, K, n_cus < 512 ? n_cus : 512, out);
}

// What a five-tick pass over rows of norm at most row_norm_max is launched with: the exponent of the queries' scale and the error bound.
int chip_debug_halfq_bound(int32_t D, double row_norm_max, int32_t *e, double *E)
{
    if (!e || !E || D <= 0 || !(row_norm_max >= 0.0)) return CHIP_ERR_INVALID_ARG;
    *e = halfq_exponent(row_norm_max);
    *E = halfq_error_bound(D, row_norm_max, *e);
    return CHIP_OK;
}

// Tuning aid, not part of the ABI (no declaration in cerebro_hip.h): with CHIP_SCAN_STAMPS=1 the row-batched scan kernel leaves four
// s_memrealtime (100 MHz) stamps per wave -- entry, queries staged, rows done, block merge done -- of the most recent launch.
int chip_debug_scan_stamps(chip_ctx *c, unsigned long long *out, int64_t n_waves)
{
    if (!c || !out || c->group || !c->stamps_dev || n_waves > (int64_t)c->max_grid * 16 + 16) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    resident_stop(c);
    CHIP_HIP(c, hipDeviceSynchronize());
    CHIP_HIP(c, hipMemcpy(out, c->stamps_dev, (size_t)n_waves * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return CHIP_OK;
}

int chip_profile_enable(chip_ctx *c, int32_t on)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return group_profile_enable(c, on);
    std::lock_guard<std::mutex> qlk(c->query_mu);
    (void)hipSetDevice(c->device);
    (void)coalesce_flush(c);        // a pass is timed as a whole or not at all
    if (on) resident_stop(c);       // profiled launches want the chip as a launch finds it
    c->prof_on = on != 0;
    return CHIP_OK;
}

int chip_profile_reset(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) c = static_cast<chip_ctx *>(group_root(c));
    std::lock_guard<std::mutex> qlk(c->query_mu);
    (void)hipSetDevice(c->device);
    (void)coalesce_flush(c);
    c->prof_used = 0;
    return CHIP_OK;
}

int chip_profile_scan(chip_ctx *c, double *total_ms, int64_t *n_launches, double *bytes_per_launch_last, double *span_ms)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) {   // the root device's launches (every device scans its own 1/G of the prefix)
        const int rc = group_synchronize(c);
        if (rc != CHIP_OK) return rc;
        c = static_cast<chip_ctx *>(group_root(c));
    }
    std::lock_guard<std::mutex> qlk(c->query_mu);
    CHIP_HIP(c, hipSetDevice(c->device));
    (void)coalesce_flush(c);
    CHIP_HIP(c, hipStreamSynchronize(c->s_scan));
    if (c->s_scan2) CHIP_HIP(c, hipStreamSynchronize(c->s_scan2));
    CHIP_HIP(c, hipStreamSynchronize(c->s_query));
    double tot = 0.0, span = 0.0;
    for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
        float ms = 0.f;
        CHIP_HIP(c, hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]));
        tot += ms;
        CHIP_HIP(c, hipEventElapsedTime(&ms, c->prof_ev[0], c->prof_ev[i + 1]));  // launches alternate between two streams
        if (ms > span) span = ms;
    }
    if (total_ms) *total_ms = tot;
    if (n_launches) *n_launches = (int64_t)(c->prof_used / 2);
    if (bytes_per_launch_last) *bytes_per_launch_last = c->prof_bytes_last;
    if (span_ms) *span_ms = span;
    return CHIP_OK;
}

}  // extern "C"
