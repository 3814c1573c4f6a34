// chip_internal.h -- private definitions shared by the translation units of libcerebro_hip.so.
// gfx950 / CDNA4 only: wave = 64 lanes, no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>
#include <utility>
#include <condition_variable>
#include <vector>
#include "../../include/cerebro_hip.h"

namespace chip {

constexpr int kWave = 64;
constexpr int kMaxSegs = 4096;          // segment table entries (device resident)
constexpr int64_t kSegBytesTarget = 512ll << 20;  // ~512 MiB per DB segment

// ---- launch argument blocks (passed by value; all members wave-uniform) ----
struct ScanArgs {
    const void *const *seg_table;   // device array of segment base pointers (rows of float or double: Ctx::elem)
    int32_t seg_shift;              // local row r lives in segment r >> seg_shift ...
    int64_t seg_mask;               // ... at row (r & seg_mask)
    int64_t n_rows;                 // local rows [0, n_rows) are scanned
    int32_t D;
    int32_t K;
    const void *q[CHIP_MAX_NQ];     // query descriptors (device, storage type, D each, 16-B aligned)
    int64_t idx_mul, idx_add;       // global index = local * idx_mul + idx_add  (round-robin shard map)
    chip_topk_entry *partial;       // [gridDim.x][NQ][K]
    int32_t q64 = 0;                // queries staged in LDS as fp64 (scan_q64)
    int32_t rows_form = 0;          // > 0: row-batched kernel with this many rows per wave in flight (scan_rows_form)
    int32_t plain_loads = 0;        // row-batched kernel: temporal loads (the prefix fits the Infinity Cache and is re-read every tick)
    int32_t dyn_claim = 0;          // row-batched kernel, R = 1: the waves of a workgroup CLAIM their rows from an LDS counter instead of the static map (CHIP_SCAN_CLAIM=1)
    unsigned long long *stamps = nullptr;   // tuning only (CHIP_SCAN_STAMPS): 4 wall-clock stamps per wave of the row-batched kernel
    // fused tick (row-batched kernel, plain ctx): the LAST workgroup to finish reduces the per-workgroup best entries and writes the
    // decision record itself -- a tick is then ONE launch.  fused_result == nullptr: lists only, K2 follows as a launch of its own.
    chip_tick_result *fused_result = nullptr;
    int32_t *fused_ticket = nullptr;        // arrival counter of this launch's list buffer (0 at launch, reset by the last workgroup)
    unsigned long long *fused_seq = nullptr; // completion word of the tick's slot in pinned host memory: written (system-scope RELEASE) after the
    unsigned long long fused_seq_val = 0;    // record, so that a host that polls it sees the record complete (chip_api.hip tick_collect_slot)
    int64_t tick_l = 0;
    int32_t locality = 0;
    double thresh = 0.0;
};

// ---- resident scan (opt-in: CHIP_TICK_RESIDENT=1; kernels.hip db_scan_resident, resident.hip) ----
// A synchronous tick over a cache-sized prefix is ~4 us of host API up to the doorbell + ~3 us from the doorbell to the first wave in
// front of a ~29 us kernel (profiles/r05_short_scan.md).  With the mode on, ONE instance of the row-batched scan stays on the chip (one
// workgroup per CU, the shape such a tick launches anyway) and runs the scan body once per COMMAND: the host writes a 64-byte line in
// pinned memory, workgroup 0 polls it over PCIe and relays it to the other workgroups through device memory.
struct ResidentCmd {           // exactly one 64-byte line: read by the device with ONE wave load, accepted when head == tail
    uint32_t head;             // command number, written first ...
    int32_t locality;
    int64_t n_rows;            // rows of the prefix;  < 0: leave
    int64_t tick_l;            // the tick's l (queries: rows l-1, l-2, l-3)
    double thresh;
    uint64_t result;           // chip_tick_result * (device address of the slot's pinned record)
    uint64_t seq_ptr;          // the slot's completion word (device address) ...
    uint64_t seq_val;          // ... and what to store there
    uint32_t dyn_claim;
    uint32_t tail;             // ... == head, written last
};
static_assert(sizeof(ResidentCmd) == 64, "one cache line, one PCIe read");
constexpr uint32_t kResidentLeave = 0xffffffffu;   // head / tail of the line that sends the workgroups home (never a command number)

struct ResidentArgs {
    ScanArgs base;                    // everything a command does not carry (segment table, D, lists, ticket, shard map)
    const uint32_t *cmd_host;         // the ResidentCmd line the host writes: pinned host memory, or device memory behind a large PCIe BAR
    uint32_t *cmd_dev;                // one 64-byte line per workgroup in device memory: workgroup 0 copies the accepted line into each
    unsigned long long *exit_host;    // the instance stores its id here (system-scope release) when it leaves
    unsigned long long instance;
    unsigned long long lease_ticks;   // 100 MHz ticks without a command after which the instance leaves by itself (a dead host must
                                      // not hold the chip; a live one relaunches on its next tick)
    uint32_t done;                    // number of the last command completed before this instance was launched
    uint32_t direct;                  // 1: the HOST writes every workgroup's line (device memory behind the PCIe BAR); workgroup 0 relays
                                      //    nothing but its own decision to leave
};

// ---- several ticks in one DB pass (kernels.hip shared_pass: db_scan_topk_multi / db_scan_shared_f64 / db_scan_prefilter; chip_api.hip coalesce_*) ----
constexpr int kMultiMaxTicks = 3;                   // ticks of 3 queries each that one exact pass can serve (9 fp32 queries of 4096 elements = 144 KiB of LDS; double rows: 2)
// four ticks in one DB pass: fp32 prefilter + certified exact rescoring (kernels.hip db_scan_prefilter / tick_rescore)
constexpr int kPrefilterTicks = 4;                  // ticks of the prefilter pass: 12 fp32 queries, those the LDS does not hold are read in place
constexpr int kRescoreCap = 32;                     // rows per query that tick_rescore scores exactly; more candidates than that: uncertified
// five ticks in one DB pass: the same prefilter with all 15 queries staged in LDS as fp16 (kernels.hip db_scan_halfq)
constexpr int kHalfqTicks = 5;
constexpr int kPassMaxTicks = kHalfqTicks;          // the deepest pass: what PassArgs, RescoreArgs, Ctx::parked and the list buffers are sized for
struct PassArgs {                                   // one shared pass of T <= kPassMaxTicks ticks, whichever kernel serves it
    const void *const *seg_table;                   // as ScanArgs (plain single-GPU ctx: global index == local row)
    int32_t seg_shift;
    int64_t seg_mask;
    int64_t n_rows;                                 // rows [0, n_rows) are read: the longest prefix of the pass
    int32_t D;
    int32_t K;
    int64_t k[kPassMaxTicks];                       // tick t sees rows [0, k[t])
    const void *q[3 * kPassMaxTicks];               // queries of tick t: q[3 t .. 3 t + 2] (device, the rows' type, D each, 16-B aligned)
    chip_topk_entry *partial;                       // [tick][gridDim.x][3][K]: every tick's block of lists is what ONE launch of db_scan_topk leaves
                                                    // (prefilter: fp32 score widened to double, row; sorted by score desc, index desc)
    float q_up;                                     // db_scan_halfq only: 2^e, what a query is multiplied by before it is rounded to fp16 ...
    double s_down, s_up;                            // ... and 2^-e, 2^e: a score on its way into a list (exact in fp64) and a threshold on its way back
};
struct RescoreArgs {                                // one launch per pass: workgroup 3 t + i serves query i of tick t
    const void *const *seg_table;
    int32_t seg_shift;
    int64_t seg_mask;
    int32_t D;
    int32_t K;
    const chip_topk_entry *in;                      // [tick][n_lists][3][K]: the prefilter's lists
    int32_t n_lists;
    int32_t wpb;                                    // waves per workgroup of the pass: with a tick's prefix, how many rows a workgroup owned
    int64_t k[kPassMaxTicks];
    const void *q[3 * kPassMaxTicks];
    double E;                                       // bound on |fp32 score - exact score| of every pair of published rows, rounded up
    chip_topk_entry *out;                           // [tick][3][K] exact lists: a tick's block is what topk_merge reads as ONE workgroup's lists
    uint32_t *cert[kPassMaxTicks];                  // per tick three words in pinned host memory: 1 the query's certificate holds, 2 it does not
};
// K2 of a five-tick pass: ONE launch, workgroup t merges tick t's three exact lists and writes its record (kernels.hip pass_merge)
struct PassMergeArgs {
    const chip_topk_entry *in;                      // [tick][3][K]: what tick_rescore left
    int32_t K;
    chip_tick_result *result[kPassMaxTicks];
    int64_t l[kPassMaxTicks];
    int32_t locality[kPassMaxTicks];
    double thresh[kPassMaxTicks];
};

struct MergeArgs {
    const chip_topk_entry *in;      // [n_lists][NQ][K]
    int32_t n_lists;
    int32_t K;
    chip_topk_entry *out;           // [NQ][K]   (may be null)
    chip_tick_result *result;       // decision record (may be null => no decision)
    int64_t l;                      // tick position (for idx_curr)
    int32_t locality;
    double thresh;
};

// bulk ticks (batch.hip chip_loop_ticks_bulk): one launch of bulk_tick_finish (kernels.hip) per group, workgroup t finishes tick t
struct BulkFinishArgs {
    const void *const *seg_table;
    int32_t seg_shift;
    int64_t seg_mask;
    int32_t D;
    int32_t KL;                     // entries per list of the group (the library's own choice, <= CHIP_MAX_TOPK)
    int32_t K;                      // the caller's topk <= KL
    const chip_topk_entry *lists;   // [group queries][KL]: what topk_merge_batch left; query 3 t + i is row l_t - 1 - i
    const int64_t *rows;            // [group queries] the query rows (the gather's image of them)
    double E;                       // as RescoreArgs
    int32_t locality;
    double thresh;
    chip_tick_result *rec;          // [ticks]
    chip_topk_entry *out;           // [ticks][3][K] exact lists
    uint32_t *words;                // [ticks][2]: 1 certified (all three queries) / 2 not, rows scored exactly
};

struct Ctx;

// ---- owned memory: an array of T in device memory (DevBuf) or in pinned, device-mapped host memory (PinnedBuf).  Freed by the destructor.
// reserve(): grow-only scratch.  Nothing but a compare when n fits; otherwise the old array is freed and n elements are allocated inside a
// ResidentPause (hipFree waits for the whole device, see resident_pause), so no free of a live ctx happens outside a pause.  A unit that
// regrows several buffers in one go keeps ONE pause of its own over the group (pauses nest): that is what stops the tick thread relaunching
// an instance between two frees.  Contents are not kept; after a failure the buffer is empty and the status is CHIP_HIP's.
// alloc(): the one allocation of a fixed-size buffer, WITHOUT a pause: for create (no instance can exist yet) and for code that holds
// Resident::mu (resident_alloc_body) -- resident_pause takes that mutex, so reserve() must never be called with it held.
template <class T> class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(Ctx *c, size_t n);
    int reserve(Ctx *c, size_t n);
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    void swap(DevBuf &o) { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }   // (the caller frees what it got inside a pause of its own)
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }
private:
    T *p_ = nullptr;
    size_t cap_ = 0;   // elements
};
template <class T> class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    int alloc(Ctx *c, size_t n);
    int reserve(Ctx *c, size_t n);
    void release() { if (h_) (void)hipHostFree(h_); h_ = d_ = nullptr; cap_ = 0; }
    T *host() const { return h_; }
    T *dev() const { return d_; }   // the same memory as the device addresses it
    size_t capacity() const { return cap_; }
private:
    T *h_ = nullptr, *d_ = nullptr;
    size_t cap_ = 0;
};

// ---- descriptor projection (project.hip): z = normalise(Mt x + b) made on the device, for chip_project and the projected append.
// Everything is guarded by append_mu: the calls are appends, or share the append's stream and staging buffer.
struct Projection {
    DevBuf<char> buf;                 // [matrix: D rows of in_dim elements][bias: D doubles][y: one group's descriptors x D doubles], replaced as a whole
    DevBuf<float> x;                  // the raw descriptors of the running call (n x in_dim), grown on demand
    size_t mat_bytes = 0;
    int32_t in_dim = 0;               // 0: no projection set
    int32_t matrix_type = 0;          // CHIP_PROJ_F32 / CHIP_PROJ_F64
    int32_t D = 0;
    bool has_bias = false;
    int64_t last_passes = 0, last_singles = 0, last_pass_descriptors = 0;   // what the last projecting call launched (chip_debug_project_last)
    double *bias() const { return reinterpret_cast<double *>(buf.get() + mat_bytes); }
    double *y() const { return bias() + D; }
};
// Where the rows of an append come from: host rows of `elem` bytes per value, or (raw != null) n raw descriptors for the ctx's
// projection -- host memory or memory of the ctx's device -- whose rows are made in the staging buffer as doubles (elem == 8).
struct AppendSrc {
    const void *desc;
    int elem;
    const float *raw = nullptr;
    const float *fmap = nullptr;      // a third kind (vlad.hip): n_maps feature maps of `positions` positions in `layout`, one after the other,
    int32_t positions = 0;            // each pooled into one row -- directly (clusters * channels == D) or through the ctx's projection
    int32_t layout = 0;               // (== its in_dim)
    int32_t n_maps = 0;
};
int project_stage_input(Ctx *c, const float *x, int64_t n);   // raw descriptors -> Projection::x, enqueued on s_append
int project_chunk(Ctx *c, int64_t from, int64_t m);           // staged descriptors [from, from + m) -> rows 0 .. m-1 of stage_dev, on s_append
void project_count_reset(Ctx *c);                             // a projecting call begins: chip_debug_project_last counts from here

// ---- NetVLAD pooling (vlad.hip): feature map -> pooled float32 vector, for chip_vlad and the pooled append.  Guarded by append_mu.
struct Vlad {
    DevBuf<char> w;                   // [bias: K+G doubles, padded to an even count][Wt: (K+G) x C floats][centres: K x C floats], replaced as a whole
    // the scratch of one GROUP of maps (vlad.hip vlad_group; a single call is a group of one), every array map-major:
    DevBuf<float> raw;                // CHIP_VLAD_NCHW maps as they came, before the transposing stage-in
    DevBuf<float> x;                  // the maps of the running group, maps x N x C
    DevBuf<double> a;                 // soft assignment, maps x N x (K+G)
    DevBuf<double> part;              // [P_j: maps x blocks x K x C][S_j: maps x blocks x K]
    DevBuf<double> vu;                // [V: maps x K x C][U: maps x K x C][A: maps x K]
    DevBuf<float> out;                // chip_vlad_batch: [v: maps x K x C floats][flag word]
    int32_t C = 0, K = 0, G = 0;      // C == 0: no weights set
    int32_t last_n = 0;               // positions per map of the last pooled group whose stages a, V, A are on the device (0: none)
    int32_t last_maps = 0;            // and its maps: chip_debug_vlad_stage reads the last one's
    int bias_count() const { return (K + G + 1) & ~1; }
    double *bias() const { return reinterpret_cast<double *>(w.get()); }
    float *Wt() const { return reinterpret_cast<float *>(w.get() + (size_t)bias_count() * sizeof(double)); }
    float *centres() const { return Wt() + (size_t)(K + G) * C; }
};
int vlad_chunk(Ctx *c, const AppendSrc &src, int64_t from, int64_t m);   // maps [from, from + m) -> rows 0 .. m-1 of stage_dev (directly, or through project_chunk), on s_append

// kernels.hip
int launch_resident(Ctx *c, hipStream_t s, const ResidentArgs &ra, int grid);   // CHIP_ERR_UNSUPPORTED in a build without the rows form
int launch_scan(Ctx *c, hipStream_t s, const ScanArgs &a, int nq, int grid);
int launch_merge(Ctx *c, hipStream_t s, const MergeArgs &a, int nq);
int scan_multi_max_ticks(const Ctx *c);   // ticks one shared pass can serve on this ctx (0 / 2 / 3: storage type, D, LDS)
// the shared pass for n_ticks ticks over rows of D elements of elem bytes: staged (q64, double rows) / in-place (NG) queries, LDS, shape -- or CHIP_ERR_UNSUPPORTED
int scan_multi_plan(int D, int elem, int n_ticks, int K, int grid, chip_debug_scan_launch *f);
int scan_multi_grid(const Ctx *c);
int launch_scan_multi(Ctx *c, hipStream_t s, const PassArgs &a, int n_ticks, int grid);
// the prefilter pass of kPrefilterTicks ticks over float rows of D elements: staged / in-place (NG) queries, LDS, shape -- or CHIP_ERR_UNSUPPORTED
int scan_prefilter_plan(int D, int elem, int K, int grid, chip_debug_scan_launch *f);
bool scan_prefilter_usable(const Ctx *c);           // this ctx may serve four parked ticks with the prefilter pass (row norms included)
double prefilter_error_bound(int D, double row_norm_max);   // E of DESIGN.md 3, rounded up
int launch_scan_prefilter(Ctx *c, hipStream_t s, const PassArgs &a, int grid);
// the five-tick pass over float rows of D elements: all 15 queries staged as fp16 (NG = 0) -- or CHIP_ERR_UNSUPPORTED
int scan_halfq_plan(int D, int elem, int K, int grid, chip_debug_scan_launch *f);
bool scan_halfq_usable(const Ctx *c);               // this ctx may serve five parked ticks with the fp16-query pass (row norms included)
int halfq_exponent(double row_norm_max);            // e: the staged queries are fl16(2^e q), 2^e N <= 2^15
double halfq_error_bound(int D, double row_norm_max, int e);   // E_h of DESIGN.md 3, rounded up
int launch_scan_halfq(Ctx *c, hipStream_t s, const PassArgs &a, int grid);   // (a.q_up, a.s_down, a.s_up set from halfq_exponent)
int launch_rescore(Ctx *c, hipStream_t s, const RescoreArgs &a, int n_ticks);
int launch_pass_merge(Ctx *c, hipStream_t s, const PassMergeArgs &a, int n_ticks);
int launch_bulk_finish(Ctx *c, hipStream_t s, const BulkFinishArgs &a, int n_ticks);
int scan_grid_for(const Ctx *c, int64_t n_rows, int nq, bool q64);
bool scan_q64(const Ctx *c, int nq, bool long_scan);
int scan_rows_form(const Ctx *c, int64_t n_rows, int nq, int grid, bool q64, bool sync_tick = false);
// Which instantiation a launch of K1 is (family, template arguments, shape, LDS): the ONE place that chooses it.  launch_scan launches
// what this says and keeps the record (Ctx::last_scan, chip_debug_last_scan); chip_debug_scan_plan calls it on a ctx without a device.
int scan_select(const Ctx *c, const ScanArgs &a, int nq, int grid, chip_debug_scan_launch *f);
int scan_forms_built();              // CHIP_SCAN_FORM_* bits of this build (-DCHIP_NO_ROWS_FORM leaves the row-batched kernel out)
int launch_scores(Ctx *c, hipStream_t s, const ScanArgs &a, double *out_dev);   // K1s: all scores of one query, out[local row]
int launch_store_rows(Ctx *c, hipStream_t s, const void *src, int src_elem, int64_t n, int64_t first_global, uint32_t *flags_dev, bool write_ring,
                      int64_t row_stride = 1);
int launch_synth(Ctx *c, hipStream_t s, int64_t first_global, int64_t n, uint64_t seed,
                 const int64_t *plant_dst_dev, const int64_t *plant_src_dev, const int32_t *plant_kind_dev, int64_t n_plant, int unit);

// How a slot is collected (tick_collect_slot).  Set once per tick, where it is known (the writer is named on the right):
enum class SlotState : uint8_t {
    Free,        // nothing enqueued                                                              tick_collect_slot (every way out but a failed wait)
    Immediate,   // result already final on the host (skipped / too short)                        tick_begin
    Parked,      // enqueued, not yet submitted: waits for company in Ctx::parked                 tick_enqueue_slot
    Event,       // wait for wait_ev                                                              tick_submit, coalesce_submit, merge_enqueue_slot (exchange / group ticks)
    Poll,        // poll seq_host for seq_want, wait_ev if the word does not arrive               tick_submit (fused launch, CHIP_TICK_POLL)
    Resident,    // command to the resident scan instance: no event, the completion word is all  resident_tick_enqueue
    Failed,      // the pass this tick left with could not be submitted: collect returns err     coalesce_flush
};

struct Slot {
    hipEvent_t done = nullptr;
    hipEvent_t wait_ev = nullptr;       // what collect waits for: `done`, or the merge event of the tick's list buffer (same-stream ticks)
    PinnedBuf<chip_tick_result> rec;    // the decision record: the deciding workgroup stores it straight into host memory
    SlotState state = SlotState::Free;
    int64_t prev_last_l = 0;            // last_l before this tick was enqueued ...
    int64_t tick_l = 0;                 // ... the l this tick committed ...
    unsigned long long *seq_host = nullptr, *seq_dev = nullptr;   // completion word of this slot (in Ctx::seq_all)
    unsigned long long seq_want = 0;    // value the fused tick in flight will store there
    uint64_t pass_no = 0;               // Ctx::pass_no of the long scan that serves this tick
    int32_t err = 0;                    // SlotState::Failed: what collect returns
    // a tick served by the prefilter pass: what collect needs to run it again alone if its certificate did not hold
    bool prefilter = false;
    uint32_t *cert_host = nullptr, *cert_dev = nullptr;   // this slot's three words in Ctx::cert_all (one per query): 1 certified, 2 not
    int64_t pf_k = 0;
    chip_dot_params pf_p{};
    const void *pf_q[3] = {};
    int64_t *last_l_ptr = nullptr;      // ... and where to restore it if the tick comes back CHIP_TICK_FAILED (only while no newer
                                        //     tick has been enqueued: *last_l_ptr == tick_l)
};

// ---- resident scan instance (resident.hip): everything the opt-in mode keeps.  Guarded by `mu`, which queriers (query_mu held) and the
// appender (append_mu held) take LAST; `enabled` and `busy` are written with query_mu held as well: the tick path reads them under it alone.
struct Resident {
    bool enabled = false;                   // CHIP_TICK_RESIDENT=1 in a build with the row-batched kernel, and no set-up has failed
    double max_bytes = 512.0 * 1024 * 1024; // prefixes up to this size take it (CHIP_RESIDENT_MAX_MIB)
    int32_t lease_ms = 250;                 // CHIP_RESIDENT_LEASE_MS
    hipStream_t stream = nullptr;
    PinnedBuf<char> pinned;                 // the allocations behind the pointers below: 128 bytes, the command line + the line of the exit word
    DevBuf<char> cmd_vram;                  // ... one line in device memory (CHIP_RESIDENT_BAR=1)
    bool cmd_in_vram = false;               // the command line is in device memory, written by the host through the PCIe BAR
    bool direct = false;                    // ... and so is every workgroup's own line (no relay): CHIP_RESIDENT_BAR=2
    ResidentCmd pending{};                  // the command in flight (re-posted to an instance launched for it)
    int64_t test_skip_master = 0;           // test hook (CHIP_TEST_RESIDENT_SKIP_MASTER)
    bool test_skipped = false;
    ResidentCmd *cmd_host = nullptr;        // the line as the host writes it + its device address
    uint32_t *cmd_hostdev = nullptr;
    DevBuf<uint32_t> cmd_dev;               // [max_grid] lines of 64 bytes
    unsigned long long *exit_host = nullptr, *exit_hostdev = nullptr;
    DevBuf<chip_topk_entry> partial;
    DevBuf<int32_t> ticket;                 // one 64-byte line
    unsigned long long instance = 0;        // id of the instance launched last (0: none yet)
    bool alive = false;                     // launched and not yet seen to have left
    bool ready = false;                     // resident_alloc has completed: every buffer above exists (published LAST)
    int32_t inhibit = 0;                    // > 0: no instance may be launched (resident_pause .. resident_resume); ticks are launched meanwhile
    bool busy = false;                      // a command is in flight (one at a time)
    uint32_t cmd_no = 0, done = 0;          // last number posted / last number seen complete
    int32_t grid = 0;
    Slot *slot = nullptr;                   // the slot of the command in flight
    int64_t ticks = 0, launches = 0;        // ticks it has served / instances launched (chip_debug_resident_stats)
    std::mutex mu;
};

struct PnpState;   // pnp.hip / icp.hip / batch.hip / match.hip: a unit's scratch, created on first use (PnP: at create)
struct IcpState;
struct BatchState;
struct MatchState;
struct FrameStore; // frame_store.h: the frame store and the buffers of the calls that fill it
struct OrbState;
struct Exchange;   // chip_multi.hip: how a sharded ctx trades its per-shard top-k lists (RCCL communicator / device copies)
struct Group;      // chip_multi.hip: a ctx made of G per-device sub-contexts driven from one process

struct Ctx {
    int32_t D = 0;
    int32_t device = 0;
    int32_t rank = 0, nranks = 1;
    int32_t n_cus = 0;
    char arch[32] = {0};

    // --- storage type: 4 = float rows (default), 8 = double rows.  store_auto: still undecided -- the first append of a
    //     descriptor that is not float32-representable into the EMPTY DB switches to double (chip_create semantics).
    int32_t elem = 4;
    bool store_auto = true;

    // --- DB storage: fixed-size segments, never moved once allocated ---
    int32_t seg_shift = 0;
    int64_t seg_rows = 0;
    std::vector<void *> segs;            // host copy of the table
    DevBuf<void *> seg_table_dev;        // device table [kMaxSegs]
    DevBuf<char> ring_dev;               // [CHIP_RING_ROWS][D]  most recent rows (all ranks)
    int64_t rows_global = 0;             // published length (guarded by mu)
    int64_t rows_local = 0;
    int64_t lossy_rows = 0;
    mutable std::mutex mu;               // guards rows_*, segs growth
    std::mutex append_mu;                // serialises appenders
    mutable std::mutex query_mu;         // serialises queriers (scratch buffers are per ctx); guards last_l
    std::mutex ring_mu;                  // sharded: ring residency check .. scan event  vs  the appender's ring writes
    int64_t rows_pending = 0;            // length an in-flight append will publish (ring_mu)
    hipEvent_t last_scan_ev[2] = {};     // newest scan per scan stream (ring_mu)
    std::mutex pnp_mu;
    std::mutex icp_mu;            // ICP has its own stream and lock: it may run underneath a PnP call

    // --- streams ---
    hipStream_t s_query = nullptr, s_append = nullptr, s_pnp = nullptr;
    bool own_query_stream = true;

    // --- append staging ---
    DevBuf<char> stage_dev;              // staging for host descriptors
    size_t stage_bytes = 0;
    DevBuf<uint32_t> flags_dev;          // bit0: not-f32-representable, bit1: non-finite, bit2: finite but +-Inf as a float
    PinnedBuf<uint32_t> flags_host;
    DevBuf<unsigned long long> norm2_dev;     // float rows: bits of the largest fp64 sum of squares among the rows the running append has stored
    PinnedBuf<unsigned long long> norm2_host;
    double row_norm_max = 0.0;                // upper bound on the L2 norm of every published row (float rows; mu): sqrt of the above, times 1 + 2^-30

    // --- query scratch ---
    // Scans run back-to-back on s_scan; the merge of tick i runs on the ctx stream (s_query) behind ev_scan[b], so
    // it (and, sharded, the all-gather + global merge that follow it on the ctx stream) overlaps the scan of tick
    // i+1.  Partial lists live in a ring of kRing buffers; a scan waits for the merge that last read its buffer.
    // Deeper than the number of ticks a caller can keep in flight (CHIP_MAX_INFLIGHT): in steady state the merge that last
    // read a buffer is long complete when its next scan is enqueued, so no barrier packet is put in front of the scan
    // (each one costs the scan stream ~7 us; 64 x 512 KiB of HBM is nothing).
    static constexpr int kRing = 64;
    hipStream_t s_scan = nullptr;
    hipStream_t s_scan2 = nullptr;   // second scan stream for short scans (CHIP_SCAN_STREAMS=1 disables)
    hipStream_t s_scan_x[2] = {};    // third / fourth stream of the same-stream short tick (CHIP_SCAN_STREAMS, default 4)
    uint64_t n_same_stream = 0;      // same-stream ticks so far (round robin over the tick streams)
    DevBuf<chip_topk_entry> partial_dev[kRing]; // [max_grid][CHIP_MAX_NQ][CHIP_MAX_TOPK]
    int32_t partial_lists[kRing] = {};                               // grid of the scan that filled it
    hipEvent_t ev_scan[kRing] = {};             // scan into buffer b finished
    hipEvent_t ev_merged[kRing] = {};           // merge out of buffer b finished
    DevBuf<int32_t> tickets_dev;                // [kRing] arrival counters of the fused tick (one per list buffer)
    PinnedBuf<unsigned long long> seq_all;      // [CHIP_MAX_INFLIGHT] completion words of the slots
    unsigned long long tick_seq = 0;            // last value handed out
    bool tick_poll = true;                      // CHIP_TICK_POLL: fused ticks are collected by polling the completion word
    bool tick_fused = true;                     // CHIP_TICK_FUSED=0 disables
    Resident res;                               // resident scan instance (CHIP_TICK_RESIDENT=1; resident.hip)
    uint64_t n_enqueued = 0;
    int32_t max_grid = 0;
    PinnedBuf<chip_topk_entry> topk;          // [CHIP_MAX_NQ][CHIP_MAX_TOPK]: the last block writes results straight here

    DevBuf<char> qvec_dev;                    // [CHIP_MAX_NQ][D] external query vectors (storage type)
    DevBuf<double> scores_dev;                // chip_query_scores scratch (grown on demand)
    DevBuf<unsigned long long> stamps_dev;    // tuning only (CHIP_SCAN_STAMPS=1): [max_grid * 16 waves][4]

    // --- sharded tick inside the library (chip_multi.hip) ---
    std::vector<char> qconv;                  // host conversion scratch of external query vectors
    int64_t cap_hint = 0;
    int32_t group_transport = 0;              // CHIP_EXCHANGE_* of a group ctx
    mutable int last_comm = 0;                // last ncclResult_t (1000: a bootstrap was abandoned at its deadline)
    int32_t comm_init_abandoned = 0;          // a helper thread of this ctx is still inside an RCCL bootstrap (chip_multi.hip)
    Exchange *xchg = nullptr;                 // non-null: chip_loop_tick* work on this sharded ctx
    Group *group = nullptr;                   // non-null: this ctx is a group of per-device sub-contexts
    Ctx *parent = nullptr;                    // sub-context of a group
    Slot slots[CHIP_MAX_INFLIGHT];
    int64_t last_l = 0;

    // --- several pipelined ticks per DB pass (chip_api.hip coalesce_*; query_mu) ---
    struct ParkedTick { Slot *slot; int64_t k, l; chip_dot_params p; const void *q[3]; };
    int32_t coalesce_max = 5;            // CHIP_TICK_COALESCE: 0 = every tick is a pass of its own, 2 .. 5 = at most that many ticks per pass
    bool coalesce_force = false;         // chip_debug_coalesce_force: park even when no scan is running (tests)
    ParkedTick parked[kPassMaxTicks];
    int32_t n_parked = 0;
    hipEvent_t pass_ev = nullptr;        // end of the newest long scan submitted (one of ev_scan[])
    bool pass_shared = false;            // ... and whether that scan is a shared pass (false: one tick's launch)
    uint64_t pass_no = 0;                // long scans submitted so far
    int64_t coalesce_passes = 0, coalesce_ticks = 0;   // passes of more than one tick / the ticks they served (chip_debug_coalesce_stats)
    int64_t prefilter_passes = 0, prefilter_ticks = 0, prefilter_uncertified = 0;   // prefilter passes / their ticks / those of them run again alone
    PinnedBuf<uint32_t> cert_all;        // [CHIP_MAX_INFLIGHT][4] certificate words of the slots (three used)
    chip_debug_scan_launch last_scan{};  // the last top-k scan launched (launch_scan / launch_scan_multi; query_mu): chip_debug_last_scan
    // the last prefilter pass submitted (coalesce_submit; query_mu): where its lists are and what it was launched with -- chip_debug_last_pass.
    // The list buffer is not reused before kRing further enqueues; the certificate words are the slots' own (pinned host memory), which
    // only the next prefilter pass through the same slot overwrites.
    struct LastPass { int32_t family = 0, ticks = 0, grid = 0, wpb = 0, K = 0, e = 0, ring = 0; double E = 0.0; int64_t k[kPassMaxTicks] = {}; const uint32_t *cert[kPassMaxTicks] = {}; } last_pass;

    // --- scan tuning (resolved at create; CHIP_SCAN_* env overrides for A/B runs) ---
    int32_t scan_block = 0;       // 0 = auto
    int32_t scan_blocks_per_cu = 2;
    int32_t scan_reserve = 0;
    int32_t scan_variant = 0;
    int32_t scan_streams = 4;      // CHIP_SCAN_STREAMS: tick streams created (1: s_scan alone, 2: + s_scan2, 3 / 4: + s_scan_x)
    bool tick_same_stream = true;  // short ticks of a plain ctx: merge on the scan's stream (CHIP_TICK_SAME_STREAM=0 disables)
    int32_t scan_claim = -1;      // CHIP_SCAN_CLAIM: rows claimed within the workgroup (row-batched kernel, R = 1): -1 auto, 0 never (static row -> wave map), 1 always
    int32_t scan_rows = 0;        // CHIP_SCAN_ROWS: 0 = auto (prefixes up to scan_plain_bytes), 1..3 = row-batched kernel with that R for every scan, -1 = never
    double scan_plain_bytes = 768.0 * 1024 * 1024;   // prefixes up to this size: rows form, R = 1, temporal loads (CHIP_SCAN_PLAIN_MIB)
    double scan_sync_plain_bytes = 4096.0 * 1024 * 1024;   // SYNCHRONOUS ticks: the row-batched (fused, one-launch) form up to this size (CHIP_SCAN_SYNC_PLAIN_MIB)
    double scan_half_bytes = 192.0 * 1024 * 1024;    // prefixes up to this size: launches take half of every CU's workgroup slots (CHIP_SCAN_HALF_MIB)
    int32_t scan_short_bpc = 1;       // workgroups per CU of a launch over a cache-sized prefix (CHIP_SCAN_SHORT_BPC; 0 = as any other)
    double scan_overlap_bytes = 8.0 * 1024 * 1024 * 1024;   // launches up to this size alternate between the two scan streams (CHIP_SCAN_OVERLAP_GIB)

    // --- profiling ---
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;     // start/stop pairs
    size_t prof_used = 0;
    double prof_bytes_last = 0.0;

    // --- pnp scratch (pnp.hip) ---
    PnpState *pnp_state = nullptr;
    IcpState *icp_state = nullptr;
    BatchState *batch_state = nullptr;
    MatchState *match_state = nullptr;
    FrameStore *frame_store = nullptr;   // frames.hip: created by the first frame call that needs it; guarded by match_mu
    OrbState *orb_state = nullptr;   // orb.hip: created by the first chip_orb_detect; its calls take match_mu
    Projection proj;                 // project.hip (append_mu)
    Vlad vlad;                       // vlad.hip (append_mu)
    std::mutex match_mu;         // serialises the matching calls of a ctx; taken BEFORE pnp_mu / icp_mu (chip_*_ransac_matched)

    mutable hipError_t last_hip = hipSuccess;
};

#define CHIP_HIP(ctx, expr)                                  \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) {                              \
            (ctx)->last_hip = _e;                            \
            return _e == hipErrorOutOfMemory ? CHIP_ERR_OOM : CHIP_ERR_HIP; \
        }                                                    \
    } while (0)

// global index <-> local row (round-robin sharding)
inline bool owns_row(const Ctx *c, int64_t g) { return c->nranks == 1 || (g % c->nranks) == c->rank; }
inline int64_t local_of(const Ctx *c, int64_t g) { return c->nranks == 1 ? g : g / c->nranks; }
// number of local rows among global rows [0,k)
inline int64_t local_count(const Ctx *c, int64_t k) {
    if (c->nranks == 1) return k;
    return k > c->rank ? (k - c->rank + c->nranks - 1) / c->nranks : 0;
}
inline char *row_ptr_host(const Ctx *c, int64_t local) {
    return static_cast<char *>(c->segs[(size_t)(local >> c->seg_shift)]) + (local & (c->seg_rows - 1)) * (int64_t)c->D * c->elem;
}
inline char *ring_ptr(const Ctx *c, int64_t g) {
    return c->ring_dev + (g % CHIP_RING_ROWS) * (int64_t)c->D * c->elem;
}

// ---- chip_api.hip: single-ctx building blocks, shared with chip_multi.hip ----
struct RingGuard {   // sharded ctx: residency check .. scan event recorded, vs the appender's ring writes (see query_row_ptrs)
    std::unique_lock<std::mutex> lk;
    explicit RingGuard(Ctx *c) : lk(c->ring_mu, std::defer_lock) { if (c->ring_dev) lk.lock(); }
};
int ctx_create(chip_ctx **out, int32_t D, int64_t capacity_hint, int32_t device, int32_t rank, int32_t nranks, uint32_t flags);
void ctx_destroy(chip_ctx *c);
int ctx_append(Ctx *c, const AppendSrc &src, int64_t n, uint32_t flags, int64_t *first_index);
// the phases of an append, for callers that must take the same decision on several contexts (group_append): reserve -> store the
// DB rows (unpublished; owner_only: upload only the rows this shard owns) -> [switch an empty undecided DB to double rows] ->
// mirror the newest rows into the ring and publish the length.  The caller holds the append lock.
int append_reserve(Ctx *c, int64_t first, int64_t n);
int append_store_db(Ctx *c, const AppendSrc &src, int64_t first, int64_t n, bool owner_only, uint32_t *bad);
bool append_can_switch_to_double(const Ctx *c, int64_t first);
int append_switch_to_double(Ctx *c, int64_t n);
int append_ring_publish(Ctx *c, const AppendSrc &src, int64_t first, int64_t n, bool lossy);
int synth_generate(Ctx *c, int64_t first, int64_t n, uint64_t seed, const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant, int unit);
void append_publish(Ctx *c, int64_t new_total, bool lossy, int64_t n);
int64_t published_rows(const Ctx *c);
int ctx_append_synthetic(Ctx *c, int64_t n, uint64_t seed, const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant, int unit);
int ctx_read_row(Ctx *c, int64_t g, int64_t total, void *out);          // one row, storage type, async on s_query
int query_row_ptrs(Ctx *c, const int64_t *rows, int nq, int64_t n_global, const void **q);
int upload_query_vectors(Ctx *c, const void *queries, int src_elem, int nq, const void **q);   // -> qvec_dev (on s_scan)
struct ScanRequest {                        // what enqueue_scan_merge is asked for; with its receipt, on the caller's stack
    int64_t k = 0;                          // the global prefix [0, k)
    const void *const *q = nullptr;         // nq query descriptors (device, storage type)
    int nq = 0;
    int K = 0;
    chip_topk_entry *out = nullptr;         // [nq][K] lists (device or pinned host); null: none
    chip_tick_result *res = nullptr;        // decision record of Cerebro.cpp:1056 (needs p); null: no decision
    int64_t l = 0;                          // tick position
    const chip_dot_params *p = nullptr;
    bool tick = false;                      // the queries are resident rows: the launch may leave s_scan for another tick stream
    bool sync_tick = false;                 // a synchronous chip_loop_tick: the scan form is chosen for latency, not throughput
    bool merge_on_scan_stream = false;      // the caller accepts the scan's stream as the merge stream (it orders what follows by the receipt)
    unsigned long long *seq_dev = nullptr;  // completion word a FUSED launch stores seq_val to (null: none)
    unsigned long long seq_val = 0;
};
struct ScanReceipt {
    hipStream_t merge_stream = nullptr;     // the stream the merge (or the fused scan) ran on
    hipEvent_t done_ev = nullptr;           // the tick's completion event, if it has one of its own (merge on the scan's stream); else null
    bool fused = false;                     // the launch was the one-launch tick: the kernel stores the completion word itself
};
int enqueue_scan_merge(Ctx *c, const ScanRequest &rq, ScanReceipt *rcpt = nullptr);
// "This tick's merge stays on the scan's stream", from facts (enqueue_scan_merge and, on a ctx without streams, chip_debug_scan_plan)
bool tick_merge_on_scan_stream(const Ctx *c, bool tick, bool short_scan, bool second_tick_stream, bool caller_accepts);
template <class Args> inline void scan_args_db(const Ctx *c, Args *a)   // the segment-table / D part of a ScanArgs / PassArgs
{
    a->seg_table = c->seg_table_dev; a->seg_shift = c->seg_shift; a->seg_mask = c->seg_rows - 1; a->D = c->D;
}
MergeArgs merge_args(const chip_topk_entry *in, int32_t n_lists, int32_t K, chip_topk_entry *out, chip_tick_result *result, int64_t l, const chip_dot_params *p);
// A profiled launch (prof_on): the next start / stop event pair (prof_ev grows on demand), start recorded on s; the caller records *stop
int prof_begin(Ctx *c, hipStream_t s, double bytes, hipEvent_t *stop);
int merge_enqueue_slot(Ctx *c, int64_t l, const chip_dot_params *p, const void *dev_gathered, int32_t n_lists, int32_t topk, Slot &s);
int merge_enqueue_out(Ctx *c, const void *dev_gathered, int32_t n_lists, int nq, int32_t topk, chip_topk_entry *out);
// The head of every tick: busy check, the reference's bookkeeping against n_rows published rows, what a CHIP_TICK_FAILED rolls back, and for
// SKIPPED / TOO_SHORT the immediate result with its last_l commit.  CHIP_TICK_SCANNED: the caller enqueues the scan over [0, *k) and commits *last_l.
int tick_begin(Slot &s, int64_t n_rows, int64_t *last_l, int64_t l, const chip_dot_params *p, int32_t *status, int64_t *k);
// The rule alone (Cerebro.cpp:960-966, :1019-1022): status and k of a tick at l against n published rows and the loop state last_l, which it does
// not write.  tick_begin and the bulk call (batch.hip bulk_sequence) both come here.  fill_immediate: the record of a tick that is not scanned.
int tick_prepare(int64_t n, int64_t last_l, int64_t l, const chip_dot_params *p, int32_t *status, int64_t *k_out);
void fill_immediate(chip_tick_result *r, int32_t status);
int tick_collect_slot(Ctx *c, Slot &s, chip_tick_result *out);
// Parking policy of the pipelined tick (no device needed): what an enqueue does with a tick that could share a pass, given the ticks
// already parked, the most one pass may serve and whether a scan of this ctx is still running.
enum { kCoalesceLaunch = 0, kCoalescePark = 1, kCoalesceParkFlush = 2 };
int coalesce_decide(int n_parked, int t_max, bool scan_running);
int coalesce_flush(Ctx *c);     // every parked tick leaves now, together, as one pass (query_mu held); no-op with nothing parked
int sync_topk_out(Ctx *c, int nq, int K, double *scores, int64_t *idx);
int ctx_scores_local(Ctx *c, int64_t k, const void *q, double *u_global, int64_t stride_mul, int64_t stride_add);
int env_int(const char *name, int dflt);
void scan_read_knobs(Ctx *c);   // every CHIP_SCAN_* / CHIP_TICK_* variable that decides WHICH scan is launched -> Ctx (chip_create and chip_debug_scan_plan)
// The per-launch policy of a top-k scan over n_local rows: a.q64, a.rows_form, a.plain_loads, a.dyn_claim and the grid.  Returns whether
// the scan is a short one (up to scan_overlap_bytes).
bool scan_policy(const Ctx *c, int64_t n_local, int nq, bool sync_tick, ScanArgs *a, int *grid);
// A tick as ONE launch (kernels.hip fused_tick_finish): same-stream short ticks through the row-batched kernel, decision wanted, no list output
bool scan_tick_fused(const Ctx *c, bool same_stream, const ScanArgs &a, bool decision_only, int nq);
// ---- resident.hip: the resident scan instance ----
void resident_read_knobs(Ctx *c);   // CHIP_TICK_RESIDENT, CHIP_RESIDENT_*, CHIP_TEST_RESIDENT_SKIP_MASTER (chip_create)
bool resident_eligible(Ctx *c, int64_t k);   // query_mu held
constexpr int kResidentPaused = 1;   // (internal, > 0: not a status code) the mode is paused, launch this tick
int resident_tick_enqueue(Ctx *c, int64_t k, int64_t l, const chip_dot_params *p, Slot &s);   // CHIP_OK: s is SlotState::Resident
int resident_collect(Ctx *c, Slot &s);
void resident_wait_command(Ctx *c);   // chip_synchronize: a command in flight is on no stream, its slot's completion word says when it is complete
void resident_destroy(Ctx *c);        // ctx_destroy, after the device is idle
void resident_stop(Ctx *c);    // retire the resident scan instance and wait until it has left the chip (no-op without one): called before
                               // anything that rewrites the segment table, frees device memory or wants the chip to itself
// resident_stop + NO new instance until resident_resume: ticks that arrive meanwhile are launched.  For sections that free / allocate
// device memory (hipFree waits for the whole device -- a tick thread relaunching the instance in between would make it wait for as long
// as ticks keep coming: ADVICE r5) or rewrite the segment table.  Nests; chip_resident_pause / _resume are the public form.  Without an
// instance a pause is one uncontended mutex and a counter.
void resident_pause(Ctx *c);
void resident_resume(Ctx *c);
struct ResidentPause {          // scope guard: every early return of a CHIP_HIP(...) inside the section resumes
    Ctx *c;
    bool on;
    explicit ResidentPause(Ctx *ctx, bool cond = true) : c(ctx), on(cond) { if (on) resident_pause(c); }
    ~ResidentPause() { if (on) resident_resume(c); }
    ResidentPause(const ResidentPause &) = delete;
    ResidentPause &operator=(const ResidentPause &) = delete;
};
template <class T> int DevBuf<T>::alloc(Ctx *c, size_t n)   // (the buffer is empty)
{
    const hipError_t e = hipMalloc((void **)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    CHIP_HIP(c, e);
    cap_ = n;
    return CHIP_OK;
}
template <class T> int DevBuf<T>::reserve(Ctx *c, size_t n)
{
    if (n <= cap_) return CHIP_OK;
    ResidentPause paused(c);
    release();
    return alloc(c, n);
}
template <class T> int PinnedBuf<T>::alloc(Ctx *c, size_t n)
{
    hipError_t e = hipHostMalloc((void **)&h_, n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) h_ = nullptr;
    else if ((e = hipHostGetDevicePointer((void **)&d_, h_, 0)) != hipSuccess) release();
    CHIP_HIP(c, e);
    cap_ = n;
    return CHIP_OK;
}
template <class T> int PinnedBuf<T>::reserve(Ctx *c, size_t n)
{
    if (n <= cap_) return CHIP_OK;
    ResidentPause paused(c);
    release();
    return alloc(c, n);
}
constexpr uint32_t kCreateStoreMask = 3u;   // CHIP_CREATE_STORE_F32 | CHIP_CREATE_STORE_F64

// ---- chip_multi.hip: exchange of per-shard lists inside the library (RCCL / device copies), groups of sub-contexts ----
constexpr int kXRing = 64;                  // >= CHIP_MAX_INFLIGHT: list buffers of a tick are not reused while it is in flight
constexpr int kListEntries = CHIP_MAX_NQ * CHIP_MAX_TOPK;
void exchange_destroy(Ctx *c);
int exchange_comm_ranks(const Ctx *c);      // ncclCommCount of the attached communicator, 0 if none
void group_destroy(Ctx *c);
// sharded ctx with an RCCL communicator attached (one process per GPU): scan -> local merge -> all-gather -> merge, all enqueued
int xchg_tick_enqueue(Ctx *c, int64_t l, int64_t k, const chip_dot_params *p, bool sync_tick, Slot &s, bool fail_local);
int xchg_query(Ctx *c, int64_t k, const void *const *q, int nq, int K, double *scores, int64_t *idx, bool fail_local);
int xchg_fetch_rows(Ctx *c, const int64_t *rows, int nq, int64_t n_local_published, const void **q, bool *fail_local);
// group ctx (chip_create_multi): every entry point of the header that makes sense on a group
int group_append(Ctx *gc, const void *desc, int src_elem, int64_t n, uint32_t flags, int64_t *first_index);
int group_append_synthetic(Ctx *gc, int64_t n, uint64_t seed, const int64_t *pd, const int64_t *ps, const int32_t *pk, int64_t n_plant, int unit);
int group_read_rows(Ctx *gc, const int64_t *rows, int64_t n, void *out, int out_elem);
int group_tick_enqueue(Ctx *gc, int64_t l, const chip_dot_params *p, int32_t slot);
int group_tick_collect(Ctx *gc, int32_t slot, chip_tick_result *out);
int group_query(Ctx *gc, int64_t k, const int64_t *rows, const void *vectors, int vec_elem, int nq, int K, double *scores, int64_t *idx);
int group_scores(Ctx *gc, int64_t k, int64_t query_row, double *u);
int group_synchronize(Ctx *gc);
int group_profile_enable(Ctx *gc, int on);
Ctx *group_root(Ctx *gc);
int group_size(const Ctx *gc);

// batch.hip: the many-query (MFMA) mode in pieces, so that chip_multi.hip can run it over the shards of a DB
int32_t batch_qpad(int32_t Q);            // Q rounded up to the query-tile granularity (BM) of db_gemm_topk
int batch_local_enqueue(Ctx *c, int64_t k, const float *queries, int32_t Q, int32_t topk, chip_topk_entry **out_dev, int32_t *Qpad_out);
int batch_deliver(Ctx *c, const chip_topk_entry *list_dev, int32_t Q, int32_t topk, float *scores, int64_t *idx);
int batch_exchange_buffers(Ctx *c, int n_lists, int32_t Qpad, int32_t topk, chip_topk_entry **gathered, chip_topk_entry **merged, hipEvent_t *ev_done);
int batch_merge_lists(Ctx *c, hipStream_t s, const chip_topk_entry *in, int n_lists, int32_t Qpad, int32_t Q, int32_t topk, chip_topk_entry *out);
int debug_merge_lists(Ctx *c, int form, const chip_topk_entry *lists, int32_t n_lists, int32_t nq, int32_t K, chip_topk_entry *out, int64_t l,
                      const chip_dot_params *p, chip_tick_result *result);   // chip_debug_merge_lists behind its checks
int group_query_batch(Ctx *gc, int64_t k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx, bool cast_rows);
int xchg_query_batch(Ctx *c, int64_t k, const float *queries, int32_t Q, int32_t topk, float *scores, int64_t *idx, bool fail_local, bool cast_rows);

// pnp.hip
int pnp_create(Ctx *c);
void pnp_destroy(Ctx *c);
void icp_destroy(Ctx *c);
void batch_destroy(Ctx *c);
void match_destroy(Ctx *c);   // match.hip
void frame_store_destroy(Ctx *c);   // frames.hip
void orb_destroy(Ctx *c);     // orb.hip
// orb.hip in pieces, so that frames.hip can put a frame straight from its pair (chip_frame_put_orb_stereo).  orb_check: the statuses of
// chip_orb_detect for the size and the parameters, d the parameters in force.  orb_enqueue: the detector and (describe) the descriptor of
// one image -- host memory, or device memory with dense rows -- enqueued on s up to the copy of the first `back` bytes of its output
// (eight int32 kept counts, then the records) into pinned memory; orb_describe writes to desc_dev / kp_dev (null: the state's own
// buffer / nowhere).  orb_finished, once s has drained: the kept total and the counts.  The caller holds match_mu throughout.
int orb_check(int32_t width, int32_t height, const chip_orb_params *p, chip_orb_params *d);
int orb_enqueue(Ctx *c, hipStream_t s, const uint8_t *image, const uint8_t *image_dev, int32_t width, int32_t height, const chip_orb_params &d,
                bool describe, uint8_t *desc_dev, float2 *kp_dev, size_t back);
int orb_finished(Ctx *c, bool describe, int32_t n_features, int32_t *total, int32_t level_counts[8]);
// The batched put's half of the same (chip_frame_put_orb_stereo_batch): the G <= kFramePutGroup left images of pairs that lie in device
// memory (pair f at pairs_dev + f * pair_stride), one launch per stage over all frames, descriptors and keypoints written straight into the
// rows of slot[f] of the frame store (desc_base / kp_base: slot 0).  The kept counts stay on the device, frame f's eight int32 at
// *out_dev + f * *out_stride; orb_batch_counts enqueues their one copy into pinned memory.  *launches grows by the launches made.
constexpr int kFramePutGroup = 16;
int orb_batch_enqueue(Ctx *c, hipStream_t s, const uint8_t *pairs_dev, size_t pair_stride, int32_t G, int32_t width, int32_t height,
                      const chip_orb_params &d, uint8_t *desc_base, float2 *kp_base, int32_t slot_kp, const int32_t *slot, int32_t *launches,
                      const uint8_t **out_dev, size_t *out_stride);
int orb_batch_counts(Ctx *c, hipStream_t s, int32_t G, const int32_t **counts);
// the scratch of a group of G frames, grown if it must (inside one pause); probe: allocates nothing and returns 1 if something would grow, else 0
int orb_batch_reserve(Ctx *c, int32_t G, int32_t width, int32_t height, const chip_orb_params &d, bool probe);
// the solvers on correspondence sets that already are in device memory (match.hip's sets): same kernels, same results as the
// host-pointer entries chip_pnp_ransac / chip_icp_ransac; the caller has validated the arguments and holds match_mu
int pnp_ransac_device(Ctx *c, const double *X_dev, const double *uv_dev, int32_t N, const chip_ransac_params *p, double *T_colmajor,
                      float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary);
int pnp_ransac_device_batch(Ctx *c, int32_t P, const double *const *X_dev, const double *const *uv_dev, const int32_t *N, const chip_ransac_params *p,
                            const uint64_t *seeds, double *T_colmajor, float *confidence, uint8_t *const *inlier_mask, chip_ransac_summary *summary);
int icp_ransac_device(Ctx *c, const double *A_dev, const double *B_dev, int32_t N, const chip_ransac_params *p, double *T_colmajor,
                      float *confidence, uint8_t *inlier_mask, chip_ransac_summary *summary);
// the enqueue half of chip_icp_ransac_matched_batch: R validated problems on device-resident sets, one pair of launches on the ICP
// stream; problem r is answer at[r] of the `total` that chip_icp_ransac_matched_batch_collect delivers.  The caller holds match_mu.
int icp_enqueue_device_batch(Ctx *c, int32_t R, const double *const *A_dev, const double *const *B_dev, const int32_t *N, const chip_ransac_params *p,
                             const uint64_t *seeds, int32_t total, const int32_t *at);
// before a match call rewrites the slabs: waits for the kernels of a pending matched ICP batch (which stays collectable).  match_mu held.
int icp_wait_matched(Ctx *c);
// chip_debug_ransac_record's ICP leg (icp.hip; the PnP leg lives with its state in pnp.hip): c is a plain ctx, every output may be null
int icp_debug_record(Ctx *c, int32_t problem, chip_debug_ransac_shape *shape, int32_t *valid, double *cost, int32_t *nin, double *T_colmajor,
                     unsigned long long *mask);

}  // namespace chip

struct chip_ctx : chip::Ctx {};
