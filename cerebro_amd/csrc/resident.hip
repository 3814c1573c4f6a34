// resident.hip -- the resident scan instance (opt-in: CHIP_TICK_RESIDENT=1; kernels.hip db_scan_resident, chip_internal.h ResidentCmd
// and struct Resident).  Host code only: set-up, the command line protocol with the kernel, retire / pause, the collect of a command.  Lock
// order: query_mu or append_mu first, Resident::mu last.
#include "chip_internal.h"
#include <chrono>
#include <cstdio>
#include <cstring>

namespace chip {

void resident_read_knobs(Ctx *c)
{
    // opt-in: synchronous ticks over cache-sized prefixes go to a scan instance that stays on the chip (chip_internal.h ResidentCmd)
    c->res.enabled = env_int("CHIP_TICK_RESIDENT", 0) != 0 && (scan_forms_built() & CHIP_SCAN_FORM_ROWS) != 0;
    c->res.max_bytes = (double)env_int("CHIP_RESIDENT_MAX_MIB", 512) * 1024 * 1024;   // 32k rows of 4096 floats: the reference's capacity is 29k
    c->res.lease_ms = env_int("CHIP_RESIDENT_LEASE_MS", 250);
#ifdef CHIP_TEST_HOOKS
    c->res.test_skip_master = env_int("CHIP_TEST_RESIDENT_SKIP_MASTER", 0);
#endif
    if (c->res.lease_ms < 1) c->res.lease_ms = 1;
}

static inline void host_store_fence()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_sfence();                        // drains the write-combining buffers of the BAR mapping
#else
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}
// (CHIP_TICK_RESIDENT=1; kernels.hip db_scan_resident, chip_internal.h ResidentCmd).  Host side: one command at a time; the line is
// written head first, tail last (x86 stores stay in order; the fences keep the compiler from moving them).
static void resident_write_line(Ctx *c, const ResidentCmd &cmd)
{
    if (c->res.direct) {
        // every workgroup's own line, through the write-combining BAR mapping: eight 8-byte stores per line in address order (head first,
        // tail last; a full 64-byte line leaves the CPU as one PCIe write), one fence for all of them
        ResidentCmd t = cmd;
        t.tail = t.head;
        uint64_t w[8];
        std::memcpy(w, &t, 64);
        volatile uint64_t *d = reinterpret_cast<volatile uint64_t *>(c->res.cmd_host);
        int first = 0;
#ifdef CHIP_TEST_HOOKS   // test build only (make testlibs -> cerebro_amd/lib/hooks/): the product library has no fault injection
        // CHIP_TEST_RESIDENT_SKIP_MASTER=k: the k-th command never reaches workgroup 0's line -- the other workgroups run it, workgroup 0
        // leaves at its lease without it: exactly what a command posted in the moment the lease runs out can look like (tests drive
        // resident_collect's recovery with it)
        if (cmd.n_rows >= 0 && c->res.test_skip_master > 0 && c->res.ticks + 1 == c->res.test_skip_master && !c->res.test_skipped) {
            first = 1;
            c->res.test_skipped = true;
        }
#endif
        for (int j = first; j < c->res.grid; j++)
            for (int i = 0; i < 8; i++) d[j * 8 + i] = w[i];
        host_store_fence();
        return;
    }
    ResidentCmd *d = c->res.cmd_host;
    __atomic_store_n(&d->head, cmd.head, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_RELEASE);
    d->locality = cmd.locality;
    d->n_rows = cmd.n_rows;
    d->tick_l = cmd.tick_l;
    d->thresh = cmd.thresh;
    d->result = cmd.result;
    d->seq_ptr = cmd.seq_ptr;
    d->seq_val = cmd.seq_val;
    d->dyn_claim = cmd.dyn_claim;
    __atomic_store_n(&d->tail, cmd.head, __ATOMIC_RELEASE);
    // a line in device memory is written through the write-combining BAR mapping: push it out (one full 64-byte line = one PCIe write)
    if (c->res.cmd_in_vram) host_store_fence();
}

static uint32_t resident_next_number(Ctx *c)
{
    uint32_t n = c->res.cmd_no + 1;
    if (n == 0u || n == kResidentLeave) n = 1u;
    c->res.cmd_no = n;
    return n;
}

void resident_destroy(Ctx *c)
{
    if (c->res.stream) { (void)hipStreamDestroy(c->res.stream); c->res.stream = nullptr; }
    c->res.pinned.release(); c->res.cmd_vram.release(); c->res.cmd_dev.release(); c->res.partial.release(); c->res.ticket.release();
    c->res.cmd_host = nullptr; c->res.cmd_hostdev = nullptr; c->res.exit_host = nullptr; c->res.exit_hostdev = nullptr;
    c->res.cmd_in_vram = false; c->res.direct = false;
    c->res.ready = false;
}

// does a pattern the CPU stores through the BAR mapping of `v` (64 bytes of device memory) read back through a copy?  Leaves zeros.
static bool bar_write_probe(void *v)
{
    if (hipMemset(v, 0, 64) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    uint32_t back[16] = {0};
    volatile uint32_t *w = static_cast<volatile uint32_t *>(v);
    for (int i = 0; i < 16; i++) w[i] = 0x5eed0000u + (uint32_t)i;
    host_store_fence();
    bool ok = hipMemcpy(back, v, 64, hipMemcpyDeviceToHost) == hipSuccess;
    for (int i = 0; ok && i < 16; i++) ok = back[i] == 0x5eed0000u + (uint32_t)i;
    for (int i = 0; i < 16; i++) w[i] = 0u;
    host_store_fence();
    return ok;
}

// One workgroup per CU, so that the ctx's other kernels (append, PnP, ICP) still find registers and LDS next to the instance.  That
// shape is what a launch gives a cache-sized prefix anyway, and a synchronous tick loses nothing with it up to the reference's own
// capacity (29k rows: 93.9-94.7 us launched with one workgroup per CU, 93.8-94.1 with two; profiles/r05_resident.md).
static int resident_grid(const Ctx *c)
{
    const int grid = c->n_cus * (c->scan_short_bpc > 0 ? c->scan_short_bpc : 1);
    return grid < c->max_grid ? grid : c->max_grid;
}

static int resident_alloc_body(Ctx *c)
{
    // A stream of the HIGHEST priority: the runtime multiplexes streams onto a few hardware queues per priority level, and a packet
    // behind the resident kernel in its queue would wait for the instance to leave (measured: a tick stream that shared the queue
    // stalled for the whole lease).  The ctx's other streams are of the default priority, so this one gets a queue to itself.
    int pr_lo = 0, pr_hi = 0;
    CHIP_HIP(c, hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi));
    CHIP_HIP(c, hipStreamCreateWithPriority(&c->res.stream, hipStreamNonBlocking, pr_hi));
    // (alloc, not reserve, throughout: Resident::mu is held and a pause would take it again)
    int rc = c->res.pinned.alloc(c, 128);   // the command line + the line of the exit word
    if (rc != CHIP_OK) return rc;
    char *h = c->res.pinned.host(), *hd = c->res.pinned.dev();
    std::memset(h, 0, 128);
    c->res.cmd_host = reinterpret_cast<ResidentCmd *>(h);
    c->res.exit_host = reinterpret_cast<unsigned long long *>(h + 64);
    c->res.cmd_hostdev = reinterpret_cast<uint32_t *>(hd);
    c->res.exit_hostdev = reinterpret_cast<unsigned long long *>(hd + 64);
    // Where the command line lives.  With a large PCIe BAR the host can store straight into device memory, and a posted write that the
    // device then finds locally beats a line the device has to fetch over PCIe (ping-pong with one polling wave: 1.89 us against 2.52,
    // scripts/probes/bar_pingpong.hip).  Used when the device says so AND a pattern written that way into THE buffer itself reads back
    // through a copy (probing a throw-away allocation says nothing about this one); CHIP_RESIDENT_BAR=0 keeps the line in
    // pinned host memory.
    // CHIP_RESIDENT_BAR=2 (the default) goes one step further: the host writes EVERY workgroup's line that way (16 KiB per command,
    // 0.6 us of host time) and nobody relays: 10k rows 35.9-36.4 -> 34.7-35.0 us.  1: only workgroup 0's line, relayed on the device.
    c->res.grid = resident_grid(c);
    rc = c->res.cmd_dev.alloc(c, (size_t)c->max_grid * 16);
    if (rc != CHIP_OK) return rc;
    CHIP_HIP(c, hipMemset(c->res.cmd_dev, 0, (size_t)c->max_grid * 64));
    const int bar_mode = env_int("CHIP_RESIDENT_BAR", 2);
    int large_bar = 0;
    if (bar_mode != 0 && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, c->device) == hipSuccess && large_bar) {
        if (bar_mode == 2) {
            // the workgroups' lines themselves are the host's target (line 0 is workgroup 0's): probe the first and the last line of them
            if (bar_write_probe(c->res.cmd_dev.get()) && bar_write_probe(c->res.cmd_dev + (size_t)(c->max_grid - 1) * 16)) {
                c->res.cmd_in_vram = true;
                c->res.direct = true;
                c->res.cmd_host = reinterpret_cast<ResidentCmd *>(c->res.cmd_dev.get());
                c->res.cmd_hostdev = c->res.cmd_dev;
            }
        }
        if (!c->res.direct) {                   // mode 1, or mode 2 whose lines are not host-writable: one line of its own, relayed on the device
            if (c->res.cmd_vram.alloc(c, 64) == CHIP_OK) {
                if (bar_write_probe(c->res.cmd_vram.get())) {
                    c->res.cmd_in_vram = true;
                    c->res.cmd_host = reinterpret_cast<ResidentCmd *>(c->res.cmd_vram.get());
                    c->res.cmd_hostdev = reinterpret_cast<uint32_t *>(c->res.cmd_vram.get());
                } else {
                    c->res.cmd_vram.release();
                }
            }
        }
    }
    rc = c->res.partial.alloc(c, (size_t)c->max_grid * CHIP_MAX_NQ * CHIP_MAX_TOPK);
    if (rc == CHIP_OK) rc = c->res.ticket.alloc(c, 16);
    return rc;
}

// Resident::mu held.  Either everything exists afterwards (ready, published last) or nothing does and the mode is off for this ctx: the
// caller falls back to the launched tick (a half-built state must not be entered by the next tick).
static int resident_alloc(Ctx *c)
{
    if (c->res.ready) return CHIP_OK;
    const int rc = resident_alloc_body(c);
    if (rc != CHIP_OK) {
        resident_destroy(c);
        c->res.enabled = false;
        std::fprintf(stderr, "[cerebro_hip] resident scan instance: allocation failed (%s) -- this ctx launches its ticks\n", chip_strerror(rc));
        return CHIP_ERR_UNSUPPORTED;
    }
    c->res.ready = true;
    return CHIP_OK;
}

// A new instance behind whatever the stream still holds (the previous one on its way out).  Resident::mu held.
static int resident_launch(Ctx *c)
{
    ResidentArgs ra;
    ScanArgs &a = ra.base;
    scan_args_db(c, &a);
    a.n_rows = 0;
    a.K = 1;
    for (int i = 0; i < CHIP_MAX_NQ; i++) a.q[i] = nullptr;
    a.idx_mul = 1;
    a.idx_add = 0;
    a.partial = c->res.partial;
    a.rows_form = 1;
    a.plain_loads = 1;
    a.fused_ticket = c->res.ticket;
    a.stamps = c->stamps_dev;            // tuning only (CHIP_SCAN_STAMPS=1)
    ra.cmd_host = c->res.cmd_hostdev;
    ra.cmd_dev = c->res.cmd_dev;
    ra.exit_host = c->res.exit_hostdev;
    ra.instance = ++c->res.instance;
    ra.lease_ticks = (unsigned long long)c->res.lease_ms * 100000ull;   // s_memrealtime: 100 MHz
    ra.done = c->res.done;
    ra.direct = c->res.direct ? 1u : 0u;
    // the workgroups' lines still hold what the previous instance was told last (its leave mark included), the ticket whatever it left.
    // (direct mode: the lines are the host's to write -- the caller has posted the command the new instance is to find there)
    if (!c->res.direct) CHIP_HIP(c, hipMemsetAsync(c->res.cmd_dev, 0, (size_t)c->max_grid * 64, c->res.stream));
    CHIP_HIP(c, hipMemsetAsync(c->res.ticket, 0, 64, c->res.stream));
    int rc = launch_resident(c, c->res.stream, ra, c->res.grid);
    if (rc != CHIP_OK) return rc;
    c->res.alive = true;
    c->res.launches++;
    return CHIP_OK;
}

static bool resident_has_left(const Ctx *c)
{
    return __atomic_load_n(c->res.exit_host, __ATOMIC_ACQUIRE) == c->res.instance;
}

static void resident_stop_locked(Ctx *c)
{
    if (!c->res.ready || !c->res.alive) return;
    if (c->res.busy && c->res.slot) {   // a command is still running: let it finish (its collector only reads the completion word)
        const volatile unsigned long long *w = c->res.slot->seq_host;
        for (long spin = 0; spin < (1L << 28) && __atomic_load_n(w, __ATOMIC_ACQUIRE) != c->res.slot->seq_want && !resident_has_left(c); spin++) {}
    }
    if (!resident_has_left(c)) {
        ResidentCmd cmd{};
        cmd.head = resident_next_number(c);
        cmd.n_rows = -1;
        resident_write_line(c, cmd);
        c->res.done = cmd.head;          // nobody runs a leave command twice
    }
    (void)hipStreamSynchronize(c->res.stream);
    c->res.alive = false;
}

void resident_stop(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->res.mu);
    resident_stop_locked(c);
}

void resident_pause(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->res.mu);
    c->res.inhibit++;                    // from here on resident_tick_enqueue launches nothing (it checks under this mutex)
    resident_stop_locked(c);
}

void resident_resume(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->res.mu);
    if (c->res.inhibit > 0) c->res.inhibit--;
}

bool resident_eligible(Ctx *c, int64_t k)
{
    if (!c->res.enabled || c->nranks != 1 || c->xchg || c->parent || c->group || !c->own_query_stream || c->prof_on || !c->tick_fused ||
        !c->tick_poll || c->res.busy)
        return false;
    if ((double)k * c->D * c->elem > c->res.max_bytes) return false;
    return scan_rows_form(c, k, 3, resident_grid(c), false) == 1;
}

// The tick as a command to the resident instance (launched here if there is none, or if the last one has left).  query_mu held.
int resident_tick_enqueue(Ctx *c, int64_t k, int64_t l, const chip_dot_params *p, Slot &s)
{
    std::lock_guard<std::mutex> lk(c->res.mu);
    if (c->res.inhibit > 0) return kResidentPaused;   // a section that frees / allocates / rewrites the table is open: this tick is launched
    int rc = resident_alloc(c);
    if (rc != CHIP_OK) return rc;
    if (c->res.alive && resident_has_left(c)) c->res.alive = false;
    const bool launch = !c->res.alive;
    if (launch && c->res.direct) (void)hipStreamSynchronize(c->res.stream);   // the old instance is gone before its lines are rewritten
    s.seq_want = ++c->tick_seq;
    ResidentCmd cmd{};
    cmd.head = resident_next_number(c);
    cmd.locality = p->locality;
    cmd.n_rows = k;
    cmd.tick_l = l;
    cmd.thresh = p->thresh;
    cmd.result = (uint64_t)(uintptr_t)s.rec.dev();
    cmd.seq_ptr = (uint64_t)(uintptr_t)s.seq_dev;
    cmd.seq_val = s.seq_want;
    // rows claimed within the workgroup: beyond cache-sized prefixes, as for launches (29k rows: 92.3 -> 91.7 us; neutral at 10k)
    cmd.dyn_claim = (c->scan_claim == 1 || (c->scan_claim < 0 && (double)k * c->D * c->elem > c->scan_half_bytes)) ? 1u : 0u;
    c->res.pending = cmd;
    resident_write_line(c, cmd);           // (before the launch: an instance must never find the previous one's leave mark in its lines)
    if (launch) {
        rc = resident_launch(c);
        if (rc == CHIP_ERR_UNSUPPORTED) c->res.enabled = false;   // this ctx's shape has no resident form: every tick is launched from here on
        if (rc != CHIP_OK) return rc;
    }
    c->res.busy = true;
    c->res.slot = &s;
    c->res.ticks++;
    s.state = SlotState::Resident;
    s.wait_ev = nullptr;
    return CHIP_OK;
}

// Wait for the command's completion word.  An instance that left before it saw the command (its lease ran out just then) is replaced:
// the new one finds the line and runs it.
int resident_collect(Ctx *c, Slot &s)
{
    const volatile unsigned long long *w = s.seq_host;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned long spin = 1;; spin++) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == s.seq_want) break;
        if ((spin & 0x3ff) == 0) {
            std::lock_guard<std::mutex> lk(c->res.mu);
            if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == s.seq_want) break;
            if (!c->res.alive || resident_has_left(c)) {   // left by its lease, or retired by another thread (resident_stop) before it saw the line
                c->res.alive = false;
                if (c->res.direct) {
                    // some workgroups may have found the command in their lines while workgroup 0 was already leaving: send everybody
                    // home, wait until the instance is gone, then post the command again for a new one
                    ResidentCmd bye{};
                    bye.head = bye.tail = kResidentLeave;
                    bye.n_rows = -1;
                    resident_write_line(c, bye);
                    (void)hipStreamSynchronize(c->res.stream);
                    if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == s.seq_want) break;   // (it had run after all)
                }
                // (one line for all: it may hold the leave command of a resident_stop that gave up waiting for this one)
                resident_write_line(c, c->res.pending);
                const int rc = resident_launch(c);
                if (rc != CHIP_OK) { c->res.busy = false; c->res.slot = nullptr; return rc; }
            }
            if ((spin & 0xfffff) == 0 && std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0).count() > 30) {
                c->last_hip = hipErrorLaunchTimeOut;
                c->res.busy = false;          // whatever state the instance is in, its lease ends it; later ticks may try again
                c->res.slot = nullptr;
                return CHIP_ERR_HIP;
            }
        }
    }
    std::lock_guard<std::mutex> lk(c->res.mu);
    c->res.busy = false;
    c->res.slot = nullptr;
    c->res.done = c->res.cmd_no;
    return CHIP_OK;
}

void resident_wait_command(Ctx *c)
{
    std::lock_guard<std::mutex> lk(c->res.mu);
    if (c->res.busy && c->res.slot) {
        const volatile unsigned long long *w = c->res.slot->seq_host;
        for (long spin = 0; spin < (1L << 28) && __atomic_load_n(w, __ATOMIC_ACQUIRE) != c->res.slot->seq_want && c->res.alive && !resident_has_left(c); spin++) {}
    }
}

}  // namespace chip

extern "C" {

// Public form of the pause the library takes around its own frees / allocations (include/cerebro_hip.h): an integrator brackets
// device-wide operations of OTHER libraries in the same process with it.  No-ops (CHIP_OK) on ctxs without the resident mode.
int chip_resident_pause(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_OK;                 // group / sharded ctxs never run the resident instance
    (void)hipSetDevice(c->device);
    { std::lock_guard<std::mutex> qlk(c->query_mu); (void)chip::coalesce_flush(c); }
    chip::resident_pause(c);
    return CHIP_OK;
}

int chip_resident_resume(chip_ctx *c)
{
    if (!c) return CHIP_ERR_INVALID_ARG;
    if (c->group) return CHIP_OK;
    chip::resident_resume(c);
    return CHIP_OK;
}

// Tuning aid, not part of the ABI (no declaration in cerebro_hip.h): how many ticks the resident scan instance (CHIP_TICK_RESIDENT=1) has
// served and how many instances were launched for them -- tests use it to prove which path a tick took.
int chip_debug_resident_stats(chip_ctx *c, int64_t *ticks, int64_t *launches)
{
    if (!c || !ticks || !launches || c->group) return CHIP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->res.mu);
    *ticks = c->res.ticks;
    *launches = c->res.launches;
    return CHIP_OK;
}

// ... and where its command lines live: -1 no instance has been set up yet, 0 pinned host memory + relay, 1 workgroup 0's line in
// device memory behind the PCIe BAR + relay, 2 every workgroup's line written by the host through the BAR
int chip_debug_resident_mode(chip_ctx *c)
{
    if (!c || c->group) return -1;
    std::lock_guard<std::mutex> lk(c->res.mu);
    if (!c->res.stream) return -1;
    return c->res.direct ? 2 : (c->res.cmd_in_vram ? 1 : 0);
}

}  // extern "C"
