"""The scan form matrix: every kernel form the scan dispatcher can choose (cerebro_amd/csrc/kernels.hip scan_select, chip_api.hip
scan_policy), each with the knobs and the kind of call that reach it and the form the case must be SEEN to run.  Plain data, shared by
tests/test_scan_plan.py (CPU: the planner must agree with every row, and must not be able to reach a form no row names) and
tests/test_scan_forms_gpu.py (device: every row against the oracle, chip.last_scan() against the row).

A form is the kernel instantiation plus the modes that change what its code does:
  rows(R, ntl, claimed, fused)   db_scan_topk_rows<T, NQ, R, NTL>, rows claimed or mapped statically, fused tick or lists
  one(U, NT, FULL)               db_scan_topk<T, NQ, U, FULL, NT, 1>; NT = 8 is the fp64-staged-query form (q64)
  wide(NG, FULL)                 db_scan_topk_wide<NQ, NG, FULL>
A query case runs nq = 1..4 (`form` holds for every nq unless `by_nq` says otherwise); a tick case runs the three queries of a tick.
`grid` x `block` is the launch at the case's full prefix with three queries on 256 compute units."""
from __future__ import annotations

N_CUS = 256
QUERY, TICK, SYNC = "query", "tick", "sync"      # chip_query_rows / chip_loop_tick_enqueue + _collect / chip_loop_tick
FORM_FIELDS = ("family", "U", "NT", "FULL", "NG", "R", "NTL", "claimed", "fused", "q64")


def rows(R, ntl=0, claimed=0, fused=0):
    return dict(family="rows", U=0, NT=0, FULL=0, NG=0, R=R, NTL=ntl, claimed=claimed, fused=fused, q64=0)


def one(U, NT, FULL=1):
    return dict(family="one_row", U=U, NT=NT, FULL=FULL, NG=0, R=1, NTL=0, claimed=0, fused=0, q64=1 if NT == 8 else 0)


def wide(NG, FULL):
    return dict(family="wide", U=0, NT=0, FULL=FULL, NG=NG, R=0, NTL=0, claimed=0, fused=0, q64=0)


class Case:
    def __init__(self, name, D, elem, env, call, form, grid, block, by_nq=None, n_rows=None):
        self.name, self.D, self.elem, self.env, self.call = name, D, elem, dict(env), call
        self.form, self.grid, self.block, self.by_nq = form, grid, block, dict(by_nq or {})
        self.n_rows = n_rows            # None: sized against the geometry (rows_for); a number: that many rows (the bench's shape)

    def nqs(self):
        return (1, 2, 3, 4) if self.call == QUERY else (3,)

    def form_for(self, nq):
        return self.by_nq.get(nq, self.form)

    def keys(self):
        """the forms this case names: (form fields..., elem, nq)"""
        return {form_key(self.form_for(nq), self.elem, nq) for nq in self.nqs()}

    def __repr__(self):
        return self.name


def form_key(form, elem, nq):
    return tuple(form[f] for f in FORM_FIELDS) + (elem, nq)


def rows_for(W, R):
    """rows of a case's DB: two full passes of every wave, a third one that ends in the middle of the grid, and a little"""
    return (2 * R + 1) * W + W // 2 + 37


def prefixes(W, R, wpb, N):
    """the prefixes a case scans, placed against the geometry: W waves, R rows per wave and pass, wpb waves per workgroup"""
    ks = {0, 1, 63, 64, 65, W - 1, W, W + 1, R * W - 1, R * W, R * W + 1, R * W + wpb - 1, 2 * R * W + 1,
          (2 * R + 1) * W - 1, (2 * R + 1) * W, (2 * R + 1) * W + 1, N - 50, N}
    for base in (R * W, N // (R * W) * (R * W)):      # the second pass, and the last pass of the whole DB:
        for j in range(1, R + 1):                     # it holds 1 .. R rows of about half of the waves, and j rows of exactly every wave
            ks.update((base + (j - 1) * W + W // 2 + 3, base + j * W - 1, base + j * W, base + j * W + 1))
    return sorted(k for k in ks if 0 <= k <= N)


NO_ROWS = {"CHIP_SCAN_ROWS": "-1"}
NTL = {"CHIP_SCAN_PLAIN_MIB": "0"}
LONG = {"CHIP_SCAN_OVERLAP_GIB": "0", "CHIP_TICK_COALESCE": "0"}      # every scan takes the long-scan path; pipelined ticks never park
UNFUSED = {"CHIP_TICK_FUSED": "0"}


def R_(n):
    return {"CHIP_SCAN_ROWS": str(n)}


def _c(name, D, elem, env, call, form, grid, block, **kw):
    return Case(name, D, elem, env, call, form, grid, block, **kw)


CASES = [
    # ---- the row-batched kernel, R = 1 (what every cache-sized prefix runs) ----
    _c("rows1-half-query", 1024, 4, {}, QUERY, rows(1), 256, 512),
    _c("rows1-half-sync", 1024, 4, {}, SYNC, rows(1, fused=1), 256, 512),
    _c("rows1-half-tick", 2048, 4, {}, TICK, rows(1, fused=1), 256, 512),
    _c("rows1-half-sync-unfused", 1024, 4, UNFUSED, SYNC, rows(1), 256, 512),
    _c("rows1-half-tick-unfused", 1024, 4, UNFUSED, TICK, rows(1), 256, 512),
    _c("rows1-full-static-query", 1024, 4, {"CHIP_SCAN_SHORT_BPC": "0", "CHIP_SCAN_CLAIM": "0"}, QUERY, rows(1), 512, 512),
    _c("rows1-full-static-sync", 2048, 4, {"CHIP_SCAN_SHORT_BPC": "0", "CHIP_SCAN_CLAIM": "0"}, SYNC, rows(1, fused=1), 512, 512),
    _c("rows1-full-claimed-query", 1024, 4, {"CHIP_SCAN_SHORT_BPC": "0"}, QUERY, rows(1, claimed=1), 512, 512),
    _c("rows1-halfmib0-claimed-sync", 2048, 4, {"CHIP_SCAN_HALF_MIB": "0"}, SYNC, rows(1, claimed=1, fused=1), 512, 512),
    _c("rows1-halfmib0-claimed-tick-unfused", 1024, 4, dict(UNFUSED, CHIP_SCAN_HALF_MIB="0"), TICK, rows(1, claimed=1), 512, 512),
    _c("rows1-half-claimed-query", 2048, 4, {"CHIP_SCAN_CLAIM": "1"}, QUERY, rows(1, claimed=1), 256, 512),
    _c("rows1-half-claimed-tick", 1024, 4, {"CHIP_SCAN_CLAIM": "1"}, TICK, rows(1, claimed=1, fused=1), 256, 512),
    _c("rows1-4096-query", 4096, 4, {}, QUERY, rows(1, claimed=1), 512, 512, n_rows=14_500),    # 237 MB: beyond half occupancy
    _c("rows1-ntl-sync", 1024, 4, NTL, SYNC, rows(1, ntl=1, fused=1), 256, 512),
    _c("rows1-ntl-claimed-sync", 2048, 4, dict(NTL, CHIP_SCAN_HALF_MIB="0"), SYNC, rows(1, ntl=1, claimed=1, fused=1), 512, 512),
    _c("rows1-ntl-sync-unfused", 1024, 4, dict(NTL, **UNFUSED), SYNC, rows(1, ntl=1), 256, 512),
    _c("rows1-ntl-claimed-sync-unfused", 1024, 4, dict(NTL, CHIP_SCAN_HALF_MIB="0", **UNFUSED), SYNC, rows(1, ntl=1, claimed=1), 512, 512),
    _c("rows1-ntl-query", 1024, 4, dict(NTL, **R_(1)), QUERY, rows(1, ntl=1), 256, 512),
    _c("rows1-ntl-claimed-query", 2048, 4, dict(NTL, CHIP_SCAN_CLAIM="1", **R_(1)), QUERY, rows(1, ntl=1, claimed=1), 256, 512),
    # ---- R = 2 on the reference's default model at its own capacity: the bench's shape, default knobs ----
    _c("rows2-8192x29k-query", 8192, 4, {}, QUERY, rows(2, ntl=1), 256, 1024, by_nq={4: one(4, 6)}, n_rows=29_000),
    _c("rows2-8192x29k-sync", 8192, 4, {}, SYNC, rows(2, ntl=1, fused=1), 256, 1024, n_rows=29_000),
    _c("rows2-8192x29k-tick", 8192, 4, {}, TICK, rows(2, ntl=1, fused=1), 256, 1024, n_rows=29_000),
    _c("rows2-8192-ntl-tick-unfused", 8192, 4, dict(NTL, **UNFUSED), TICK, rows(2, ntl=1), 256, 1024),
    _c("rows2-8192-ntl-sync", 8192, 4, NTL, SYNC, rows(2, ntl=1, fused=1), 256, 1024),
    # ---- R = 2, 3 forced: temporal and non-temporal loads, 1 / 2 / 4 batches per row ----
    _c("rows2-t-1batch-query", 1024, 4, R_(2), QUERY, rows(2), 256, 512, by_nq={4: rows(1)}),
    _c("rows3-t-1batch-query", 1024, 4, R_(3), QUERY, rows(3), 256, 512, by_nq={4: rows(1)}),
    _c("rows2-ntl-2batch-query", 2048, 4, dict(NTL, **R_(2)), QUERY, rows(2, ntl=1), 256, 512, by_nq={4: rows(1, ntl=1)}),
    _c("rows3-ntl-2batch-query", 2048, 4, dict(NTL, **R_(3)), QUERY, rows(3, ntl=1), 256, 512, by_nq={4: rows(1, ntl=1)}),
    _c("rows2-t-4batch-sync", 4096, 4, R_(2), SYNC, rows(2, fused=1), 256, 512),
    _c("rows3-ntl-4batch-tick", 4096, 4, dict(NTL, **R_(3)), TICK, rows(3, ntl=1, fused=1), 512, 512),
    _c("rows3-t-2batch-sync", 2048, 4, R_(3), SYNC, rows(3, fused=1), 256, 512),
    _c("rows2-ntl-1batch-tick", 1024, 4, dict(NTL, **R_(2)), TICK, rows(2, ntl=1, fused=1), 256, 512),
    _c("rows2-t-tick-unfused", 1024, 4, dict(UNFUSED, **R_(2)), TICK, rows(2), 256, 512),
    _c("rows3-t-sync-unfused", 1024, 4, dict(UNFUSED, **R_(3)), SYNC, rows(3), 256, 512),
    _c("rows3-ntl-sync-unfused", 1024, 4, dict(NTL, **UNFUSED, **R_(3)), SYNC, rows(3, ntl=1), 256, 512),
    # ---- double rows in the row-batched kernel ----
    _c("f64-rows1-query", 512, 8, {}, QUERY, rows(1), 256, 512),
    _c("f64-rows1-sync", 512, 8, {}, SYNC, rows(1, fused=1), 256, 512),
    _c("f64-rows1-claimed-tick", 512, 8, {"CHIP_SCAN_HALF_MIB": "0"}, TICK, rows(1, claimed=1, fused=1), 512, 512),
    _c("f64-rows1-claimed-query", 512, 8, {"CHIP_SCAN_CLAIM": "1"}, QUERY, rows(1, claimed=1), 256, 512),
    _c("f64-rows1-tick-unfused", 512, 8, UNFUSED, TICK, rows(1), 256, 512),
    _c("f64-rows1-claimed-sync-unfused", 512, 8, dict(UNFUSED, CHIP_SCAN_CLAIM="1"), SYNC, rows(1, claimed=1), 256, 512),
    _c("f64-rows2-query", 512, 8, R_(2), QUERY, rows(2), 256, 512, by_nq={4: rows(1)}),
    _c("f64-rows3-query", 512, 8, R_(3), QUERY, rows(3), 256, 512, by_nq={4: rows(1)}),
    _c("f64-rows3-ntl-sync", 512, 8, dict(NTL, **R_(3)), SYNC, rows(3, ntl=1, fused=1), 256, 512),
    _c("f64-rows1-ntl-sync", 512, 8, NTL, SYNC, rows(1, ntl=1, fused=1), 256, 512),
    _c("f64-rows1-ntl-claimed-sync", 512, 8, dict(NTL, CHIP_SCAN_HALF_MIB="0"), SYNC, rows(1, ntl=1, claimed=1, fused=1), 512, 512),
    _c("f64-rows1-ntl-query", 512, 8, dict(NTL, **R_(1)), QUERY, rows(1, ntl=1), 256, 512),
    _c("f64-rows1-ntl-claimed-query", 512, 8, dict(NTL, CHIP_SCAN_CLAIM="1", **R_(1)), QUERY, rows(1, ntl=1, claimed=1), 256, 512),
    _c("f64-rows3-tick", 512, 8, R_(3), TICK, rows(3, fused=1), 256, 512),
    _c("f64-rows3-ntl-query", 512, 8, dict(NTL, **R_(3)), QUERY, rows(3, ntl=1), 256, 512, by_nq={4: rows(1, ntl=1)}),
    _c("f64-rows1-4096-query", 4096, 8, {}, QUERY, rows(1), 256, 1024, by_nq={1: rows(1, claimed=1), 2: rows(1, claimed=1)}),
    _c("f64-rows2-4096-sync", 4096, 8, R_(2), SYNC, rows(2, fused=1), 256, 1024),
    _c("f64-rows2-4096-ntl-tick", 4096, 8, NTL, TICK, rows(2, ntl=1, fused=1), 256, 1024),
    _c("f64-rows2-4096-ntl-query", 4096, 8, NTL, QUERY, rows(2, ntl=1), 256, 1024, by_nq={4: one(4, 6)}),
    # ---- the one-row kernel: asm-issued loads (whole 4 KiB / 2 KiB batches) and the builtin path ----
    _c("one-u4-query", 1024, 4, NO_ROWS, QUERY, one(4, 6), 256, 512),
    _c("one-u4-tick", 2048, 4, NO_ROWS, TICK, one(4, 6), 256, 512),
    _c("one-u2-query", 1536, 4, {}, QUERY, one(2, 6), 256, 512),
    _c("one-u2-sync", 1536, 4, {}, SYNC, one(2, 6), 256, 512),
    _c("one-builtin-partial-query", 1000, 4, {}, QUERY, one(8, 1, FULL=0), 256, 512),
    _c("one-builtin-partial-4100-query", 4100, 4, {}, QUERY, one(8, 1, FULL=0), 256, 512),
    _c("one-builtin-full-query", 4096, 4, {"CHIP_SCAN_VARIANT": "1"}, QUERY, one(8, 1), 256, 512),
    _c("one-builtin-full-tick", 4096, 4, {"CHIP_SCAN_VARIANT": "1"}, TICK, one(8, 1), 256, 512),
    _c("f64-one-u4-query", 512, 8, NO_ROWS, QUERY, one(4, 6), 256, 512),
    _c("f64-one-u2-query", 768, 8, {}, QUERY, one(2, 6), 256, 512),
    _c("f64-one-builtin-partial-query", 1000, 8, {}, QUERY, one(8, 1, FULL=0), 256, 512),
    _c("f64-one-builtin-full-query", 1024, 8, {"CHIP_SCAN_VARIANT": "1"}, QUERY, one(8, 1), 256, 512),
    # ---- fp64-staged queries (long scans of float rows) ----
    _c("q64-query", 1024, 4, LONG, QUERY, one(4, 8), 256, 512),
    _c("q64-tick", 1024, 4, LONG, TICK, one(4, 8), 256, 512),
    _c("q64-4096-sync", 4096, 4, LONG, SYNC, one(4, 8), 256, 1024),
    # ---- the reserved grid of a sharded / group ctx ----
    _c("reserve-rows-half-query", 1024, 4, {"CHIP_SCAN_RESERVE": "4"}, QUERY, rows(1), 252, 512),
    _c("reserve-rows-full-sync", 1024, 4, {"CHIP_SCAN_RESERVE": "4", "CHIP_SCAN_SHORT_BPC": "0"}, SYNC, rows(1, claimed=1, fused=1), 508, 512),
    _c("reserve-one-query", 1024, 4, dict(NO_ROWS, CHIP_SCAN_RESERVE="4", CHIP_SCAN_SHORT_BPC="0"), QUERY, one(4, 6), 508, 512),
    # ---- double rows wider than the LDS holds the queries of: some are read in place ----
    _c("wide-8192", 8192, 8, {}, QUERY, wide(1, 1), 256, 1024, by_nq={1: rows(2, ntl=1), 2: rows(2, ntl=1), 4: wide(2, 1)}),
    _c("wide-8200", 8200, 8, {}, QUERY, wide(1, 0), 256, 1024, by_nq={1: one(8, 1, FULL=0), 2: one(8, 1, FULL=0), 4: wide(2, 0)}),
    _c("wide-6144", 6144, 8, {}, QUERY, rows(1), 256, 1024, by_nq={1: rows(1, claimed=1), 4: wide(1, 1)}),
    _c("wide-6824", 6824, 8, {}, QUERY, one(8, 1, FULL=0), 256, 1024, by_nq={4: wide(1, 0)}),
]
assert len({c.name for c in CASES}) == len(CASES)

# the documented knobs (README), as the CPU sweep sets them one at a time
KNOB_SETTINGS = [{}] + [{"CHIP_SCAN_ROWS": v} for v in ("-1", "1", "2", "3")] + [{"CHIP_SCAN_CLAIM": v} for v in ("0", "1")] + [
    {"CHIP_SCAN_SHORT_BPC": "0"}, {"CHIP_SCAN_PLAIN_MIB": "0"}, {"CHIP_SCAN_HALF_MIB": "0"}, {"CHIP_SCAN_SYNC_PLAIN_MIB": "0"},
    {"CHIP_SCAN_OVERLAP_GIB": "0"}, {"CHIP_SCAN_RESERVE": "4"}, {"CHIP_SCAN_VARIANT": "1"}, {"CHIP_SCAN_VARIANT": "7"}, {"CHIP_TICK_FUSED": "0"}]
SCAN_ENV = sorted({k for c in CASES for k in c.env} | {k for s in KNOB_SETTINGS for k in s} |
                  {"CHIP_SCAN_BLOCK", "CHIP_SCAN_BPC", "CHIP_SCAN_STREAMS", "CHIP_TICK_SAME_STREAM"})

CALL_CODE = {QUERY: 0, TICK: 1, SYNC: 2}         # CHIP_SCAN_CALL_*


def case_geometry(case, plan):
    """(N, W, R, wpb) of a case: the rows of its DB and the geometry of the launch over all of them (three queries), from
    plan(D, elem, nq, K, n_rows, call) -> dict, which is capi.scan_plan under the case's knobs."""
    n = case.n_rows or 10_000
    for _ in range(4):
        p = plan(case.D, case.elem, 3, 8, n, CALL_CODE[case.call])
        W, R = p["grid"] * p["block"] // 64, max(p["R"], 1)
        if p["family"] == "wide":
            R = 1
        want = case.n_rows or rows_for(W, R)
        if want == n:
            return n, W, R, p["block"] // 64
        n = want
    raise AssertionError(f"{case.name}: the geometry does not settle")
