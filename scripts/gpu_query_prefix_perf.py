#!/usr/bin/env python3
"""Measurements of the prefix-per-query mode (profiles/query_prefix.md).  Medians of 30, the variants alternating in one process; the
driver runs every step as a child of its own under `timeout` and stops at the first that fails.

    python scripts/gpu_query_prefix_perf.py                       # every step
    python scripts/gpu_query_prefix_perf.py --step join --rows 29000
    python scripts/gpu_query_prefix_perf.py --step parent --parent-lib /path/to/the/parent/commit's/libcerebro_hip.so

Steps
  join    4096-D x `rows` unit rows, causal self-join of all rows at lag 50, topk 5:
            (a)  Chip.self_join: one chip_query_batch_rows_f32;
            (a') the same prefixes with the rows handed over as host vectors (chip_query_batch_prefix_f32): (a') - (a) is what the gather
                 kernel saves against memset + H2D + transpose_queries (and the host's copy of the vectors into sorted order);
            (b)  the same groups of 4096 queries through chip_query_batch_f32 at k = max of the group: the rectangle plus uploads;
            (c)  the chip_query_rows loop at four rows per call, timed on 200 calls spread evenly over the range and scaled.
  parent  chip_query_batch_f32 at Q = 256 x 1M rows on this tree and on another build of the library (the parent commit's), both loaded
          into this process, calls alternating."""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
D, LAG, TOPK, REPS, GROUP = 4096, 50, 5, 30, 4096


def ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def step_join(rows_n):
    from cerebro_amd import capi
    with capi.Chip(D) as chip:
        chip.append_synthetic(rows_n, 7, unit=True)
        rows = np.arange(rows_n, dtype=np.int64)
        k = np.maximum(0, rows - LAG)
        plan = capi.query_prefix_plan(k, 4, TOPK)
        vec = chip.read_rows(rows)                                             # the host vectors of (a') and (b)
        groups = [(g, min(g + GROUP, rows_n)) for g in range(0, rows_n, GROUP)]

        def a():
            chip.self_join(0, rows_n, LAG, TOPK)

        def a_host():
            chip.query_batch_prefix(k, vec, TOPK)

        def b():
            for lo, hi in groups:
                chip.query_batch(int(k[hi - 1]), vec[lo:hi], TOPK)

        for f in (a, a_host, b):                                               # warm-up: buffers allocated, code objects loaded
            f()
        last = chip.debug_query_prefix_last()
        t = {"a": [], "a_host": [], "b": []}
        for _ in range(REPS):
            t["a"].append(ms(a))
            t["a_host"].append(ms(a_host))
            t["b"].append(ms(b))
        calls = np.linspace(4, rows_n - 4, 200).astype(np.int64)               # (c): 200 of the rows_n / 4 calls
        chip.query_rows(int(calls[100]), calls[100] + np.arange(4), TOPK)
        tc = [ms(lambda r=r: chip.query_rows(int(max(0, r - LAG)), r + np.arange(4), TOPK)) for r in calls]
        out = {"step": "join", "rows": rows_n, "D": D, "topk": TOPK, "lag": LAG, "units": plan["units"], "units_rect": plan["units_rect"],
               "units_over_rect": round(plan["units"] / plan["units_rect"], 4), "last": last,
               "a_rows_call": summary(t["a"]), "a_host_vectors": summary(t["a_host"]), "b_rectangle_groups": summary(t["b"]),
               "a_over_b": round(statistics.median(t["a"]) / statistics.median(t["b"]), 4),
               "gather_saves_ms": round(statistics.median(t["a_host"]) - statistics.median(t["a"]), 3),
               "c_query_rows_loop_scaled_ms": round(statistics.mean(tc) * rows_n / 4, 1), "c_calls_timed": len(tc)}
        print(json.dumps(out), flush=True)


def raw_ctx(lib, rows_n):
    lib.chip_create.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.chip_db_append_synthetic_unit.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.chip_query_batch_f32.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.chip_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert lib.chip_create(C.byref(h), D, 0, 0, 0, 1) == 0
    assert lib.chip_db_append_synthetic_unit(h, rows_n, 7, None, None, None, 0) == 0
    return h


def step_parent(parent_lib, rows_n=1_000_000, Q=256):
    libs = {"this_tree": C.CDLL(str(ROOT / "cerebro_amd" / "lib" / "libcerebro_hip.so")), "parent": C.CDLL(str(parent_lib))}
    assert not hasattr(libs["parent"], "chip_query_batch_rows_f32"), "the other library is not the parent commit's"
    q = np.random.default_rng(3).standard_normal((Q, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sc, ix = np.empty((Q, TOPK), dtype=np.float32), np.empty((Q, TOPK), dtype=np.int64)
    ctx = {n: raw_ctx(lib, rows_n) for n, lib in libs.items()}
    res = {}

    def call(n):
        assert libs[n].chip_query_batch_f32(ctx[n], rows_n, q.ctypes.data, Q, TOPK, sc.ctypes.data, ix.ctypes.data) == 0

    for n in libs:
        call(n)
        res[n] = (sc.copy(), ix.copy())
    same = bool(np.array_equal(res["this_tree"][1], res["parent"][1]) and res["this_tree"][0].tobytes() == res["parent"][0].tobytes())
    t = {n: [] for n in libs}
    for _ in range(REPS):
        for n in libs:
            t[n].append(ms(lambda n=n: call(n)))
    for n, lib in libs.items():
        lib.chip_destroy(ctx[n])
    print(json.dumps({"step": "parent", "rows": rows_n, "Q": Q, "D": D, "same_bits": same, **{n: summary(v) for n, v in t.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["join", "parent"])
    ap.add_argument("--rows", type=int, default=29000)
    ap.add_argument("--parent-lib")
    ap.add_argument("--step-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.step == "join":
        return step_join(a.rows)
    if a.step == "parent":
        return step_parent(a.parent_lib)
    steps = [["--step", "join", "--rows", "29000"], ["--step", "join", "--rows", "100000"]]
    if a.parent_lib:
        steps.append(["--step", "parent", "--parent-lib", a.parent_lib])
    for s in steps:
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__] + s)
        if r.returncode != 0:
            print(f"step {s} ended with status {r.returncode}: stopping", flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
