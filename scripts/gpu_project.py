#!/usr/bin/env python3
"""The descriptor projection at 32768 -> 4096 (ReljaNetVLAD's shape), measured in one visit -> profiles/project.md.

  python scripts/gpu_project.py [--reps 30] [--out profiles/project.md] [--no-trace] [--parent-tree DIR]

  1. host wall time, medians of --reps after warm-up, the variants ALTERNATING in one process, for a float and a double matrix:
     chip_db_append_projected_f32 of one row, chip_project, chip_db_append_f64 of one ready row -- and what the reference's server does
     today, np.matmul + np.linalg.norm on this host (numpy's summation order, NOT the definition's), with numpy's threads as they
     come and, in a child process, limited to one;
  2. the kernels project_rows and project_finish, and db_scan_topk over a 4096-D x 250k float DB of the same visit, from one
     `rocprofv3 --kernel-trace --stats` run of its own;
  3. with --parent-tree (a checkout of the parent commit with its library built): bench.py's headline and a 10k synchronous tick of
     this tree and of the parent, alternating: the guard that nothing that existed before has moved.
The code-object figures of the earlier kernels (this tree against the parent) are read as tests/test_codeobj_disparity.py: metadata does.
The part of an existing output file from "# What the figures say" on is kept."""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, os.environ.get("GPU_PROJECT_TREE") or str(ROOT))     # (the 10k-tick child of part 3 imports the tree it is told to)

import numpy as np  # noqa: E402

IN_DIM, D = 32768, 4096
WARMUP = 3
KEEP = "# What the figures say"
SCAN_ROWS = 250_000
HBM_PEAK = 8.0e12


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def data(dtype):
    rng = np.random.default_rng(32768)
    Mt = rng.standard_normal((D, IN_DIM), dtype=np.float32)
    if dtype == np.float64:
        Mt = Mt.astype(np.float64) + 1e-9 * rng.standard_normal((D, 1))      # genuinely double values, cheaply
    return Mt, rng.standard_normal(D), rng.standard_normal(IN_DIM, dtype=np.float32)


def numpy_reference(reps):
    """np.matmul(u, WPCA_M) + WPCA_b; u /= np.linalg.norm(u) for float32 and float64 operands -> {dtype name: median ms}"""
    out = {}
    for dtype in (np.float32, np.float64):
        Mt, b, x = data(dtype)
        M = np.ascontiguousarray(Mt.T)                                          # the server's layout: in_dim x D
        u, bb = x.astype(dtype), b.astype(dtype)

        def server():
            v = np.matmul(u, M) + bb
            return v / np.linalg.norm(v)
        for _ in range(WARMUP):
            server()
        out[np.dtype(dtype).name] = statistics.median(ms(server) for _ in range(reps))
    return out


def numpy_threads():
    try:
        from threadpoolctl import threadpool_info
        return ", ".join(f"{p.get('internal_api')} {p.get('num_threads')}" for p in threadpool_info()) or "unknown"
    except Exception:
        return f"unknown (no threadpoolctl; OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})"


def wall_times(reps):
    from cerebro_amd import capi
    rows = {}
    for dtype in (np.float32, np.float64):
        Mt, b, x = data(dtype)
        with capi.Chip(D) as chip:
            chip.project_set(Mt, b)
            z = chip.project(x)
            variants = {"chip_db_append_projected_f32, one row": lambda: chip.append_projected(x),
                        "chip_project, one row": lambda: chip.project(x),
                        "chip_db_append_f64, one ready row": lambda: chip.append_f64(z)}
            for _ in range(WARMUP):
                for fn in variants.values():
                    fn()
            t = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    t[k].append(ms(fn))
            rows[np.dtype(dtype).name] = {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}
    return rows


def trace_child():
    """what the traced run executes: projections with both matrix types, and scans of a 250k-row DB"""
    from cerebro_amd import capi
    for dtype in (np.float32, np.float64):
        Mt, b, x = data(dtype)
        with capi.Chip(D) as chip:
            chip.project_set(Mt, b)
            for _ in range(WARMUP + 30):
                chip.project(x)
    with capi.Chip(D, capacity_hint=SCAN_ROWS) as chip:
        chip.append_synthetic(SCAN_ROWS, 7, [], unit=True)
        for _ in range(WARMUP + 30):
            chip.query_rows(SCAN_ROWS - 60, [SCAN_ROWS - 1, SCAN_ROWS - 2, SCAN_ROWS - 3], 8)


def kernel_trace():
    """-> {kernel name: (calls, median ns)} from one rocprofv3 run of trace_child"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "project", "--", sys.executable, __file__, "--trace-child"],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        durations = {}
        for path in Path(tmp).rglob("*kernel_trace.csv"):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    durations.setdefault(row["Kernel_Name"], []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return {k: (len(v), statistics.median(v)) for k, v in durations.items()}


def tick10k_child():
    from cerebro_amd import capi
    with capi.Chip(4096, capacity_hint=10_000) as chip:
        chip.append_synthetic(10_000, 3, [], unit=True)
        p = capi.default_dot_params()
        p.min_new = -(1 << 30)
        for _ in range(200):
            chip.loop_tick(10_000, p)
        t = [ms(lambda: chip.loop_tick(10_000, p)) for _ in range(2000)]
    print(json.dumps({"tick10k_us": 1e3 * statistics.median(t)}))


def regression(parent: Path, rounds=6):
    """bench.py's headline line and the 10k synchronous tick, this tree and the parent alternating (and taking turns to go first)
    -> {tree: {figure: [values]}}"""
    out = {"this tree": {}, "parent": {}}
    for i in range(rounds):
        for name, root in (("this tree", ROOT), ("parent", parent))[::1 if i % 2 == 0 else -1]:
            r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5"], cwd=root, capture_output=True, text=True, timeout=900)
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            for k, v in line.items():
                if isinstance(v, (int, float)) and not isinstance(v, bool):
                    out[name].setdefault(k, []).append(v)
            r = subprocess.run([sys.executable, __file__, "--tick10k-child"], cwd=root, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, GPU_PROJECT_TREE=str(root)))
            out[name].setdefault("tick10k_us", []).append(json.loads(r.stdout.splitlines()[-1])["tick10k_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "project.md"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=6, help="runs per tree of part 3")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--numpy-child", action="store_true")
    ap.add_argument("--tick10k-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        return trace_child()
    if a.numpy_child:
        return print(json.dumps({"times": numpy_reference(a.reps), "threads": numpy_threads()}))
    if a.tick10k_child:
        return tick10k_child()

    from cerebro_amd import capi
    with capi.Chip(D) as chip:
        info = chip.info()
    L = [f"# The descriptor projection at {IN_DIM} -> {D}: measured figures", "",
         f"Written by `scripts/gpu_project.py --reps {a.reps}` on {info['arch']} ({info['n_cus']} CUs).  Host wall times are medians of {a.reps} calls",
         "after warm-up, the variants alternating in one process; every call ends in a stream synchronise.", ""]
    L += ["## 1. Host wall time per call (ms: median, min .. max)", "", "| matrix | call | median | min .. max |", "|---|---|---|---|"]
    for dt, rows in wall_times(a.reps).items():
        for k, (med, lo, hi) in rows.items():
            L.append(f"| {dt} | {k} | {med:.3f} | {lo:.3f} .. {hi:.3f} |")
    own = {"times": numpy_reference(a.reps), "threads": numpy_threads()}
    env1 = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run([sys.executable, __file__, "--numpy-child", "--reps", str(a.reps)], capture_output=True, text=True, env=env1, timeout=900)
    one = json.loads(r.stdout.splitlines()[-1]) if r.returncode == 0 else None
    L += ["", "What the reference's server does today on this host, `np.matmul(u, WPCA_M) + WPCA_b; u /= np.linalg.norm(u)`, both operands of the",
          "dtype named (numpy's BLAS order, not the definition's; the dtype of the reference's files is unknown here):", "",
          "| dtypes | numpy threads | median ms |", "|---|---|---|"]
    for dt, v in own["times"].items():
        L.append(f"| {dt} x {dt} | as they come: {own['threads']} | {v:.2f} |")
    for dt, v in (one["times"].items() if one else ()):
        L.append(f"| {dt} x {dt} | limited to one: {one['threads']} | {v:.2f} |")
    if not one:
        L.append("| | limited to one | not measured |")
    if not a.no_trace:
        k = kernel_trace()
        L += ["", "## 2. Kernel times (rocprofv3 --kernel-trace --stats, a run of its own: median ns over the calls)", "",
              "| kernel | calls | median us | bytes read | share of 8 TB/s |", "|---|---|---|---|---|"]
        for name, (calls, med) in sorted(k.items()):
            nbytes = None
            if "project_rows" in name:
                nbytes = IN_DIM * D * (8 if "<double" in name else 4)
            elif "db_scan_topk" in name:
                nbytes = (SCAN_ROWS - 60) * D * 4
            if "project_" in name or "db_scan_topk" in name:
                share = f"{nbytes / (med * 1e-9) / HBM_PEAK:.3f}" if nbytes else ""
                L.append(f"| `{name}` | {calls} | {med / 1e3:.1f} | {nbytes or ''} | {share} |")
    else:
        L += ["", "## 2. Kernel times", "", "not measured (--no-trace)"]
    if a.parent_tree:
        reg = regression(Path(a.parent_tree).resolve(), a.rounds)
        L += ["", "## 3. This tree against the parent commit, alternating in one visit", "", "| figure | this tree | parent |", "|---|---|---|"]
        for key in sorted(reg["this tree"]):
            if key in reg["parent"] and key not in ("n_gpus", "steps", "warmup"):
                L.append(f"| {key} | {', '.join(f'{v:.4g}' for v in reg['this tree'][key])} | {', '.join(f'{v:.4g}' for v in reg['parent'][key])} |")
    else:
        L += ["", "## 3. This tree against the parent commit", "", "not measured (no --parent-tree)"]
    out = Path(a.out)
    kept = out.read_text().split(KEEP, 1)[1] if out.exists() and KEEP in out.read_text() else "\n"
    out.write_text("\n".join(L) + "\n\n" + KEEP + kept)
    print("\n".join(L))


if __name__ == "__main__":
    main()
