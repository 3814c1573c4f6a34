#!/usr/bin/env python3
"""Batched ingest at the reference's shapes, measured in one visit -> profiles/project_batch.md.

  python scripts/gpu_project_batch_perf.py [--reps 30] [--out profiles/project_batch.md] [--parent-lib SO] [--alt-lib SO] [--no-trace] [--no-pmc]

  1. kernels (one `rocprofv3 --kernel-trace --stats` run of its own per library): project_pass against project_rows and project_finish,
     float and double matrix, 32768 -> 4096.  --alt-lib is a build of this tree with the other group width (-DCHIP_PROJ_WIDTH=4);
  2. FETCH_SIZE of one shared pass against one single launch (`rocprofv3 --pmc FETCH_SIZE`, a run of its own);
  3. host wall time, medians of --reps after warm-up, the libraries ALTERNATING in one process (each is mapped RTLD_LOCAL and driven
     through the C ABI, so the parent commit's library needs none of the new entry points): chip_db_append_projected_f32 at n = 1, 8
     and 64; chip_db_append_vlad_f32 and chip_db_append_f64 of one row; 16 maps of 1410 x 512, K = 16 (straight to 8192-D) and of
     540 x 512, K = 64 (through the projection) by one batched call and by the loop of single calls.
The part of an existing output file from "# What the figures say" on is kept."""
import argparse
import csv
import ctypes as C
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
IN_DIM, D = 32768, 4096
WARMUP = 3
KEEP = "# What the figures say"
HBM_PEAK = 8.0e12
P, I32, I64, U32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32


def ptr(a):
    return a.ctypes.data_as(P)


class Lib:
    """one build of libcerebro_hip.so through the C ABI: only what is measured here"""

    def __init__(self, name, path):
        self.name = name
        if "torch" not in sys.modules:                                          # one HIP runtime per process (cerebro_amd.capi.load_library)
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        self.so = C.CDLL(str(path))
        sigs = {"chip_create": [C.POINTER(P), I32, I64, I32, I32, I32], "chip_project_set": [P, I32, P, I32, P], "chip_project": [P, P, I64, P],
                "chip_db_append_projected_f32": [P, P, I64, U32, C.POINTER(I64)], "chip_db_append_f64": [P, P, I64, U32, C.POINTER(I64)],
                "chip_vlad_set": [P, I32, I32, I32, P, P, P], "chip_db_append_vlad_f32": [P, P, I32, I32, U32, C.POINTER(I64)],
                "chip_db_append_vlad_batch_f32": [P, P, I32, I32, I32, U32, C.POINTER(I64)]}
        for fn, args in sigs.items():
            if hasattr(self.so, fn):
                getattr(self.so, fn).argtypes = args
                getattr(self.so, fn).restype = C.c_int
        self.so.chip_destroy.argtypes = [P]
        self.so.chip_destroy.restype = None
        self.has_batch = hasattr(self.so, "chip_db_append_vlad_batch_f32")

    def call(self, fn, *args):
        rc = getattr(self.so, fn)(*args)
        if rc != 0:
            raise RuntimeError(f"{self.name}: {fn} returned {rc}")

    def create(self, dim):
        h = P()
        self.call("chip_create", C.byref(h), dim, 0, 0, 0, 1)
        return h


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def matrix(dtype):
    rng = np.random.default_rng(32768)
    Mt = np.tile(rng.standard_normal((D, 2048), dtype=np.float32), (1, IN_DIM // 2048))   # 512 MiB, made cheaply
    return Mt if dtype == np.float32 else Mt.astype(np.float64) * (1 + 2.0 ** -40)


def alternate(variants, reps):
    """{name: callable} -> {name: (median, min, max)} of `reps` calls each, taken in turns"""
    for _ in range(WARMUP):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def projected_appends(libs, reps):
    out = {}
    first = I64()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((64, IN_DIM), dtype=np.float32)
    for dtype in (np.float32, np.float64):
        Mt = matrix(dtype)
        ctx = {lib.name: lib.create(D) for lib in libs}
        variants = {}
        for lib in libs:
            h = ctx[lib.name]
            lib.call("chip_project_set", h, IN_DIM, ptr(Mt), 1 if dtype == np.float32 else 2, None)
            z = np.empty((1, D))
            lib.call("chip_project", h, ptr(x), 1, ptr(z))
            lib.call("chip_db_append_projected_f32", h, ptr(x), 1, 0, C.byref(first))      # the storage decision, once
            for n in (1, 8, 64):
                variants[(lib.name, f"chip_db_append_projected_f32, n = {n}")] = (lambda lib=lib, h=h, n=n: lib.call("chip_db_append_projected_f32", h, ptr(x), n, 0, C.byref(first)))
            variants[(lib.name, "chip_db_append_f64, one ready row")] = (lambda lib=lib, h=h, z=z: lib.call("chip_db_append_f64", h, ptr(z), 1, 0, C.byref(first)))
        out[np.dtype(dtype).name] = alternate(variants, reps)
        for lib in libs:
            lib.so.chip_destroy(ctx[lib.name])
        del Mt
    return out


def pooled_appends(libs, reps):
    """16 maps per call on the two routes -> {route: {(lib, call): (median, min, max)}}"""
    out = {}
    first = I64()
    B, Cch = 16, 512
    for route, N, K, dim in (("direct: 16 maps of 1410 x 512, K = 16 -> 8192", 1410, 16, 8192), ("projected: 16 maps of 540 x 512, K = 64 -> 32768 -> 4096", 540, 64, D)):
        rng = np.random.default_rng(K)
        Wt = (rng.standard_normal((K, Cch)) * 0.09).astype(np.float32)
        bias = (0.5 * rng.standard_normal(K)).astype(np.float32)
        centres = (0.3 * rng.standard_normal((K, Cch))).astype(np.float32)
        maps = np.maximum(rng.standard_normal((B, N, Cch)), 0).astype(np.float32)
        Mt = matrix(np.float32) if K * Cch != dim else None
        ctx = {lib.name: lib.create(dim) for lib in libs}
        variants = {}
        for lib in libs:
            h = ctx[lib.name]
            lib.call("chip_vlad_set", h, Cch, K, 0, ptr(Wt), ptr(bias), ptr(centres))
            if Mt is not None:
                lib.call("chip_project_set", h, IN_DIM, ptr(Mt), 1, None)
            lib.call("chip_db_append_vlad_f32", h, ptr(maps), N, 1, 0, C.byref(first))

            def loop(lib=lib, h=h):
                for m in range(B):
                    lib.call("chip_db_append_vlad_f32", h, ptr(maps[m]), N, 1, 0, C.byref(first))
            variants[(lib.name, "loop of 16 chip_db_append_vlad_f32")] = loop
            variants[(lib.name, "chip_db_append_vlad_f32, one map")] = (lambda lib=lib, h=h: lib.call("chip_db_append_vlad_f32", h, ptr(maps), N, 1, 0, C.byref(first)))
            if lib.has_batch:
                variants[(lib.name, "one chip_db_append_vlad_batch_f32 of 16")] = (lambda lib=lib, h=h: lib.call("chip_db_append_vlad_batch_f32", h, ptr(maps), B, N, 1, 0, C.byref(first)))
        out[route] = alternate(variants, reps)
        for lib in libs:
            lib.so.chip_destroy(ctx[lib.name])
    return out


def trace_child(path, n):
    """what a traced run executes: chip_project of n descriptors, both matrix types"""
    lib = Lib("traced", path)
    x = np.random.default_rng(1).standard_normal((n, IN_DIM), dtype=np.float32)
    z = np.empty((n, D))
    for dtype in (np.float32, np.float64):
        Mt = matrix(dtype)
        h = lib.create(D)
        lib.call("chip_project_set", h, IN_DIM, ptr(Mt), 1 if dtype == np.float32 else 2, None)
        for _ in range(WARMUP + 30):
            lib.call("chip_project", h, ptr(x), n, ptr(z))
        lib.so.chip_destroy(h)


def rocprof(args, path, n):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([exe, *args, "--output-format", "csv", "-d", tmp, "-o", "pb", "--", sys.executable, __file__, "--trace-child", str(path), "--n", str(n)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        rows = []
        for p in Path(tmp).rglob("*.csv"):
            with open(p, newline="") as f:
                rows += [dict(row, _file=p.name) for row in csv.DictReader(f)]
    return rows


def kernel_times(path, n):
    d = {}
    for row in rocprof(["--kernel-trace", "--stats"], path, n):
        if row["_file"].endswith("kernel_trace.csv") and "project_" in row["Kernel_Name"]:
            d.setdefault(row["Kernel_Name"], []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return {k: (len(v), statistics.median(v), min(v), max(v)) for k, v in d.items()}


def fetch_sizes(path, n):
    d = {}
    for row in rocprof(["--pmc", "FETCH_SIZE"], path, n):
        if row.get("Counter_Name") == "FETCH_SIZE" and "project_" in row.get("Kernel_Name", ""):
            d.setdefault(row["Kernel_Name"], []).append(float(row["Counter_Value"]))
    return {k: (len(v), statistics.median(v)) for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "project_batch.md"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--alt-lib")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-pmc", action="store_true")
    ap.add_argument("--trace-child")
    ap.add_argument("--n", type=int, default=8)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.trace_child, a.n)

    this = ROOT / "cerebro_amd" / "lib" / "libcerebro_hip.so"
    sys.path.insert(0, str(ROOT))
    from cerebro_amd import capi
    plan = capi.project_plan(IN_DIM, capi.CHIP_PROJ_F32, 64)
    with capi.Chip(D) as chip:
        info = chip.info()
    L = [f"# Batched ingest at {IN_DIM} -> {D}: measured figures", "",
         f"Written by `scripts/gpu_project_batch_perf.py --reps {a.reps}` on {info['arch']} ({info['n_cus']} CUs).  This tree's group width is {plan['width']}",
         f"(slab {plan['slab']} elements, {plan['lds_bytes']} B of LDS, {plan['block']} threads).  Host wall times are medians of {a.reps} calls after warm-up,",
         "the libraries alternating in one process; every call ends in a stream synchronise.", ""]
    builds = [("this tree", this)] + ([("other width", Path(a.alt_lib))] if a.alt_lib else []) + ([("parent", Path(a.parent_lib))] if a.parent_lib else [])
    if not a.no_trace:
        L += ["## 1. Kernel times (rocprofv3 --kernel-trace --stats, a run of its own per library: ns over the calls)", "",
              "| library | descriptors per call | kernel | calls | median us | min .. max us | matrix bytes | share of 8 TB/s | us per descriptor |", "|---|---|---|---|---|---|---|---|---|"]
        for name, path in builds:
            n = 1 if name == "parent" else 12 - plan["width"] if name == "other width" else plan["width"]   # widths 4 and 8
            for k, (calls, med, lo, hi) in sorted(kernel_times(path, n).items()):
                nbytes = IN_DIM * D * (8 if "<double" in k else 4) if "project_finish" not in k else None
                per = n if "project_pass" in k else 1
                L.append(f"| {name} | {n} | `{k}` | {calls} | {med / 1e3:.1f} | {lo / 1e3:.1f} .. {hi / 1e3:.1f} | {nbytes or ''} | "
                         f"{(f'{nbytes / (med * 1e-9) / HBM_PEAK:.3f}' if nbytes else '')} | {med / 1e3 / per:.1f} |")
    else:
        L += ["## 1. Kernel times", "", "not measured (--no-trace)"]
    if not a.no_pmc:
        L += ["", "## 2. FETCH_SIZE (rocprofv3 --pmc FETCH_SIZE, a run of its own; KiB as the counter reports them, median over the calls)", "",
              "| descriptors per call | kernel | calls | FETCH_SIZE |", "|---|---|---|---|"]
        try:
            for n in (plan["width"], 1):
                for k, (calls, med) in sorted(fetch_sizes(this, n).items()):
                    L.append(f"| {n} | `{k}` | {calls} | {med:.0f} |")
        except Exception as e:                                                   # the counter may not be collectable on a shared machine
            L.append(f"| | not measured: {str(e).splitlines()[-1][:120]} | | |")
    else:
        L += ["", "## 2. FETCH_SIZE", "", "not measured (--no-pmc)"]
    libs = [Lib(name, path) for name, path in builds]
    L += ["", "## 3. chip_db_append_projected_f32 (ms per call: median, min .. max; descriptors per second from the median)", "",
          "| matrix | library | call | median | min .. max | descriptors / s |", "|---|---|---|---|---|---|"]
    for dt, rows in projected_appends(libs, a.reps).items():
        for (lib, call), (med, lo, hi) in rows.items():
            n = int(call.rsplit("= ", 1)[1]) if "n = " in call else 1
            L.append(f"| {dt} | {lib} | {call} | {med:.3f} | {lo:.3f} .. {hi:.3f} | {1e3 * n / med:.0f} |")
    L += ["", "## 4. Pooled appends, 16 maps (ms: median, min .. max)", "", "| route | library | call | median | min .. max |", "|---|---|---|---|---|"]
    for route, rows in pooled_appends(libs, a.reps).items():
        for (lib, call), (med, lo, hi) in rows.items():
            L.append(f"| {route} | {lib} | {call} | {med:.3f} | {lo:.3f} .. {hi:.3f} |")
    out = Path(a.out)
    kept = out.read_text().split(KEEP, 1)[1] if out.exists() and KEEP in out.read_text() else "\n"
    out.write_text("\n".join(L) + "\n\n" + KEEP + kept)
    print("\n".join(L))


if __name__ == "__main__":
    main()
