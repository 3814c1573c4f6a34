#!/usr/bin/env python3
"""The NetVLAD pooling at the two production shapes, measured in one visit -> profiles/vlad.md.

  python scripts/gpu_vlad_perf.py [--reps 30] [--out profiles/vlad.md] [--no-trace] [--parent-tree DIR]

  1. host wall time, medians of --reps after warm-up, the variants ALTERNATING in one process:
       default model  1410 x 512, K = 16 -> D = 8192:  chip_db_append_vlad_f32 | chip_vlad | chip_db_append_f64 of a ready row
       Relja          540 x 512, K = 64 -> 32768 -> 4096 (float matrix):  chip_db_append_vlad_f32 | chip_vlad |
                      chip_db_append_projected_f32 of a ready vector
     and a plain float32 numpy evaluation of the layer on this host, as the "what it replaces" figure -- numpy, NOT TensorFlow: the
     reference's TF1 server runs on no machine of this project;
  2. the vlad_* kernels from one `rocprofv3 --kernel-trace --stats` run of its own;
  3. with --parent-tree (a checkout of the parent commit with its library built): chip_db_append_f64 (D = 8192, one ready row) and
     chip_db_append_projected_f32 (32768 -> 4096, one ready vector), medians of --reps, one child process per tree and round, the
     trees alternating and taking turns to go first: ctx_append / append_pass gained a branch, and these are the calls through it.
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
sys.path.insert(0, os.environ.get("GPU_VLAD_TREE") or str(ROOT))     # (the children of part 3 import the tree they are told to)

import numpy as np  # noqa: E402

WARMUP = 3
KEEP = "# What the figures say"
SHAPES = {"default": dict(N=1410, C=512, K=16, D=8192, in_dim=0), "relja": dict(N=540, C=512, K=64, D=4096, in_dim=32768)}


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def data(s):
    rng = np.random.default_rng(s["N"] + s["K"])
    Wt = (rng.standard_normal((s["K"], s["C"])) * (2.0 / np.sqrt(s["C"]))).astype(np.float32)
    bias = (0.5 * rng.standard_normal(s["K"])).astype(np.float32)
    centres = (0.3 * rng.standard_normal((s["K"], s["C"]))).astype(np.float32)
    x = np.maximum(rng.standard_normal((s["N"], s["C"])), 0).astype(np.float32)
    Mt = rng.standard_normal((s["D"], s["in_dim"]), dtype=np.float32) if s["in_dim"] else None
    return Wt, bias, centres, x, Mt


def numpy_layer(x, Wt, bias, centres):
    """the Keras layer in float32 numpy: softmax(x W + b), sum a (x + C) as two matrix products, both normalisations"""
    s = x @ Wt.T + bias
    e = np.exp(s - s.max(axis=1, keepdims=True))
    a = e / e.sum(axis=1, keepdims=True)
    W = a.T @ x + a.sum(axis=0)[:, None] * centres
    W /= np.sqrt(np.maximum((W * W).sum(axis=1, keepdims=True), 1e-12))
    w = W.ravel()
    return w / np.sqrt(max(float(w @ w), 1e-12))


def wall_times(reps):
    from cerebro_amd import capi
    out = {}
    for name, s in SHAPES.items():
        Wt, bias, centres, x, Mt = data(s)
        with capi.Chip(s["D"]) as chip:
            chip.vlad_set(Wt, bias, centres)
            if Mt is not None:
                chip.project_set(Mt)
            v = chip.vlad(x)
            ready = (lambda: chip.append_projected(v)) if Mt is not None else (lambda r=v.astype(np.float64)[None, :]: chip.append_f64(r))
            variants = {"chip_db_append_vlad_f32": lambda: chip.append_vlad(x, positions=s["N"]),
                        "chip_vlad": lambda: chip.vlad(x, positions=s["N"]),
                        ("chip_db_append_projected_f32 of a ready vector" if Mt is not None else "chip_db_append_f64 of a ready row"): ready,
                        "numpy float32 evaluation of the layer on this host (not TF)": lambda: numpy_layer(x, Wt, bias, centres)}
            for _ in range(WARMUP):
                for fn in variants.values():
                    fn()
            t = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    t[k].append(ms(fn))
            out[name] = {k: (statistics.median(u), min(u), max(u)) for k, u in t.items()}
    return out


def trace_child():
    from cerebro_amd import capi
    for name, s in SHAPES.items():
        Wt, bias, centres, x, _ = data(s)
        with capi.Chip(256) as chip:                           # chip_vlad needs nothing of the DB
            chip.vlad_set(Wt, bias, centres)
            xt = np.ascontiguousarray(x.T)
            for _ in range(WARMUP + 30):
                chip.vlad(x, positions=s["N"])
            for _ in range(WARMUP + 30):
                chip.vlad(xt, capi.CHIP_VLAD_NCHW, positions=s["N"])


def kernel_trace():
    """-> {kernel name: [durations ns]} from one rocprofv3 run of trace_child (the two shapes follow each other: 66 calls each)"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "vlad", "--", sys.executable, __file__, "--trace-child"],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        rows = []
        for path in Path(tmp).rglob("*kernel_trace.csv"):
            with open(path, newline="") as f:
                rows += [(int(row["Start_Timestamp"]), row["Kernel_Name"], int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) for row in csv.DictReader(f)]
    durations = {}
    for _, name, d in sorted(rows):
        durations.setdefault(name, []).append(d)
    return durations


def append_child(reps):
    """chip_db_append_f64 at D = 8192 and chip_db_append_projected_f32 at 32768 -> 4096 of whatever tree this process imports"""
    from cerebro_amd import capi
    rng = np.random.default_rng(5)
    out = {}
    with capi.Chip(8192) as chip:
        row = rng.standard_normal((1, 8192)).astype(np.float32).astype(np.float64)
        for _ in range(WARMUP):
            chip.append_f64(row)
        out["chip_db_append_f64_ms"] = statistics.median(ms(lambda: chip.append_f64(row)) for _ in range(reps))
    with capi.Chip(4096) as chip:
        chip.project_set(rng.standard_normal((4096, 32768), dtype=np.float32))
        x = rng.standard_normal(32768, dtype=np.float32)
        for _ in range(WARMUP):
            chip.append_projected(x)
        out["chip_db_append_projected_f32_ms"] = statistics.median(ms(lambda: chip.append_projected(x)) for _ in range(reps))
    print(json.dumps(out))


def regression(parent: Path, reps, rounds):
    out = {"this tree": {}, "parent": {}}
    for i in range(rounds):
        for name, root in (("this tree", ROOT), ("parent", parent))[::1 if i % 2 == 0 else -1]:
            r = subprocess.run([sys.executable, __file__, "--append-child", "--reps", str(reps)], cwd=root, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, GPU_VLAD_TREE=str(root)))
            if r.returncode != 0:
                raise RuntimeError(f"append child of {name} failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
            for k, v in json.loads(r.stdout.splitlines()[-1]).items():
                out[name].setdefault(k, []).append(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vlad.md"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=5, help="child processes per tree of part 3")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--append-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        return trace_child()
    if a.append_child:
        return append_child(a.reps)

    from cerebro_amd import capi
    with capi.Chip(256) as chip:
        info = chip.info()
    L = ["# The NetVLAD pooling at the two production shapes: measured figures", "",
         f"Written by `scripts/gpu_vlad_perf.py --reps {a.reps}` on {info['arch']} ({info['n_cus']} CUs).  Host wall times are medians of {a.reps} calls",
         "after warm-up, the variants alternating in one process; every device call ends in a stream synchronise.", ""]
    L += ["## 1. Host wall time per call (ms: median, min .. max)", "", "| shape | call | median | min .. max |", "|---|---|---|---|"]
    for name, rows in wall_times(a.reps).items():
        s = SHAPES[name]
        shape = f"{name}: {s['N']} x {s['C']}, K = {s['K']}" + (f" -> {s['in_dim']} -> {s['D']}" if s["in_dim"] else f" -> {s['D']}")
        for k, (med, lo, hi) in rows.items():
            L.append(f"| {shape} | {k} | {med:.3f} | {lo:.3f} .. {hi:.3f} |")
    if not a.no_trace:
        L += ["", "## 2. Kernel times (rocprofv3 --kernel-trace --stats, a run of its own: median us over the calls of each shape)", "",
              "| kernel | calls | default shape | Relja shape |", "|---|---|---|---|"]
        for name, d in sorted(kernel_trace().items()):
            if "vlad_" in name:
                first, second = d[:len(d) // 2], d[len(d) // 2:]       # trace_child: every call of the default shape, then Relja's
                L.append(f"| `{name}` | {len(d)} | {statistics.median(first) / 1e3:.1f} | {statistics.median(second) / 1e3:.1f} |")
    else:
        L += ["", "## 2. Kernel times", "", "not measured (--no-trace)"]
    if a.parent_tree:
        reg = regression(Path(a.parent_tree).resolve(), a.reps, a.rounds)
        L += ["", f"## 3. This tree against the parent commit: medians of {a.reps} (ms), one child process per entry, alternating in one visit", "",
              "| call | this tree | range | parent | range |", "|---|---|---|---|---|"]
        for key in sorted(reg["this tree"]):
            t, p = reg["this tree"][key], reg["parent"][key]
            L.append(f"| {key} | {', '.join(f'{v:.4f}' for v in t)} | {min(t):.4f} .. {max(t):.4f} | {', '.join(f'{v:.4f}' for v in p)} | {min(p):.4f} .. {max(p):.4f} |")
    else:
        L += ["", "## 3. This tree against the parent commit", "", "not measured (no --parent-tree)"]
    out = Path(a.out)
    kept = out.read_text().split(KEEP, 1)[1] if out.exists() and KEEP in out.read_text() else "\n"
    out.write_text("\n".join(L) + "\n\n" + KEEP + kept)
    print("\n".join(L))


if __name__ == "__main__":
    main()
