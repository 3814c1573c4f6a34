#!/usr/bin/env python3
"""chip_orb_detect on the 752 x 480 textured frame at the defaults, measured in one visit -> profiles/orb_detect.md.

  python scripts/gpu_orb_detect.py [--reps 30] [--limit 420] [--out profiles/orb_detect.md] [--no-trace] [--parent-lib SO]

  1. host wall time of the call, median of --reps after warm-up, with n and the per-level counts;
  2. examples/orb_detect with a repetition count: the same call from C++ and the example's host restatement of the definition (a plain
     loop, not OpenCV's implementation); cv::ORB itself only where OpenCV exists;
  3. the kernels from one `rocprofv3 --kernel-trace --stats` run of its own over the same rounds;
  4. with --parent-lib: chip_match_batch_stored at B = 8 of this tree and of that build of the parent commit, two child processes
     each, alternating.
The part of an existing output file from "# What the figures say" on is kept."""
import argparse
import csv
import json
import os
import re
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from cerebro_amd import capi, synth  # noqa: E402

FULL = dict(n_true=4600, n_outlier_a=400, n_outlier_b=900, flip_rate=0.05, n_duplicates=60, n_border=48, seed=12)
WARMUP = 5
KERNELS = ("orb_pyramid", "orb_fast_score", "orb_candidates", "orb_select", "orb_moments")
ORB = ("chip_orb_params_default", "chip_build_has_orb_detect", "chip_orb_plan", "chip_orb_detect", "chip_debug_orb_level")
KEEP = "# What the figures say"
W, H, B = 752, 480, 8


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def frame() -> np.ndarray:
    """blocks of 5 pixels of random brightness under pixel noise (tests/orb_detect_cases.py: texture)"""
    rng = np.random.default_rng(752480)
    blocks = rng.integers(30, 226, ((H + 4) // 5, (W + 4) // 5))
    img = np.repeat(np.repeat(blocks, 5, 0), 5, 1)[:H, :W] + rng.integers(-25, 26, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)


def detect_rounds(reps: int):
    img = frame()
    kp = np.zeros(capi.CHIP_ORB_N_FEATURES, capi.ORB_KEYPOINT_DTYPE)
    n = capi.C.c_int32()
    counts = (capi.C.c_int32 * 8)()
    t = []
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        for r in range(WARMUP + reps):
            def call():
                st = chip.lib.chip_orb_detect(chip.h, capi._ptr(img), W, H, None, capi._ptr(kp), len(kp), capi.C.byref(n), counts)
                if st != 0:
                    sys.exit(f"chip_orb_detect -> status {st}")
            v = ms(call)
            if r >= WARMUP:
                t.append(v)
    return arch, t, n.value, list(counts)


def stored_rounds(reps: int):
    sc = synth.make_match_scene(**FULL)
    Kinv = np.ascontiguousarray(sc["Kinv"], np.float64)
    t = []
    with capi.Chip(4096) as chip:
        chip.frame_store_reserve(B + 1, max(len(sc["a"]["kp"]), len(sc["b"]["kp"])))
        chip.frame_put(0, sc["a"])
        for j in range(B):
            chip.frame_put(1 + j, sc["b"])
        ids = list(range(1, B + 1))
        for r in range(WARMUP + reps):
            v = ms(lambda: chip.match_batch_stored(0, ids, Kinv))
            if r >= WARMUP:
                t.append(v)
    return t


def kernel_times(trace_dir: Path) -> dict:
    out = {}
    for path in trace_dir.rglob("*kernel_trace.csv"):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                for k in KERNELS:
                    if re.search(r"\b" + k + r"\b", name):
                        out.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: (len(v), statistics.median(v), min(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "orb_detect.md"))
    ap.add_argument("--limit", type=int, default=420, help="seconds the whole run may take")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libcerebro_hip.so of the parent commit, for section 4")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-json", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    left = lambda: max(1, int(deadline - time.monotonic()))          # noqa: E731
    if args.child_json:
        if os.environ.get("CHIP_LIB"):                               # another build of the library: it lacks the new entries
            for name in ORB:
                capi._SIGS.pop(name, None)
        t = stored_rounds(args.reps)
        print("JSON " + json.dumps([statistics.median(t), min(t), max(t)]))
        return
    arch, t, n, counts = detect_rounds(args.reps)
    if args.child:
        return
    out = [f"# chip_orb_detect on a 752 x 480 frame at the defaults ({arch}, medians of {args.reps} after {WARMUP} warm-up rounds, scripts/gpu_orb_detect.py)", "",
           f"Frame: the synthetic textured {W} x {H} frame of tests/orb_detect_cases.py; n_features 5000, 8 levels, FAST threshold 0, border 31.",
           f"n = {n}, per level {counts}.", "",
           f"chip_orb_detect (upload 0.36 MB, 7 + 4 launches, {32 + 32 * 5000} bytes back, host wall time): median {statistics.median(t):.3f} ms, "
           f"min .. max {min(t):.3f} .. {max(t):.3f}.", ""]
    exe = ROOT / "cerebro_amd" / "lib" / "orb_detect"
    if exe.exists():
        p = subprocess.run([str(exe), str(max(3, args.reps // 3))], capture_output=True, text=True, timeout=left())
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        if p.returncode != 0 or len(lines) < 4:
            sys.exit("the example failed:\n" + p.stdout + p.stderr)
        out += ["The same call from C++ (examples/orb_detect.cc) next to the definition restated as a plain loop on the host CPU:", ""] + ["    " + l for l in lines]
        out += ["", "That loop is this project's restatement, a plain loop, not OpenCV's implementation: no speed-up against cv::ORB follows from it."]
    else:
        out += ["The example binary is not built: host restatement **not measured**."]
    try:
        import cv2
        orb = cv2.ORB_create(5000)
        orb.setFastThreshold(0)
        img = frame()
        tc = [ms(lambda: orb.detect(img, None)) for _ in range(WARMUP + args.reps)][WARMUP:]
        out += [f"cv::ORB::detect (OpenCV {cv2.__version__}) on this host: median {statistics.median(tc):.2f} ms."]
    except ImportError:
        out += ["cv::ORB on the target host: **not measured** (no OpenCV on it)."]
    out += [""]
    kt = {}
    if not args.no_trace and shutil.which("rocprofv3"):
        td = Path(tempfile.mkdtemp(prefix="orb_detect_trace_"))
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(td), "-o", "orb", "--", sys.executable, __file__,
                            "--child", "--reps", str(args.reps), "--limit", str(left())], capture_output=True, text=True, timeout=left())
        if p.returncode != 0:
            sys.exit("the traced child failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
        kt = kernel_times(td)
        shutil.rmtree(td, ignore_errors=True)
    if kt:
        out += ["Kernels (`rocprofv3 --kernel-trace --stats`, a run of its own over the same rounds; us; orb_pyramid runs once per level above 0):", "",
                "| kernel | launches | median | min |", "|---|---|---|---|"]
        out += [f"| `{k}` | {kt[k][0]} | {kt[k][1]:.1f} | {kt[k][2]:.1f} |" for k in KERNELS if k in kt]
    else:
        out += ["Kernel times: **not measured**."]
    if args.parent_lib:
        rows = []
        for label, lib in (("this tree", None), ("parent", args.parent_lib)) * 2:
            env = dict(os.environ)
            if lib:
                env.update(CHIP_LIB=str(Path(lib).resolve()), CHIP_ALLOW_LIB_OVERRIDE="1")
            p = subprocess.run([sys.executable, __file__, "--child-json", "--reps", str(args.reps), "--limit", str(left())], capture_output=True, text=True,
                               timeout=left(), env=env)
            m = re.search(r"^JSON (.*)$", p.stdout, flags=re.M)
            if p.returncode != 0 or not m:
                sys.exit("a comparison child failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
            rows.append((label, json.loads(m.group(1))))
        out += ["", f"chip_match_batch_stored at B = {B} (the frames of profiles/match_store.md) on this tree and on a build of the parent commit, one process "
                "each, alternating (median, min .. max; ms):", "", "| build | chip_match_batch_stored |", "|---|---|"]
        out += [f"| {label} | {r[0]:.3f} ({r[1]:.3f} .. {r[2]:.3f}) |" for label, r in rows]
    text = "\n".join(out) + "\n"
    dst = Path(args.out)
    if dst.exists() and KEEP in dst.read_text():
        old = dst.read_text()
        text += "\n" + old[old.index(KEEP):]
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
