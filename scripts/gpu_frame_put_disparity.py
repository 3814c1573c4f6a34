#!/usr/bin/env python3
"""Measures chip_frame_put_disparity (CHIP_DISP_S16 and CHIP_DISP_F32) against chip_frame_put, the parent's unchanged call and the
yardstick, and chip_disparity_to_xyz against the host loop of examples/frame_put_disparity.cc (profiles/frame_put_disparity.md holds
this script's output).

  python scripts/gpu_frame_put_disparity.py [--reps 30] [--limit 280] [--out profiles/frame_put_disparity.md] [--no-trace]

On the 5323-keypoint frame at 752 x 480 of profiles/match_store.md (full_5000_5000, the b frame), its 3-D image turned into an int16
disparity (the nearest raw value at a stored pixel, StereoBM's -16 elsewhere):
  1. ONE process times the four calls: 5 warm-up rounds, then --reps rounds in which chip_frame_put, the two disparity puts (replaces
     in their own slots) and chip_disparity_to_xyz ALTERNATE; medians, and the spread (min .. max) of chip_frame_put;
  2. the example binary times the same calls from C++ and the plain host loop on the host CPU (frame_put_disparity 5323 3 reps);
  3. kernel times come from ONE `rocprofv3 --kernel-trace --stats` run of its own over a child that repeats the rounds.
Every call's status is checked and the records of the three puts are compared; the first failure ends the script.  The script runs under
a time limit of its own: --limit seconds for the whole run (an alarm ends the process; the children get what is left of it).  A section
of the output file that starts with the line "# What the figures say" is kept as it is."""
from __future__ import annotations

import argparse
import csv
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
KERNELS = ("frame_gather", "disparity_gather", "disparity_to_xyz")
KEEP = "# What the figures say"
# EuRoC-like cv::stereoRectify Q: [1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0 1/baseline 0]
F_PX, CX, CY, BASELINE = 458.654, 367.215803962, 248.375340610, 0.110073808127
Q = np.array([[1, 0, 0, -CX], [0, 1, 0, -CY], [0, 0, 0, F_PX], [0, 0, 1.0 / BASELINE, 0]], np.float64)


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def disparity_of(xyz: np.ndarray) -> np.ndarray:
    q23, q32 = float(np.float32(Q[2, 3])), float(np.float32(Q[3, 2]))
    z = xyz[:, :, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        raw = np.rint(16.0 * (q23 / z) / q32)
    ok = (z != 0) & np.isfinite(raw) & (raw >= -32768) & (raw <= 32767)
    return np.where(ok, raw, -16.0).astype(np.int16)


def prepare(chip):
    """the calls as raw ctypes calls on arrays prepared once; ids 0 (image), 1 (int16 disparity), 2 (float disparity)"""
    b = synth.make_match_scene(**FULL)["b"]
    desc = np.ascontiguousarray(b["desc"], np.uint8)
    kp = np.ascontiguousarray(b["kp"], np.float32)
    d16 = disparity_of(np.asarray(b["xyz"], np.float32))
    d32 = d16.astype(np.float32)
    h, w = d16.shape
    n = len(kp)
    Qd = np.ascontiguousarray(Q).reshape(16)
    lib, hd = chip.lib, chip.h
    chip.frame_store_reserve(3, n)
    xyz = chip.disparity_to_xyz(d16, Q)                              # the image chip_frame_put gets: the same frame
    dense = np.zeros_like(xyz)
    f = capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, n, w, h, xyz.ctypes.data)

    def check(st, what):
        if st != 0:
            sys.exit(f"{what} -> status {st}")

    calls = dict(
        put=lambda: check(lib.chip_frame_put(hd, 0, capi.C.byref(f)), "chip_frame_put"),
        s16=lambda: check(lib.chip_frame_put_disparity(hd, 1, capi._ptr(desc), capi._ptr(kp), n, w, h, capi._ptr(d16), capi.CHIP_DISP_S16, capi._ptr(Qd)), "chip_frame_put_disparity"),
        f32=lambda: check(lib.chip_frame_put_disparity(hd, 2, capi._ptr(desc), capi._ptr(kp), n, w, h, capi._ptr(d32), capi.CHIP_DISP_F32, capi._ptr(Qd)), "chip_frame_put_disparity"),
        dense=lambda: check(lib.chip_disparity_to_xyz(hd, capi._ptr(d16), capi.CHIP_DISP_S16, w, h, capi._ptr(Qd), capi._ptr(dense)), "chip_disparity_to_xyz"))

    def same():
        pts = [chip.frame_read(i)["pts"].tobytes() for i in range(3)]
        if not (pts[0] == pts[1] == pts[2]) or dense.tobytes() != xyz.tobytes():
            sys.exit("the three puts or the two dense images differ")

    sizes = dict(n=n, w=w, h=h, put=xyz.nbytes, s16=d16.nbytes, f32=d32.nbytes)
    return calls, same, sizes, (desc, kp, d16, d32, Qd, xyz, dense, f)


def rounds(calls, reps: int) -> dict:
    t = {k: [] for k in calls}
    for r in range(WARMUP + reps):                                   # the variants alternate inside the timed window
        for k, fn in calls.items():
            v = ms(fn)
            if r >= WARMUP:
                t[k].append(v)
    return t


def kernel_times(trace_dir: Path) -> dict:
    """kernel -> (calls, average us, min us) from the kernel trace rocprofv3 wrote as csv"""
    out = {}
    for path in trace_dir.rglob("*kernel_trace.csv"):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                for k in KERNELS:
                    if re.search(r"\b" + k + r"\b", name):
                        out.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: (len(v), statistics.mean(v), min(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_put_disparity.md"))
    ap.add_argument("--limit", type=int, default=280, help="seconds the whole run may take")
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes its csv files (default: a temporary directory, removed afterwards)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    left = lambda: max(1, int(deadline - time.monotonic()))          # noqa: E731
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        calls, same, sz, keep = prepare(chip)
        t = rounds(calls, args.reps)
        same()
    if args.child:
        return
    med = {k: statistics.median(v) for k, v in t.items()}
    out = [f"# chip_frame_put_disparity against chip_frame_put ({arch}, medians of {args.reps} after {WARMUP} warm-up rounds, scripts/gpu_frame_put_disparity.py)", "",
           f"Frame: {sz['n']} keypoints at {sz['w']} x {sz['h']} (full_5000_5000, the b frame of profiles/match_store.md), its image as an int16 disparity.",
           "Host wall time of the calls, each a replace in its own slot; the variants alternate in one process.", "",
           "| call | bytes of the map uploaded (MB) | median (ms) | min .. max (ms) | against chip_frame_put |", "|---|---|---|---|---|"]
    for k, label in (("put", "chip_frame_put (3-D image)"), ("s16", "chip_frame_put_disparity, CHIP_DISP_S16"), ("f32", "chip_frame_put_disparity, CHIP_DISP_F32")):
        out.append(f"| {label} | {sz[k] / 1e6:.2f} | {med[k]:.3f} | {min(t[k]):.3f} .. {max(t[k]):.3f} | {med[k] / med['put']:.2f} |")
    out += ["", f"chip_disparity_to_xyz (upload {sz['s16'] / 1e6:.2f} MB, kernel, {sz['put'] / 1e6:.2f} MB back into pageable memory): "
            f"median {med['dense']:.3f} ms, min .. max {min(t['dense']):.3f} .. {max(t['dense']):.3f}.", ""]
    # 2: the example's C++ timing, with the host loop on the host CPU
    exe = ROOT / "cerebro_amd" / "lib" / "frame_put_disparity"
    line = None
    if exe.exists():
        p = subprocess.run([str(exe), str(sz["n"]), "3", str(args.reps)], capture_output=True, text=True, timeout=left())
        m = re.search(r"^timing .*$", p.stdout, flags=re.M)
        if p.returncode != 0 or not m:
            sys.exit("the example failed:\n" + p.stdout + p.stderr)
        line = m.group(0)
        hm = re.search(r"host loop ([\d.]+), chip_disparity_to_xyz ([\d.]+)", line)
        out += ["The same calls from C++ (examples/frame_put_disparity.cc, one process, alternating), with the reference's loop restated on the host CPU:", "",
                "    " + line, "",
                f"Host loop {float(hm.group(1)):.3f} ms against chip_disparity_to_xyz {float(hm.group(2)):.3f} ms: ratio {float(hm.group(1)) / float(hm.group(2)):.2f}.", ""]
    else:
        out += ["The example binary is not built: host loop **not measured**.", ""]
    # 3: kernel times, one rocprofv3 run of its own
    kt = {}
    if not args.no_trace and shutil.which("rocprofv3"):
        td = Path(args.trace_dir or tempfile.mkdtemp(prefix="frame_put_disparity_trace_"))
        td.mkdir(parents=True, exist_ok=True)
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(td), "-o", "fpd", "--", sys.executable, __file__,
                            "--child", "--reps", str(args.reps), "--limit", str(left())], capture_output=True, text=True, timeout=left())
        if p.returncode != 0:
            sys.exit("the traced child failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
        kt = kernel_times(td)
        if not args.trace_dir:
            shutil.rmtree(td, ignore_errors=True)
    if kt:
        out += ["Kernels (`rocprofv3 --kernel-trace --stats`, a run of its own over the same rounds; us):", "", "| kernel | calls | average | min |", "|---|---|---|---|"]
        out += [f"| `{k}` | {kt[k][0]} | {kt[k][1]:.1f} | {kt[k][2]:.1f} |" for k in KERNELS if k in kt]
    else:
        out += ["Kernel times: **not measured**."]
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
