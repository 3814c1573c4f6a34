#!/usr/bin/env python3
"""Measures chip_frame_put_stereo against chip_frame_put_disparity (CHIP_DISP_S16) and chip_frame_put (3-D image), chip_stereo_bm, and
the kernels bm_prefilter, bm_keypoints and bm_dense (profiles/frame_put_stereo.md holds this script's output).

  python scripts/gpu_frame_put_stereo.py [--reps 30] [--limit 420] [--out profiles/frame_put_stereo.md] [--no-trace] [--parent-lib SO]

On the 5323 keypoints at 752 x 480 of profiles/match_store.md (full_5000_5000, the b frame) with a synthetic rectified pair (a random
texture smoothed once, the left image shifted by a piecewise-constant integer disparity of 4 .. 40 pixels per 94-pixel tile):
  1. ONE process times the calls: 5 warm-up rounds, then --reps rounds in which chip_frame_put (the image chip_disparity_to_xyz makes of
     the map), chip_frame_put_disparity (the map chip_stereo_bm makes of the pair), chip_frame_put_stereo and chip_stereo_bm ALTERNATE;
     medians and spreads.  The script FAILS when the stereo put's median exceeds chip_frame_put's;
  2. the example binary times the same calls from C++ and its plain host restatement of the definition (NOT OpenCV's implementation);
  3. kernel times come from ONE `rocprofv3 --kernel-trace --stats` run of its own over a child that repeats the rounds;
  4. with --parent-lib: chip_frame_put and chip_frame_put_disparity of this tree and of that build of the parent commit, two child
     processes each, alternating (CHIP_LIB / CHIP_ALLOW_LIB_OVERRIDE select the library).
Every call's status is checked and the records of the three puts are compared; the first failure ends the script.  The script runs under
a time limit of its own: --limit seconds for the whole run.  A section of the output file that starts with the line
"# What the figures say" is kept as it is."""
from __future__ import annotations

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
KERNELS = ("frame_gather", "disparity_gather", "bm_prefilter", "bm_keypoints", "bm_dense")
STEREO = ("chip_stereo_bm_params_default", "chip_build_has_stereo_bm", "chip_stereo_bm", "chip_frame_put_stereo")
KEEP = "# What the figures say"
F_PX, CX, CY, BASELINE = 458.654, 367.215803962, 248.375340610, 0.110073808127
Q = np.array([[1, 0, 0, -CX], [0, 1, 0, -CY], [0, 0, 0, F_PX], [0, 0, 1.0 / BASELINE, 0]], np.float64)
W, H, TILE, PAD = 752, 480, 94, 64


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def stereo_pair(rng):
    """-> (left, right) uint8 (H, W)"""
    t = rng.integers(0, 256, (H, W + PAD)).astype(np.int32)
    p = np.pad(t, 1, mode="edge")
    base = ((sum(p[dy:dy + H, dx:dx + W + PAD] for dy in range(3) for dx in range(3)) + 4) // 9).astype(np.uint8)
    shifts = rng.integers(4, 41, ((H + TILE - 1) // TILE, (W + TILE - 1) // TILE))
    s = np.repeat(np.repeat(shifts, TILE, 0), TILE, 1)[:H, :W]
    return np.take_along_axis(base, np.arange(W)[None, :] + PAD - s, 1), np.ascontiguousarray(base[:, PAD:])


def synthetic_map(rng) -> np.ndarray:
    """for a library without the block matcher (the parent): an int16 map of the same size with a fifth of the pixels invalid"""
    d = rng.integers(64, 640, (H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.2] = -16
    return d


def prepare(chip, stereo: bool):
    """the calls as raw ctypes calls on arrays prepared once; ids 0 (image), 1 (int16 map), 2 (pair)"""
    b = synth.make_match_scene(**FULL)["b"]
    desc = np.ascontiguousarray(b["desc"], np.uint8)
    kp = np.ascontiguousarray(b["kp"], np.float32)
    n = len(kp)
    rng = np.random.default_rng(7)
    left, right = stereo_pair(rng)
    Qd = np.ascontiguousarray(Q).reshape(16)
    lib, hd = chip.lib, chip.h
    chip.frame_store_reserve(3, n)
    d16 = chip.stereo_bm(left, right) if stereo else synthetic_map(rng)
    xyz = chip.disparity_to_xyz(d16, Q)                              # the image chip_frame_put gets: the same frame
    dense = np.zeros_like(d16)
    f = capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, n, W, H, xyz.ctypes.data)

    def check(st, what):
        if st != 0:
            sys.exit(f"{what} -> status {st}")

    calls = dict(
        put=lambda: check(lib.chip_frame_put(hd, 0, capi.C.byref(f)), "chip_frame_put"),
        s16=lambda: check(lib.chip_frame_put_disparity(hd, 1, capi._ptr(desc), capi._ptr(kp), n, W, H, capi._ptr(d16), capi.CHIP_DISP_S16, capi._ptr(Qd)), "chip_frame_put_disparity"))
    if stereo:
        calls["pair"] = lambda: check(lib.chip_frame_put_stereo(hd, 2, capi._ptr(desc), capi._ptr(kp), n, W, H, capi._ptr(left), capi._ptr(right), None, capi._ptr(Qd)), "chip_frame_put_stereo")
        calls["dense"] = lambda: check(lib.chip_stereo_bm(hd, capi._ptr(left), capi._ptr(right), W, H, None, capi._ptr(dense)), "chip_stereo_bm")

    def same():
        pts = [chip.frame_read(i)["pts"] for i in range(3 if stereo else 2)]
        if any(p.tobytes() != pts[0].tobytes() for p in pts) or (stereo and dense.tobytes() != d16.tobytes()):
            sys.exit("the puts or the two dense maps differ")
        return int((pts[0][:, 2] > 0.1).sum())

    sizes = dict(n=n, put=xyz.nbytes, s16=d16.nbytes, pair=left.nbytes + right.nbytes, valid=float((d16 != -16).mean()))
    return calls, same, sizes, (desc, kp, d16, left, right, Qd, xyz, dense, f)


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_put_stereo.md"))
    ap.add_argument("--limit", type=int, default=420, help="seconds the whole run may take")
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes its csv files (default: a temporary directory, removed afterwards)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libcerebro_hip.so of the parent commit, for section 4")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-json", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    left = lambda: max(1, int(deadline - time.monotonic()))          # noqa: E731
    if args.child_json and os.environ.get("CHIP_LIB"):               # another build of the library: it may lack the new entries
        for name in STEREO:
            capi._SIGS.pop(name, None)
    stereo = not args.child_json                                     # the comparison children run the same two calls on the same map
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        calls, same, sz, keep = prepare(chip, stereo)
        t = rounds(calls, args.reps)
        with_depth = same()
    if args.child_json:
        print("JSON " + json.dumps({k: [statistics.median(v), min(v), max(v)] for k, v in t.items() if k in ("put", "s16")}))
        return
    if args.child:
        return
    med = {k: statistics.median(v) for k, v in t.items()}
    out = [f"# chip_frame_put_stereo against the two other puts ({arch}, medians of {args.reps} after {WARMUP} warm-up rounds, scripts/gpu_frame_put_stereo.py)", "",
           f"Frame: {sz['n']} keypoints at {W} x {H} (full_5000_5000, the b frame of profiles/match_store.md) with a synthetic rectified pair; "
           f"{100 * sz['valid']:.0f} % of its map's pixels and {with_depth} of its keypoints have a disparity.",
           "Host wall time of the calls, each a replace in its own slot; the variants alternate in one process.", "",
           "| call | bytes uploaded besides the keypoints (MB) | median (ms) | min .. max (ms) | against chip_frame_put |", "|---|---|---|---|---|"]
    for k, label in (("put", "chip_frame_put (3-D image)"), ("s16", "chip_frame_put_disparity, CHIP_DISP_S16"), ("pair", "chip_frame_put_stereo (the pair)")):
        out.append(f"| {label} | {sz[k] / 1e6:.2f} | {med[k]:.3f} | {min(t[k]):.3f} .. {max(t[k]):.3f} | {med[k] / med['put']:.2f} |")
    gate = med["pair"] <= med["put"]
    out += ["", f"Condition (the stereo put's median must not exceed chip_frame_put's, same run): {med['pair']:.3f} <= {med['put']:.3f} ms: "
            + ("**met**." if gate else "**NOT met**."),
            f"The stereo put costs {med['pair'] - med['s16']:+.3f} ms over the int16 put of the same bytes.", "",
            f"chip_stereo_bm (upload {sz['pair'] / 1e6:.2f} MB, bm_prefilter, bm_dense, {sz['s16'] / 1e6:.2f} MB back into pageable memory): "
            f"median {med['dense']:.3f} ms, min .. max {min(t['dense']):.3f} .. {max(t['dense']):.3f}.", ""]
    # 2: the example's C++ timing, with the host restatement on the host CPU
    exe = ROOT / "cerebro_amd" / "lib" / "frame_put_stereo"
    if exe.exists():
        p = subprocess.run([str(exe), str(sz["n"]), "3", str(max(3, args.reps // 3))], capture_output=True, text=True, timeout=left())
        m = re.search(r"^timing .*$", p.stdout, flags=re.M)
        if p.returncode != 0 or not m:
            sys.exit("the example failed:\n" + p.stdout + p.stderr)
        out += ["The same calls from C++ (examples/frame_put_stereo.cc, one process, alternating), with the definition restated as a plain loop on the host CPU:", "",
                "    " + m.group(0), "",
                "That loop is this project's restatement with running sums, not OpenCV's implementation: no speed-up against cv::StereoBM follows "
                "from it.  cv::StereoBM on the target host: **not measured** (no machine of this project has OpenCV).", ""]
    else:
        out += ["The example binary is not built: host restatement **not measured**.", ""]
    # 3: kernel times, one rocprofv3 run of its own
    kt = {}
    if not args.no_trace and shutil.which("rocprofv3"):
        td = Path(args.trace_dir or tempfile.mkdtemp(prefix="frame_put_stereo_trace_"))
        td.mkdir(parents=True, exist_ok=True)
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(td), "-o", "fps", "--", sys.executable, __file__,
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
    # 4: the two unchanged calls against the parent commit's build
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
        out += ["", "The two unchanged calls on this tree and on a build of the parent commit, one process each, alternating (median, min .. max; ms):", "",
                "| build | chip_frame_put | chip_frame_put_disparity S16 |", "|---|---|---|"]
        out += [f"| {label} | {r['put'][0]:.3f} ({r['put'][1]:.3f} .. {r['put'][2]:.3f}) | {r['s16'][0]:.3f} ({r['s16'][1]:.3f} .. {r['s16'][2]:.3f}) |" for label, r in rows]
    text = "\n".join(out) + "\n"
    dst = Path(args.out)
    if dst.exists() and KEEP in dst.read_text():
        old = dst.read_text()
        text += "\n" + old[old.index(KEEP):]
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(text)
    print(text)
    if not gate:
        sys.exit("the stereo put is slower than chip_frame_put")


if __name__ == "__main__":
    main()
