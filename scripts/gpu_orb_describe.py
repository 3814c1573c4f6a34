#!/usr/bin/env python3
"""chip_orb_detect_describe and chip_frame_put_orb_stereo on the 752 x 480 textured frame at the defaults, measured in one visit
-> profiles/orb_describe.md.

  python scripts/gpu_orb_describe.py [--reps 30] [--limit 420] [--out profiles/orb_describe.md] [--no-trace] [--parent-lib SO]

  1. host wall time, medians of --reps after warm-up, the variants ALTERNATING in one process: chip_orb_detect, chip_orb_detect_describe,
     chip_frame_put_orb_stereo, and the same put composed on the host (chip_orb_detect_describe, then chip_frame_put_stereo with the
     records' (x, y): its copy down and up again included);
  2. examples/orb_frame_put with a repetition count: the two puts from C++ and the example's host restatement of blur + descriptor (a
     plain loop, not OpenCV's implementation);
  3. the kernels orb_blur and orb_describe from one `rocprofv3 --kernel-trace --stats` run of its own over the same rounds;
  4. with --parent-lib: chip_orb_detect, chip_frame_put_stereo and chip_match_batch_stored at B = 8 of this tree and of that build of the
     parent commit, two child processes each, alternating: the guard that nothing that existed before has moved.
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
KERNELS = ("orb_moments", "orb_blur", "orb_describe", "bm_prefilter", "bm_keypoints")
NEW = ("chip_build_has_orb_describe", "chip_orb_bin", "chip_orb_pattern", "chip_orb_detect_describe", "chip_debug_orb_blur", "chip_frame_put_orb_stereo")
KEEP = "# What the figures say"
W, H, B, N = 752, 480, 8, 5000


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def pair():
    """blocks of 5 pixels of random brightness under pixel noise (tests/orb_detect_cases.py: texture) and the same 16 columns on"""
    rng = np.random.default_rng(752480)
    blocks = rng.integers(30, 226, ((H + 4) // 5, (W + 4) // 5))
    img = np.repeat(np.repeat(blocks, 5, 0), 5, 1)[:H, :W] + rng.integers(-25, 26, (H, W))
    left = np.clip(img, 0, 255).astype(np.uint8)
    return left, np.ascontiguousarray(np.roll(left, -16, axis=1))


def ok(st: int, what: str):
    if st != 0:
        sys.exit(f"{what} -> status {st}")


def rounds(reps: int, variants) -> dict:
    """name -> times of the named calls, alternating in one process; variants: the new calls or those the parent has too"""
    left, right = pair()
    Q = np.ascontiguousarray([1, 0, 0, -367.2, 0, 1, 0, -248.4, 0, 0, 0, 458.7, 0, 0, 1 / 0.11, 0], dtype=np.float64)
    kp = np.zeros(N, capi.ORB_KEYPOINT_DTYPE)
    desc = np.zeros((N, 32), np.uint8)
    n = capi.C.c_int32()
    p, C = capi._ptr, capi.C
    sc = synth.make_match_scene(**FULL)
    Kinv = np.ascontiguousarray(sc["Kinv"], np.float64)
    t = {v: [] for v in variants}
    with capi.Chip(4096) as chip:
        lib, h = chip.lib, chip.h
        chip.frame_store_reserve(B + 3, max(N, len(sc["a"]["kp"]), len(sc["b"]["kp"])))
        chip.frame_put(0, sc["a"])
        for j in range(B):
            chip.frame_put(1 + j, sc["b"])
        ids = list(range(1, B + 1))

        def detect():
            ok(lib.chip_orb_detect(h, p(left), W, H, None, p(kp), N, C.byref(n), None), "chip_orb_detect")

        def describe():
            ok(lib.chip_orb_detect_describe(h, p(left), W, H, None, p(kp), N, C.byref(n), None, p(desc)), "chip_orb_detect_describe")

        def put_stereo():
            xy = np.ascontiguousarray(np.stack([kp["x"][:n.value], kp["y"][:n.value]], axis=1), dtype=np.float32)
            ok(lib.chip_frame_put_stereo(h, 101, p(desc), p(xy), n.value, W, H, p(left), p(right), None, p(Q)), "chip_frame_put_stereo")

        def put_orb():
            ok(lib.chip_frame_put_orb_stereo(h, 100, W, H, p(left), p(right), None, None, p(Q), C.byref(n)), "chip_frame_put_orb_stereo")

        def composed():
            describe()
            put_stereo()

        calls = dict(detect=detect, describe=describe, put_orb=put_orb, composed=composed, put_stereo=put_stereo,
                     stored=lambda: chip.match_batch_stored(0, ids, Kinv))
        if "put_stereo" in variants and "describe" not in variants:        # the parent: random descriptors at the detector's keypoints
            detect()
            desc[:] = np.random.default_rng(1).integers(0, 256, desc.shape)
        for r in range(WARMUP + reps):
            for v in variants:
                x = ms(calls[v])
                if r >= WARMUP:
                    t[v].append(x)
    return chip_arch(), t, n.value


def chip_arch() -> str:
    with capi.Chip(4096) as c:
        return c.info()["arch"]


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


def fmt(v) -> str:
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "orb_describe.md"))
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
            for name in NEW:
                capi._SIGS.pop(name, None)
        _, t, _ = rounds(args.reps, ("detect", "put_stereo", "stored"))
        print("JSON " + json.dumps({k: [statistics.median(v), min(v), max(v)] for k, v in t.items()}))
        return
    if args.child:
        rounds(args.reps, ("describe", "put_orb"))
        return
    arch, t, n = rounds(args.reps, ("detect", "describe", "put_orb", "composed"))
    out = [f"# ORB descriptors on the device: 752 x 480 at the defaults ({arch}, medians of {args.reps} after {WARMUP} warm-up rounds, scripts/gpu_orb_describe.py)", "",
           f"Frame: the synthetic textured {W} x {H} frame of tests/orb_detect_cases.py (the right image: the same, 16 columns on); n_features 5000, "
           f"8 levels, FAST threshold 0, border 31; n = {n}.  Host wall time, the four variants alternating in one process (median, min .. max; ms):", "",
           "| call | ms |", "|---|---|",
           f"| `chip_orb_detect` ({32 + 32 * N} bytes back) | {fmt(t['detect'])} |",
           f"| `chip_orb_detect_describe` (+ orb_blur, orb_describe, {32 * N} bytes more back) | {fmt(t['describe'])} |",
           f"| `chip_frame_put_orb_stereo` ({2 * W * H} bytes up, 32 bytes back) | {fmt(t['put_orb'])} |",
           f"| composed: `chip_orb_detect_describe`, then `chip_frame_put_stereo` ({3 * W * H + 40 * N} bytes up, {32 + 64 * N} back) | {fmt(t['composed'])} |", ""]
    exe = ROOT / "cerebro_amd" / "lib" / "orb_frame_put"
    if exe.exists():
        p = subprocess.run([str(exe), str(N), "3", str(max(3, args.reps // 3))], capture_output=True, text=True, timeout=left())
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        if p.returncode != 0 or not lines:
            sys.exit("the example failed:\n" + p.stdout + p.stderr)
        out += ["The same from C++ (examples/orb_frame_put.cc, one process, alternating), with the descriptor restated as a plain loop on the host CPU:", ""]
        out += ["    " + l for l in lines]
        out += ["", "That loop is this project's restatement, a plain loop, not OpenCV's implementation: no speed-up against cv::ORB::compute follows from it."]
    else:
        out += ["The example binary is not built: host restatement **not measured**."]
    try:
        import cv2  # noqa: F401
        out += ["cv::ORB::compute: OpenCV exists on this host but makes other bits; **not measured** here."]
    except ImportError:
        out += ["cv::ORB::compute on the target host: **not measured** (no OpenCV on it)."]
    out += [""]
    kt = {}
    if not args.no_trace and shutil.which("rocprofv3"):
        td = Path(tempfile.mkdtemp(prefix="orb_describe_trace_"))
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(td), "-o", "orb", "--", sys.executable, __file__,
                            "--child", "--reps", str(args.reps), "--limit", str(left())], capture_output=True, text=True, timeout=left())
        if p.returncode != 0:
            sys.exit("the traced child failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
        kt = kernel_times(td)
        shutil.rmtree(td, ignore_errors=True)
    if kt:
        out += ["Kernels (`rocprofv3 --kernel-trace --stats`, a run of its own over the rounds of the two describing calls; us):", "",
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
        out += ["", f"The guard: calls that existed before, on this tree and on a build of the parent commit, one process each, alternating (median, min .. max; ms; "
                f"chip_frame_put_stereo with {N} keypoints, chip_match_batch_stored at B = {B} on the frames of profiles/match_store.md):", "",
                "| build | chip_orb_detect | chip_frame_put_stereo | chip_match_batch_stored |", "|---|---|---|---|"]
        out += ["| " + label + " | " + " | ".join(f"{r[k][0]:.3f} ({r[k][1]:.3f} .. {r[k][2]:.3f})" for k in ("detect", "put_stereo", "stored")) + " |" for label, r in rows]
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
