#!/usr/bin/env python3
"""chip_frame_put_raw_orb_stereo and chip_rectify_pair on a 752 x 480 textured raw pair at the defaults, measured in one visit
-> profiles/rectify.md.

  python scripts/gpu_rectify.py [--reps 30] [--limit 420] [--out profiles/rectify.md] [--no-trace] [--parent-lib SO]

  1. host wall time, medians of --reps after warm-up, the variants ALTERNATING in one process: chip_frame_put_raw_orb_stereo (two-stage
     maps), chip_frame_put_orb_stereo on the pair already rectified, chip_rectify_pair, and the raw put with one-stage maps;
  2. examples/frame_put_raw_stereo with a repetition count: the same from C++, with the example's host restatement of the
     rectification (a plain loop, not OpenCV's implementation) alone and in front of chip_frame_put_orb_stereo;
  3. the kernel rectify_pair from one `rocprofv3 --kernel-trace --stats` run of its own: rounds of chip_rectify_pair with two-stage
     maps, then as many with one-stage maps;
  4. with --parent-lib: chip_frame_put_orb_stereo and chip_match_batch_stored at B = 8 of this tree and of that build of the parent
     commit, two child processes each, alternating: the guard that nothing that existed before has moved.
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
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from cerebro_amd import capi, synth  # noqa: E402

FULL = dict(n_true=4600, n_outlier_a=400, n_outlier_b=900, flip_rate=0.05, n_duplicates=60, n_border=48, seed=12)
WARMUP = 5
NEW = ("chip_build_has_rectify", "chip_rectify_quantize", "chip_remap", "chip_rectify_set_maps", "chip_rectify_pair", "chip_frame_put_raw_orb_stereo")
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


def calibration():
    """-> (left maps, right maps): x1, y1 a radial-tangential undistortion, x2, y2 the homography of a small rotation (tests/rectify_cases.py)"""
    import rectify_cases as RC
    return (RC.radtan(W, H) + RC.rotation(W, H, 0.004, -0.007, 0.009), RC.radtan(W, H, k1=-0.27, p1=-1e-4) + RC.rotation(W, H, -0.005, 0.006, -0.004))


def raw_pair(maps):
    """the textured pair warped through the mirrored maps, so that the calibration brings roughly the texture back"""
    import np_mirror_rectify as R
    import rectify_cases as RC
    gx, gy = RC.grid(W, H)
    inv = lambda m: ((2 * gx - m[0]).astype(np.float32), (2 * gy - m[1]).astype(np.float32))   # noqa: E731
    return tuple(R.rectify(img, *inv(m[2:]), *inv(m[:2])) for img, m in zip(pair(), maps))


def ok(st: int, what: str):
    if st != 0:
        sys.exit(f"{what} -> status {st}")


def rounds(reps: int, variants) -> tuple:
    """name -> times of the named calls, alternating in one process; variants: the new calls or those the parent has too"""
    Q = np.ascontiguousarray([1, 0, 0, -367.2, 0, 1, 0, -248.4, 0, 0, 0, 458.7, 0, 0, 1 / 0.11, 0], dtype=np.float64)
    n = capi.C.c_int32()
    p, C = capi._ptr, capi.C
    sc = synth.make_match_scene(**FULL)
    Kinv = np.ascontiguousarray(sc["Kinv"], np.float64)
    new = any(v in variants for v in ("put_raw", "rectify", "put_raw_one", "rectify_one"))
    left, right = pair()
    t = {v: [] for v in variants}
    with capi.Chip(4096) as chip:
        lib, h = chip.lib, chip.h
        chip.frame_store_reserve(B + 3, max(N, len(sc["a"]["kp"]), len(sc["b"]["kp"])))
        chip.frame_put(0, sc["a"])
        for j in range(B):
            chip.frame_put(1 + j, sc["b"])
        ids = list(range(1, B + 1))
        if new:
            maps = calibration()
            lraw, rraw = raw_pair(maps)
            two = [maps[0], maps[1]]
            one = [maps[0][:2], maps[1][:2]]
            chip.rectify_set_maps(*two)
            left, right = chip.rectify_pair(lraw, rraw)                # the pair already rectified
            lo, ro = np.zeros_like(lraw), np.zeros_like(rraw)
            state = dict(stages=2)

            def want(stages):                                          # (not timed) the one-stage variants swap the maps in and out
                if state["stages"] != stages:
                    chip.rectify_set_maps(*(two if stages == 2 else one))
                    state["stages"] = stages

            def put_raw():
                ok(lib.chip_frame_put_raw_orb_stereo(h, 100, W, H, p(lraw), p(rraw), None, None, p(Q), C.byref(n)), "chip_frame_put_raw_orb_stereo")

            def rectify():
                ok(lib.chip_rectify_pair(h, p(lraw), p(rraw), W, H, p(lo), p(ro)), "chip_rectify_pair")

        def put_orb():
            ok(lib.chip_frame_put_orb_stereo(h, 101, W, H, p(left), p(right), None, None, p(Q), C.byref(n)), "chip_frame_put_orb_stereo")

        calls = dict(put_orb=put_orb, stored=lambda: chip.match_batch_stored(0, ids, Kinv))
        if new:
            calls.update(put_raw=put_raw, rectify=rectify, put_raw_one=put_raw, rectify_one=rectify)
        for r in range(WARMUP + reps):
            for v in variants:
                if new:
                    want(1 if v.endswith("_one") else 2)
                x = ms(calls[v])
                if r >= WARMUP:
                    t[v].append(x)
        arch = chip.info()["arch"]
    return arch, t, n.value


def kernel_times(trace_dir: Path) -> list:
    """the durations (us) of rectify_pair in launch order"""
    rows = []
    for path in trace_dir.rglob("*kernel_trace.csv"):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                if re.search(r"\brectify_pair\b", row.get("Kernel_Name", "")):
                    rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    return [d for _, d in sorted(rows)]


def fmt(v) -> str:
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rectify.md"))
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
        _, t, _ = rounds(args.reps, ("put_orb", "stored"))
        print("JSON " + json.dumps({k: [statistics.median(v), min(v), max(v)] for k, v in t.items()}))
        return
    if args.child:                                                   # all two-stage launches, then all one-stage launches
        rounds(args.reps, ("rectify",))
        rounds(args.reps, ("rectify_one",))
        return
    arch, t, n = rounds(args.reps, ("put_raw", "put_orb", "rectify", "put_raw_one", "rectify_one"))
    px = W * H
    out = [f"# Rectification on the device: 752 x 480 at the defaults ({arch}, medians of {args.reps} after {WARMUP} warm-up rounds, scripts/gpu_rectify.py)", "",
           f"Raw pair: the synthetic textured {W} x {H} frame of tests/orb_detect_cases.py (the right image: the same, 16 columns on) warped through the "
           f"mirrored calibration; maps: a radial-tangential undistortion and the homography of a small rotation per eye (tests/rectify_cases.py), "
           f"{32 * px} bytes on the device for two stages; n_features 5000, 8 levels, FAST threshold 0, border 31; n = {n}.  Host wall time, the "
           "variants alternating in one process (median, min .. max; ms):", "",
           "| call | ms |", "|---|---|",
           f"| `chip_frame_put_raw_orb_stereo`, two stages ({2 * px} bytes up, 32 bytes back) | {fmt(t['put_raw'])} |",
           f"| `chip_frame_put_orb_stereo` on the pair already rectified ({2 * px} bytes up, 32 bytes back) | {fmt(t['put_orb'])} |",
           f"| `chip_frame_put_raw_orb_stereo`, one stage | {fmt(t['put_raw_one'])} |",
           f"| `chip_rectify_pair`, two stages ({2 * px} bytes up, {2 * px} back) | {fmt(t['rectify'])} |",
           f"| `chip_rectify_pair`, one stage | {fmt(t['rectify_one'])} |", "",
           f"The price of rectification on the device: {statistics.median(t['put_raw']) - statistics.median(t['put_orb']):.3f} ms per frame (difference "
           "of the first two medians).", ""]
    exe = ROOT / "cerebro_amd" / "lib" / "frame_put_raw_stereo"
    if exe.exists():
        p = subprocess.run([str(exe), str(N), "3", str(args.reps)], capture_output=True, text=True, timeout=left())
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        if p.returncode != 0 or not lines:
            sys.exit("the example failed:\n" + p.stdout + p.stderr)
        out += ["The same from C++ (examples/frame_put_raw_stereo.cc, one process, alternating), with the rectification restated as a plain loop on the host CPU:", ""]
        out += ["    " + l for l in lines]
        out += ["", "That loop is this project's restatement, a plain loop, not OpenCV's implementation: no speed-up against cv::remap follows from it."]
    else:
        out += ["The example binary is not built: host restatement **not measured**."]
    out += ["cv::remap on the target host: **not measured** (no OpenCV on it).", ""]
    kt = []
    if not args.no_trace and shutil.which("rocprofv3"):
        td = Path(tempfile.mkdtemp(prefix="rectify_trace_"))
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(td), "-o", "rectify", "--", sys.executable, __file__,
                            "--child", "--reps", str(args.reps), "--limit", str(left())], capture_output=True, text=True, timeout=left())
        if p.returncode != 0:
            sys.exit("the traced child failed:\n" + p.stdout[-2000:] + p.stderr[-2000:])
        kt = kernel_times(td)
        shutil.rmtree(td, ignore_errors=True)
    per = WARMUP + args.reps + 1                                     # + 1: the launch that makes the rectified pair of put_orb
    if len(kt) == 2 * per:
        two, one = kt[1 + WARMUP:per], kt[per + 1 + WARMUP:]
        out += ["Kernel (`rocprofv3 --kernel-trace --stats`, a run of its own: rounds of `chip_rectify_pair` with two-stage maps, then with one-stage maps; us):", "",
                "| kernel | launches | median | min |", "|---|---|---|---|",
                f"| `rectify_pair`, two stages, both eyes | {len(two)} | {statistics.median(two):.1f} | {min(two):.1f} |",
                f"| `rectify_pair`, one stage, both eyes | {len(one)} | {statistics.median(one):.1f} | {min(one):.1f} |"]
    else:
        out += [f"Kernel times: **not measured** ({len(kt)} launches of rectify_pair in the trace, {2 * per} expected)."]
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
                f"chip_frame_put_orb_stereo on the textured pair, chip_match_batch_stored at B = {B} on the frames of profiles/match_store.md):", "",
                "| build | chip_frame_put_orb_stereo | chip_match_batch_stored |", "|---|---|---|"]
        out += ["| " + label + " | " + " | ".join(f"{r[k][0]:.3f} ({r[k][1]:.3f} .. {r[k][2]:.3f})" for k in ("put_orb", "stored")) + " |" for label, r in rows]
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
