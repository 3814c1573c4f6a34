#!/usr/bin/env python3
"""Measures chip_match_batch_stored (frames kept on the device) against chip_match_batch on host frames, the parent's unchanged path and
the yardstick, and chip_frame_put alone (profiles/match_store.md holds this script's output).

  python scripts/gpu_match_store_perf.py [--reps 30] [--limit 280] [--out profiles/match_store.md]

On the 5000 / 5323-keypoint frames at 752 x 480 of profiles/match_batch.md (full_5000_5000), B = 1 / 4 / 8 / 16, the B candidates being
the scene's b frame put under B ids:
  1. ONE process times the three calls at every B: 5 warm-up calls, then --reps rounds in which the host-frame call and the stored call
     ALTERNATE; medians.  chip_frame_put (one 5323-keypoint frame, a replace in its own slot) is timed the same way;
  2. per B, a child process with CHIP_MATCH_BATCH_TIMING=1 (the knob is read once per process) repeats the alternating rounds: at exit the
     library prints the device time of the three kernels by events, for the host-frame runs and for the stored runs of THAT process, and
     the child reports its own call medians next to them (the event records are inside its calls).
Every call's status is checked; the first failing one ends the script.  The script runs under a time limit of its own: --limit seconds
for the whole run (an alarm ends the process; the children, which get what is left of it, are ended with it).  A section of the output file that starts with the line "# Code objects" is kept as it is."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import signal
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from cerebro_amd import capi, synth  # noqa: E402

FULL = dict(n_true=4600, n_outlier_a=400, n_outlier_b=900, flip_rate=0.05, n_duplicates=60, n_border=48, seed=12)
BS = (1, 4, 8, 16)
WARMUP = 5
KEEP = "# Code objects"


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def prepare(chip, sc, B: int):
    """the three calls as raw ctypes calls on frames prepared once; the query is stored under id 1000, the candidate under ids 0 .. B - 1"""
    fa, keep_a = chip._match_frame(sc["a"])
    fb1, keep_b = chip._match_frame(sc["b"])
    fb = (capi.MatchFrame * B)(*([fb1] * B))
    Ki = np.ascontiguousarray(sc["Kinv"], dtype=np.float64).reshape(9)
    sm_h, sm_s = (capi.MatchSummary * B)(), (capi.MatchSummary * B)()
    ids = np.arange(B, dtype=np.int64)
    lib, h = chip.lib, chip.h

    def check(st, what):
        if st != 0:
            sys.exit(f"{what} -> status {st}")

    check(lib.chip_frame_put(h, 1000, C.byref(fa)), "chip_frame_put")
    for j in range(B):
        check(lib.chip_frame_put(h, j, C.byref(fb1)), "chip_frame_put")

    def host():
        check(lib.chip_match_batch(h, C.byref(fa), fb, B, capi._ptr(Ki), sm_h), "chip_match_batch")

    def stored():
        check(lib.chip_match_batch_stored(h, 1000, capi._ptr(ids), B, capi._ptr(Ki), sm_s), "chip_match_batch_stored")

    def put():
        check(lib.chip_frame_put(h, 0, C.byref(fb1)), "chip_frame_put")

    def same():
        if bytes(sm_h) != bytes(sm_s):
            sys.exit(f"B = {B}: the summaries of the two paths differ")

    return host, stored, put, same, (keep_a, keep_b, Ki, ids, fb, fa)


def rounds(host, stored, put, same, reps: int):
    for _ in range(WARMUP):
        host(); stored(); put()
    th, ts, tp = [], [], []
    for _ in range(reps):                                            # the two paths alternate inside the timed window
        th.append(ms(host)); ts.append(ms(stored))
    same()
    for _ in range(reps):
        tp.append(ms(put))
    return statistics.median(th), statistics.median(ts), statistics.median(tp)


def child(B: int, reps: int):
    sc = synth.make_match_scene(**FULL)
    with capi.Chip(4096) as chip:
        chip.frame_store_reserve(max(BS) + 1, len(sc["b"]["kp"]))
        host, stored, put, same, keep = prepare(chip, sc, B)
        th, ts, _ = rounds(host, stored, put, same, reps)
    print(f"child B={B} host {th:.4f} stored {ts:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "match_store.md"))
    ap.add_argument("--limit", type=int, default=280, help="seconds the whole run may take")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    if args.child:
        child(args.child, args.reps)
        return
    assert args.reps >= 20
    sc = synth.make_match_scene(**FULL)
    n1, n2 = len(sc["a"]["kp"]), len(sc["b"]["kp"])
    rows = []
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        chip.frame_store_reserve(max(BS) + 1, max(n1, n2))
        for B in BS:
            host, stored, put, same, keep = prepare(chip, sc, B)
            rows.append([B, *rounds(host, stored, put, same, args.reps)])
    for r in rows:
        env = dict(os.environ, CHIP_MATCH_BATCH_TIMING="1")
        p = subprocess.run([sys.executable, __file__, "--child", str(r[0]), "--reps", str(args.reps), "--limit", str(max(1, int(deadline - time.monotonic())))],
                           env=env, capture_output=True, text=True, timeout=max(1.0, deadline - time.monotonic()))
        mh = re.search(r"match batch kernel timing over (\d+) calls \(us\): hamming_match_split ([\d.]+), gms_batch ([\d.]+), pose_sets_batch ([\d.]+)", p.stderr)
        ms_ = re.search(r"match batch stored kernel timing over (\d+) calls \(us\): hamming_match_split ([\d.]+), gms_batch ([\d.]+), pose_sets_stored_batch ([\d.]+)", p.stderr)
        mc = re.search(r"child B=\d+ host ([\d.]+) stored ([\d.]+)", p.stdout)
        if p.returncode != 0 or not (mh and ms_ and mc):
            sys.exit("child failed:\n" + p.stdout + p.stderr)
        r += [[float(x) for x in mh.groups()[1:]], [float(x) for x in ms_.groups()[1:]], float(mc.group(1)), float(mc.group(2))]
    out = [f"# chip_match_batch_stored against chip_match_batch on host frames ({arch}, medians of {args.reps} after {WARMUP} warm-up calls, scripts/gpu_match_store_perf.py)", "",
           f"Frames: {n1} / {n2} keypoints at 752 x 480 (full_5000_5000), the candidate stored under B ids.  Host wall time of the calls; the two paths",
           "alternate in one process.  chip_frame_put: one candidate frame (descriptors, keypoints, the 4.33 MB image, frame_gather), a replace.", "",
           "| B | chip_match_batch, host frames (ms) | chip_match_batch_stored (ms) | ratio | chip_frame_put (ms) |", "|---|---|---|---|---|"]
    for B, th, ts, tp, *_ in rows:
        out.append(f"| {B} | {th:.3f} | {ts:.3f} | {th / ts:.2f} | {tp:.3f} |")
    out += ["", "Kernels by events (us; a process per B with CHIP_MATCH_BATCH_TIMING=1, averages over its calls of each path) and that process's own call medians",
            "(the event records and reads are inside them):", "",
            "| B | path | hamming_match_split | gms_batch | pose_sets_batch / pose_sets_stored_batch | sum (us) | call in that process (ms) | call / sum |", "|---|---|---|---|---|---|---|---|"]
    for B, th, ts, tp, kh, ks, ch, cs in rows:
        out.append(f"| {B} | host frames | {kh[0]:.1f} | {kh[1]:.1f} | {kh[2]:.1f} | {sum(kh):.1f} | {ch:.3f} | {1e3 * ch / sum(kh):.2f} |")
        out.append(f"| {B} | stored | {ks[0]:.1f} | {ks[1]:.1f} | {ks[2]:.1f} | {sum(ks):.1f} | {cs:.3f} | {1e3 * cs / sum(ks):.2f} |")
    ok_le = all(ts <= th for _, th, ts, *_ in rows)
    (r8,) = [r for r in rows if r[0] == 8]
    ksum = sum(r8[5])
    over = 1e3 * r8[2] / ksum - 1.0
    out += ["", "Acceptance:", "",
            f"- the stored call's median is no larger than the host-frame call's at every B: {'yes' if ok_le else 'NO'};",
            f"- B = 8: stored call {1e3 * r8[2]:.1f} us (first table) against the kernel sum {ksum:.1f} us of the stored path: {100 * over:+.1f} % "
            f"(bound: within 25 %): {'met' if over <= 0.25 else 'MISSED'}."]
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
