#!/usr/bin/env python3
"""Measures chip_match_batch_stored_modes (GMS with scale / rotation) against chip_match_batch_stored, the plain filter and the yardstick
(profiles/gms_modes.md holds this script's output).

  python scripts/gpu_gms_modes_perf.py [--reps 30] [--limit 420] [--out profiles/gms_modes.md]

On the frames profiles/match_store.md was measured on (full_5000_5000: 5000 / 5323 keypoints at 752 x 480, the candidate stored under B
ids), B = 1 / 4 / 8 / 16:
  1. ONE process times the plain call and the modes call at modes = 1, 2, 3 at every B: 5 warm-up calls each, then --reps rounds in which
     the four calls ALTERNATE; medians;
  2. per (B, modes), a child process with CHIP_MATCH_BATCH_TIMING=1 (the knob is read once per process) repeats the alternation of the
     plain call and that modes call: at exit the library prints the device time of each kernel by events, for the plain runs
     (hamming_match_split, gms_batch, pose_sets_stored_batch) and for the modes runs (gms_grid_modes + gms_mode_select in gms_batch's place).
The yardstick of a row is gms_batch IN THE SAME CHILD.  Every call's status is checked; the first failing one ends the script.  The
script runs under a time limit of its own: --limit seconds for the whole run (an alarm ends the process and its children)."""
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
MODES = (1, 2, 3)
WARMUP = 5
TABLE_AREA = {1: 3080 / 400, 2: 1.0, 3: 3080 / 400}                  # summed table columns over plain's 400


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def prepare(chip, sc, B: int):
    """-> call(modes): the stored call (modes 0: chip_match_batch_stored) as a raw ctypes call on frames put once"""
    fa, keep_a = chip._match_frame(sc["a"])
    fb1, keep_b = chip._match_frame(sc["b"])
    Ki = np.ascontiguousarray(sc["Kinv"], dtype=np.float64).reshape(9)
    sm, ch = (capi.MatchSummary * B)(), (capi.GmsChoice * B)()
    ids = np.arange(B, dtype=np.int64)
    lib, h = chip.lib, chip.h

    def check(st, what):
        if st != 0:
            sys.exit(f"{what} -> status {st}")

    check(lib.chip_frame_put(h, 1000, C.byref(fa)), "chip_frame_put")
    for j in range(B):
        check(lib.chip_frame_put(h, j, C.byref(fb1)), "chip_frame_put")

    def call(modes: int):
        if modes:
            check(lib.chip_match_batch_stored_modes(h, 1000, capi._ptr(ids), B, capi._ptr(Ki), modes, sm, ch), "chip_match_batch_stored_modes")
        else:
            check(lib.chip_match_batch_stored(h, 1000, capi._ptr(ids), B, capi._ptr(Ki), sm), "chip_match_batch_stored")
        return sm[0].n_matches_gms

    return call, (keep_a, keep_b, Ki, ids, fa, fb1)


def rounds(call, which, reps: int):
    for m in which:
        for _ in range(WARMUP):
            call(m)
    t = {m: [] for m in which}
    for _ in range(reps):                                            # the calls alternate inside the timed window
        for m in which:
            t[m].append(ms(lambda: call(m)))
    return {m: statistics.median(v) for m, v in t.items()}


def child(B: int, modes: int, reps: int):
    sc = synth.make_match_scene(**FULL)
    with capi.Chip(4096) as chip:
        chip.frame_store_reserve(max(BS) + 1, len(sc["b"]["kp"]))
        call, keep = prepare(chip, sc, B)
        t = rounds(call, (0, modes), reps)
    print(f"child B={B} modes={modes} plain {t[0]:.4f} with {t[modes]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gms_modes.md"))
    ap.add_argument("--limit", type=int, default=420, help="seconds the whole run may take")
    ap.add_argument("--child", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return
    assert args.reps >= 20
    sc = synth.make_match_scene(**FULL)
    n1, n2 = len(sc["a"]["kp"]), len(sc["b"]["kp"])
    calls, kept = {}, {}
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        chip.frame_store_reserve(max(BS) + 1, max(n1, n2))
        for B in BS:
            call, keep = prepare(chip, sc, B)
            kept[B] = {m: call(m) for m in (0,) + MODES}
            calls[B] = rounds(call, (0,) + MODES, args.reps)
    kern = {}
    for B in BS:
        for m in MODES:
            env = dict(os.environ, CHIP_MATCH_BATCH_TIMING="1")
            left = max(1, int(deadline - time.monotonic()))
            p = subprocess.run([sys.executable, __file__, "--child", str(B), str(m), "--reps", str(args.reps), "--limit", str(left)], env=env,
                               capture_output=True, text=True, timeout=left)
            kp = re.search(r"match batch stored kernel timing over \d+ calls \(us\): hamming_match_split ([\d.]+), gms_batch ([\d.]+), "
                           r"pose_sets_stored_batch ([\d.]+)", p.stderr)
            km = re.search(r"match batch stored modes kernel timing over \d+ calls \(us\): hamming_match_split ([\d.]+), gms_grid_modes ([\d.]+), "
                           r"gms_mode_select ([\d.]+), pose_sets_stored_batch ([\d.]+)", p.stderr)
            if p.returncode != 0 or not (kp and km):
                sys.exit("child failed:\n" + p.stdout + p.stderr)
            kern[B, m] = ([float(x) for x in kp.groups()], [float(x) for x in km.groups()])
    out = [f"# GMS with scale / rotation against the plain filter ({arch}, medians of {args.reps} after {WARMUP} warm-up calls, scripts/gpu_gms_modes_perf.py)", "",
           f"Frames: {n1} / {n2} keypoints at 752 x 480 (full_5000_5000, the frames of profiles/match_store.md), the candidate stored under B ids.",
           "Host wall time of chip_match_batch_stored (plain) and chip_match_batch_stored_modes; the four calls alternate in one process.",
           f"GMS survivors of the candidate: plain {kept[1][0]}, modes 1 / 2 / 3: {kept[1][1]} / {kept[1][2]} / {kept[1][3]}.", "",
           "| B | plain (ms) | modes = 1, scale (ms) | modes = 2, rotation (ms) | modes = 3, both (ms) | ratios to plain |", "|---|---|---|---|---|---|"]
    for B in BS:
        t = calls[B]
        out.append(f"| {B} | {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} | {t[3]:.3f} | {t[1] / t[0]:.2f} / {t[2] / t[0]:.2f} / {t[3] / t[0]:.2f} |")
    out += ["", "Kernels by events (us; a process per (B, modes) with CHIP_MATCH_BATCH_TIMING=1 alternating the plain and the modes call; averages over its",
            "calls of each kind).  The yardstick is gms_batch in the same process:", "",
            "| B | modes | gms_batch (plain) | gms_grid_modes | gms_mode_select | (grid + select) / gms_batch | hamming_match_split | pose_sets_stored_batch |",
            "|---|---|---|---|---|---|---|---|"]
    ratio = {}
    for B in BS:
        for m in MODES:
            kp, km = kern[B, m]
            ratio[B, m] = (km[1] + km[2]) / kp[1]
            out.append(f"| {B} | {m} | {kp[1]:.1f} | {km[1]:.1f} | {km[2]:.1f} | {ratio[B, m]:.2f} | {km[0]:.1f} | {km[3]:.1f} |")
    out += ["", "Against what the structure predicts (B = 8):", ""]
    for m, bound, why in ((2, 2.0, "only the score step grows"), (3, 7.7, "the summed table area of the five scales")):
        r = ratio[8, m]
        out.append(f"- modes = {m}: {r:.2f} x gms_batch (bound {bound} x: {why}): {'within' if r <= bound else 'ABOVE -- see the split above'};")
    out.append(f"- modes = 1: {ratio[8, 1]:.2f} x gms_batch.")
    text = "\n".join(out) + "\n"
    dst = Path(args.out)
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
