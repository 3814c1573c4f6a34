#!/usr/bin/env python3
"""Measures chip_match_batch against sequential chip_match_pair calls of the same build (profiles/match_batch.md holds this script's
output, one section per visit; to compare two builds run it from each tree in turn with --out).

  python scripts/gpu_match_batch_perf.py [--reps 30] [--out profiles/match_batch.md]

On 5000 / 5000-keypoint frames at 752 x 480 (the full_5000_5000 scene of tests/test_match_gpu.py), in one process per row, warm-up first,
medians of --reps runs:
  1. chip_match_batch at B = 1, 4, 8, 16 against B sequential chip_match_pair calls (raw ctypes calls on frames prepared once; the B
     candidates are the scene's b frame B times -- the work does not depend on which candidate it is);
  2. the three kernels alone by hipEvents (CHIP_MATCH_BATCH_TIMING=1, a child process per B: the knob is read once);
  3. the whole verification, verify_candidates against B x verify_candidate (examples/verify_candidates.cc on its own 5000-point scene:
     B - 2 views that pass, one unrelated and one empty candidate);
  4. chip_orb_match alone on the same descriptors."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
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


def median_ms(fn, reps: int) -> float:
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t)


def prepare(chip, sc, B: int):
    fa, keep_a = chip._match_frame(sc["a"])
    fb1, keep_b = chip._match_frame(sc["b"])
    fb = (capi.MatchFrame * B)(*([fb1] * B))
    Ki = np.ascontiguousarray(sc["Kinv"], dtype=np.float64).reshape(9)
    sm = (capi.MatchSummary * B)()
    lib, h = chip.lib, chip.h

    def batch():
        assert lib.chip_match_batch(h, C.byref(fa), fb, B, capi._ptr(Ki), sm) == 0

    def pairs():
        for j in range(B):
            assert lib.chip_match_pair(h, C.byref(fa), C.byref(fb[j]), capi._ptr(Ki), C.byref(sm[j])) == 0

    return batch, pairs, (keep_a, keep_b, Ki, sm, fb, fa)


def kernels_child(B: int, reps: int):
    sc = synth.make_match_scene(**FULL)
    with capi.Chip(4096) as chip:
        batch, _, keep = prepare(chip, sc, B)
        for _ in range(reps + 3):
            batch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "match_batch.md"))
    ap.add_argument("--kernels-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        kernels_child(args.kernels_child, args.reps)
        return
    assert args.reps >= 20
    sc = synth.make_match_scene(**FULL)
    n1, n2 = len(sc["a"]["kp"]), len(sc["b"]["kp"])
    rows = []
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        for B in BS:
            batch, pairs, keep = prepare(chip, sc, B)
            for _ in range(3):
                batch(); pairs()
            tp, tb = [], []
            for _ in range(args.reps):                               # the two paths alternate inside the timed window
                tp.append(median_ms(pairs, 1)); tb.append(median_ms(batch, 1))
            rows.append([B, statistics.median(tp), statistics.median(tb)])
        d1, d2 = (np.ascontiguousarray(sc[k]["desc"], dtype=np.uint8) for k in "ab")
        idx, dist = np.empty(n1, np.int32), np.empty(n1, np.int32)

        def orb():
            assert chip.lib.chip_orb_match(chip.h, capi._ptr(d1), n1, capi._ptr(d2), n2, capi._ptr(idx), capi._ptr(dist)) == 0

        for _ in range(3):
            orb()
        t_orb = median_ms(orb, args.reps)
    for r in rows:
        env = dict(os.environ, CHIP_MATCH_BATCH_TIMING="1")
        p = subprocess.run([sys.executable, __file__, "--kernels-child", str(r[0]), "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=600)
        m = re.search(r"hamming_match_split ([\d.]+), gms_batch ([\d.]+), pose_sets_batch ([\d.]+)", p.stderr)
        assert p.returncode == 0 and m, p.stdout + p.stderr
        r += [float(x) for x in m.groups()]
    exe = ROOT / "cerebro_amd" / "lib" / "verify_candidates"
    whole = []
    for B in (4, 8, 16):
        p = subprocess.run([str(exe), "5000", str(B), str(args.reps)], capture_output=True, text=True, timeout=600)
        m = re.search(r"timing B=(\d+) n=(\d+) reps=\d+: \d+ x verify_candidate ([\d.]+) ms, verify_candidates ([\d.]+) ms", p.stdout)
        assert p.returncode == 0 and m, p.stdout + p.stderr
        whole.append((B, int(m.group(2)), float(m.group(3)), float(m.group(4))))
    out = [f"# chip_match_batch against sequential chip_match_pair calls ({arch}, medians of {args.reps}, scripts/gpu_match_batch_perf.py)", "",
           f"Frames: {n1} / {n2} keypoints at 752 x 480 (full_5000_5000).  Host wall time of the calls, uploads included; kernel columns: device time by events.", "",
           "| B | B x chip_match_pair (ms) | chip_match_batch (ms) | ratio | hamming_match_split (us) | gms_batch (us) | pose_sets_batch (us) |",
           "|---|---|---|---|---|---|---|"]
    for B, tp, tb, k0, k1, k2 in rows:
        out.append(f"| {B} | {tp:.3f} | {tb:.3f} | {tp / tb:.2f} | {k0:.1f} | {k1:.1f} | {k2:.1f} |")
    out += ["", "Whole verification (examples/verify_candidates, its own scene: B - 2 views that pass all gates, one unrelated and one empty candidate):", "",
            "| B | keypoints of the query | B x verify_candidate (ms) | verify_candidates (ms) | ratio |", "|---|---|---|---|---|"]
    for B, n, t1, tb in whole:
        out.append(f"| {B} | {n} | {t1:.3f} | {tb:.3f} | {t1 / tb:.2f} |")
    out += ["", f"chip_orb_match alone, {n1} x {n2} descriptors: {t_orb:.3f} ms"]
    text = "\n".join(out) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
