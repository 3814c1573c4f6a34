#!/usr/bin/env python3
"""Measures chip_match_pairs_stored (a list of (query, candidate) pairs, every pair with a query frame of its own) against the loop of
chip_match_batch_stored calls with B = 1 that it replaces and against chip_match_batch_stored with one shared query frame
(profiles/match_pairs.md holds this script's output).

  python scripts/gpu_match_pairs_perf.py [--reps 30] [--limit 420] [--parent-lib PATH] [--out profiles/match_pairs.md]

On the 5000 / 5323-keypoint frames at 752 x 480 of profiles/match_store.md (full_5000_5000).  The store holds 16 query frames (the
scene's a frame with its keypoints rolled by another amount per copy: distinct slots, distinct order, the same work) and 16 candidates
(the scene's b frame under 16 ids):
  1. ONE process times, at P = 1 / 4 / 8 / 16, the pair list (query k against candidate k), the P sequential calls with B = 1 on the same
     pairs, and the batch of B = P candidates of query 0: 5 warm-up rounds, then --reps rounds in which the three ALTERNATE; medians;
  2. the run-to-run spread of chip_match_batch_stored at B = 8: five such medians per process, two processes for this tree and -- with
     --parent-lib, a build of the parent commit's library -- two for the parent, alternating, through the same code (--spread);
  3. per variant at P = 8, a child process with CHIP_MATCH_BATCH_TIMING=1 (read once per process): at exit the library prints the device
     time of the kernels by events;
  4. the whole verification from the timing mode of examples/verify_pairs_stored (P = 8).
Every call's status is checked; the first failing one ends the script.  The script runs under a time limit of its own: --limit seconds
for the whole run (an alarm ends the process; the children get what is left of it).  A section of the output file that starts with
the line "# Code objects" is kept as it is."""
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
PS = (1, 4, 8, 16)
WARMUP = 5
SPREAD_RUNS = 5
KEEP = "# Code objects"
PAIRS_SYMBOLS = ("chip_build_has_match_pairs", "chip_match_pairs_stored")


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def check(st, what):
    if st != 0:
        sys.exit(f"{what} -> status {st}")


def fill_store(chip, sc):
    """query k under id 1000 + k, candidate k under id k, k < 16"""
    n1, n2 = len(sc["a"]["kp"]), len(sc["b"]["kp"])
    chip.frame_store_reserve(2 * max(PS), max(n1, n2))
    for k in range(max(PS)):
        a = dict(desc=np.roll(sc["a"]["desc"], 37 * k, axis=0), kp=np.roll(sc["a"]["kp"], 37 * k, axis=0), xyz=sc["a"]["xyz"])
        chip.frame_put(1000 + k, a)
        chip.frame_put(k, sc["b"])


def variants(chip, sc, P: int, with_pairs: bool = True):
    """-> dict name -> call, raw ctypes calls on ids prepared once"""
    lib, h = chip.lib, chip.h
    Ki = np.ascontiguousarray(sc["Kinv"], dtype=np.float64).reshape(9)
    a_ids = np.arange(1000, 1000 + P, dtype=np.int64)
    b_ids = np.arange(P, dtype=np.int64)
    sm_p, sm_l, sm_s = (capi.MatchSummary * P)(), (capi.MatchSummary * P)(), (capi.MatchSummary * P)()
    keep = (Ki, a_ids, b_ids, sm_p, sm_l, sm_s)

    def pairs():
        check(lib.chip_match_pairs_stored(h, capi._ptr(a_ids), capi._ptr(b_ids), P, capi._ptr(Ki), 0, sm_p, None), "chip_match_pairs_stored")

    def loop():
        for j in range(P):
            check(lib.chip_match_batch_stored(h, int(a_ids[j]), C.c_void_p(b_ids.ctypes.data + 8 * j), 1, capi._ptr(Ki), C.byref(sm_l[j])), "chip_match_batch_stored")

    def shared():
        check(lib.chip_match_batch_stored(h, 1000, capi._ptr(b_ids), P, capi._ptr(Ki), sm_s), "chip_match_batch_stored")

    def same():
        if bytes(sm_p) != bytes(sm_l):
            sys.exit(f"P = {P}: the summaries of the pair list and of the loop differ")

    out = dict(loop=loop, shared=shared)
    if with_pairs:
        out["pairs"] = pairs
    return out, same, keep


def rounds(calls: dict, reps: int) -> dict:
    for _ in range(WARMUP):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(reps):                                            # the variants alternate inside the timed window
        for k, fn in calls.items():
            t[k].append(ms(fn))
    return {k: statistics.median(v) for k, v in t.items()}


def child_kernels(which: str, P: int, reps: int):
    sc = synth.make_match_scene(**FULL)
    with capi.Chip(4096) as chip:
        fill_store(chip, sc)
        calls, same, keep = variants(chip, sc, P)
        med = rounds({which: calls[which]}, reps)
    print(f"child {which} P={P} call {med[which]:.4f}")


def child_spread(reps: int):
    """five medians of chip_match_batch_stored at B = 8 on whatever library CHIP_LIB names"""
    sc = synth.make_match_scene(**FULL)
    with capi.Chip(4096) as chip:
        fill_store(chip, sc)
        calls, same, keep = variants(chip, sc, 8, with_pairs=False)
        meds = [rounds(dict(shared=calls["shared"]), reps)["shared"] for _ in range(SPREAD_RUNS)]
    print("spread " + " ".join(f"{m:.4f}" for m in meds))


def run_child(args_list, env, deadline):
    p = subprocess.run([sys.executable, __file__, *args_list, "--limit", str(max(1, int(deadline - time.monotonic())))], env=env, capture_output=True,
                       text=True, timeout=max(1.0, deadline - time.monotonic()))
    if p.returncode != 0:
        sys.exit("child failed:\n" + p.stdout + p.stderr)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "match_pairs.md"))
    ap.add_argument("--limit", type=int, default=420, help="seconds the whole run may take")
    ap.add_argument("--parent-lib", default="", help="libcerebro_hip.so built from the parent commit, for the B = 8 spread")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--spread", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    if args.spread:
        if os.environ.get("CHIP_LIB"):                               # the parent's library has no pair list: do not bind what it lacks
            for name in PAIRS_SYMBOLS:
                capi._SIGS.pop(name, None)
        child_spread(args.reps)
        return
    if args.child:
        child_kernels(args.child, 8, args.reps)
        return
    assert args.reps >= 20
    sc = synth.make_match_scene(**FULL)
    n1, n2 = len(sc["a"]["kp"]), len(sc["b"]["kp"])
    rows = []
    with capi.Chip(4096) as chip:
        arch = chip.info()["arch"]
        fill_store(chip, sc)
        for P in PS:
            calls, same, keep = variants(chip, sc, P)
            med = rounds(calls, args.reps)
            same()
            rows.append((P, med["pairs"], med["loop"], med["shared"]))
    # ---- the spread of the shared-query batch at B = 8, this tree and the parent
    here, parent = [], []
    for _ in range(2):                                               # tree, parent, tree, parent
        here += [float(x) for x in re.search(r"spread (.*)", run_child(["--spread", "--reps", str(args.reps)], dict(os.environ), deadline).stdout).group(1).split()]
        if args.parent_lib:
            env = dict(os.environ, CHIP_LIB=str(Path(args.parent_lib).resolve()), CHIP_ALLOW_LIB_OVERRIDE="1")
            parent += [float(x) for x in re.search(r"spread (.*)", run_child(["--spread", "--reps", str(args.reps)], env, deadline).stdout).group(1).split()]
    # ---- kernels by events at P = 8
    kernels = {}
    pat = {"pairs": r"match pairs stored kernel timing over (\d+) calls \(us\): hamming_match_pairs ([\d.]+), pairs_gms ([\d.]+), pose_sets_stored_pairs ([\d.]+)",
           "loop": r"match batch stored kernel timing over (\d+) calls \(us\): hamming_match_split ([\d.]+), gms_batch ([\d.]+), pose_sets_stored_batch ([\d.]+)",
           "shared": r"match batch stored kernel timing over (\d+) calls \(us\): hamming_match_split ([\d.]+), gms_batch ([\d.]+), pose_sets_stored_batch ([\d.]+)"}
    for which in ("pairs", "loop", "shared"):
        p = run_child(["--child", which, "--reps", str(args.reps)], dict(os.environ, CHIP_MATCH_BATCH_TIMING="1"), deadline)
        m, mc = re.search(pat[which], p.stderr), re.search(r"child \w+ P=8 call ([\d.]+)", p.stdout)
        if not (m and mc):
            sys.exit("child output not understood:\n" + p.stdout + p.stderr)
        kernels[which] = ([float(x) for x in m.groups()[1:]], float(mc.group(1)))
    # ---- the whole verification
    exe = ROOT / "cerebro_amd" / "lib" / "verify_pairs_stored"
    v = subprocess.run([str(exe), "5000", "8", str(args.reps)], capture_output=True, text=True, timeout=max(1.0, deadline - time.monotonic()))
    if v.returncode != 0:
        sys.exit("verify_pairs_stored failed:\n" + v.stdout + v.stderr)
    vlines = [l for l in v.stdout.splitlines() if l.startswith("timing") or l.startswith("stages apart")]

    out = [f"# chip_match_pairs_stored against the loop of batches of one it replaces ({arch}, medians of {args.reps} after {WARMUP} warm-up rounds, scripts/gpu_match_pairs_perf.py)", "",
           f"Frames: {n1} / {n2} keypoints at 752 x 480 (full_5000_5000): 16 query frames and 16 candidates in the store.  Host wall time of the calls; the",
           "three variants alternate in one process.  pair list: P pairs (query k, candidate k) in one chip_match_pairs_stored; loop: the same P pairs as",
           "P sequential chip_match_batch_stored calls with B = 1; shared query: chip_match_batch_stored with B = P candidates of query 0.", "",
           "| P | pair list (ms) | loop of P x (B = 1) (ms) | loop / pair list | shared query, B = P (ms) | pair list / shared |", "|---|---|---|---|---|---|"]
    for P, tp, tl, ts in rows:
        out.append(f"| {P} | {tp:.3f} | {tl:.3f} | {tl / tp:.2f} | {ts:.3f} | {tp / ts:.2f} |")
    out += ["", f"Run-to-run spread of chip_match_batch_stored at B = 8 ({SPREAD_RUNS} medians of {args.reps} per process, two processes per library, the libraries",
            "alternating; ms):", "",
            "| library | medians | min | max |", "|---|---|---|---|",
            f"| this tree | {' '.join(f'{x:.3f}' for x in here)} | {min(here):.3f} | {max(here):.3f} |"]
    if parent:
        out.append(f"| parent commit | {' '.join(f'{x:.3f}' for x in parent)} | {min(parent):.3f} | {max(parent):.3f} |")
    else:
        out.append("| parent commit | not measured (no --parent-lib) | | |")
    out += ["", "Kernels by events at P = 8 (us; a process per variant with CHIP_MATCH_BATCH_TIMING=1, averages over its launches -- for the loop: per call",
            "with B = 1, eight of which make the loop) and that process's own median (the event records and reads are inside it):", "",
            "| variant | matcher | GMS | sets | sum (us) | per P = 8 (us) | median in that process (ms) |", "|---|---|---|---|---|---|---|"]
    names = dict(pairs="pair list (hamming_match_pairs, pairs_gms, pose_sets_stored_pairs)", loop="loop, per call with B = 1 (hamming_match_split, gms_batch, pose_sets_stored_batch)",
                 shared="shared query, B = 8 (the same three)")
    for which in ("pairs", "loop", "shared"):
        k, call = kernels[which]
        out.append(f"| {names[which]} | {k[0]:.1f} | {k[1]:.1f} | {k[2]:.1f} | {sum(k):.1f} | {sum(k) * (8 if which == 'loop' else 1):.1f} | {call:.3f} |")
    out += ["", "Whole verification (examples/verify_pairs_stored 5000 8 " + str(args.reps) + "; its places have 5000 down to 3250 keypoints):", ""] + [f"    {l}" for l in vlines]
    (r8,) = [r for r in rows if r[0] == 8]
    ratio = r8[2] / r8[1]
    out += ["", "Acceptance:", "",
            f"- P = 8: the pair list takes {r8[1]:.3f} ms, the loop it replaces {r8[2]:.3f} ms in the same run: {ratio:.2f} x ({'beats it' if ratio > 1 else 'DOES NOT BEAT IT'}"
            f"{'' if ratio >= 2 else '; below 2 x, see the kernel times above'});"]
    if parent:
        mid = statistics.median(here)
        where = "inside the parent's range" if min(parent) <= mid <= max(parent) else "BELOW the parent's range (faster)" if mid < min(parent) else "ABOVE THE PARENT'S RANGE (slower)"
        out.append(f"- chip_match_batch_stored at B = 8: this tree's medians {min(here):.3f} .. {max(here):.3f} ms, the parent's {min(parent):.3f} .. {max(parent):.3f} ms "
                   f"(spread {max(parent) - min(parent):.3f} ms); this tree's middle median {mid:.3f} ms is {where}.")
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
