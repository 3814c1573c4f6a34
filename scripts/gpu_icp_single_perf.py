#!/usr/bin/env python3
"""Times the blocking chip_icp_ransac -- one estimation -- on several builds of the library in one visit (profiles/icp_batch.md, section
"A single estimation on the shared bodies", holds this script's output).

  python scripts/gpu_icp_single_perf.py --build parent=DIR --build tree=cerebro_amd/lib [--build NAME=DIR ..] [--runs 5] [--limit 600]

DIR holds a libcerebro_hip.so; the FIRST build is the yardstick.  The builds alternate, --runs times, one fresh child process per build
and run (CHIP_LIB + CHIP_ALLOW_LIB_OVERRIDE=1 select the build); the first child that does not exit 0 ends the script.  A child times,
with a host clock around the call (it ends in a stream synchronise), make_icp_scene(N, outlier_frac=0.3, noise=0.01, seed=7) at N = 512
(the scene of bench.py's icp leg) and N = 4096, reference mode and n_hypotheses = 8000: per row --warmup calls, then the median of --reps.
It also prints a digest of T, the mask and the summary per row; nothing is written unless all builds agree on every digest.
A build HOLDS a row if its median over the runs is no larger than the yardstick's median plus the yardstick's own spread on that row
(the largest minus the smallest of its run medians)."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
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

NS = (512, 4096)
MODES = (("reference", 0), ("n_hypotheses = 8000", 8000))
HEAD = "## A single estimation on the shared bodies"


def child(warmup: int, reps: int):
    """the four rows on whichever build CHIP_LIB names; one JSON line"""
    import numpy as np
    from cerebro_amd import capi, synth
    out = dict(ms={}, digest={})
    with capi.Chip(64) as chip:
        lib, h = chip.lib, chip.h
        for N in NS:
            A, B = (np.ascontiguousarray(x, dtype=np.float64) for x in synth.make_icp_scene(N=N, outlier_frac=0.3, noise=0.01, seed=7)[:2])
            T = np.zeros(16); mask = np.zeros(N, np.uint8); conf = C.c_float(); summ = capi.RansacSummary()
            A_p, B_p, T_p, mask_p = capi._ptr(A), capi._ptr(B), capi._ptr(T), capi._ptr(mask)   # converted once: not part of a timed call
            for mode, nh in MODES:
                p = capi.default_icp_params()
                p.n_hypotheses = nh
                p.seed = 3
                p_p, conf_p, summ_p = C.byref(p), C.byref(conf), C.byref(summ)

                def call():
                    st = lib.chip_icp_ransac(h, A_p, B_p, N, p_p, T_p, conf_p, mask_p, summ_p)
                    if st != 0:
                        sys.exit(f"chip_icp_ransac -> status {st}")

                for _ in range(warmup):
                    call()
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call()
                    ts.append(1e3 * (time.perf_counter() - t0))
                key = f"{mode}|{N}"
                out["ms"][key] = statistics.median(ts)
                d = hashlib.sha256(T.tobytes() + mask.tobytes() + bytes(summ) + bytes(conf))
                out["digest"][key] = d.hexdigest()[:16]
    print("CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="append", default=[], metavar="NAME=DIR", help="a build to time; the first one is the yardstick")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "icp_batch.md"))
    ap.add_argument("--limit", type=int, default=600, help="seconds the whole run may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    if args.child:
        child(args.warmup, args.reps)
        return
    builds = []
    for b in args.build:
        name, _, d = b.partition("=")
        so = Path(d).resolve() / "libcerebro_hip.so"
        if not name or not so.exists():
            ap.error(f"--build {b}: no {so}")
        builds.append((name, so))
    if len(builds) < 2:
        ap.error("at least two --build NAME=DIR")

    kids = {name: [] for name, _ in builds}
    for _ in range(args.runs):
        for name, so in builds:
            env = dict(os.environ, CHIP_LIB=str(so), CHIP_ALLOW_LIB_OVERRIDE="1")
            left = deadline - time.monotonic()
            p = subprocess.run([sys.executable, __file__, "--child", "--warmup", str(args.warmup), "--reps", str(args.reps), "--limit", str(max(1, int(left)))],
                               env=env, capture_output=True, text=True, timeout=max(1.0, min(120, left)))
            if p.returncode != 0:
                sys.exit(f"child on {name} failed ({p.returncode}):\n{p.stdout}{p.stderr}")   # nothing more is started
            kids[name].append(json.loads(re.search(r"CHILD (.*)", p.stdout).group(1)))
            print(name, kids[name][-1]["ms"], flush=True)

    keys = [f"{mode}|{N}" for N in NS for mode, _ in MODES]
    first = builds[0][0]
    for key in keys:
        seen = {k["digest"][key] for ks in kids.values() for k in ks}
        if len(seen) != 1:
            sys.exit(f"the builds do not agree on {key}: {sorted(seen)}; nothing written")

    names = [name for name, _ in builds]
    out = [HEAD, "",
           f"Measured by scripts/gpu_icp_single_perf.py on one MI355X in one visit: the builds ({', '.join(names)}) alternate, {args.runs} runs each, a fresh",
           f"process per build and run.  A call is the blocking `chip_icp_ransac` on `make_icp_scene(N, outlier_frac=0.3, noise=0.01, seed=7)`; per row and run",
           f"{args.warmup} calls warm up, then the median of {args.reps}; a figure is the median over the runs, the range the smallest – largest run median.  Host wall",
           f"time, µs.  All builds returned the same T, mask and summary on every row (digest).  A build holds a row if its median is no larger than",
           f"`{first}`'s median plus `{first}`'s own spread (largest − smallest run median).", "",
           "| N | mode | " + " | ".join(f"{n} | {n}'s range" for n in names) + f" | bound ({first} + spread) | " + " | ".join(f"{n} holds" for n in names[1:]) + " |",
           "|---|---|" + "---|---|" * len(names) + "---|" + "---|" * (len(names) - 1)]
    verdict = {n: True for n in names[1:]}
    for N in NS:
        for mode, _ in MODES:
            key = f"{mode}|{N}"
            med = {n: [1e3 * k["ms"][key] for k in kids[n]] for n in names}
            bound = statistics.median(med[first]) + (max(med[first]) - min(med[first]))
            cells = [f"{statistics.median(med[n]):.2f} | {min(med[n]):.2f} – {max(med[n]):.2f}" for n in names]
            holds = []
            for n in names[1:]:
                ok = statistics.median(med[n]) <= bound
                verdict[n] = verdict[n] and ok
                holds.append("yes" if ok else "NO")
            out.append(f"| {N} | {mode} | " + " | ".join(cells) + f" | {bound:.2f} | " + " | ".join(holds) + " |")
    out += [""] + [f"- `{n}` holds every row: {'yes' if verdict[n] else 'NO'}" for n in names[1:]] + [""]
    section = "\n".join(out)
    dst = Path(args.out)
    old = dst.read_text() if dst.exists() else ""
    if HEAD in old:                                                  # a section of an earlier run: replaced, what follows it is kept
        at = old.index(HEAD)
        nxt = old.find("\n## ", at + len(HEAD))
        text = old[:at] + section + ("\n" + old[nxt + 1:] if nxt >= 0 else "")
    else:
        text = old.rstrip("\n") + ("\n\n" if old else "") + section
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(text)
    print(section)


if __name__ == "__main__":
    main()
