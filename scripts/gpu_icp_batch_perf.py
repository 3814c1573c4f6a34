#!/usr/bin/env python3
"""Measures the batched ICP-RANSAC on matched sets against the parent commit's build (profiles/icp_batch.md holds this script's output).

  python scripts/gpu_icp_batch_perf.py --parent DIR [--runs 4] [--reps 30] [--limit 900] [--out profiles/icp_batch.md]

DIR holds the parent commit's build: libcerebro_hip.so, libcerebro_host.so, the examples verify_candidates_stored and
verify_candidates_composed (the latter compiled from this tree's source against the parent's libraries: it uses entry points the parent
has).  Everything alternates parent build / this tree, --runs times, on one box in one visit; a figure is the median over the runs of the
per-run medians of --reps, its range the smallest and largest run median.
  1. whole verification: examples/verify_candidates_stored in timing mode (it prints verify_candidates and verify_candidates_stored) at
     B = 4 / 8 / 16, and on the parent the split of the composition (match call, PnP batch call, ICP loop) by verify_candidates_composed;
  2. chip_icp_ransac_matched_batch against P x (chip_match_select + chip_icp_ransac_matched) at P = 1 / 4 / 8 / 16, reference mode and
     n_hypotheses = 8000, on the 3-D / 3-D sets of the 5000-keypoint scene of profiles/match_batch.md stored under 16 ids (child processes:
     CHIP_LIB + CHIP_ALLOW_LIB_OVERRIDE=1 select the build);
  3. P = 8: enqueue -> chip_pnp_ransac_matched_batch (16 problems) -> collect against the PnP call alone and against the PnP call followed
     by the blocking ICP batch: how much of the ICP is hidden.
Every GPU step is a child process under its own timeout; the first one that fails ends the script.  A section of the output file that
starts with the line "## Code objects" is kept as it is."""
from __future__ import annotations

import argparse
import ctypes as C
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

FULL = dict(n_true=4600, n_outlier_a=400, n_outlier_b=900, flip_rate=0.05, n_duplicates=60, n_border=48, seed=12)
BS = (4, 8, 16)
PS = (1, 4, 8, 16)
MODES = (("reference", 0), ("n_hypotheses = 8000", 8000))
WARMUP = 5
KEEP = "## Code objects"
NEW = ("chip_build_has_icp_batch", "chip_icp_ransac_batch", "chip_icp_ransac_matched_batch_enqueue", "chip_icp_ransac_matched_batch_collect",
       "chip_icp_ransac_matched_batch")


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def child(reps: int):
    """parts 2 and 3 on whichever build CHIP_LIB names; one JSON line"""
    import numpy as np
    from cerebro_amd import capi, synth
    blob = Path(capi.LIB_PATH).read_bytes()
    have_batch = all(n.encode() in blob for n in NEW)
    if not have_batch:                                               # the parent's build: bind what it has
        for n in NEW:
            capi._SIGS.pop(n)
    sc = synth.make_match_scene(**FULL)
    out = dict(have_batch=have_batch, loop={}, batch={}, hidden=None)
    with capi.Chip(4096) as chip:
        lib, h = chip.lib, chip.h
        chip.frame_store_reserve(17, max(len(sc["a"]["kp"]), len(sc["b"]["kp"])))
        chip.frame_put(1000, sc["a"])
        for j in range(16):
            chip.frame_put(j, sc["b"])
        sms = chip.match_batch_stored(1000, list(range(16)), sc["Kinv"])
        out["n_3d3d"] = int(sms[0].n_3d3d)

        def check(st, what):
            if st != 0:
                sys.exit(f"{what} -> status {st}")

        T = np.zeros((32, 16)); conf = np.zeros(32, np.float32); status = np.zeros(32, np.int32)
        c1 = C.c_float()
        T_p, conf_p, status_p, c1_p = capi._ptr(T), capi._ptr(conf), capi._ptr(status), C.byref(c1)   # converted once: not part of a timed call
        for mode, nh in MODES:
            p = capi.default_icp_params()
            p.n_hypotheses = nh
            for P in PS:
                cand = np.arange(P, dtype=np.int32)
                cand_p, p_p = capi._ptr(cand), C.byref(p)

                def loop():
                    for j in range(P):
                        check(lib.chip_match_select(h, j), "chip_match_select")
                        check(lib.chip_icp_ransac_matched(h, p_p, T_p, c1_p, None, None), "chip_icp_ransac_matched")

                def batch():
                    check(lib.chip_icp_ransac_matched_batch(h, P, cand_p, p_p, None, T_p, conf_p, None, None, status_p), "chip_icp_ransac_matched_batch")

                for _ in range(WARMUP):
                    loop()
                    if have_batch:
                        batch()
                tl = [ms(loop) for _ in range(reps)]                 # back to back on either build: the loop is timed the same way on both
                tb = [ms(batch) for _ in range(reps)] if have_batch else []
                out["loop"][f"{mode}|{P}"] = statistics.median(tl)
                if have_batch:
                    out["batch"][f"{mode}|{P}"] = statistics.median(tb)
        if have_batch:                                               # part 3
            P = 8
            cand = np.arange(P, dtype=np.int32)
            pc = np.repeat(np.arange(P, dtype=np.int32), 2)
            which = np.tile(np.array([capi.CHIP_SET_AB, capi.CHIP_SET_BA], np.int32), P)
            pp, pi = capi.default_ransac_params(), capi.default_icp_params()
            pst = np.zeros(2 * P, np.int32)
            cand_p, pc_p, which_p, pst_p, pp_p, pi_p = capi._ptr(cand), capi._ptr(pc), capi._ptr(which), capi._ptr(pst), C.byref(pp), C.byref(pi)

            def pnp():
                check(lib.chip_pnp_ransac_matched_batch(h, 2 * P, pc_p, which_p, pp_p, None, T_p, conf_p, None, None, pst_p), "chip_pnp_ransac_matched_batch")

            def under():
                check(lib.chip_icp_ransac_matched_batch_enqueue(h, P, cand_p, pi_p, None, status_p), "enqueue")
                pnp()
                check(lib.chip_icp_ransac_matched_batch_collect(h, T_p, conf_p, None, None), "collect")

            def after():
                pnp()
                check(lib.chip_icp_ransac_matched_batch(h, P, cand_p, pi_p, None, T_p, conf_p, None, None, status_p), "batch")

            for _ in range(WARMUP):
                pnp(); under(); after()
            t = [[], [], []]
            for _ in range(reps):
                t[0].append(ms(pnp)); t[1].append(ms(under)); t[2].append(ms(after))
            out["hidden"] = [statistics.median(x) for x in t]
    print("CHILD " + json.dumps(out))


def mid(xs):
    return statistics.median(xs)


def rng(xs, d=3):
    return f"{min(xs):.{d}f} – {max(xs):.{d}f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=False, help="directory with the parent commit's build")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "icp_batch.md"))
    ap.add_argument("--limit", type=int, default=900, help="seconds the whole run may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    signal.alarm(args.limit)                                         # SIGALRM's default action ends the process, main or child
    deadline = time.monotonic() + args.limit
    if args.child:
        child(args.reps)
        return
    if not args.parent:
        ap.error("--parent DIR is required")
    parent = Path(args.parent).resolve()
    tree = ROOT / "cerebro_amd" / "lib"
    builds = (("parent", parent), ("tree", tree))

    def run(cmd, env=None, limit=120):
        left = deadline - time.monotonic()
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=max(1.0, min(limit, left)))
        if p.returncode != 0:
            sys.exit(f"{cmd} failed ({p.returncode}):\n{p.stdout}{p.stderr}")   # nothing more is started
        return p.stdout

    # ---- 1: the examples in timing mode, parent and tree alternating
    whole = {(b, B, k): [] for b, _ in builds for B in BS for k in ("host", "stored")}
    split = {B: [] for B in BS}
    pat = re.compile(r"verify_candidates ([\d.]+) ms, verify_candidates_stored ([\d.]+) ms")
    pat2 = re.compile(r"composed ([\d.]+) ms = match ([\d.]+) \+ pnp batch ([\d.]+) \+ icp loop ([\d.]+)")
    for _ in range(args.runs):
        for B in BS:
            for name, d in builds:
                m = pat.search(run([str(d / "verify_candidates_stored"), "3000", str(B), str(args.reps)]))
                whole[(name, B, "host")].append(float(m.group(1)))
                whole[(name, B, "stored")].append(float(m.group(2)))
            m = pat2.search(run([str(parent / "verify_candidates_composed"), "3000", str(B), str(args.reps)]))
            split[B].append([float(x) for x in m.groups()])
    # ---- 2 and 3: child processes on either build
    kids = {name: [] for name, _ in builds}
    for _ in range(args.runs):
        for name, d in builds:
            env = dict(os.environ, CHIP_LIB=str(d / "libcerebro_hip.so"), CHIP_ALLOW_LIB_OVERRIDE="1")
            o = run([sys.executable, __file__, "--child", "--reps", str(args.reps), "--limit", str(max(1, int(deadline - time.monotonic())))], env=env, limit=300)
            kids[name].append(json.loads(re.search(r"CHILD (.*)", o).group(1)))
    if kids["parent"][0]["have_batch"] or not kids["tree"][0]["have_batch"]:
        sys.exit("--parent must name a build without the batched ICP, the tree's build must have it")

    out = [f"# Batched ICP-RANSAC on matched sets (`chip_icp_ransac_batch`, `chip_icp_ransac_matched_batch`)", "",
           f"Measured by scripts/gpu_icp_batch_perf.py on one MI355X in one visit: the parent commit's build and this tree alternate, {args.runs} runs each;",
           f"a figure is the median over the runs of the per-run medians of {args.reps} calls, the range is the smallest – largest run median.  Host wall time, ms.", "",
           "## 1. Whole verification", "",
           "`examples/verify_candidates_stored 3000 B 30` (2-of-B candidates rejected before the solvers: B − 2 survivors).", "",
           "| B | call | parent | parent's range | tree | tree's range | gain | tree ≤ top of parent's range |", "|---|---|---|---|---|---|---|---|"]
    ok1 = True
    for B in BS:
        for k, call in (("stored", "verify_candidates_stored"), ("host", "verify_candidates")):
            a, b = whole[("parent", B, k)], whole[("tree", B, k)]
            ok = mid(b) <= max(a)
            ok1 = ok1 and ok
            out.append(f"| {B} | `{call}` | {mid(a):.3f} | {rng(a)} | {mid(b):.3f} | {rng(b)} | {100 * (1 - mid(b) / mid(a)):+.1f} % | {'yes' if ok else 'NO'} |")
    out += ["", "The split of the tail on the parent (`verify_candidates_composed` linked against the parent's libraries: the composition from single",
            "calls is the parent's `verify_matched`): wall time of the match call, the PnP batch call and the ICP loop.", "",
            "| B | composed | `chip_match_batch_stored` | `chip_pnp_ransac_matched_batch` | ICP loop (B − 2 × select + `chip_icp_ransac_matched`) |", "|---|---|---|---|---|"]
    for B in BS:
        cols = list(zip(*split[B]))
        out.append(f"| {B} | " + " | ".join(f"{mid(c):.3f}" for c in cols) + " |")
    out += ["", "## 2. The batched call against P single calls", "",
            f"The 3-D / 3-D sets of the 5000-keypoint scene of profiles/match_batch.md ({kids['tree'][0]['n_3d3d']} points per candidate), 16 candidates on stored frames.",
            "loop = P × (`chip_match_select` + `chip_icp_ransac_matched`), batch = one `chip_icp_ransac_matched_batch`.", "",
            "| mode | P | parent: loop | parent's range | tree: loop | tree's loop range | tree: batch | tree's batch range | batch ≤ top of the loop's range |", "|---|---|---|---|---|---|---|---|---|"]
    ok2 = True
    ok_p1 = True
    for mode, _ in MODES:
        for P in PS:
            key = f"{mode}|{P}"
            pl = [k["loop"][key] for k in kids["parent"]]
            tl = [k["loop"][key] for k in kids["tree"]]
            tb = [k["batch"][key] for k in kids["tree"]]
            ok = mid(tb) <= max(tl)                                   # the loop's own spread over the runs is the margin
            ok2 = ok2 and ok
            if P == 1:
                ok_p1 = ok_p1 and mid(tb) <= max(pl) and mid(tl) <= max(pl)
            out.append(f"| {mode} | {P} | {mid(pl):.4f} | {rng(pl, 4)} | {mid(tl):.4f} | {rng(tl, 4)} | {mid(tb):.4f} | {rng(tb, 4)} | {'yes' if ok else 'NO'} |")
    hid = list(zip(*[k["hidden"] for k in kids["tree"]]))
    t_pnp, t_under, t_after = (mid(x) for x in hid)
    icp_alone = t_after - t_pnp
    hidden = 1.0 - (t_under - t_pnp) / icp_alone if icp_alone > 0 else float("nan")
    out += ["", "## 3. How much of the ICP is hidden (P = 8, reference mode, 16 PnP problems)", "",
            "| sequence | ms | range |", "|---|---|---|",
            f"| `chip_pnp_ransac_matched_batch` alone | {t_pnp:.3f} | {rng(hid[0])} |",
            f"| enqueue → `chip_pnp_ransac_matched_batch` → collect | {t_under:.3f} | {rng(hid[1])} |",
            f"| `chip_pnp_ransac_matched_batch`, then the blocking `chip_icp_ransac_matched_batch` | {t_after:.3f} | {rng(hid[2])} |", "",
            f"The blocking ICP batch adds {1e3 * icp_alone:.0f} µs behind the PnP call; enqueued before it, it adds {1e3 * (t_under - t_pnp):.0f} µs: "
            f"{100 * hidden:.0f} % of it is hidden.", "",
            "## Acceptance", "",
            f"- 1: the tree's median is no larger than the top of the parent's range at every B, both calls: {'yes' if ok1 else 'NO'};",
            f"- 2: the batch's median is no larger than the top of the loop's range at every P, both modes: {'yes' if ok2 else 'NO'}; at P = 1 the single call and the batch are no larger than the top of the parent's range of the single call: {'yes' if ok_p1 else 'NO'}.", ""]
    text = "\n".join(out) + "\n"
    dst = Path(args.out)
    if dst.exists() and KEEP in dst.read_text():
        old = dst.read_text()
        text += old[old.index(KEEP):]
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
