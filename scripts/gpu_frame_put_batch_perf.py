#!/usr/bin/env python3
"""Batched frame puts at 752 x 480 and the defaults (n = 5000), measured in one visit -> profiles/frame_put_batch.md.

  python scripts/gpu_frame_put_batch_perf.py [--reps 30] [--out profiles/frame_put_batch.md] [--parent-lib SO] [--no-trace]

  1. host wall time, medians of --reps after warm-up, the variants ALTERNATING in one process (each library is mapped RTLD_LOCAL and
     driven through the C ABI, so the parent commit's library needs none of the new entry points): chip_frame_put_raw_orb_stereo_batch
     and chip_frame_put_orb_stereo_batch at F = 1, 4, 16 and 64 against the loop of F single calls on this tree; the single calls of
     this tree against the parent's; chip_frame_put_records;
  2. kernels and copies from ONE `rocprofv3 --kernel-trace --memory-copy-trace --stats` run of its own: rounds of one raw batch of 16
     and of 16 single raw puts.
The frames: the textured warped raw pair of profiles/rectify.md (scripts/gpu_rectify.py) and copies of it rolled by 8 f columns.
The part of an existing output file from "# What the figures say" on is kept."""
import argparse
import csv
import ctypes as C
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

W, H, N = 752, 480, 5000
FS = (1, 4, 16, 64)
WARMUP = 3
TRACE_ROUNDS = 10
KEEP = "# What the figures say"
P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
Q = np.array([1.0, 0.0, 0.0, -367.215803962, 0.0, 1.0, 0.0, -248.375340610, 0.0, 0.0, 0.0, 458.654, 0.0, 0.0, 1.0 / 0.110073808127, 0.0])


def ptr(a):
    return a.ctypes.data_as(P)


class Lib:
    """one build of libcerebro_hip.so through the C ABI: only what is measured here"""

    def __init__(self, name, path):
        self.name = name
        if "torch" not in sys.modules:                                          # one HIP runtime per process (cerebro_amd.capi.load_library)
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        self.so = C.CDLL(str(path))
        single = [P, I64, I32, I32, P, P, P, P, P, C.POINTER(I32)]
        batch = [P, P, I32, I32, I32, P, P, P, P, P, P]
        sigs = {"chip_create": [C.POINTER(P), I32, I64, I32, I32, I32], "chip_frame_store_reserve": [P, I32, I32],
                "chip_rectify_set_maps": [P, I32, I32] + [P] * 8, "chip_frame_put_orb_stereo": single, "chip_frame_put_raw_orb_stereo": single,
                "chip_frame_put_orb_stereo_batch": batch, "chip_frame_put_raw_orb_stereo_batch": batch,
                "chip_frame_read": [P, I64, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32), P, P, P],
                "chip_frame_put_records": [P, I64, P, P, P, I32, I32, I32], "chip_debug_frame_put_last": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)]}
        for fn, args in sigs.items():
            if hasattr(self.so, fn):
                getattr(self.so, fn).argtypes = args
                getattr(self.so, fn).restype = C.c_int
        self.so.chip_destroy.argtypes = [P]
        self.so.chip_destroy.restype = None
        self.has_batch = hasattr(self.so, "chip_frame_put_raw_orb_stereo_batch")

    def call(self, fn, *args):
        rc = getattr(self.so, fn)(*args)
        if rc != 0:
            raise RuntimeError(f"{self.name}: {fn} returned {rc}")

    def create(self, maps, n_slots):
        h = P()
        self.call("chip_create", C.byref(h), 4096, 0, 0, 0, 1)
        self.call("chip_frame_store_reserve", h, n_slots, N)
        self.call("chip_rectify_set_maps", h, W, H, *[ptr(m) for m in maps[0] + maps[1]])
        return h


def frames(n):
    import gpu_rectify as GR
    maps = tuple(tuple(np.ascontiguousarray(m, np.float32) for m in eye) for eye in GR.calibration())
    left, right = GR.raw_pair(maps)
    return maps, [(np.ascontiguousarray(np.roll(left, 8 * f, axis=1)), np.ascontiguousarray(np.roll(right, 8 * f, axis=1))) for f in range(n)]


def ms(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def alternate(variants, reps):
    """{name: callable} -> {name: (median, min, max)} of `reps` calls each, taken in turns"""
    for _ in range(WARMUP):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


class Puts:
    """the calls of one library on one ctx, on the shared frames"""

    def __init__(self, lib, maps, fr):
        self.lib, self.fr = lib, fr
        self.h = lib.create(maps, 2 * max(FS) + 2)
        self.kept = np.zeros(max(FS), np.int32)
        self.one = I32()
        self.left = (C.c_void_p * len(fr))(*[f[0].ctypes.data for f in fr])
        self.right = (C.c_void_p * len(fr))(*[f[1].ctypes.data for f in fr])
        self.ids = np.arange(len(fr), dtype=np.int64)

    def batch(self, F, raw):
        fn = "chip_frame_put_raw_orb_stereo_batch" if raw else "chip_frame_put_orb_stereo_batch"
        return lambda: self.lib.call(fn, self.h, ptr(self.ids), F, W, H, self.left, self.right, None, None, ptr(Q), ptr(self.kept))

    def loop(self, F, raw):
        fn = "chip_frame_put_raw_orb_stereo" if raw else "chip_frame_put_orb_stereo"

        def run():
            for f in range(F):
                self.lib.call(fn, self.h, 1000 + f, W, H, ptr(self.fr[f][0]), ptr(self.fr[f][1]), None, None, ptr(Q), C.byref(self.one))
        return run

    def records(self, F):
        """F frames read once (not timed) -> the call that puts them back from their records"""
        self.batch(F, True)()
        saved = []
        for f in range(F):
            n, w, h = I32(), I32(), I32()
            d, k, r = np.zeros((N, 32), np.uint8), np.zeros((N, 2), np.float32), np.zeros((N, 4), np.float32)
            self.lib.call("chip_frame_read", self.h, f, C.byref(n), C.byref(w), C.byref(h), ptr(d), ptr(k), ptr(r))
            saved.append((d, k, r, n.value))

        def run():
            for f, (d, k, r, n) in enumerate(saved):
                self.lib.call("chip_frame_put_records", self.h, f, ptr(d), ptr(k), ptr(r), n, W, H)
        return run


def trace_child(path):
    """what the traced run executes: rounds of one raw batch of 16, then rounds of 16 single raw puts"""
    maps, fr = frames(16)
    p = Puts(Lib("traced", path), maps, fr)
    for _ in range(WARMUP + TRACE_ROUNDS):
        p.batch(16, True)()
    for _ in range(WARMUP + TRACE_ROUNDS):
        p.loop(16, True)()
    p.lib.so.chip_destroy(p.h)


def traced(path):
    """-> ({kernel: durations us in launch order}, {copy direction: durations us})"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    kernels, copies = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([exe, "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "fpb", "--", sys.executable, __file__,
                            "--trace-child", str(path)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        for p in Path(tmp).rglob("*.csv"):
            with open(p, newline="") as f:
                for row in csv.DictReader(f):
                    if p.name.endswith("kernel_trace.csv"):
                        kernels.setdefault(row["Kernel_Name"], []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
                    elif p.name.endswith("memory_copy_trace.csv"):
                        copies.setdefault(row.get("Direction", "?"), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: [d for _, d in sorted(v)] for k, v in kernels.items()}, copies


SINGLE_OF = dict(fb_rectify="rectify_pair", fb_pyramid="orb_pyramid", fb_fast_score="orb_fast_score", fb_candidates="orb_candidates", fb_select="orb_select",
                 fb_moments="orb_moments", fb_blur="orb_blur", fb_describe="orb_describe", fb_prefilter="bm_prefilter", fb_keypoints="bm_keypoints")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_put_batch.md"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child")
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.trace_child)

    this = ROOT / "cerebro_amd" / "lib" / "libcerebro_hip.so"
    maps, fr = frames(max(FS))
    mine = Puts(Lib("this tree", this), maps, fr)
    parent = Puts(Lib("parent", Path(a.parent_lib)), maps, fr) if a.parent_lib else None
    L = [f"# Batched frame puts: {W} x {H} at the defaults (n = {N}), measured figures", "",
         f"Written by `scripts/gpu_frame_put_batch_perf.py --reps {a.reps}`.  Frames: the textured warped raw pair of profiles/rectify.md and copies of it",
         f"rolled by 8 f columns; two-stage maps.  Host wall times are medians of {a.reps} calls after {WARMUP} warm-up rounds, the variants alternating in one",
         "process; every call ends in a stream synchronise.  The rectified form is fed the same bytes (its time does not depend on what they show).", ""]
    # ---- 1: batch against loop on this tree
    L += ["## 1. One batch call against the loop of single calls, this tree (ms for all F frames: median, min .. max)", "",
          "| form | F | one batch call | loop of F single calls | ratio of medians | ms per frame, batch | groups, launches, waits of the batch |", "|---|---|---|---|---|---|---|"]
    spread_ok = {}
    for raw in (True, False):
        variants = {}
        for F in FS:
            variants[("batch", F)] = mine.batch(F, raw)
            variants[("loop", F)] = mine.loop(F, raw)
        t = alternate(variants, a.reps)
        for F in FS:
            mine.batch(F, raw)()
            g, l, w = I32(), I32(), I32()
            mine.lib.call("chip_debug_frame_put_last", mine.h, C.byref(g), C.byref(l), C.byref(w))
            b, lo = t[("batch", F)], t[("loop", F)]
            L.append(f"| {'raw' if raw else 'rectified'} | {F} | {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}) | {lo[0]:.3f} ({lo[1]:.3f} .. {lo[2]:.3f}) | {lo[0] / b[0]:.2f} | "
                     f"{b[0] / F:.3f} | {g.value}, {l.value}, {w.value} |")
            if F == 16:
                spread_ok[raw] = (lo[0] - b[0], lo[2] - lo[1], lo[0] / b[0])
    L += [""]
    for raw, (gain, spread, ratio) in spread_ok.items():
        L.append(f"The bar, {'raw' if raw else 'rectified'} form at F = 16: the batch is {gain:.3f} ms faster than the loop it replaces (ratio {ratio:.2f}); the loop's own min .. max "
                 f"spread in this visit is {spread:.3f} ms: {'met' if gain > spread else 'NOT met'}.")
    # ---- 2: the single calls, this tree against the parent
    L += ["", "## 2. The single calls, this tree against the parent commit's library in the same process (ms per call: median, min .. max)", "",
          "| library | chip_frame_put_raw_orb_stereo | chip_frame_put_orb_stereo |", "|---|---|---|"]
    if parent:
        for _ in range(2):                                                       # two rounds, so that the visit's own drift shows
            variants = {}
            for p in (mine, parent):
                variants[(p.lib.name, True)] = p.loop(1, True)
                variants[(p.lib.name, False)] = p.loop(1, False)
            t = alternate(variants, a.reps)
            for p in (mine, parent):
                r, s = t[(p.lib.name, True)], t[(p.lib.name, False)]
                L.append(f"| {p.lib.name} | {r[0]:.3f} ({r[1]:.3f} .. {r[2]:.3f}) | {s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f}) |")
    else:
        L.append("| parent | not measured (no --parent-lib) | |")
    # ---- 3: records
    t = alternate({F: mine.records(F) for F in (1, 16)}, a.reps)
    L += ["", "## 3. chip_frame_put_records (ms for all F frames of 5000 keypoints: median, min .. max)", "", "| F | ms | ms per frame |", "|---|---|---|"]
    L += [f"| {F} | {v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f}) | {v[0] / F:.3f} |" for F, v in t.items()]
    # ---- 4: kernels and copies
    L += ["", f"## 4. Kernels and copies (one rocprofv3 --kernel-trace --memory-copy-trace --stats run of its own: {WARMUP + TRACE_ROUNDS} raw batches of 16, then as many",
          "loops of 16 single raw puts; us per launch: median, min)", ""]
    if a.no_trace:
        L.append("not measured (--no-trace)")
    else:
        try:
            kernels, copies = traced(this)
            L += ["| stage | batch entry, one launch for 16 frames | launches | single form, one launch per frame | launches | 16 x single / batch |", "|---|---|---|---|---|---|"]
            tot_b = tot_s = 0.0
            for b, s in SINGLE_OF.items():
                named = lambda n: next((v for k, v in kernels.items() if re.search(r"(?<![a-z_])" + n + r"(?![a-z_])", k)), None)   # noqa: E731
                kb, ks = named(b), named(s)
                if not kb or not ks:
                    L.append(f"| `{b}` / `{s}` | not in the trace | | | | |")
                    continue
                per_b = statistics.median(kb) * len(kb) / (WARMUP + TRACE_ROUNDS)            # us per batch call (the pyramid: its launches summed)
                per_s = statistics.median(ks) * len(ks) / (WARMUP + TRACE_ROUNDS)            # us per loop of 16
                tot_b += per_b
                tot_s += per_s
                L.append(f"| `{b}` / `{s}` | {statistics.median(kb):.1f}, {min(kb):.1f} | {len(kb)} | {statistics.median(ks):.1f}, {min(ks):.1f} | {len(ks)} | {per_s / per_b:.2f} |")
            L += ["", f"Kernel time per 16 frames (medians x launches): batch {tot_b:.0f} us, loop of single calls {tot_s:.0f} us.", "",
                  "| copies, direction | count | median us | total us per round of both |", "|---|---|---|---|"]
            for d, v in sorted(copies.items()):
                L.append(f"| {d} | {len(v)} | {statistics.median(v):.1f} | {sum(v) / (WARMUP + TRACE_ROUNDS):.0f} |")
        except Exception as e:                                                   # a trace that cannot be taken must not lose the figures above
            L.append(f"not measured: {str(e).splitlines()[-1][:160]}")
    out = Path(a.out)
    kept = out.read_text().split(KEEP, 1)[1] if out.exists() and KEEP in out.read_text() else "\n"
    out.write_text("\n".join(L) + "\n\n" + KEEP + kept)
    print("\n".join(L))


if __name__ == "__main__":
    main()
