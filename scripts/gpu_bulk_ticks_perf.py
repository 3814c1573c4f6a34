"""Bulk ticks (chip_loop_ticks_bulk) against the loop of pipelined ticks (chip_loop_tick_enqueue / _collect, 16 in flight) on the same ctx and
the same schedule, one device, float rows.

    python scripts/gpu_bulk_ticks_perf.py [--configs 4096x100000x3,8192x29000x3,4096x1000000x732] [--rounds 3] [--topk 1] [--out FILE]
    python scripts/gpu_bulk_ticks_perf.py --lib PATH ...           (another build of the library, e.g. one with -DCHIP_BULK_LIST_LEN=8)
    python scripts/gpu_bulk_ticks_perf.py --rows-call 4096x100000x4096 [--lib PATH]     (chip_query_batch_rows_f32 alone: the unchanged path)
    python scripts/gpu_bulk_ticks_perf.py --configs surrogate          (the EuRoC surrogate of tests/euroc_surrogate.py: its rows, its tick schedule)
    python scripts/gpu_bulk_ticks_perf.py --breakeven 4096x100000      (T = 1, 2, 4, ... scanned ticks at the end of the DB: from which T on the call wins)

A config is D x rows x step: the ticks at l = 56, 56 + step, ... up to the DB's length (step 3 is the whole schedule of a live node, a larger
step a sample of it).  Synthetic unit rows.  A warm-up of both legs first (and the records of the two compared: they must be equal); then
the legs alternate within a round, wall time per leg, the median over the rounds is reported."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from cerebro_amd import capi

NEW = ("chip_build_has_bulk_ticks", "chip_loop_ticks_bulk", "chip_bulk_ticks_plan", "chip_debug_bulk_ticks_last")
WINDOW = 16


def use_library(path, without_new):
    """bind another build of the library (one library per process); without_new: a build from before the bulk call"""
    saved = {n: capi._SIGS.pop(n) for n in NEW} if without_new else {}
    capi._lib = capi.load_library(path)
    capi._SIGS.update(saved)


def pipelined(chip, ls, p):
    out, pending = [], []
    chip.loop_reset()
    for i, l in enumerate(ls):
        if len(pending) == WINDOW:
            out.append(bytes(chip.loop_tick_collect(pending.pop(0))))
        chip.loop_tick_enqueue(int(l), i % WINDOW, p)
        pending.append(i % WINDOW)
    while pending:
        out.append(bytes(chip.loop_tick_collect(pending.pop(0))))
    return out


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4096x100000x3,8192x29000x3,4096x1000000x732")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--topk", type=int, default=1)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", action="store_true", help="--lib is a build from before the bulk call (with --rows-call)")
    ap.add_argument("--rows-call", default=None, help="D x rows x Q: time chip_query_batch_rows_f32 alone")
    ap.add_argument("--breakeven", default=None, help="D x rows: both legs for T = 1, 2, 4, ... 256 ticks at the end of the DB")
    ap.add_argument("--no-ticks", action="store_true", help="leave the pipelined leg out (a run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        use_library(a.lib, a.parent_lib)
    lines = []
    if a.rows_call:
        D, rows, Q = (int(x) for x in a.rows_call.split("x"))
        with capi.Chip(D, capacity_hint=rows) as chip:
            chip.append_synthetic(rows, 1, unit=True)
            qr = (np.arange(Q, dtype=np.int64) * 37 + 60) % rows
            k = np.maximum(0, qr - 50)
            chip.query_batch_rows(qr, k, 8)
            ts = [wall(lambda: chip.query_batch_rows(qr, k, 8))[1] for _ in range(max(a.rounds, 5))]
            lines.append(f"chip_query_batch_rows_f32 D={D} rows={rows} Q={Q} topk=8 lib={a.lib or 'this tree'}: median {statistics.median(ts) * 1e3:.2f} ms "
                         f"(min {min(ts) * 1e3:.2f}, {len(ts)} calls)")
            print(lines[-1], flush=True)
    elif a.breakeven:
        D, rows = (int(x) for x in a.breakeven.split("x"))
        p = capi.default_dot_params()
        lines += ["| D | rows | T | bulk ms | pipelined ms | pipelined / bulk |", "|---|---|---|---|---|---|"]
        with capi.Chip(D, capacity_hint=rows) as chip:
            chip.append_synthetic(rows, 1, unit=True)
            for T in (1, 2, 4, 8, 16, 32, 64, 128, 256):
                ls = np.arange(rows - 3 * (T - 1), rows + 1, 3, dtype=np.int64)
                assert len(ls) == T
                assert [bytes(r) for r in chip.loop_ticks_bulk(ls, p, 0, a.topk)[0]] == pipelined(chip, ls, p)
                tb, tp = [], []
                for _ in range(max(a.rounds, 7)):
                    tb.append(wall(lambda: chip.loop_ticks_bulk(ls, p, 0, a.topk))[1])
                    tp.append(wall(lambda: pipelined(chip, ls, p))[1])
                b, q = statistics.median(tb), statistics.median(tp)
                lines.append(f"| {D} | {rows} | {T} | {b * 1e3:.3f} | {q * 1e3:.3f} | {q / b:.2f} |")
                print(lines[-1], flush=True)
    else:
        lines += ["| D | rows | step | ticks | KL | bulk s | bulk ticks/s | pipelined s | pipelined ticks/s | pipelined / bulk | groups | certified | uncertified | exact reruns | rescored rows |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        p = capi.default_dot_params()
        for cfg in a.configs.split(","):
            if cfg == "surrogate":
                sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
                import euroc_surrogate
                run = euroc_surrogate.make_run("mh01")
                D, rows, step = run["db"].shape[1], run["db"].shape[0], "surrogate"
                ls = np.asarray(run["ticks"], dtype=np.int64)
            else:
                D, rows, step = (int(x) for x in cfg.split("x"))
                ls = np.arange(56, rows + 1, step, dtype=np.int64)
            with capi.Chip(D, capacity_hint=rows) as chip:
                if cfg == "surrogate":
                    chip.append_f32(run["db"].astype(np.float32))
                else:
                    chip.append_synthetic(rows, 1, unit=True)
                recs = chip.loop_ticks_bulk(ls, p, 0, a.topk)[0]              # warm-up, and the comparison
                dbg = chip.debug_bulk_ticks_last()
                if not a.no_ticks:
                    want = pipelined(chip, ls, p)
                    assert [bytes(r) for r in recs] == want, "the bulk records differ from the pipelined ticks'"
                tb, tp = [], []
                for _ in range(a.rounds):
                    tb.append(wall(lambda: chip.loop_ticks_bulk(ls, p, 0, a.topk))[1])
                    if not a.no_ticks:
                        tp.append(wall(lambda: pipelined(chip, ls, p))[1])
                b = statistics.median(tb)
                q = statistics.median(tp) if tp else float("nan")
                lines.append(f"| {D} | {rows} | {step} | {len(ls)} | {dbg['list_len']} | {b:.3f} | {len(ls) / b:.0f} | {q:.3f} | {len(ls) / q:.0f} | {q / b:.2f} | "
                             f"{dbg['groups']} | {dbg['certified']} | {dbg['uncertified']} | {dbg['exact_reruns']} | {dbg['rescored_rows']} |")
                print(lines[-1], flush=True)
    if a.out:
        out = Path(a.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        with out.open("a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
