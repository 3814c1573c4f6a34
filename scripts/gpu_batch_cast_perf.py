"""Many-query mode on double rows (chip_query_batch_cast_f32) against the float-row call and against the only other way to answer
the same queries on a double-row DB -- chip_query_vectors_f64 four at a time -- on one device, D = 4096.

    python scripts/gpu_batch_cast_perf.py [--rows 100000,1000000] [--q 128,256,512] [--rounds 3] [--out profiles/batch_cast_f64.md]
    python scripts/gpu_batch_cast_perf.py --rows 1000000 --q 256 --no-vectors      (a short run to put under rocprofv3 --kernel-trace --stats)

Both contexts hold the same synthetic rows (float-valued, so the cast is lossless there and the cast call must return the float
call's indices and score bits: asserted).  A warm-up call first; the legs alternate within a round; kernel time is the library's own
(chip_profile_enable / chip_profile_scan: events around the GEMM launch, or around each scan pass of the four-at-a-time leg)."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from cerebro_amd import capi

D, K, PEAK_TF = 4096, 8, 157.3


def timed(chip, fn):
    chip.profile_enable(True)
    chip.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = time.perf_counter() - t0
    ms, cnt, _bytes, _span = chip.profile_scan()
    chip.profile_enable(False)
    return out, wall * 1e3, ms, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--q", default="128,256,512")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-vectors", action="store_true", help="leave the four-at-a-time fp64 leg out")
    ap.add_argument("--out", default="profiles/batch_cast_f64.md")
    a = ap.parse_args()
    lines = ["# Many-query mode on double rows: `chip_query_batch_cast_f32` vs the float-row call vs `chip_query_vectors_f64` x Q/4", "",
             f"One device, D = {D}, top-{K}, synthetic rows (float-valued: the cast call returned the float call's indices and score bits in every",
             f"run below). Kernel times from `chip_profile_scan` (best of {a.rounds} alternating rounds after a warm-up call); TFLOP/s against {PEAK_TF};",
             "HBM GB/s of the cast call on 8 D bytes per row and query tile. `fp64 x Q/4`: the same Q queries through `chip_query_vectors_f64`,",
             "four per call, kernel time summed over the Q/4 passes.", "",
             "| rows | Q | float kernel ms | TFLOP/s | cast kernel ms | TFLOP/s | HBM GB/s | cast / float | cast call ms | fp64 x Q/4 kernel ms | fp64 x Q/4 wall ms | fp64 / cast |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for rows in [int(x) for x in a.rows.split(",")]:
        with capi.Chip(D, capacity_hint=rows) as cf, capi.Chip(D, capacity_hint=rows, storage="f64") as cd:
            cf.append_synthetic(rows, 1)
            cd.append_synthetic(rows, 1)
            assert cf.info()["storage_bytes"] == 4 and cd.info()["storage_bytes"] == 8
            for Q in [int(x) for x in a.q.split(",")]:
                q = cf.read_rows(np.arange(Q) * 37 % rows)
                q64 = q.astype(np.float64)
                fl = 2.0 * Q * rows * D
                legs = {"float": lambda: cf.query_batch(rows, q, K),
                        "cast": lambda: cd.query_batch(rows, q, K, cast_rows=True)}
                chips = {"float": cf, "cast": cd, "fp64": cd}
                if not a.no_vectors:
                    legs["fp64"] = lambda: [cd.query_vectors_f64(rows, q64[i:i + 4], K) for i in range(0, Q, 4)]
                for fn in legs.values():
                    fn()                                                     # warm-up: buffers, first launches
                best = {}
                for _ in range(a.rounds):
                    for name, fn in legs.items():
                        out, wall, kms, cnt = timed(chips[name], fn)
                        assert cnt >= 1, (name, cnt)
                        if name not in best or kms < best[name][0]:
                            best[name] = (kms, wall)
                        if name == "float":
                            ref = out
                            assert (out[1][:, 0] == np.arange(Q) * 37 % rows).all()
                        elif name == "cast":
                            assert np.array_equal(out[1], ref[1]) and out[0].tobytes() == ref[0].tobytes(), "cast call differs from the float call"
                        else:
                            assert all(int(o[1][j, 0]) == (i * 4 + j) * 37 % rows for i, o in enumerate(out) for j in range(o[1].shape[0]))
                f_ms, c_ms = best["float"][0], best["cast"][0]
                qtiles = (Q + 127) // 128 if (Q + 127) // 128 * 128 % 256 else (Q + 255) // 256
                row = [rows, Q, f"{f_ms:.2f}", f"{fl / f_ms / 1e9:.1f}", f"{c_ms:.2f}", f"{fl / c_ms / 1e9:.1f}",
                       f"{rows * D * 8.0 * qtiles / c_ms / 1e6:.0f}", f"{c_ms / f_ms:.3f}", f"{best['cast'][1]:.2f}"]
                if "fp64" in best:
                    v_ms, v_wall = best["fp64"]
                    row += [f"{v_ms:.1f}", f"{v_wall:.1f}", f"{v_ms / c_ms:.1f}"]
                    if rows >= 1_000_000 and Q == 256:
                        assert c_ms < v_ms and best["cast"][1] < v_wall, "the cast call must beat the same queries four at a time"
                else:
                    row += ["not run"] * 3
                lines.append("| " + " | ".join(str(x) for x in row) + " |")
                print(lines[-1], flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
