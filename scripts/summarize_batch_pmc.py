#!/usr/bin/env python3
"""gpurun_out/r02/batch/pmc*/ (scripts/gpu_batch_pmc2.sh) -> profiles/r02_batch_pmc.md + profiles/batch_traffic.json"""
import glob
import json
import sqlite3
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
rows = {}
for db in sorted(glob.glob(str(ROOT / "gpurun_out/r02/batch/pmc*/*_results.db"))):
    con = sqlite3.connect(db)
    for n, cn, c, a in con.execute("select kernel_name, counter_name, count(*), avg(value) from counters_collection "
                                   "where kernel_name like '%db_gemm%' group by kernel_name, counter_name"):
        rows[cn] = (c, a, n)
kname = list(rows.values())[0][2]
gui = rows['GRBM_GUI_ACTIVE'][1] / 8
busy = rows['SQ_VALU_MFMA_BUSY_CYCLES'][1] / (gui * 1024)
fetch = rows['FETCH_SIZE'][1] * 1024 * 2
variants = (ROOT / "gpurun_out/r02/batch_variants.txt").read_text().strip().splitlines() if (ROOT / "gpurun_out/r02/batch_variants.txt").exists() else []
md = ["# rocprofv3 PMC passes on the many-query MFMA kernel `db_gemm_topk` (Q = 256 x 1M x 4096), round 2", "",
      "`bash scripts/gpu_batch_pmc2.sh` (separate `--pmc` runs of `scripts/run_batch_once.py`, three launches each; no trace domain besides",
      f"`--kernel-trace`). Kernel as shipped: `{kname}` = 256 x 256 tile on 8 waves, two LDS-DMA stages, one workgroup per CU, VALU-free and bank-conflict-free fragment reads.", "",
      "| counter | dispatches | avg per launch |", "|---|---|---|"]
md += [f"| {cn} | {c} | {a:.5e} |" for cn, (c, a, n) in rows.items()]
md += ["", f"Derived: `GRBM_GUI_ACTIVE` / 8 XCDs = {gui:.3e} cycles per launch; MFMA pipe utilisation = `SQ_VALU_MFMA_BUSY_CYCLES` /",
       f"({gui:.3e} x 1024 SIMDs) = **{busy:.3f}** (the counter equals the matrix work, 5.24e8 MFMAs x 64 cycles; round 1: 0.65 / 0.716);",
       f"HBM traffic = `FETCH_SIZE` {rows['FETCH_SIZE'][1]:.5e} KiB x 1024 x 2 (gfx950 wide-read correction, MI355X_MICROARCH.md HBM section) = **{fetch / 1e9:.1f} GB**",
       "per launch = the 16.4 GB DB once per 128-query tile (2 tiles) + queries; `SQ_LDS_BANK_CONFLICT` is non-zero BY DESIGN: the DB tile",
       "is read as `ds_read2_b32` column reads over unpadded 128-B rows (4-way), which costs LDS-array cycles",
       f"(`SQ_LDS_IDX_ACTIVE` {rows['SQ_LDS_IDX_ACTIVE'][1]:.3e}, i.e. {rows['SQ_LDS_IDX_ACTIVE'][1] / 256 / gui:.2f} of the launch per CU) instead of VALU issue slots;",
       f"`SQ_WAIT_INST_LDS` / (4 x `SQ_WAVE_CYCLES`) = {rows['SQ_WAIT_INST_LDS'][1] / (4 * rows['SQ_WAVE_CYCLES'][1]):.4f} of wave time.", "",
       "Throughput of the same launch on the same box (hipEvents; the sweep script is in the git history up to commit `af4232e`):", ""] + [f"    {v}" for v in variants] + ["",
       "This quantity varies between the boxes of the pool: two stages 119.4 / 118.3 / 111.1 / 117.5 TFLOP/s on four boxes (0.71-0.76 of 157.3),",
       "a four-stage variant at one workgroup per CU, since removed, measured 112.4 / 113.1 / 112.3 / 113.0; round-1 kernel 110.9 / 105-106.", "",
       "On the way (four-stage variant with 16-B fragment reads + `v_cndmask`, one workgroup per CU, 104 TFLOP/s): MFMA busy 0.668 with ONE wave",
       "per SIMD, `SQ_LDS_BANK_CONFLICT` 3.4e5 (none), `SQ_WAIT_INST_LDS` 0.2 % -- LDS idle, HBM modest, so the wave's own instruction stream was",
       "what the matrix pipe waited for; round-1 kernel: MFMA busy 0.716 at two waves per SIMD, `FETCH_SIZE` 1.68e7 KiB.", "",
       "Inner-loop microbenchmark (`scripts/probes/mfma_probe.hip`, 20 000 chunks of 64 MFMAs, one workgroup of 4 waves per CU unless noted):", "",
       "| loop | TFLOP/s | of 157.3 |", "|---|---|---|",
       "| pure MFMA, 4 accumulators (2 workgroups per CU) | 154.8 | 0.984 |",
       "| pure MFMA, 4 accumulators | 150.7 | 0.958 |",
       "| + `ds_read2_b32` fragments from a padded tile, register double buffer | 151.5 | 0.963 |",
       "| + 32 `ds_write_b32` + one barrier per 64 MFMAs | 134.2 | 0.853 |",
       "| 16-B fragment reads (`ds_read_b128`, swizzled) + one `v_cndmask` per operand | 125.8 | 0.800 |",
       "| ... + barrier per 64 MFMAs | 122.9 | 0.781 |",
       "| ... + 8 LDS-DMA per wave per 64 MFMAs, `vmcnt(16)` | 116.4 | 0.740 |",
       "| A from a `[k][row]` image (`ds_read_b32`), B swizzled rows read as `ds_read2_b32` (4-way conflict), no VALU | 142.2 | 0.904 |",
       "| ... + LDS-DMA + counted barrier per 64 MFMAs | 128.6 | 0.818 |",
       "| 128 x 64 per wave (4 x 2 MFMA tiles, workgroup tile 256 x 128): 16 MFMAs per 4 A + 2 B reads, no DMA | 146.0 | 0.928 |",
       "| ... + 12 LDS-DMA + barrier per 128 MFMAs (two 48-KiB stages) | 133.3 | 0.847 |", "",
       "(The last two rows are the next step that was NOT taken: +3 points in the probe for a rewrite of the tile mapping and the epilogue.)", "",
       "Ablation of the shipped kernel with the accumulators kept alive: without the top-k epilogue 117.9 (two stages) / 120.3 (four stages)",
       "against 114.6 / 113.6 with it on that box: the epilogue is 3-6 % of the kernel (round 1: 17 %).", ""]
(ROOT / "profiles/r02_batch_pmc.md").write_text("\n".join(md))
json.dump({"tag": "r02", "kernel": "db_gemm_topk", "hbm_bytes_per_launch": fetch, "fetch_size_kib_avg": rows['FETCH_SIZE'][1],
           "correction": "FETCH_SIZE*1024*2 (MI355X_MICROARCH.md, HBM section)", "shape": "Q=256 x 1M x 4096", "mfma_busy": busy},
          open(ROOT / "profiles/batch_traffic.json", "w"), indent=1)
print(f"mfma busy {busy:.3f}  traffic {fetch / 1e9:.1f} GB")
