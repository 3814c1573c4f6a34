"""Tiny driver for a HIP-call trace (rocprofv3 --hip-trace -- python scripts/run_owner_calls_once.py <kind> [calls]) of the calls whose
scratch the library owns: `pnp` (chip_pnp_ransac, 512 correspondences x 1000 hypotheses), `icp` (chip_icp_ransac, 300 points x 500
hypotheses), `batch` (chip_query_batch_f32, 256 queries over 100k rows).  Every call after the first is of the same size, so it must
neither allocate nor free (profiles/r08_buffer_owners.md)."""
import sys
sys.path.insert(0, '.')
import numpy as np
from cerebro_amd import capi
from cerebro_amd.synth import make_scene, make_icp_scene

kind = sys.argv[1]
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
if kind == "pnp":
    X, uv, T, inl = make_scene(N=512, outlier_frac=0.3, noise_px=0.5, seed=4242)
    with capi.Chip(64) as chip:
        p = capi.default_ransac_params(); p.n_hypotheses = 1000
        for i in range(calls):
            p.seed = 4242 + i
            r = chip.pnp_ransac(X, uv, p)
        print("ok", r["summary"])
elif kind == "icp":
    A, B = make_icp_scene(N=300, outlier_frac=0.2, noise=0.02, seed=1)[:2]
    with capi.Chip(64) as chip:
        p = capi.default_icp_params(); p.n_hypotheses = 500
        for i in range(calls):
            p.seed = 7 + i
            r = chip.icp_ransac(A, B, p)
        print("ok", r["summary"])
elif kind == "batch":
    rows, Q, D = 100_000, 256, 4096
    with capi.Chip(D, capacity_hint=rows) as chip:
        chip.append_synthetic(rows, 1)
        q = chip.read_rows((np.arange(Q) * 379) % rows)
        for _ in range(calls):
            sc, ix = chip.query_batch(rows, q, 8)
        print("ok", int((ix[:, 0] == (np.arange(Q) * 379) % rows).sum()))
else:
    raise SystemExit("kind: pnp | icp | batch")
