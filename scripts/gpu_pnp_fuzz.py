"""Fuzz (also run, smaller, by tests/test_fuzz_gpu.py): GPU PnP/ICP RANSAC vs the oracle on many odd scenes (planar, duplicated points, tiny/huge scale, heavy
outliers, minimal N).  Everything must match bit for bit; prints a summary."""
import sys, time
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import np_mirror_pnp as M
import ctypes as C
import oracle_lib as O
from cerebro_amd import capi

from pnp_fuzz_scenes import scene  # noqa: E402  (tests/pnp_fuzz_scenes.py: shared with the CPU test that counts the ties these scenes produce)


def same(g, o):
    ok = g["summary"]["best_hypothesis"] == o["summary"]["best_hypothesis"] and g["summary"]["n_models"] == o["summary"]["n_models"] \
        and g["summary"]["n_iterations"] == o["summary"]["n_iterations"] and np.array_equal(g["mask"], o["mask"])
    if o["summary"]["best_hypothesis"] >= 0:
        ok = ok and np.array_equal(g["T"].view(np.uint64), o["T"].view(np.uint64)) and g["confidence"] == o["confidence"]
    else:
        ok = ok and bool(np.isnan(g["T"]).all())
    return ok

def icp_score(T, A, B, thresh=0.1, use_mle=1):
    """orc_icp_score_model through the library handle itself: T is the 4x4 pose as oracle_lib returns it"""
    lib = O._bind_icp()
    lib.orc_icp_score_model.restype = None
    lib.orc_icp_score_model.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 3
    A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
    Tc = np.ascontiguousarray(T.T.reshape(16))
    cost = C.c_double(); nin = C.c_int32(); mask = np.zeros(A.shape[0], dtype=np.uint8)
    lib.orc_icp_score_model(Tc.ctypes.data, A.ctypes.data, B.ctypes.data, A.shape[0], thresh, use_mle, C.addressof(cost), C.addressof(nin), mask.ctypes.data)
    return cost.value, nin.value, mask


def record_differs(chip, leg, P, Q, seed):
    """Every hypothesis of the call just made (chip_debug_ransac_record: also the losers, the rejected ones and, in the adaptive mode, those
    after the stopping point) against the oracle's hypothesis of the same index under this sweep's parameters (default sample size,
    threshold and scoring, fresh sampler).  Integers equal, cost and pose by bit pattern, mask words equal; a rejected hypothesis has cost
    +inf, no inliers, a NaN pose and an empty mask row.  Returns the first difference as text, None if there is none."""
    pnp = leg == capi.CHIP_RANSAC_LEG_PNP
    d = chip.ransac_record(leg)
    words = d["words"]
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)   # noqa: E731
    for h in range(d["H"]):
        if pnp:
            ok, T, smp = O.pnp_hypothesis(P, Q, seed, h)
            if not np.array_equal(d["sample"][h], smp): return f"hypothesis {h}: sample"
        else:
            ok, T, _ = O.icp_hypothesis(P, Q, seed, h)
        if d["valid"][h] != ok: return f"hypothesis {h}: valid {d['valid'][h]} oracle {ok}"
        if not ok:
            if not (np.isinf(d["cost"][h]) and d["nin"][h] == 0 and np.isnan(d["T"][h]).all() and not d["mask"][h].any()):
                return f"hypothesis {h}: a rejected hypothesis carries a cost, inliers, a pose or mask bits"
            continue
        cost, nin, mask = O.score_model(T, P, Q) if pnp else icp_score(T, P, Q)
        row = np.zeros(8 * words, dtype=np.uint8)
        pb = np.packbits(mask, bitorder="little")
        row[:pb.size] = pb
        if not np.array_equal(u64(d["T"][h]), u64(T.T.reshape(16))): return f"hypothesis {h}: pose"
        if not np.array_equal(d["mask"][h], row.view("<u8")): return f"hypothesis {h}: mask"
        if d["nin"][h] != nin or float(d["cost"][h]).hex() != float(cost).hex(): return f"hypothesis {h}: inliers {d['nin'][h]} / {nin}, cost {d['cost'][h]!r} / {cost!r}"
    return None


def run(n=240, seed=7):
    rng = np.random.default_rng(seed)
    bad = []
    n_models = 0
    with capi.Chip(64) as chip:
        for i in range(n):
            X, uv = scene(i, rng)
            for H in (0, 60):
                sd = 5000 + i
                p = capi.default_ransac_params(); p.n_hypotheses = H; p.seed = sd
                g = chip.pnp_ransac(X, uv, p)
                o = O.pnp_ransac(X, uv, O.ransac_params(n_hypotheses=H, seed=sd))
                n_models += o["summary"]["n_models"]
                if not same(g, o): bad.append(("pnp", i, H, g["summary"], o["summary"]))
                why = record_differs(chip, capi.CHIP_RANSAC_LEG_PNP, X, uv, sd)
                if why: bad.append(("pnp record", i, H, why))
            A = X; B = X @ M.make_scene(N=20, seed=i)[2][:3, :3].T + rng.normal(0, 0.01, X.shape)
            pi = capi.default_icp_params(); pi.n_hypotheses = 40; pi.seed = 9000 + i
            gi = chip.icp_ransac(A, B, pi)
            oi = O.icp_ransac(A, B, O.icp_params(n_hypotheses=40, seed=9000 + i))
            if not same(gi, oi): bad.append(("icp", i, gi["summary"], oi["summary"]))
            why = record_differs(chip, capi.CHIP_RANSAC_LEG_ICP, A, B, 9000 + i)
            if why: bad.append(("icp record", i, why))
    return bad, n_models


if __name__ == "__main__":
    t0 = time.time()
    bad, n_models = run(int(sys.argv[1]) if len(sys.argv) > 1 else 240)
    print(f"fuzz: {len(bad)} mismatches, {n_models} oracle models, {time.time()-t0:.1f} s")
    for b in bad[:10]: print(b)
