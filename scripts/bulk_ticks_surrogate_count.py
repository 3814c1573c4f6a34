"""Certified / uncertified ticks of chip_loop_ticks_bulk on the EuRoC surrogate (tests/euroc_surrogate.py: AR(1) rows, temporal neighbours
1e-2 .. 1e-5 apart, revisits), counted WITHOUT a GPU by the numpy model of the call (tests/np_mirror_bulk_ticks.py: the oracle's fmaf-chain
lists, the certificate, exact rescoring) -- the figure the choice of the list length KL rests on (profiles/bulk_ticks.md).

    python scripts/bulk_ticks_surrogate_count.py [--variant mh01] [--kl 16,8] [--topk 1,8]

Per (KL, topk): scanned ticks, certified, uncertified, rows rescored, and the largest number of list entries within 2E of a query's best."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

import euroc_surrogate
import np_mirror_bulk_ticks as nm
import oracle_lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="mh01")
    ap.add_argument("--kl", default="16,8")
    ap.add_argument("--topk", default="1,8")
    a = ap.parse_args()
    run = euroc_surrogate.make_run(a.variant)
    db = run["db"].astype(np.float32)
    assert np.array_equal(db.astype(np.float64), run["db"])
    n = len(db)
    norm = float(np.sqrt((run["db"] ** 2).sum(1).max())) * (1.0 + 2.0 ** -30)
    E = nm.error_bound(db.shape[1], norm)
    status, k, _ = nm.sequence(run["ticks"], n)
    scanned = [(l, kk) for l, s, kk in zip(run["ticks"], status, k) if s == nm.SCANNED]
    print(f"surrogate {a.variant}: {n} rows of {db.shape[1]}, {len(run['ticks'])} ticks, {len(scanned)} scanned, E = {E:.3e}", flush=True)
    kls = [int(x) for x in a.kl.split(",")]
    topks = [int(x) for x in a.topk.split(",")]
    lists = {}
    for l, kk in scanned:                                   # one fmaf-chain scan per tick at the longest list; a shorter list is its head
        lists[l] = oracle_lib.scan_topk_fmaf(db, kk, db[[l - 1, l - 2, l - 3]], max(kls))
    print("| KL | topk | scanned | certified | uncertified | rows rescored | most entries within 2E of the best |")
    print("|---|---|---|---|---|---|---|")
    for KL in kls:
        for topk in topks:
            if topk > KL:
                continue
            cert = resc = most = 0
            for l, kk in scanned:
                ls, li = lists[l]
                ok = True
                for j in range(3):
                    s, i = ls[j, :KL], li[j, :KL]
                    G = s[topk - 1]
                    thr = nm.threshold(G, E)
                    R = int(((i >= 0) & (s >= thr)).sum())
                    dropped = i[KL - 1] >= 0
                    ok &= (not dropped) or s[KL - 1] < thr
                    resc += R
                    most = max(most, int(((i >= 0) & (s >= nm.threshold(s[0], E))).sum()))
                cert += ok
            print(f"| {KL} | {topk} | {len(scanned)} | {cert} | {len(scanned) - cert} | {resc} | {most} |", flush=True)


if __name__ == "__main__":
    main()
