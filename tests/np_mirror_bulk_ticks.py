"""numpy model of bulk_tick_finish (cerebro_amd/csrc/kernels.hip) and of the call around it (batch.hip chip_loop_ticks_bulk):
per query, from the sorted list of KL fp32 fmaf-chain scores the many-query GEMM leaves (oracle_lib.scan_topk_fmaf with K = KL) and the
error bound E -- G, M, thr, the candidate set R, the certificate -- then the exact scores of R in the scan's own arithmetic
(oracle_lib.scan_topk), the topk best by (score desc, index desc), and the tick's record by the accept rule of Cerebro.cpp:1056."""
import numpy as np

import oracle_lib

SKIPPED, TOO_SHORT, SCANNED = 0, 1, 2


def error_bound(D, norm_max):
    """E as prefilter_error_bound (kernels.hip) evaluates it"""
    u32, u64 = 2.0 * D * 2.0 ** -24, (D + 8.0) * 2.0 ** -53
    g = u32 / (1.0 - u32) + u64 / (1.0 - u64)
    return (g * norm_max * norm_max + D * 2.0 ** -148) * (1.0 + 2.0 ** -40)


def threshold(G, E):
    with np.errstate(invalid="ignore"):
        thr = np.float64(G) - np.float64(2.0) * np.float64(E)
        return float(thr - np.abs(thr) * np.float64(2.0 ** -51))


def finish_query(list_s, list_i, topk, E, db, q):
    """one query: list_s / list_i the KL entries (sorted; unused (-inf, -1)), db the rows, q the query vector.
    -> dict(G, M, dropped, thr, R, certified, s [topk], i [topk])"""
    list_s, list_i = np.asarray(list_s, np.float64), np.asarray(list_i, np.int64)
    KL = len(list_s)
    G = float(list_s[topk - 1])                            # -inf where that slot is unused
    dropped = bool(list_i[KL - 1] >= 0)
    M = float(list_s[KL - 1])
    thr = threshold(G, E)
    R = list_i[(list_i >= 0) & (list_s >= thr)]
    certified = (not dropped) or M < thr                   # strict
    s = np.full(topk, -np.inf)
    i = np.full(topk, -1, np.int64)
    if len(R):
        rows = np.sort(R)                                  # ascending: the oracle's index order on the subset is the rows' own
        es, ei = oracle_lib.scan_topk(db[rows], len(rows), q, len(rows))
        n = min(topk, len(rows))
        s[:n], i[:n] = es[0, :n], rows[ei[0, :n]]
    return dict(G=G, M=M, dropped=dropped, thr=thr, R=R, certified=certified, s=s, i=i)


def decide(tops_s, tops_i, l, locality=12, thresh=float(np.float32(0.85))):
    """the record of a scanned tick from the best entry of each query (topk_merge.h tick_decision)"""
    r = dict(status=SCANNED, found=0, idx_curr=-1, idx_prev=-1, score=0.0, argmax=[int(x) for x in tops_i], maxv=[float(x) for x in tops_s])
    a = r["argmax"]
    if min(a) >= 0 and abs(a[0] - a[1]) < locality and abs(a[0] - a[2]) < locality and r["maxv"][0] > thresh:
        r.update(found=1, idx_curr=l - 1, idx_prev=a[0], score=r["maxv"][0])
    return r


def tick(db, l, k, KL, topk, E, locality=12, thresh=float(np.float32(0.85))):
    """one scanned tick: queries db[l-1], db[l-2], db[l-3] against rows [0, k).
    -> dict(certified, rescored, q: [3 x finish_query], s [3, topk], i [3, topk], record)"""
    q = db[[l - 1, l - 2, l - 3]]
    ls, li = oracle_lib.scan_topk_fmaf(db, k, q, KL)
    per = [finish_query(ls[j], li[j], topk, E, db, q[j]) for j in range(3)]
    s, i = np.stack([p["s"] for p in per]), np.stack([p["i"] for p in per])
    return dict(certified=all(p["certified"] for p in per), rescored=sum(len(p["R"]) for p in per), q=per, s=s, i=i,
                record=decide(s[:, 0], i[:, 0], l, locality, thresh))


def sequence(ls, n_rows, last_l=0, lag=50, min_new=3, min_k=5):
    """(status, k) of the ticks at ls run one after the other, and the loop state afterwards (chip_api.hip tick_prepare)"""
    status, k = [], []
    for l in ls:
        assert 0 <= l <= n_rows
        if l - last_l < min_new:
            status.append(SKIPPED); k.append(0)
            continue
        assert l >= 3
        kk = l - lag
        status.append(SCANNED if kk > min_k else TOO_SHORT)
        k.append(kk if kk > min_k else 0)
        last_l = l
    return status, k, last_l


def immediate(status):
    return dict(status=status, found=0, idx_curr=-1, idx_prev=-1, score=0.0, argmax=[-1] * 3, maxv=[-np.inf] * 3)
