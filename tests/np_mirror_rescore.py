"""numpy models of what a prefilter pass leaves behind (cerebro_amd/csrc/kernels.hip shared_pass / tick_rescore), driven by the
pass's LISTS and its geometry, not by a score vector:
  * owned / owned_count: the row -> workgroup map of the pass (workgroup b owns the rows r with r mod tw in [b wpb, (b + 1) wpb), tw = grid wpb);
  * pass_lists: the list of K every workgroup must leave for one query -- the K best rows it owns inside the prefix by (pass score
    descending, index descending), empty entries (-inf, -1) behind them;
  * rescore: tick_rescore for one query from the workgroup lists -- G, M (with the kernel's ownership count, its clamp included), thr, the
    candidate set R, the certificate word and the exact list.
tests/test_prefilter_bound.py `mirror` is the ancestor (round-robin owners of single rows, scores instead of lists); it stays as it is."""
import numpy as np

CAP = 32                         # kRescoreCap


def owned_count(b, k, grid, wpb):
    """rows of the prefix [0, k) that tick_rescore says workgroup b owned: whole laps of tw rows give wpb each, the last, partial lap gives
    (k mod tw - b wpb) clamped to [0, wpb]"""
    tw = grid * wpb
    part = k % tw - b * wpb
    part = 0 if part < 0 else wpb if part > wpb else part
    return (k // tw) * wpb + part


def owner(rows, grid, wpb):
    """the workgroup that scores each row (shared_pass: wave g = b wpb + w owns rows g, g + tw, ...)"""
    return (np.asarray(rows) % (grid * wpb)) // wpb


def pass_lists(scores, k, grid, wpb, K):
    """(s [grid, K] float64, i [grid, K] int64): per workgroup the K best rows of [0, k) it owns by (scores descending, index descending)"""
    idx = np.arange(k)
    s = np.asarray(scores[:k], dtype=np.float64)
    own = owner(idx, grid, wpb)
    order = np.lexsort((-idx, -s, own))                  # by workgroup, then score descending, then index descending (-0.0 == 0.0: the index decides)
    own_sorted = own[order]
    start = np.searchsorted(own_sorted, np.arange(grid), side="left")
    end = np.searchsorted(own_sorted, np.arange(grid), side="right")
    out_s = np.full((grid, K), -np.inf)
    out_i = np.full((grid, K), -1, dtype=np.int64)
    for b in range(grid):
        sel = order[start[b]:min(end[b], start[b] + K)]
        out_s[b, :len(sel)] = s[sel]
        out_i[b, :len(sel)] = sel
    return out_s, out_i


def topk_by_key(scores, idx, K):
    """the K best of (score descending, index descending), padded with (-inf, -1)"""
    scores, idx = np.asarray(scores, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    order = np.lexsort((-idx, -scores))[:K]
    s = np.full(K, -np.inf)
    i = np.full(K, -1, dtype=np.int64)
    s[:len(order)] = scores[order]
    i[:len(order)] = idx[order]
    return s, i


def rescore(cand_s, cand_i, k, wpb, K, E, exact, cap=CAP):
    """tick_rescore for one query.  cand_s / cand_i [grid, K]: the workgroup lists (sorted, unused entries (-inf, -1)); exact: float64 array of
    the oracle's score of every row (indexed by row).  Returns dict(G, M, dropped, thr, R, cert, exact_s, exact_i); exact_s / exact_i are
    the list the kernel writes when |R| <= cap, None beyond it (which `cap` rows the kernel keeps then is the order of its atomics)."""
    cand_s, cand_i = np.asarray(cand_s, dtype=np.float64), np.asarray(cand_i, dtype=np.int64)
    grid = cand_s.shape[0]
    # M: the K-th entries of the lists whose workgroup owned more than K rows of the prefix
    M, dropped = -np.inf, False
    for b in range(grid):
        if cand_i[b, K - 1] < 0:
            continue
        if owned_count(b, k, grid, wpb) > K and cand_s[b, K - 1] > M:
            M, dropped = float(cand_s[b, K - 1]), True
    # G: the K-th largest score of all entries (-inf with fewer than K rows; indices are unique, so by key == by score)
    valid = cand_i >= 0
    vs = np.sort(cand_s[valid])[::-1]
    G = float(vs[K - 1]) if len(vs) >= K else -np.inf
    with np.errstate(invalid="ignore"):
        thr = np.float64(G) - np.float64(2.0) * np.float64(E)
        thr = thr - np.abs(thr) * np.float64(2.0 ** -51)
    ok = (not dropped) or M < thr                        # strict
    in_R = valid & (cand_s >= thr)
    R = np.sort(cand_i[in_R])
    cert = 1 if ok and len(R) <= cap else 2
    es = ei = None
    if len(R) <= cap:
        es, ei = topk_by_key(np.asarray(exact, dtype=np.float64)[R], R, K)
    return dict(G=G, M=M, dropped=dropped, thr=float(thr), R=R, cert=cert, exact_s=es, exact_i=ei)


def bits(a):
    """float64 array -> its bit patterns (a comparison of these tells -0.0 from 0.0 and does not call two NaNs equal by accident)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
