"""Crafted list sets for the top-K list merge (csrc/topk_merge.h), a plain reference of the merge and a reach model of its staging.

A QUERY is a list of n_lists lists; each list is either FAILED (the list of a shard that could not take part: (-inf, -2) in every entry)
or at most K (score, idx) entries sorted by (score descending, idx descending).  A CASE stacks nq queries into [n_lists][nq][K] arrays,
unused slots (-inf, -1).  Input contract, kept by every generator and checked by check_contract(): lists sorted by key, indices unique per
query across lists, no NaN.  -0.0 and +0.0 are EQUAL scores: the index orders them.

reference()  what the merge must deliver: all valid entries of a query, sorted, the first K, padded; the failure mark; the tick record.
reach()      a model of the STAGING only -- which heads a wave of 64 lists sees, which it posts, the threshold T1 (the K-th best posted head),
             which prefixes survive -- so that a CPU test can say which paths of the kernel a case set reaches.  It ranks with Python's sort.
"""
from __future__ import annotations

import functools
import math
import struct
from dataclasses import dataclass, field

import numpy as np

FAILED = "failed"
NEG_INF = float("-inf")
DBL_MAX = 1.7976931348623157e308
SUBNORMAL = 5e-324
MAX_TOPK, MAX_LISTS = 16, 512
THRESH = 0.85000002384185791015625      # capi.default_dot_params(): (double)(float)0.85
LOCALITY = 12
TICK_L = 1000
TICK_SCANNED, TICK_FAILED = 2, 3

N_LISTS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512)
KS = (1, 2, 5, 8, 15, 16)


def key(e):
    """sort key of an entry: Python compares the tuple (score, idx), and 0.0 == -0.0"""
    return (e[0], e[1])


# ------------------------------------------------------------------------------------------------ the order-preserving key image
def okey(s: float) -> int:
    """the 64-bit integer whose unsigned order is the order of the doubles (no NaN), -0.0 taking the image of +0.0"""
    b = struct.unpack("<Q", struct.pack("<d", s))[0]
    if b == 1 << 63:
        b = 0
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def hi32(s: float) -> int:
    return okey(s) >> 32


def nudge(base: float, j: int) -> float:
    """the double j units in the last place further from zero than base: same upper 32 key bits for 0 <= j < 2**20"""
    b = struct.unpack("<Q", struct.pack("<d", base))[0]
    return struct.unpack("<d", struct.pack("<Q", b + j))[0]


# ------------------------------------------------------------------------------------------------ reference
def reference_query(lists, K):
    ents = [e for l in lists if l is not FAILED for e in l if e[1] >= 0]
    ents.sort(key=key, reverse=True)
    top = ents[:K]
    return top + [(NEG_INF, -1)] * (K - len(top))


def reference(case, form):
    """(scores [nq][K], idx [nq][K], record or None).  Form 0: one workgroup merges all nq queries, writes the failure mark to out[0] and the
    record.  Form 1: one workgroup per four queries, each with its own out[0]; no record."""
    nq, K = case.nq, case.K
    tops = [reference_query(q, K) for q in case.queries]
    sc = np.array([[e[0] for e in t] for t in tops], dtype=np.float64).reshape(nq, K)
    ix = np.array([[e[1] for e in t] for t in tops], dtype=np.int64).reshape(nq, K)
    failed = any(l is FAILED for l in case.queries[0])
    if failed:
        for g in ([0] if form == 0 else range(0, nq, 4)):
            ix[g, 0] = -2
    rec = None
    if form == 0:
        argmax = [tops[q][0][1] if q < nq else -1 for q in range(3)]
        maxv = [tops[q][0][0] if q < nq else NEG_INF for q in range(3)]
        rec = dict(status=TICK_FAILED if failed else TICK_SCANNED, found=0, idx_curr=-1, idx_prev=-1, score=0.0, argmax=argmax, maxv=maxv)
        # Cerebro.cpp:1056  abs(u_argmax-um_argmax) < LOCALITY && abs(u_argmax-umm_argmax) < LOCALITY && u_max > THRESH
        if nq >= 3 and min(argmax) >= 0 and abs(argmax[0] - argmax[1]) < case.locality and abs(argmax[0] - argmax[2]) < case.locality \
                and maxv[0] > case.thresh:
            rec.update(found=1, idx_curr=case.l - 1, idx_prev=argmax[0], score=maxv[0])
    return sc, ix, rec


# ------------------------------------------------------------------------------------------------ reach model
def reach(lists, K):
    """the staging of one query: heads per wave of 64 lists, collisions in the upper 32 key bits, T1, survivors"""
    heads = [(j, l[0]) for j, l in enumerate(lists) if l is not FAILED and l]
    waves = {}
    for j, h in heads:
        waves.setdefault(j // 64, []).append(h)
    posted = []
    for hs in waves.values():
        posted += sorted(hs, key=key, reverse=True)[:K]     # a wave posts its K best heads
    nv = len(posted)
    T1 = sorted(posted, key=key, reverse=True)[K - 1] if nv >= K else None      # None: fewer than K heads, everything survives
    surv = []
    for j, h in heads:
        if T1 is not None and key(h) < key(T1):
            continue
        for e in lists[j]:                                     # sorted: the survivors of a list are a prefix
            if T1 is not None and key(e) < key(T1):
                break
            surv.append(e)
    return dict(valid_heads=[len(waves.get(w, [])) for w in range(MAX_LISTS // 64)],
                wave_collision=any(len({hi32(s) for s, _ in hs}) < len(hs) for hs in waves.values()),
                nv=nv, posted_collision=len({hi32(s) for s, _ in posted}) < nv, T1=T1, n=len(surv), survivors=surv)


# ------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    K: int
    queries: list                   # [nq] queries
    forms: tuple = (0,)
    l: int = TICK_L
    locality: int = LOCALITY
    thresh: float = THRESH
    kinds: tuple = ()
    _arrays: tuple = field(default=None, repr=False)

    @property
    def nq(self):
        return len(self.queries)

    @property
    def n_lists(self):
        return len(self.queries[0])

    def arrays(self):
        """(scores float64, idx int64), each [n_lists][nq][K]"""
        if self._arrays is None:
            sc = np.full((self.n_lists, self.nq, self.K), NEG_INF, dtype=np.float64)
            ix = np.full((self.n_lists, self.nq, self.K), -1, dtype=np.int64)
            for q, lists in enumerate(self.queries):
                for j, l in enumerate(lists):
                    if l is FAILED:
                        ix[j, q, :] = -2
                        continue
                    for r, (s, i) in enumerate(l):
                        sc[j, q, r] = s
                        ix[j, q, r] = i
            self._arrays = (sc, ix)
        return self._arrays


def check_contract(case):
    for lists in case.queries:
        assert len(lists) == case.n_lists and 1 <= case.n_lists <= MAX_LISTS and 1 <= case.K <= MAX_TOPK
        seen = set()
        for l in lists:
            if l is FAILED:
                continue
            assert len(l) <= case.K
            for a, b in zip(l, l[1:]):
                assert key(a) > key(b), (case.name, a, b)
            for s, i in l:
                assert not math.isnan(s) and i >= 0 and i not in seen, (case.name, s, i)
                seen.add(i)
    for q in case.queries[1:]:      # a failed shard's list is failed for every query
        assert [l is FAILED for l in q] == [l is FAILED for l in case.queries[0]]


def finish(lists, K):
    """every list sorted and cut to K entries"""
    return [l if l is FAILED else sorted(l, key=key, reverse=True)[:K] for l in lists]


def fresh_indices(rng, n):
    """n distinct indices; the upper 32 bits vary, so that the order of the low words alone is not the order"""
    return [int(i) + (int(h) << 32) for i, h in zip(rng.permutation(4 * n + 64)[:n], rng.integers(0, 3, n))]


def background(rng, n_lists, K, lo, hi, fill="full"):
    """distinct random scores in [lo, hi) dealt at random to the lists.  fill: entries per list -- full (K), random (0 .. K), sparse
    (most lists empty), alternate (full, empty, full, ...)"""
    if fill == "full":
        cnt = [K] * n_lists
    elif fill == "random":
        cnt = [int(c) for c in rng.integers(0, K + 1, n_lists)]
    elif fill == "sparse":
        cnt = [int(c) if rng.random() < 0.2 else 0 for c in rng.integers(1, K + 1, n_lists)]
    else:
        cnt = [K if j % 2 == 0 else 0 for j in range(n_lists)]
    n = sum(cnt)
    scores = rng.uniform(lo, hi, n)
    while len(set(scores.tolist())) < n:
        scores = rng.uniform(lo, hi, n)
    idx = fresh_indices(rng, n)
    lists, at = [], 0
    for c in cnt:
        lists.append([(float(scores[at + r]), idx[at + r]) for r in range(c)])
        at += c
    return lists


class Planter:
    """entries planted into a background; indices stay unique"""

    def __init__(self, rng, lists):
        self.lists = lists
        self.next = 1 << 40
        self.rng = rng

    def idx(self, n=1):
        """n fresh indices, ascending"""
        out = [self.next + 7 * r for r in range(n)]
        self.next += 7 * n + 1000
        return out

    def put(self, j, score, idx):
        self.lists[j].append((score, idx))

    def spread(self, n, wave=None):
        """n list positions: in wave `wave`, or (None) in different waves where there are several, else just different lists"""
        nl = len(self.lists)
        if wave is not None:
            lo, hi = 64 * wave, min(64 * wave + 64, nl)
            if lo >= hi:
                lo, hi = 0, min(64, nl)
            pool = list(range(lo, hi))
        else:
            pool = list(range(nl))
        self.rng.shuffle(pool)
        if wave is None:                        # one list per wave first
            seen, first, rest = set(), [], []
            for j in pool:
                (rest if j // 64 in seen else first).append(j)
                seen.add(j // 64)
            pool = first + rest
        return [pool[r % len(pool)] for r in range(n)]


def kind_a(rng, n_lists, K, neg=False):
    """a. distinct random scores, positive and negative, dealt at random"""
    return finish(background(rng, n_lists, K, -5.0, 5.0 if not neg else -1.0), K)


def kind_b(rng, n_lists, K, pos):
    """b. all K winners in one list (pos: an index, negative from the end)"""
    lists = background(rng, n_lists, K, -1.0, 1.0)
    j = pos % n_lists
    p = Planter(rng, lists)
    lists[j] = [(10.0 + r, i) for r, i in enumerate(p.idx(K))]
    return finish(lists, K)


def kind_c(rng, n_lists, K, full, wave=None):
    """c. K strong lists whose heads beat every other head.  One of them holds the lowest strong head h (= T1) and nothing else above it; `full`
    of the others hold K entries above h, the remaining K - 1 - full only their head: full * K + K - full survivors, K (K - 1) + 1 at most."""
    assert n_lists >= K and 0 <= full <= K - 1
    lists = background(rng, n_lists, K, -1.0, 1.0)
    p = Planter(rng, lists)
    strong = p.spread(K, wave)
    assert len(set(strong)) == K
    hi = iter(rng.permutation(K * K + 8).tolist())           # distinct values above h = 100
    ids = iter(rng.permutation(p.idx(K * K + K)).tolist())
    for r, j in enumerate(strong):
        tail = lists[j][:K - 1]
        if r == 0:
            lists[j] = [(100.0, next(ids))] + tail
        elif r <= full:
            lists[j] = [(101.0 + next(hi), next(ids)) for _ in range(K)]
        else:
            lists[j] = [(101.0 + next(hi), next(ids))] + tail
    return finish(lists, K)


def kind_d_ties(rng, n_lists, K):
    """d. the same score under different indices: 2K heads in different waves (the index decides which K are kept), and the same score again
    below a higher head"""
    lists = background(rng, n_lists, K, -1.0, 1.0)
    p = Planter(rng, lists)
    where = p.spread(2 * K + 2)
    ids = rng.permutation(p.idx(2 * K + 2)).tolist()
    for r, j in enumerate(where):
        if r < 2:
            p.put(j, 6.0 + r, p.idx()[0])     # a higher head: the tied entry of this list is no head
        p.put(j, 5.0, ids[r])
    return finish(lists, K)


def kind_d_flat(rng, n_lists, K):
    """d. every entry of every list the same score: the top-K is the K highest indices"""
    lists = background(rng, n_lists, K, 0.0, 1.0, "full")
    return finish([[(2.5, i) for _, i in l] for l in lists], K)


def kind_e(rng, n_lists, K, neg=False):
    """e. near-ties: groups of scores that agree in the upper 32 key bits and differ below, the larger score under the smaller index and the
    other way round: heads of one wave, heads of different waves, non-head entries.  neg: every score of the query negative."""
    lists = background(rng, n_lists, K, -9.0, -8.0) if neg else background(rng, n_lists, K, 0.0, 1.0)
    p = Planter(rng, lists)

    def group(base, where, below_head):
        ids = p.idx(len(where))                                # ascending
        for r, j in enumerate(where):
            if below_head:
                p.put(j, (-4.0 if neg else 32.0) + 0.25 * (r + 1), p.idx()[0])
            p.put(j, nudge(base, 1 + 3 * r), ids[r])              # |score| grows with the index ...
        ids = p.idx(len(where))
        for r, j in enumerate(where):
            p.put(j, nudge(base, 2 + 3 * r), ids[len(where) - 1 - r])   # ... and falls with it
    if neg:     # (everything else of the query lies below -8)
        group(-1.0, p.spread(3, wave=0), False)
        group(-1.5, p.spread(3), False)
        group(-6.0, p.spread(3), True)        # under heads of -3.75, -3.5, -3.25
    else:
        group(16.0, p.spread(3, wave=0), False)
        group(12.0, p.spread(3), False)
        group(8.0, p.spread(3), True)         # under heads of 32.25, 32.5, 32.75
    return finish(lists, K)


def kind_f_sparse(rng, n_lists, K, extra=0):
    """f. special values and little else: +inf, DBL_MAX, subnormals, +0.0 / -0.0 (equal scores: the index decides), valid entries scoring -inf
    (only the index tells them from padding)"""
    vals = [float("inf"), DBL_MAX, 1.0, SUBNORMAL, 0.0, -0.0, 0.0, -0.0, -SUBNORMAL, -1.0, -DBL_MAX, NEG_INF, NEG_INF]
    vals += [float(v) for v in rng.uniform(-0.5, 0.5, extra)]
    ids = fresh_indices(rng, len(vals))
    lists = [[] for _ in range(n_lists)]
    p = Planter(rng, lists)
    for v, i, j in zip(vals, ids, p.spread(len(vals))):
        if len(lists[j]) < K:
            p.put(j, v, i)
    return finish(lists, K)


def kind_f_dense(rng, n_lists, K):
    """f. the same special values as heads and entries among full random lists"""
    lists = background(rng, n_lists, K, -1.0, 1.0)
    p = Planter(rng, lists)
    vals = [float("inf"), DBL_MAX, SUBNORMAL, 0.0, -0.0, 0.0, -0.0, -SUBNORMAL, -DBL_MAX, NEG_INF, NEG_INF]
    for v, j in zip(vals, p.spread(len(vals))):
        lists[j] = lists[j][:K - 1]
        p.put(j, v, p.idx()[0])
    return finish(lists, K)


def kind_f_zeros(rng, n_lists, K, wave=None):
    """f. one +0.0 and one -0.0 head as the LAST two of the K winners, -0.0 under the higher index, and nothing else in the query that shares
    upper key bits (no second zero of either sign, no -inf next to padding): only the equal image of the two zeros sends the ranking to the
    exact comparison, where the index decides"""
    lists = [[] for _ in range(n_lists)]
    p = Planter(rng, lists)
    i0, i1 = p.idx(2)
    ents = [(1.0 + r, i) for r, i in enumerate(p.idx(max(K - 2, 0)))] + [(0.0, i0), (-0.0, i1)]
    ents += [(-1.0 - r, i) for r, i in enumerate(p.idx(6))]
    for (v, i), j in zip(ents, p.spread(len(ents), wave)):
        if len(lists[j]) < K:
            p.put(j, v, i)
    return finish(lists, K)


def kind_g(rng, n_lists, K, what):
    """g. short and empty lists"""
    if what in ("random", "sparse", "alternate"):
        return finish(background(rng, n_lists, K, -5.0, 5.0, what), K)
    total = {"K": K, "K-1": K - 1, "one": 1, "none": 0, "K-onewave": K, "K-onelist": K}[what]
    lists = [[] for _ in range(n_lists)]
    p = Planter(rng, lists)
    scores = rng.permutation(total + 3)[:total]
    where = p.spread(total, wave=1 if what == "K-onewave" else None)
    if what == "K-onelist":
        where = [where[0]] * total
    for s, i, j in zip(scores, p.idx(total), where):
        if len(lists[j]) < K:
            p.put(j, float(s) - 2.0, i)
    return finish(lists, K)


def with_failed(lists, pos):
    out = list(lists)
    out[pos % len(lists)] = FAILED
    return out


def c_full(K, which):
    """`full` of kind_c for: max -> K (K - 1) + 1 survivors; mid / low -> at K = 16, 166 and 106 (129-192 and 65-128)"""
    return {"max": K - 1, "mid": max(0, (5 * K) // 8), "low": max(0, (3 * K) // 8)}[which]


def _seed(*parts):
    h = 0
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % (1 << 32)
    return h


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []

    def add(name, K, builders, forms, kinds, **kw):
        """builders: per query a function (rng) -> query"""
        rng = np.random.default_rng(_seed(name))
        c = Case(name=name, K=K, queries=[b(rng) for b in builders], forms=forms, kinds=(kinds,), **kw)
        cases.append(c)
        return c

    # ---- every content kind at n_lists 65 and 512 and at K 8 and 16: four queries, both kernels
    for n in (65, 512):
        for K in (8, 16):
            t = f"n{n}_K{K}"
            wave7 = 7 * 64 + 5 if n > 7 * 64 + 5 else n - 2
            add(f"a_{t}", K, [lambda r: kind_a(r, n, K), lambda r: kind_a(r, n, K, True), lambda r: kind_a(r, n, K), lambda r: kind_a(r, n, K, True)],
                (0, 1), "a")
            add(f"b_{t}", K, [lambda r: kind_b(r, n, K, 0), lambda r: kind_b(r, n, K, -1), lambda r: kind_b(r, n, K, wave7),
                              lambda r: kind_b(r, n, K, 64)], (0, 1), "b")
            add(f"c_{t}", K, [lambda r: kind_c(r, n, K, c_full(K, "max")), lambda r: kind_c(r, n, K, c_full(K, "mid")),
                              lambda r: kind_c(r, n, K, c_full(K, "low")), lambda r: kind_c(r, n, K, c_full(K, "max"), wave=n // 64 - 1 if n >= 128 else 0)],
                (0, 1), "c")
            add(f"d_{t}", K, [lambda r: kind_d_ties(r, n, K), lambda r: kind_d_flat(r, n, K), lambda r: kind_d_ties(r, n, K),
                              lambda r: kind_d_flat(r, n, K)], (0, 1), "d")
            add(f"e_{t}", K, [lambda r: kind_e(r, n, K), lambda r: kind_e(r, n, K, True), lambda r: kind_e(r, n, K, True),
                              lambda r: kind_e(r, n, K)], (0, 1), "e")
            add(f"f_{t}", K, [lambda r: kind_f_sparse(r, n, K), lambda r: kind_f_dense(r, n, K), lambda r: kind_f_zeros(r, n, K),
                              lambda r: kind_f_zeros(r, n, K, wave=0)], (0, 1), "f")
            add(f"f2_{t}", K, [lambda r: kind_f_sparse(r, n, K, extra=12), lambda r: kind_f_dense(r, n, K), lambda r: kind_f_zeros(r, n, K, wave=1),
                               lambda r: kind_f_sparse(r, n, K)], (0, 1), "f")
            add(f"g1_{t}", K, [lambda r: kind_g(r, n, K, "random"), lambda r: kind_g(r, n, K, "alternate"), lambda r: kind_g(r, n, K, "K"),
                               lambda r: kind_g(r, n, K, "K-1")], (0, 1), "g")
            add(f"g2_{t}", K, [lambda r: kind_g(r, n, K, "one"), lambda r: kind_g(r, n, K, "none"), lambda r: kind_g(r, n, K, "K-onewave"),
                               lambda r: kind_g(r, n, K, "sparse")], (0, 1), "g")
            add(f"g3_{t}", K, [lambda r: kind_g(r, n, K, "K-onelist"), lambda r: kind_g(r, n, K, "none"), lambda r: kind_g(r, n, K, "none"),
                               lambda r: kind_g(r, n, K, "one")], (0, 1), "g")
            for pos, tag in ((0, "first"), (-1, "last"), (64, "wave1")):
                add(f"h_{tag}_{t}", K, [lambda r: with_failed(kind_a(r, n, K), pos), lambda r: with_failed(kind_g(r, n, K, "random"), pos),
                                        lambda r: with_failed(kind_d_ties(r, n, K), pos), lambda r: with_failed(kind_g(r, n, K, "none"), pos)],
                    (0, 1), "h")
            # i. a different kind per query, one empty, one at maximal survivors: the per-query LDS regions must not bleed
            add(f"i4_{t}", K, [lambda r: kind_g(r, n, K, "none"), lambda r: kind_c(r, n, K, K - 1), lambda r: kind_e(r, n, K, True),
                               lambda r: kind_f_sparse(r, n, K)], (0, 1), "i")
            if (n, K) != (512, 16):      # (keeps every input at a few hundred KiB)
                add(f"i8_{t}", K, [lambda r: kind_a(r, n, K), lambda r: kind_g(r, n, K, "none"), lambda r: kind_c(r, n, K, K - 1),
                                   lambda r: kind_d_flat(r, n, K), lambda r: kind_e(r, n, K), lambda r: kind_g(r, n, K, "random"),
                                   lambda r: kind_f_dense(r, n, K), lambda r: kind_c(r, n, K, K - 1)], (1,), "i")
    for K in (8, 16):       # the failed list alone
        add(f"h_alone_K{K}", K, [lambda r: [FAILED]] * 4, (0, 1), "h")
        add(f"h_alone_K{K}_nq1", K, [lambda r: [FAILED]], (0,), "h")
    add("h_last_n129_K5_nq3", 5, [lambda r: with_failed(kind_a(r, 129, 5), -1), lambda r: with_failed(kind_d_ties(r, 129, 5), -1),
                                  lambda r: with_failed(kind_a(r, 129, 5), -1)], (0,), "h")

    # ---- every n_lists x every K, NQ 1 .. 4 in turn (form 0; the four-query ones through topk_merge_batch as well, every third as nq = 8)
    count = 0
    for n in N_LISTS:
        for K in KS:
            nq = 1 + count % 4
            menu = [lambda r: kind_a(r, n, K), lambda r: kind_d_ties(r, n, K), lambda r: kind_e(r, n, K, count % 2 == 1),
                    lambda r: kind_g(r, n, K, "random"), lambda r: kind_b(r, n, K, -1), lambda r: kind_f_dense(r, n, K),
                    lambda r: kind_d_flat(r, n, K), (lambda r: kind_c(r, n, K, K - 1)) if n >= K else (lambda r: kind_a(r, n, K, True))]
            builders = [menu[(count + q) % len(menu)] for q in range(nq)]
            add(f"sweep_n{n}_K{K}_nq{nq}", K, builders, (0, 1) if nq == 4 else (0,), "s")
            if nq == 4 and count % 3 == 0:
                add(f"sweep8_n{n}_K{K}", K, [menu[(count + 3 + q) % len(menu)] for q in range(8)], (1,), "s")
            count += 1

    # ---- the accept rule (form 0, NQ = 3): |argmax0 - argmax1|, |argmax0 - argmax2| at locality - 1 and locality, maxv[0] at thresh and
    # the next double above it, a query with no valid entry
    above = math.nextafter(THRESH, math.inf)
    for name, d1, d2, top, empty in [("near_near_above", LOCALITY - 1, LOCALITY - 1, above, None), ("near_near_neg", -(LOCALITY - 1), -(LOCALITY - 1), above, None),
                                     ("near_mixed_above", LOCALITY - 1, -(LOCALITY - 1), above, None),
                                     ("far_near_above", LOCALITY, LOCALITY - 1, above, None), ("near_far_above", LOCALITY - 1, LOCALITY, above, None),
                                     ("near_farneg_above", LOCALITY - 1, -LOCALITY, above, None), ("farneg_near_above", -LOCALITY, LOCALITY - 1, above, None),
                                     ("near_near_thresh", LOCALITY - 1, LOCALITY - 1, THRESH, None), ("near_near_below", 1, 0, math.nextafter(THRESH, 0.0), None),
                                     ("empty_q0", 1, 1, above, 0), ("empty_q1", 1, 1, above, 1), ("empty_q2", 1, 1, above, 2),
                                     ("same_row", 0, 0, 1.0, None)]:
        for n, K in ((65, 8), (3, 1), (512, 16)):
            a0 = 5000

            def q(r, top_idx, top_score, is_empty, n=n, K=K):
                if is_empty:
                    return [[] for _ in range(n)]
                lists = background(r, n, K, 0.0, 0.5)        # (indices below 2**35 + ..., never a0 +- 12: fresh_indices are < 4 n K + 64 + multiples of 2**32)
                lists = [[e for e in l if abs((e[1] & 0xFFFFFFFF) - a0) > 2 * LOCALITY or e[1] >> 32] for l in lists]
                j = int(r.integers(0, n))
                lists[j] = lists[j][:K - 1] + [(top_score, top_idx)]
                return finish(lists, K)
            add(f"accept_{name}_n{n}_K{K}", K, [lambda r: q(r, a0, top, empty == 0), lambda r: q(r, a0 - d1, 0.75, empty == 1),
                                               lambda r: q(r, a0 - d2, 0.75, empty == 2)], (0,), "accept")
    for c in cases:
        check_contract(c)
    assert len({c.name for c in cases}) == len(cases)
    return cases
