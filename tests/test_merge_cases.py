"""The crafted list sets of tests/merge_cases.py on the CPU: the selection argument of the merge holds on them (the exact top-K lies within
the survivors of the staging), and the set REACHES the paths of csrc/topk_merge.h it was written for -- conditions on the inputs, so that
tests/test_merge_gpu.py cannot pass by never entering a path."""
import numpy as np
import pytest

import merge_cases as mc


@pytest.fixture(scope="module")
def reached():
    """per (case, query): the reach model's report"""
    return [(c, q, mc.reach(lists, c.K)) for c in mc.all_cases() for q, lists in enumerate(c.queries)]


def test_okey_is_order_preserving():
    vals = [float("-inf"), -mc.DBL_MAX, -1.0, mc.nudge(-1.0, -1), -mc.SUBNORMAL, 0.0, mc.SUBNORMAL, 1.0, mc.nudge(1.0, 1), mc.DBL_MAX, float("inf")]
    keys = [mc.okey(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert mc.okey(-0.0) == mc.okey(0.0)
    assert mc.hi32(mc.nudge(16.0, 9)) == mc.hi32(16.0) and mc.hi32(mc.nudge(-6.0, 9)) == mc.hi32(-6.0) and mc.nudge(-6.0, 9) < -6.0


def test_shapes_cover_every_axis_value():
    cases = mc.all_cases()
    assert {c.n_lists for c in cases} >= set(mc.N_LISTS)
    assert {c.K for c in cases} >= set(mc.KS)
    assert {c.nq for c in cases if 0 in c.forms} == {1, 2, 3, 4}
    assert {c.nq for c in cases if 1 in c.forms} == {4, 8}
    for kind in "abcdefghi":
        for n in (65, 512):
            for K in (8, 16):
                assert any(c.kinds == (kind,) and c.n_lists == n and c.K == K for c in cases), (kind, n, K)
    for c in cases:
        sc, ix = c.arrays()
        assert sc.nbytes + ix.nbytes <= 1 << 20
        assert c.nq in (1, 2, 3, 4) if 0 in c.forms else c.nq % 4 == 0


def test_top_k_lies_within_the_survivors(reached):
    for c, q, r in reached:
        surv = set(r["survivors"])
        assert len(surv) == r["n"]                                   # (indices are unique: no entry twice)
        top = [e for e in mc.reference_query(c.queries[q], c.K) if e[1] >= 0]
        assert all(e in surv for e in top), (c.name, q)
        assert r["n"] <= c.K * (c.K - 1) + 1 <= 241, (c.name, q, r["n"])


def test_case_set_reaches_the_paths_it_claims(reached):
    n16 = [r["n"] for c, q, r in reached if c.K == 16]
    assert any(r["wave_collision"] for _, _, r in reached)              # wave_rank falls back to the exact comparison
    assert any(r["posted_collision"] for _, _, r in reached)            # wave_rank2 does
    assert any(r["posted_collision"] and not r["wave_collision"] for _, _, r in reached)   # ... with heads that collide only across waves
    assert any(0 < r["nv"] < c.K for c, _, r in reached)                # fewer than K heads: everything survives
    assert any(r["nv"] == 0 for _, _, r in reached)
    for lo, hi in ((1, 64), (65, 128), (129, 192), (193, 241)):          # the four survivor slots of a lane
        assert any(lo <= n <= hi for n in n16), (lo, hi)
    assert 241 in n16 and max(n16) == 241
    assert any(0 < r["n"] < c.K for c, _, r in reached)                 # padding behind valid entries
    assert any(r["n"] == 0 for _, _, r in reached)
    assert any(r["n"] == c.K for c, _, r in reached) and any(r["n"] == c.K - 1 and c.K > 1 for c, _, r in reached)
    # more than one wave of heads in both kernels, and the second workgroup of the many-query merge
    assert any(1 in c.forms and sum(v > 0 for v in r["valid_heads"]) == 8 for c, _, r in reached)
    assert any(1 in c.forms and c.nq == 8 and q >= 4 and r["n"] == 241 for c, q, r in reached)
    # i. an empty query next to one at maximal survivors, in both kernels
    for form in (0, 1):
        assert any(form in c.forms and {0, c.K * (c.K - 1) + 1} <= {mc.reach(l, c.K)["n"] for l in c.queries} for c in mc.all_cases() if c.kinds == ("i",))


def test_case_contents_are_what_their_kind_says():
    by = {c.name: c for c in mc.all_cases()}
    # c. the three survivor counts at K = 16
    assert [mc.reach(l, 16)["n"] for l in by["c_n512_K16"].queries] == [241, 166, 106, 241]
    # e. near-ties: the larger score under the smaller index AND under the larger one, among the winners, for positive and negative scores
    for q in (0, 1):
        top = mc.reference_query(by["e_n512_K16"].queries[q], 16)
        pairs = [(a, b) for a, b in zip(top, top[1:]) if mc.hi32(a[0]) == mc.hi32(b[0]) and a[0] != b[0]]
        assert any(a[1] < b[1] for a, b in pairs) and any(a[1] > b[1] for a, b in pairs), q
        assert all(e[0] < 0 for e in top) == (q == 1)
    # d. equal scores: the K highest indices win
    flat = by["d_n65_K8"].queries[1]
    assert [e[1] for e in mc.reference_query(flat, 8)] == sorted((e[1] for l in flat for e in l), reverse=True)[:8]
    # f. -0.0 and +0.0 among the winners in index order, a valid -inf entry in the output next to padding
    for q in (2, 3):     # the two zeros are the only heads that share upper key bits, and they are the last two winners
        lists = by["f_n65_K8"].queries[q]
        r = mc.reach(lists, 8)
        heads = [l[0] for l in lists if l]
        assert len({mc.hi32(s) for s, _ in heads}) == len(heads) - 1 and sum(s == 0.0 for s, _ in heads) == 2
        assert not any(s == mc.NEG_INF for s, _ in heads) and r["T1"][0] == 0.0 and not np.signbit(r["T1"][0]) and r["posted_collision"]
        top = mc.reference_query(lists, 8)
        assert [bool(np.signbit(s)) for s, _ in top[6:]] == [True, False] and top[6][0] == top[7][0] == 0.0 and top[6][1] > top[7][1]
    top = mc.reference_query(by["f_n65_K16"].queries[0], 16)
    zeros = [e for e in top if e[0] == 0.0]
    assert len(zeros) == 4 and [e[1] for e in zeros] == sorted((e[1] for e in zeros), reverse=True)
    assert {np.signbit(e[0]) for e in zeros} == {True, False}
    assert [e for e in top if e[0] == mc.NEG_INF and e[1] >= 0] and top[-1] == (mc.NEG_INF, -1)
    # the accept rule: found exactly where both distances are below the locality and the score above the threshold
    found = {c.name: mc.reference(c, 0)[2]["found"] for c in mc.all_cases() if c.kinds == ("accept",) and c.n_lists == 65}
    assert found == {f"accept_{k}_n65_K8": v for k, v in dict(near_near_above=1, near_near_neg=1, near_mixed_above=1, far_near_above=0, near_far_above=0,
                                                              near_farneg_above=0, farneg_near_above=0, near_near_thresh=0, near_near_below=0, empty_q0=0,
                                                              empty_q1=0, empty_q2=0, same_row=1).items()}
    r = mc.reference(by["accept_empty_q1_n65_K8"], 0)[2]
    assert r["argmax"][1] == -1 and r["maxv"][1] == mc.NEG_INF and r["argmax"][0] == 5000
    r = mc.reference(by["accept_near_near_thresh_n65_K8"], 0)[2]
    assert r["maxv"][0] == mc.THRESH and r["argmax"] == [5000, 5000 - 11, 5000 - 11]
    # h. the failed list: the mark, the status, and the others merged as if it were empty
    c = by["h_first_n65_K8"]
    sc, ix, rec = mc.reference(c, 0)
    assert ix[0, 0] == -2 and rec["status"] == mc.TICK_FAILED and ix[1, 0] >= 0
    assert mc.reference_query(c.queries[1], 8) == mc.reference_query([[]] + c.queries[1][1:], 8)
