"""CPU tests of what chip_loop_ticks_bulk rests on: the certificate over the GEMM's list of KL fp32 fmaf-chain scores.
  * wherever the mirror (tests/np_mirror_bulk_ticks.py) says "certified", its top-topk IS exact selection over the whole prefix, bit for
    bit -- on random unit rows, on rows with runs of near-copies (where some queries do not certify), and on the crafted cases;
  * the crafted cases of tests/test_bulk_ticks_gpu.py sit on the side of M < thr they claim;
  * the mis-ordering case really is mis-ordered in fp32."""
import numpy as np
import pytest

import np_mirror_bulk_ticks as nm
import oracle_lib

D, KL = 64, 16


def unit_rows(rng, n, d=D):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x.astype(np.float64), axis=1)[:, None]).astype(np.float32)


def norm_bound(db):
    return float(np.sqrt((db.astype(np.float64) ** 2).sum(1).max())) * (1.0 + 2.0 ** -30)


def check_certified_is_exact(db, ticks, topk, E, lag=50):
    n_cert = n_unc = 0
    for l in ticks:
        k = l - lag
        t = nm.tick(db, l, k, KL, topk, E)
        es, ei = oracle_lib.scan_topk(db, k, db[[l - 1, l - 2, l - 3]], topk)
        for j in range(3):
            if t["q"][j]["certified"]:
                assert (t["s"][j].view(np.int64) == es[j].view(np.int64)).all() and (t["i"][j] == ei[j]).all(), (l, j)
                assert len(t["q"][j]["R"]) <= KL
        n_cert += t["certified"]
        n_unc += not t["certified"]
    return n_cert, n_unc


@pytest.mark.parametrize("topk", [1, 5, 8])
def test_certified_lists_are_exact_on_unit_rows(topk):
    db = unit_rows(np.random.default_rng(11), 500)
    E = nm.error_bound(D, norm_bound(db))
    n_cert, n_unc = check_certified_is_exact(db, range(57, 500, 9), topk, E)
    assert n_cert > 0 and n_unc == 0                       # unit rows of 64 elements are nowhere near 2 E of one another


def test_runs_of_near_copies_certify_some_and_not_others():
    rng = np.random.default_rng(5)
    db = unit_rows(rng, 400)
    db[100:130] = db[100]                                  # thirty identical rows: more than KL within 2 E of the best for a query close to them
    db[300] = db[100]
    db[299] = db[100]
    db[298] = db[100]
    E = nm.error_bound(D, norm_bound(db))
    n_cert, n_unc = check_certified_is_exact(db, [301, 250, 200, 170], 8, E)
    t = nm.tick(db, 301, 251, KL, 8, E)
    assert not t["certified"] and t["q"][0]["dropped"] and t["q"][0]["M"] >= t["q"][0]["thr"]
    assert n_unc >= 1 and n_cert >= 1


# ---- the crafted cases of the GPU test: one-hot queries, rows x e_0 -- the fp32 score and the exact score of a row are both exactly x
def one_hot_db(x, n_query=3):
    """rows x[i] e_0 followed by n_query rows e_0 (the tick's queries, beyond the prefix)"""
    db = np.zeros((len(x) + n_query, D), np.float32)
    db[:len(x), 0] = x
    db[len(x):, 0] = 1.0
    return db


def crafted_tick(x, topk=1):
    db = one_hot_db(np.asarray(x, np.float32))
    E = nm.error_bound(D, norm_bound(db))
    l = len(db)
    return nm.tick(db, l, len(x), KL, topk, E), E, db


TOP = [3, 17, 18, 40, 41, 42, 77, 90, 91, 120, 133, 150, 151, 180, 190, 199]      # KL rows of a prefix of 200


def test_equal_rows_at_the_top_of_a_long_prefix():
    """KL - 1 equal rows at the top, the rest far below: the KL-th entry is one of the rest, M < thr, certified with |R| = KL - 1.  KL equal rows
    fill the list: M IS their score, and M < G - 2 E cannot hold -- a list of KL entries does not say what lies below its last one -- so the
    tick is not certified (and runs again exactly); the rows it would have ranked are those KL, the highest index first."""
    assert len(TOP) == KL
    x = np.full(200, -1.0, np.float32)
    x[TOP[:-1]] = 0.5
    t, E, db = crafted_tick(x)
    assert t["certified"] and t["record"]["argmax"] == [TOP[-2]] * 3
    for q in t["q"]:
        assert q["dropped"] and q["M"] == -1.0 and q["G"] == 0.5 and len(q["R"]) == KL - 1
    x[TOP] = 0.5
    t, E, db = crafted_tick(x)
    assert not t["certified"] and t["record"]["argmax"] == [TOP[-1]] * 3
    for q in t["q"]:
        assert q["dropped"] and q["M"] == 0.5 and q["G"] == 0.5 and len(q["R"]) == KL and not q["M"] < q["thr"]


def test_sides_of_the_certificate():
    """A prefix of exactly KL rows leaves the last slot used and nothing below it: the mirror (like the kernel) cannot tell, and says "not
    certified" only where M >= thr.  KL rows at the top of which the KL-th is below thr certify; at or above thr they do not."""
    # KL - 1 rows in the prefix, all equal: the last slot is unused, nothing was dropped -> certified, winner = the highest index
    t, E, _ = crafted_tick(np.full(KL - 1, 0.5, np.float32))
    assert t["certified"] and [len(q["R"]) for q in t["q"]] == [KL - 1] * 3 and t["record"]["argmax"] == [KL - 2] * 3
    assert not t["q"][0]["dropped"]
    # KL and KL + 1 equal rows: the last slot is used at the score of the best -> not certified
    for n in (KL, KL + 1):
        t, E, _ = crafted_tick(np.full(n, 0.5, np.float32))
        assert not t["certified"] and t["q"][0]["dropped"] and t["q"][0]["M"] == 0.5 and t["record"]["argmax"] == [n - 1] * 3
    # a long prefix: the top row G, then KL - 1 rows at m, everything else far below.  m one float below thr certifies, at thr does not.
    G = np.float32(0.9)
    _, E, _ = crafted_tick(np.full(100, -1.0, np.float32))
    thr = nm.threshold(G, E)
    f = np.float32(thr)
    below, at = (np.nextafter(f, np.float32(-1)), f) if np.float64(f) >= thr else (f, np.nextafter(f, np.float32(1)))
    assert np.float64(below) < thr <= np.float64(at) and np.nextafter(below, np.float32(1)) == at and at < G
    for m, want in ((below, True), (at, False)):
        x = np.full(100, -1.0, np.float32)
        x[50] = G
        x[10:10 + KL - 1] = m
        t, E2, _ = crafted_tick(x)
        assert E2 == E and t["certified"] == want, (float(m), thr)
        q = t["q"][0]
        assert q["G"] == float(G) and q["M"] == float(m) and q["dropped"] and len(q["R"]) == (1 if want else KL)
        assert t["record"]["argmax"] == [50] * 3 and t["record"]["found"] == 1


def misordered_db():
    """rows a (index 5) and b (index 9) and the query q = e_0 + e_1 + e_2 + e_3 (norm 2, the largest): the fp32 chain gives a . q = 1 (each
    2^-24 added to 1 is a tie that rounds to even) and b . q = 1 + 2^-23, the exact scores are 1 + 3 2^-24 and 1 + 2^-23."""
    db = np.zeros((70, D), np.float32)
    db[:, 4] = -0.25                                       # background rows: score 0 against q
    db[5, :4] = [1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]
    db[9, 0] = 1.0 + 2.0 ** -23
    db[60:, :] = 0
    db[60:, :4] = 1.0                                      # rows 60 .. 69: the queries of the ticks at l = 63 .. 70 (lag 50: prefixes 13 .. 20)
    return db


def test_the_misordering_case_is_misordered_in_fp32():
    db = misordered_db()
    q = db[[62]]
    fs, fi = oracle_lib.scan_topk_fmaf(db, 13, q, 2)
    es, ei = oracle_lib.scan_topk(db, 13, q, 2)
    assert fi[0].tolist() == [9, 5] and fs[0].tolist() == [1.0 + 2.0 ** -23, 1.0]          # the chain puts b first ...
    assert ei[0].tolist() == [5, 9] and es[0].tolist() == [1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -23]   # ... the exact order a, at the lower index
    E = nm.error_bound(D, norm_bound(db))
    t = nm.tick(db, 63, 13, KL, 1, E)
    assert t["certified"] and t["rescored"] >= 6 and t["record"]["argmax"] == [5] * 3 and t["record"]["maxv"][0] == 1.0 + 3 * 2.0 ** -24
