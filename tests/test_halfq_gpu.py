"""GPU tests of the five-tick pass: five pipelined ticks share one fp32 pass over the DB whose 15 queries are staged in LDS as fp16
(cerebro_amd/csrc/kernels.hip db_scan_halfq), tick_rescore proves per query which rows can be in the exact top-8 and scores those in fp64
(with the bound E_h).  The bar is the one of test_prefilter_gpu.py: every 64-byte decision record of a window of five
forced-parked ticks equals, byte for byte, the record of the same tick issued alone with coalescing off, one per window the CPU oracle's --
where the certificate holds AND where it does not.  CHIP_SCAN_OVERLAP_GIB=0 makes every scan a long one, parking is forced."""
import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi
from test_prefilter_gpu import (A_IDX, B_IDX, DUP_HI, DUP_LO, K_TIE, L0, N_ROWS, PLANTS, SEED, alone_records, every_tick_params, make_chip, rec,
                                run_window)

pytestmark = pytest.mark.gpu
E_SCALE = 14                     # the exponent these DBs get: their largest row norm lies in (1, 2)


def halfq_two_terms(x1, q1, x2, q2, e=E_SCALE):
    """what db_scan_halfq computes for a row that is zero but for elements 0 and 2: the query elements staged as fl16(2^e q), both products
    through the low half of lane 0's accumulator by fma -- fl(x2 h2 + fl(x1 h1)) --, every other addition adds a zero; then 2^-e (exact).
    (x h and x2 h2 + acc are exact in fp64 for the magnitudes used here, so one conversion is the one rounding of each fma.)"""
    h1 = np.float64((np.float32(q1) * np.float32(2.0 ** e)).astype(np.float16))
    h2 = np.float64((np.float32(q2) * np.float32(2.0 ** e)).astype(np.float16))
    acc = (np.asarray(x1, np.float64) * h1).astype(np.float32)
    return (np.asarray(x2, np.float64) * h2 + acc.astype(np.float64)).astype(np.float32).astype(np.float64) * 2.0 ** -e


def near_tie_rows():
    """(a, b, q, exact_a, exact_b): rows a = (a1, 0, a2, 0, ...), b likewise, and the query's elements 0 and 2 (the existing construction), such
    that the exact scores differ by less than one fp32 ulp of the sum with a ahead, and the scores of the pass -- query rounded to fp16,
    fp32 sum -- are in the opposite order."""
    q1, q2 = np.float32(0.5) * np.float32(1 + 2.0 ** -12 + 2.0 ** -21), np.float32(-0.5) * np.float32(1 + 2.0 ** -9)
    rng = np.random.default_rng(5)
    x1 = (1 + rng.integers(0, 1 << 12, 200_000) * 2.0 ** -23).astype(np.float32)
    x2 = (0.5 + rng.integers(0, 1 << 12, 200_000) * 2.0 ** -24).astype(np.float32)
    exact = x1.astype(np.float64) * np.float64(q1) + x2.astype(np.float64) * np.float64(q2)     # exact: both products and their sum fit 53 bits
    approx = halfq_two_terms(x1, q1, x2, q2)
    order = np.argsort(exact)
    lo, hi = order[:-1], order[1:]
    ulp = np.spacing(np.abs(approx[hi]).astype(np.float32)).astype(np.float64)
    ok = (exact[hi] > exact[lo]) & (exact[hi] - exact[lo] < ulp) & (approx[hi] < approx[lo])
    i = int(np.flatnonzero(ok)[0])
    a, b = int(hi[i]), int(lo[i])
    return (x1[a], x2[a]), (x1[b], x2[b]), (q1, q2), float(exact[a]), float(exact[b])


_DB = {}


def build_db(D):
    """the synthetic rows with the near-tie pair and its query planted; float32 [N_ROWS, D]"""
    if D not in _DB:
        db = np.ascontiguousarray(oracle_lib.synth_rows(SEED, range(N_ROWS), D, PLANTS), dtype=np.float32)
        a, b, q, ea, eb = near_tie_rows()
        db[A_IDX] = 0
        db[B_IDX] = 0
        db[A_IDX, 0], db[A_IDX, 2] = a
        db[B_IDX, 0], db[B_IDX, 2] = b
        db[K_TIE + 49, 0], db[K_TIE + 49, 2] = q
        db.setflags(write=False)
        _DB[D] = (db, a, b, q, ea, eb)
    return _DB[D]


@pytest.mark.parametrize("D", [4096, 1024])
def test_windows_of_five_equal_ticks_issued_alone(monkeypatch, D):
    db, a, b, q, ea, eb = build_db(D)
    # the near-tie pair, on the CPU first: exact scores less than one fp32 ulp apart with row A ahead, the pass's scores the other way round
    sa, sb = float(halfq_two_terms(a[0], q[0], a[1], q[1])), float(halfq_two_terms(b[0], q[0], b[1], q[1]))
    assert ea > eb and ea - eb < np.spacing(np.float32(sa)) and sa < sb
    qrow = db[K_TIE + 49].astype(np.float64)
    assert float(db[A_IDX].astype(np.float64) @ qrow) == ea and float(db[B_IDX].astype(np.float64) @ qrow) == eb
    others = np.delete(db[:K_TIE].astype(np.float64) @ qrow, [A_IDX, B_IDX])
    assert others.max() < eb - 0.01                  # the pair is the top two of that query: the exact order decides the record

    p = every_tick_params()
    plan = capi.halfq_plan(D)
    with make_chip(monkeypatch, D, db) as chip:
        assert chip.info()["storage_bytes"] == 4
        assert capi.halfq_bound(D, chip.info()["row_norm_max"])[0] == E_SCALE
        ls, _ = run_window(chip, [L0, L0 + 3, L0 + 6, L0 + 9, L0 + 12], p)         # the geometry, from a first window
        assert (ls["family"], ls["ticks"], ls["R"], ls["nq"], ls["elem"], ls["NG"], ls["lds_bytes"]) == \
            ("halfq", 5, 4, 15, 4, 0, plan["lds_bytes"]), ls
        W, R = ls["grid"] * ls["block"] // 64, ls["R"]
        P = R * W
        assert 2 * P + 100 < N_ROWS
        windows = [[P - 2, P + 1, P + 4, 2 * P, P - 1], [2 * P + 4, 2 * P - 2, P, 2 * P + 1, 2 * P - 1],                   # both sides of a pass boundary
                   [10, W + 3, N_ROWS - 50, P - 1, 9], [N_ROWS - 50, 10, W - 1, 11, N_ROWS - 51],                         # lists not full; the whole DB
                   [DUP_HI + 1, DUP_HI - 1, DUP_HI + 4, DUP_HI, DUP_HI + 2], [DUP_HI, DUP_HI + 1, N_ROWS - 50, DUP_HI + 2, DUP_HI - 2],   # the duplicate pair
                   [K_TIE, K_TIE + 3, A_IDX, K_TIE - 3, K_TIE + 6]]                                                       # the near tie; a prefix that ends before row A
        all_l = sorted({k + 50 for w in windows for k in w})
        alone = alone_records(monkeypatch, D, db, all_l, p)
        # what the planted rows are there for, in the reference records themselves
        assert list(rec(alone[DUP_HI + 1 + 50]).argmax) == [DUP_HI] * 3 and list(rec(alone[DUP_HI + 50]).argmax) == [DUP_LO] * 3
        r = rec(alone[K_TIE + 50])
        assert r.argmax[0] == A_IDX and float(r.maxv[0]).hex() == ea.hex()
        op = oracle_lib.default_params()
        op.min_new = -(1 << 30)
        launches = chip.last_scan()["launches"]
        before = chip.prefilter_stats()
        for w in windows:
            ls, got = run_window(chip, w, p)
            launches += 1
            assert (ls["family"], ls["ticks"], ls["n_rows"], ls["launches"]) == ("halfq", 5, max(w), launches), (w, ls)
            assert got == [alone[k + 50] for k in w], (w, [i for i, k in enumerate(w) if got[i] != alone[k + 50]])
            k = min(w)
            o = oracle_lib.LoopOracle(db, op).tick(k + 50)
            r = rec(got[w.index(k)])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
        passes, ticks, unc = (x - y for x, y in zip(chip.prefilter_stats(), before))
        # Gaussian scores: the gap between the K-th score and the best dropped one (about 0.8 sigma at these sizes) is several times 2 E_h
        # (0.16 sigma at D = 4096, less at D = 1024: DESIGN.md 3), and a tie of two rows is two candidates: every tick certifies
        assert (passes, ticks, unc) == (len(windows), 5 * len(windows), 0), (passes, ticks, unc)
        assert chip.coalesce_stats()[0] >= len(windows)

        # a window of four is the fp32 prefilter pass, windows of two and three the fp64 pass, as before
        w = windows[0][:4]
        before = chip.prefilter_stats()
        ls, got = run_window(chip, w, p)
        assert (ls["family"], ls["ticks"], ls["nq"]) == ("prefilter", 4, 12), ls
        assert got == [alone[k + 50] for k in w]
        assert tuple(x - y for x, y in zip(chip.prefilter_stats(), before)) == (1, 4, 0)
        for w in (windows[0][:2], windows[0][:3]):
            ls, got = run_window(chip, w, p)
            assert (ls["family"], ls["ticks"]) == ("multi", len(w)), ls
            assert got == [alone[k + 50] for k in w]

        # a row scaled by 1000, beyond every prefix: the norm bound grows, the error bound swamps every gap, no tick certifies
        big = (db[123].astype(np.float32) * np.float32(1000.0))[None, :]
        chip.append_f32(np.ascontiguousarray(big))
        assert capi.halfq_bound(D, chip.info()["row_norm_max"])[0] == 5
        before = chip.prefilter_stats()
        ls, got = run_window(chip, windows[0], p)
        assert (ls["family"], ls["ticks"]) == ("halfq", 5) and got == [alone[k + 50] for k in windows[0]]
        assert tuple(x - y for x, y in zip(chip.prefilter_stats(), before)) == (1, 5, 5)


def test_all_rows_equal_never_certifies(monkeypatch):
    D, n = 1024, 3_000
    row = oracle_lib.synth_rows(SEED, [7], D)
    db = np.ascontiguousarray(np.repeat(np.asarray(row, dtype=np.float32), n, axis=0))
    p = every_tick_params()
    w = [2_000, 2_003, 2_900, 2_500, 2_001]
    alone = alone_records(monkeypatch, D, db, [k + 50 for k in w], p)
    with make_chip(monkeypatch, D, db) as chip:
        ls, got = run_window(chip, w, p)
        assert (ls["family"], ls["ticks"]) == ("halfq", 5)
        assert got == [alone[k + 50] for k in w]
        assert chip.prefilter_stats() == (1, 5, 5)
        assert list(rec(got[0]).argmax) == [w[0] - 1] * 3       # every row ties: the highest index of the prefix


def test_coalesce_4_never_launches_the_five_tick_pass(monkeypatch):
    D = 1024
    db = build_db(D)[0]
    p = every_tick_params()
    w = [L0, L0 + 3, L0 + 6, L0 + 9, L0 + 12, L0 + 15, L0 + 18, L0 + 21, L0 + 24]
    alone = alone_records(monkeypatch, D, db, [k + 50 for k in w], p)
    with make_chip(monkeypatch, D, db, 4) as chip:
        families = []
        for s, k in enumerate(w):                                # the fourth parked tick releases a pass of four; last_scan releases what is parked
            chip.loop_tick_enqueue(k + 50, s, p)
            if s % 4 == 3 or s == len(w) - 1:
                ls = chip.last_scan()
                families.append((ls["family"], ls["ticks"]))
        got = [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]
        assert families[:2] == [("prefilter", 4), ("prefilter", 4)] and families[2][0] not in ("halfq", "prefilter", "multi"), families
        assert got == [alone[k + 50] for k in w]
        # (the rows behind L0 are copies of one row: the longer prefixes hold more than eight rows that tie at the top, and such a tick
        # runs again alone -- how many do is the data's business, not this test's)
        assert chip.prefilter_stats()[:2] == (2, 8)
