"""GPU tests of the prefilter pass: four pipelined ticks share one fp32 pass over the DB (cerebro_amd/csrc/kernels.hip db_scan_prefilter),
tick_rescore proves per query which rows can be in the exact top-8 and scores those in fp64.  The bar is the one of
test_tick_coalesce_gpu.py: every 64-byte decision record of a window of four forced-parked ticks equals, byte for byte, the record of the
same tick issued alone with coalescing off, one per window the CPU oracle's -- where the certificate holds AND where it does not (such a
tick runs again alone).  CHIP_SCAN_OVERLAP_GIB=0 makes every scan a long one, parking is forced, coalescing is at its default."""
import math

import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
SEED = 424243
N_ROWS = 16_600                  # just above 2 R W + 100 on 256 CUs (W = 2048 waves, R = 4 rows per wave and pass)
L0 = 12_000
DUP_LO, DUP_HI = 5_000, L0 - 50 + 1
# as test_tick_coalesce_gpu.py: the query rows of the ticks around L0 and DUP_HI are copies of DUP_LO
PLANTS = [(DUP_HI, DUP_LO, 2)] + [(r, DUP_LO, 2) for r in range(L0 - 3, L0 + 60)]
A_IDX, B_IDX = 7_001, 3_003      # the two rows of near_tie_rows()
K_TIE = 9_000                    # prefix of the tick whose first query (row K_TIE + 49) meets them


def every_tick_params():
    p = capi.default_dot_params()
    p.min_new = -(1 << 30)
    return p


def rec(b):
    return capi.TickResult.from_buffer_copy(b)


def f32_two_terms(x1, q1, x2, q2):
    """what db_scan_prefilter computes for a row that is zero but for elements 0 and 2: both go through the low half of lane 0's accumulator,
    fl(x2 q2 + fl(x1 q1)); every other addition of the sum adds a zero.  (x2 q2 + acc is exact in fp64 for the magnitudes used here.)"""
    acc = np.float32(x1) * np.float32(q1)
    return np.float32(np.float64(x2) * np.float64(q2) + np.float64(acc))


def near_tie_rows():
    """(a, b, q, exact_a, exact_b): rows a = (a1, 0, a2, 0, ...), b likewise, and the query's elements 0 and 2, such that the exact scores
    differ by less than one fp32 ulp of the sum with a ahead, and the fp32 scores are in the opposite order."""
    q1, q2 = np.float32(0.5) * np.float32(1 + 2.0 ** -12 + 2.0 ** -21), np.float32(-0.5) * np.float32(1 + 2.0 ** -9)
    rng = np.random.default_rng(5)
    x1 = (1 + rng.integers(0, 1 << 12, 200_000) * 2.0 ** -23).astype(np.float32)
    x2 = (0.5 + rng.integers(0, 1 << 12, 200_000) * 2.0 ** -24).astype(np.float32)
    exact = x1.astype(np.float64) * np.float64(q1) + x2.astype(np.float64) * np.float64(q2)     # exact: both products and their sum fit 53 bits
    acc = x1 * q1
    approx = (x2.astype(np.float64) * np.float64(q2) + acc.astype(np.float64)).astype(np.float32)
    order = np.argsort(exact)
    lo, hi = order[:-1], order[1:]
    ulp = np.spacing(approx[hi])
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


def make_chip(monkeypatch, D, db, coalesce=None):
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    if coalesce is None:
        monkeypatch.delenv("CHIP_TICK_COALESCE", raising=False)
    else:
        monkeypatch.setenv("CHIP_TICK_COALESCE", str(coalesce))
    chip = capi.Chip(D, capacity_hint=len(db) + 64)
    chip.append_f32(db)
    if coalesce != 0:
        chip.coalesce_force(True)
    return chip


def alone_records(monkeypatch, D, db, ls, p):
    with make_chip(monkeypatch, D, db, 0) as ref:
        out = {l: bytes(ref.loop_tick(l, p)) for l in ls}
        assert ref.coalesce_stats() == (0, 0) and ref.prefilter_stats() == (0, 0, 0)
        return out


def run_window(chip, w, p):
    for s, k in enumerate(w):
        chip.loop_tick_enqueue(k + 50, s, p)
    ls = chip.last_scan()
    return ls, [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]


@pytest.mark.parametrize("D", [4096, 1024])
def test_windows_of_four_equal_ticks_issued_alone(monkeypatch, D):
    db, a, b, q, ea, eb = build_db(D)
    # the near-tie pair, on the CPU first: exact scores less than one fp32 ulp apart with row A ahead, fp32 scores the other way round
    sa, sb = f32_two_terms(a[0], q[0], a[1], q[1]), f32_two_terms(b[0], q[0], b[1], q[1])
    assert ea > eb and ea - eb < np.spacing(sa) and sa < sb
    qrow = db[K_TIE + 49].astype(np.float64)
    assert float(db[A_IDX].astype(np.float64) @ qrow) == ea and float(db[B_IDX].astype(np.float64) @ qrow) == eb
    others = np.delete(db[:K_TIE].astype(np.float64) @ qrow, [A_IDX, B_IDX])
    assert others.max() < eb - 0.01                  # the pair is the top two of that query: the exact order decides the record

    p = every_tick_params()
    plan = capi.prefilter_plan(D)
    with make_chip(monkeypatch, D, db) as chip:
        assert chip.info()["storage_bytes"] == 4
        ls, _ = run_window(chip, [L0, L0 + 3, L0 + 6, L0 + 9], p)         # the geometry, from a first window
        assert (ls["family"], ls["ticks"], ls["R"], ls["nq"], ls["elem"], ls["NG"], ls["lds_bytes"]) == \
            ("prefilter", 4, 4, 12, 4, plan["NG"], plan["lds_bytes"]), ls
        W, R = ls["grid"] * ls["block"] // 64, ls["R"]
        P = R * W
        assert 2 * P + 100 < N_ROWS
        windows = [[P - 2, P + 1, P + 4, 2 * P], [2 * P + 4, 2 * P - 2, P, 2 * P + 1],            # both sides of a pass boundary
                   [10, W + 3, N_ROWS - 50, P - 1], [N_ROWS - 50, 10, W - 1, 11],                 # lists not full; the whole DB
                   [DUP_HI + 1, DUP_HI - 1, DUP_HI + 4, DUP_HI], [DUP_HI, DUP_HI + 1, N_ROWS - 50, DUP_HI + 2],   # the duplicate pair
                   [K_TIE, K_TIE + 3, A_IDX, K_TIE - 3]]                                          # the near tie; a prefix that ends before row A
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
            assert (ls["family"], ls["ticks"], ls["n_rows"], ls["launches"]) == ("prefilter", 4, max(w), launches), (w, ls)
            assert got == [alone[k + 50] for k in w], (w, [i for i, k in enumerate(w) if got[i] != alone[k + 50]])
            k = min(w)
            o = oracle_lib.LoopOracle(db, op).tick(k + 50)
            r = rec(got[w.index(k)])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
        passes, ticks, unc = (x - y for x, y in zip(chip.prefilter_stats(), before))
        # Gaussian scores: the gap between the K-th score and the best dropped one (about 0.8 sigma at these sizes) is several times 2 E
        # (0.1 sigma at D = 4096, less at D = 1024: DESIGN.md 3), and a tie of two rows is two candidates: every tick certifies
        assert (passes, ticks, unc) == (len(windows), 4 * len(windows), 0), (passes, ticks, unc)
        assert chip.coalesce_stats()[0] >= len(windows)

        # windows of two and three are the fp64 pass, as before
        for w in ([P - 2, P + 1], [P - 2, P + 1, 2 * P]):
            ls, got = run_window(chip, w, p)
            assert (ls["family"], ls["ticks"]) == ("multi", len(w)), ls
            assert got == [alone[k + 50] for k in w]
        assert chip.prefilter_stats()[0] == before[0] + len(windows)

        # a row scaled by 1000, beyond every prefix: the norm bound grows, the error bound swamps every gap, no tick certifies
        big = (db[123].astype(np.float32) * np.float32(1000.0))[None, :]
        chip.append_f32(np.ascontiguousarray(big))
        want = float(np.sqrt((big.astype(np.float64) ** 2).sum()))
        assert want <= chip.info()["row_norm_max"] <= want * (1 + 1e-6)
        before = chip.prefilter_stats()
        ls, got = run_window(chip, windows[0], p)
        assert ls["family"] == "prefilter" and got == [alone[k + 50] for k in windows[0]]
        assert tuple(x - y for x, y in zip(chip.prefilter_stats(), before)) == (1, 4, 4)


def test_all_rows_equal_never_certifies(monkeypatch):
    D, n = 1024, 3_000
    row = oracle_lib.synth_rows(SEED, [7], D)
    db = np.ascontiguousarray(np.repeat(np.asarray(row, dtype=np.float32), n, axis=0))
    p = every_tick_params()
    w = [2_000, 2_003, 2_900, 2_500]
    alone = alone_records(monkeypatch, D, db, [k + 50 for k in w], p)
    with make_chip(monkeypatch, D, db) as chip:
        ls, got = run_window(chip, w, p)
        assert (ls["family"], ls["ticks"]) == ("prefilter", 4)
        assert got == [alone[k + 50] for k in w]
        assert chip.prefilter_stats() == (1, 4, 4)
        assert list(rec(got[0]).argmax) == [w[0] - 1] * 3       # every row ties: the highest index of the prefix


def test_row_norm_max_follows_every_append(monkeypatch):
    D = 1024
    # the correctly rounded norm of the heaviest row (exact squares, math.fsum); N is at most 1 + 2^-29 of it: tests/ingest_cases.py TIGHT
    norm = lambda x: max(math.sqrt(math.fsum((r * r).tolist())) for r in np.asarray(x, dtype=np.float64))
    monkeypatch.delenv("CHIP_TICK_COALESCE", raising=False)
    with capi.Chip(D, capacity_hint=4096) as chip:
        assert chip.info()["row_norm_max"] == 0.0
        a = np.ascontiguousarray(oracle_lib.synth_rows(SEED, range(300), D), dtype=np.float32) * np.float32(0.5)
        chip.append_f32(a)
        want = norm(a)
        assert want <= chip.info()["row_norm_max"] <= want * (1 + 2.0 ** -29)
        plants = [(310, 5, 1), (320, 6, 2)]
        chip.append_synthetic(200, SEED, plants)                 # rows 300 .. 499: generated rows and both kinds of plants
        want = max(want, norm(oracle_lib.synth_rows(SEED, range(300, 500), D, plants)))
        assert want <= chip.info()["row_norm_max"] <= want * (1 + 2.0 ** -29)
        c = np.ascontiguousarray(oracle_lib.synth_rows(SEED + 1, range(40), D), dtype=np.float32).astype(np.float64) * 2.0
        chip.append_f64(c)                                       # float64 on the wire, float rows in the DB
        assert chip.info()["storage_bytes"] == 4
        want = max(want, norm(c))
        assert want <= chip.info()["row_norm_max"] <= want * (1 + 2.0 ** -29)
