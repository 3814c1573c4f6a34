"""CPU tests of what the five-tick pass rests on (cerebro_amd/csrc/kernels.hip db_scan_halfq / tick_rescore):
  * a numpy mirror of the pass's scores -- queries staged as fl16(2^e q), round to nearest even, fp32 sums in three orders, scaled back by
    2^-e -- and of tick_rescore's decision with E_h, against exact selection by the oracle's scores: |score - exact score| <= E_h on every
    pair, and whenever the mirror certifies, its top-8 IS the exact one, bit for bit;
  * the exponent e and the bound E_h as the library evaluates them (chip_debug_halfq_bound) against the formula of DESIGN.md 3;
  * the candidate count on Gaussian scores at the benchmark's sigma stays within kRescoreCap;
  * scan_halfq_plan, the function the launch sizes itself with, through chip_debug_halfq_plan."""
import math

import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi
from test_prefilter_bound import CAP, K, U32, U64, fp32_scores, mirror, topk_by_key

D, N = 256, 20_000


def exponent(norm_max):
    """the largest e with 2^e N <= 2^15, inside [-100, 100] (halfq_exponent, kernels.hip)"""
    if norm_max <= 0:
        return 15
    m, x = math.frexp(norm_max)
    if m == 0.5:
        x -= 1
    return max(-100, min(100, 15 - x))


def error_bound(D, n, e):
    """E_h as the issue states it and halfq_error_bound (kernels.hip) evaluates it"""
    g32 = 2 * D * U32 / (1 - 2 * D * U32)
    g64 = (D + 8) * U64 / (1 - (D + 8) * U64)
    h = 2.0 ** -11
    E = g64 * n * n + (g32 * (1 + h) + h) * n * n + (1 + g32) * n * math.sqrt(D) * 2.0 ** (-25 - e) + D * 2.0 ** (-149 - e)
    return E * (1 + 2.0 ** -40)


def stage(q, e):
    """fl16(2^e q), round to nearest even, fp16 subnormals kept: what the workgroups store in LDS"""
    with np.errstate(over="raise"):
        scaled = q.astype(np.float32) * np.float32(2.0 ** e)        # exact: a power of two
        h = scaled.astype(np.float16)
    assert np.isfinite(h).all()
    return h


def halfq_scores(db, q, e, order):
    """the pass's score of every row: fp32 sum of row x staged query in one of three orders, then 2^-e in fp64 (exact)"""
    s = fp32_scores(db, stage(q, e).astype(np.float32), order)      # fp16 -> fp32 is exact
    assert np.isfinite(s).all()
    return s.astype(np.float64) * 2.0 ** -e


def unit_rows(rng, n=N):
    db = rng.standard_normal((n, D)).astype(np.float32)
    db /= np.linalg.norm(db.astype(np.float64), axis=1)[:, None].astype(np.float32)
    return db


def case_unit(rng):
    return unit_rows(rng), [int(x) for x in rng.integers(0, N, 3)]


def case_subnormal(rng):
    """query rows whose small elements become fp16 subnormals (below 2^-14 after scaling) or zero (below 2^-25)"""
    db = unit_rows(rng)
    qs = [17, 4_242]
    for qi, lo in zip(qs, (-36.0, -45.0)):
        small = (2.0 ** rng.uniform(lo, -28.0, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
        small[:8] = (rng.standard_normal(8) / 4).astype(np.float32)   # a few elements of ordinary size carry the score
        db[qi] = small
    e = exponent(1.0)
    h = np.abs(stage(db[qs[0]], e).astype(np.float64))
    assert ((h > 0) & (h < 2.0 ** -14)).any() and (stage(db[qs[1]], e)[8:] == 0).any()
    return db, qs


def case_one_hot(rng):
    """a one-hot query whose single element IS the norm bound: the largest staged half there can be, at both ends of a binade"""
    db = unit_rows(rng) * np.float32(0.5)
    db[5] = 0
    db[5, 3] = np.float32(2.0) - np.float32(2.0 ** -22)              # N just below a power of two: 2^e N just below 2^15
    return db, [5, 77]


def case_one_hot_pow2(rng):
    db = unit_rows(rng) * np.float32(0.5)
    db[5] = 0
    db[5, 3] = np.float32(1.0)                                        # N = 1 exactly: e = 15 and the staged half is 2^15
    return db, [5, 77]


def case_large(rng):
    return unit_rows(rng) * np.float32(1e3), [1, 9_000]


def case_small(rng):
    return unit_rows(rng) * np.float32(1e-3), [1, 9_000]


def case_midpoints(rng):
    """every element of the query halfway between two neighbouring halves after scaling (ties to even, both directions)"""
    db = unit_rows(rng)
    j = rng.integers(0, 512, D)
    q = (1 + (2 * j + 1) * 2.0 ** -11) * 2.0 ** -5 * rng.choice([-1.0, 1.0], D)
    db[31] = q.astype(np.float32)
    assert (db[31].astype(np.float64) == q).all() and np.linalg.norm(q) <= 1.0
    h = stage(db[31], exponent(1.0)).astype(np.float64) * 2.0 ** -exponent(1.0)
    assert (np.abs(h - q) == 2.0 ** -16).all()                      # half an fp16 ulp of [2^10, 2^11) scaled back, every element
    return db, [31, 500]


CASES = {"unit": case_unit, "subnormal": case_subnormal, "one_hot": case_one_hot, "one_hot_pow2": case_one_hot_pow2,
         "large": case_large, "small": case_small, "midpoints": case_midpoints}


@pytest.mark.needs_hip_build          # (the oracle's exact scores and the library's bound come from compiled code)
@pytest.mark.parametrize("case", sorted(CASES))
def test_bound_and_certified_lists(case):
    rng = np.random.default_rng(100 + sorted(CASES).index(case))
    db, qs = CASES[case](rng)
    db = np.ascontiguousarray(db, dtype=np.float32)
    true_max = float(np.sqrt((db.astype(np.float64) ** 2).sum(axis=1)).max())
    n_cert = n_all = 0
    for norm_max in (true_max, true_max * (1 + 2.0 ** -30)):        # the bound the library keeps may sit a little above the largest norm
        e = exponent(norm_max)
        E = error_bound(D, norm_max, e)
        got_e, got_E = capi.halfq_bound(D, norm_max)
        assert got_e == e and abs(got_E - E) <= E * 1e-14, (norm_max, e, got_e, E, got_E)   # (one formula, two evaluation orders)
        assert 2.0 ** e * norm_max <= 2.0 ** 15
        for qi in qs:
            q = db[qi]
            exact = np.asarray(oracle_lib.scores(db, N, q), dtype=np.float64)
            for order in range(3):
                approx = halfq_scores(db, q, e, order)
                err = np.abs(approx - exact).max()
                assert err <= E, (case, qi, order, err, E)             # the bound, on every pair
                for k_rows in (5, 100, 7_777, N):
                    certified, es, ei = mirror(approx, exact, k_rows, E)
                    n_all += 1
                    if not certified:
                        continue
                    n_cert += 1
                    ws, wi = topk_by_key(exact[:k_rows], np.arange(k_rows), K)
                    assert [float(x).hex() for x in es] == [float(x).hex() for x in ws] and list(ei) == list(wi), (case, qi, order, k_rows)
    if case == "unit":
        assert n_cert == n_all           # sigma = 1/16 at D = 256: 2 E_h is a few hundredths of it, the gaps are tenths


@pytest.mark.needs_hip_build
def test_exponent_and_usable_range():
    for n, e in ((1.0, 15), (0.75, 15), (1.0 + 2.0 ** -30, 14), (2.0, 14), (1e3, 5), (1e-3, 24), (0.0, 15), (2.0 ** 104, -89), (1e-40, 100), (1e300, -100)):
        assert capi.halfq_bound(4096, n)[0] == exponent(n) == e, n
    # the benchmark's data: unit rows of 4096 elements
    e, E = capi.halfq_bound(4096, 1.0 + 2.0 ** -30)
    assert 9.7e-4 < E < 9.9e-4


def test_candidates_on_gaussian_scores_stay_within_the_cap():
    """1M scores of sigma = 1/64 (unit rows of 4096 elements), 150 draws: the rows within 2 E_h of the 8th best are the most R can hold"""
    E = error_bound(4096, 1.0 + 2.0 ** -30, 14)
    rng = np.random.default_rng(2024)
    counts = []
    for _ in range(150):
        s = rng.standard_normal(1_000_000, dtype=np.float32).astype(np.float64) / 64
        top = -np.partition(-s, 64)[:65]
        G = np.sort(top)[-K]
        counts.append(int((top >= G - 2 * E).sum()))
        assert counts[-1] < 65
    assert max(counts) <= CAP, max(counts)
    assert np.mean(counts) < CAP / 2


@pytest.mark.needs_hip_build
def test_halfq_plan():
    p = capi.halfq_plan(4096)
    assert (p["family"], p["ticks"], p["nq"], p["NG"], p["R"], p["block"], p["grid"], p["elem"]) == ("halfq", 5, 15, 0, 4, 512, 256, 4)
    assert p["lds_bytes"] == 15 * 4096 * 2 + 8 * 15 * 8 * 16 <= 163_840
    for d in (1024, 2048, 3072):
        p = capi.halfq_plan(d)
        assert (p["nq"], p["NG"], p["lds_bytes"]) == (15, 0, 15 * d * 2 + 8 * 15 * 8 * 16)
    assert capi.halfq_plan(5120, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED                # 150 KiB of halves + 15 KiB of lists
    assert capi.halfq_plan(8192, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED
    assert capi.halfq_plan(4096, elem=8, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED        # double rows
    assert capi.halfq_plan(1000, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED                # not whole 4 KiB batches
    # the four-tick pass is sized as before
    assert (capi.prefilter_plan(4096)["ticks"], capi.prefilter_plan(4096)["NG"]) == (4, 3)
