"""CPU tests of what the prefilter pass rests on (cerebro_amd/csrc/kernels.hip db_scan_prefilter / tick_rescore):
  * a numpy mirror of tick_rescore's decision -- per-owner lists of 8 by fp32 score, G, M, the candidate set R, the certificate
    M < G - 2 E -- against exact selection by the oracle's scores: whenever the mirror certifies, its top-8 IS the exact one, bit for
    bit, whatever order the fp32 scores were summed in;
  * the bound itself: |fp32 score - exact score| <= E on every (row, query) pair;
  * scan_prefilter_plan, the function the launch sizes itself with, through chip_debug_prefilter_plan."""
import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi

D, N, K, OWNERS, CAP = 256, 20_000, 8, 16, 32
U32, U64 = 2.0 ** -24, 2.0 ** -53


def error_bound(D, norm_max):
    """E as prefilter_error_bound (kernels.hip) evaluates it"""
    g32 = 2 * D * U32 / (1 - 2 * D * U32)
    g64 = (D + 8) * U64 / (1 - (D + 8) * U64)
    return ((g32 + g64) * norm_max * norm_max + D * 2.0 ** -148) * (1 + 2.0 ** -40)


def fp32_scores(db, q, order):
    """fp32 dot products of every row with q, summed in one of three orders, multiply then add (two roundings per term)"""
    prod = db * q[None, :]                                           # float32 x float32 -> float32
    if order == 0:                                                   # ascending chain
        acc = np.zeros(len(db), np.float32)
        for j in range(db.shape[1]):
            acc = acc + prod[:, j]
        return acc
    if order == 1:                                                   # descending chain
        acc = np.zeros(len(db), np.float32)
        for j in range(db.shape[1] - 1, -1, -1):
            acc = acc + prod[:, j]
        return acc
    while prod.shape[1] > 1:                                         # pairwise tree, halves
        h = prod.shape[1] // 2
        prod = prod[:, :h] + prod[:, h:]
    return prod[:, 0]


def topk_by_key(scores, idx, k):
    """the k best of (score desc, index desc)"""
    order = np.lexsort((-idx, -scores))[:k]
    return scores[order], idx[order]


def mirror(approx, exact, k_rows, E):
    """tick_rescore over rows [0, k_rows) owned round robin: (certified, exact scores, indices of the list it would write)"""
    idx = np.arange(k_rows)
    cand, M = [], -np.inf
    for o in range(OWNERS):
        mine = idx[o::OWNERS]
        s, i = topk_by_key(approx[mine].astype(np.float64), mine, K)
        cand.append(i)
        if len(mine) > K:
            M = max(M, s[-1])                                        # an owner of more than K rows dropped some: none above its K-th score
    cand = np.concatenate(cand)
    s_all = approx[cand].astype(np.float64)
    G = np.sort(s_all)[-K] if len(cand) >= K else -np.inf
    thr = G - 2 * E
    thr -= abs(thr) * 2.0 ** -51
    R = cand[s_all >= thr]
    certified = (M == -np.inf or M < thr) and len(R) <= CAP
    es, ei = topk_by_key(exact[R], R, K)
    return certified, es, ei


def gaussian(rng):
    db = rng.standard_normal((N, D)).astype(np.float32)
    db /= np.linalg.norm(db.astype(np.float64), axis=1)[:, None].astype(np.float32)
    return db, [int(x) for x in rng.integers(0, N, 4)]


def near_duplicates(rng):
    db, qs = gaussian(rng)
    for qi in qs:                                                    # 40 rows within a few fp32 ulps of each query
        rows = rng.choice(np.setdiff1d(np.arange(N), qs), 40, replace=False)
        db[rows] = db[qi][None, :] * (1 + rng.integers(-4, 5, (40, D)) * np.float32(2.0 ** -23))
    return db, qs


def all_equal(rng):
    row = rng.standard_normal(D).astype(np.float32)
    return np.repeat((row / np.float32(np.linalg.norm(row)))[None, :], N, axis=0), [3, 11_111]


@pytest.mark.needs_hip_build          # (the oracle's exact scores come from its compiled library)
@pytest.mark.parametrize("family", ["gaussian", "near_duplicates", "all_equal"])
def test_certified_lists_are_the_exact_ones(family):
    rng = np.random.default_rng({"gaussian": 11, "near_duplicates": 12, "all_equal": 13}[family])
    db, qs = {"gaussian": gaussian, "near_duplicates": near_duplicates, "all_equal": all_equal}[family](rng)
    db = np.ascontiguousarray(db)
    norm_max = float(np.sqrt((db.astype(np.float64) ** 2).sum(axis=1)).max()) * (1 + 2.0 ** -30)
    E = error_bound(D, norm_max)
    n_cert = n_all = n_cert_long = 0
    for qi in qs:
        q = db[qi]
        exact = np.asarray(oracle_lib.scores(db, N, q), dtype=np.float64)
        assert float(exact[qi]).hex() == float(oracle_lib.dot_tree(q, db[qi])).hex()
        for order in range(3):
            approx = fp32_scores(db, q, order)
            assert np.abs(approx.astype(np.float64) - exact).max() <= E                  # the bound, on every pair
            for k_rows in (5, 100, 7_777, N):
                certified, es, ei = mirror(approx, exact, k_rows, E)
                n_all += 1
                if not certified:
                    continue
                n_cert += 1
                n_cert_long += k_rows > CAP
                ws, wi = topk_by_key(exact[:k_rows], np.arange(k_rows), K)
                assert [float(x).hex() for x in es] == [float(x).hex() for x in ws] and list(ei) == list(wi), (family, qi, order, k_rows)
    if family == "gaussian":
        assert n_cert == n_all                   # gap between the 8th score and the best dropped one: tenths of a sigma; 2 E: a thousandth
    if family == "all_equal":
        # no prefix of the DB certifies but the 5-row one, where no list is full (nothing was dropped) and all 5 rows are rescored
        assert n_cert_long == 0 and n_cert == 2 * 3
    if family == "near_duplicates":
        assert 0 < n_cert                        # (the short prefixes at least)


@pytest.mark.needs_hip_build
def test_prefilter_plan():
    p = capi.prefilter_plan(1024)
    assert (p["family"], p["ticks"], p["nq"], p["NG"], p["R"], p["block"], p["grid"]) == ("prefilter", 4, 12, 0, 4, 512, 256)
    assert p["lds_bytes"] == 12 * 1024 * 4 + 8 * 12 * 8 * 16
    p = capi.prefilter_plan(4096)
    assert (p["family"], p["ticks"], p["nq"], p["NG"]) == ("prefilter", 4, 12, 3)            # 9 staged + 3 read in place
    assert p["lds_bytes"] == 9 * 4096 * 4 + 8 * 12 * 8 * 16 <= 160 * 1024
    for d in (1024, 2048, 3072, 4096):
        assert capi.prefilter_plan(d)["lds_bytes"] <= 160 * 1024
    assert capi.prefilter_plan(8192, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED
    assert capi.prefilter_plan(5120, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED            # five in place: no such instantiation
    assert capi.prefilter_plan(4096, elem=8, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED    # double rows
    assert capi.prefilter_plan(1000, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED            # not whole 4 KiB batches
    # the fp64 pass is sized as before: no fourth tick there
    assert capi.multi_plan(4096, 4, 4, 8, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED
    assert capi.multi_plan(4096, 4, 3)["ticks"] == 3
