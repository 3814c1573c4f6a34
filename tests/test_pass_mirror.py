"""CPU tests of the oracle's mirrors of the prefilter passes' own arithmetic (oracle/dot_scan.c orc_pass_score_f32 / orc_pass_score_halfq /
orc_pass_scores) and of the list-driven numpy model of tick_rescore (tests/np_mirror_rescore.py).  The GPU tests hold the device to these bit
for bit (tests/test_pass_lists_gpu.py, tests/test_rescore_gpu.py); here, without a GPU:
  * the fp16 rounding the mirror writes out on the bits equals numpy's conversion on every pattern of a sweep with all half-way cases, the
    subnormal range and the overflow edge;
  * both mirrors stay within E / E_h of the oracle's exact scores on every case of test_halfq_bound.CASES and on test_prefilter_bound's
    three families (the premise of the certificate, DESIGN.md 3, for the kernel's own summation order);
  * both mirrors reproduce f32_two_terms / halfq_two_terms on the near-tie rows of the GPU tests, bit for bit;
  * the model of tick_rescore agrees with its ancestor test_prefilter_bound.mirror where that one's geometry applies (workgroups of one wave)."""
import numpy as np
import pytest

import np_mirror_rescore as model
import oracle_lib
import test_halfq_bound as hb
import test_halfq_gpu as hg
import test_prefilter_bound as pb
import test_prefilter_gpu as pg
from cerebro_amd import capi


def sweep():
    """fp32 bit patterns: around every half and every midpoint of two neighbouring halves (exact, one fp32 ulp either side), a dense walk
    through the fp16 subnormal range and below it, every pattern around the overflow edge, and random patterns of the whole range"""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)          # every finite non-negative half, exactly
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)   # exact: one more bit than a half
    assert (mid.astype(np.float64) * 2 == h[:-1].astype(np.float64) + h[1:].astype(np.float64)).all()
    base = np.concatenate([h, mid]).view(np.uint32)
    around = np.concatenate([base + d for d in (0, 1, 2)] + [np.maximum(base, d) - d for d in (1, 2)]).astype(np.uint32)
    lo, hi = np.float32(2.0 ** -27).view(np.uint32), np.float32(2.0 ** -13).view(np.uint32)
    dense = np.arange(int(lo), int(hi), 61, dtype=np.uint32)                                # 14 binades, about 1.9M patterns
    edge = np.arange(int(np.float32(65504.0).view(np.uint32)) - 5000, int(np.float32(65536.0).view(np.uint32)) + 5000, dtype=np.uint32)
    rnd = np.random.default_rng(7).integers(0, 0x7F800000, 2_000_000, dtype=np.uint32)      # finite
    pos = np.concatenate([around, dense, edge, rnd, np.array([0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000], np.uint32)])
    return np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)


def test_fp16_rounding_on_the_bits_equals_numpy():
    x = sweep()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = oracle_lib.f16_round_bits(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(x[i].view(np.uint32), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    # the sweep holds what it says: ties in both directions, subnormal and vanishing halves, values that overflow
    a = np.abs(x.astype(np.float64))
    assert ((a > 0) & (a < 2.0 ** -14)).sum() > 1_000_000 and (a == 2.0 ** -25).any() and (a >= 65520).any() and (a == 65519.99609375).any()
    # widening is exact and staging is conversion + widening of 2^e q
    q = x[np.isfinite(x)][:100_000]
    for e in (0, 14, -3):
        with np.errstate(over="ignore", under="ignore"):
            want = (q * np.float32(2.0 ** e)).astype(np.float16).astype(np.float32)
        got = oracle_lib.halfq_stage(q, e)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), e


def prefilter_families():
    for name, seed in (("gaussian", 11), ("near_duplicates", 12), ("all_equal", 13)):
        rng = np.random.default_rng(seed)
        yield name, {"gaussian": pb.gaussian, "near_duplicates": pb.near_duplicates, "all_equal": pb.all_equal}[name](rng)


CASES = sorted(hb.CASES) + ["gaussian", "near_duplicates", "all_equal"]


@pytest.mark.needs_hip_build          # (the library's bound)
@pytest.mark.parametrize("case", CASES)
def test_mirrors_stay_within_the_bounds(case):
    if case in hb.CASES:
        db, qs = hb.CASES[case](np.random.default_rng(100 + sorted(hb.CASES).index(case)))
    else:
        db, qs = dict(prefilter_families())[case]
    db = np.ascontiguousarray(db, dtype=np.float32)
    D, n = db.shape[1], len(db)
    norm_max = float(np.sqrt((db.astype(np.float64) ** 2).sum(axis=1)).max()) * (1 + 2.0 ** -30)
    E = pb.error_bound(D, norm_max)
    e = hb.exponent(norm_max)
    Eh = hb.error_bound(D, norm_max, e)
    got_e, got_Eh = capi.halfq_bound(D, norm_max)
    assert got_e == e and abs(got_Eh - Eh) <= Eh * 1e-14
    q = db[qs]
    exact = np.stack([oracle_lib.scores(db, n, x, nthreads=8) for x in q])
    f32 = oracle_lib.pass_scores(db, n, q)
    hq = oracle_lib.pass_scores(db, n, q, halfq=True, e=e)
    assert np.isfinite(f32).all() and np.isfinite(hq).all()
    err, err_h = np.abs(f32 - exact).max(), np.abs(hq - exact).max()
    assert err <= E, (case, err, E)
    assert err_h <= Eh, (case, err_h, Eh)
    assert (f32 == f32.astype(np.float32)).all()                  # a list score of the four-tick pass is an fp32 value
    # the single-pair entries are the batched ones
    for j, r in ((0, 0), (len(qs) - 1, n - 1), (0, int(qs[0]))):
        assert float(oracle_lib.pass_score_f32(db[r], q[j])).hex() == float(f32[j, r]).hex()
        assert oracle_lib.pass_score_halfq(db[r], q[j], e).hex() == float(hq[j, r]).hex()
    # the staged query is numpy's (test_halfq_bound.stage), element for element
    for x in q:
        assert (oracle_lib.halfq_stage(x, e).view(np.uint32) == hb.stage(x, e).astype(np.float32).view(np.uint32)).all()


def test_mirrors_reproduce_the_two_term_rows():
    D = 1024
    for near, two_terms, halfq in ((pg.near_tie_rows, pg.f32_two_terms, False), (hg.near_tie_rows, hg.halfq_two_terms, True)):
        a, b, q, ea, eb = near()
        qrow = np.zeros(D, np.float32)
        qrow[0], qrow[2] = q
        for x in (a, b):
            row = np.zeros(D, np.float32)
            row[0], row[2] = x
            want = float(two_terms(x[0], q[0], x[1], q[1]))
            got = oracle_lib.pass_score_halfq(row, qrow, hg.E_SCALE) if halfq else float(oracle_lib.pass_score_f32(row, qrow))
            assert got.hex() == want.hex(), (halfq, x)
            db = np.ascontiguousarray(row[None, :])
            assert float(oracle_lib.pass_scores(db, 1, qrow, halfq=halfq, e=hg.E_SCALE)[0, 0]).hex() == want.hex()


def test_lane_order_and_tree():
    """the order itself, on values where it shows: 2^24 and ones.  A lane's low half takes elements 4L and 4L + 2 of every 256, its high half
    4L + 1 and 4L + 3; the halves are added, then lanes l and l ^ 32, ^ 16, ..."""
    D = 512
    q = np.ones(D, np.float32)
    row = np.zeros(D, np.float32)
    row[0], row[2], row[256] = 2.0 ** 24, 1.0, 1.0                 # low half of lane 0: (2^24 + 1) + 1 in fp32 = 2^24; as one sum it would be 2^24 + 2
    assert float(oracle_lib.pass_score_f32(row, q)) == 2.0 ** 24
    row[:] = 0
    row[0], row[1], row[3] = 2.0 ** 24, 1.0, 1.0                   # high half of lane 0 holds 1 + 1 first: 2^24 + 2
    assert float(oracle_lib.pass_score_f32(row, q)) == 2.0 ** 24 + 2
    row[:] = 0
    row[0], row[4 * 32], row[4 * 16] = 2.0 ** 24, 1.0, 1.0         # lanes 0, 32, 16: (2^24 + 1) + 1 = 2^24 -- lane 32 meets lane 0 before lane 16 does
    assert float(oracle_lib.pass_score_f32(row, q)) == 2.0 ** 24
    row[:] = 0
    row[0], row[4 * 16], row[4 * 48] = 2.0 ** 24, 1.0, 1.0         # lanes 16 and 48 meet each other first: 2^24 + 2
    assert float(oracle_lib.pass_score_f32(row, q)) == 2.0 ** 24 + 2


def test_rescore_model_agrees_with_its_ancestor():
    """workgroups of one wave (wpb = 1) are test_prefilter_bound.mirror's round-robin owners of single rows: same certificate, same list"""
    rng = np.random.default_rng(21)
    n, K, grid = 3_000, pb.K, pb.OWNERS
    n_cert = 0
    for trial in range(40):
        approx = rng.standard_normal(n).astype(np.float32)
        if trial % 2:
            approx[rng.integers(0, n, 60)] = approx.max()          # ties at the top
        exact = approx.astype(np.float64) + rng.uniform(-1e-3, 1e-3, n)
        E = [1e-3, 0.05, 0.2][trial % 3]
        for k in (5, 100, 129, 1_777, n):
            want_cert, want_s, want_i = pb.mirror(approx, exact, k, E)
            cs, ci = model.pass_lists(approx, k, grid, 1, K)
            got = model.rescore(cs, ci, k, 1, K, E, exact, cap=pb.CAP)
            assert (got["cert"] == 1) == bool(want_cert), (trial, k)
            if want_cert:
                n_cert += 1
                assert list(got["exact_i"][:len(want_i)]) == list(want_i) and (model.bits(got["exact_s"][:len(want_s)]) == model.bits(want_s)).all()
    assert n_cert > 20


@pytest.mark.needs_hip_build
def test_last_pass_entry_at_the_boundary(chip_lib):
    """chip_debug_last_pass without a GPU: declared, exported, bound; the record's layout; a NULL ctx is a status code and nothing is written"""
    import ctypes as C
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "cerebro_hip.h").read_text()
    assert "int chip_debug_last_pass(chip_ctx *ctx, chip_debug_pass_info *info, chip_topk_entry *cand, chip_topk_entry *exact, uint32_t *cert);" in header
    assert hasattr(chip_lib, "chip_debug_last_pass") and "chip_debug_last_pass" in capi.declared_symbols()
    assert C.sizeof(capi.PassInfo) == 6 * 4 + 5 * 8 + 8 and capi.PassInfo.k.offset == 24 and capi.PassInfo.E.offset == 64
    info = capi.PassInfo()
    info.family, info.E = -3, 9.0
    cert = np.full(15, 7, np.uint32)
    assert chip_lib.chip_debug_last_pass(None, C.byref(info), None, None, cert.ctypes.data_as(C.c_void_p)) == capi.CHIP_ERR_INVALID_ARG
    assert chip_lib.chip_debug_last_pass(None, None, None, None, None) == capi.CHIP_ERR_INVALID_ARG
    assert (info.family, info.E) == (-3, 9.0) and (cert == 7).all()


def test_owned_count_is_the_row_map():
    for grid, wpb in ((3, 2), (256, 8), (5, 8)):
        tw = grid * wpb
        for k in list(range(0, 3 * tw + 2)) if tw < 100 else [0, 1, 7, 8, 9, tw - 1, tw, tw + 1, tw + 8 * 7 - 1, tw + 8 * 7, tw + 8 * 7 + 1, 2 * tw + 50, 3 * tw]:
            own = model.owner(np.arange(k), grid, wpb)
            counts = np.bincount(own, minlength=grid)
            assert [model.owned_count(b, k, grid, wpb) for b in range(grid)] == list(counts), (grid, wpb, k)
