"""GPU tests of what the prefilter passes THEMSELVES compute (cerebro_amd/csrc/kernels.hip db_scan_prefilter, four ticks, and db_scan_halfq,
five): every score of every workgroup list, read back with chip_debug_last_pass, has the bits of the oracle's mirror of the kernel's
arithmetic (oracle/dot_scan.c orc_pass_scores) and is within E / E_h of the exact score; every list is the top K of the rows its workgroup
owns inside the tick's prefix; tick_rescore's certificate words and exact lists are the list-driven model's (tests/np_mirror_rescore.py).
The record-level tests (test_prefilter_gpu.py, test_halfq_gpu.py) see none of this where the certificate holds with room to spare.
  * test_scores_and_lists: Gaussian rows at D = 1024 (one batch per row), 2048 (a chain across a batch boundary), 4096 (the four-tick
    pass reads three queries in place: another fma path), prefixes on both sides of a wave's first pass and prefixes where lists stay short;
  * test_halfq_staging_edges: the five-tick pass's fp16 staging on the inputs of tests/test_halfq_bound.py -- subnormal and vanishing halves,
    midpoints, one-hot queries at the norm bound, norms of 1e3 and 1e-3 -- and on DBs scaled until the exponent clamps (e = 100) or is negative."""
import numpy as np
import pytest

import test_halfq_bound as hb
from cerebro_amd import capi
from pass_checks import TICKS, check_window
from test_prefilter_gpu import N_ROWS, build_db, every_tick_params, make_chip, run_window

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [1024, 2048, 4096])
@pytest.mark.parametrize("family", ["prefilter", "halfq"])
def test_scores_and_lists(monkeypatch, family, D):
    db = build_db(D)[0]
    T = TICKS[family]
    plan = (capi.prefilter_plan if family == "prefilter" else capi.halfq_plan)(D)
    with make_chip(monkeypatch, D, db) as chip:
        ls, _ = run_window(chip, [12_000 + 3 * t for t in range(T)], every_tick_params())       # the geometry, from a first window
        assert (ls["family"], ls["NG"]) == (family, plan["NG"])
        assert ls["NG"] == (3 if (family, D) == ("prefilter", 4096) else 0)
        W, R = ls["grid"] * ls["block"] // 64, ls["R"]
        P = R * W
        assert 2 * P + 100 < N_ROWS
        # (both windows at every D: a short prefix shows a query slot only the first row of a group, so every slot needs a long one as well)
        windows = [[P - 2, P + 1, P + 4, 2 * P, P - 1][:T],              # both sides of the row at which a wave starts its second group
                   [10, W + 3, N_ROWS - 50, W - 1, 9][:T]]               # k < W: most lists are not full, many are empty
        for w in windows:
            _, lp, res = check_window(chip, db, w, family, alone=False)
            for t in (t for t, k in enumerate(w) if k < W):      # what "not full" means, in the lists read back: a workgroup holds at most its eight rows of the first lap
                assert (lp["cand_i"][t, :, 0, 0] >= 0).sum() == -(-w[t] // (ls["block"] // 64))
                assert ((lp["cand_i"][t, :, 0, :] >= 0).sum(axis=1) < lp["K"]).any()


def test_last_pass_read_back(monkeypatch):
    """the entry itself: CHIP_ERR_BUSY until a prefilter pass was submitted (an fp64 pass of three ticks is none), any output pointer may be
    NULL, and the copy is the same after the window's ticks ran again alone and after a later pass of another kind"""
    import ctypes as C
    D = 1024
    db = build_db(D)[0]
    p = every_tick_params()
    with make_chip(monkeypatch, D, db) as chip:
        assert chip.lib.chip_debug_last_pass(chip.h, None, None, None, None) == capi.CHIP_ERR_BUSY
        ls, _ = run_window(chip, [9_000, 9_003, 9_006], p)
        assert ls["family"] == "multi" and chip.lib.chip_debug_last_pass(chip.h, None, None, None, None) == capi.CHIP_ERR_BUSY
        w = [9_000, 9_003, 9_006, 9_009, 9_012]
        ls, got = run_window(chip, w, p)
        assert ls["family"] == "halfq"
        assert chip.lib.chip_debug_last_pass(chip.h, None, None, None, None) == capi.CHIP_OK
        info = capi.PassInfo()
        assert chip.lib.chip_debug_last_pass(chip.h, C.byref(info), None, None, None) == capi.CHIP_OK
        assert (capi.SCAN_FAMILY_NAMES[info.family], info.ticks, info.grid, info.wpb, info.K, list(info.k)) == ("halfq", 5, ls["grid"], ls["block"] // 64, 8, w)
        cert = np.zeros((5, 3), np.uint32)
        assert chip.lib.chip_debug_last_pass(chip.h, None, None, None, cert.ctypes.data_as(C.c_void_p)) == capi.CHIP_OK and np.isin(cert, (1, 2)).all()
        a = chip.last_pass()
        assert (a["cert"] == cert).all()
        assert [bytes(chip.loop_tick(k + 50, p)) for k in w] == got
        ls, _ = run_window(chip, [9_100, 9_103], p)
        assert ls["family"] == "multi"
        b = chip.last_pass()
        assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a)
        # a four-tick pass replaces it
        run_window(chip, w[:4], p)
        c = chip.last_pass()
        assert (c["family"], c["ticks"], c["e"], c["k"]) == ("prefilter", 4, 0, w[:4]) and c["cand_s"].shape == (4, ls["grid"], 3, 8)
    with capi.Chip(D, devices=[0, 0]) as grp:                                   # a group ctx has no such pass
        assert grp.lib.chip_debug_last_pass(grp.h, None, None, None, None) == capi.CHIP_ERR_INVALID_ARG


# ---- the staging of the five-tick pass at its edges
N_EDGE, D_EDGE, L_EDGE = 3_000, 1024, 2_900


def spread(db256):
    """the 256 columns of a case of test_halfq_bound over rows of 1024: column c -> 256 (c // 64) + 4 (c % 64) + c // 64, so that every lane
    gets one element in each KiB of the batch and in each of its four accumulator slots; the other columns are zero.  Norms and dot
    products are the case's."""
    c = np.arange(256)
    out = np.zeros((len(db256), D_EDGE), np.float32)
    out[:, 256 * (c // 64) + 4 * (c % 64) + c // 64] = db256
    return out


def edge_db(case):
    """(db [N_EDGE, 1024], window): the first rows of the case's DB, and at the rows the window's ticks take their queries from -- rows
    l - 1, l - 2, l - 3 of l = L_EDGE + 3 t + 50 -- the case's query rows in turn"""
    scale = {"tiny": 2.0 ** -103, "huge": 2.0 ** 100}.get(case)
    name = "unit" if scale else case
    db256, qs = hb.CASES[name](np.random.default_rng(100 + sorted(hb.CASES).index(name)))
    db256 = np.asarray(db256, dtype=np.float32)
    if scale:
        db256 = db256 * np.float32(scale)                          # a power of two: exact
    small = db256[:N_EDGE].copy()
    w = [L_EDGE - 50 + 3 * t for t in range(5)]
    for j, r in enumerate(k + 50 - 1 - i for k in w for i in range(3)):
        small[r] = db256[qs[j % len(qs)]]
    db = spread(small)
    db.setflags(write=False)
    return db, w


@pytest.mark.parametrize("case", sorted(hb.CASES) + ["tiny", "huge"])
def test_halfq_staging_edges(monkeypatch, case):
    db, w = edge_db(case)
    with make_chip(monkeypatch, D_EDGE, db) as chip:
        e, E = capi.halfq_bound(D_EDGE, chip.info()["row_norm_max"])
        want_e = {"tiny": 100, "huge": -86, "large": 5, "small": 24, "one_hot": 14, "one_hot_pow2": 14}.get(case, 14)
        assert e == want_e, (case, e)
        _, lp, _ = check_window(chip, db, w, "halfq")              # (its own assertions: e and E read back are these, records equal the ticks issued alone)
        assert (lp["e"], lp["E"]) == (e, E)
        # the case is on the device what it is on the CPU: the staged queries hold the halves the case is about
        q = db[[k + 49 for k in w]].astype(np.float64) * 2.0 ** e
        h = np.abs(q.astype(np.float32).astype(np.float16).astype(np.float64))
        if case == "subnormal":
            assert ((h > 0) & (h < 2.0 ** -14)).any() and ((h == 0) & (q != 0)).any()
        if case == "midpoints":
            assert (np.abs(h[0] - np.abs(q[0]))[q[0] != 0] == 0.25).all()      # halves in [2^9, 2^10) are 1/2 apart: every element sits halfway
        if case.startswith("one_hot"):
            assert h.max() == 2.0 ** 15 or h.max() == 2.0 ** 14
