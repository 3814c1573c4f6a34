"""GPU tests of pipelined ticks that share a DB pass on a DOUBLE-row DB (cerebro_amd/csrc/kernels.hip db_scan_shared_f64, chip_api.hip
coalesce_*): the double-row counterparts of tests/test_tick_coalesce_gpu.py and of the pass-boundary test of the float kernel.  The bar is
the same: every 64-byte decision record of a pipelined run equals, byte for byte, the record of the same tick issued alone through
chip_loop_tick with coalescing off, and the CPU oracle's (orc_dot_tree_f64 order).  The rows are genuinely float64 (relja_like of
tests/test_f64_gpu.py: not float32-representable); at D = 4096 two of a pass's six queries are read in place from global memory, at
D = 1024 all six are staged.  CHIP_SCAN_OVERLAP_GIB=0 makes every scan take the long-scan path and parking is forced, as in the float
tests.  Double rows share a pass between TWO ticks, whatever CHIP_TICK_COALESCE >= 2 says.  One full-size case (1M rows, 32.8 GB) runs
unforced, as the benchmark does."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi
from test_f64_gpu import relja_like
from test_tick_coalesce_gpu import DUP_HI, DUP_LO, L0, N_ROWS, PLANTS, every_tick_params, pipelined, rec

pytestmark = pytest.mark.gpu
SEED = 424_242
NTH = min(16, os.cpu_count() or 1)
SMALL = dict(D=1024, rows=3_000, l0=2_000)        # all six queries staged; prefixes span several workgroups' first groups only


@functools.lru_cache(maxsize=2)
def database(D, rows):
    plants = PLANTS if rows == N_ROWS else [(SMALL["l0"] - 50 + 1, 1_234, 2)] + [(r, 1_234, 2) for r in range(SMALL["l0"] - 3, SMALL["l0"] + 60)]
    db = relja_like(SEED, rows, D, plants)
    assert not np.array_equal(db.astype(np.float32).astype(np.float64), db)      # genuinely float64
    db.setflags(write=False)
    return db


def make_chip(monkeypatch, coalesce, D=4096, rows=N_ROWS, force=True):
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    monkeypatch.setenv("CHIP_TICK_COALESCE", str(coalesce))
    chip = capi.Chip(D, capacity_hint=rows + 64, storage="f64")
    chip.append_f64(database(D, rows))
    if coalesce and force:
        chip.coalesce_force(True)
    return chip


def one_by_one(monkeypatch, ls, p, resets=(), **kw):
    with make_chip(monkeypatch, 0, **kw) as ref:
        out = []
        for i, l in enumerate(ls):
            if i in resets:
                ref.loop_reset()
            out.append(bytes(ref.loop_tick(l, p)))
        assert ref.coalesce_stats() == (0, 0)
        assert ref.last_scan()["family"] != "multi"
        return out, ref.last_l()


def oracle_params():
    op = oracle_lib.default_params()
    op.min_new = -(1 << 30)
    return op


def assert_record_is_the_oracles(r, o):
    assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
    assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()


@pytest.mark.parametrize("tmax", [2, 3])
def test_pipelined_windows_equal_ticks_issued_one_by_one(monkeypatch, tmax):
    p = every_tick_params()
    ls = [L0 + 3 * i for i in range(7)] + [40] + [L0 + 21 + 3 * i for i in range(5)] + [L0 + 7, L0 + 100, N_ROWS]   # 40: too short
    want, want_last = one_by_one(monkeypatch, ls, p)
    assert rec(want[7]).status == capi.CHIP_TICK_TOO_SHORT
    # the planted pair: the first tick's prefix ends before DUP_HI, every later one holds both copies -> the higher index wins the tie
    assert list(rec(want[0]).argmax) == [DUP_LO] * 3 and list(rec(want[1]).argmax) == [DUP_HI] * 3
    assert rec(want[0]).maxv[0] == rec(want[1]).maxv[0]
    assert_record_is_the_oracles(rec(want[1]), oracle_lib.LoopOracle64(database(4096, N_ROWS), oracle_params()).tick(ls[1]))
    with make_chip(monkeypatch, tmax) as chip:
        for window in (1, 2, 3, 4, 16):
            chip.loop_reset()
            before = chip.coalesce_stats()
            got = pipelined(chip, ls, p, window)
            assert got == want, (tmax, window, [i for i, (g, w) in enumerate(zip(got, want)) if g != w])
            assert chip.last_l() == want_last
            passes, ticks = (a - b for a, b in zip(chip.coalesce_stats(), before))
            if window == 1:
                assert (passes, ticks) == (0, 0)           # every collect releases its own tick: passes of one
            else:
                assert passes >= 1 and ticks > passes and ticks <= len(ls) - 1 and ticks <= 2 * passes   # double rows: two ticks per pass
        assert ticks >= 12          # window 16: the 7 + 5 scanned ticks around the too-short one leave two at a time


def test_narrow_double_rows_with_every_query_staged(monkeypatch):
    D, rows, l0 = SMALL["D"], SMALL["rows"], SMALL["l0"]
    p = every_tick_params()
    ls = [l0 + 3 * i for i in range(6)] + [40, l0 + 7, 600, rows]
    want, want_last = one_by_one(monkeypatch, ls, p, D=D, rows=rows)
    assert_record_is_the_oracles(rec(want[1]), oracle_lib.LoopOracle64(database(D, rows), oracle_params()).tick(ls[1]))
    with make_chip(monkeypatch, 2, D=D, rows=rows) as chip:
        for window in (1, 2, 3, 16):
            chip.loop_reset()
            before = chip.coalesce_stats()
            assert pipelined(chip, ls, p, window) == want and chip.last_l() == want_last
            passes, ticks = (a - b for a, b in zip(chip.coalesce_stats(), before))
            assert (passes, ticks) == (0, 0) if window == 1 else (passes >= 1 and passes < ticks <= 2 * passes)
        chip.loop_tick_enqueue(l0, 0, p)
        chip.loop_tick_enqueue(l0 + 9, 1, p)
        f = chip.last_scan()
        assert (f["family"], f["elem"], f["ticks"], f["nq"], f["R"], f["q64"], f["NG"], f["n_rows"]) == ("multi", 8, 2, 6, 4, 6, 0, l0 + 9 - 50), f
        assert [bytes(chip.loop_tick_collect(s)) for s in (0, 1)] == [want[0], want[3]]


def test_shared_pass_at_its_pass_boundary(monkeypatch):
    """The windows of the float kernel's pass-boundary test on the double DB: prefixes on both sides of P = 4 W and 2 P (W waves of the
    launch, four rows per wave and pass), ten rows / about W rows / the whole DB in one pass, the duplicate's upper copy as the last row
    of one tick and beyond the prefix of the other; last_scan() says which kernel served each window and where its queries were."""
    p = every_tick_params()
    with make_chip(monkeypatch, 2) as chip:          # the geometry, from a first forced window
        for s in range(2):
            chip.loop_tick_enqueue(L0 + 3 * s, s, p)
        ls = chip.last_scan()
        assert (ls["family"], ls["ticks"], ls["R"], ls["nq"], ls["elem"], ls["block"]) == ("multi", 2, 4, 6, 8, 512), ls
        assert ls["q64"] + ls["NG"] == ls["nq"] and ls["NG"] > 0 and ls["q64"] >= 1, ls
        assert ls == dict(capi.multi_plan(4096, 8, 2, ls["K"], chip.info()["n_cus"]), n_rows=ls["n_rows"], launches=ls["launches"])
        W, R = ls["grid"] * ls["block"] // 64, ls["R"]
        assert ls["n_rows"] == L0 + 3 - 50 and 2 * R * W + 100 < N_ROWS
        for s in range(2):
            chip.loop_tick_collect(s)
    P = R * W
    windows = [[P - 2, P + 1, P + 4], [2 * P + 4, 2 * P - 2, 2 * P + 1], [P, 2 * P, P - 1], [10, W + 3, N_ROWS - 50], [N_ROWS - 50, W - 1, 10],
               [DUP_HI + 1, DUP_HI - 1, DUP_HI + 4], [DUP_HI, DUP_HI + 1, N_ROWS - 50]]       # prefixes k; the tick is l = k + 50
    windows = [w[:2] for w in windows] + [[w[0], w[2]] for w in windows] + [[w[1], w[2]] for w in windows]
    all_l = sorted({k + 50 for w in windows for k in w})
    alone, _ = one_by_one(monkeypatch, all_l, p)
    alone = dict(zip(all_l, alone))
    db, op = database(4096, N_ROWS), oracle_params()
    with make_chip(monkeypatch, 2) as chip:
        launches = chip.last_scan()["launches"]
        for w in windows:
            before = chip.coalesce_stats()
            for s, k in enumerate(w):
                chip.loop_tick_enqueue(k + 50, s, p)
            ls = chip.last_scan()
            launches += 1
            assert (ls["family"], ls["elem"], ls["ticks"], ls["nq"], ls["n_rows"], ls["launches"]) == ("multi", 8, len(w), 3 * len(w), max(w), launches), (w, ls)
            assert tuple(a - b for a, b in zip(chip.coalesce_stats(), before)) == (1, len(w))
            got = [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]
            assert got == [alone[k + 50] for k in w], (w, [i for i, k in enumerate(w) if got[i] != alone[k + 50]])
            k = min(w)
            assert_record_is_the_oracles(rec(got[w.index(k)]), oracle_lib.LoopOracle64(db, op).tick(k + 50))
        # the planted pair: the tick whose LAST row is the upper copy reports it, the tick whose prefix ends just before it the lower copy
        assert list(rec(alone[DUP_HI + 1 + 50]).argmax) == [DUP_HI] * 3 and list(rec(alone[DUP_HI + 50]).argmax) == [DUP_LO] * 3


def test_skipped_tick_between_parked_ones_and_default_params(monkeypatch):
    p = capi.default_dot_params()        # min_new = 3: a tick closer than 3 to the last one is SKIPPED and leaves last_l alone
    ls = [L0, L0 + 3, L0 + 4, L0 + 7, L0 + 10, L0 + 11, L0 + 12, L0 + 13, L0 + 30]
    want, want_last = one_by_one(monkeypatch, ls, p)
    assert [rec(w).status for w in want].count(capi.CHIP_TICK_SKIPPED) == 3
    with make_chip(monkeypatch, 2) as chip:
        assert pipelined(chip, ls, p, 16) == want and chip.last_l() == want_last
        assert chip.coalesce_stats() == (3, 6)       # the six scanned ticks leave two at a time


def test_out_of_order_collects_busy_slots_and_reset_in_mid_stream(monkeypatch):
    p = capi.default_dot_params()
    ls = [L0, L0 + 3, L0 + 6, L0 + 9, L0 + 3, L0 + 6, L0 + 9, L0 + 12]      # positions wrap after four ticks: chip_loop_reset
    want, want_last = one_by_one(monkeypatch, ls, p, resets=(4,))
    assert all(rec(w).status == capi.CHIP_TICK_SCANNED for w in want)
    with make_chip(monkeypatch, 2) as chip:
        for i, l in enumerate(ls):
            if i == 4:
                chip.loop_reset()
            chip.loop_tick_enqueue(l, i, p)
            if i in (0, 6):     # slot i is parked now: enqueueing into it again is refused and disturbs nothing
                with pytest.raises(capi.ChipError) as e:
                    chip.loop_tick_enqueue(l + 3, i, p)
                assert e.value.status == capi.CHIP_ERR_BUSY
                assert chip.last_l() == l
        order = [7, 2, 0, 5, 6, 1, 4, 3]
        got = {s: bytes(chip.loop_tick_collect(s)) for s in order}
        assert [got[i] for i in range(len(ls))] == want and chip.last_l() == want_last
        with pytest.raises(capi.ChipError) as e:
            chip.loop_tick_collect(3)
        assert e.value.status == capi.CHIP_ERR_BUSY
        assert chip.coalesce_stats() == (4, 8)       # every second tick sends its pair off


def test_append_synchronize_query_and_destroy_with_a_tick_parked(monkeypatch):
    p = capi.default_dot_params()
    ls = [L0, L0 + 3, L0 + 6, L0 + 9, L0 + 12, L0 + 15]
    want, _ = one_by_one(monkeypatch, ls, p)
    with make_chip(monkeypatch, 2) as chip:
        extra = relja_like(99, 40, 4096)
        chip.loop_tick_enqueue(ls[0], 0, p)
        chip.append_f64(extra)                      # rows beyond every prefix in flight: the parked tick does not see them
        assert chip.size() == N_ROWS + 40
        chip.loop_tick_enqueue(ls[1], 1, p)         # the second parked tick sends both off
        assert chip.coalesce_stats() == (1, 2)
        chip.loop_tick_enqueue(ls[2], 2, p)
        assert chip.coalesce_stats() == (1, 2)      # parked
        chip.synchronize()                          # releases and waits: a pass of one tick is the one-tick kernel's
        assert chip.coalesce_stats() == (1, 2) and chip.last_scan()["family"] != "multi"
        assert [bytes(chip.loop_tick_collect(s)) for s in (0, 1, 2)] == want[:3]
        chip.loop_tick_enqueue(ls[3], 0, p)
        sc, ix = chip.query_rows(ls[3] - 50, [ls[3] - 1], 1)      # any other scan of the ctx releases the parked tick first
        assert int(ix[0][0]) == DUP_HI
        assert bytes(chip.loop_tick_collect(0)) == want[3]
        assert bytes(chip.loop_tick(ls[4], p)) == want[4]         # the synchronous tick is a pass of its own
        chip.loop_tick_enqueue(ls[5], 5, p)
        # leaving the block destroys the ctx with a tick parked: it is submitted and drained like any enqueued tick
    with make_chip(monkeypatch, 2) as chip:           # ... and the device is fine afterwards
        assert bytes(chip.loop_tick(ls[0], p)) == want[0]


def test_shared_pass_and_one_tick_kernels_agree_with_one_oracle_on_whole_lists(monkeypatch):
    """Not only the winner: the top-8 lists of the same prefixes through chip_query_rows (the one-tick kernel) equal the oracle's bit for
    bit, and the records of a forced window equal their first column."""
    p = every_tick_params()
    db = database(4096, N_ROWS)
    with make_chip(monkeypatch, 2) as chip:
        for w in ([L0, L0 + 3], [N_ROWS, 8192 + 50 + 5]):
            for s, l in enumerate(w):
                chip.loop_tick_enqueue(l, s, p)
            assert chip.last_scan()["family"] == "multi"
            recs = [rec(bytes(chip.loop_tick_collect(s))) for s in range(2)]
            for l, r in zip(w, recs):
                k = l - 50
                sc, ix = chip.query_rows(k, [l - 1, l - 2, l - 3], 8)
                assert chip.last_scan()["family"] != "multi"
                wsc, wix = oracle_lib.scan_topk_f64(db, k, db[[l - 1, l - 2, l - 3]], 8, nthreads=NTH)
                assert np.array_equal(ix, wix) and sc.tobytes() == wsc.tobytes(), (l, ix, wix)
                assert list(r.argmax) == list(wix[:, 0]) and [float(x).hex() for x in r.maxv] == [float(x).hex() for x in wsc[:, 0]], (l, r.argmax, wix[:, 0])


def test_full_size_pipelined_ticks_equal_synchronous_ticks(monkeypatch):
    """1M double rows (32.8 GB: long scans by the default bound), 16 ticks in flight, nothing forced, default environment: ticks park
    behind running scans as they do in bench.py --storage f64.  Every record equals the synchronous tick's."""
    monkeypatch.delenv("CHIP_SCAN_OVERLAP_GIB", raising=False)
    monkeypatch.delenv("CHIP_TICK_COALESCE", raising=False)
    rows, p = 1_000_000, capi.default_dot_params()
    src = 123_456
    plants = [(rows - 40 - j, src - j, 1) for j in range(3)]
    ls = [rows - 90 + 3 * i for i in range(16)] + [rows - 39]     # the last tick's queries are the planted revisit
    with capi.Chip(4096, capacity_hint=rows, storage="f64") as chip:
        chip.append_synthetic(rows, 771177, plants)
        want = [bytes(chip.loop_tick(l, p)) for l in ls]
        assert chip.coalesce_stats() == (0, 0)
        assert rec(want[-1]).found == 1 and rec(want[-1]).idx_prev == src and rec(want[0]).found == 0
        chip.loop_reset()
        assert pipelined(chip, ls, p, 16) == want
        passes, ticks = chip.coalesce_stats()
        assert passes >= 4 and ticks > passes          # a 4.8 ms scan outlasts the enqueues behind it
