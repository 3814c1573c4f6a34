"""GPU tests of pipelined ticks that share a DB pass (CHIP_TICK_COALESCE: cerebro_amd/csrc/kernels.hip db_scan_topk_multi,
chip_api.hip coalesce_*).  The bar: every 64-byte decision record of a pipelined run equals, byte for byte, the record of the same
tick issued alone through chip_loop_tick with coalescing off (and, for one tick, the CPU oracle) -- whatever the window, whatever
lies between the parked ticks, whoever releases them.  The sizes are cheap (24k rows); CHIP_SCAN_OVERLAP_GIB=0 makes every scan
take the long-scan path, and parking is forced (chip_debug_coalesce_force) because whether a small scan is still running when the
next enqueue arrives is a race.  One full-size case (1M rows) runs unforced, as the benchmark does."""
import os

import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
D = 4096
SEED, N_ROWS = 771177, 24_000
L0 = 20_000                      # first tick of the runs below; prefix k = l - 50
DUP_LO, DUP_HI = 12_345, L0 - 50 + 1      # two identical rows; DUP_HI lies inside [k(L0), k(L0 + 3))
# every query row of the ticks L0, L0 + 3, ... is a copy of DUP_LO, and so is DUP_HI: a tick whose prefix holds both rows sees two
# equal best scores and must report the HIGHER index; a tick whose prefix ends before DUP_HI must report DUP_LO
PLANTS = [(DUP_HI, DUP_LO, 2)] + [(r, DUP_LO, 2) for r in range(L0 - 3, L0 + 60)]


def every_tick_params():
    p = capi.default_dot_params()
    p.min_new = -(1 << 30)          # every tick runs, whatever the previous l was
    return p


def make_chip(monkeypatch, coalesce, rows=N_ROWS, plants=PLANTS, force=True):
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    monkeypatch.setenv("CHIP_TICK_COALESCE", str(coalesce))
    chip = capi.Chip(D, capacity_hint=rows + 64)
    chip.append_synthetic(rows, SEED, plants)
    if coalesce and force:
        chip.coalesce_force(True)
    return chip


def one_by_one(monkeypatch, ls, p, resets=()):
    with make_chip(monkeypatch, 0) as ref:
        out = []
        for i, l in enumerate(ls):
            if i in resets:
                ref.loop_reset()
            out.append(bytes(ref.loop_tick(l, p)))
        assert ref.coalesce_stats() == (0, 0)
        return out, ref.last_l()


def pipelined(chip, ls, p, window, resets=()):
    out, pending = [], []
    for i, l in enumerate(ls):
        if len(pending) == window:
            out.append(bytes(chip.loop_tick_collect(pending.pop(0))))
        if i in resets:
            chip.loop_reset()
        chip.loop_tick_enqueue(l, i % window, p)
        pending.append(i % window)
    while pending:
        out.append(bytes(chip.loop_tick_collect(pending.pop(0))))
    return out


def rec(b):
    return capi.TickResult.from_buffer_copy(b)


@pytest.mark.parametrize("tmax", [2, 3])
def test_pipelined_windows_equal_ticks_issued_one_by_one(monkeypatch, tmax):
    assert capi.load_library().chip_build_has_tick_coalesce() == 1
    p = every_tick_params()
    ls = [L0 + 3 * i for i in range(7)] + [40] + [L0 + 21 + 3 * i for i in range(5)] + [L0 + 7, L0 + 100, N_ROWS]   # 40: too short
    want, want_last = one_by_one(monkeypatch, ls, p)
    assert rec(want[7]).status == capi.CHIP_TICK_TOO_SHORT
    # the planted pair: the first tick's prefix ends before DUP_HI, every later one holds both copies -> the higher index wins the tie
    assert list(rec(want[0]).argmax) == [DUP_LO] * 3 and list(rec(want[1]).argmax) == [DUP_HI] * 3
    assert rec(want[0]).maxv[0] == rec(want[1]).maxv[0]
    # one record against the CPU oracle
    l = ls[1]
    qrows = oracle_lib.synth_rows(SEED, [l - 1, l - 2, l - 3], D, PLANTS)
    wsc, wix = oracle_lib.scan_topk_synth(SEED, l - 50, D, qrows, 1, PLANTS, nthreads=os.cpu_count() or 1)
    r = rec(want[1])
    assert list(r.argmax) == list(wix[:, 0]) and [float(x).hex() for x in r.maxv] == [float(x).hex() for x in wsc[:, 0]]
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
                assert passes >= 1 and ticks > passes and ticks <= len(ls) - 1 and ticks <= tmax * passes
        if tmax == 3:   # window 16: the 7 + 5 scanned ticks around the too-short one leave three at a time
            assert ticks >= 12


def test_skipped_tick_between_parked_ones_and_default_params(monkeypatch):
    p = capi.default_dot_params()        # min_new = 3: a tick closer than 3 to the last one is SKIPPED and leaves last_l alone
    ls = [L0, L0 + 3, L0 + 4, L0 + 7, L0 + 10, L0 + 11, L0 + 12, L0 + 13, L0 + 30]
    want, want_last = one_by_one(monkeypatch, ls, p)
    assert [rec(w).status for w in want].count(capi.CHIP_TICK_SKIPPED) == 3
    with make_chip(monkeypatch, 3) as chip:
        assert pipelined(chip, ls, p, 16) == want and chip.last_l() == want_last
        passes, ticks = chip.coalesce_stats()
        assert (passes, ticks) == (2, 6)


def test_out_of_order_collects_busy_slots_and_reset_in_mid_stream(monkeypatch):
    p = capi.default_dot_params()
    ls = [L0, L0 + 3, L0 + 6, L0 + 9, L0 + 3, L0 + 6, L0 + 9, L0 + 12]      # positions wrap after four ticks: chip_loop_reset
    want, want_last = one_by_one(monkeypatch, ls, p, resets=(4,))
    assert all(rec(w).status == capi.CHIP_TICK_SCANNED for w in want)
    with make_chip(monkeypatch, 3) as chip:
        for i, l in enumerate(ls):
            if i == 4:
                chip.loop_reset()
            chip.loop_tick_enqueue(l, i, p)
            if i in (1, 7):     # slot i is parked now: enqueueing into it again is refused and disturbs nothing
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
        assert chip.coalesce_stats() == (3, 8)       # 3 + 3 at the third parked tick, 2 at the first collect


def test_append_synchronize_query_and_destroy_with_ticks_parked(monkeypatch):
    p = capi.default_dot_params()
    ls = [L0, L0 + 3, L0 + 6, L0 + 9, L0 + 12]
    want, _ = one_by_one(monkeypatch, ls, p)
    with make_chip(monkeypatch, 3) as chip:
        extra = oracle_lib.synth_rows(99, range(40), D)
        chip.loop_tick_enqueue(ls[0], 0, p)
        chip.loop_tick_enqueue(ls[1], 1, p)
        chip.append_f32(extra)                      # rows beyond every prefix in flight: the parked ticks do not see them
        assert chip.size() == N_ROWS + 40
        assert chip.coalesce_stats() == (0, 0)      # still parked
        chip.synchronize()                          # releases and waits
        assert chip.coalesce_stats() == (1, 2)
        assert [bytes(chip.loop_tick_collect(s)) for s in (0, 1)] == want[:2]
        chip.loop_tick_enqueue(ls[2], 0, p)
        sc, ix = chip.query_rows(ls[2] - 50, [ls[2] - 1], 1)      # any other scan of the ctx releases the parked tick first
        assert int(ix[0][0]) == DUP_HI
        assert bytes(chip.loop_tick_collect(0)) == want[2]
        assert bytes(chip.loop_tick(ls[3], p)) == want[3]         # the synchronous tick is a pass of its own
        chip.loop_tick_enqueue(ls[4], 5, p)
        chip.loop_tick_enqueue(ls[4] + 3, 6, p)
        # leaving the block destroys the ctx with two ticks parked: they are submitted and drained like any enqueued tick
    with make_chip(monkeypatch, 3) as chip:           # ... and the device is fine afterwards
        assert bytes(chip.loop_tick(ls[0], p)) == want[0]


def test_full_size_pipelined_ticks_equal_synchronous_ticks(monkeypatch):
    """1M rows (16.4 GB: long scans by the default bound), 16 ticks in flight, nothing forced: ticks park behind running scans as
    they do in bench.py.  Every record equals the synchronous tick's."""
    monkeypatch.delenv("CHIP_SCAN_OVERLAP_GIB", raising=False)
    monkeypatch.delenv("CHIP_TICK_COALESCE", raising=False)
    rows, p = 1_000_000, capi.default_dot_params()
    src = 123_456
    plants = [(rows - 40 - j, src - j, 1) for j in range(3)]
    ls = [rows - 90 + 3 * i for i in range(16)] + [rows - 39]     # the last tick's queries are the planted revisit
    with capi.Chip(D, capacity_hint=rows) as chip:
        chip.append_synthetic(rows, SEED, plants)
        want = [bytes(chip.loop_tick(l, p)) for l in ls]
        assert chip.coalesce_stats() == (0, 0)
        assert rec(want[-1]).found == 1 and rec(want[-1]).idx_prev == src and rec(want[0]).found == 0
        chip.loop_reset()
        assert pipelined(chip, ls, p, 16) == want
        passes, ticks = chip.coalesce_stats()
        assert passes >= 4 and ticks > passes          # a 2.4 ms scan outlasts the enqueues behind it


@pytest.mark.parametrize("tmax", [2, 3])
def test_shared_pass_at_its_pass_boundary(monkeypatch, tmax):
    """The shared pass gives every wave R = 4 rows per pass (one 8-wave workgroup per CU: W waves, 4 W rows per pass).  Windows of forced-
    parked ticks whose prefixes (a) lie on both sides of a pass boundary, (b) are ten rows, about W rows and the whole DB in ONE pass,
    (c) hold a duplicate pair whose upper copy is the LAST row of one tick and beyond the prefix of another: every record equals, byte
    for byte, the record of the same tick issued alone with coalescing off, one per window the CPU oracle's, and last_scan() says which
    kernel served the window."""
    p = every_tick_params()
    with make_chip(monkeypatch, tmax) as chip:          # the geometry, from a first forced window
        for s in range(tmax):
            chip.loop_tick_enqueue(L0 + 3 * s, s, p)
        ls = chip.last_scan()
        assert (ls["family"], ls["ticks"], ls["R"], ls["nq"], ls["elem"]) == ("multi", tmax, 4, 3 * tmax, 4), ls
        W, R = ls["grid"] * ls["block"] // 64, ls["R"]
        assert ls["n_rows"] == L0 + 3 * (tmax - 1) - 50 and 2 * R * W + 100 < N_ROWS
        for s in range(tmax):
            chip.loop_tick_collect(s)
    P = R * W
    windows = [[P - 2, P + 1, P + 4], [2 * P + 4, 2 * P - 2, 2 * P + 1], [P, 2 * P, P - 1], [10, W + 3, N_ROWS - 50], [N_ROWS - 50, W - 1, 10],
               [DUP_HI + 1, DUP_HI - 1, DUP_HI + 4], [DUP_HI, DUP_HI + 1, N_ROWS - 50]]       # prefixes k; the tick is l = k + 50
    windows = [w[:tmax] for w in windows] + ([[w[0], w[2]] for w in windows] if tmax == 2 else [])
    all_l = sorted({k + 50 for w in windows for k in w})
    alone, _ = one_by_one(monkeypatch, all_l, p)
    alone = dict(zip(all_l, alone))
    db = oracle_lib.synth_rows(SEED, range(N_ROWS), D, PLANTS)
    op = oracle_lib.default_params()
    op.min_new = -(1 << 30)
    with make_chip(monkeypatch, tmax) as chip:
        launches = chip.last_scan()["launches"]
        for w in windows:
            before = chip.coalesce_stats()
            for s, k in enumerate(w):
                chip.loop_tick_enqueue(k + 50, s, p)
            ls = chip.last_scan()
            launches += 1
            assert (ls["family"], ls["ticks"], ls["n_rows"], ls["launches"]) == ("multi", len(w), max(w), launches), (w, ls)
            assert tuple(a - b for a, b in zip(chip.coalesce_stats(), before)) == (1, len(w))
            got = [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]
            assert got == [alone[k + 50] for k in w], (w, [i for i, k in enumerate(w) if got[i] != alone[k + 50]])
            k = min(w)
            o = oracle_lib.LoopOracle(db, op).tick(k + 50)
            r = rec(got[w.index(k)])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
        # the planted pair: the tick whose LAST row is the upper copy reports it, the tick whose prefix ends just before it the lower copy
        assert list(rec(alone[DUP_HI + 1 + 50]).argmax) == [DUP_HI] * 3 and list(rec(alone[DUP_HI + 50]).argmax) == [DUP_LO] * 3
