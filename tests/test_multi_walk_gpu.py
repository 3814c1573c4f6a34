"""GPU tests of the query-first walk of the offers of the shared pass (cerebro_amd/csrc/kernels.hip db_scan_topk_multi).

When a group of four rows sets a lane in the pre-check, the kernel walks the group's offers LIST BY LIST: for each query whose own compare
against its threshold sets a lane, the four rows in ascending order, each against the threshold as it stands by then, each behind the
tests `row < rows of the pass` and `row < prefix of the query's tick`.  Lists are independent of one another, so this admits what the
row-first walk admitted.  The harness and the bar are those of tests/test_multi_offers_gpu.py (its helpers are imported): forced-parked
windows at CHIP_SCAN_OVERLAP_GIB=0, every 64-byte record equal, byte for byte, to the record of the same tick issued alone with coalescing
off, one tick per window equal to the CPU oracle's record; and every planted answer is first confirmed by the oracle over the planted DB,
then asserted on the device.  The cases are those a query-first walk could get wrong and that file does not hold:

  (a) many pairs in one group: rows rr = 0..3 of one group each enter a different list, of two different ticks;
  (b) one row that enters T lists, one per tick, in one group: the ticks' prefixes are 10 rows apart, the first query rows of the later
      ticks are exact copies of the first tick's (a plant copies the UNPLANTED content of its source), and the row is a noisy copy of it;
  (c) a tie between rows rr = 1 and rr = 3 in one list (`>=`: the later index wins) while row rr = 2 enters another list of the same tick;
  (d) a row behind tick 0's prefix that beats the thresholds of a list of tick 0 and of the same list of tick T - 1 (whose first query is a
      copy of tick 0's), in a group where another row does enter tick 0's list: tick 0 answers the row it sees, tick T - 1 the later
      of two equal scores;
  (e) groups in which the stand-in of a row beyond the pass sets a lane: the first rows of two waves are exact copies of a query each, and
      the pass ends inside those waves' last groups, whose missing rows the kernel replaces by the wave's first row (a lane set, never
      offered).  Whether another lane of such a group is set as well is up to the unplanted rows: with top-8 lists after three groups
      a real row of the group very likely sets one too, so this is NOT strictly "a group whose only lane is the stand-in's".  What
      the case does catch: a stand-in wrongly offered would enter with the larger index, win the tie and change argmax.

The query-first walk admits exactly what the row-first walk admitted, so every case here passes on a row-first kernel as well: the file
guards against a WRONG reordering of the offers (same bytes as the tick alone, same answers as the oracle); it does not detect whether
the list-by-list walk or its step-over is in use, and nothing pins the walk's order.

T = 2 and T = 3 ticks per pass, D = 1024 and 4096, DB of 16 W + 1800 rows (W waves in the launch)."""
import pytest

import oracle_lib
from cerebro_amd import capi
from test_multi_offers_gpu import COPY, K, NOISY, R, SEED, Cases, every_tick_params, geometry, make_chip, rec

pytestmark = pytest.mark.gpu


def build_walk_cases(W, T):
    assert W > 64, W               # the waves used below exist, and a row one group-row later has the larger index
    c = Cases(W, T)

    def close(n):
        """a hand-made window of T prefixes n rows apart"""
        ks = [c._next_k + n * s for s in range(T)]
        c._next_k += 60 * T
        assert ks[-1] + 50 <= c.n_rows
        c.windows.append(ks)
        return len(c.windows) - 1, ks

    # (a) four rows of one group, four lists of two ticks
    w, ks = c.whole()
    for rr, (s, qi) in enumerate([(0, 0), (1, 1), (0, 2), (1, 0)]):
        c.plant(c.pos(12, 3, rr), ks[s], qi, NOISY)
        c.expect[(w, s, qi)] = c.pos(12, 3, rr)
    # (b) one row, T lists: no query row of the window lies inside a prefix of the window
    w, ks = close(10)
    for s in range(1, T):
        c.plants.append((ks[s] + 49, ks[0] + 49, COPY))
    c.plant(c.pos(17, 2, 1), ks[0], 0, NOISY)
    for s in range(T):
        c.expect[(w, s, 0)] = c.pos(17, 2, 1)
    # (c) a tie of rows 1 and 3 in one list, row 2 into another list of the same tick
    w, ks = c.whole()
    for rr in (1, 3):
        c.plant(c.pos(23, 2, rr), ks[T - 1], 0, COPY)
    c.plant(c.pos(23, 2, 2), ks[T - 1], 1, NOISY)
    c.expect[(w, T - 1, 0)] = c.pos(23, 2, 3)
    c.expect[(w, T - 1, 1)] = c.pos(23, 2, 2)
    # (d) tick 0 sees rows 0, 1 of wave 31's group 2; row 3 of the group is an exact copy of tick 0's first query, which is tick T - 1's too
    ks = [c.pos(31, 2, 2)] + ([c.pos(32, 2, 1)] if T == 3 else []) + [16 * W + 1700]
    c.windows.append(ks)
    w = len(c.windows) - 1
    c.plant(c.pos(31, 2, 1), ks[0], 0, NOISY)
    c.plants.append((c.pos(31, 2, 3), ks[0] + 49, COPY))
    c.plants.append((ks[T - 1] + 49, ks[0] + 49, COPY))
    c.expect[(w, 0, 0)] = c.pos(31, 2, 1)
    assert ks[0] + 49 < c.pos(31, 2, 3) < ks[T - 1]
    c.expect[(w, T - 1, 0)] = c.pos(31, 2, 3)          # ties with row ks[0] + 49, the query itself, and has the larger index
    # (e) the pass ends behind row 1 of group 3 of waves 40 and 41: their rows 2, 3 are stood in for by rows 40 and 41
    end = c.pos(40, 3, 2)
    ks = [end - 10 * (T - 1 - s) for s in range(T)]
    c.windows.append(ks)
    w = len(c.windows) - 1
    c.plant(40, ks[T - 1], 0, COPY)
    c.plant(41, ks[0], 1, COPY)
    c.expect[(w, T - 1, 0)] = 40
    c.expect[(w, 0, 1)] = 41
    c.plants.sort()
    assert len({d for d, _, _ in c.plants}) == len(c.plants)
    return c


@pytest.mark.parametrize("D,tmax", [(1024, 3), (1024, 2), (4096, 3), (4096, 2)])
def test_query_first_walk_admits_what_the_row_first_walk_admitted(monkeypatch, D, tmax):
    p = every_tick_params()
    W = geometry(monkeypatch, D, tmax)
    c = build_walk_cases(W, tmax)
    n_rows = c.n_rows
    db = oracle_lib.synth_rows(SEED, range(n_rows), D, c.plants)
    op = oracle_lib.default_params()
    op.min_new = -(1 << 30)
    oracle = {}
    for (wi, s, qi), row in c.expect.items():          # the plants decide the answers: said by the oracle before the device is asked
        l = c.windows[wi][s] + 50
        if l not in oracle:
            oracle[l] = oracle_lib.LoopOracle(db, op).tick(l)
        assert oracle[l]["argmax"][qi] == row, (D, tmax, wi, s, qi, row, oracle[l]["argmax"])
    all_l = sorted({k + 50 for w in c.windows for k in w})
    with make_chip(monkeypatch, D, n_rows, 0, c.plants) as ref:
        alone = {l: bytes(ref.loop_tick(l, p)) for l in all_l}
        assert ref.coalesce_stats() == (0, 0)
    with make_chip(monkeypatch, D, n_rows, tmax, c.plants) as chip:
        for wi, w in enumerate(c.windows):
            before = chip.coalesce_stats()
            for s, k in enumerate(w):
                chip.loop_tick_enqueue(k + 50, s, p)
            ls = chip.last_scan()
            assert (ls["family"], ls["ticks"], ls["n_rows"], ls["K"]) == ("multi", len(w), max(w), K), (w, ls)
            assert ls["grid"] * ls["block"] // 64 == W and ls["R"] == R
            assert tuple(a - b for a, b in zip(chip.coalesce_stats(), before)) == (1, len(w))
            got = [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]
            assert got == [alone[k + 50] for k in w], (D, tmax, wi, w, [k for i, k in enumerate(w) if got[i] != alone[k + 50]])
            for (ww, s, qi), row in c.expect.items():
                if ww == wi:
                    assert rec(got[s]).argmax[qi] == row, (D, tmax, wi, s, qi, row, list(rec(got[s]).argmax))
            s = min(s for (ww, s, _) in c.expect if ww == wi)
            o = oracle[w[s] + 50]
            r = rec(got[s])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
