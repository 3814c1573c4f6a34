"""GPU tests of the offers of the shared pass (cerebro_amd/csrc/kernels.hip db_scan_topk_multi).

When the four rows of a group are complete the kernel holds, per query, the four rows' scores in the four 16-lane rows of one register.
ONE vector compare per query against the admission thresholds the group starts with decides whether any (row, query) pair of the group
is offered at all; only then are the rows walked one by one (row ascending, query ascending, each against the threshold as it stands
by then, `>=`: the later index wins a tie).  These are the cases in which that pre-check and the walk could disagree.  The bar is the
one of tests/test_multi_stream_gpu.py: every 64-byte record of a forced-parked window equals, byte for byte, the record of the same tick
issued alone with coalescing off, and one tick per window equals the CPU oracle's; where the planted rows decide the answer, the
expected row is asserted as well.  With W waves in the launch, wave g owns rows g, g + W, g + 2 W, ... and its group j holds rows
g + (4 j + rr) W, rr = 0..3 (`Chip.last_scan()` gives W); the pass keeps K = 8 entries per wave and query, whatever the caller asks.

  (a) ties: exact copies of a tick's query row, so that equal scores meet -- two and four in one group (the walk must see the threshold
      rise inside the group), twelve in three consecutive groups of one wave (a full list of equal scores: the ninth meets the K-th
      entry with `>=`), ten in ten waves (the merge decides);
  (b) a group in which one (row, query) pair enters a list, for each of the four rows and a query of each tick;
  (c) ticks whose prefixes end inside a group: a score above the threshold that belongs to a row the tick must not see (an exact copy,
      behind the prefix) next to a lower one that it sees (a noisy copy);
  (d) prefixes shorter than K rows per wave: lists that never fill, thresholds that stay -inf, with a tie planted.

T = 2 and T = 3 ticks per pass, D = 1024 and 4096."""
import pytest

import oracle_lib
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
SEED = 515253
R, K = 4, 8
COPY, NOISY = 2, 1          # kinds of planted rows (oracle/dot_scan.c orc_synth_row_f32): exact copy of src, 5 src + noise (cos ~ 0.98)


def every_tick_params():
    p = capi.default_dot_params()
    p.min_new = -(1 << 30)          # every tick runs, whatever the previous l was
    return p


def make_chip(monkeypatch, D, rows, coalesce, plants=()):
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    monkeypatch.setenv("CHIP_TICK_COALESCE", str(coalesce))
    chip = capi.Chip(D, capacity_hint=rows + 64)
    chip.append_synthetic(rows, SEED, plants)
    if coalesce:
        chip.coalesce_force(True)
    return chip


def rec(b):
    return capi.TickResult.from_buffer_copy(b)


def geometry(monkeypatch, D, tmax):
    """W of the launches of this machine, from a first forced window on a small DB"""
    p = every_tick_params()
    with make_chip(monkeypatch, D, 2_000, tmax) as chip:
        for s in range(tmax):
            chip.loop_tick_enqueue(1000 + 3 * s, s, p)
        ls = chip.last_scan()
        assert (ls["family"], ls["ticks"], ls["R"], ls["nq"], ls["K"]) == ("multi", tmax, R, 3 * tmax, K), ls
        for s in range(tmax):
            chip.loop_tick_collect(s)
    return ls["grid"] * ls["block"] // 64


class Cases:
    """windows (lists of prefixes k; the tick is l = k + 50 and its queries are rows k + 49, k + 48, k + 47), the rows planted for them and
    the answers the plants dictate: expect[(window, tick, query)] = row"""

    def __init__(self, W, T):
        self.W, self.T = W, T
        self.n_rows = 16 * W + 1800
        self.windows, self.plants, self.expect = [], [], {}
        self._next_k = 16 * W + 100

    def pos(self, g, j, rr):
        return g + (R * j + rr) * self.W

    def whole(self):
        """a window of T prefixes that cover four full groups of every wave, 60 rows apart (no query row of one is one of another)"""
        ks = [self._next_k + 60 * s for s in range(self.T)]
        self._next_k += 60 * self.T
        assert ks[-1] + 50 <= self.n_rows
        self.windows.append(ks)
        return len(self.windows) - 1, ks

    def plant(self, dst, k, qi, kind):
        assert all(d != dst for d, _, _ in self.plants) and dst < k
        self.plants.append((dst, k + 49 - qi, kind))


def build_cases(W, T):
    c = Cases(W, T)
    # (a) ties in one group: four copies for tick 0 / query 0, two for tick 1 / query 1
    w, ks = c.whole()
    for rr in range(R):
        c.plant(c.pos(5, 2, rr), ks[0], 0, COPY)
    c.expect[(w, 0, 0)] = c.pos(5, 2, 3)
    for rr in (1, 2):
        c.plant(c.pos(7, 3, rr), ks[1], 1, COPY)
    c.expect[(w, 1, 1)] = c.pos(7, 3, 2)
    # (a) twelve copies in three consecutive groups of one wave, for the last tick
    w, ks = c.whole()
    for j in (1, 2, 3):
        for rr in range(R):
            c.plant(c.pos(11, j, rr), ks[T - 1], 0, COPY)
    c.expect[(w, T - 1, 0)] = c.pos(11, 3, 3)
    # (a) ten copies in ten waves of several workgroups, same group number and row
    w, ks = c.whole()
    for g in range(20, 30):
        c.plant(c.pos(g, 2, 1), ks[0], 2, COPY)
    c.expect[(w, 0, 2)] = c.pos(29, 2, 1)
    # (b) one pair of a group enters a list: row rr of the group, a query of tick rr % T
    for rr in range(R):
        w, ks = c.whole()
        s, qi = rr % T, rr % 3
        c.plant(c.pos(40 + rr, 3, rr), ks[s], qi, NOISY)
        c.expect[(w, s, qi)] = c.pos(40 + rr, 3, rr)
    # (c) prefixes that end inside a group of wave 50: tick 0 sees rows rr = 0, 1 of the group, the last tick the whole DB
    ks = [c.pos(50, 2, 2)] + ([c.pos(51, 2, 1)] if T == 3 else []) + [16 * W + 1700]
    c.windows.append(ks)
    w = len(c.windows) - 1
    c.plant(c.pos(50, 2, 1), ks[0], 0, NOISY)
    c.plants.append((c.pos(50, 2, 3), ks[0] + 49, COPY))          # behind tick 0's prefix, inside the pass
    c.expect[(w, 0, 0)] = c.pos(50, 2, 1)
    if T == 3:                                                    # tick 1 ends after row 0 of wave 51's group: its copy in row 2 is not for it
        c.plant(c.pos(51, 2, 0), ks[1], 1, NOISY)
        c.plants.append((c.pos(51, 2, 2), ks[1] + 48, COPY))
        c.expect[(w, 1, 1)] = c.pos(51, 2, 0)
    # (d) lists that never fill: fewer than K rows per wave in every prefix, a tie in wave 3's first group
    ks = [W + 9, 3 * W + 7, 7 * W - 1][:T]
    c.windows.append(ks)
    w = len(c.windows) - 1
    for rr in (0, 1):
        c.plant(c.pos(3, 0, rr), ks[T - 1], 0, COPY)
    c.expect[(w, T - 1, 0)] = c.pos(3, 0, 1)
    c.plants.sort()
    return c


@pytest.mark.parametrize("D,tmax", [(1024, 3), (1024, 2), (4096, 3), (4096, 2)])
def test_offers_where_the_group_check_and_the_walk_could_disagree(monkeypatch, D, tmax):
    p = every_tick_params()
    W = geometry(monkeypatch, D, tmax)
    c = build_cases(W, tmax)
    n_rows = c.n_rows
    all_l = sorted({k + 50 for w in c.windows for k in w})
    with make_chip(monkeypatch, D, n_rows, 0, c.plants) as ref:
        alone = {l: bytes(ref.loop_tick(l, p)) for l in all_l}
        assert ref.coalesce_stats() == (0, 0)
    db = oracle_lib.synth_rows(SEED, range(n_rows), D, c.plants)
    op = oracle_lib.default_params()
    op.min_new = -(1 << 30)
    with make_chip(monkeypatch, D, n_rows, tmax, c.plants) as chip:
        for wi, w in enumerate(c.windows):
            before = chip.coalesce_stats()
            for s, k in enumerate(w):
                chip.loop_tick_enqueue(k + 50, s, p)
            ls = chip.last_scan()
            assert (ls["family"], ls["ticks"], ls["n_rows"], ls["K"]) == ("multi", len(w), max(w), K), (w, ls)
            assert ls["grid"] * ls["block"] // 64 == W
            assert tuple(a - b for a, b in zip(chip.coalesce_stats(), before)) == (1, len(w))
            got = [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]
            assert got == [alone[k + 50] for k in w], (D, tmax, wi, w, [k for i, k in enumerate(w) if got[i] != alone[k + 50]])
            planted = sorted({s for (ww, s, _) in c.expect if ww == wi})
            for (ww, s, qi), row in c.expect.items():
                if ww == wi:
                    assert rec(got[s]).argmax[qi] == row, (D, tmax, wi, s, qi, row, list(rec(got[s]).argmax))
            s = planted[0]
            o = oracle_lib.LoopOracle(db, op).tick(w[s] + 50)
            r = rec(got[s])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
