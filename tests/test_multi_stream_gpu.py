"""GPU tests of the shared pass (cerebro_amd/csrc/kernels.hip db_scan_topk_multi) at the edges of its load stream.

A wave of that kernel walks its rows as ONE stream of 1 KiB loads: a load slot is issued again, for the data that comes next, as soon
as its contents have been converted -- across the KiBs of a 4 KiB batch, across the batches of a row, across the boundary between two
groups of R = 4 rows, and through the reduction and the offers.  The bar is the one of tests/test_tick_coalesce_gpu.py: every 64-byte
record of a forced-parked window equals, byte for byte, the record of the same tick issued alone with coalescing off, and one tick
per window equals the CPU oracle's.  The prefixes are the ones a pipelined stream can get wrong:

  * a pass shorter than one row per wave (most waves own nothing and must load nothing);
  * waves with zero, one, a partial and exactly one group of R rows (W waves: W, W + 5, R W - 1, R W, R W + 1 rows), and prefixes one
    row before / on / after the next multiples of R W (a wave's last group follows its last-but-one without a gap);
  * prefixes that end one row before / on / after a segment boundary of the DB (the read-ahead of the group that straddles it takes
    every row base from the segment table);
  * the whole DB;

at D = 1024 (one batch per row: the stream crosses a group boundary at every batch), D = 4096 (two and three ticks per pass) and
D = 6144 (two ticks: what still fits the LDS).  The ticks of a window have different prefixes, so a row is offered to some lists and
not to others."""
import numpy as np
import pytest

import oracle_lib
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
SEED = 424243
SEG_BYTES = 512 << 20            # float rows: a segment holds the largest power of two of rows within this


def every_tick_params():
    p = capi.default_dot_params()
    p.min_new = -(1 << 30)          # every tick runs, whatever the previous l was
    return p


def make_chip(monkeypatch, D, rows, coalesce):
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    monkeypatch.setenv("CHIP_TICK_COALESCE", str(coalesce))
    chip = capi.Chip(D, capacity_hint=rows + 64)
    chip.append_synthetic(rows, SEED, ())
    if coalesce:
        chip.coalesce_force(True)
    return chip


def rec(b):
    return capi.TickResult.from_buffer_copy(b)


def seg_rows(D):
    n = 1
    while 2 * n * D * 4 <= SEG_BYTES:
        n *= 2
    return n


def edge_prefixes(W, R, n_rows, seg):
    P = R * W
    ks = [60, W // 3, W - 1, W, W + 5, 2 * W, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, n_rows - 50]
    if seg + 1 <= n_rows - 50:
        ks += [seg - 1, seg, seg + 1]
    return sorted(set(ks))


@pytest.mark.parametrize("D,tmax,n_rows", [(1024, 3, 20_000), (1024, 2, 20_000), (4096, 3, 33_100), (4096, 2, 33_100), (6144, 2, 17_000)])
def test_forced_windows_at_the_edges_of_the_stream(monkeypatch, D, tmax, n_rows):
    p = every_tick_params()
    seg = seg_rows(D)
    with make_chip(monkeypatch, D, n_rows, tmax) as chip:      # the geometry, from a first forced window
        for s in range(tmax):
            chip.loop_tick_enqueue(1000 + 3 * s, s, p)
        ls = chip.last_scan()
        assert (ls["family"], ls["ticks"], ls["R"], ls["nq"], ls["elem"], ls["wg_per_cu"]) == ("multi", tmax, 4, 3 * tmax, 4, 1), ls
        assert ls["lds_bytes"] >= 3 * tmax * D * 4 and ls["lds_bytes"] <= 160 * 1024
        W, R = ls["grid"] * ls["block"] // 64, ls["R"]
        for s in range(tmax):
            chip.loop_tick_collect(s)
    ks = edge_prefixes(W, R, n_rows, seg)
    assert 2 * R * W + 1 <= n_rows - 50, "the DB of this test must hold more than two full groups per wave"
    if D == 4096:
        assert seg + 1 <= n_rows - 50, "the DB of this test must cross a segment boundary"
    # windows: neighbours in the sorted list (prefixes a few rows apart share a pass) and far-apart ones (the short tick rides a long pass)
    near = [ks[i:i + tmax] for i in range(0, len(ks) - tmax + 1, tmax)]
    far = [[ks[i], ks[-1 - i]] + ([ks[len(ks) // 2]] if tmax == 3 else []) for i in range(3)]
    windows = near + far + [[ks[-1]] * tmax]
    all_l = sorted({k + 50 for w in windows for k in w})
    with make_chip(monkeypatch, D, n_rows, 0) as ref:
        alone = {l: bytes(ref.loop_tick(l, p)) for l in all_l}
        assert ref.coalesce_stats() == (0, 0)
    db = oracle_lib.synth_rows(SEED, range(n_rows), D, ())
    op = oracle_lib.default_params()
    op.min_new = -(1 << 30)
    with make_chip(monkeypatch, D, n_rows, tmax) as chip:
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
            assert got == [alone[k + 50] for k in w], (D, tmax, w, [k for i, k in enumerate(w) if got[i] != alone[k + 50]])
            k = w[len(w) // 2]
            o = oracle_lib.LoopOracle(db, op).tick(k + 50)
            r = rec(got[len(w) // 2])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
