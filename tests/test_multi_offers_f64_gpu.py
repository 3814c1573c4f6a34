"""GPU test of the offers of the shared pass on DOUBLE rows (cerebro_amd/csrc/kernels.hip db_scan_shared_f64).

The three shared-pass kernels run one skeleton: the same group pre-check and the same query-first walk of the offers.  So the cases of
tests/test_multi_offers_gpu.py -- those in which the pre-check and the walk could disagree: ties inside a group, twelve equal scores in
one wave, one pair entering per row, prefixes ending inside a group, lists that never fill -- are planted in a double-row DB as well
(`Cases` / `build_cases` are that module's, imported).  The rows are relja_like's of tests/test_f64_gpu.py (genuinely float64); it takes
the same (dst, src, kind) plants: kind 2 is an exact copy of src, kind 1 src plus noise of a fifth of its norm (cos ~ 0.98), as in
orc_synth_row_f32.  Double rows share a pass between T = 2 ticks; at D = 1024 all six queries are staged, at D = 3584 one of them is read
in place (NG = 1).  The bar is the float test's: every 64-byte record of a forced window equals, byte for byte, the record of the same
tick issued alone with coalescing off; one tick per window equals the CPU oracle's (orc_dot_tree_f64 order); where the planted rows
decide the answer, the expected row is asserted."""
import pytest

import oracle_lib
from cerebro_amd import capi
from test_f64_gpu import relja_like
from test_multi_offers_gpu import COPY, K, NOISY, R, SEED, build_cases, every_tick_params, rec

pytestmark = pytest.mark.gpu
T = 2
assert (COPY, NOISY) == (2, 1)          # relja_like: kind 2 copies src, every other kind adds noise to it


def make_chip(monkeypatch, D, db, coalesce):
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    monkeypatch.setenv("CHIP_TICK_COALESCE", str(coalesce))
    chip = capi.Chip(D, capacity_hint=len(db) + 64, storage="f64")
    chip.append_f64(db)
    if coalesce:
        chip.coalesce_force(True)
    return chip


def geometry(monkeypatch, D, staged, ng):
    """W of the launches of this machine, from a first forced window on a small DB; the window is served by the instantiation meant"""
    p = every_tick_params()
    with make_chip(monkeypatch, D, relja_like(SEED, 2_000, D), T) as chip:
        for s in range(T):
            chip.loop_tick_enqueue(1000 + 3 * s, s, p)
        ls = chip.last_scan()
        assert (ls["family"], ls["elem"], ls["ticks"], ls["R"], ls["nq"], ls["K"], ls["q64"], ls["NG"]) == ("multi", 8, T, R, 3 * T, K, staged, ng), ls
        for s in range(T):
            chip.loop_tick_collect(s)
    return ls["grid"] * ls["block"] // 64


@pytest.mark.parametrize("D,staged,ng", [(1024, 6, 0), (3584, 5, 1)])
def test_offers_on_double_rows_where_the_group_check_and_the_walk_could_disagree(monkeypatch, D, staged, ng):
    p = every_tick_params()
    W = geometry(monkeypatch, D, staged, ng)
    c = build_cases(W, T)
    assert not {src for _, src, _ in c.plants} & {dst for dst, _, _ in c.plants}      # relja_like plants one after another: no chains
    db = relja_like(SEED, c.n_rows, D, c.plants)
    db.setflags(write=False)
    all_l = sorted({k + 50 for w in c.windows for k in w})
    with make_chip(monkeypatch, D, db, 0) as ref:
        alone = {l: bytes(ref.loop_tick(l, p)) for l in all_l}
        assert ref.coalesce_stats() == (0, 0) and ref.last_scan()["family"] != "multi"
    op = oracle_lib.default_params()
    op.min_new = -(1 << 30)
    with make_chip(monkeypatch, D, db, T) as chip:
        for wi, w in enumerate(c.windows):
            before = chip.coalesce_stats()
            for s, k in enumerate(w):
                chip.loop_tick_enqueue(k + 50, s, p)
            ls = chip.last_scan()
            assert (ls["family"], ls["elem"], ls["ticks"], ls["n_rows"], ls["K"], ls["NG"]) == ("multi", 8, len(w), max(w), K, ng), (w, ls)
            assert ls["grid"] * ls["block"] // 64 == W
            assert tuple(a - b for a, b in zip(chip.coalesce_stats(), before)) == (1, len(w))
            got = [bytes(chip.loop_tick_collect(s)) for s in range(len(w))]
            assert got == [alone[k + 50] for k in w], (D, wi, w, [k for i, k in enumerate(w) if got[i] != alone[k + 50]])
            planted = sorted({s for (ww, s, _) in c.expect if ww == wi})
            for (ww, s, qi), row in c.expect.items():
                if ww == wi:
                    assert rec(got[s]).argmax[qi] == row, (D, wi, s, qi, row, list(rec(got[s]).argmax))
            s = planted[0]
            o = oracle_lib.LoopOracle64(db, op).tick(w[s] + 50)
            r = rec(got[s])
            assert r.status == capi.CHIP_TICK_SCANNED and list(r.argmax) == o["argmax"] and r.found == o["found"] and r.idx_prev == o["idx_prev"]
            assert [float(x).hex() for x in r.maxv] == [float(x).hex() for x in o["maxv"]] and float(r.score).hex() == float(o["score"]).hex()
