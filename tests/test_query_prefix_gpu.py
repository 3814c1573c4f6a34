"""Many-query mode with a prefix PER QUERY (chip_query_batch_rows_f32, chip_query_batch_prefix_f32 and their cast forms; kernels
gather_query_tiles and db_gemm_prefixed of cerebro_amd/csrc/batch.hip).  Definition: entry j of a call is, bit for bit, what
chip_query_batch_f32(k[j], q_j, 1, topk) returns; the oracle per query is oracle_lib.scan_topk_fmaf(db, k_j, q_j, K), grouped by
distinct k.  Bar: indices equal and fp32 score bits equal.  The oracle answers every (pattern, query) once with its top-16 list; the
top-K list of a total order is its first K entries.

Shapes, the smallest that reach each path: (128, 5000, 600) with the grid capped to 1 / 3 / 19 workgroups (claimed tiles and query
halves, the 128 tile), (64, 1500, 512) (the 256 tile and its two 128-column epilogue passes), (4096, 2000, 130) (128 K-chunks)."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import scenarios
from cerebro_amd import capi
from test_batch_cast_gpu import f32bits, relja_like
from test_batch_edges_gpu import SEG_D, compare, merged, open_chip, seg_rows, set_wgs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EDGE_K = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LAG = 50


def want_lists(db32, q, k):
    """the oracle's top-16 list of every query j over rows [0, k[j]): one scan per distinct k"""
    ws = np.empty((len(k), 16), dtype=np.float64)
    wi = np.empty((len(k), 16), dtype=np.int64)
    for kk in np.unique(k):
        sel = np.nonzero(k == kk)[0]
        ws[sel], wi[sel] = oracle_lib.scan_topk_fmaf(db32, int(kk), q[sel], 16)
    return ws, wi


@functools.lru_cache(maxsize=None)
def case(D, N, Q, storage):
    """the DB of a shape and its patterns: name -> (rows, k, want scores, want indices); computed once, never written to"""
    plants, loops, ties = scenarios.loop_plants(N, 4, seed=D + Q)
    db = relja_like(7 * D, N, D, plants) if storage == "f64" else scenarios.build_db(7 * D, N, D, plants)
    db32 = db.astype(np.float32)
    rng = np.random.default_rng(D + N + Q)
    s, t1, t2 = ties[0]                                       # rows t1 < t2 are bit-identical copies of row s < t1
    planted = {int(r) for p in plants for r in p[:2]} | {int(r) for t in ties for r in t}
    lone = next(r for r in range(N // 2, N) if r not in planted)   # a row nothing is a copy of
    pats = {}
    rows = np.arange(N - Q, N, dtype=np.int64)                # self-join: consecutive rows at lag 50
    pats["self_join"] = (rows, np.maximum(0, rows - LAG))
    rows, k = rng.integers(0, N, Q), rng.integers(0, N + 1, Q)   # unsorted random prefixes: the permutation
    rows[:5], k[:5] = (t1, t1, lone, N - 1, 0), (t2, t2 + 1, lone + 1, N, 0)   # ties (only t1 | t2 first), self-match, the ends
    pats["random"] = (rows, k)
    pats["all_equal"] = (rng.integers(0, N, Q), np.full(Q, N - LAG))
    Qe = 256 if Q % 256 == 0 else 128                         # ONE query tile whose limits fall in either 64-column half, either
    pats["edges"] = (rng.integers(0, N, Qe), np.array([EDGE_K[j % len(EDGE_K)] for j in range(Qe)]))   # pass and at the tile edge
    k = rng.integers(0, N + 1, Q)
    k[rng.permutation(Q)[:min(256, Q - 1)]] = 0               # a whole query tile (either shape) of k = 0 after the sort
    pats["empty_tile"] = (rng.integers(0, N, Q), k)
    out = {}
    for name, (rows, k) in pats.items():
        rows, k = np.asarray(rows, dtype=np.int64), np.asarray(k, dtype=np.int64)
        out[name] = (rows, k) + want_lists(db32, db32[rows], k)
    return db, db32, out, (s, t1, t2, lone)


def check_rows(chip, pat, K, cast, ctx):
    rows, k, ws, wi = pat
    compare(chip.query_batch_rows(rows, k, K, cast_rows=cast), (ws[:, :K], wi[:, :K]), ctx)


PARAMS = [(128, 5000, 600, 1), (128, 5000, 600, 3), (128, 5000, 600, 19), (64, 1500, 512, 0), (4096, 2000, 130, 0)]


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("D,N,Q,wgs", PARAMS)
def test_prefix_per_query_against_the_oracle(D, N, Q, wgs, storage, monkeypatch):
    db, db32, pats, (s, t1, t2, lone) = case(D, N, Q, storage)
    cast = storage == "f64"
    set_wgs(monkeypatch, wgs)
    with open_chip(D, db, storage) as chip:
        for K in (1, 8, 16):
            for name, pat in pats.items():
                check_rows(chip, pat, K, cast, f"{name} {storage} D={D} N={N} Q={Q} wgs={wgs} K={K}")
            # host vectors through the same kernels: the float casts of the same rows
            rows, k, ws, wi = pats["random"]
            compare(chip.query_batch_prefix(k, db32[rows], K, cast_rows=cast), (ws[:, :K], wi[:, :K]), f"host vectors {storage} K={K}")
            # all k equal: the bits of the one-prefix call on the same vectors
            rows, k, ws, wi = pats["all_equal"]
            one = chip.query_batch(int(k[0]), db32[rows], K, cast_rows=cast)
            got = chip.query_batch_rows(rows, k, K, cast_rows=cast)
            assert np.array_equal(got[1], one[1]) and np.array_equal(f32bits(got[0]), f32bits(one[0])), (storage, K)
        # what the crafted entries of "random" must show (K = 16 lists)
        gs, gi = chip.query_batch_rows(*pats["random"][:2], 16, cast_rows=cast)
        assert list(gi[0][:2]) == [t1, s] and gs[0][0] == gs[0][1]            # k = t2: of the duplicates only t1 and s are visible
        assert list(gi[1][:3]) == [t2, t1, s] and gs[1][0] == gs[1][2]        # k = t2 + 1: t2 first (index descending)
        assert gi[2][0] == lone                                              # k > row: the row finds itself
        assert gi[3][0] == N - 1
        assert (gi[4] == -1).all() and np.isneginf(gs[4]).all()               # k = 0
        # a whole query tile of k = 0: all -inf / -1
        rows, k = pats["empty_tile"][:2]
        gs, gi = chip.query_batch_rows(rows, k, 8, cast_rows=cast)
        assert (k == 0).sum() >= 129 and (gi[k == 0] == -1).all() and np.isneginf(gs[k == 0]).all()
        if cast:                                                             # the _f32 entries keep refusing double rows
            for call in (lambda: chip.query_batch_rows(rows, k, 8), lambda: chip.query_batch_prefix(k, db32[rows], 8)):
                with pytest.raises(capi.ChipError) as e:
                    call()
                assert e.value.status == capi.CHIP_ERR_UNSUPPORTED


def test_self_join_stub_is_the_rows_call():
    D, N, Q = 64, 1500, 512
    db, db32, pats, _ = case(D, N, Q, "f32")
    rows, k, ws, wi = pats["self_join"]
    with open_chip(D, db, "f32") as chip:
        compare(chip.self_join(N - Q, Q, LAG, 5), (ws[:, :5], wi[:, :5]), "self_join")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_prefix_across_a_segment_boundary(storage, monkeypatch):
    """Query rows and prefixes on both sides of a segment boundary (8192 rows per segment at D = 8224).  Both loaders of the prefix
    kernel take ONE segment base per DB tile and 32-bit offsets; the gather takes every query row's base from the segment table."""
    D, seg = SEG_D, seg_rows(SEG_D)
    n = seg + 300
    db = relja_like(4242, n, D)
    if storage == "f32":
        db = db.astype(np.float32)
    db[seg] = db[seg - 1]                                     # an exact duplicate pair across the boundary
    db32 = db.astype(np.float32)
    rows = np.array([seg, seg - 1, seg - 1, 100, seg + 1, n - 1, seg + 299, 5, seg, seg - 2, 0, seg + 128], dtype=np.int64)
    k = np.array([seg, seg, seg + 1, n, seg + 1, seg - 1, seg + 129, seg + 257, n, seg + 127, seg + 256, seg - 1], dtype=np.int64)
    q = db32[rows]
    head = oracle_lib.scan_topk_fmaf(db32, seg - 1, q, 16)                   # once; the short tail [seg - 1, k) per prefix
    ws, wi = np.empty((len(k), 16)), np.empty((len(k), 16), dtype=np.int64)
    for kk in np.unique(k):
        sel = np.nonzero(k == kk)[0]
        tail = oracle_lib.scan_topk_fmaf(db32[seg - 1:], int(kk) - (seg - 1), q[sel], 16)
        ws[sel], wi[sel] = merged((head[0][sel], head[1][sel]), tail, seg - 1, 16)
    assert list(wi[0][:1]) == [seg - 1] and list(wi[2][:2]) == [seg, seg - 1]   # the duplicates: below the boundary only | both
    with open_chip(D, db, storage) as chip:
        assert chip.info()["capacity_local"] == 2 * seg                      # two segments, or this test shows nothing
        for wgs in (0, 3):
            set_wgs(monkeypatch, wgs)
            for K in (8, 16):
                got = chip.query_batch_rows(rows, k, K, cast_rows=storage == "f64")
                compare(got, (ws[:, :K], wi[:, :K]), f"segments {storage} rows wgs={wgs} K={K}")
        got = chip.query_batch_prefix(k, q, 8, cast_rows=storage == "f64")
        compare(got, (ws[:, :8], wi[:, :8]), f"segments {storage} host vectors")


def test_three_groups_and_the_kernels_own_tile_count():
    """(32, 9000, 9000) self-join at lag 50: groups of 4096, 4096 and 808 queries.  units_claimed is the sum of the work counters the
    GEMM advanced itself (read back after each launch): the kernel is shown to walk the triangle, not the rectangle."""
    D, N = 32, 9000
    db = scenarios.build_db(32, N, D, [])
    rows = np.arange(N, dtype=np.int64)
    k = np.maximum(0, rows - LAG)
    ws, wi = want_lists(db, db, k)
    plan = capi.query_prefix_plan(k, 4, 5)
    assert plan["groups"] == 3 and plan["units"] < plan["units_rect"]
    with open_chip(D, db, "f32") as chip:
        compare(chip.self_join(0, N, LAG, 5), (ws[:, :5], wi[:, :5]), "three groups")
        last = chip.debug_query_prefix_last()
        print(last, plan["units"], plan["units_rect"])
        assert last["groups"] == 3 and last["waits"] <= 3 and last["launches"] == 9
        assert last["units_claimed"] == last["units_planned"] == plan["units"]
        chip.query_batch_prefix(k[:300], db[:300], 5)
        last = chip.debug_query_prefix_last()
        assert (last["groups"], last["launches"]) == (1, 3) and last["units_claimed"] == last["units_planned"]


def test_errors_and_the_ctx_afterwards():
    D, N = 64, 700
    db = scenarios.build_db(5, N, D, [])
    rows = np.arange(100, 400, dtype=np.int64)
    k = rows - LAG
    ws, wi = want_lists(db, db[rows], k)
    R, U, A = capi.CHIP_ERR_RANGE, capi.CHIP_ERR_UNSUPPORTED, capi.CHIP_ERR_INVALID_ARG

    def refused(status, call):
        with pytest.raises(capi.ChipError) as e:
            call()
        assert e.value.status == status

    with open_chip(D, db, "f32") as chip:
        bad = k.copy()
        bad[7] = -1
        refused(R, lambda: chip.query_batch_rows(rows, bad, 5))
        bad[7] = N + 1
        refused(R, lambda: chip.query_batch_rows(rows, bad, 5))
        refused(R, lambda: chip.query_batch_prefix(bad, db[rows], 5))
        bad = rows.copy()
        bad[299] = N
        refused(R, lambda: chip.query_batch_rows(bad, k, 5))
        bad[299] = -1
        refused(R, lambda: chip.query_batch_rows(bad, k, 5))
        refused(U, lambda: chip.query_batch_rows(rows, k, 0))
        refused(U, lambda: chip.query_batch_rows(rows, k, capi.CHIP_MAX_TOPK + 1))
        refused(A, lambda: chip.query_batch_rows(rows[:0], k[:0], 5))        # Q < 1
        sc, ix = np.zeros((300, 5), dtype=np.float32), np.zeros((300, 5), dtype=np.int64)
        for args in ((None, capi._ptr(k)), (capi._ptr(rows), None)):         # a NULL pointer
            assert chip.lib.chip_query_batch_rows_f32(chip.h, args[0], args[1], 300, 5, capi._ptr(sc), capi._ptr(ix)) == A
        assert chip.lib.chip_query_batch_rows_f32(chip.h, capi._ptr(rows), capi._ptr(k), 300, 5, None, capi._ptr(ix)) == A
        assert chip.lib.chip_query_batch_prefix_f32(chip.h, capi._ptr(k), None, 300, 5, capi._ptr(sc), capi._ptr(ix)) == A
        assert not sc.any() and not ix.any()                                 # nothing was written
        # the ctx afterwards: a valid call and a tick give the oracle's answers
        compare(chip.query_batch_rows(rows, k, 5), (ws[:, :5], wi[:, :5]), "after the refused calls")
        orc = oracle_lib.LoopOracle(db)
        for l in scenarios.default_schedule(N)[-3:]:
            chip.loop_reset()
            orc.state.last_l = 0
            g_, o_ = chip.loop_tick(l).as_dict(), orc.tick(l)
            assert (g_["found"], g_["argmax"]) == (o_["found"], o_["argmax"])
    with capi.Chip(36) as chip:                                               # D % 32 != 0
        chip.append_f32(np.full((4, 36), 0.1, dtype=np.float32))
        refused(U, lambda: chip.query_batch_rows([1, 2], [1, 1], 2))
    with capi.Chip(D, devices=[0, 0]) as chip:                                # a group ctx
        chip.append_f32(db)
        refused(U, lambda: chip.query_batch_rows(rows, k, 5))
    with capi.Chip(D, shard_rank=0, shard_count=2) as chip:                   # a sharded ctx
        chip.append_f32(db)
        refused(U, lambda: chip.query_batch_rows(rows, k, 5))
        refused(U, lambda: chip.query_batch_prefix(k, db[rows], 5))


def test_self_join_example_prints_all_equal():
    exe = ROOT / "cerebro_amd" / "lib" / "self_join"
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout, r.stdout
