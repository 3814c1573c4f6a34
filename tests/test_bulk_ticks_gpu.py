"""GPU tests of chip_loop_ticks_bulk (cerebro_amd/csrc/batch.hip; kernels.hip bulk_tick_finish).  The bar of every case: each record equals,
byte for byte, the record of the same tick in the loop of chip_loop_tick on the same ctx after chip_loop_reset, each list equals
chip_query_rows' bit for bit, the loop state returned equals chip_loop_last_l after that loop, and (where the DB is small) the records equal
the CPU oracle's tick.  What a case adds is said with it.

Two things to know when reading the cases (tests/test_bulk_ticks_mirror.py has the reasoning):
  * KL equal rows at the top with the rest far below fill the list, so M is the score of the best and M < G - 2 E cannot hold: that tick is
    NOT certified and runs again exactly; KL - 1 equal rows is the largest such set that certifies.  Both are tested, the winner the highest index.
  * 4300 rows walked at l = 56, 59, ... to the end give 1415 scanned ticks, whose last group (150 queries) pads to 256 and takes the 256 tile
    like the full one.  The schedule stops at 1405 ticks (120 queries in the last group: the 128 tile), and a call of 100 ticks (300
    queries: three 128-query tiles) is walked next to it."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_mirror_bulk_ticks as nm
import oracle_lib
from cerebro_amd import capi
from test_batch_cast_gpu import relja_like
from test_bulk_ticks_mirror import misordered_db, unit_rows

pytestmark = pytest.mark.gpu
SCANNED = capi.CHIP_TICK_SCANNED


def params(**kw):
    p = capi.default_dot_params()
    for name, v in kw.items():
        setattr(p, name, v)
    return p


def orc_params(p):
    o = oracle_lib.default_params()
    o.locality, o.thresh, o.lag, o.min_new, o.min_k = p.locality, p.thresh, p.lag, p.min_new, p.min_k
    return o


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_bulk(chip, ls, topk, p=None, db=None, lists=True):
    """the bulk call over ls against the loop of ticks, chip_query_rows and (db given) the oracle.  -> (records, scores, idx, debug read-back)"""
    p = p or capi.default_dot_params()
    chip.loop_reset()
    want = [bytes(chip.loop_tick(l, p)) for l in ls]
    want_last = chip.last_l()
    chip.loop_reset()
    recs, sc, ix, last = chip.loop_ticks_bulk(ls, p, 0, topk)
    dbg = chip.debug_bulk_ticks_last()
    assert chip.last_l() == 0                                    # the ctx's own loop state is not the call's
    got = [bytes(r) for r in recs]
    assert got == want, [(ls[t], recs[t].as_dict(), capi.TickResult.from_buffer_copy(want[t]).as_dict()) for t in range(len(ls)) if got[t] != want[t]][:3]
    assert last == want_last
    oracle = oracle_lib.LoopOracle(db, orc_params(p)) if db is not None else None
    for t, l in enumerate(ls):
        if oracle is not None:
            assert recs[t].as_dict() == oracle.tick(l), (l, recs[t].as_dict())
        if recs[t].status != SCANNED:
            assert (sc[t] == -np.inf).all() and (ix[t] == -1).all(), l
        elif lists:
            ws, wi = chip.query_rows(l - p.lag, [l - 1, l - 2, l - 3], topk)
            assert (ix[t] == wi).all() and (bits(sc[t]) == bits(ws)).all(), (l, ix[t], wi)
            assert recs[t].argmax[:] == list(ix[t, :, 0]) and bits(list(recs[t].maxv)).tolist() == bits(sc[t, :, 0]).tolist()
    n_scan = sum(r.status == SCANNED for r in recs)
    assert dbg["certified"] + dbg["uncertified"] == n_scan or dbg["groups"] == 0
    assert dbg["exact_reruns"] == (dbg["uncertified"] if dbg["groups"] else n_scan)
    assert dbg["waits"] == dbg["groups"] and dbg["launches"] == 4 * dbg["groups"]
    return recs, sc, ix, dbg


# ---------------------------------------------------------------------------------------------------------------- the schedule
D_S, N_S = 64, 700
PLANT_DST = range(396, 405)          # rows 396 .. 404: near-copies of ...


def schedule_db(src0):
    """700 unit rows; rows 396 .. 404 are near-copies (cosine about 0.96) of rows src0 .. src0 + 8 -- inside one locality window, so the
    ticks at l = 399, 402, 405 find a loop -- and rows 500 .. 502 near-copies of rows 50, 200 and 300: above the threshold, not local"""
    rng = np.random.default_rng(20)
    db = unit_rows(rng, N_S, D_S)
    noise = unit_rows(rng, 12, D_S)
    pairs = [(d, src0 + i) for i, d in enumerate(PLANT_DST)] + [(500, 50), (501, 200), (502, 300)]
    for j, (dst, src) in enumerate(pairs):
        v = db[src].astype(np.float64) + 0.3 * noise[j]
        db[dst] = (v / np.linalg.norm(v)).astype(np.float32)
    return db


@functools.lru_cache(maxsize=None)
def schedule(src0=96):
    db = schedule_db(src0)
    db.setflags(write=False)
    return db


def norm_bound_of(chip):
    return chip.info()["row_norm_max"]


@pytest.mark.parametrize("topk", [1, 5, 8])
def test_whole_schedule(topk):
    db, ls = schedule(), list(range(3, N_S + 1))
    with capi.Chip(D_S) as chip:
        chip.append_f32(db)
        recs, sc, ix, dbg = check_bulk(chip, ls, topk, db=db)
        st = [r.status for r in recs]
        assert {capi.CHIP_TICK_SKIPPED, capi.CHIP_TICK_TOO_SHORT, SCANNED} == set(st)
        found = {ls[t] for t, r in enumerate(recs) if r.found}
        assert {399, 402, 405} <= found and len(found) < st.count(SCANNED) / 2
        assert recs[ls.index(501)].maxv[0] > 0.85 and recs[ls.index(501)].argmax[0] == 50 and not recs[ls.index(501)].found   # above the threshold, not local
        # the certificate, against the CPU mirror on the same inputs: the same ticks certify (for this seed: all of them)
        E = nm.error_bound(D_S, norm_bound_of(chip))
        assert dbg["E"] == E and dbg["list_len"] in (8, 16)
        mirror = [nm.tick(db, l, l - 50, dbg["list_len"], topk, E) for t, l in enumerate(ls) if st[t] == SCANNED]
        unc = sum(not m["certified"] for m in mirror)
        assert unc == 0 and dbg["uncertified"] == unc and dbg["certified"] == len(mirror) and dbg["exact_reruns"] == 0
        assert dbg["rescored_rows"] == sum(m["rescored"] for m in mirror) and dbg["groups"] == 1


def test_a_moved_plant_changes_the_records():
    ls = [399, 402, 405]
    out = []
    for src0 in (96, 196):
        db = schedule(src0)
        with capi.Chip(D_S) as chip:
            chip.append_f32(db)
            recs, _, _, _ = check_bulk(chip, ls, 1, params(min_new=-1000), db=db)
            out.append(recs)
    for a, b in zip(*out):
        assert a.found == 1 and b.found == 1 and abs(a.idx_prev - b.idx_prev) == 100 and bytes(a) != bytes(b)


@pytest.mark.parametrize("k", [6, 7, 15, 16, 17])
def test_short_prefixes(k):
    db, p = schedule(), params(lag=10)
    with capi.Chip(D_S) as chip:
        chip.append_f32(db)
        recs, sc, ix, dbg = check_bulk(chip, [k + 10], 8, p, db=db)
        assert recs[0].status == SCANNED and (ix[0] >= 0).sum(axis=1).tolist() == [min(k, 8)] * 3
        if k < dbg["list_len"]:
            assert (dbg["certified"], dbg["uncertified"]) == (1, 0)       # the last slot of every list is unused: nothing dropped
        if k < 8:
            assert dbg["rescored_rows"] == 3 * k                           # fewer rows than topk: G = -inf, every row is a candidate
    assert (ix[0, :, min(k, 8):] == -1).all() and (sc[0, :, min(k, 8):] == -np.inf).all()


def test_runs_of_identical_rows_rerun_the_ticks_they_leave_uncertified():
    """thirty identical rows (a platform standing still): more than KL rows tie at the top of the queries close to them, those ticks do
    not certify and run again exactly -- the same ticks as in the CPU mirror, and every record still the loop's"""
    rng = np.random.default_rng(5)
    db = unit_rows(rng, 400, D_S)
    db[100:130] = db[100]
    db[298:301] = db[100]
    ls = [170, 200, 250, 301, 304, 400]
    with capi.Chip(D_S) as chip:
        chip.append_f32(db)
        recs, sc, ix, dbg = check_bulk(chip, ls, 8, params(min_new=-1000), db=db)
        E = nm.error_bound(D_S, norm_bound_of(chip))
        mirror = [nm.tick(db, l, l - 50, dbg["list_len"], 8, E) for l in ls]
        unc = sum(not m["certified"] for m in mirror)
        assert 1 <= unc < len(ls) and (dbg["uncertified"], dbg["exact_reruns"], dbg["certified"]) == (unc, unc, len(ls) - unc)
        assert recs[ls.index(301)].argmax[:] == [129] * 3             # the highest index of the tie


# ---------------------------------------------------------------------------------------------------------------- tiles and groups
D_T, N_T = 32, 4300


@functools.lru_cache(maxsize=None)
def tile_db():
    db = unit_rows(np.random.default_rng(32), N_T, D_T)
    db.setflags(write=False)
    return db


@pytest.mark.parametrize("wgs", [0, 2])
def test_two_groups_and_both_tiles(wgs, monkeypatch):
    if wgs:
        monkeypatch.setenv("CHIP_BATCH_WGS", str(wgs))       # a workgroup walks many claimed tiles
    else:
        monkeypatch.delenv("CHIP_BATCH_WGS", raising=False)
    db = tile_db()
    ls = [56 + 3 * i for i in range(1405)]
    plan = capi.bulk_ticks_plan(ls, N_T)
    assert (plan["groups"], plan["tile_full"], plan["tile_last"], plan["ticks_scanned"]) == (2, 256, 128, 1405)
    with capi.Chip(D_T) as chip:
        chip.append_f32(db)
        recs, sc, ix, dbg = check_bulk(chip, ls, 5, db=db if not wgs else None)
        assert dbg["groups"] == 2 and all(r.status == SCANNED for r in recs)
        # (every tick is compared above; these are the ones at the edges: ticks 84 .. 86 hold queries 252 .. 260 -- tick 85 straddles the
        # first 256-query tile boundary -- and ticks 1364 / 1365 are the last of the full group and the first of the last)
        for t in (84, 85, 86, 1364, 1365, 1404):
            assert recs[t].argmax[0] >= 0 and recs[t].idx_curr in (-1, ls[t] - 1)
        short = ls[500:600]                                   # 300 queries: three 128-query tiles, ticks 42 and 85 straddle their boundaries
        assert capi.bulk_ticks_plan(short, N_T, params(min_new=-10 ** 6))["tile_last"] == 128
        check_bulk(chip, short, 8, params(min_new=-10 ** 6))


# ---------------------------------------------------------------------------------------------------------------- both sides of the certificate
D_C = 64
P_C = dict(lag=3, min_new=-10 ** 6, min_k=0)                 # the tick at l = n + 3 sees the prefix [0, n); its queries are rows n .. n + 2


def crafted_chip(n, fill):
    """rows x e_0 (background x = -1, row 0 appended first: it fixes the norm bound and with it E), then three rows e_0: the queries of the
    tick at l = n + 3.  fill(x, E, KL) places the scores."""
    x = np.full(n, -1.0, np.float32)
    chip = capi.Chip(D_C)
    row0 = np.zeros((1, D_C), np.float32)
    row0[0, 0] = -1.0
    chip.append_f32(row0)
    norm = norm_bound_of(chip)
    E = nm.error_bound(D_C, norm)
    KL = capi_list_len(chip)
    fill(x, E, KL)
    assert x[0] == -1.0 and np.abs(x).max() == 1.0
    db = np.zeros((n + 3, D_C), np.float32)
    db[:n, 0] = x
    db[n:, 0] = 1.0
    chip.append_f32(db[1:])
    assert norm_bound_of(chip) == norm
    return chip, db, E, KL


def capi_list_len(chip):
    """KL of this build (the read-back says it before any call as well)"""
    return chip.debug_bulk_ticks_last()["list_len"]


TOP_ROWS = [3, 17, 18, 40, 41, 42, 77, 90, 91, 120, 133, 150, 151, 180, 190, 199]


@pytest.mark.parametrize("n_equal", ["KL-1", "KL", "KL+1"])
def test_equal_rows_at_the_top(n_equal):
    m = {}

    def fill(x, E, KL):
        top = (TOP_ROWS + [201, 202])[16 - KL:][:KL + {"KL-1": -1, "KL": 0, "KL+1": 1}[n_equal]]
        x[top] = 0.5
        m.update(top=top)

    chip, db, E, KL = crafted_chip(260, fill)
    with chip:
        recs, sc, ix, dbg = check_bulk(chip, [263], 1, params(**P_C), db=db)
        assert dbg["E"] == E and recs[0].argmax[:] == [max(m["top"])] * 3 and recs[0].maxv[0] == 0.5      # the highest index wins the tie
        if n_equal == "KL-1":
            assert (dbg["certified"], dbg["uncertified"], dbg["exact_reruns"], dbg["rescored_rows"]) == (1, 0, 0, 3 * (KL - 1))
        else:
            assert (dbg["certified"], dbg["uncertified"], dbg["exact_reruns"], dbg["rescored_rows"]) == (0, 1, 1, 3 * KL)
        want = nm.tick(db, 263, 260, KL, 1, E)
        assert want["certified"] == (n_equal == "KL-1") and want["record"] == recs[0].as_dict()


@pytest.mark.parametrize("side", ["below", "at"])
def test_the_last_entry_one_float_either_side_of_the_threshold(side):
    G = np.float32(0.9)
    m = {}

    def fill(x, E, KL):
        thr = nm.threshold(G, E)
        f = np.float32(thr)
        below, at = (np.nextafter(f, np.float32(-1)), f) if np.float64(f) >= thr else (f, np.nextafter(f, np.float32(1)))
        assert np.float64(below) < thr <= np.float64(at) and np.nextafter(below, np.float32(1)) == at and at < G
        x[50] = G
        x[10:10 + KL - 1] = below if side == "below" else at
        m.update(v=float(below if side == "below" else at), thr=thr)

    chip, db, E, KL = crafted_chip(100, fill)
    with chip:
        recs, sc, ix, dbg = check_bulk(chip, [103], 1, params(**P_C), db=db)
        assert dbg["E"] == E and recs[0].argmax[:] == [50] * 3 and recs[0].found == 1
        want = (1, 0, 0, 3) if side == "below" else (0, 1, 1, 3 * KL)
        assert (dbg["certified"], dbg["uncertified"], dbg["exact_reruns"], dbg["rescored_rows"]) == want, (m, dbg)


def test_fp32_misordering_is_repaired_by_the_exact_scores():
    db = misordered_db()
    with capi.Chip(db.shape[1]) as chip:
        chip.append_f32(db)
        recs, sc, ix, dbg = check_bulk(chip, [63], 2, db=db)
        fs, fi = chip.query_batch(13, db[[62]], 2)
        assert fi[0].tolist() == [9, 5]                           # the GEMM's own order: b first
        assert recs[0].argmax[:] == [5] * 3 and ix[0, 0].tolist() == [5, 9] and recs[0].maxv[0] == 1.0 + 3 * 2.0 ** -24
        assert (dbg["certified"], dbg["uncertified"]) == (1, 0) and dbg["rescored_rows"] >= 2


# ---------------------------------------------------------------------------------------------------------------- segment boundary
def test_ticks_across_a_segment_boundary():
    D, seg = 8224, 8192
    n = seg + 300
    db = relja_like(4242, n, D).astype(np.float32)
    p = params(lag=3, min_new=1, min_k=0)
    ls = list(range(seg - 7, seg + 14))                           # 21 ticks: query rows and prefix ends on both sides of row 8192
    db[seg - 1] = db[seg + 2]                                     # the best row of the ticks that ask with row 8194 is 8191 ...
    db[seg] = db[seg + 5]                                         # ... and of those that ask with row 8197 it is 8192
    with capi.Chip(D) as chip:
        chip.append_f32(db)
        info = chip.info()
        assert info["rows_local"] == n and info["capacity_local"] == 2 * seg, info       # two segments
        recs, sc, ix, dbg = check_bulk(chip, ls, 5, p)
        assert dbg["groups"] == 1 and all(r.status == SCANNED for r in recs)
        by_l = {l: r for l, r in zip(ls, recs)}
        assert by_l[seg + 3].argmax[0] == seg - 1 and by_l[seg + 6].argmax[0] == seg      # query rows 8194 and 8197 themselves
        assert by_l[seg + 4].argmax[1] == seg - 1 and by_l[seg + 8].argmax[2] == seg


# ---------------------------------------------------------------------------------------------------------------- purity
def test_a_bulk_call_between_parked_ticks_changes_nothing(monkeypatch):
    D, rows, L0 = 4096, 24_000, 20_000
    monkeypatch.setenv("CHIP_SCAN_OVERLAP_GIB", "0")
    monkeypatch.setenv("CHIP_TICK_COALESCE", "3")
    ls = [L0, L0 + 3, L0 + 6, L0 + 7, L0 + 9]
    p = capi.default_dot_params()
    runs = []
    with capi.Chip(D, capacity_hint=rows + 64) as chip:
        chip.append_synthetic(rows, 771177, [(L0 - 50 + 1, 12_345, 2)])
        chip.coalesce_force(True)
        for with_bulk in (False, True):
            chip.loop_reset()
            for i, l in enumerate(ls[:2]):
                chip.loop_tick_enqueue(l, i, p)               # both park
            if with_bulk:
                bulk = chip.loop_ticks_bulk([L0 + 100, L0 + 101, L0 + 103], p, 5, 3)
                assert [r.status for r in bulk[0]] == [SCANNED, capi.CHIP_TICK_SKIPPED, SCANNED] and bulk[3] == L0 + 103
                assert chip.last_l() == ls[1]
            for i, l in enumerate(ls[2:], start=2):
                chip.loop_tick_enqueue(l, i, p)
            runs.append(([bytes(chip.loop_tick_collect(i)) for i in range(len(ls))], chip.last_l()))
        chip.coalesce_force(False)
        assert runs[0] == runs[1] and runs[0][1] == ls[-1]
        assert [capi.TickResult.from_buffer_copy(b).status for b in runs[0][0]] == [SCANNED, SCANNED, SCANNED, capi.CHIP_TICK_SKIPPED, SCANNED]
        chip.loop_reset()
        check_bulk(chip, ls, 1, p, lists=False)


# ---------------------------------------------------------------------------------------------------------------- status table
def raw_call(chip, ls, topk, T=None, null=()):
    """the C call with out / scores / idx / last_l_out prefilled: (status, untouched)"""
    ls = np.ascontiguousarray(ls, np.int64)
    T = len(ls) if T is None else T
    n = max(len(ls), 1)
    out = np.full(n * C.sizeof(capi.TickResult), 0x5A, np.uint8)
    k = max(topk, 1)
    sc, ix, last = np.full(n * 3 * k, 7.0), np.full(n * 3 * k, 7, np.int64), C.c_int64(77)
    args = [chip.h, ls.ctypes.data, T, None, 0, topk, out.ctypes.data, sc.ctypes.data, ix.ctypes.data, C.byref(last)]
    for i in null:
        args[i] = None
    rc = chip.lib.chip_loop_ticks_bulk(*args)
    return rc, bool((out == 0x5A).all() and (sc == 7.0).all() and (ix == 7).all() and last.value == 77)


def test_status_table():
    db = schedule()
    with capi.Chip(D_S) as chip:
        chip.append_f32(db)
        assert raw_call(chip, [60, 63], 1)[0] == capi.CHIP_OK
        for kw in (dict(T=0), dict(T=-1), dict(null=(1,)), dict(null=(6,)), dict(null=(0,))):
            assert raw_call(chip, [60, 63], 1, **kw) == (capi.CHIP_ERR_INVALID_ARG, True), kw
        for topk in (0, 9, 16):
            assert raw_call(chip, [60, 63], topk) == (capi.CHIP_ERR_UNSUPPORTED, True), topk
        for ls in ([60, N_S + 1], [60, -1], [63, 1000]):
            assert raw_call(chip, ls, 1) == (capi.CHIP_ERR_RANGE, True), ls
        assert raw_call(chip, [60, N_S], 8)[0] == capi.CHIP_OK
        assert raw_call(chip, [60], 1, null=(7, 8, 9))[0] == capi.CHIP_OK       # lists and last_l_out are optional
    with capi.Chip(48) as chip:                                   # D % 32 != 0
        chip.append_f32(np.ones((80, 48), np.float32))
        assert raw_call(chip, [60, 63], 1) == (capi.CHIP_ERR_UNSUPPORTED, True)
    with capi.Chip(D_S, storage="f64") as chip:                   # double rows
        chip.append_f64(db.astype(np.float64))
        assert raw_call(chip, [60, 63], 1) == (capi.CHIP_ERR_UNSUPPORTED, True)
    with capi.Chip(D_S, devices=[0, 0]) as chip:                  # a chip_create_multi ctx (two sub-contexts on one device)
        chip.append_f32(db)
        assert raw_call(chip, [60, 63], 1) == (capi.CHIP_ERR_UNSUPPORTED, True)
        assert chip.loop_tick(60).status == SCANNED                # (the ctx itself works)
    with capi.Chip(D_S, shard_rank=0, shard_count=2) as chip:     # a shard (refused before its rows are looked at)
        assert raw_call(chip, [60, 63], 1) == (capi.CHIP_ERR_UNSUPPORTED, True)


def test_rows_beyond_the_norm_bound_take_the_exact_path():
    db = schedule().copy()
    db[5] *= np.float32(2.0 ** 61)                                # norm^2 = 2^122 > 2^120: an fp32 partial sum may overflow
    with capi.Chip(D_S) as chip:
        chip.append_f32(db)
        assert norm_bound_of(chip) ** 2 > 2.0 ** 120
        recs, sc, ix, dbg = check_bulk(chip, [60, 63], 8, db=db)
        assert (dbg["groups"], dbg["certified"], dbg["uncertified"], dbg["exact_reruns"], dbg["E"]) == (0, 0, 0, 2, 0.0)
        assert all(r.status == SCANNED for r in recs)
