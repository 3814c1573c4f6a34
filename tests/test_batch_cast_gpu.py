"""Many-query mode on DOUBLE-row DBs (chip_query_batch_cast_f32, Chip.query_batch(..., cast_rows=True)): every row element enters
the fp32 GEMM as (float)x -- what the reference's faiss variants do with their MatrixXd DB (X.cast<float>(), src/Cerebro.cpp:422,569,
807) -- and then the semantics of chip_query_batch_f32 apply.  Definition: oracle_lib.scan_topk_fmaf(db.astype(np.float32), k, q, K);
bar: indices equal and fp32 score bits equal.  Data: float64 descriptors none of whose elements is float32-representable."""
import functools
import os
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import scenarios
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def relja_like(seed, N, D, plants=()):
    """float64 descriptors that are NOT float32-representable: unit-norm rows of a float64 matmul, like
    np.matmul(u, WPCA_M) + WPCA_b followed by /= norm (server.py:148-149).  Planted rows are noisy copies / duplicates."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((64, D))
    db = rng.standard_normal((N, 64)) @ W + 0.01 * rng.standard_normal(D)
    for dst, src, kind in sorted(plants):
        db[dst] = db[src] if kind == 2 else db[src] + 0.2 * np.linalg.norm(db[src]) / np.sqrt(D) * rng.standard_normal(D)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    assert not np.array_equal(db.astype(np.float32).astype(np.float64), db)
    return db


def f32bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Want:
    """The oracle's top-16 lists of one (db32, q), one scan per prefix k; the top-K list of a total order is their first K entries."""

    def __init__(self, db32, q):
        self.db32, self.q, self.memo = db32, q, {}

    def __call__(self, k, K):
        if k not in self.memo:
            self.memo[k] = oracle_lib.scan_topk_fmaf(self.db32, k, self.q, 16)
        s, i = self.memo[k]
        return s[:, :K], i[:, :K]


def check(chip, want, k, K, q=None):
    ws, wi = want(k, K)
    gs, gi = chip.query_batch(k, want.q if q is None else q, K, cast_rows=True)
    assert np.array_equal(gi, wi), (k, K, gi[:2], wi[:2])
    assert np.array_equal(f32bits(gs), f32bits(ws)), (k, K)                 # bit-exact fp32 scores


def queries_of(db, Q, seed):
    """float casts of DB rows plus two foreign rows"""
    rng = np.random.default_rng(seed)
    D = db.shape[1]
    return np.concatenate([db[rng.choice(db.shape[0], Q - 2, replace=False)], relja_like(seed + 1, 2, D)]).astype(np.float32)


# Q is padded to 128s; a multiple of 256 takes the 256 x 256 / 8-wave tile (K <= 8 on double rows), anything else the 128 x 128 one
@pytest.mark.parametrize("D,N,Q", [(32, 300, 5), (512, 1500, 64), (1024, 3000, 200), (4096, 1200, 130), (256, 2600, 300), (64, 1500, 512)])
def test_cast_parity_on_double_rows(D, N, Q):
    plants, loops, ties = scenarios.loop_plants(N, 4, seed=D + Q)
    db = relja_like(7 * D, N, D, plants)
    db32 = db.astype(np.float32)
    q = queries_of(db, Q, Q)
    lq = loops[0][1]
    q[0] = db32[lq]                                      # the planted revisit
    want = Want(db32, q)
    with capi.Chip(D, storage="f64") as chip:
        chip.append_f64(db)
        assert chip.info()["storage_bytes"] == 8
        for K in (1, 8, 16):
            for k in (0, 1, 127, 128, 129, 255, 256, 257, N - 50, N):
                check(chip, want, k, K)
        # an exact-duplicate plant stays a duplicate under the cast: three equal scores, index-descending
        s, t1, t2 = ties[0]
        sc, ix = chip.query_batch(N, db32[[s]], 3, cast_rows=True)
        assert list(ix[0]) == [t2, t1, s] and sc[0][0] == sc[0][1] == sc[0][2]
        # sanity against the fp64 scan of the same double rows: same best match, scores within fp32 round-off
        s64, i64 = chip.query_vectors_f64(N - 50, db[[lq]], 1)
        s32, i32 = chip.query_batch(N - 50, db32[[lq]], 1, cast_rows=True)
        assert i32[0, 0] == i64[0, 0] and abs(float(s32[0, 0]) - s64[0, 0]) < 1e-5
        # the old entry keeps refusing double rows: the lossy cast is opt-in
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N, q, 4)
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N + 1, q, 4, cast_rows=True)
        assert e.value.status == capi.CHIP_ERR_RANGE


@functools.lru_cache(maxsize=None)
def _claimed(Q):
    D, N = 128, 5000
    db = relja_like(11, N, D)
    q = db[np.random.default_rng(Q).choice(N, Q, replace=False)].astype(np.float32)
    return db, Want(db.astype(np.float32), q)


# 5000 rows = 20 tiles of 256 / 40 tiles of 128; the capped grid makes every workgroup walk many claimed tiles, and the last, partial
# round is cut into query halves where that fills the grid better ((256, 8): 16 whole tiles + 4 x 2 halves; (100, 16): 32 + 8 x 2)
@pytest.mark.parametrize("Q,wgs", [(256, 1), (256, 3), (256, 8), (256, 19), (100, 2), (100, 16)])
def test_cast_claimed_tiles(Q, wgs, monkeypatch):
    db, want = _claimed(Q)
    N = db.shape[0]
    monkeypatch.setenv("CHIP_BATCH_WGS", str(wgs))
    with capi.Chip(db.shape[1], storage="f64") as chip:
        chip.append_f64(db)
        for k in (N, N - 257, 4097, 1023):
            check(chip, want, k, 8)


def test_cast_entry_on_a_float_row_ctx_is_the_float_call():
    D, N, Q = 512, 1500, 64
    db = scenarios.build_db(7 * D, N, D, [])
    q = db[np.random.default_rng(Q).choice(N, Q, replace=False)]
    with capi.Chip(D) as chip:
        chip.append_f32(db)
        for K, k in ((8, N), (16, N - 50), (1, 129)):
            a, b = chip.query_batch(k, q, K), chip.query_batch(k, q, K, cast_rows=True)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_cast_mixed_appends():
    """append_f64 and append_f32 rows in one double DB (float rows widen exactly), as test_f64_tick_sequence_and_auto_switch does for ticks"""
    D, N, Q = 1024, 1500, 200
    db = relja_like(7, N, D)
    dbm = db.copy()
    dbm[700:760] = db[700:760].astype(np.float32)
    want = Want(dbm.astype(np.float32), queries_of(dbm, Q, 5))
    with capi.Chip(D) as chip:
        chip.append_f64(db[:1])                                  # the first genuinely-double row switches the empty DB to double rows
        chip.append_f64(db[1:700])
        chip.append_f32(db[700:760].astype(np.float32))
        chip.append_f64(db[760:])
        assert chip.info()["storage_bytes"] == 8 and chip.info()["lossy_rows"] == 0
        for K, k in ((8, N), (16, N), (8, 730), (1, 701)):
            check(chip, want, k, K)


@pytest.mark.parametrize("G,D,N,Q", [(3, 128, 4100, 70), (2, 4096, 1500, 130)])
def test_cast_on_a_group_ctx(G, D, N, Q):
    plants, loops, ties = scenarios.loop_plants(N, 4, seed=G + Q)
    db = relja_like(3 * D + G, N, D, plants)
    want = Want(db.astype(np.float32), queries_of(db, Q, G * Q))
    with capi.Chip(D, devices=[0] * G, storage="f64") as chip:
        chip.append_f64(db[:N // 2])
        chip.append_f64(db[N // 2:])
        for K in (1, 8, 16):
            for k in (0, 1, G - 1, G, G + 1, 257, N - 50, N):
                check(chip, want, k, K)
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N + 1, want.q, 4, cast_rows=True)
        assert e.value.status == capi.CHIP_ERR_RANGE
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N, want.q, 4)
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
        # the tick path of the same group still works between batch calls (shared scan streams / query buffers)
        orc = oracle_lib.LoopOracle64(db)
        for l in scenarios.default_schedule(N)[-6:]:
            chip.loop_reset()
            orc.state.last_l = 0
            g_, o_ = chip.loop_tick(l).as_dict(), orc.tick(l)
            assert (g_["found"], g_["argmax"]) == (o_["found"], o_["argmax"])
        check(chip, want, N, 8)


def test_cast_on_a_sharded_ctx_with_the_in_library_exchange():
    """world size 1 (RCCL refuses two ranks on one device): local pass -> agreement -> ncclAllGather of the lists -> merge"""
    D, N, Q = 256, 2100, 140
    db = relja_like(17, N, D)
    want = Want(db.astype(np.float32), queries_of(db, Q, 3))
    with capi.Chip(D, storage="f64") as chip:
        chip.comm_init_rank(capi.comm_unique_id(), 1, 0)
        assert chip.info()["exchange"] == capi.CHIP_EXCHANGE_RCCL
        chip.append_f64(db)
        for K in (1, 8):
            for k in (0, 129, N):
                check(chip, want, k, K)
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N + 5, want.q, 8, cast_rows=True)      # beyond what this rank has published: the failure mark, not a hang
        assert e.value.status == capi.CHIP_ERR_SHARD_FAILED
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N, want.q, 8)
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
        check(chip, want, N, 8)                                      # and the communicator is still in step


def test_cast_sharded_without_exchange_lists_are_consistent():
    D, N, Q, G = 256, 1100, 70, 3
    db = relja_like(5, N, D)
    q = db[:Q].astype(np.float32)
    want_s, want_i = oracle_lib.scan_topk_fmaf(db.astype(np.float32), N, q, 8)
    parts = []
    for r in range(G):
        with capi.Chip(D, shard_rank=r, shard_count=G, storage="f64") as chip:
            chip.append_f64(db)
            parts.append(chip.query_batch(N, q, 8, cast_rows=True))
    for qi in range(Q):
        cand = sorted(((float(s), int(i)) for ps, pi in parts for s, i in zip(ps[qi], pi[qi]) if i >= 0), key=lambda t: (-t[0], -t[1]))[:8]
        assert [c[1] for c in cand] == list(want_i[qi])
        assert np.array_equal(f32bits([c[0] for c in cand]), f32bits(want_s[qi]))


def test_cast_error_surface():
    with capi.Chip(36, storage="f64") as chip:                    # D % 32 != 0
        chip.append_f64(np.full((4, 36), 0.1))
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(4, np.zeros((2, 36), dtype=np.float32), 4, cast_rows=True)
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
    with capi.Chip(64, storage="f64") as chip:
        chip.append_f64(np.full((4, 64), 0.1))
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(4, np.zeros((2, 64), dtype=np.float32), 4)
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED         # the old entry on double rows
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(4, np.zeros((2, 64), dtype=np.float32), capi.CHIP_MAX_TOPK + 1, cast_rows=True)
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED


def _worker(rank, world, uid_path, ret):
    """one rank of a 2-rank exchange on device 0 over the RCCL stand-in: double rows, the cast entry, every rank checks every result"""
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    D, N = 512, 1500
    db = relja_like(733, N, D)
    db32 = db.astype(np.float32)
    with capi.Chip(D, device=0, shard_rank=rank, shard_count=world, storage="f64") as chip:
        if rank == 0:
            with open(uid_path + ".tmp", "wb") as f:
                f.write(capi.comm_unique_id())
            os.replace(uid_path + ".tmp", uid_path)
        t0 = time.time()
        while not os.path.exists(uid_path):
            assert time.time() - t0 < 120
            time.sleep(0.01)
        chip.comm_init_rank(open(uid_path, "rb").read(), world, rank)
        assert chip.info()["comm_ranks"] == world
        chip.append_f64(db[:700])
        chip.append_f32(db32[700:710])                               # float rows widen exactly
        chip.append_f64(db[710:])
        dbm = db32.copy()
        assert chip.info()["storage_bytes"] == 8 and chip.info()["rows_local"] == len(range(rank, N, world))
        for Q, K in ((70, 8), (130, 16), (256, 8)):
            q = dbm[(np.arange(Q) * 13) % N]
            sc, ix = chip.query_batch(N - 50, q, K, cast_rows=True)
            wsc, wix = oracle_lib.scan_topk_fmaf(dbm, N - 50, q, K)
            assert np.array_equal(ix, wix) and np.array_equal(f32bits(sc), f32bits(wsc)), (rank, Q, K)
        with pytest.raises(capi.ChipError) as e:
            chip.query_batch(N - 50, dbm[:4], 8)                      # the old entry refuses on every rank, before anything collective
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
        got, want = chip.query_vectors_f64(777, db[[11, 400]], 5), oracle_lib.scan_topk_f64(np.concatenate([db[:700], db32[700:710], db[710:]]), 777, db[[11, 400]], 5)
        assert np.array_equal(got[1], want[1])                        # the exchange is still in step
        ret[rank] = 1


def test_cast_over_the_rccl_stand_in_two_ranks(tmp_path):
    from test_fakerccl_gpu import BASE_ENV, _spawn
    ret = _spawn(_worker, 2, tmp_path, (), dict(BASE_ENV))
    assert len(ret) == 2 and set(ret.values()) == {1}
