"""GPU parity of EVERY kernel form the scan dispatcher can choose (tests/scan_form_cases.py), at prefixes where a wave owns several
rows, with proof of which form ran.  Per case: the knobs are set before the ctx exists, the DB is sized against the launch geometry
(W waves, R rows per wave and pass: two full passes and a ragged third), exact duplicates of one row sit in neighbouring waves,
neighbouring workgroups, the same wave in one pass / in consecutive passes, row 0 and the last row; every prefix class is scanned and
indices AND fp64 score bits are compared with a plain host selection over the oracle's score vectors; chip.last_scan() must name the
form the case row names and equal capi.scan_plan for the same arguments -- a case that silently ran another kernel fails."""
import functools
import os

import numpy as np
import pytest

import oracle_lib
import scan_form_cases as sfc
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
SEED = 40_917
THREADS = min(os.cpu_count() or 1, 32)
KS_ALL = (1, 5, 16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=2)
def base_f32(D, N):
    return oracle_lib.synth_rows(SEED, range(N), D)


def host_db(case, N, dups, src):
    """the DB on the host: float rows of the integer-domain generator (the device generates the same rows itself), or genuinely double
    rows (unit-norm rows of a float64 matmul: not float32-representable); rows `dups` are bit-identical copies of row `src`"""
    if case.elem == 4:
        db = base_f32(case.D, N).copy()
    else:
        rng = np.random.default_rng(SEED + case.D)
        db = rng.standard_normal((N, 48)) @ rng.standard_normal((48, case.D)) + 0.01 * rng.standard_normal(case.D)
        db /= np.linalg.norm(db, axis=1, keepdims=True)
        assert not np.array_equal(db.astype(np.float32).astype(np.float64), db)
    db[dups] = db[src]
    return db


def select(u, k, K):
    """top K of u[:k] by (score descending, index descending): a plain selection that shares nothing with the device's list structures"""
    sc, ix = np.full(K, -np.inf), np.full(K, -1, dtype=np.int64)
    if k > 0:
        s = u[:k]
        kk = min(K, k)
        cand = np.nonzero(s >= np.partition(s, k - kk)[k - kk])[0] if k > 4 * K else np.arange(k)
        top = cand[np.lexsort((-cand, -s[cand]))][:kk]
        sc[:kk], ix[:kk] = s[top], top
    return sc, ix


def same_tick(g, o):
    for key in ("status", "found", "idx_curr", "idx_prev", "argmax"):
        assert g[key] == o[key], (key, g, o)
    assert float(g["score"]).hex() == float(o["score"]).hex()
    assert [float(x).hex() for x in g["maxv"]] == [float(x).hex() for x in o["maxv"]]


def every_tick_params():
    p = capi.default_dot_params()
    p.min_new = -(1 << 30)          # every tick runs, whatever the previous l was
    return p


def oracle_tick(db, l):
    p = oracle_lib.default_params()
    p.min_new = -(1 << 30)
    return (oracle_lib.LoopOracle64 if db.dtype == np.float64 else oracle_lib.LoopOracle)(db, p).tick(l)


def check_launch(chip, case, n_cus, nq, K, k, call, top, launches):
    """the record of the launch just made: it IS a new launch, over k rows, equal to the plan for the same arguments; at the case's
    largest prefix (`top`) it is the form -- and, with three queries, the grid and block -- the case row names"""
    ls = chip.last_scan()
    assert ls["launches"] == launches and ls["n_rows"] == k and ls["nq"] == nq, (ls, launches, k)
    pl = capi.scan_plan(case.D, case.elem, nq, K, k, sfc.CALL_CODE[call], n_cus)
    assert {f: v for f, v in ls.items() if f != "launches"} == {f: v for f, v in pl.items() if f != "launches"}, (ls, pl)
    if top:
        want = case.form_for(nq)
        assert {f: ls[f] for f in sfc.FORM_FIELDS} == want, (case.name, nq, ls, want)
        if nq == 3:
            assert (ls["grid"], ls["block"]) == (case.grid, case.block), ls
    return ls


@pytest.mark.parametrize("case", sfc.CASES, ids=repr)
def test_scan_form(monkeypatch, case):
    for k in sfc.SCAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    with capi.Chip(case.D, storage="f64" if case.elem == 8 else "f32") as chip:
        n_cus = chip.info()["n_cus"]
        N, W, R, wpb = sfc.case_geometry(case, lambda *a: capi.scan_plan(*a, n_cus))
        tick_kind = case.call != sfc.QUERY
        ks = sfc.prefixes(W, R, wpb, N)
        tick_ks = [k for k in ks if 6 <= k <= N - 50]
        # the duplicates: row r (first pass, not a workgroup's first wave) and its copies in the next wave, the next workgroup, the same
        # wave one row on (the same pass when R >= 2, else the next pass), the same wave one pass on, row 0 and the last row;
        # a tick's newest query row (l - 1) is a copy too, so that every tick sees the tie
        r = W // 3 + 3
        dups = {0, r + 1, r + wpb, r + W, r + R * W, N - 1}
        if tick_kind:
            dups |= {k + 49 for k in tick_ks}
        dups = sorted(dups - {r})
        db = host_db(case, N, dups, r)
        if case.elem == 4:
            plants = [(d, r, 2) for d in dups]
            chip.append_synthetic(N, SEED, plants)
        else:
            chip.append_f64(db)
        assert chip.size() == N and chip.last_scan()["family"] == "none"
        copies = sorted(dups + [r])
        launches = 0

        if not tick_kind:
            qrows = [N - 1, N - 2, r + 1, 5]                  # two copies of row r, two plain rows
            u = [oracle_lib.scores(db, N, db[q], nthreads=THREADS) for q in qrows]
            for nq in case.nqs():
                for K in KS_ALL:
                    # every prefix class for three queries and 16 entries; the other (nq, K) take every other prefix, alternating
                    sub = ks if (nq, K) == (3, 16) else ks[(nq + K) % 2::2] + [N]
                    for k in sub:
                        sc, ix = chip.query_rows(k, qrows[:nq], K)
                        launches += 1
                        want = [select(u[i], k, K) for i in range(nq)]
                        assert np.array_equal(ix, np.array([w[1] for w in want])), (nq, K, k, ix, want)
                        assert np.array_equal(bits(sc), bits(np.array([w[0] for w in want]))), (nq, K, k, sc, want)
                        check_launch(chip, case, n_cus, nq, K, k, sfc.QUERY, k == N, launches)
                # the planted copies come back index-descending with bit-equal scores
                sc, ix = chip.query_rows(N, qrows[:nq], 16)
                launches += 1
                assert list(ix[0][:len(copies)]) == copies[::-1] and len(set(bits(sc[0][:len(copies)]).tolist())) == 1
            # external query vectors take the same kernels
            sc, ix = (chip.query_vectors_f64 if case.elem == 8 else chip.query_vectors)(N - 7, db[qrows[:3]], 5)
            launches += 1
            for i in range(3):
                w = select(u[i], N - 7, 5)
                assert np.array_equal(ix[i], w[1]) and np.array_equal(bits(sc[i]), bits(w[0]))
            check_launch(chip, case, n_cus, 3, 5, N - 7, sfc.QUERY, False, launches)
            # the host selection itself against the oracle's own top-k
            for k, K in ((ks[3], 5), (R * W + 1, 16), (N, 16)):
                q = db[qrows]
                want = (oracle_lib.scan_topk_synth(SEED, k, case.D, q, K, plants, nthreads=THREADS) if case.elem == 4
                        else oracle_lib.scan_topk_f64(db, k, q, K, nthreads=THREADS))
                for i in range(4):
                    w = select(u[i], k, K)
                    assert np.array_equal(want[1][i], w[1]) and np.array_equal(bits(want[0][i]), bits(w[0])), (k, K, i)
            return

        p = every_tick_params()
        top_k = tick_ks[-1]

        def check_record(g, k):
            l = k + 50
            assert g["status"] == capi.CHIP_TICK_SCANNED, g
            for i in range(3):
                sc, ix = select(oracle_lib.scores(db, k, db[l - 1 - i], nthreads=THREADS), k, 1)
                assert g["argmax"][i] == ix[0] and float(g["maxv"][i]).hex() == float(sc[0]).hex(), (k, i, g, sc, ix)
            assert g["argmax"][0] == max(c for c in copies if c < k), (k, g)      # the newest query is a copy: the highest copy wins
            if k in (tick_ks[0], tick_ks[len(tick_ks) // 2], top_k):
                same_tick(g, oracle_tick(db, l))

        if case.call == sfc.SYNC:
            for k in tick_ks:
                g = chip.loop_tick(k + 50, p).as_dict()
                launches += 1
                check_launch(chip, case, n_cus, 3, capi.CHIP_DEFAULT_TOPK, k, sfc.SYNC, k == top_k, launches)
                check_record(g, k)
        else:
            for w0 in range(0, len(tick_ks), 3):              # three ticks in flight
                win = tick_ks[w0:w0 + 3]
                for s, k in enumerate(win):
                    chip.loop_tick_enqueue(k + 50, s, p)
                launches += len(win)
                check_launch(chip, case, n_cus, 3, capi.CHIP_DEFAULT_TOPK, win[-1], sfc.TICK, win[-1] == top_k, launches)
                for s, k in enumerate(win):
                    check_record(chip.loop_tick_collect(s).as_dict(), k)
        assert chip.coalesce_stats() == (0, 0)
