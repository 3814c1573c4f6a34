"""What the GPU tests of the prefilter passes share (tests/test_pass_lists_gpu.py, tests/test_rescore_gpu.py): one window of forced-parked
ticks, the pass read back (chip_debug_last_pass), and EVERY entry of every list held to the oracle's mirror of the pass's arithmetic and to
the list-driven model of tick_rescore.  Nothing is sampled, no tolerance but E / E_h as the pass itself was given it."""
import numpy as np

import np_mirror_rescore as model
import oracle_lib
import test_halfq_bound as hb
import test_prefilter_bound as pb
from cerebro_amd import capi
from test_prefilter_gpu import every_tick_params, rec, run_window

TICKS = {"prefilter": 4, "halfq": 5}


def hexs(a):
    return [float(x).hex() for x in np.asarray(a).ravel()]


def check_window(chip, db, w, family, expect_cert=None, alone=True):
    """Run the window w (prefixes; tick t is issued at l = w[t] + 50, its queries are rows l - 1, l - 2, l - 3) as ONE pass of `family` and check
    everything the pass left.  Returns (records, last_pass dict, model results [T][3])."""
    p = every_tick_params()
    T = TICKS[family]
    assert len(w) == T
    D = db.shape[1]
    unc_before = chip.prefilter_stats()
    ls, got = run_window(chip, w, p)
    assert (ls["family"], ls["ticks"], ls["n_rows"]) == (family, T, max(w)), ls
    lp = chip.last_pass()
    grid, wpb, K = ls["grid"], ls["block"] // 64, ls["K"]
    assert (lp["family"], lp["ticks"], lp["grid"], lp["wpb"], lp["K"], lp["k"]) == (family, T, grid, wpb, K, list(w)), lp
    assert lp["cand_s"].shape == (T, grid, 3, K) and lp["exact_s"].shape == (T, 3, K)

    # the bound and the scale the pass was submitted with: the library's own functions of the ctx's norm bound, and the formulas of the bound tests
    norm_max = chip.info()["row_norm_max"]
    if family == "halfq":
        e, E = capi.halfq_bound(D, norm_max)
        assert (lp["e"], lp["E"]) == (e, E), (lp["e"], lp["E"], e, E)
        assert e == hb.exponent(norm_max) and abs(E - hb.error_bound(D, norm_max, e)) <= E * 1e-14
    else:
        e, E = 0, lp["E"]
        assert lp["e"] == 0 and abs(E - pb.error_bound(D, norm_max)) <= E * 1e-14

    kmax = max(w)
    qrows = [k + 50 - 1 - i for k in w for i in range(3)]
    queries = np.ascontiguousarray(db[qrows])
    mirror = oracle_lib.pass_scores(db, kmax, queries, halfq=family == "halfq", e=e)          # [3T, kmax]: the pass's score of every pair
    exact = np.stack([oracle_lib.scores(db, kmax, q, nthreads=16) for q in queries])         # the oracle's fp64 score of every pair

    results = []
    n_entries = 0
    for t, k in enumerate(w):
        results.append([])
        for q in range(3):
            gs, gi = lp["cand_s"][t, :, q], lp["cand_i"][t, :, q]                            # [grid, K]
            m, x = mirror[3 * t + q], exact[3 * t + q]
            valid = gi >= 0
            n_entries += gi.size
            where = (family, list(w), t, q)
            # every entry: a row inside the prefix that its workgroup owns, no row twice
            rows = gi[valid]
            assert ((rows >= 0) & (rows < k)).all(), where
            assert (model.owner(rows, grid, wpb) == np.nonzero(valid)[0]).all(), where
            assert len(np.unique(rows)) == len(rows), where
            assert (np.isneginf(gs[~valid])).all() and (gi[~valid] == -1).all(), where
            # the premise of the proof first, on its own: every score the pass kept is within E of the exact score of its pair
            err = np.abs(gs[valid] - x[rows])
            assert err.size == 0 or err.max() <= E, (where, float(err.max()), E)
            # every entry's score has exactly the bits of the mirror for that (row, query)
            bad = np.flatnonzero(model.bits(gs[valid]) != model.bits(m[rows]))
            assert bad.size == 0, (where, len(bad), [(int(rows[i]), float(gs[valid][i]).hex(), float(m[rows[i]]).hex()) for i in bad[:4]])
            # every list is the top K of (score descending, index descending) over the rows its workgroup owns inside the prefix
            ws, wi = model.pass_lists(m, k, grid, wpb, K)
            assert (gi == wi).all(), (where, np.argwhere(gi != wi)[:4].tolist())
            assert (model.bits(gs) == model.bits(ws)).all(), where
            # tick_rescore from the lists the device holds: certificate word and exact list
            r = model.rescore(gs, gi, k, wpb, K, E, x)
            results[-1].append(r)
            assert int(lp["cert"][t, q]) == r["cert"], (where, int(lp["cert"][t, q]), {a: r[a] for a in ("G", "M", "dropped", "thr", "cert")}, len(r["R"]))
            if r["exact_s"] is not None:                                                     # (beyond the cap the kernel keeps whichever rows came first)
                assert list(lp["exact_i"][t, q]) == list(r["exact_i"]), (where, lp["exact_i"][t, q], r["exact_i"])
                assert hexs(lp["exact_s"][t, q]) == hexs(r["exact_s"]), where
    assert n_entries == T * grid * 3 * K

    certs = [[r["cert"] for r in tick] for tick in results]
    if expect_cert is not None:
        assert [int(all(c == 1 for c in tick)) for tick in certs] == list(expect_cert), (family, list(w), certs)
    # ticks whose certificate did not hold ran again alone: the counter moved by the model's count
    n_unc = sum(1 for tick in certs if any(c != 1 for c in tick))
    assert tuple(a - b for a, b in zip(chip.prefilter_stats(), unc_before)) == (1, T, n_unc), (family, list(w), certs)

    # the records: what topk_merge gives on the exact lists read back (halfq: the five came out of the one pass_merge launch) ...
    for t, k in enumerate(w):
        if all(c == 1 for c in certs[t]):
            _, _, r = chip.debug_merge_lists(0, lp["exact_s"][t][None], lp["exact_i"][t][None], l=k + 50, params=p, record=True)
            assert bytes(r) == got[t], (family, list(w), t)
    # ... and the record of the same tick issued alone (the synchronous tick never shares a pass)
    if alone:
        for t, k in enumerate(w):
            assert bytes(chip.loop_tick(k + 50, p)) == got[t], (family, list(w), t, certs[t])
            a = rec(got[t])
            best = [model.topk_by_key(exact[3 * t + q][:k], np.arange(k), 1) for q in range(3)]
            assert list(a.argmax) == [int(b[1][0]) for b in best] and hexs(a.maxv) == hexs([b[0][0] for b in best]), (family, list(w), t)
    return got, lp, results
