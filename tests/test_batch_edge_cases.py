"""The case families of tests/batch_edge_cases.py must BITE: each condition below holds on the CPU oracle alone, and proves that a
kernel which sums in another order, fuses an MFMA k-pair into one three-term add, flushes subnormals, mixes up the signed zeros or
mishandles non-finite scores would fail tests/test_batch_edges_gpu.py.  Conditions, not measurements."""
import ctypes as C

import numpy as np

import batch_edge_cases as bec
import oracle_lib
from batch_edge_cases import N, QROWS, SPECIAL, U

FLT_MIN = 2.0 ** -126


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def chain_scores(db32, q32):
    """every score of the oracle's fmaf chain, float32 [nq][rows]"""
    lib = oracle_lib.load()
    db32, q32 = np.ascontiguousarray(db32, dtype=np.float32), np.ascontiguousarray(q32, dtype=np.float32)
    out = np.empty((q32.shape[0], db32.shape[0]), dtype=np.float32)
    D = db32.shape[1]
    for i, qv in enumerate(q32):
        qp = qv.ctypes.data_as(C.c_void_p)
        for r in range(db32.shape[0]):
            out[i, r] = lib.orc_dot_fmaf_f32(qp, db32[r].ctypes.data_as(C.c_void_p), D)
    return out


def exact_scores(db32, q32):
    """fp64 accumulation of the exact products, rounded to float once"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (q32.astype(np.float64) @ db32.astype(np.float64).T).astype(np.float32)


def top_of(scores, K):
    """index list of the top-K of one score vector by (score desc, index desc), NaN never enters"""
    order = sorted((i for i in range(len(scores)) if scores[i] == scores[i]), key=lambda i: (-float(scores[i]), -i))
    return order[:K]


def test_placement_and_prefixes():
    assert {0, 63, 64, 127, 128, 255, 256, N - 1} <= set(SPECIAL) and any(640 < r < N - 1 for r in SPECIAL)
    ks = bec.prefixes()
    for r in SPECIAL:
        assert r in ks and r + 1 in ks and (r + 2 in ks or r + 2 > N)
    for name, fam in bec.FAMILIES.items():
        db, q, what = fam()
        db2, q2, _ = fam()
        assert db.tobytes() == db2.tobytes() and q.tobytes() == q2.tobytes(), name          # deterministic
        assert q.shape == (bec.NQ, what["D"]) and q.dtype == np.float32 and db.shape[1] == what["D"]
        assert db.dtype == (np.float64 if name == "cast_edges" else np.float32)
        assert np.isfinite(db).all(), name                                                    # appends refuse NaN / Inf rows


def test_overflow_bites():
    db, q, what = bec.overflow()
    assert np.isfinite(q).all()
    mags = np.abs(np.concatenate([db[db != 0], q[q != 0]]))
    assert mags.min() >= 2.0 ** 61.5 * (1 - 2.0 ** -24) and mags.max() <= 2.0 ** 63.5       # (the float nearest to 2^61.5 may lie just below it)
    sel = sorted(set(QROWS) | set(range(5, 13)))
    with np.errstate(over="ignore"):
        ch, ex = chain_scores(db, q[sel]), exact_scores(db, q[sel])
    assert not np.isnan(ch).any()                       # fmaf(finite, finite, +-inf) = +-inf: finite inputs never give NaN
    lost = (~np.isfinite(ch) & np.isfinite(ex)).sum(axis=1)
    assert (lost >= 4).sum() >= 4, lost
    differ = [t for i, t in enumerate(sel) if top_of(ch[i], 8) != top_of(ex[i], 8)]
    assert len(differ) >= 2, differ
    # the plants: the chain is infinite with the sign of the plant, the exact sum finite, for the probe queries of either sign
    for t in what["probes"]:
        i = sel.index(t)
        sgn = 1.0 if q[t, what["reserved"][0]] > 0 else -1.0
        for r, (a1, a2, b, c, s) in what["plants"].items():
            assert ch[i, r] == sgn * s * np.inf and np.isfinite(ex[i, r]) and ex[i, r] != 0, (t, r)
    # overflow happens AT b -- at an even and at an odd k of a k-pair -- with the cancelling term in the same pair, in the next and across 31/32
    pats = bec.OVERFLOW_PATTERNS
    assert {b % 2 for _, _, b, _ in pats} == {0, 1}
    assert any(b % 2 == 0 and c == b + 1 for _, _, b, c in pats) and any(c // 2 == b // 2 + 1 for _, _, b, c in pats)
    assert any((b, c) == (31, 32) for _, _, b, c in pats) and any(a2 // 2 == b // 2 for _, a2, b, _ in pats)
    i3 = sel.index(3)                                   # the half-scale probe: the same rows without an overflow
    assert np.isfinite(ch[i3]).all() and all(ch[i3, r] != 0 for r in what["plants"])
    # the oracle's own lists are the lists of these chains
    ws, wi = oracle_lib.scan_topk_fmaf(db, N, q[sel], 8)
    for i in range(len(sel)):
        assert list(wi[i]) == top_of(ch[i], 8)


def test_subnormal_bites():
    db, q, what = bec.subnormal()
    dense = what["dense"][:12]
    ws, wi = oracle_lib.scan_topk_fmaf(db, N, q[dense], 16)
    sub = [(np.abs(ws[i]) > 0).all() and (np.abs(ws[i]) < FLT_MIN).all() for i in range(len(dense))]
    assert sum(sub) >= 4
    assert max(len(set(ws[i])) for i in range(len(dense))) >= 8          # distinct subnormal scores, not one tie
    # flushing results to zero changes the lists of the dense queries ...
    ch = chain_scores(db, q[dense[:4]])
    flushed = np.where(np.abs(ch) < FLT_MIN, np.float32(0), ch)
    assert sum(top_of(ch[i], 8) != top_of(flushed[i], 8) for i in range(4)) >= 2
    # ... and flushing subnormal INPUTS those of the probes that multiply a subnormal element by about 1e3
    p23 = [t for t, kind in what["kinds"].items() if kind in (1, 2)]
    assert len(p23) >= 2
    dbf, qf = np.where(np.abs(db) < FLT_MIN, np.float32(0), db), np.where(np.abs(q) < FLT_MIN, np.float32(0), q)
    assert (dbf != db).any() and (qf != q).any()
    ch2, ch2f = chain_scores(db, q[p23]), chain_scores(dbf, qf[p23])
    assert sum(top_of(ch2[i], 8) != top_of(ch2f[i], 8) for i in range(len(p23))) >= 2
    # rows whose exact sum lies between two subnormals: every step of the chain rounds (multiples of 2^-149, by hand)
    p1 = [t for t, kind in what["kinds"].items() if kind == 0][0]
    chain_u, exact_u = (4, 4, 2, 4, 0), (3, 3, 1, 6, 2)
    got = chain_scores(db[list(what["plants"])], q[[p1]])[0]
    for r, g in zip(what["plants"], got):
        pat = what["plants"][r]
        assert float(g) == chain_u[pat] * U and chain_u[pat] != exact_u[pat], (r, pat, float(g) / U)
    assert float(chain_scores(db[[1]], q[[p1]])[0, 0]) == 0.0             # an ordinary row scores +0.0 against a probe


def test_signed_zero_lists_by_hand():
    db, q, what = bec.signed_zero()
    kind, qk = what["kind"], what["queries"]
    assert {kind[r] for r in SPECIAL} == {bec.SZ_UNDERFLOW, bec.SZ_NEG}
    for name in ("zero", "mzero", "under"):
        ts = [t for t, n_ in qk.items() if n_ == name]
        assert ts
        for k in (1, 2, 16, 17, 64, 65, 129, 257, 651, N):
            ws, wi = oracle_lib.scan_topk_fmaf(db, k, q[ts], 16)
            idx = [k - 1 - j if j < k else -1 for j in range(16)]          # index-descending: every row ties at zero
            sc = [np.float32(-np.inf) if i < 0 else np.float32(-0.0) if name == "under" and kind[i] == bec.SZ_UNDERFLOW else np.float32(0.0) for i in idx]
            for i in range(len(ts)):
                assert list(wi[i]) == idx, (name, k)
                assert list(bits(ws[i])) == list(bits(sc)), (name, k)     # +0.0 bit patterns; -0.0 only where the chain ends in an underflow
    assert any(bits(np.float32(s))[()] == 0x80000000 for s in oracle_lib.scan_topk_fmaf(db, N, q[[t for t, n_ in qk.items() if n_ == "under"][:1]], 16)[0][0])
    # "cancel": the CANCEL rows score exactly +0.0 among the real scores of the others
    tc = [t for t, n_ in qk.items() if n_ == "cancel"][0]
    ch = chain_scores(db, q[[tc]])[0]
    assert all(bits(ch[r])[()] == 0 for r in range(N) if kind[r] == bec.SZ_CANCEL) and (ch[kind != bec.SZ_CANCEL] != 0).all()


def test_negzero_heads_by_hand():
    db, q, what = bec.negzero_heads()
    ws, wi = oracle_lib.scan_topk_fmaf(db, what["N"], q[what["probes"][:1]], 8)
    assert what["minus_zero"] > what["plus_zero"]
    assert list(wi[0]) == what["pos"][::-1] + [what["minus_zero"], what["plus_zero"]]
    assert list(bits(ws[0][6:])) == [0x80000000, 0]
    heads = chain_scores(db, q[what["probes"][:1]])[0]
    tiles = [heads[t * 128:(t + 1) * 128].max() for t in range(10)]
    assert len({float(x) for x in tiles}) == 9 and tiles[6] == 0 and tiles[7] == 0   # no two heads alike but the two zeros


def test_all_tie_lists_by_hand():
    db, q, what = bec.all_tie()
    assert (db == db[0]).all() and N >= 600
    for k in (1, 15, 16, 17, 257, N):
        ws, wi = oracle_lib.scan_topk_fmaf(db, k, q[:8], 16)
        idx = [k - 1 - j if j < k else -1 for j in range(16)]
        for t in range(8):
            s = np.float32(0.0) if t in what["zero"] else chain_scores(db[:1], q[[t]])[0, 0]
            assert list(wi[t]) == idx
            assert list(bits(ws[t])) == [bits(s)[()] if i >= 0 else bits(np.float32(-np.inf))[()] for i in idx]
    assert 0 in what["zero"] and not q[0].any() and not np.signbit(q[0]).any() and q[1].any()


def test_nonfinite_queries_bite():
    db, q, what = bec.nonfinite_queries()
    qk = what["queries"]
    K = 16
    by = {n_: [t for t, m in qk.items() if m == n_] for n_ in ("nan", "inf1", "inf2")}
    assert all(by.values())
    # every tile row the kernel's blocks begin or end on carries a non-finite query -- also in the repeated queries 256.. -- next to finite ones
    for t in (0, 31, 32, 63, 64, 127, 128, 255, 256, 256 + 31, 256 + 32, 256 + 127):
        assert not np.isfinite(q[t]).all(), t
    assert {qk[t] for t in (0, 31, 32, 63, 64, 127, 128, 255)} == {"nan", "inf1", "inf2"}
    for t in (2, 4, 30, 33, 62, 65, 126, 129, 254, 256 + 33):
        assert np.isfinite(q[t]).all(), t
    ws, wi = oracle_lib.scan_topk_fmaf(db, N, q, K)
    for t in by["nan"]:
        assert (wi[t] == -1).all() and np.isneginf(ws[t]).all()
    for t in by["inf1"]:                                 # a real row at -inf inside the top-K of a prefix of N >= K rows
        assert list(wi[t][:len(what["plus"])]) == what["plus"][::-1] and np.isposinf(ws[t][:len(what["plus"])]).all()
        assert np.isneginf(ws[t][len(what["plus"]):]).all() and (wi[t][len(what["plus"]):] >= 0).all()
    ws20, wi20 = oracle_lib.scan_topk_fmaf(db, 20, q[by["inf1"]], K)       # 20 >= K rows, 7 of them score NaN
    assert ((wi20 >= 0).sum(axis=1) == 13).all() and (wi20[:, 13:] == -1).all()
    assert any((wi[t] >= 0).all() and not np.isfinite(ws[t]).all() for t in by["inf2"])
    # the neighbours of every non-finite query are finite queries with finite lists
    for t in qk:
        for nb in (t - 1, t + 1):
            if 0 <= nb < bec.NQ_BASE and nb not in qk:
                assert np.isfinite(q[nb]).all() and np.isfinite(ws[nb]).all()


def test_cast_edges_bite():
    db, q, what = bec.cast_edges()
    with np.errstate(over="ignore"):
        db32 = db.astype(np.float32)
    # numpy's cast is the definition: check it against the values written down next to each edge
    for j, r in enumerate(bec.CAST_FINITE_ROWS):
        for i, (x, want) in enumerate(bec.CAST_FINITE):
            p = bec.cast_position(i, j)
            assert db[r, p] == x and bits(db32[r, p])[()] == bits(np.float32(want))[()], (r, i)
    for j, r in enumerate(bec.CAST_INF_ROWS):
        for i, x in enumerate(bec.CAST_INF):
            assert db32[r, bec.cast_position(3 * i + 1, j)] == np.float32(np.copysign(np.inf, x))
    nz = db != 0
    got = db32[nz]
    assert np.isposinf(got).any() and np.isneginf(got).any() and ((np.abs(got) > 0) & (np.abs(got) < FLT_MIN)).any()
    assert (bits(got) == 0).any() and (bits(got) == 0x80000000).any()     # +0.0 and -0.0 out of non-zero doubles
    # all eight 16-byte slots of a chunk, all four store rotations
    slots = {(bec.cast_position(i, j) % 32) // 4 for j in range(len(bec.CAST_FINITE_ROWS)) for i in range(len(bec.CAST_FINITE))}
    assert slots == set(range(8))
    for tile in (128, 256):
        assert {((r % tile) >> 3) & 3 for r in bec.CAST_FINITE_ROWS} == {0, 1, 2, 3}
        assert {((r % tile) >> 3) & 3 for r in bec.CAST_INF_ROWS} >= {0, 1, 2}
    # a probe of position p sees the finite edge rows that hold an edge there on top of the (negative) ordinary rows
    seen = set()
    for t, p in what["probes"].items():
        if t < 64:
            continue
        ws, wi = oracle_lib.scan_topk_fmaf(db32, N, q[[t]], 16)
        for r in wi[0]:
            if what["edges"].get(int(r)) == "finite":
                j = bec.CAST_FINITE_ROWS.index(int(r))
                seen |= {i for i in range(len(bec.CAST_FINITE)) if bec.cast_position(i, j) == p}
    assert seen == set(range(len(bec.CAST_FINITE))), seen
