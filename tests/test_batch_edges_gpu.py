"""The many-query mode (cerebro_amd/csrc/batch.hip db_gemm_topk + merge_sorted_lists; chip_query_batch_f32 on float rows,
chip_query_batch_cast_f32 on double rows) at its edges, against the oracle's fmaf chain (oracle_lib.scan_topk_fmaf of
db.astype(float32)): indices equal, scores equal as uint32 bit patterns -- never as floats, a -0.0 is not a +0.0 here.

  * the families of tests/batch_edge_cases.py -- fp32 overflow, subnormals, signed zeros, a -0.0 list head, all-tie, non-finite queries,
    the edges of the double -> float cast -- on both storage types and both tile shapes, K = 1, 8, 16, prefixes that end one row
    before / on / after every special row, with the default grid and with the grid capped to 1 and 3 workgroups (one workgroup's register lists then carry +-inf and real -inf entries across claimed tiles and
    through the query-half units);
  * the all-tie DB on a group ctx and on shard contexts (the K highest indices live on different shards);
  * a DB that crosses a segment boundary, per storage type, at D = 8224 (8192 rows per segment, 257 K-chunks);
  * D = 8192 itself.

Tile shapes.  The query count is padded to a multiple of 128; a padded count that is a multiple of 256 takes the 256 x 256 tile (on double
rows only for K <= 8), anything else the 128 x 128 one.  Q = 256 and Q = 130 both pad to 256 (the wide tile, full and with 126 zero
queries; the small one on double rows at K = 16); Q = 300 pads to 384 -- three 128 x 128 query tiles, query 128 = row 0 of the second,
256 = row 0 of the third, the last one partial -- and Q = 5 is one 128 x 128 tile."""
import functools

import numpy as np
import pytest

import batch_edge_cases as bec
import oracle_lib
from cerebro_amd import capi
from test_batch_cast_gpu import f32bits, relja_like

pytestmark = pytest.mark.gpu
SEG_BYTES = 512 << 20            # the segment target of configure_storage (chip_api.hip): rows are counted as floats for either storage type


def seg_rows(D):
    """mirror of configure_storage: the largest power of two of rows within SEG_BYTES / (4 D), at least 64"""
    n = 64
    while 2 * n * D * 4 <= SEG_BYTES:
        n *= 2
    return n


class Want:
    """the oracle's top-16 lists of one (db32, q), one scan per prefix, shared by every test of the family"""

    def __init__(self, db32, q):
        self.db32, self.q, self.memo = db32, q, {}

    def __call__(self, k, K, Q):
        if k not in self.memo:
            s, i = oracle_lib.scan_topk_fmaf(self.db32, k, self.q, 16)
            s.setflags(write=False)
            i.setflags(write=False)
            self.memo[k] = (s, i)
        s, i = self.memo[k]
        return s[:Q, :K], i[:Q, :K]


@functools.lru_cache(maxsize=None)
def family(name):
    db, q, what = bec.FAMILIES[name]()
    with np.errstate(over="ignore"):
        db32 = db.astype(np.float32)
    return db, q, what, Want(db32, q)


def open_chip(D, db, storage, **kw):
    """float rows as they are; "f64": the same values (or the family's own doubles) as double rows, read through the cast entry"""
    if storage == "f64":
        chip = capi.Chip(D, storage="f64", **kw)
        chip.append_f64(np.asarray(db, dtype=np.float64))
        assert chip.info()["storage_bytes"] == 8
    else:
        chip = capi.Chip(D, **kw)
        chip.append_f32(db)
        assert chip.info()["storage_bytes"] == 4
    return chip


def compare(got, want, ctx):
    (gs, gi), (ws, wi) = got, want
    if not np.array_equal(gi, wi):
        t = int(np.nonzero((gi != wi).any(axis=1))[0][0])
        raise AssertionError(f"{ctx}: indices of query {t}: got {list(gi[t])} scores {list(gs[t])}, want {list(wi[t])} scores {list(ws[t])}")
    gb, wb = f32bits(gs), f32bits(ws)
    if not np.array_equal(gb, wb):
        t = int(np.nonzero((gb != wb).any(axis=1))[0][0])
        raise AssertionError(f"{ctx}: score bits of query {t}: got {[hex(x) for x in gb[t]]}, want {[hex(x) for x in wb[t]]}")


def set_wgs(monkeypatch, wgs):
    if wgs:
        monkeypatch.setenv("CHIP_BATCH_WGS", str(wgs))
    else:
        monkeypatch.delenv("CHIP_BATCH_WGS", raising=False)


QS = [256, 130, 300, 5]
CASES = [(n, s) for n in bec.FLOAT_FAMILIES for s in ("f32", "f64")] + [("cast_edges", "f64")]


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name,storage", CASES)
def test_family_against_the_oracle(name, storage, Q, monkeypatch):
    db, q, what, want = family(name)
    ks = bec.family_prefixes(name, what)
    with open_chip(what["D"], db, storage) as chip:
        for wgs in (0, 1, 3):
            set_wgs(monkeypatch, wgs)
            for K in (1, 8, 16):
                for k in ks:
                    got = chip.query_batch(k, q[:Q], K, cast_rows=storage == "f64")
                    compare(got, want(k, K, Q), f"{name} {storage} Q={Q} wgs={wgs} K={K} k={k}")


def host_merge(parts, qi, K):
    """(score desc, index desc) over the shards' lists, as test_batch_sharded_lists_are_consistent does; ties compare equal as floats"""
    cand = sorted(((float(s), int(i)) for ps, pi in parts for s, i in zip(ps[qi], pi[qi]) if i >= 0), key=lambda t: (-t[0], -t[1]))[:K]
    cand += [(-np.inf, -1)] * (K - len(cand))
    return [c[0] for c in cand], [c[1] for c in cand]


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_all_tie_across_shards(storage):
    """every row ties: the K highest indices of a prefix live on different shards, so the cross-shard merge ranks on its exact path"""
    db, q, what, want = family("all_tie")
    G, D, cast = 3, what["D"], storage == "f64"
    ks = (1, 2, 3, 4, 17, 257, bec.N - 1, bec.N)
    with open_chip(D, db, storage, devices=[0] * G) as chip:
        for Q in QS:
            for K in (1, 8, 16):
                for k in ks:
                    compare(chip.query_batch(k, q[:Q], K, cast_rows=cast), want(k, K, Q), f"group {storage} Q={Q} K={K} k={k}")
    Q = 300                                          # three small query tiles per shard
    shards = [open_chip(D, db, storage, shard_rank=r, shard_count=G) for r in range(G)]
    try:
        for K in (1, 8, 16):
            for k in ks:
                parts = [c.query_batch(k, q[:Q], K, cast_rows=cast) for c in shards]
                for r, (ps, pi) in enumerate(parts):
                    assert ((pi < 0) | (pi % G == r)).all()                # a shard answers for its own rows, global indices
                ws, wi = want(k, K, Q)
                for t in (0, 1, 2, 3, 31, 32, 127, 128, 129, 255, 256, 299):
                    s, i = host_merge(parts, t, K)
                    assert i == list(wi[t]) and list(f32bits(s)) == list(f32bits(ws[t])), (storage, K, k, t)
    finally:
        for c in shards:
            c.close()


# ---------------------------------------------------------------------------------------------------------------- segment crossing
SEG_D = 8224                     # 8192 rows per segment: 257 MiB of float rows, 514 MiB of double rows; 257 K-chunks
CHECKED = (0, 1, 2, 3, 4, 31, 32, 63, 64, 127, 128, 255, 256, 299)   # the queries the oracle answers (per-query results are independent)


def merged(head, tail, off, K):
    """top-K of a union = top-K of the union of the top-Ks: the list of [0, off) and the list of the short tail, indices offset"""
    (hs, hi), (ts, ti) = head, tail
    out_s, out_i = np.full((hs.shape[0], K), -np.inf), np.full((hs.shape[0], K), -1, dtype=np.int64)
    for t in range(hs.shape[0]):
        cand = [(float(s), int(i)) for s, i in zip(hs[t], hi[t]) if i >= 0] + [(float(s), int(i) + off) for s, i in zip(ts[t], ti[t]) if i >= 0]
        cand = sorted(cand, key=lambda c: (-c[0], -c[1]))[:K]
        out_s[t, :len(cand)], out_i[t, :len(cand)] = [c[0] for c in cand], [c[1] for c in cand]
    return out_s, out_i


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_batch_across_a_segment_boundary(storage, monkeypatch):
    """The float loader takes every row's base from seg_table[row >> seg_shift]; the cast loader one base per tile and 32-bit byte
    offsets.  Tiles on both sides of the boundary, one workgroup walking claimed tiles from segment 0 into segment 1 (capped grid),
    duplicates that straddle the boundary, a query equal to the first row of segment 1."""
    D, seg = SEG_D, seg_rows(SEG_D)
    n = seg + 300
    assert seg == 8192
    db = relja_like(4242, n, D)
    if storage == "f32":
        db = db.astype(np.float32)
    db[seg] = db[seg - 1]                        # an exact duplicate pair across the boundary
    db[seg + 200] = db[100]                      # a segment-0 row again, late in segment 1
    db32 = db.astype(np.float32)
    q = db32[np.random.default_rng(7).choice(n, 300, replace=False)].copy()
    for t, r in ((1, seg), (2, 100), (3, seg + 200), (4, seg + 1), (63, seg - 2), (64, n - 1)):
        q[t] = db32[r]
    qc = q[list(CHECKED)]
    head = oracle_lib.scan_topk_fmaf(db32, seg - 1, qc, 16)                       # once; the tail [seg - 1, k) per prefix
    ks = (seg - 1, seg, seg + 1, seg + 127, seg + 128, seg + 129, seg + 255, seg + 256, seg + 257, n)
    wants = {k: merged(head, oracle_lib.scan_topk_fmaf(db32[seg - 1:], k - (seg - 1), qc, 16), seg - 1, 16) for k in ks}
    assert list(wants[n][1][1][:2]) == [seg, seg - 1] and list(wants[n][1][2][:2]) == [seg + 200, 100]   # the plants top their queries
    with open_chip(D, db, storage) as chip:
        info = chip.info()
        assert info["rows_local"] == n and info["capacity_local"] == 2 * seg, info                    # two segments, or this test shows nothing
        for wgs in (0, 3):
            set_wgs(monkeypatch, wgs)
            for Q, K in ((256, 8), (130, 16), (300, 8), (300, 16)):   # wide; wide (small on double rows); small, three query tiles
                sel = [j for j, t in enumerate(CHECKED) if t < Q]
                rows = [CHECKED[j] for j in sel]
                for k in ks:
                    gs, gi = chip.query_batch(k, q[:Q], K, cast_rows=storage == "f64")
                    ws, wi = wants[k]
                    compare((gs[rows], gi[rows]), (ws[sel][:, :K], wi[sel][:, :K]), f"segments {storage} wgs={wgs} Q={Q} K={K} k={k}")


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_batch_parity_at_D_8192(storage):
    """the reference's default model width: 256 K-chunks through the two-stage ring"""
    D, n = 8192, 600
    db = relja_like(8192, n, D)
    if storage == "f32":
        db = db.astype(np.float32)
    db32 = db.astype(np.float32)
    q = db32[np.random.default_rng(11).choice(n, 300, replace=False)]
    want = Want(db32, q)
    with open_chip(D, db, storage) as chip:
        for Q, K in ((130, 8), (256, 8), (300, 8), (130, 16), (256, 16), (300, 16)):
            for k in (257, n):
                compare(chip.query_batch(k, q[:Q], K, cast_rows=storage == "f64"), want(k, K, Q), f"D=8192 {storage} Q={Q} K={K} k={k}")
