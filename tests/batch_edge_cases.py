"""Edge-case families of the many-query mode (cerebro_amd/csrc/batch.hip db_gemm_topk, the shared merge_sorted_lists, the entries
chip_query_batch_f32 / chip_query_batch_cast_f32).  Deterministic, seeded generators shared by tests/test_batch_edge_cases.py (CPU:
each family must bite on the oracle alone) and tests/test_batch_edges_gpu.py (device: every family against the oracle, bit for bit).

A family returns (db, queries, what): db is float32 [N][D] (float64 for the cast edges), queries float32 [384][D] -- 256 generated ones, the
first 128 repeated behind them; the tests run queries[:Q] for Q = 256 and 130 (both pad to 256: the 256 x 256 tile), Q = 300 (pads to
384: three 128 x 128 query tiles) and Q = 5 (one 128 x 128 tile), so everything special sits at the tile rows QROWS, the first five
included -- and `what` names the planted rows / queries for the checks that need them.

Geometry.  D = 64 is two K-chunks of 32 (the k = 31/32 boundary lies inside the chain), D = 96 an odd number of chunks.  N = 700
is three 256-row tiles or six 128-row tiles, the last one partial.  Every family puts its special rows at SPECIAL: the first and
last row of a tile of either shape, the last row of the DB and rows inside the final partial tile; prefixes() ends one row before,
on and one row after each of them.

"Probe" queries are non-zero only on a reserved set of elements on which ordinary rows hold zero: an ordinary row scores +0.0
against a probe and the planted rows' crafted scores stand on top of the list (or, negated, at its bottom) where a top-K check sees
them."""
from __future__ import annotations

import numpy as np

N = 700
SPECIAL = (0, 63, 64, 127, 128, 255, 256, 650, 690, N - 1)       # 650, 690: inside the partial tile of both shapes (512.., 640..)
QROWS = (0, 1, 2, 3, 4, 31, 32, 63, 64, 127, 128, 255)            # rows of the special queries (128 = row 0 of the second small tile, of the upper half of the wide one)
NQ_BASE, NQ = 256, 384                                             # generated queries; with queries[:128] repeated at 256..383
U = 2.0 ** -149                                                    # the smallest float subnormal
FLT_MAX = float(np.finfo(np.float32).max)


def prefixes(n=N, rows=SPECIAL):
    """prefixes [0, k) whose last row is one before, on, and one after every special row"""
    return sorted({k for r in rows for k in (r, r + 1, r + 2) if 0 <= k <= n})


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _queries(q):
    """384 queries: a padded count that is no multiple of 256 (the 128 x 128 tile) spans three query tiles; row 256 = row 0 again"""
    return _f32(np.concatenate([q, q[:NQ - NQ_BASE]]))


def _sparse(rng, n, D, allowed, nnz, lo, hi):
    """n rows with nnz non-zero elements on `allowed`, magnitudes 2^[lo, hi), random signs"""
    out = np.zeros((n, D), dtype=np.float64)
    for r in range(n):
        pos = rng.choice(allowed, nnz, replace=False)
        out[r, pos] = np.exp2(rng.uniform(lo, hi, nnz)) * rng.choice([-1.0, 1.0], nnz)
    return out


# ------------------------------------------------------------------------------------------------------------------ overflow
# (a1, a2, b, c): three products P = 2^126.6 at a1, a2, b -- the chain is 2P (finite) before b and overflows AT b -- and a cancelling
# -c P at c.  fmaf(finite, finite, +-inf) = +-inf, so the chain stays infinite while the exact sum (3 - c) P is finite.  b at an even
# and at an odd k of an MFMA k-pair (2j, 2j+1); c in the same pair, in the next pair, across k = 31/32; a2 and b in one pair.
OVERFLOW_PATTERNS = ((8, 9, 14, 15), (8, 9, 15, 16), (8, 9, 14, 16), (26, 27, 31, 32), (26, 27, 30, 31), (27, 28, 32, 33),
                     (8, 14, 15, 16), (26, 30, 31, 32))
OVERFLOW_CANCEL = (1.0, 1.14, 1.05, 1.1)                          # times 2^63.3 stays within 2^63.5


def overflow(seed=61):
    D = 64
    rng = np.random.default_rng(seed)
    reserved = list(range(8, 17)) + list(range(26, 35))
    free = [e for e in range(D) if e not in reserved]
    db = _sparse(rng, N, D, free, 12, 61.5, 63.5)
    q = _sparse(rng, NQ_BASE, D, list(range(D)), 40, 61.5, 63.5)
    v = 2.0 ** 63.3
    probe = np.zeros(D)
    probe[reserved] = v
    plants = {}
    for j, r in enumerate(SPECIAL):
        a1, a2, b, c = OVERFLOW_PATTERNS[j % len(OVERFLOW_PATTERNS)]
        sign = -1.0 if j % 3 == 2 else 1.0
        db[r, [a1, a2, b]] = sign * v
        db[r, c] = -sign * OVERFLOW_CANCEL[j % 4] * v
        plants[r] = (a1, a2, b, c, sign)
    probes = []
    for j, t in enumerate(QROWS):
        if j % 3 == 2:
            continue                                   # every third special slot keeps its dense random query
        q[t] = probe if j % 3 == 0 else -probe
        probes.append(t)
    q[3] = probe * 2.0 ** -0.5                          # the same plants with P / 2: nothing overflows, the chain is exact
    probes.remove(3)
    return _f32(db), _queries(q), dict(D=D, plants=plants, probes=probes, reserved=reserved)


# ------------------------------------------------------------------------------------------------------------------ subnormal
def subnormal(seed=62):
    D = 96
    rng = np.random.default_rng(seed)
    r1, r2, r3 = [14, 15, 16, 30, 31, 32, 33], [62, 63], [64, 65]
    reserved = r1 + r2 + r3
    free = [e for e in range(D) if e not in reserved]
    db = _sparse(rng, N, D, free, len(free), -76, -72)
    q = _sparse(rng, NQ_BASE, D, free, len(free), -76, -72)
    p1 = np.zeros(D)
    p1[r1] = 2.0 ** -74                                 # times x 2^-75 on the row side: a product of x smallest subnormals
    p2 = np.zeros(D)
    p2[62], p2[63] = 1e3, 1e2                           # times a SUBNORMAL row element
    p3 = np.zeros(D)
    p3[64], p3[65] = 1e-40, 3e-41                       # a SUBNORMAL query element times about 1e3
    h = 2.0 ** -75
    # rows whose exact sum lies between two subnormals: (element, multiple of 2^-149 its product with p1 is)
    tie_rows = [((14, 1.5), (15, 1.5)),                 # 2u, then 3.5u -> 4u; exact 3u (one rounding: 3u)
                ((31, 1.5), (32, 1.5)),                 # the same across the chunk boundary
                ((30, 1.5), (31, -0.5)),                # 2u, then 1.5u -> 2u; exact u
                ((15, 2.5), (16, 2.5), (30, 0.5)),      # 2u, 4.5u -> 4u, 4.5u -> 4u; exact 5.5u -> 6u
                ((32, 0.5), (33, 0.5), (14, 0.5))]      # k order 14, 32, 33: 0.5u -> 0 three times; exact 1.5u -> 2u
    plants = {}
    for j, r in enumerate(SPECIAL):
        for e, m in tie_rows[j % len(tie_rows)]:
            db[r, e] = m * h
        db[r, 62], db[r, 63] = 1e-40 * (1 + j), -2e-41 * (1 + j % 3)
        db[r, 64], db[r, 65] = 1e3 + j, 1e3 - 7 * j
        plants[r] = j % len(tie_rows)
    kinds = {}
    for j, t in enumerate(QROWS):
        if j % 4 == 3:
            continue
        kinds[t] = j % 4
        q[t] = (p1, p2, p3)[j % 4]
    q[4] = -p1
    kinds[4] = 3
    return _f32(db), _queries(q), dict(D=D, plants=plants, kinds=kinds, dense=[t for t in range(NQ_BASE) if t not in kinds])


# ------------------------------------------------------------------------------------------------------------------ signed zero
SZ_CANCEL, SZ_NEG, SZ_UNDERFLOW, SZ_POS = 0, 1, 2, 3
SZ_E = 20                                                # the element the underflow query looks at


def signed_zero(seed=63):
    """Row kinds: CANCEL (x, -x) pairs; NEG all negative, -0.0 at SZ_E; UNDERFLOW all negative, -2^-76 at SZ_E; POS positive with
    -0.0 elements, +0.0 at SZ_E.  Query kinds: "zero" all +0.0; "mzero" all -0.0; "under" 2^-76 at SZ_E only -- an UNDERFLOW row
    scores -2^-152 -> -0.0 there and every later product is -0.0, so the chain ENDS at -0.0, every other row at +0.0; "cancel" equal
    powers of two within each pair (exact products: CANCEL rows score +0.0 among the real scores of the others)."""
    D = 64
    rng = np.random.default_rng(seed)
    kind = np.array([r % 4 for r in range(N)])
    for j, r in enumerate(SPECIAL):
        kind[r] = SZ_UNDERFLOW if j % 2 == 0 else SZ_NEG
    db = np.zeros((N, D))
    for r in range(N):
        x = rng.uniform(0.5, 2.0, D)
        if kind[r] == SZ_CANCEL:
            x[1::2] = -x[0::2]
            x[SZ_E] = x[SZ_E + 1] = 0.0
        elif kind[r] == SZ_NEG:
            x = -x
            x[SZ_E] = -0.0
        elif kind[r] == SZ_UNDERFLOW:
            x = -x
            x[SZ_E] = -2.0 ** -76
        else:
            x[rng.choice(D, 6, replace=False)] = -0.0
            x[SZ_E] = 0.0
        db[r] = x
    q = rng.uniform(-1.0, 1.0, (NQ_BASE, D))
    under = np.zeros(D)
    under[SZ_E] = 2.0 ** -76
    cancel = np.repeat(np.exp2(rng.integers(-3, 4, D // 2)), 2)
    cancel[SZ_E] = cancel[SZ_E + 1] = 0.0
    qk = {}
    for j, t in enumerate(QROWS):
        name = ("zero", "under", "mzero", "cancel")[j % 4]
        q[t] = {"zero": np.zeros(D), "mzero": -np.zeros(D), "under": under, "cancel": cancel}[name]
        qk[t] = name
    db32 = _f32(db)
    assert np.signbit(db32[db32 == 0]).any()
    return db32, _queries(q), dict(D=D, kind=kind, queries=qk)


def negzero_heads(seed=64):
    """A -0.0 score as the head of one workgroup's list next to a +0.0 head of another, with no two heads alike otherwise: the head
    ranking of merge_sorted_lists must order them by INDEX (-0.0 == +0.0).  Ten 128-row tiles (ten lists at the default grid); tiles
    0..5 hold one positive score each, tile 6 a +0.0 row, tile 7 a -0.0 row (the higher index), everything else is negative: the
    top-8 is the six positives, the -0.0 row, the +0.0 row."""
    D, n = 64, 9 * 128 + 40
    rng = np.random.default_rng(seed)
    db = -rng.uniform(0.5, 2.0, (n, D))
    db[:, SZ_E] = 0.0
    pos = [t * 128 + 37 for t in range(6)]
    for j, r in enumerate(pos):
        db[r, 0] = 1.0 + j
    a, b = 6 * 128 + 5, 7 * 128 + 9
    db[a, 0] = 0.0
    db[b, 0] = -0.0
    db[b, SZ_E] = -2.0 ** -76
    q = rng.uniform(-1.0, 1.0, (NQ_BASE, D))
    under = np.zeros(D)
    under[0], under[SZ_E] = 1.0, 2.0 ** -76
    for t in QROWS:
        q[t] = under
    return _f32(db), _queries(q), dict(D=D, N=n, pos=pos, plus_zero=a, minus_zero=b, probes=list(QROWS))


# ------------------------------------------------------------------------------------------------------------------ all-tie
def all_tie(seed=65):
    """every row is the same vector: any query ties all rows; queries[t] for t in QROWS is the zero query (score +0.0)"""
    D = 64
    rng = np.random.default_rng(seed)
    row = rng.standard_normal(D)
    db = np.tile(row, (N, 1))
    q = rng.standard_normal((NQ_BASE, D))
    for t in QROWS[::2]:
        q[t] = 0.0
    return _f32(db), _queries(q), dict(D=D, zero=list(QROWS[::2]))


# ------------------------------------------------------------------------------------------------------------------ non-finite queries
NF_E0, NF_E1, NF_E2 = 40, 7, 33
NF_QROWS = (0, 31, 32, 63, 64, 127, 128, 255)           # every one of these tile rows carries a non-finite query


def nonfinite_queries(seed=66):
    """Finite rows; queries of kind "nan" (one NaN element), "inf1" (+inf at NF_E0: a row holding a zero there scores 0 x inf = NaN,
    a positive element +inf, a negative one -inf) and "inf2" (+inf at NF_E1, -inf at NF_E2) at every tile row of NF_QROWS (and 1, 3) among finite ones.  Rows r % 3 == 0 and
    the special rows of even rank hold the zero, the special rows of odd rank and rows 2, 5, 8, 11 a positive element, all others a
    negative one: the "inf1" list is a few +inf rows, then real rows at -inf."""
    D = 64
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((N, D))
    e0 = -np.abs(db[:, NF_E0]) - 0.01
    e0[::3] = 0.0
    e0[[2, 5, 8, 11]] = 0.7
    for j, r in enumerate(SPECIAL):
        e0[r] = 0.0 if j % 2 == 0 else 0.5 + j
    db[:, NF_E0] = e0
    q = rng.standard_normal((NQ_BASE, D))
    qk = {}
    for j, t in enumerate(NF_QROWS + (1, 3)):            # rows 2, 4, 30, 33, 62, 65, 126, 129, 254 stay finite neighbours
        name = ("nan", "inf1", "inf2")[j % 3]
        qk[t] = name
        if name == "nan":
            q[t, 5] = np.nan
        elif name == "inf1":
            q[t, NF_E0] = np.inf
        else:
            q[t, NF_E1], q[t, NF_E2] = np.inf, -np.inf
    return _f32(db), _queries(q), dict(D=D, queries=qk, plus=sorted([2, 5, 8, 11] + [r for j, r in enumerate(SPECIAL) if j % 2]))


# ------------------------------------------------------------------------------------------------------------------ cast edges
F32_OVERFLOW_BOUNDARY = (2.0 - 2.0 ** -24) * 2.0 ** 127          # halfway between FLT_MAX and 2^128: ties to even = overflow
CAST_FINITE = (                                                  # double -> what (float)x must be
    (FLT_MAX, FLT_MAX),
    (float(np.nextafter(F32_OVERFLOW_BOUNDARY, 0.0)), FLT_MAX),   # the largest double that still rounds down
    (1.5 * U, 2 * U),                                             # tie -> even
    (2.5 * U, 2 * U),                                             # tie -> even, downwards
    (0.5 * U, 0.0),                                               # exactly half -> +0.0
    (float(np.nextafter(0.5 * U, 1.0)), U),                       # just above half
    (-2.0 ** -151, -0.0),
    (-1.5 * U, -2 * U),
    (2.0 ** -127 * (1 + 2.0 ** -30), 2.0 ** -127),                # just above 2^-127: a subnormal float
    (1 + 2.0 ** -24, 1.0),                                        # halfway between two normal floats: even below
    (1 + 3 * 2.0 ** -24, 1 + 2.0 ** -22),                         # even above
    (-(1 + 2.0 ** -24), -1.0),
    (-(1 + 3 * 2.0 ** -24), -(1 + 2.0 ** -22)),
    (float(np.nextafter(2.0 ** -126, 0.0)), 2.0 ** -126),         # the largest double below FLT_MIN rounds up to a normal
)
CAST_INF = (1e300, -1e300, F32_OVERFLOW_BOUNDARY, float(np.nextafter(F32_OVERFLOW_BOUNDARY, np.inf)),
            -float(np.nextafter(F32_OVERFLOW_BOUNDARY, np.inf)))
# 8-row blocks of a tile are loaded by wave (block % waves) into an LDS image rotated by block & 3 floats: the 16-, 8- and 4-byte store
# branches of the cast loader.  SPECIAL has rotations 0 and 3 (and 1, 2 in the partial tile); rows 8, 16, 72, 80 add 1 and 2 up front.
CAST_FINITE_ROWS = SPECIAL + (8, 16)
CAST_INF_ROWS = (24, 32, 72, 80, 520)


def cast_position(i, j):
    """element of edge value i in edge row number j: over all eight 16-byte slots of a chunk, all four floats of a slot, both chunks"""
    return 4 * ((i + j) % 8) + (i % 4) + 32 * ((i // 8 + j) % 2)


def cast_edges(seed=67):
    """float64 rows.  Ordinary elements are negative, not float32-representable doubles; the probe queries 2^20 e_p (p = 0..63, at
    tile rows 64..127, negated at 128..191, and 0, 1, 3 for p = 0, 5, 34) score an ordinary row negative, so the finite edge rows -- tiny, zero or huge --
    top the list of the position that holds their edge value.  A row with a cast-to-inf element scores NaN against any probe
    of another position (0 x inf) and +-inf against its own."""
    D = 64
    rng = np.random.default_rng(seed)
    db = -np.abs(rng.standard_normal((N, D))) * 0.1 - 1e-3
    edges = {}
    for j, r in enumerate(CAST_FINITE_ROWS):
        for i, (x, _) in enumerate(CAST_FINITE):
            db[r, cast_position(i, j)] = x
        edges[r] = "finite"
    for j, r in enumerate(CAST_INF_ROWS):
        for i, x in enumerate(CAST_INF):
            db[r, cast_position(3 * i + 1, j)] = x
        edges[r] = "inf"
    q = rng.standard_normal((NQ_BASE, D))
    probes = {}
    for p in range(D):
        q[64 + p] = 0.0
        q[64 + p, p] = 2.0 ** 20
        probes[64 + p] = p
        q[128 + p] = -q[64 + p]                         # the negated probe: the negative edges on top
        probes[128 + p] = p
    for t, p in ((0, 0), (1, 5), (3, 34)):
        q[t] = q[64 + p]
        probes[t] = p
    return np.ascontiguousarray(db), _queries(q), dict(D=D, edges=edges, probes=probes)


# ------------------------------------------------------------------------------------------------------------------ the matrix
FLOAT_FAMILIES = {"overflow": overflow, "subnormal": subnormal, "signed_zero": signed_zero, "negzero_heads": negzero_heads,
                  "all_tie": all_tie, "nonfinite_queries": nonfinite_queries}
FAMILIES = dict(FLOAT_FAMILIES, cast_edges=cast_edges)


def family_prefixes(name, what):
    if name == "negzero_heads":
        n = what["N"]
        return sorted(set(prefixes(n, (0, 127, 128, 255, 256, what["plus_zero"], what["minus_zero"], 1151, 1152, n - 1))))
    if name == "cast_edges":
        return sorted(set(prefixes(N, SPECIAL + (8, 16, 24, 32, 72, 80))))
    return prefixes()
