"""The descriptor projection (include/cerebro_hip.h "descriptor projection") restated in plain Python and numpy: the definition the
device is compared against, bit for bit.

    t_j = dot_tree(x, Mt[j])      float matrix: lane L accumulates elements k*256 + 4L + c, the products exact in fp64
                                  double matrix: elements k*128 + 2L + c of (double)x, ONE fused multiply-add per term
                                  then the xor butterfly acc[L] += acc[L ^ m], m = 32 .. 1
    y_j = t_j + b_j               (b None: y_j = t_j)
    s = dot_tree_f64(y, y), r = sqrt(s), z_j = y_j / r

Two forms: `project_exact` does every fused multiply-add as float(Fraction(a) * Fraction(b) + Fraction(c)) -- exact, then ONE
correctly rounded conversion -- and is what small shapes are checked with; `project` goes through the oracle's pinned dot products
(tests/oracle_lib.py orc_dot_tree_*) for the large ones.  tests/test_project_mirror.py holds the two against each other."""
from fractions import Fraction

import numpy as np

import oracle_lib


def fma(a, b, c) -> float:
    """a * b + c with one rounding.  Non-finite operands take numpy's a * b + c: no rounding question arises there."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:      # an exact zero sum keeps IEEE's sign: +0 unless both addends are -0
        return -0.0 if (np.signbit(a) != np.signbit(b)) and np.signbit(c) else 0.0
    return float(r)


def _butterfly(acc):
    acc = list(acc)
    for m in (32, 16, 8, 4, 2, 1):
        acc = [float(np.float64(acc[L]) + np.float64(acc[L ^ m])) for L in range(64)]
    return acc[0]


def dot_tree_exact(q, row, per_lane: int) -> float:
    """per_lane 4: the float-row order (chunks of 256), 2: the double-row order (chunks of 128); q, row: equal-length sequences"""
    n = len(q)
    acc = [0.0] * 64
    with np.errstate(all="ignore"):
        for base in range(0, n, 64 * per_lane):
            for L in range(64):
                for c in range(per_lane):
                    e = base + per_lane * L + c
                    if e < n:
                        acc[L] = fma(q[e], row[e], acc[L])
        return _butterfly(acc)


def project_exact(x, Mt, bias=None):
    """-> (y, z) of ONE raw descriptor, every step restated; Mt's dtype (float32 / float64) is the matrix type"""
    x = np.asarray(x, dtype=np.float32)
    Mt = np.asarray(Mt)
    assert Mt.dtype in (np.float32, np.float64) and Mt.shape[1] == x.size
    per_lane = 4 if Mt.dtype == np.float32 else 2
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        y = np.array([dot_tree_exact(xd, Mt[j].astype(np.float64), per_lane) for j in range(Mt.shape[0])], dtype=np.float64)
        if bias is not None:
            y = y + np.asarray(bias, dtype=np.float64)
        s = dot_tree_exact(y, y, 2)
        return y, y / np.sqrt(np.float64(s))


def project(x, Mt, bias=None, nthreads: int = 8):
    """-> (y, z) for x of shape (in_dim,) or (n, in_dim): the fast form, through the oracle's dot products"""
    Mt = np.ascontiguousarray(Mt)
    assert Mt.dtype in (np.float32, np.float64)
    X = np.ascontiguousarray(x, dtype=np.float32)
    one = X.ndim == 1
    X = X.reshape(-1, Mt.shape[1])
    Y = np.empty((X.shape[0], Mt.shape[0]), dtype=np.float64)
    Z = np.empty_like(Y)
    with np.errstate(all="ignore"):
        for i in range(X.shape[0]):
            y = oracle_lib.scores(Mt, Mt.shape[0], X[i].astype(Mt.dtype), nthreads=nthreads)   # float32 -> float64 is exact
            if bias is not None:
                y = y + np.asarray(bias, dtype=np.float64)
            Y[i] = y
            Z[i] = y / np.sqrt(np.float64(oracle_lib.dot_tree_f64(y, y)))
    return (Y[0], Z[0]) if one else (Y, Z)


def exact_dot(x, row) -> Fraction:
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, row)), Fraction(0))


def chain_dot(x, row, fused: bool) -> float:
    """a plain ascending chain: acc = acc + x[e] * row[e] (fused: one rounding per term) -- an order the definition is NOT"""
    acc = 0.0
    for a, b in zip(x, row):
        acc = fma(a, b, acc) if fused else float(np.float64(acc) + np.float64(float(a)) * np.float64(float(b)))
    return acc


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
