"""The NetVLAD pooling (include/cerebro_hip.h "NetVLAD pooling") restated in Python: the definition the device is compared against,
bit for bit.

    s[n][k] = dot_tree_f32(x[n], Wt[k]) + bias[k]                        k < K+G
    m = max_k s[n][k];  e_k = vlad_exp(s[n][k] - m);  Z = ((0 + e_0) + e_1) + ...;  a[n][k] = e_k / Z
    P_j[k][c] = chain over the 64 positions of block j of  acc + (a[n][k] * x[n][c]);  S_j[k] likewise of a[n][k]      k < K
    V = chain over j of P_j;  A = chain over j of S_j;  Wv = V + (A * centres)
    U[k] = Wv[k] / sqrt(max'(dot_tree_f64(Wv[k], Wv[k]), 1e-12));  v = float32(U / sqrt(max'(dot_tree_f64(U, U), 1e-12)))

Two forms.  `vlad_exact` does every operation on Fractions with ONE correctly rounded conversion each (the fused multiply-adds of the
trees through np_mirror_project.fma) and is what tiny shapes are checked with; `vlad` is vectorised numpy -- every step a single IEEE
operation, so numpy is exact here -- with the trees through the oracle's pinned dot products.  tests/test_vlad_mirror.py holds the two
against each other.  `block` and `fused` select orders the definition is NOT (one plain chain; fma in the aggregation): the mirror test
uses them to show that the test data tells them apart."""
import ctypes
import math
from fractions import Fraction

import numpy as np

import oracle_lib
from np_mirror_project import dot_tree_exact

BLOCK = 64
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
COEF = [1.0 / float(math.factorial(i)) for i in range(14)]
EPS = 1e-12


# ---------------------------------------------------------------------------------------------- the exact form
def _rn(fr: Fraction) -> float:
    return float(fr)            # one correctly rounded conversion (an exact zero is +0: no step of the definition produces -0)


def _mul(a, b):
    return _rn(Fraction(a) * Fraction(b))


def _add(a, b):
    return _rn(Fraction(a) + Fraction(b))


def _sub(a, b):
    return _rn(Fraction(a) - Fraction(b))


def _div(a, b):
    return _rn(Fraction(a) / Fraction(b))


def _sqrt(q: float) -> float:
    """the correctly rounded square root, checked exactly: r is the double nearest sqrt(q) iff q lies between the squares of the
    midpoints to r's neighbours"""
    r = math.sqrt(q)
    lo, hi = (Fraction(r) + Fraction(math.nextafter(r, 0.0))) / 2, (Fraction(r) + Fraction(math.nextafter(r, math.inf))) / 2
    assert lo * lo <= Fraction(q) <= hi * hi
    return r


def vlad_exp_exact(t: float) -> float:
    if t < -700.0:
        return 0.0
    kf = float(round(_mul(t, LOG2E)))          # Python's round() of a float: ties to even
    r = _sub(_sub(t, _mul(kf, LN2_HI)), _mul(kf, LN2_LO))
    p = COEF[13]
    for i in range(12, -1, -1):
        p = _add(_mul(p, r), COEF[i])
    return _rn(Fraction(p) * Fraction(2) ** int(kf))     # exact: the result is normal


def vlad_exact(x, Wt, bias, centres):
    """-> dict(s, a, V, A, U, v) of one map x (N, C); K = centres.shape[0], the other rows of Wt are ghosts.  Tiny shapes only."""
    x, Wt, bias, centres = (np.asarray(t, dtype=np.float32) for t in (x, Wt, bias, centres))
    N, C = x.shape
    KG, K = Wt.shape[0], centres.shape[0]
    xd, wd = x.astype(np.float64), Wt.astype(np.float64)
    s = np.empty((N, KG))
    a = np.empty((N, KG))
    for n in range(N):
        for k in range(KG):
            s[n, k] = _add(dot_tree_exact(xd[n], wd[k], 4), float(bias[k]))
        m = s[n, 0]
        for k in range(1, KG):
            if s[n, k] > m:
                m = s[n, k]
        e = [vlad_exp_exact(_sub(s[n, k], m)) for k in range(KG)]
        Z = 0.0
        for k in range(KG):
            Z = _add(Z, e[k])
        for k in range(KG):
            a[n, k] = _div(e[k], Z)
    V = np.zeros((K, C))
    A = np.zeros(K)
    for n0 in range(0, N, BLOCK):
        blk = range(n0, min(n0 + BLOCK, N))
        for k in range(K):
            S = 0.0
            for n in blk:
                S = _add(S, a[n, k])
            A[k] = _add(A[k], S)
            for c in range(C):
                P = 0.0
                for n in blk:
                    P = _add(P, _mul(a[n, k], xd[n, c]))
                V[k, c] = _add(V[k, c], P)
    U = np.empty((K, C))
    for k in range(K):
        w = [_add(V[k, c], _mul(A[k], float(centres[k, c]))) for c in range(C)]
        q = dot_tree_exact(w, w, 2)
        r = _sqrt(q if q > EPS else EPS)
        U[k] = [_div(wc, r) for wc in w]
    u = U.ravel()
    q = dot_tree_exact(u, u, 2)
    r = _sqrt(q if q > EPS else EPS)
    v = np.array([_div(e, r) for e in u]).astype(np.float32)        # float64 -> float32: round to nearest even
    return dict(s=s, a=a, V=V, A=A, U=U, v=v)


# ---------------------------------------------------------------------------------------------- the fast form
def vlad_exp(t) -> np.ndarray:
    t = np.asarray(t, dtype=np.float64)
    small = t < -700.0
    tt = np.where(small, 0.0, t)
    kf = np.rint(tt * LOG2E)
    r = (tt - kf * LN2_HI) - kf * LN2_LO
    p = np.full_like(tt, COEF[13])
    for i in range(12, -1, -1):
        p = p * r + COEF[i]
    scale = ((1023 + kf.astype(np.int64)) << 52).view(np.float64)
    return np.where(small, 0.0, p * scale)


def scores(x, Wt, bias, nthreads: int = 8) -> np.ndarray:
    """s (N, K+G): the oracle's float-row tree (the products commute, so the map may play the DB)"""
    x, Wt = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(Wt, dtype=np.float32)
    s = np.empty((x.shape[0], Wt.shape[0]))
    for k in range(Wt.shape[0]):
        s[:, k] = oracle_lib.scores(x, x.shape[0], Wt[k], nthreads=nthreads)
    return s + np.asarray(bias, dtype=np.float32).astype(np.float64)[None, :]


def softmax(s) -> np.ndarray:
    m = s.max(axis=1)                  # as a value the maximum does not depend on the order of the walk
    e = vlad_exp(s - m[:, None])
    Z = np.zeros(s.shape[0])
    for k in range(s.shape[1]):
        Z = Z + e[:, k]
    return e / Z[:, None]


_libm = None


def _fma(a, b, c):
    """elementwise fma(a, b, c) through libm: for the fused variant only (NOT the definition)"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        _libm.fma.restype = ctypes.c_double
        _libm.fma.argtypes = [ctypes.c_double] * 3
    a, b, c = np.broadcast_arrays(a, b, c)
    return np.array([_libm.fma(p, q, r) for p, q, r in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())]).reshape(a.shape)


def aggregate(a, x, K, block: int = BLOCK, fused: bool = False):
    """-> (V (K, C), A (K,)): blocks of `block` positions (the definition: 64), chains ascending"""
    N, C = x.shape
    xd = x.astype(np.float64)
    V, A = np.zeros((K, C)), np.zeros(K)
    for n0 in range(0, N, block):
        P, S = np.zeros((K, C)), np.zeros(K)
        for n in range(n0, min(n0 + block, N)):
            ak = a[n, :K]
            P = _fma(ak[:, None], xd[n][None, :], P) if fused else P + ak[:, None] * xd[n][None, :]
            S = S + ak
        V = V + P
        A = A + S
    return V, A


def vlad(x, Wt, bias, centres, block: int = BLOCK, fused: bool = False, nthreads: int = 8):
    """-> dict(s, a, V, A, U, v) of one map x (N, C): the fast form"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    centres = np.asarray(centres, dtype=np.float32)
    K = centres.shape[0]
    with np.errstate(all="ignore"):
        s = scores(x, Wt, bias, nthreads)
        a = softmax(s)
        V, A = aggregate(a, x, K, block, fused)
        Wv = V + A[:, None] * centres.astype(np.float64)
        q = np.array([oracle_lib.dot_tree_f64(Wv[k], Wv[k]) for k in range(K)])
        U = Wv / np.sqrt(np.where(q > EPS, q, EPS))[:, None]
        u = np.ascontiguousarray(U.ravel())
        qq = np.float64(oracle_lib.dot_tree_f64(u, u))
        v = (u / np.sqrt(qq if qq > EPS else np.float64(EPS))).astype(np.float32)
    return dict(s=s, a=a, V=V, A=A, U=U, v=v)


def keras_layer_f64(x, Wt, bias, centres) -> np.ndarray:
    """A straightforward float64 numpy evaluation of the Keras layer (predict_utils.py NetVLADLayer.call): np.exp softmax over all K+G
    clusters, sum over positions of a * (x + C) for the kept ones, l2_normalize per cluster and of the flattening -> float64 (K*C,)"""
    x, Wt, bias, centres = (np.asarray(t, dtype=np.float64) for t in (x, Wt, bias, centres))
    K = centres.shape[0]
    s = x @ Wt.T + bias
    e = np.exp(s - s.max(axis=1, keepdims=True))
    a = (e / e.sum(axis=1, keepdims=True))[:, :K]
    W = (a[:, :, None] * (x[:, None, :] + centres[None, :, :])).sum(axis=0)
    W = W / np.sqrt(np.maximum((W * W).sum(axis=1, keepdims=True), EPS))
    w = W.ravel()
    return w / np.sqrt(max(float((w * w).sum()), EPS))


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(np.array_equal(a.view(u), b.view(u)))


def first_difference(a, b):
    """index, got, want of the first element whose bits differ (for a failing test's message)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    d = np.flatnonzero(a.view(u).ravel() != b.view(u).ravel())
    return None if d.size == 0 else (int(d[0]), a.ravel()[d[0]].hex() if a.dtype == np.float64 else float(a.ravel()[d[0]]),
                                     b.ravel()[d[0]].hex() if b.dtype == np.float64 else float(b.ravel()[d[0]]), int(d.size))
