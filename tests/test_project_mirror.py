"""The restatement of the descriptor projection (tests/np_mirror_project.py) checked against itself and against exact arithmetic, on
the CPU: its two forms agree bit for bit; y lies within the standard error bound of the exact rational value; and the test data
tells summation orders apart, so that "equal bits" on the GPU means the defined order and no other."""
from fractions import Fraction

import numpy as np
import pytest

import np_mirror_project as M
import oracle_lib

U = Fraction(1, 2 ** 53)          # unit roundoff of fp64


def data(in_dim, D, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(in_dim).astype(np.float32)
    Mt = rng.standard_normal((D, in_dim)).astype(np.float32).astype(dtype) if dtype == np.float32 else rng.standard_normal((D, in_dim))
    b = rng.standard_normal(D)
    return x, Mt, b


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [4, 68, 256])             # 4: the smallest D chip_create takes
@pytest.mark.parametrize("in_dim", [256, 512, 768])
def test_the_two_forms_agree_and_lie_within_the_bound(in_dim, D, dtype):
    x, Mt, b = data(in_dim, D, dtype, 1000 * in_dim + D)
    if dtype == np.float64:
        assert (Mt.astype(np.float32).astype(np.float64) != Mt).mean() > 0.9      # genuinely double values
    y0, z0 = M.project_exact(x, Mt, None)
    y1, z1 = M.project_exact(x, Mt, b)
    for bias, (ye, ze) in ((None, (y0, z0)), (b, (y1, z1))):
        yf, zf = M.project(x, Mt, bias)
        assert M.same_bits(ye, yf) and M.same_bits(ze, zf), (in_dim, D, dtype, bias is not None)
        assert abs(float(np.dot(zf, zf)) - 1.0) < 1e-12
    # |y - exact| <= gamma_n * sum |x_i m_ij| (+ |b_j|) + ulp(y), n = in_dim + 8: at most in_dim / 64 roundings in a lane's chain, six in
    # the butterfly, one for the bias -- in_dim + 8 covers every order of in_dim terms (Higham, Accuracy and Stability, 3.1) -- and one
    # ulp for the final rounding being counted against the computed value
    n = in_dim + 8
    gamma = n * U / (1 - n * U)
    for j in range(0, D, max(1, D // 16)):
        exact = M.exact_dot(x, Mt[j])
        mag = sum((abs(Fraction(float(a)) * Fraction(float(m))) for a, m in zip(x, Mt[j])), Fraction(0))
        for y, eb, mb in ((y0, Fraction(0), Fraction(0)), (y1, Fraction(float(b[j])), abs(Fraction(float(b[j]))))):
            ulp = Fraction(float(np.spacing(abs(y[j]))))
            assert abs(Fraction(float(y[j])) - (exact + eb)) <= gamma * (mag + mb) + ulp, (in_dim, D, j)


def test_the_data_tells_summation_orders_apart():
    """in_dim 256, float32 normal data, 200 outputs: the defined order against a plain ascending chain, and the float-type order against
    the double-type order on the same (widened) values.  Measured here: 162 and more of 200 differ; half is demanded."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal(256).astype(np.float32)
    Mt = rng.standard_normal((200, 256)).astype(np.float32)
    xd, Md = x.astype(np.float64), Mt.astype(np.float64)
    tree32 = np.array([oracle_lib.dot_tree(x, Mt[j]) for j in range(200)])
    tree64 = np.array([oracle_lib.dot_tree_f64(xd, Md[j]) for j in range(200)])
    lib = oracle_lib.load()
    chain = np.array([lib.orc_dot_seq_f64(oracle_lib._p(xd), oracle_lib._p(np.ascontiguousarray(Md[j])), 256) for j in range(200)])
    assert M.same_bits(chain[:8], [M.chain_dot(xd, Md[j], fused=False) for j in range(8)])      # (the products are exact: fused or not)
    assert M.same_bits(chain[:8], [M.chain_dot(xd, Md[j], fused=True) for j in range(8)])
    assert (tree32 != chain).sum() >= 100, (tree32 != chain).sum()
    assert (tree32 != tree64).sum() >= 100, (tree32 != tree64).sum()
    assert (tree64 != chain).sum() >= 100, (tree64 != chain).sum()
    # and on genuinely double data the fused chain is not the unfused one: the fma's single rounding is part of the definition
    Mg = rng.standard_normal((40, 256))
    fused = [M.chain_dot(xd, Mg[j], fused=True) for j in range(40)]
    plain = [M.chain_dot(xd, Mg[j], fused=False) for j in range(40)]
    assert sum(a != b for a, b in zip(fused, plain)) >= 20


def test_fma_is_correctly_rounded_where_multiply_then_add_is_not():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30          # a * b = 1 - 2^-60 exactly: rounds to 1.0, so a * b - 1 gives 0 unfused
    assert a * b - 1.0 == 0.0 and M.fma(a, b, -1.0) == -(2.0 ** -60)
    assert M.fma(0.0, -1.0, 0.0) == 0.0 and not np.signbit(M.fma(0.0, -1.0, 0.0))
    assert np.isnan(M.fma(np.inf, 0.0, 1.0)) and M.fma(np.inf, 1.0, 1.0) == np.inf


def test_nothing_is_special_cased():
    x, Mt, b = data(256, 4, np.float32, 3)
    with np.errstate(all="ignore"):
        y, z = M.project(np.zeros(256, np.float32), Mt, None)
        assert (y == 0).all() and np.isnan(z).all()                                  # r == 0
        y, z = M.project(np.zeros(256, np.float32), Mt, b)
        assert M.same_bits(y, b) and np.isfinite(z).all()                            # a pure-bias row
        xn = x.copy(); xn[17] = np.nan
        assert np.isnan(M.project(xn, Mt, b)[1]).all()
