"""CPU checks of tests/ingest_cases.py, the references of tests/test_ingest_edges_gpu.py: the value table of the narrowing check against an
independent rule (exact rational arithmetic against the float32 neighbours, struct for the bits), and the norm bound's two inequalities and
its summation order."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import ingest_cases as IC
import oracle_lib

FLT_MAX = Fraction(2 ** 24 - 1) * Fraction(2) ** 104
DS = (4, 260, 1028, 4096, 10240)


# ---------------------------------------------------------------------------------------------- the independent rule
def f32_of_bits(b: int) -> Fraction:
    """the value of a finite non-negative float32 from its bits, as a rational"""
    e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    assert e != 0xFF
    return Fraction(m, 1 << 149) if e == 0 else Fraction((1 << 23) | m) * Fraction(2) ** (e - 150)


def round_by_rule(x: float):
    """(class, float32 bits) of a finite double, by the rule itself: find the float32 neighbours lo <= |x| <= hi by bisection over the
    bit patterns (which are ordered like the values), take the nearer, on a tie the one whose last bit is 0; 0x7f800000 (Inf, the 'float'
    2^128 as far as rounding goes) may win"""
    sign = 0x80000000 if math.copysign(1.0, x) < 0 else 0
    a = abs(Fraction(x))
    val = lambda b: Fraction(2) ** 128 if b == 0x7F800000 else f32_of_bits(b)
    lo, hi = 0, 0x7F800000
    if a >= val(hi):
        return IC.OVERFLOW, sign | hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if val(mid) <= a:
            lo = mid
        else:
            hi = mid
    if val(lo) == a:
        return IC.EXACT, sign | lo
    dl, dh = a - val(lo), val(hi) - a
    b = lo if dl < dh else hi if dh < dl else (lo if lo % 2 == 0 else hi)
    return (IC.OVERFLOW if b == 0x7F800000 else IC.INEXACT), sign | b


def test_table_holds_the_named_values():
    have = {(IC.f64_bits(x), c) for x, c in IC.TABLE}
    named = {
        IC.EXACT: [0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 1 + 2.0 ** -23, float(np.finfo(np.float32).max), float(np.float32(0.1))],
        IC.INEXACT: [0.1, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -52, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -52), 1.5 * 2.0 ** -149, 5e-324,
                     float(np.finfo(np.float32).max) + 2.0 ** 102, math.nextafter(float.fromhex("0x1.ffffffp+127"), 0.0)],
        IC.OVERFLOW: [float.fromhex("0x1.ffffffp+127"), 2.0 ** 128, 1e39, float(np.finfo(np.float64).max)],
        IC.NONFINITE: [math.inf, -math.inf],
    }
    for cls, xs in named.items():
        for x in xs:
            assert (IC.f64_bits(x), cls) in have, (x.hex(), cls)
            if cls != IC.NONFINITE and x != 0:
                assert (IC.f64_bits(-x), cls) in have, (x.hex(), cls)
    nans = [x for x, c in IC.TABLE if x != x]
    assert all(c == IC.NONFINITE for x, c in IC.TABLE if x != x)
    bits = [IC.f64_bits(x) for x in nans]
    assert any(b >> 63 == 0 and b & ((1 << 51) - 1) == 0 for b in bits)          # a plain quiet NaN
    assert any(b >> 63 == 1 and b & ((1 << 51) - 1) != 0 for b in bits)          # sign bit and payload


def test_table_against_the_rule():
    for x, cls in IC.TABLE:
        assert IC.classify(x) == cls, (x.hex() if x == x else "nan", cls)
        if cls == IC.NONFINITE:
            continue
        want_cls, want_bits = round_by_rule(x)
        assert want_cls == cls, (x.hex(), cls, want_cls)
        got = struct.unpack("<I", struct.pack("<f", IC.stored([x])[0]))[0]
        assert got == want_bits == IC.stored_bits(x), (x.hex(), hex(got), hex(want_bits))
    # the cases that are there for a reason, by name
    sb = IC.stored_bits
    assert sb(-0.0) == 0x80000000 and sb(0.0) == 0
    assert sb(1 + 2.0 ** -24) == 0x3F800000 and sb(float.fromhex("0x1.0000010000001p+0")) == 0x3F800001           # the tie down, just above it up
    assert sb(2.0 ** -150) == 0 and sb(-(2.0 ** -150)) == 0x80000000 and sb(float.fromhex("0x1.0000000000001p-150")) == 1
    assert sb(1.5 * 2.0 ** -149) == 2 and sb(5e-324) == 0 and sb(-5e-324) == 0x80000000
    assert sb(float.fromhex("0x1.fffffefffffffp+127")) == 0x7F7FFFFF and sb(float.fromhex("0x1.ffffffp+127")) == 0x7F800000
    assert sb(-1e39) == 0xFF800000


def rows_at_scales(D, n=50):
    rng = np.random.default_rng(D)
    scales = 10.0 ** rng.uniform(-20, 17, n)
    rows = np.stack([(rng.standard_normal(D) * s).astype(np.float32) for s in scales])
    assert np.isfinite(rows).all()
    return rows


@pytest.mark.parametrize("D", DS)
def test_norm_bits_is_the_oracle_tree_and_the_bound_holds(D):
    rows = rows_at_scales(D)
    bulk = IC.norm_bits_rows(rows)
    worst = 0.0
    for i, (r, ss) in enumerate(zip(rows, bulk)):
        assert IC.norm_bits(r).hex() == float(ss).hex()                         # the oracle's tree == the numpy statement of it, D % 256 != 0 and D = 4
        if i < 10 or D <= 1028:                                                 # the rational sum is the slow part
            true_ss = sum(Fraction(v) ** 2 for v in r.astype(np.float64).tolist())
            worst = max(worst, abs(Fraction(float(ss)) - true_ss) / true_ss)
        N, exact = IC.norm_of(float(ss)), IC.norm_exact(r)
        assert exact <= N <= exact * IC.TIGHT, (D, exact.hex(), N.hex())
    assert worst < 46 * Fraction(1, 2 ** 53), float(worst)


@pytest.mark.parametrize("D", DS)
def test_norm_edges(D):
    """the rows the device tests plant: weight in the last element, the last 4-group, all-subnormal, one FLT_MAX, all zero"""
    last = np.zeros(D, np.float32); last[D - 1] = 3.0
    group = np.zeros(D, np.float32); group[D - 4:] = (1.0, -2.0, 0.5, 4.0)
    tiny = np.full(D, 2.0 ** -149, np.float32)
    huge = IC.f32_rows(1, D, 3)[0]; huge[D // 2] = np.finfo(np.float32).max
    for r in (last, group, tiny, huge):
        ss = IC.norm_bits(r)
        assert ss == float(IC.norm_bits_rows(r[None, :])[0]) and math.isfinite(ss) and ss > 0
        assert IC.norm_exact(r) <= IC.norm_of(ss) <= IC.norm_exact(r) * IC.TIGHT
    assert IC.norm_bits(last) == 9.0 and IC.norm_exact(last) == 3.0
    assert IC.norm_bits(tiny) == D * 2.0 ** -298                                # exact: a power of two times D
    assert IC.norm_bits(np.zeros(D, np.float32)) == 0.0 and IC.norm_of(0.0) == 0.0


def test_norm_bits_follows_the_tree_order():
    """one element of 2^27 and 1023 of 1: every lane's chain holds 4 (lane 0: 2^54 + 3, rounded), the tree adds 4-multiples to 2^54 --
    representable steps -- while a running sum from the large element on loses every single 1 to rounding"""
    D = 1024
    r = np.ones(D, np.float32)
    r[0] = 2.0 ** 27
    tree = IC.norm_bits(r)
    assert tree == float(IC.norm_bits_rows(r[None, :])[0])
    seq = 0.0
    for v in r.astype(np.float64).tolist():
        seq += v * v
    assert seq == 2.0 ** 54                                                     # 2^54 + 1 rounds back to 2^54 (ulp 4), 1023 times
    # the tree: lanes 1 .. 63 hold 16 each (4 chunks x 4), lane 0 holds 2^54 (its fifteen 1s are lost one by one)
    assert tree == 2.0 ** 54 + 63 * 16 and tree != seq
    assert math.fsum((r.astype(np.float64) ** 2).tolist()) == 2.0 ** 54 + 1024  # the truth (1023 rounds to even, ulp 4)
    assert IC.norm_exact(r) <= IC.norm_of(tree)
