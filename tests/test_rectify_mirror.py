"""The numpy restatement of the rectification (tests/np_mirror_rectify.py) against exact rational arithmetic and against what a remap
must do in the cases anyone can work out by hand.  No GPU, no library.  The definition is this project's own (include/cerebro_hip.h)
and is not pinned against OpenCV."""
from fractions import Fraction
from math import floor, isinf, isnan

import numpy as np

import np_mirror_rectify as R
import rectify_cases as RC


def exact_q(m: float) -> int:
    """Q in rational arithmetic: 32 * clamp(m) rounded to the nearest integer, ties to even"""
    if isnan(m):
        return -64
    c = Fraction(-2) if m < -2 or (isinf(m) and m < 0) else Fraction(32768) if m > 32768 else Fraction(m)
    p = 32 * c
    lo = floor(p)
    if p - lo != Fraction(1, 2):
        return floor(p + Fraction(1, 2))
    return lo if lo % 2 == 0 else lo + 1


def exact_value(img, qx: int, qy: int) -> Fraction:
    """the bilinear value at (qx / 32, qy / 32) of an image (a grid of ints or Fractions) continued with 0"""
    h, w = len(img), len(img[0])
    at = lambda y, x: Fraction(img[y][x]) if 0 <= y < h and 0 <= x < w else Fraction(0)
    x0, y0 = qx // 32, qy // 32                                       # floor division: the arithmetic shift
    a, b = Fraction(qx - 32 * x0, 32), Fraction(qy - 32 * y0, 32)
    return at(y0, x0) * (1 - a) * (1 - b) + at(y0, x0 + 1) * a * (1 - b) + at(y0 + 1, x0) * (1 - a) * b + at(y0 + 1, x0 + 1) * a * b


def exact_remap(img, qx, qy, rounded=True):
    out = [[exact_value(img, int(qx[y][x]), int(qy[y][x])) for x in range(qx.shape[1])] for y in range(qx.shape[0])]
    return [[floor(v + Fraction(1, 2)) for v in row] for row in out] if rounded else out


def test_quantiser_equals_rational_arithmetic_on_the_edge_list():
    e = RC.quantiser_edges()
    got = R.quantize(e)
    assert got.dtype == np.int32 and [int(v) for v in got] == [exact_q(float(v)) for v in e]
    q = lambda v: int(R.quantize(np.float32(v)))
    assert q(float("nan")) == -64 and q(float("inf")) == 32 * 32768 and q(float("-inf")) == -64 and q(-0.0) == 0 and q(1e30) == 1 << 20
    assert q(3.015625) == 96 and q(3.046875) == 98                   # ties go to even
    assert q(-2.0) == -64 and q(np.nextafter(np.float32(-2), np.float32(0))) == -64 and q(-1.984375) == -64 and q(-1.953125) == -62
    # a coordinate at a clamp has every tap outside any supported image
    assert (-64 >> 5, -64 & 31) == (-2, 0) and (1 << 20) >> 5 == 32768


def test_sample_equals_floor_of_exact_plus_half_on_the_edge_sets():
    w, h = 13, 9
    img = RC.image(w, h)
    for mx, my in (RC.tap_edges(w, h), RC.random_map(w, h, 5), RC.family("sixty_fourth", w, h), RC.radtan(w, h)):
        qx, qy = R.quantize(mx), R.quantize(my)
        assert R.sample(img, qx, qy).tolist() == exact_remap(img.tolist(), qx, qy)
    img, mx, my, n = RC.half_case()
    qx, qy = R.quantize(mx), R.quantize(my)
    assert (R.weighted_sum(img, qx, qy)[0, :n] % 1024 == 512).all()  # every block sits exactly on a half ...
    assert R.sample(img, qx, qy).tolist() == exact_remap(img.tolist(), qx, qy)
    want = [(p00 * (32 - a) * (32 - b) + p01 * a * (32 - b) + p10 * (32 - a) * b + p11 * a * b + 512) // 1024 for p00, p01, p10, p11, a, b in RC.HALF_BLOCKS]
    assert R.remap(img, mx, my)[0, :n].tolist() == want and want[0] == 1   # ... and rounds up: taps (0, 1) at a = 16 give 1


def test_identity_returns_the_image_and_an_integer_shift_is_a_shift_with_a_zero_border():
    for w, h in ((1, 1), (5, 1), (3, 2), (37, 11)):
        img = RC.image(w, h)
        assert np.array_equal(R.remap(img, *RC.identity(w, h)), img)
    img = RC.image(37, 11)
    for dx, dy in ((3, -2), (-5, 1), (0, 11), (37, 0), (-36, -10)):
        want = np.zeros_like(img)
        ys, xs = np.mgrid[0:11, 0:37]
        ok = (xs + dx >= 0) & (xs + dx < 37) & (ys + dy >= 0) & (ys + dy < 11)
        want[ok] = img[(ys + dy)[ok], (xs + dx)[ok]]
        assert np.array_equal(R.remap(img, *RC.shift(37, 11, dx, dy)), want), (dx, dy)


def test_two_stages_are_two_one_stage_passes():
    w, h = 41, 23
    raw = RC.image(w, h)
    for s1, s2 in ((RC.radtan(w, h), RC.rotation(w, h)), (RC.random_map(w, h, 1), RC.random_map(w, h, 2)), (RC.tap_edges(w, h), RC.tap_edges(w, h))):
        u = R.rectify(raw, *s1)
        assert u.dtype == np.uint8 and np.array_equal(u, R.remap(raw, *s1))
        assert np.array_equal(R.rectify(raw, *s1, *s2), R.remap(u, *s2))


def test_a_u_value_on_a_half_distinguishes_rounded_from_unrounded_u():
    c = RC.half_u_case()
    q1, q2 = [R.quantize(m) for m in c["s1"]], [R.quantize(m) for m in c["s2"]]
    u_exact = exact_remap(c["raw"].tolist(), *q1, rounded=False)
    y, x = c["at"]
    assert u_exact[y][x] == Fraction(1, 2) and R.remap(c["raw"], *c["s1"])[y, x] == 1
    unrounded = exact_remap(u_exact, *q2)                            # what a kernel that kept U exact would give
    got = R.rectify(c["raw"], *c["s1"], *c["s2"])
    assert got.tolist() == exact_remap(exact_remap(c["raw"].tolist(), *q1), *q2)
    assert got[y, x] == c["rounded"] == 1 and unrounded[y][x] == c["unrounded"] == 0


def test_a_hand_worked_3_x_2_example():
    img = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    mx = np.array([[0.5, 1.25, 2.5], [-0.5, 1.0, 2.0]], np.float32)
    my = np.array([[0.0, 0.5, 0.0], [1.0, 0.75, 1.5]], np.float32)
    # (0,0): halfway between 10 and 20                                  = 15
    # (0,1): x 1.25, y 0.5: row 0 gives 22.5, row 1 gives 52.5, mean    = 37.5 -> 38
    # (0,2): x 2.5 on row 0: 30 and the border 0                        = 15
    # (1,0): x -0.5 on row 1: the border 0 and 40                       = 20
    # (1,1): x 1, y 0.75: 0.25 * 20 + 0.75 * 50                         = 42.5 -> 43
    # (1,2): x 2, y 1.5: 60 and the border below, halves                = 30
    assert R.quantize(mx).tolist() == [[16, 40, 80], [-16, 32, 64]] and R.quantize(my).tolist() == [[0, 16, 0], [32, 24, 48]]
    assert R.remap(img, mx, my).tolist() == [[15, 38, 15], [20, 43, 30]]
