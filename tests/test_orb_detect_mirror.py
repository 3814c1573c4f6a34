"""The numpy restatement of the ORB detector (tests/np_mirror_orb_detect.py) against itself and against hand-made events, numpy alone:
the per-pixel transcription and the vectorised form agree on every case of tests/orb_detect_cases.py, every constructed event of the
definition occurs, the quotas sum to n_features and the level sizes are those of exact rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import np_mirror_orb_detect as O
import orb_detect_cases as OC


@pytest.mark.parametrize("case", OC.all_cases(), ids=lambda c: c["name"])
def test_both_forms_agree_on_every_case(case):
    sa, sb = {}, {}
    a, ca = O.detect(case["img"], case["params"], stages=sa)
    b, cb = O.detect(case["img"], case["params"], loops=True, stages=sb)
    assert ca == cb and a.tobytes() == b.tobytes()
    for l in range(case["params"]["n_levels"]):
        assert np.array_equal(sa["images"][l], sb["images"][l]) and np.array_equal(sa["scores"][l], sb["scores"][l])
    assert sum(ca) == len(a) and all(n <= L["quota"] for n, L in zip(ca, sa["levels"]))


# ---------------------------------------------------------------------------------------------- the FAST score
def ring_image(ip: int, ring_values) -> np.ndarray:
    """7 x 7, centre ip, ring pixel k = ring_values[k], everything else ip"""
    img = np.full((7, 7), ip, np.int64)
    for (dx, dy), v in zip(O.RING, ring_values):
        img[3 + dy, 3 + dx] = v
    return img


def S_of(ip, ring_values) -> int:
    img = ring_image(ip, ring_values)
    s = O.score_pixel(img, 3, 3)
    assert O.score_plane(img)[3, 3] == s == O.score_plane_loops(img)[3, 3]
    return s


def test_isolated_pixel():
    img = OC.with_dots(65, 65, [(32, 32, 200)])
    S = O.score_plane(img)
    assert S[32, 32] == 149 and (S[3:-3, 3:-3][S[3:-3, 3:-3] != -1].size == 1)   # the ring sees 50 everywhere: min(I_p - I_k) = 150
    L = O.plan(65, 65, O.params(n_levels=1, border=16))[0]
    assert list(O.candidates(S, L, 0)) == [32 * 65 + 32] == list(O.candidates_loops(S, L, 0))
    a, bb, c = O.harris_parts(img, 32, 32)
    assert c == 0 and a == bb and a > 0
    assert O.harris_loops(img, 32, 32) == 21 * a * a == int(O.harris(img, [32 * 65 + 32])[0])


def test_straight_edge_and_the_corner_of_a_square():
    edge = OC.by_name("edge")["img"]
    S = O.score_plane(edge)
    assert (S[3:-3, 3:-3] == -1).all()                                            # either side of an edge: 7 or 9 ring pixels differ, never 9 in a row beyond 0
    sq = OC.by_name("square")["img"]
    S = O.score_plane(sq)
    for x, y in ((28, 30), (57, 30), (28, 59), (57, 59)):                         # the four corner pixels of the filled square
        assert S[y, x] == 210 - 50 - 1
    assert S[30, 40] == -1 and S[45, 40] == -1                                    # on its side, inside it


@pytest.mark.parametrize("start", (2, 11, 15))                                     # inside the index range, wrapping 15 -> 0
@pytest.mark.parametrize("sign", (+1, -1))                                        # bright, dark
def test_arc_of_eight_is_no_corner_and_of_nine_is_one(start, sign):
    for length, corner in ((8, False), (9, True)):
        ring = [100] * 16
        for j in range(length):
            ring[(start + j) % 16] = 100 + sign * 30
        s = S_of(100, ring)
        assert (s >= 0) == corner and s == (29 if corner else -1), (length, s)


def test_equal_to_the_threshold_is_not_brighter():
    t = 20
    assert S_of(100, [100 + t] * 9 + [100] * 7) == t - 1                          # I_k == I_p + t: S < t, no corner at t
    assert S_of(100, [100 + t + 1] * 9 + [100] * 7) == t                          # one more: a corner at t
    assert S_of(100, [100 - t] * 9 + [100] * 7) == t - 1
    assert S_of(0, [255] * 16) == 254 and S_of(255, [0] * 16) == 254
    assert S_of(100, [255, 0] * 8) == -101 and S_of(128, [255, 0] * 8) == -128    # no arc agrees in sign: max(-100, -155) - 1, max(-128, -127) - 1
    assert S_of(255, [255, 0] * 8) == -1 and S_of(0, [255, 0] * 8) == -1
    assert S_of(50, [50] * 16) == -1                                              # flat


def test_two_adjacent_pixels_of_equal_score_keep_nothing():
    c = OC.by_name("adjacent_equal")
    S = O.score_plane(c["img"])
    assert S[35, 34] == S[35, 35] and S[35, 34] >= 0
    L = O.plan(70, 70, c["params"])[0]
    assert len(O.candidates(S, L, 0)) == len(O.candidates_loops(S, L, 0)) == 0
    one = O.score_plane(OC.with_dots(70, 70, [(34, 35, 200), (35, 35, 199)]))    # unequal: the larger one stays
    assert list(O.candidates(one, L, 0)) == [35 * 70 + 34]


def test_detection_rectangle_one_inside_and_one_outside_each_side():
    w, h, b = 80, 72, 20
    p = O.params(n_levels=1, border=b, n_features=100)
    L = O.plan(w, h, p)[0]
    assert (L["x0"], L["y0"], L["x1"], L["y1"]) == (b, b, w - 1 - b, h - 1 - b)
    inside = [(b, 36), (w - 1 - b, 30), (40, b), (48, h - 1 - b)]
    outside = [(b - 1, 44), (w - b, 52), (56, b - 1), (32, h - b)]
    for form in (False, True):
        kp, _ = O.detect(OC.with_dots(w, h, [(x, y, 200) for x, y in inside + outside]), p, loops=form)
        assert sorted(zip(kp["x_level"].tolist(), kp["y_level"].tolist())) == sorted(inside)


def test_equal_keys_are_resolved_by_raster_index_and_quota_edges():
    img = OC.dot_grid(5, 4, border=16)                                            # 20 candidates of equal R
    for quota in (19, 20, 21, 1):                                                 # quota + 1, quota and quota - 1 candidates; n_features = 1
        for form in (False, True):
            kp, counts = O.detect(img, O.params(n_levels=1, n_features=quota, border=16), loops=form)
            assert counts[0] == len(kp) == min(quota, 20) and len(set(kp["response"].tolist())) == 1
            raster = (kp["y_level"].astype(int) * img.shape[1] + kp["x_level"]).tolist()
            want = [(16 + 8 * j) * img.shape[1] + 16 + 8 * i for j in range(4) for i in range(5)][:quota]
            assert raster == want
    assert list(O.select([5, 9, 5, 9, 5], [10, 11, 12, 13, 14], 3)) == [0, 1, 3] == list(O.select_loops([5, 9, 5, 9, 5], [10, 11, 12, 13, 14], 3))
    assert list(O.select([-7, -7, -9], [1, 2, 3], 1)) == [0]


def test_bilinear_weights_and_the_clamp_at_both_ends():
    # 2 : 1 in x: X = ((2x + 1) * 8 * 1024) // 4 - 1024 = 4096 x + 1024: x0 = 2x, a = 1024 -- the mean of two pixels, rounded half up
    src = np.array([[0, 1, 10, 13, 255, 255, 7, 8]], np.uint8)
    assert O.downsample(src, 4, 1).tolist() == [[1, 12, 255, 8]] == O.downsample_loops(src, 4, 1).tolist()
    # the same size: X = 2048 x: a = 0, the pixel itself
    img = np.random.default_rng(3).integers(0, 256, (5, 9)).astype(np.uint8)
    assert np.array_equal(O.downsample(img, 9, 5), img)
    i0, i1, a = O.axis(6, 5)                                                      # X = (2x + 1) * 6144 // 5 - 1024
    assert a.tolist() == [(((2 * x + 1) * 6144) // 5 - 1024) & 2047 for x in range(5)] and i0.tolist() == [0, 1, 2, 3, 4] and i1.tolist() == [1, 2, 3, 4, 5]
    # a = 2047 needs a destination of 1024 or more: 1024 from 1025, X = 2047 * 1025 - 1024 = 1023 * 2048 + 2047 at x = 1023
    i0, i1, a = O.axis(1025, 1024)
    assert (a[1023], i0[1023], i1[1023]) == (2047, 1023, 1024) and a[0] == 1 and i0[0] == 0
    row = np.zeros((1, 1025), np.uint8); row[0, 1024] = 255
    assert O.downsample(row, 1024, 1)[0, 1023] == (255 * 2047 * 2048 + (1 << 21)) >> 22 == O.downsample_loops(row, 1024, 1)[0, 1023] == 255
    # upsampling reaches both clamps: X < 0 at the left end, X > (n - 1) * 2048 at the right
    i0, i1, a = O.axis(2, 4)
    assert (i0.tolist(), i1.tolist(), a.tolist()) == ([0, 0, 0, 1], [1, 1, 1, 1], [0, 512, 1536, 0])
    assert O.downsample(np.array([[0, 200]], np.uint8), 4, 1).tolist() == [[0, 50, 150, 200]]


def test_patch_pixels_and_its_moments():
    """the umax table gives 31 + 2 (31 + 31 + 31 + 29 + 29 + 29 + 27 + 27 + 25 + 23 + 21 + 19 + 17 + 13 + 7) = 749 pixels (not 709)"""
    off = O.patch_offsets()
    assert O.UMAX == (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
    assert len(off) == len(set(off)) == 749 == 31 + 2 * sum(2 * u + 1 for u in O.UMAX[1:])
    flat = np.full((40, 40), 93, np.uint8)
    assert O.moments_loops(flat, 20, 20) == (0, 0)
    x = np.arange(40, dtype=np.int64)
    ramp_x = np.broadcast_to(3 * x + 10, (40, 40)).astype(np.uint8)              # I = 3 (x - 20) + 70 around (20, 20)
    sum_u2 = sum(u * u for u, _ in off)                                           # sum u = sum v = sum u v = 0 by symmetry
    assert O.moments_loops(ramp_x, 20, 19) == (3 * sum_u2, 0)
    ramp_y = np.ascontiguousarray(ramp_x.T)
    sum_v2 = sum(v * v for _, v in off)
    assert O.moments_loops(ramp_y, 18, 20) == (0, 3 * sum_v2) and sum_u2 == sum_v2 == 2 * sum(v * v * (2 * O.UMAX[v] + 1) for v in range(16))
    m10, m01 = O.moments(ramp_y + ramp_x // 3, [18, 20], [20, 19])
    assert [(int(a), int(b)) for a, b in zip(m10, m01)] == [O.moments_loops(ramp_y + ramp_x // 3, 18, 20), O.moments_loops(ramp_y + ramp_x // 3, 20, 19)]


# ---------------------------------------------------------------------------------------------- the plan
def test_quotas_sum_to_n_features():
    """for every n_features in 1 .. 16384 and n_levels in 1 .. 8; the rounded quotas alone exceed n_features in ONE case, 7 on 8 levels
    (2 + 1 + 1 + 1 + 1 + 1 + 1 = 8), which is why the definition takes the minimum with what is left"""
    bound = []
    for nl in range(1, 9):
        for nf in range(1, 16385):
            q = [L["quota"] for L in O.plan(64, 64, O.params(n_features=nf, n_levels=nl))]
            assert sum(q) == nf and min(q) >= 0, (nl, nf, q)
            rounded = [int(np.floor(x + 0.5)) for x in _nd_sequence(nf, nl)]
            if q[:-1] != rounded:
                bound.append((nl, nf, q, rounded))
    assert bound == [(8, 7, [2, 1, 1, 1, 1, 1, 0, 0], [2, 1, 1, 1, 1, 1, 1])]
    assert [L["quota"] for L in O.plan(752, 480, O.params(n_features=1))] == [0] * 7 + [1]
    assert [L["quota"] for L in O.plan(752, 480, O.params())] == [1086, 905, 754, 628, 524, 436, 364, 303]


def _nd_sequence(nf, nl):
    f = 1.0 / 1.2
    g = 1.0
    for _ in range(nl):
        g *= f
    nd = float(nf) * (1.0 - f) / (1.0 - g)
    out = []
    for _ in range(nl - 1):
        out.append(nd)
        nd *= f
    return out


def test_level_sizes_at_752_x_480_are_those_of_exact_arithmetic():
    levels = O.plan(752, 480, O.params())
    for l, L in enumerate(levels):
        s = Fraction(6, 5) ** l
        exact = [int(Fraction(n) / s + Fraction(1, 2)) for n in (752, 480)]       # floor of a positive rational
        assert [L["width"], L["height"]] == exact, l
    assert [(L["width"], L["height"]) for L in levels] == [(752, 480), (627, 400), (522, 333), (435, 278), (363, 231), (302, 193), (252, 161), (210, 134)]


def test_full_frame_fills_every_level():
    kp, counts = OC.full_frame_mirror()
    levels = O.plan(*OC.FULL, O.params())
    assert len(kp) == 5000 and counts == [L["quota"] for L in levels] and all(L["x1"] >= L["x0"] for L in levels)
    assert (np.diff(kp["level"].astype(int)) >= 0).all()
