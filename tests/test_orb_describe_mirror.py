"""The numpy restatement of the ORB descriptor (tests/np_mirror_orb_describe.py) against the figures its definition states in
include/cerebro_hip.h, its two forms against each other, and the property the construction is for: an image turned by a quarter turn
gives the same descriptors.  numpy alone, no library, no device."""
import hashlib
import math

import numpy as np
import pytest

import np_mirror_orb_describe as D
import orb_describe_cases as DC
import orb_detect_cases as OC

PATTERN_SHA = "0a170a01e941c47e3dc21a502fbec04104b548ddedf269114180a0504526a179"
STEERED_SHA = "489d64ba52aef79c6fa46391b51cc6fe2e3764aa946f9283360aca763ba5969f"
MAX_KEYPOINTS = 16384                             # CHIP_MATCH_MAX_KEYPOINTS: a quota above every candidate count here
M_MAX = 2_900_000                                 # above the largest moment of a patch: 255 * sum |u| over the 749 pixels < 2^22


# ---------------------------------------------------------------------------------------------- the tables
def test_generator_reproduces_the_stated_pattern():
    P, attempts = D.pattern_with_attempts()
    assert attempts == 303 and P.shape == (256, 4) and P.dtype == np.int8
    assert P[:3].tolist() == [[-6, -10, -4, 0], [-7, -3, 2, -5], [-1, -5, 5, 3]] and P[255].tolist() == [-9, -2, -2, -6]
    assert hashlib.sha256(P.tobytes()).hexdigest() == PATTERN_SHA
    q = P.astype(int)
    assert ((q[:, 0] ** 2 + q[:, 1] ** 2) <= 169).all() and ((q[:, 2] ** 2 + q[:, 3] ** 2) <= 169).all()
    assert (((q[:, 0] - q[:, 2]) ** 2 + (q[:, 1] - q[:, 3]) ** 2) >= 9).all()
    both = {tuple(r) for r in q.tolist()} | {(r[2], r[3], r[0], r[1]) for r in q.tolist()}
    assert len(both) == 512                                                                    # no pair twice, in either order


def test_trigonometric_tables_are_the_rounded_products():
    assert D.COS[:9] == (16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0)
    assert D.SIN[:9] == (0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384)
    for k in range(32):
        c, s = 16384 * math.cos(2 * math.pi * k / 32), 16384 * math.sin(2 * math.pi * k / 32)
        assert (D.COS[k], D.SIN[k]) == (round(c), round(s))
        assert min(abs(abs(c) % 1 - 0.5), abs(abs(s) % 1 - 0.5)) > 0.03                        # far from a rounding half
        assert (D.COS[(k + 8) % 32], D.SIN[(k + 8) % 32]) == (-D.SIN[k], D.COS[k])


def test_steered_table_sha_range_no_collapse_and_quarter_turn_symmetry():
    T = D.steered()
    assert T.shape == (32, 256, 4) and T.dtype == np.int8 and hashlib.sha256(T.tobytes()).hexdigest() == STEERED_SHA
    assert np.array_equal(T, D.steered_loops())
    assert T.min() >= -13 and T.max() <= 13 and np.array_equal(T[0], D.pattern())
    assert ((T[:, :, 0] != T[:, :, 2]) | (T[:, :, 1] != T[:, :, 3])).all()                     # no pair on one pixel under any bin
    for k in range(32):
        a, b = T[k].astype(int), T[(k + 8) % 32].astype(int)
        assert np.array_equal(b[:, 0], -a[:, 1]) and np.array_equal(b[:, 1], a[:, 0])
        assert np.array_equal(b[:, 2], -a[:, 3]) and np.array_equal(b[:, 3], a[:, 2])
    P = D.pattern().astype(int)
    for k in range(32):                                                                        # no product on an exact half
        for x, y in ((P[:, 0], P[:, 1]), (P[:, 2], P[:, 3])):
            assert ((x * D.COS[k] - y * D.SIN[k] + 8192) % 16384 != 0).all() and ((x * D.SIN[k] + y * D.COS[k] + 8192) % 16384 != 0).all()


# ---------------------------------------------------------------------------------------------- the bin
def test_bin_ties_zero_and_axes():
    assert 3196 * D.COS[0] + 315 * D.SIN[0] == 3196 * D.COS[1] + 315 * D.SIN[1]                # an exact tie of bins 0 and 1
    assert D.orb_bin(3196, 315) == 0 and not D.bin_is_unique(3196, 315)
    assert D.orb_bin(0, 0) == 0 and D.orb_bin(0, 1) == 8 and D.orb_bin(-1, 0) == 16 and D.orb_bin(0, -1) == 24 and D.orb_bin(1, 0) == 0
    assert D.bins([3196, 0, 0, -1, 0], [315, 0, 1, 0, -1]).tolist() == [0, 0, 8, 16, 24]


def test_bin_at_moments_whose_int32_products_would_wrap():
    assert M_MAX * 16384 > 2 ** 31
    ms = [(a * M_MAX, b * M_MAX) for a in (-1, 0, 1) for b in (-1, 0, 1)] + [(M_MAX, 1), (-M_MAX, -1), (M_MAX - 1, M_MAX), (-M_MAX, M_MAX - 1)]
    ms += [(2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]          # any int32 pair the ABI can be handed
    got = D.bins([m[0] for m in ms], [m[1] for m in ms]).tolist()
    assert got == [D.orb_bin(*m) for m in ms]
    for (m10, m01), k in zip(ms, got):                                                         # Python integers, written out again
        v = [m10 * D.COS[j] + m01 * D.SIN[j] for j in range(32)]
        assert k == v.index(max(v))


def test_random_moments_lie_within_half_a_bin_of_atan2():
    rng = np.random.default_rng(3)
    m10, m01 = rng.integers(-M_MAX, M_MAX + 1, 4000), rng.integers(-M_MAX, M_MAX + 1, 4000)
    k = D.bins(m10, m01)
    assert k.tolist() == [D.orb_bin(int(a), int(b)) for a, b in zip(m10, m01)]
    diff = np.degrees(np.arctan2(m01.astype(float), m10.astype(float))) - k * 11.25
    diff = (diff + 180.0) % 360.0 - 180.0
    # half a bin, plus what rounding the table to 1 / 16384 can move a boundary by: under 0.01 degrees
    assert np.abs(diff).max() <= 5.625 + 0.01


# ---------------------------------------------------------------------------------------------- the blur
def test_blur_hand_worked_corners():
    assert D.blur(np.array([[77]], np.uint8)).tolist() == [[77]]                               # 1 x 1: every tap is the pixel, 128 * 128 * 77
    img = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)                                     # 3 x 2
    # row 0 at x = 0: taps -3 .. 0 -> 10 (9 + 17 + 24 + 28 = 78), +1 -> 20 (24), +2, +3 -> 30 (17 + 9 = 26)
    h0 = 78 * 10 + 24 * 20 + 26 * 30
    h1 = 78 * 40 + 24 * 50 + 26 * 60
    # column at y = 0: taps -3 .. 0 -> row 0 (78), +1 .. +3 -> row 1 (24 + 17 + 9 = 50)
    want = (78 * h0 + 50 * h1 + 8192) >> 14
    assert (h0, h1, want) == (2040, 5880, 28)
    assert D.blur(img)[0, 0] == want == D.blur_loops(img)[0, 0]
    img = (np.arange(49).reshape(7, 7) * 5).astype(np.uint8)                                   # 7 x 7: corner (6, 6), both clamps at once
    rows = [sum(g * int(img[y, min(6 + i, 6)]) for g, i in zip(D.G, range(-3, 4))) for y in range(7)]
    want = (sum(g * rows[min(6 + j, 6)] for g, j in zip(D.G, range(-3, 4))) + 8192) >> 14
    assert D.blur(img)[6, 6] == want == D.blur_loops(img)[6, 6]
    assert rows[6] == 9 * 225 + 17 * 230 + 24 * 235 + (28 + 24 + 17 + 9) * 240


@pytest.mark.parametrize("v", (0, 1, 50, 254, 255))
def test_blur_keeps_a_constant_image(v):
    for shape in ((1, 1), (2, 3), (7, 7), (19, 40)):
        assert (D.blur(np.full(shape, v, np.uint8)) == v).all() and (D.blur_loops(np.full(shape, v, np.uint8)) == v).all()


def test_blur_forms_agree():
    rng = np.random.default_rng(11)
    for shape in ((1, 1), (1, 9), (9, 1), (2, 3), (6, 5), (7, 7), (23, 31)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        assert np.array_equal(D.blur(img), D.blur_loops(img)), shape
    assert D.blur(np.zeros((0, 5), np.uint8)).shape == (0, 5)


# ---------------------------------------------------------------------------------------------- the whole call, both forms
@pytest.mark.parametrize("case", OC.all_cases() + DC.all_cases(), ids=lambda c: c["name"])
def test_loops_and_vectorised_forms_agree(case):
    if case["name"] == "identical_dots":
        case = dict(case, img=OC.dot_grid(9, 7, border=16, pitch=8), params=dict(case["params"], n_features=63))   # the same dots, fewer
    a = D.detect_describe(case["img"], case["params"], loops=False)
    b = D.detect_describe(case["img"], case["params"], loops=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert a[2].shape == (len(a[0]), 32) and a[2].dtype == np.uint8


def test_cases_hold_what_they_are_for():
    c = DC.by_name("corners_b16")
    recs = DC.mirror_of("corners_b16")[0]
    h, w = c["img"].shape
    at = set(zip(recs["x_level"].tolist(), recs["y_level"].tolist()))
    assert {(16, 16), (w - 17, 16), (16, h - 17), (w - 17, h - 17)} <= at                      # the reach of the taps and the blur ends on the edge
    recs = DC.mirror_of("identical_dots")[0]
    zero = (recs["m10"] == 0) & (recs["m01"] == 0)                                             # inner dots: symmetric neighbours, bin 0
    assert len(recs) == 1200 and zero.sum() >= (DC.DOTS[0] - 4) * (DC.DOTS[1] - 4) and not zero.all()
    recs = DC.mirror_of("border64")[0]
    assert len(recs) and recs["x_level"].min() >= 64


def test_all_32_bins_occur():
    recs = DC.full_frame_mirror()[0]
    assert set(D.bins(recs["m10"], recs["m01"]).tolist()) == set(range(32))
    recs = DC.mirror_of("planted_angles")[0]
    assert set(D.bins(recs["m10"], recs["m01"]).tolist()) == set(range(32))


# ---------------------------------------------------------------------------------------------- a quarter turn
@pytest.mark.parametrize("name", ("texture", "noise", "texture_w_mod4_1", "planted_angles"))
def test_quarter_turn_gives_the_same_keypoints_and_descriptors(name):
    c = next(c for c in OC.all_cases() + DC.all_cases() if c["name"] == name)
    p = dict(c["params"], n_levels=1, n_features=MAX_KEYPOINTS)
    img = c["img"]
    h, w = img.shape
    recs, counts, desc = D.detect_describe(img, p)
    trecs, tcounts, tdesc = D.detect_describe(np.rot90(img), p)
    assert 0 < counts[0] == tcounts[0] < p["n_features"]                                       # the quota is above the candidate count
    # np.rot90: the pixel (x, y) of the image is the pixel (y, w - 1 - x) of the turned one
    where = {(int(r["y_level"]), w - 1 - int(r["x_level"])): i for i, r in enumerate(recs)}
    assert set(where) == {(int(r["x_level"]), int(r["y_level"])) for r in trecs}
    unique = 0
    for j, r in enumerate(trecs):
        i = where[(int(r["x_level"]), int(r["y_level"]))]
        assert recs["response"][i] == r["response"] and (int(r["m10"]), int(r["m01"])) == (int(recs["m01"][i]), -int(recs["m10"][i]))
        if D.bin_is_unique(int(r["m10"]), int(r["m01"])):
            unique += 1
            assert D.orb_bin(int(r["m10"]), int(r["m01"])) == (D.orb_bin(int(recs["m10"][i]), int(recs["m01"][i])) - 8) % 32
            assert np.array_equal(desc[i], tdesc[j]), (name, i, j)
    assert unique >= len(recs) // 2 and unique > 0
