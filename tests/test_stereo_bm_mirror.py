"""The numpy restatement of the block matcher (tests/np_mirror_stereo_bm.py) on the CPU: its two forms agree, the case set
(tests/stereo_bm_cases.py) has the properties it claims, and the definition gives what it should on inputs whose answer is known.
numpy alone; nothing here is pinned against OpenCV (the definition is this project's own)."""
import numpy as np
import pytest

import np_mirror_stereo_bm as BM
import stereo_bm_cases as SC

INVALID = int(BM.INVALID)


def test_invalid_is_the_disparity_tests_invalid():
    import disparity_cases as DC
    assert BM.INVALID == DC.INVALID == -16


def test_shapes_cover_every_width_residue_and_the_claimed_defined_pixels():
    assert {w % 4 for w, _, _, _ in SC.SHAPES} == {0, 1, 2, 3}
    assert {nd for _, _, nd, _ in SC.SHAPES} == {16, 32, 48, 64}
    for (w, h, nd, block), want in zip(SC.SHAPES, SC.N_DEFINED):
        y0, y1, x0, x1 = BM.defined_region(w, h, nd, block)
        assert max(0, y1 - y0 + 1) * max(0, x1 - x0 + 1) == want, (w, h, nd, block)


def test_prefilter_by_hand():
    I = np.array([[1, 2, 4, 8], [3, 9, 27, 81], [5, 25, 125, 255]], np.uint8)
    P = BM.prefilter(I, 31)
    assert (P[:, 0] == 31).all() and (P[:, 3] == 31).all()
    # row 0: rows -1 and 1 are row 1: 2 (27 - 3) + 2 (4 - 1) = 54 -> clipped to 31;  row 1, x = 1: (4 - 1) + 2 (27 - 3) + (125 - 5) = 171
    assert P[0, 1] == 62 and P[1, 1] == 62
    assert BM.prefilter(np.array([[9, 8, 7, 7, 9]], np.uint8), 5).tolist() == [[5, 0, 1, 10, 5]]      # h == 1: 4 (I[x+1] - I[x-1])
    assert BM.prefilter(np.array([[3, 4, 5], [3, 5, 5]], np.uint8), 63).tolist() == [[63, 63 + 8, 63], [63, 63 + 8, 63]]   # h == 2: row -1 is row 1, row 2 is row 0


def test_the_two_forms_agree_on_every_small_case():
    seen = 0
    for c in SC.all_cases():
        a, b = BM.loops(c["left"], c["right"], c["params"]), BM.vectorised(c["left"], c["right"], c["params"])
        assert a.dtype == b.dtype == np.int16 and np.array_equal(a, b), c["name"]
        seen += int((a != INVALID).sum())
    assert seen > 500


def test_nothing_is_defined_outside_the_region_and_nothing_reaches_16_nd():
    for c in SC.all_cases():
        p = c["params"]
        d = BM.vectorised(c["left"], c["right"], p)
        h, w = d.shape
        y0, y1, x0, x1 = BM.defined_region(w, h, p["num_disparities"], p["block_size"])
        mask = np.zeros((h, w), bool)
        if y1 >= y0 and x1 >= x0:
            mask[y0:y1 + 1, x0:x1 + 1] = True
        assert (d[~mask] == INVALID).all(), c["name"]
        assert ((d == INVALID) | ((d >= 0) & (d < 16 * p["num_disparities"]))).all(), c["name"]


def test_every_event_occurs_in_the_noise_set():
    total = dict.fromkeys(SC.EVENTS, 0)
    cases = SC.noise_cases()
    for c in cases:
        assert c["left"].max() <= 3 and c["right"].max() <= 3 and c["params"]["block_size"] == 5
        for e, k in SC.events_of(c).items():
            total[e] += k
    print(len(cases), total)
    for e in SC.EVENTS:
        assert total[e] >= 1, (e, total)


def _interior(c):
    """the defined pixels at least r + 1 from every image edge: their windows see no prefilter border"""
    p = c["params"]
    h, w = c["left"].shape
    r = p["block_size"] // 2
    y0, y1, x0, x1 = BM.defined_region(w, h, p["num_disparities"], p["block_size"])
    return slice(max(y0, r + 1), min(y1, h - 2 - r) + 1), slice(max(x0, r + 1), min(x1, w - 2 - r) + 1)


def test_a_planted_shift_is_found_on_every_interior_pixel():
    """at an exact match m = 0 and the sub-pixel term is 128 (p - n) / max(p, n).  p and n sum the same column differences of the
    texture but for ONE window column each (p the first, n the last), so |p - n| / max(p, n) is about 1 / (2r + 1) times the spread
    of the column sums: at block 21 the term stays inside [-15, 16] and the value in {16 s, 16 s + 1}; at block 5 or 7 one column is
    a fifth of the window and it does not, so the property is asserted on the block-21 shapes (every planted shift of both)."""
    seen = 0
    for c in SC.small_cases():
        if not c["name"].startswith("shift") or c["params"]["block_size"] != 21:
            continue
        s = int(c["name"].split("_")[0][5:])
        v = BM.vectorised(c["left"], c["right"], c["params"])[_interior(c)].astype(int)
        assert np.isin(v, (16 * s, 16 * s + 1)).all(), (c["name"], np.unique(v))
        seen += v.size
    assert seen > 100


def test_the_full_frame_finds_its_tiles():
    c, d = SC.full_frame(), SC.full_frame_map()
    ys, xs = _interior(c)
    v, s = d[ys, xs].astype(int), c["shifts"][ys, xs]
    exact = (v == 16 * s) | (v == 16 * s + 1)
    assert exact.mean() > 0.6 and (v != INVALID).mean() > 0.7, (exact.mean(), (v != INVALID).mean())      # the rest straddles a tile edge


def test_the_half_pixel_blend():
    c = SC.case("half", *SC.planted(np.random.default_rng(5), 101, 25, 20.5), 64, 21)
    v = BM.vectorised(c["left"], c["right"], c["params"])[_interior(c)].astype(int)
    assert v.size and (np.abs(v - 328) <= 2).all(), np.unique(v)


def test_flat_pairs_keep_nothing():
    n = 0
    for c in SC.small_cases():
        if c["name"].startswith("flat"):
            assert (BM.vectorised(c["left"], c["right"], c["params"]) == INVALID).all(), c["name"]
            n += 1
    assert n == 2 * len(SC.SHAPES)


def test_period_8_the_largest_multiple_wins_or_nothing_does():
    seen = 0
    for c in SC.small_cases():
        if not c["name"].startswith("period8") or BM.details(c["left"], c["right"], c["params"]) is None:
            continue
        nd = c["params"]["num_disparities"]
        det = BM.details(c["left"], c["right"], c["params"])
        y0, _, x0, _ = det["region"]
        ys, xs = _interior(c)
        inner = slice(ys.start - y0, ys.stop - y0), slice(xs.start - x0, xs.stop - x0)
        v = BM.vectorised(c["left"], c["right"], c["params"])[ys, xs].astype(int)
        if v.size == 0:
            continue
        seen += 1
        assert ((det["sad"][::8, inner[0], inner[1]] == 0).all() and (det["m"][inner] == 0).all())      # a minimum at every multiple of 8
        assert (det["D"][inner] == 8 * ((nd - 1) // 8)).all(), c["name"]
        if c["params"]["uniqueness_ratio"] == 0:
            assert (np.abs(v - 16 * 8 * ((nd - 1) // 8)) <= 8).all(), (c["name"], np.unique(v))       # D, and a sub-pixel term of half a pixel at most
        else:
            assert (v == INVALID).all(), (c["name"], np.unique(v))
    assert seen >= 8


def test_full_swing_reaches_the_largest_sad():
    (c,) = [c for c in SC.small_cases() if c["name"] == "swing_101x25_nd64_b21"]
    det = BM.details(c["left"], c["right"], c["params"])
    assert det["sad"].max() == 441 * 126 == 55566 and det["sad"].min() == 0


def test_the_hand_worked_triple():
    # (p, m, n) = (10, 4, 7) at D = 5: q = 10 + 7 - 8 + |10 - 7| = 12, (p - n) * 256 / q = 64
    assert BM.value_of(5, 10, 4, 7) == (1280 + 768 // 12 + 15) >> 4 == 84
    # truncation toward zero shows at (7, 4, 27): q = 46, -20 * 256 / 46 = -111.3 -> -111 and the value 74; floor gives -112 and 73
    assert BM.value_of(5, 7, 4, 27) == (1280 - 111 + 15) >> 4 == 74 and (1280 - 112 + 15) >> 4 == 73
    assert BM.value_of(0, 9, 9, 9) == 0 and BM.value_of(63, 3, 3, 3) == (63 * 256 + 15) >> 4
