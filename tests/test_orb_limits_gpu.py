"""GPU parity of the ORB front end (cerebro_amd/csrc/orb.hip) at the limits it is written around, on the dotted-line images of
tests/orb_limit_cases.py: a side of CHIP_ORB_MAX_SIDE (list[kStripMaxCand] of orb_candidates, start[] and the bisection of orb_select at
2032 strips), strip segments filled to `cap` next to empty ones, the radix select with R* walked through every positive and negative
key and through more than 4096 candidates and ties, a quota of 0 on levels that have candidates, and CHIP_MATCH_MAX_KEYPOINTS kept
keypoints through the detector, the descriptor and the frame store.  Everything is compared for equality with the numpy restatement,
as in tests/test_orb_detect_gpu.py and tests/test_orb_describe_gpu.py; tests/test_orb_limits_mirror.py proves what the images are."""
import numpy as np
import pytest

import disparity_cases as DSP
import np_mirror_orb_describe as D
import np_mirror_orb_detect as O
import orb_limit_cases as LC
import stereo_bm_cases as SC
import test_orb_describe_gpu as TD
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
same_records, same_bytes = TD.same_records, TD.same_bytes


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


def check(chip, name: str, n_levels: int = 1, n_features: int = LC.MAX_KEPT):
    """chip_orb_detect and chip_orb_detect_describe == the mirror; -> (records, descriptors)"""
    return TD.check(chip, LC.case(name)["img"], LC.params(n_levels, n_features), (name, n_levels, n_features),
                    want=LC.mirror(name, n_levels, n_features)[:3])


def full_strips_deliver_cap(c: dict, got):
    """from the device's records alone: every strip a whole line falls into holds exactly cap keypoints, all in ascending raster order"""
    assert (got["level"] == 0).all() and (np.diff(LC.rasters_of(got, c["w"])) > 0).all()
    per_strip = LC.strip_counts(c, got["y_level"])
    assert len(per_strip) == c["nstrips"] and (per_strip[list(c["full"])] == c["cap"]).all(), (c["name"], per_strip)
    assert per_strip.sum() == len(got) == c["n_candidates"]


def kept_are_the_largest(got, everything, w: int, what):
    """from device records alone: the smallest kept response is >= every key of the all-kept run that was not kept"""
    left_out = everything[~np.isin(LC.rasters_of(everything, w), LC.rasters_of(got, w))]
    assert len(left_out) == len(everything) - len(got), what
    if len(left_out):
        assert got["response"].min() >= left_out["response"].max(), what


# ---------------------------------------------------------------------------------------------- a: sides of 4096
@pytest.mark.parametrize("n_levels", (1, 8))
@pytest.mark.parametrize("name", LC.SIDES)
def test_sides_of_4096(chip, name, n_levels):
    """at one level every candidate is kept; at eight the quota of level 0 (3558 of 16384, the most a call can ask for) selects among
    the 6096 or 5080, and the levels above are made of rows of up to 3413 pixels"""
    c = LC.case(name)
    st = LC.mirror(name, n_levels)[3]
    got, _ = check(chip, name, n_levels)                                                       # leaves the describing call's planes behind
    assert capi.orb_plan(c["w"], c["h"], LC.params(n_levels)) == st["levels"]
    for l, L in enumerate(st["levels"]):
        im, sc = chip.orb_level(l, L["width"], L["height"])
        assert np.array_equal(im, st["images"][l]), (name, l)
        assert np.array_equal(sc, st["scores"][l]), (name, l)
        assert np.array_equal(chip.orb_blur(l, L["width"], L["height"]), st["blurred"][l]), (name, l)   # level 0: 32 tiles across or 128 down
    if n_levels == 1:
        full_strips_deliver_cap(c, got)
    else:
        assert (got["level"] == 0).sum() == 3558 and got["level"].max() >= 1


@pytest.mark.parametrize("name", tuple(n + "_row2" for n in LC.SIDES))
def test_sides_of_4096_lines_on_the_second_rows(chip, name):
    full_strips_deliver_cap(LC.case(name), check(chip, name)[0])


# ---------------------------------------------------------------------------------------------- b: full segments
@pytest.mark.parametrize("name", ("300x45", "301x45", "301x45_split", "300x45_row2", "301x45_row2"))
def test_full_segments_at_even_and_odd_widths(chip, name):
    """cap = 134 of a rectangle 268 wide, 135 of one 269 wide; split: a strip's segment fills over both of its rows"""
    full_strips_deliver_cap(LC.case(name), check(chip, name)[0])


# ---------------------------------------------------------------------------------------------- c: every rank
def test_every_rank_of_536_distinct_keys(chip):
    """at one level only the selection depends on n_features: R* takes every one of the 368 positive and 168 negative keys in turn"""
    c = LC.case("300x45")
    want_all = LC.mirror("300x45")[0]
    everything, _ = chip.orb_detect(c["img"], LC.params())
    assert same_records(everything, want_all) and (want_all["response"] < 0).sum() == 168
    for q in range(1, 538):
        got, counts = chip.orb_detect(c["img"], LC.params(1, q))
        assert counts == [min(q, 536)] + [0] * 7, q
        assert same_records(got, LC.selected(want_all, c["w"], q)), q
        kept_are_the_largest(got, everything, c["w"], q)


# ---------------------------------------------------------------------------------------------- d: ranks with more than 4096 candidates
def test_ranks_at_the_stride_edges_of_6096_distinct_keys(chip):
    """orb_select reads its keys 4 x 1024 at a time: ranks around 1024, 4096, the count of non-negative keys and the candidate count"""
    c = LC.case("4096x41")
    want_all = LC.mirror("4096x41")[0]
    not_negative = int((want_all["response"] >= 0).sum())
    assert 4096 < not_negative < 6095
    everything, _ = chip.orb_detect(c["img"], LC.params())
    assert same_records(everything, want_all)
    for q in sorted({1023, 1024, 1025, 4095, 4096, 4097, not_negative - 1, not_negative, not_negative + 1, 6095, 6096, 6097}):
        got, counts = chip.orb_detect(c["img"], LC.params(1, q))
        assert counts == [min(q, 6096)] + [0] * 7, q
        assert same_records(got, LC.selected(want_all, c["w"], q)), q
        kept_are_the_largest(got, everything, c["w"], q)
        assert (got["response"] < 0).sum() == max(min(q, 6096) - not_negative, 0), q


@pytest.mark.parametrize("name,n_features", [("4096x41_tied", q) for q in (1024, 4095, 4096, 4097, 5000)] +
                         [("4096x73_tied", q) for q in (4097, 5000, LC.MAX_KEPT)])
def test_ranks_among_tied_keys_keep_the_first_in_raster_order(chip, name, n_features):
    """one dot value: 4056 equal keys on the first and the last line and 2028 (41 rows) or 18252 (73 rows) on the lines between"""
    c = LC.case(name)
    ras, R = LC.level0_candidates(name)
    want, want_counts = O.detect(c["img"], LC.params(1, n_features))
    got, counts = chip.orb_detect(c["img"], LC.params(1, n_features))
    assert counts == want_counts == [n_features] + [0] * 7 and same_records(got, want)
    star = got["response"].min()
    ties_kept = LC.rasters_of(got[got["response"] == star], c["w"])
    ties = ras[R == star]
    assert 0 < len(ties_kept) < len(ties) and len(ties) > 2000                                 # R* is a tied key, and the ties are cut
    assert np.array_equal(ties_kept, ties[:len(ties_kept)])
    assert (R > star).sum() + len(ties_kept) == n_features


# ---------------------------------------------------------------------------------------------- e: quota 0 beside candidates
@pytest.mark.parametrize("n_features", LC.QUOTA0_FEATURES)
def test_quota_0_on_levels_that_have_candidates(chip, n_features):
    img = LC.quota0_image()
    want = LC.quota0_mirror(n_features)
    got, desc = TD.check(chip, img, LC.params(8, n_features), n_features, want=want)
    assert len(got) == len(desc) == n_features
    if n_features in LC.QUOTA0_COUNTS:
        assert np.bincount(got["level"], minlength=8).tolist() == LC.QUOTA0_COUNTS[n_features]


# ---------------------------------------------------------------------------------------------- f: 16384 kept
@pytest.mark.parametrize("n_levels", (1, 8))
def test_16384_features_of_22352_candidates(chip, n_levels):
    got, desc = check(chip, "4096x73", n_levels)
    if n_levels == 1:
        assert len(got) == len(desc) == LC.MAX_KEPT                                            # kept, out, desc, h_desc to their last element
    else:
        assert np.bincount(got["level"], minlength=8).tolist() == [3558, 2965, 2471, 2059, 538, 0, 0, 0]


def test_a_slot_of_16384_keypoints_put_straight_from_the_pair():
    c = LC.case("4096x73")
    left = c["img"]
    right = np.ascontiguousarray(np.roll(left, -6, axis=1))                                    # a constant disparity of 6
    orb, Q = LC.params(), DSP.Q_EUROC
    want = LC.mirror("4096x73")
    with capi.Chip(4096) as ctx:
        ctx.frame_store_reserve(1, LC.MAX_KEPT)
        n = ctx.frame_put_orb_stereo(1, left, right, Q, orb, SC.PAIR_PARAMS)
        a = ctx.frame_read(1)
        recs, desc = TD.composed(ctx, 1, left, right, orb, SC.PAIR_PARAMS)                      # the same id: the one slot, replaced
        b = ctx.frame_read(1)
        assert ctx.frame_store_info() == dict(n_slots=1, slot_keypoints=LC.MAX_KEPT, n_frames=1)
        small = ctx.orb_detect_describe(left, LC.params(1, 5000))                              # the large buffers serve a normal call
    assert n == a["n"] == b["n"] == LC.MAX_KEPT and TD.same_frames(a, b)
    assert same_records(recs, want[0]) and same_bytes(desc, want[2]) and same_bytes(a["desc"], want[2])
    assert same_bytes(a["kp"], np.stack([want[0]["x"], want[0]["y"]], axis=1).astype(np.float32).reshape(-1, 2))
    assert a["pts"].shape == (LC.MAX_KEPT, 4)
    want_small = LC.mirror("4096x73", 1, 5000)
    assert same_records(small[0], want_small[0]) and small[1] == want_small[1] and same_bytes(small[2], want_small[2])
