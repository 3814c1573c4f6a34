"""GPU parity of the ORB detector (cerebro_amd/csrc/orb.hip: orb_pyramid, orb_fast_score, orb_candidates, orb_select, orb_moments
behind chip_orb_detect) through ctypes -> C ABI against the numpy restatement (tests/np_mirror_orb_detect.py).  Everything is compared
for equality: records byte for byte, pyramid levels and score planes element for element.  The definition is this project's own and
is not pinned against OpenCV."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_mirror_orb_detect as O
import orb_detect_cases as OC
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
# widths of all four residues mod 4 around the score tile's width, heights around its height
STAGE_SHAPES = tuple((w, h) for w in (OC.SCORE_TILE_W - 1, OC.SCORE_TILE_W, OC.SCORE_TILE_W + 1, OC.SCORE_TILE_W + 2)
                     for h in (OC.SCORE_TILE_H - 1, OC.SCORE_TILE_H, OC.SCORE_TILE_H + 1)) + ((7, 7), (9, 6), (261, 35), (1229, 9))
# (1229 -> 1024 columns: the bilinear fraction reaches 2047, which needs a destination of 1024 or more)


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


def status_of(call, *args):
    with pytest.raises(capi.ChipError) as e:
        call(*args)
    return e.value.status


def same_records(got, want):
    return got.dtype == want.dtype == capi.ORB_KEYPOINT_DTYPE and got.shape == want.shape and got.tobytes() == want.tobytes()


def check(chip, img, p: dict, what):
    """detect on the device == the vectorised mirror, records and counts; -> the records"""
    want, want_counts = O.detect(img, p)
    got, counts = chip.orb_detect(img, O.params(**p))
    assert counts == want_counts, (what, counts, want_counts)
    assert same_records(got, want), what
    assert not got["zero"].any()
    return got


# ---------------------------------------------------------------------------------------------- 1: stage by stage
@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_level_image_and_score_plane_equals_mirror(chip, shape):
    """the planes hold -256 where the score is not defined (within 3 of an edge); 7 x 7 has one defined pixel, 9 x 6 none"""
    w, h = shape
    img = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w)).astype(np.uint8)
    p = O.params(n_levels=3, border=16, n_features=100)
    st = {}
    O.detect(img, p, stages=st)
    chip.orb_detect(img, p)
    assert capi.orb_plan(w, h, p) == st["levels"]
    for l, L in enumerate(st["levels"]):
        im, sc = chip.orb_level(l, L["width"], L["height"])
        assert np.array_equal(im, st["images"][l]), (shape, l)
        assert np.array_equal(sc, st["scores"][l]), (shape, l)
        defined = np.zeros(sc.shape, bool)
        defined[3:L["height"] - 3, 3:L["width"] - 3] = True
        assert (sc[~defined] == O.UNDEFINED).all()
    if shape == (7, 7):
        assert (st["scores"][0] != O.UNDEFINED).sum() <= 1 and st["scores"][0][3, 3] == O.score_pixel(img.astype(np.int64), 3, 3)
    assert status_of(chip.orb_level, 3, 1, 1) == capi.CHIP_ERR_RANGE


# ---------------------------------------------------------------------------------------------- 2: the whole call
@pytest.mark.parametrize("threshold", OC.THRESHOLDS)
def test_every_case_equals_mirror(chip, threshold):
    for c in OC.all_cases():
        check(chip, c["img"], dict(c["params"], fast_threshold=threshold), (c["name"], threshold))


@pytest.mark.parametrize("border", (16, 64))
def test_border_at_both_bounds(chip, border):
    img = OC.texture(np.random.default_rng(border), 171, 150)
    got = check(chip, img, dict(n_levels=2, n_features=200, border=border), border)
    assert len(got) and got["x_level"].min() >= border and got["y_level"].min() >= border


def test_images_without_a_detection_area_and_a_flat_image(chip):
    one = check(chip, OC.with_dots(33, 33, [(16, 16, 200)]), dict(border=16), "33 x 33")       # one detection pixel at level 0, none above
    assert len(one) == 1 and (one["x_level"][0], one["y_level"][0], one["level"][0]) == (16, 16, 0)
    assert len(check(chip, np.full((1, 1), 7, np.uint8), {}, "1 x 1")) == 0
    assert len(check(chip, OC.flat(200, 90), {}, "flat")) == 0


@pytest.mark.parametrize("n_levels", range(1, 9))
def test_random_texture_at_every_level_count(chip, n_levels):
    got = check(chip, OC.texture(np.random.default_rng(160120), 160, 120), dict(n_levels=n_levels, n_features=700, border=16), n_levels)
    assert got["level"].max() == n_levels - 1                                                 # 160 x 120: level 7 is 45 x 33, one row of area


def test_full_frame_at_the_defaults(chip):
    want, want_counts = OC.full_frame_mirror()
    got, counts = chip.orb_detect(OC.full_frame())
    levels = capi.orb_plan(*OC.FULL)
    assert len(got) == 5000 and counts == want_counts == [L["quota"] for L in levels]          # every level has an area and is full
    assert same_records(got, want)


# ---------------------------------------------------------------------------------------------- 3: selection at its edges
DOTS = (40, 30)                                                                               # 1200 identical dots: more than one pass of 1024
N_DOTS = DOTS[0] * DOTS[1]


@functools.lru_cache(maxsize=None)
def dots_image(two_levels_of_brightness: bool) -> np.ndarray:
    value = (lambda i, j: 230 if (i + 2 * j) % 3 == 0 else 200) if two_levels_of_brightness else 200
    return OC.dot_grid(*DOTS, border=16, pitch=8, value=value)


# the kept prefix ends inside a wave, on a wave boundary, on the workgroup boundary of orb_select's compaction, and around the dot count
@pytest.mark.parametrize("n_features", (1, 37, OC.WAVE, 3 * OC.WAVE, OC.SELECT_THREADS - 1, OC.SELECT_THREADS, OC.SELECT_THREADS + 1,
                                        N_DOTS - 1, N_DOTS, N_DOTS + 1))
def test_equal_keys_keep_the_first_in_raster_order(chip, n_features):
    img = dots_image(False)
    assert img.shape[1] - 32 > OC.CAND_THREADS                                                 # a row is more than one pass of orb_candidates
    got = check(chip, img, dict(n_levels=1, n_features=n_features, border=16), n_features)
    assert len(got) == min(n_features, N_DOTS) and len(set(got["response"])) == 1
    raster = got["y_level"].astype(np.int64) * img.shape[1] + got["x_level"]
    assert (np.diff(raster) > 0).all() and raster[0] == 16 * img.shape[1] + 16


@pytest.mark.parametrize("extra", (0, 1, OC.WAVE, 333))
def test_threshold_key_with_larger_keys_and_ties(chip, extra):
    img = dots_image(True)
    n_bright = sum((i + 2 * j) % 3 == 0 for i in range(DOTS[0]) for j in range(DOTS[1]))
    got = check(chip, img, dict(n_levels=1, n_features=n_bright + extra, border=16), extra)
    big = got["response"].max()
    assert (got["response"] == big).sum() == n_bright and (got["response"] < big).sum() == extra


# ---------------------------------------------------------------------------------------------- 4: state
def test_buffers_of_a_large_image_serve_a_small_one_and_the_large_one_again():
    large, small = OC.full_frame(), OC.by_name("texture")
    with capi.Chip(4096) as a:
        first = a.orb_detect(large)
        mid = a.orb_detect(small["img"], small["params"])
        again = a.orb_detect(large)
    with capi.Chip(4096) as b:
        fresh_small = b.orb_detect(small["img"], small["params"])
    with capi.Chip(4096) as c:
        fresh_large = c.orb_detect(large)
    assert same_records(first[0], fresh_large[0]) and same_records(again[0], fresh_large[0]) and first[1] == again[1] == fresh_large[1]
    assert same_records(mid[0], fresh_small[0]) and mid[1] == fresh_small[1]
    assert same_records(mid[0], O.detect(small["img"], small["params"])[0])


def test_debug_statuses_and_a_group_ctx():
    c = OC.by_name("dots")
    with capi.Chip(4096) as ctx:
        assert status_of(ctx.orb_level, 0, 4, 4) == capi.CHIP_ERR_BUSY
        ctx.orb_detect(c["img"], c["params"])                                                  # two levels
        L = capi.orb_plan(c["img"].shape[1], c["img"].shape[0], c["params"])
        assert np.array_equal(ctx.orb_level(0, L[0]["width"], L[0]["height"])[0], c["img"])
        ctx.orb_level(1, L[1]["width"], L[1]["height"])
        assert status_of(ctx.orb_level, 2, 4, 4) == status_of(ctx.orb_level, -1, 4, 4) == capi.CHIP_ERR_RANGE
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.orb_detect, c["img"], c["params"]) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.orb_level, 0, 4, 4) == capi.CHIP_ERR_UNSUPPORTED


def test_first_use_under_a_resident_scan_instance(monkeypatch):
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    c = OC.by_name("texture")
    with capi.Chip(4096) as ctx:
        ctx.append_synthetic(400, 5)
        ticks = scenarios.default_schedule(400)
        for l in ticks[:8]:
            ctx.loop_tick(l)
        got, counts = ctx.orb_detect(c["img"], c["params"])
        ctx.loop_tick(ticks[8])
        larger = ctx.orb_detect(OC.full_frame())                                               # every buffer grows
        ctx.loop_tick(400)
    want, want_counts = O.detect(c["img"], c["params"])
    assert same_records(got, want) and counts == want_counts
    assert same_records(larger[0], OC.full_frame_mirror()[0])


def test_detect_between_two_pair_matches_leaves_them_unchanged():
    import match_pairs_cases as PC
    import test_match_pairs_gpu as TP
    c = OC.by_name("texture")
    with TP.new_chip() as ctx:
        TP.load(ctx, PC.frames())
        before = TP.blob(TP.pairs_all(ctx, PC.PAIRS[:3], 0))
        got, _ = ctx.orb_detect(c["img"], c["params"])
        after = TP.blob(TP.pairs_all(ctx, PC.PAIRS[:3], 0))
    assert before == after
    assert same_records(got, O.detect(c["img"], c["params"])[0])


# ---------------------------------------------------------------------------------------------- 5: closing the loop with the store
def test_detected_keypoints_go_through_a_stereo_put(chip):
    import disparity_cases as DC
    import np_mirror_stereo_bm as BM
    import stereo_bm_cases as SC
    left, right, disp = SC.pair_of_size(200, 120)
    p = dict(n_levels=3, n_features=400, border=16)
    kps = check(chip, left, p, "left image")
    assert len(kps) > 50 and kps["level"].max() == 2
    kp_xy = np.stack([kps["x"], kps["y"]], axis=1)
    desc = np.random.default_rng(9).integers(0, 256, (len(kps), 32)).astype(np.uint8)
    with capi.Chip(4096) as ctx:
        ctx.frame_store_reserve(1, 512)
        ctx.frame_put_stereo(5, dict(desc=desc, kp=kp_xy), left, right, DC.Q_EUROC, SC.PAIR_PARAMS)
        back = ctx.frame_read(5)
    assert back["n"] == len(kps) and np.array_equal(back["kp"], kp_xy) and np.array_equal(back["desc"], desc)
    want = BM.records(kp_xy, None, None, None, DC.Q_EUROC, disp=disp)
    assert BM.same_floats(back["pts"], want) and (want[:, 3] == 1.0).all()                     # every keypoint is a pixel of the image


# ---------------------------------------------------------------------------------------------- 6: the example
def test_orb_detect_example():
    exe = LIB / "orb_detect"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== the host restatement") == 2 and "DIFFERS" not in r.stdout
