"""GPU parity of the ORB descriptor (cerebro_amd/csrc/orb.hip: orb_blur, orb_describe behind chip_orb_detect_describe and
chip_frame_put_orb_stereo) through ctypes -> C ABI against the numpy restatement (tests/np_mirror_orb_describe.py).  Everything is
compared for equality: blurred planes element for element, records and descriptors byte for byte, a frame put straight from its pair
against the same frame composed from single calls.  The definition is this project's own and is not pinned against OpenCV."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import disparity_cases as DSP
import np_mirror_orb_describe as D
import np_mirror_orb_detect as O
import orb_describe_cases as DC
import orb_detect_cases as OC
import stereo_bm_cases as SC
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
Q = DSP.Q_EUROC
# widths of all four residues mod 4 around the blur tile's width, heights around its height, and the three hand-worked sizes
BLUR_SHAPES = tuple((w, h) for w in (DC.BLUR_TILE_W - 1, DC.BLUR_TILE_W, DC.BLUR_TILE_W + 1, DC.BLUR_TILE_W + 2)
                    for h in (DC.BLUR_TILE_H - 1, DC.BLUR_TILE_H, DC.BLUR_TILE_H + 1)) + ((1, 1), (3, 2), (7, 7), (261, 67))


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


def status_of(call, *args, **kw):
    with pytest.raises(capi.ChipError) as e:
        call(*args, **kw)
    return e.value.status


def same_records(got, want):
    return got.dtype == want.dtype == capi.ORB_KEYPOINT_DTYPE and got.shape == want.shape and got.tobytes() == want.tobytes()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(chip, img, p: dict, what, want=None):
    """detect_describe on the device == the mirror and == chip_orb_detect's records; -> (records, descriptors)"""
    want_recs, want_counts, want_desc = want or D.detect_describe(img, p)
    plain, plain_counts = chip.orb_detect(img, O.params(**p))
    got, counts, desc = chip.orb_detect_describe(img, O.params(**p))
    assert counts == want_counts == plain_counts, (what, counts, want_counts)
    assert same_records(got, want_recs) and same_records(got, plain), what
    assert same_bytes(desc, want_desc), (what, int((desc != want_desc).any(axis=1).sum()))
    return got, desc


# ---------------------------------------------------------------------------------------------- 1: the blurred planes
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_blurred_plane_equals_mirror(chip, shape):
    w, h = shape
    img = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w)).astype(np.uint8)
    p = O.params(n_levels=3, border=16, n_features=100)
    st = {}
    D.detect_describe(img, p, stages=st)
    chip.orb_detect_describe(img, p)
    for l, L in enumerate(st["levels"]):
        assert np.array_equal(chip.orb_blur(l, L["width"], L["height"]), st["blurred"][l]), (shape, l)
    assert status_of(chip.orb_blur, 3, 1, 1) == status_of(chip.orb_blur, -1, 1, 1) == capi.CHIP_ERR_RANGE


def test_blur_of_constant_images_and_of_255(chip):
    for v in (0, 255, 77):
        img = np.full((70, 133), v, np.uint8)
        chip.orb_detect_describe(img, O.params(n_levels=2, border=16))
        L = capi.orb_plan(133, 70, dict(n_levels=2, border=16))
        for l in range(2):
            assert (chip.orb_blur(l, L[l]["width"], L[l]["height"]) == v).all()


def test_full_frame_blur_descriptors_and_records(chip):
    recs, counts, desc, st = DC.full_frame_mirror()
    got, gdesc = check(chip, OC.full_frame(), {}, "752 x 480", want=(recs, counts, desc))
    assert len(got) == 5000 and set(D.bins(got["m10"], got["m01"]).tolist()) == set(range(32))
    for l, L in enumerate(st["levels"]):                                                       # all 8 levels, whole planes
        assert np.array_equal(chip.orb_blur(l, L["width"], L["height"]), st["blurred"][l]), l


# ---------------------------------------------------------------------------------------------- 2: the whole call
@pytest.mark.parametrize("threshold", (0, 20))
def test_every_case_equals_mirror(chip, threshold):
    kept = 0
    for c in OC.all_cases() + DC.all_cases():
        kept += len(check(chip, c["img"], dict(c["params"], fast_threshold=threshold), (c["name"], threshold))[0])
    assert kept > 1500


def test_keypoints_on_the_corners_of_the_detection_rectangle(chip):
    c = DC.by_name("corners_b16")
    got, _ = check(chip, c["img"], c["params"], "corners")
    h, w = c["img"].shape
    assert {(16, 16), (w - 17, 16), (16, h - 17), (w - 17, h - 17)} <= set(zip(got["x_level"].tolist(), got["y_level"].tolist()))


def test_identical_dots_have_bin_0(chip):
    c = DC.by_name("identical_dots")
    got, desc = check(chip, c["img"], c["params"], "dots")
    zero = (got["m10"] == 0) & (got["m01"] == 0)
    assert len(got) == 1200 and zero.sum() > 900
    h, w = c["img"].shape
    x, y = got["x_level"].astype(int), got["y_level"].astype(int)
    inner = (x >= 32) & (x <= w - 33) & (y >= 32) & (y <= h - 33)                               # two dots in: the taps and the blur reach 16
    assert inner.sum() == (DC.DOTS[0] - 4) * (DC.DOTS[1] - 4) and zero[inner].all()
    assert len({d.tobytes() for d in desc[inner]}) == 1                                         # the same surroundings, the same bits


# wave and workgroup edges of orb_describe: four waves a workgroup, one keypoint a wave
@pytest.mark.parametrize("n_features", (1, DC.WAVE - 1, DC.WAVE, DC.WAVE + 1, 257))
def test_kept_counts_at_the_edges_of_a_wave_and_a_workgroup(chip, n_features):
    img = OC.texture(np.random.default_rng(77), 203, 151)
    got, _ = check(chip, img, dict(n_levels=1, n_features=n_features, border=16), n_features)
    assert len(got) == n_features


def test_images_that_keep_nothing_leave_desc_untouched(chip):
    for img in (OC.flat(200, 90), np.full((1, 1), 7, np.uint8), OC.flat(31, 40)):
        h, w = img.shape
        kp = np.zeros(5000, capi.ORB_KEYPOINT_DTYPE)
        desc = np.full((5000, 32), 0xA5, np.uint8)
        n = capi.C.c_int32(-1)
        rc = chip.lib.chip_orb_detect_describe(chip.h, capi._ptr(img), w, h, None, capi._ptr(kp), 5000, capi.C.byref(n), None, capi._ptr(desc))
        assert rc == capi.CHIP_OK and n.value == 0 and (desc == 0xA5).all()


# ---------------------------------------------------------------------------------------------- 3: call sequences through one ctx
def test_large_small_large_and_a_plain_detect_hides_the_blur():
    large, small = OC.full_frame(), DC.by_name("texture_w_mod4_1")
    want_large, want_small = DC.full_frame_mirror(), DC.mirror_of("texture_w_mod4_1")
    with capi.Chip(4096) as a:
        assert status_of(a.orb_blur, 0, 4, 4) == capi.CHIP_ERR_BUSY                             # nothing yet
        first = a.orb_detect_describe(large)
        mid = a.orb_detect_describe(small["img"], small["params"])
        again = a.orb_detect_describe(large)
        assert np.array_equal(a.orb_blur(0, *OC.FULL), want_large[3]["blurred"][0])
        a.orb_detect(small["img"], small["params"])
        assert status_of(a.orb_blur, 0, 4, 4) == capi.CHIP_ERR_BUSY                             # a plain detect leaves no blurred plane
        a.orb_level(0, small["img"].shape[1], small["img"].shape[0])                            # ... but its levels
    for got in (first, again):
        assert same_records(got[0], want_large[0]) and got[1] == want_large[1] and same_bytes(got[2], want_large[2])
    assert same_records(mid[0], want_small[0]) and mid[1] == want_small[1] and same_bytes(mid[2], want_small[2])


def test_group_ctx_is_refused():
    c = DC.by_name("border64")
    left, right, _ = SC.pair_of_size(160, 120)
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.orb_detect_describe, c["img"], c["params"]) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.orb_blur, 0, 4, 4) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_put_orb_stereo, 1, left, right, Q, dict(n_features=100, border=16)) == capi.CHIP_ERR_UNSUPPORTED


def test_first_use_under_a_resident_scan_instance(monkeypatch):
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    c = DC.by_name("texture_w_mod4_2")
    with capi.Chip(4096) as ctx:
        ctx.append_synthetic(400, 5)
        ticks = scenarios.default_schedule(400)
        for l in ticks[:8]:
            ctx.loop_tick(l)
        got = ctx.orb_detect_describe(c["img"], c["params"])
        ctx.loop_tick(ticks[8])
        larger = ctx.orb_detect_describe(OC.full_frame())                                      # every buffer grows
        ctx.loop_tick(400)
    want, big = DC.mirror_of("texture_w_mod4_2"), DC.full_frame_mirror()
    assert same_records(got[0], want[0]) and got[1] == want[1] and same_bytes(got[2], want[2])
    assert same_records(larger[0], big[0]) and same_bytes(larger[2], big[2])


def test_describe_between_two_pair_matches_leaves_them_unchanged():
    import match_pairs_cases as PC
    import test_match_pairs_gpu as TP
    c = DC.by_name("texture_w_mod4_3")
    with TP.new_chip() as ctx:
        TP.load(ctx, PC.frames())
        before = TP.blob(TP.pairs_all(ctx, PC.PAIRS[:3], 0))
        got = ctx.orb_detect_describe(c["img"], c["params"])
        after = TP.blob(TP.pairs_all(ctx, PC.PAIRS[:3], 0))
    want = DC.mirror_of("texture_w_mod4_3")
    assert before == after
    assert same_records(got[0], want[0]) and same_bytes(got[2], want[2])


# ---------------------------------------------------------------------------------------------- 4: a frame straight from its pair
ORB_PUT = dict(n_levels=3, n_features=400, border=16)


def composed(ctx, id: int, left, right, orb, bm=None):
    """chip_orb_detect_describe -> chip_frame_put_stereo with kp_xy from the records; -> (records, descriptors)"""
    recs, _, desc = ctx.orb_detect_describe(left, orb)
    ctx.frame_put_stereo(id, dict(desc=desc, kp=np.stack([recs["x"], recs["y"]], axis=1).astype(np.float32).reshape(-1, 2)), left, right, Q, bm)
    return recs, desc


def same_frames(a: dict, b: dict):
    return (a["n"], a["width"], a["height"]) == (b["n"], b["width"], b["height"]) and all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts"))


@pytest.mark.parametrize("what", ("160x120", "163x121", "752x480", "keeps_nothing"))
def test_put_from_the_pair_equals_the_composed_path(what):
    if what == "752x480":
        f = SC.full_frame()
        left, right, orb, bm, slot = f["left"], f["right"], None, f["params"], 5000
    elif what == "keeps_nothing":
        left = right = OC.flat(160, 120)
        orb, bm, slot = dict(ORB_PUT), SC.PAIR_PARAMS, 512
    else:
        w, h = (int(v) for v in what.split("x"))                                                # 163: a width that is no multiple of 4
        left, right, _ = SC.pair_of_size(w, h)
        orb, bm, slot = dict(ORB_PUT), SC.PAIR_PARAMS, 512
    with capi.Chip(4096) as ctx:
        ctx.frame_store_reserve(2, slot)
        n = ctx.frame_put_orb_stereo(1, left, right, Q, orb, bm)
        blur0 = ctx.orb_blur(0, left.shape[1], left.shape[0])                                   # the put is a describing call
        recs, desc = composed(ctx, 2, left, right, orb, bm)
        a, b = ctx.frame_read(1), ctx.frame_read(2)
        assert ctx.frame_store_info()["n_frames"] == 2
    want = D.detect_describe(left, orb or {})
    assert n == a["n"] == len(recs) == len(want[0]) and same_frames(a, b)
    assert same_records(recs, want[0]) and same_bytes(a["desc"], want[2]) and np.array_equal(blur0, D.blur(left))
    assert same_bytes(a["kp"], np.stack([want[0]["x"], want[0]["y"]], axis=1).astype(np.float32).reshape(-1, 2))
    if what == "keeps_nothing":
        assert n == 0 and (a["width"], a["height"]) == (160, 120)                               # present and empty
    else:
        assert n > 100 and (a["pts"][:, 3] == 1.0).all()


def test_replace_across_the_four_ways_of_putting():
    import frame_store_cases as fc
    import np_mirror_stereo_bm as BM
    left, right, disp = SC.pair_of_size(160, 120)
    rng = np.random.default_rng(31)
    with capi.Chip(4096) as ctx:
        ctx.frame_store_reserve(2, 512)
        recs, desc = composed(ctx, 2, left, right, ORB_PUT, SC.PAIR_PARAMS)
        want = ctx.frame_read(2)
        f = fc.frame(rng, 300, plant_at=range(0, 300, 17))                                      # 64 x 48, with its image
        g = dict(desc=rng.integers(0, 256, (120, 32)).astype(np.uint8), kp=np.stack([recs["x"], recs["y"]], axis=1)[:120].astype(np.float32))
        ctx.frame_put(1, f)                                                                     # an image put ...
        assert ctx.frame_put_orb_stereo(1, left, right, Q, ORB_PUT, SC.PAIR_PARAMS) == want["n"]   # ... replaced by a put from the pair
        assert ctx.frame_store_info()["n_frames"] == 2 and same_frames(ctx.frame_read(1), want)
        ctx.frame_put_disparity(1, g, disp, Q)                                                  # ... by a disparity put
        r = ctx.frame_read(1)
        assert r["n"] == 120 and same_bytes(r["desc"], g["desc"])
        ctx.frame_put_orb_stereo(1, left, right, Q, ORB_PUT, SC.PAIR_PARAMS)
        assert same_frames(ctx.frame_read(1), want)
        ctx.frame_put_stereo(1, g, left, right, Q, SC.PAIR_PARAMS)                              # ... by a stereo put
        r2 = ctx.frame_read(1)
        assert r2["n"] == 120 and BM.same_floats(r2["pts"], r["pts"])
        ctx.frame_put_orb_stereo(1, left, right, Q, ORB_PUT, SC.PAIR_PARAMS)                    # and back
        assert ctx.frame_store_info()["n_frames"] == 2 and same_frames(ctx.frame_read(1), want)


def test_put_statuses_failure_rules_and_a_full_store():
    left, right, _ = SC.pair_of_size(160, 120)
    ptr, Qd = capi._ptr, np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
    n = capi.C.c_int32(-7)
    with capi.Chip(4096) as ctx:
        put = ctx.frame_put_orb_stereo
        assert status_of(put, 1, left, right, Q, ORB_PUT) == capi.CHIP_ERR_BUSY                 # no reserve
        ctx.frame_store_reserve(2, 300)
        assert status_of(put, 1, left, right, Q, dict(ORB_PUT, n_features=301)) == capi.CHIP_ERR_UNSUPPORTED   # more than a slot holds
        assert status_of(put, 1, left, right, Q, None) == capi.CHIP_ERR_UNSUPPORTED             # the defaults' 5000 as well
        assert status_of(put, 1, left, right, Q, dict(ORB_PUT, border=15)) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(put, 1, left, right, Q, ORB_PUT, dict(SC.PAIR_PARAMS, block_size=4)) == capi.CHIP_ERR_UNSUPPORTED
        raw = ctx.lib.chip_frame_put_orb_stereo
        p = capi.default_orb_params(**dict(ORB_PUT, n_features=300))
        assert raw(ctx.h, 1, 160, 120, ptr(left), None, capi.C.byref(p), None, ptr(Qd), capi.C.byref(n)) == capi.CHIP_ERR_INVALID_ARG
        assert raw(ctx.h, 1, 160, 120, ptr(left), ptr(right), capi.C.byref(p), None, ptr(Qd), None) == capi.CHIP_ERR_INVALID_ARG
        assert ctx.frame_store_info()["n_frames"] == 0 and n.value == -7                        # a refused put stores nothing
        orb = dict(ORB_PUT, n_features=300)
        k = put(1, left, right, Q, orb)
        assert k == 300 == put(2, left, right, Q, orb)                                          # the slot holds exactly what is kept
        assert status_of(put, 3, left, right, Q, orb) == capi.CHIP_ERR_OOM                      # a full store
        before = ctx.frame_read(1)
        assert status_of(put, 1, left, right, Q, dict(orb, n_features=301)) == capi.CHIP_ERR_UNSUPPORTED
        assert same_frames(ctx.frame_read(1), before)                                           # a refused replace leaves the frame
        assert put(2, left, right, Q, dict(orb, n_features=50)) == 50                           # a known id replaces in a full store
        ctx.frame_drop(1)
        assert put(3, left, right, Q, orb) == 300 and ctx.frame_store_info()["n_frames"] == 2
        assert sorted(ctx.frame_read(i)["n"] for i in (2, 3)) == [50, 300]


# ---------------------------------------------------------------------------------------------- 5: the quarter turn, matched
def test_a_frame_and_its_quarter_turn_match_as_the_mirror_predicts():
    import np_mirror_gms_modes as GM
    import np_mirror_match as MM
    rng = np.random.default_rng(90)
    left = OC.texture(rng, 200, 152)
    right = np.roll(left, -6, axis=1)                                                           # a constant disparity of 6
    tl, tr = np.rot90(left), np.rot90(right)                                                    # the twin; its records are not compared
    orb = dict(n_levels=1, n_features=2000, border=16)
    a, b = D.detect_describe(left, orb), D.detect_describe(tl, orb)
    kpa = np.stack([a[0]["x"], a[0]["y"]], axis=1).astype(np.float32)
    kpb = np.stack([b[0]["x"], b[0]["y"]], axis=1).astype(np.float32)
    idx, dist = MM.orb_bf_match(a[2], b[2])
    inl, choice = GM.gms_filter_modes(kpa, (200, 152), kpb, (152, 200), np.arange(len(idx), dtype=np.int32), idx, capi.CHIP_GMS_WITH_ROTATION)
    predicted = int(choice["n_inliers"])
    assert len(a[0]) == len(b[0]) > 300 and int((dist == 0).sum()) > len(a[0]) // 2             # unique bins: identical descriptors
    with capi.Chip(4096) as ctx:
        ctx.frame_store_reserve(2, 2000)
        assert ctx.frame_put_orb_stereo(1, left, right, Q, orb, dict(num_disparities=16, block_size=9)) == len(a[0])
        assert ctx.frame_put_orb_stereo(2, np.ascontiguousarray(tl), np.ascontiguousarray(tr), Q, orb, dict(num_disparities=16, block_size=9)) == len(b[0])
        Kinv = np.linalg.inv(np.array([[458.654, 0, 100.0], [0, 457.296, 76.0], [0, 0, 1]]))
        sm, ch = ctx.match_pairs_stored([1], [2], Kinv, capi.CHIP_GMS_WITH_ROTATION)
    assert sm[0].n_matches_all == len(a[0]) and predicted > len(a[0]) // 2
    assert sm[0].n_matches_gms >= predicted


# ---------------------------------------------------------------------------------------------- 6: the example
def test_orb_frame_put_example():
    exe = LIB / "orb_frame_put"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout
