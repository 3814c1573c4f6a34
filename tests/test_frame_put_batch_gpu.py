"""GPU parity of the batched frame puts (chip_frame_put_orb_stereo_batch, chip_frame_put_raw_orb_stereo_batch: the fb_* entries of
cerebro_amd/csrc/orb.hip and frames.hip) and of chip_frame_put_records, through ctypes -> C ABI.  The reference is the loop of single
calls under other ids on the same ctx -- every stored row, every count, byte for byte -- and, for one case, the numpy restatements
(np_mirror_rectify -> np_mirror_orb_detect / _describe -> np_mirror_stereo_bm -> np_mirror_disparity).  Nothing here has a tolerance."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import disparity_cases as DSP
import np_mirror_orb_describe as D
import np_mirror_rectify as R
import np_mirror_stereo_bm as BM
import orb_detect_cases as OC
import rectify_cases as RC
import stereo_bm_cases as SC
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
Q = DSP.Q_EUROC
ORB_PUT = dict(n_levels=3, n_features=400, border=16)
SLOT_KP = 512
# 163 x 121: chip_orb_plan accepts it, the width is no multiple of 4 and the height is odd -- level 0 has a row pitch of its own, so the
# left images go into the pyramid row by row, and a pair is no multiple of 16 bytes long, so the frames' strides are padded
SIZES = ((160, 120), (320, 240), (163, 121))
KINV = np.linalg.inv(np.array([[458.654, 0, 80.0], [0, 457.296, 60.0], [0, 0, 1]]))


def status_of(call, *args, **kw):
    with pytest.raises(capi.ChipError) as e:
        call(*args, **kw)
    return e.value.status


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_frames(a: dict, b: dict):
    return (a["n"], a["width"], a["height"]) == (b["n"], b["width"], b["height"]) and all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts"))


_PAIRS: dict = {}


def pairs(w: int, h: int, F: int) -> list:
    """F pairs of one size whose content separates the frames: 0 the textured warped pair of rectify_cases, 1 all black (keeps nothing),
    2 textured in one corner only (some levels stay short of their quota), then textures of their own with the right image shifted.
    Made once per size and shared."""
    have = _PAIRS.setdefault((w, h), [])
    while len(have) < F:
        f = len(have)
        if f == 0:
            p = RC.warped_pair(w, h)
            have.append((p["left_raw"], p["right_raw"]))
        elif f == 1:
            have.append((np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)))
        else:
            rng = np.random.default_rng(7000 + 31 * f + w)
            left = OC.texture(rng, w, h)
            if f == 2:
                corner = np.full((h, w), 50, np.uint8)
                corner[:44, :44] = left[:44, :44]
                left = corner
            have.append((left, np.roll(left, -(4 + f % 5), axis=1).copy()))
    return have[:F]


def mixed(w: int, h: int, F: int) -> list:
    """the same pairs in an order that puts the empty and the sparse frame between full ones"""
    p = pairs(w, h, F)
    order = sorted(range(F), key=lambda f: (f * 7) % max(F, 1) if F > 2 else f)
    return [p[f] for f in order]


def put_single(ctx, raw: bool):
    return ctx.frame_put_raw_orb_stereo if raw else ctx.frame_put_orb_stereo


def put_batch(ctx, raw: bool):
    return ctx.frame_put_raw_orb_stereo_batch if raw else ctx.frame_put_orb_stereo_batch


def fresh_ctx(w: int, h: int, n_slots: int, slot_kp: int = SLOT_KP):
    ctx = capi.Chip(4096)
    ctx.frame_store_reserve(n_slots, slot_kp)
    p = RC.warped_pair(w, h)
    ctx.rectify_set_maps(p["left"], p["right"])
    return ctx


# ---------------------------------------------------------------------------------------------- 1: equality with the single call
@pytest.mark.parametrize("raw", (False, True), ids=("rectified", "raw"))
@pytest.mark.parametrize("F", (1, 2, 3, 16, 17))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_equals_the_loop_of_single_calls(size, F, raw):
    w, h = size
    ps = mixed(w, h, F)
    lefts, rights = [p[0] for p in ps], [p[1] for p in ps]
    with fresh_ctx(w, h, 2 * F) as ctx:
        ns = put_batch(ctx, raw)(range(100, 100 + F), lefts, rights, Q, ORB_PUT, SC.PAIR_PARAMS)
        last = ctx.frame_put_last()
        single = [put_single(ctx, raw)(200 + f, lefts[f], rights[f], Q, ORB_PUT, SC.PAIR_PARAMS) for f in range(F)]
        got = [ctx.frame_read(100 + f) for f in range(F)]
        want = [ctx.frame_read(200 + f) for f in range(F)]
        assert ctx.frame_store_info()["n_frames"] == 2 * F
        # the eight level counts: the detector alone on what the put saw
        rect = [ctx.rectify_pair(l, r)[0] if raw else l for l, r in ps[:3]]
        counts = [ctx.orb_detect_describe(img, ORB_PUT)[1] for img in rect]
    groups = capi.frame_put_plan(w, h, F, ORB_PUT, raw)
    assert groups == dict(group=16, n_groups=1 if F <= 16 else 2)
    assert last["groups"] == last["waits"] == groups["n_groups"] and 0 < last["launches"] <= 16 * last["groups"], last
    assert ns == single == [g["n"] for g in got], (ns, single)
    for f in range(F):
        assert same_frames(got[f], want[f]), f
    for f in range(min(F, 3)):
        assert sum(counts[f]) == ns[f] and counts[f][3:] == [0] * 5, (f, counts[f])
    if F >= 3:
        assert 0 in ns and len(set(ns)) >= 3, ns                                                # empty, sparse and fuller frames in one call
    if F >= 4:
        assert max(ns) == ORB_PUT["n_features"], ns                                             # ... and one that fills every quota


def test_content_separates_the_frames():
    """what the case above relies on: frame 1 keeps nothing, frame 2 leaves levels short of their quota, frame 3 fills every quota"""
    w, h = SIZES[0]
    ps = pairs(w, h, 4)
    quotas = [lv["quota"] for lv in capi.orb_plan(w, h, ORB_PUT)]
    with capi.Chip(4096) as ctx:
        counts = [ctx.orb_detect_describe(p[0], ORB_PUT)[1] for p in ps]
    quotas += [0] * (capi.CHIP_ORB_MAX_LEVELS - len(quotas))
    assert counts[3] == quotas and sum(counts[0]) > 100 and sum(counts[1]) == 0
    assert 0 < sum(counts[2]) and any(c < q for c, q in zip(counts[2], quotas)), (counts[2], quotas)


@pytest.mark.parametrize("raw", (False, True), ids=("rectified", "raw"))
def test_batch_of_three_equals_the_numpy_mirrors(raw):
    w, h = SIZES[0]
    ps = mixed(w, h, 3)
    maps = RC.warped_pair(w, h)
    with fresh_ctx(w, h, 3) as ctx:
        ns = put_batch(ctx, raw)([1, 2, 3], [p[0] for p in ps], [p[1] for p in ps], Q, ORB_PUT, SC.PAIR_PARAMS)
        got = [ctx.frame_read(i) for i in (1, 2, 3)]
    for f, (l, r) in enumerate(ps):
        if raw:
            l, r = R.rectify(l, *maps["left"]), R.rectify(r, *maps["right"])
        recs, counts, desc = D.detect_describe(l, ORB_PUT)
        kp = np.stack([recs["x"], recs["y"]], axis=1).astype(np.float32).reshape(-1, 2)
        assert ns[f] == got[f]["n"] == len(recs) == sum(counts), f
        assert same_bytes(got[f]["desc"], desc.reshape(-1, 32)) and same_bytes(got[f]["kp"], kp), f
        if len(recs):
            assert BM.same_floats(got[f]["pts"], BM.records(kp, l, r, SC.PAIR_PARAMS, Q)), f


# ---------------------------------------------------------------------------------------------- 2: parameter corners
@pytest.mark.parametrize("orb, bm, slot_kp", (
    (dict(n_levels=1, n_features=400, border=16), None, 512),
    (dict(n_levels=8, n_features=400, border=16), None, 512),                  # the upper levels have no detection rectangle at this size
    (dict(n_levels=3, n_features=50, border=16), None, 64),                    # the quotas bite: ties are decided by raster index
    (None, None, 5000),                                                        # the defaults: 5000 features, 8 levels, border 31
    (ORB_PUT, dict(num_disparities=16, block_size=5), 512),
), ids=("one_level", "eight_levels", "fifty_features", "defaults", "nd16_block5"))
def test_parameter_corners(orb, bm, slot_kp):
    w, h = SIZES[0]
    ps = mixed(w, h, 4)
    lefts, rights = [p[0] for p in ps], [p[1] for p in ps]
    bmp = None if bm is None else dict(SC.PAIR_PARAMS, **bm)
    with fresh_ctx(w, h, 8, slot_kp) as ctx:
        for raw in (False, True):
            base = 10 if raw else 0
            ns = put_batch(ctx, raw)(range(base + 1, base + 5), lefts, rights, Q, orb, bmp)
            last = ctx.frame_put_last()
            got = [ctx.frame_read(base + 1 + f) for f in range(4)]
            single = [put_single(ctx, raw)(base + 1 + f, lefts[f], rights[f], Q, orb, bmp) for f in range(4)]    # replaces in place
            want = [ctx.frame_read(base + 1 + f) for f in range(4)]
            assert ns == single and all(same_frames(g, x) for g, x in zip(got, want)), (raw, ns, single)
            assert last["groups"] == last["waits"] == 1 and last["launches"] <= 16, last
            assert max(ns) > 0 and 0 in ns
        assert ctx.frame_store_info()["n_frames"] == 8


# ---------------------------------------------------------------------------------------------- 3: slots, replacing, all or nothing
def test_slots_need_not_be_adjacent_and_known_ids_are_replaced_in_place():
    w, h = SIZES[0]
    ps = pairs(w, h, 8)
    put = lambda ctx, i, f: ctx.frame_put_orb_stereo(i, ps[f][0], ps[f][1], Q, ORB_PUT, SC.PAIR_PARAMS)
    with fresh_ctx(w, h, 8) as ctx:
        for i in range(1, 7):
            put(ctx, i, i % 4)                                                                  # slots 0 .. 5
        ctx.frame_drop(3)                                                                       # a hole at slot 2; 6 and 7 are free
        keep = {i: ctx.frame_read(i) for i in (1, 4, 6)}
        old = {i: ctx.frame_read(i) for i in (2, 5)}
        ids, fs = [10, 2, 11, 5, 12], [4, 5, 6, 7, 0]
        ns = ctx.frame_put_orb_stereo_batch(ids, [ps[f][0] for f in fs], [ps[f][1] for f in fs], Q, ORB_PUT, SC.PAIR_PARAMS)
        last = ctx.frame_put_last()
        assert last == dict(groups=1, launches=last["launches"], waits=1) and last["launches"] <= 16
        assert ctx.frame_store_info() == dict(n_slots=8, slot_keypoints=SLOT_KP, n_frames=8)
        got = {i: ctx.frame_read(i) for i in ids}
        for i in keep:
            assert same_frames(ctx.frame_read(i), keep[i]), i                                   # the other frames' bytes are unchanged
        for i in old:
            assert not same_frames(got[i], old[i]), i                                           # replaced
        for i, f in zip(ids, fs):                                                               # each under a single call in its own slot
            assert put(ctx, i, f) == ns[ids.index(i)] and same_frames(ctx.frame_read(i), got[i]), i
        # one free slot too few: nothing changes
        ctx.frame_drop(10)
        before = {i: ctx.frame_read(i) for i in (1, 2, 4, 5, 6, 11, 12)}
        info = ctx.frame_store_info()
        call = lambda ids: ctx.frame_put_orb_stereo_batch(ids, [ps[0][0]] * len(ids), [ps[0][1]] * len(ids), Q, ORB_PUT, SC.PAIR_PARAMS)
        assert status_of(call, [1, 20, 21]) == capi.CHIP_ERR_OOM                                # two new ids, one free slot
        assert ctx.frame_store_info() == info and all(same_frames(ctx.frame_read(i), before[i]) for i in before)
        assert status_of(ctx.frame_read, 20) == capi.CHIP_ERR_RANGE
        assert call([1, 20]) == [ns[4]] * 2 and ctx.frame_store_info()["n_frames"] == 8          # exactly enough


def test_statuses():
    w, h = SIZES[0]
    ps = pairs(w, h, 3)
    lefts, rights = [p[0] for p in ps], [p[1] for p in ps]
    maps = RC.warped_pair(w, h)
    with capi.Chip(4096) as ctx:
        both = (ctx.frame_put_orb_stereo_batch, ctx.frame_put_raw_orb_stereo_batch)
        assert ctx.frame_put_last() == dict(groups=0, launches=0, waits=0)
        for put in both:
            assert status_of(put, [1, 2, 3], lefts, rights, Q, ORB_PUT) == capi.CHIP_ERR_BUSY   # no reserve
        ctx.frame_store_reserve(4, 300)
        assert status_of(both[1], [1, 2, 3], lefts, rights, Q, dict(ORB_PUT, n_features=300)) == capi.CHIP_ERR_BUSY   # no maps
        ctx.rectify_set_maps(maps["left"], maps["right"])
        small = [RC.image(80, 70)] * 3
        assert status_of(both[1], [1, 2, 3], small, small, Q, dict(ORB_PUT, n_features=300)) == capi.CHIP_ERR_INVALID_ARG   # not the maps' size
        for put in both:
            assert status_of(put, [1, 2, 1], lefts, rights, Q, dict(ORB_PUT, n_features=300)) == capi.CHIP_ERR_INVALID_ARG   # a repeated id
            assert status_of(put, [1, 2, 3], lefts, rights, Q, ORB_PUT) == capi.CHIP_ERR_UNSUPPORTED          # 400 > a slot's 300
            assert status_of(put, [1, 2, 3], lefts, rights, Q, None) == capi.CHIP_ERR_UNSUPPORTED
            assert status_of(put, [1, 2, 3], lefts, rights, Q, dict(ORB_PUT, border=15)) == capi.CHIP_ERR_UNSUPPORTED
            assert status_of(put, [1, 2, 3], lefts, rights, Q, ORB_PUT, dict(SC.PAIR_PARAMS, block_size=4)) == capi.CHIP_ERR_UNSUPPORTED
        assert ctx.frame_store_info()["n_frames"] == 0 and ctx.frame_put_last()["groups"] == 0   # a refused call stores and runs nothing
    with capi.Chip(4096, devices=[0, 0]) as grp:
        for put in (grp.frame_put_orb_stereo_batch, grp.frame_put_raw_orb_stereo_batch):
            assert status_of(put, [1, 2, 3], lefts, rights, Q, ORB_PUT) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_put_records, 1, dict(desc=np.zeros((0, 32), np.uint8), kp=np.zeros((0, 2), np.float32),
                                                        pts=np.zeros((0, 4), np.float32), width=w, height=h)) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_put_last) == capi.CHIP_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 4: records back into the store
def test_records_restore_a_store():
    w, h = SIZES[0]
    F = 5
    ps = mixed(w, h, F)
    ids = list(range(1, F + 1))
    summary = lambda s: tuple(getattr(s, k) for k, _ in capi.MatchSummary._fields_)
    with fresh_ctx(w, h, F + 1) as ctx:
        ns = ctx.frame_put_raw_orb_stereo_batch(ids, [p[0] for p in ps], [p[1] for p in ps], Q, ORB_PUT, SC.PAIR_PARAMS)
        full = [i for i, n in zip(ids, ns) if n > 100]
        assert 0 in ns and len(full) >= 3
        a_ids, b_ids = [full[0], full[0], full[1]], [full[1], full[2], full[2]]
        before = [summary(s) for s in ctx.match_pairs_stored(a_ids, b_ids, KINV)]
        saved = {i: ctx.frame_read(i) for i in ids}
        for i in ids:
            ctx.frame_drop(i)
        assert ctx.frame_store_info()["n_frames"] == 0
        for i in reversed(ids):                                                                 # other slots than before
            ctx.frame_put_records(i, saved[i])
        assert ctx.frame_store_info()["n_frames"] == F
        for i in ids:
            assert same_frames(ctx.frame_read(i), saved[i]), i
        assert [summary(s) for s in ctx.match_pairs_stored(a_ids, b_ids, KINV)] == before
        # a record whose fourth float is neither 0.0f nor 1.0f is refused and the frame stays
        bad = dict(saved[full[0]], pts=saved[full[0]]["pts"].copy())
        bad["pts"][7, 3] = 0.5
        assert status_of(ctx.frame_put_records, full[0], bad) == capi.CHIP_ERR_INVALID_ARG
        assert status_of(ctx.frame_put_records, 99, bad) == capi.CHIP_ERR_INVALID_ARG and ctx.frame_store_info()["n_frames"] == F
        assert same_frames(ctx.frame_read(full[0]), saved[full[0]])
        too_many = dict(desc=np.zeros((SLOT_KP + 1, 32), np.uint8), kp=np.zeros((SLOT_KP + 1, 2), np.float32),
                        pts=np.zeros((SLOT_KP + 1, 4), np.float32), width=w, height=h)
        assert status_of(ctx.frame_put_records, 99, too_many) == capi.CHIP_ERR_UNSUPPORTED      # more than a slot holds
        ctx.frame_put_records(99, saved[full[1]])
        assert status_of(ctx.frame_put_records, 100, saved[full[1]]) == capi.CHIP_ERR_OOM       # a full store
    with capi.Chip(4096) as ctx:
        assert status_of(ctx.frame_put_records, 1, saved[1]) == capi.CHIP_ERR_BUSY              # no reserve


# ---------------------------------------------------------------------------------------------- 5: the example
def test_frame_put_batch_example():
    exe = LIB / "frame_put_batch"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout and "all equal" in r.stdout
