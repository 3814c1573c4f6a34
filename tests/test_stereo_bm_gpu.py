"""GPU parity of the block matcher (cerebro_amd/csrc/frames.hip: bm_prefilter, bm_dense behind chip_stereo_bm, bm_keypoints behind
chip_frame_put_stereo) through ctypes -> C ABI against the numpy restatement (tests/np_mirror_stereo_bm.py), element for element.
A frame put from its rectified pair must be indistinguishable from the same frame put through chip_frame_put_disparity with
CHIP_DISP_S16 and the map of chip_stereo_bm: same records, same match results, same poses.  The case set is tests/stereo_bm_cases.py;
the definition is this project's own and is not pinned against OpenCV."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import disparity_cases as DC
import frame_store_cases as fc
import match_pairs_cases as PC
import np_mirror_stereo_bm as BM
import stereo_bm_cases as SC
from cerebro_amd import capi
from test_disparity_gpu import _same_estimate, blob, everything, same_bytes, status_of

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
KINV = PC.kinv()
N_SLOTS, SLOT_KP = 2 * len(DC.NAMES) + 4, 5000                       # the case set twice (from pairs, from maps) and four spare
VIA_MAP = 100000                                                      # id offset of the frames put through chip_frame_put_disparity
SPARE = (1, 2, 3, 4)
Q = DC.Q_EUROC
INVALID = int(BM.INVALID)
# images for the put tests, widths of all four residues mod 4: (w, h, nd, block)
PUT_SHAPES = ((100, 25, 64, 21), (101, 25, 64, 21), (90, 23, 48, 21), (43, 11, 32, 7))


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        c.frame_store_reserve(N_SLOTS, SLOT_KP)
        yield c


@pytest.fixture
def clean(chip):
    """the module's ctx with an empty store"""
    yield chip
    for i in list(SPARE) + list(range(10, 10 + N_SLOTS)) + [i + o for i in DC.ID.values() for o in (0, VIA_MAP)]:
        if chip.lib.chip_frame_drop(chip.h, i) not in (capi.CHIP_OK, capi.CHIP_ERR_RANGE):
            raise AssertionError("chip_frame_drop")
    assert chip.frame_store_info() == dict(n_slots=N_SLOTS, slot_keypoints=SLOT_KP, n_frames=0)


@functools.lru_cache(maxsize=None)
def mirror_map(name: str) -> np.ndarray:
    """the mirror's map of a case, computed once: the plain loops on the small cases, the vectorised form on the full frame"""
    if name == "full":
        return SC.full_frame_map()
    (c,) = [c for c in SC.all_cases() if c["name"] == name]
    return BM.loops(c["left"], c["right"], c["params"])


@functools.lru_cache(maxsize=None)
def put_image(k: int) -> dict:
    w, h, nd, block = PUT_SHAPES[k]
    left, right, _ = SC.tiled_pair(np.random.default_rng(40 + k), w, h, tile=16, lo=0, hi=nd - 1)
    c = SC.case(f"put{k}", left, right, nd, block)
    c["disp"] = BM.vectorised(left, right, c["params"])
    assert (c["disp"] != INVALID).sum() > 10 and (c["disp"] == INVALID).sum() > 10
    return c


def keypoints(rng, n: int, w: int, h: int, nd: int, block: int) -> np.ndarray:
    """n keypoints: the first and last defined column and row and one pixel outside each, four consecutive columns, the keypoints at the
    image border, outside and NaN of tests/frame_store_cases.py -- at scattered indices when n has room for all of them -- and the rest
    half over the whole image (and one pixel around it), half over the defined region"""
    y0, y1, x0, x1 = BM.defined_region(w, h, nd, block)
    ym, xm = (y0 + y1) // 2, (x0 + x1) // 2
    pts = [(x + 0.5, ym + 0.25) for x in (x0 - 1, x0, x1, x1 + 1)] + [(xm + 0.75, y + 0.5) for y in (y0 - 1, y0, y1, y1 + 1)]
    pts += [(x + 0.125, y0 + 0.875) for x in range(x0 + 1, x0 + 5)]
    pts += [(-0.5, 3.0), (-1.0, 3.0), (w - 0.5, 3.0), (float(w), 3.0), (np.nan, 3.0), (5.0, -0.5), (5.0, -1.0), (5.0, h - 0.5), (5.0, float(h)), (5.0, np.nan)]
    kp = np.stack([rng.uniform(-1.0, w + 1.0, n), rng.uniform(-1.0, h + 1.0, n)], axis=1)
    inside = rng.random(n) < 0.5
    kp[inside] = np.stack([rng.uniform(x0, x1 + 1.0, n), rng.uniform(y0, y1 + 1.0, n)], axis=1)[inside]
    at = rng.permutation(n)[:len(pts)] if n >= len(pts) else np.arange(n)
    if n >= 64:
        at[:3] = (0, 63, n - 1)                                       # first and last lane-0 writers of a block and the last keypoint
        at[3:] = [i for i in rng.permutation(np.arange(1, n - 1)) if i != 63][:len(at) - 3]
    kp[at] = np.array(pts[:len(at)])
    return kp.astype(np.float32)


def frame_of(rng, n, w, h, nd, block) -> dict:
    return dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), kp=keypoints(rng, n, w, h, nd, block))


# ---------------------------------------------------------------------------------------------- 1: the dense map
@pytest.mark.parametrize("k", range(len(SC.SHAPES)), ids=["%dx%d_nd%d_b%d" % s for s in SC.SHAPES])
def test_dense_map_equals_mirror_on_every_small_case(chip, k):
    assert chip.lib.chip_build_has_stereo_bm() == 1 and chip.lib.chip_abi_version() == 7
    tag = "_%dx%d_nd%d_b%d" % SC.SHAPES[k]
    mine = [c for c in SC.small_cases() if c["name"].endswith(tag)]
    assert len(mine) == 10
    for c in mine:
        got = chip.stereo_bm(c["left"], c["right"], c["params"])
        want = mirror_map(c["name"])
        assert got.dtype == np.int16 and got.shape == want.shape
        assert np.array_equal(got, want), (c["name"], int((got != want).sum()), np.argwhere(got != want)[:5])
    if SC.N_DEFINED[k] == 0:
        assert all((mirror_map(c["name"]) == INVALID).all() for c in mine)       # too small for a defined pixel: no error, all -16


def test_dense_map_equals_mirror_on_the_noise_cases(chip):
    for c in SC.noise_cases():
        got = chip.stereo_bm(c["left"], c["right"], c["params"])
        assert np.array_equal(got, mirror_map(c["name"])), c["name"]


def test_dense_map_of_the_full_frame_equals_the_vectorised_mirror(chip):
    c = SC.full_frame()
    got = chip.stereo_bm(c["left"], c["right"])                       # params None: the defaults
    want = mirror_map("full")
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5])
    assert (want != INVALID).mean() > 0.5


# ---------------------------------------------------------------------------------------------- 2: put and read back
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_put_and_read_back_equals_mirror(clean, n):
    seen = set()
    for k in range(len(PUT_SHAPES)):                                  # every width residue at every n
        c = put_image(k)
        w, h, nd, block = PUT_SHAPES[k]
        seen.add(w % 4)
        f = frame_of(np.random.default_rng(100 * n + k), n, w, h, nd, block)
        clean.frame_put_stereo(3, f, c["left"], c["right"], Q, c["params"])
        r = clean.frame_read(3)
        want = BM.records(f["kp"], c["left"], c["right"], c["params"], Q, disp=c["disp"])
        assert (r["n"], r["width"], r["height"]) == (n, w, h)
        assert same_bytes(r["desc"], f["desc"]) and same_bytes(r["kp"], f["kp"])    # as put
        assert BM.same_floats(r["pts"], want), (n, k, np.argwhere(r["pts"].view(np.uint32) != want.view(np.uint32))[:5])
        if n >= 255:
            assert (want[:, 3] == 0).any() and (want[:, 3] == 1).any() and not want[want[:, 3] == 0].any()
            inside, x, y = BM._pixel(f["kp"], w, h)
            d = c["disp"][y[inside], x[inside]]
            assert (d == INVALID).any() and (d != INVALID).any()
    assert seen == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------- 3: composition
def _composed(chip, c, f):
    """-> the two read-backs: the frame put from the pair, and through chip_stereo_bm -> chip_frame_put_disparity(S16)"""
    chip.frame_put_stereo(1, f, c["left"], c["right"], Q, c["params"])
    disp = chip.stereo_bm(c["left"], c["right"], c["params"])
    chip.frame_put_disparity(2, f, disp, Q)
    return chip.frame_read(1), chip.frame_read(2), disp


def test_put_equals_dense_map_then_disparity_put_on_every_case(clean):
    cases = SC.all_cases()
    for j, c in enumerate(cases):
        h, w = c["left"].shape
        p = c["params"]
        f = frame_of(np.random.default_rng(3000 + j), 150, w, h, p["num_disparities"], p["block_size"])
        a, b, disp = _composed(clean, c, f)
        assert all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts")) and (a["n"], a["width"], a["height"]) == (b["n"], b["width"], b["height"]), c["name"]
        assert BM.same_floats(a["pts"], BM.records(f["kp"], None, None, None, Q, disp=disp)), c["name"]


def test_put_equals_dense_map_then_disparity_put_on_the_full_frame(clean):
    c = SC.full_frame()
    f = frame_of(np.random.default_rng(5000), 5000, *SC.FULL, 64, 21)
    a, b, disp = _composed(clean, c, f)
    assert all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts"))
    assert np.array_equal(disp, mirror_map("full"))
    assert BM.same_floats(a["pts"], BM.records(f["kp"], None, None, None, Q, disp=mirror_map("full")))
    assert (a["pts"][:, 3] == 1).sum() > 4000


def test_no_value_reaches_16_nd(chip):
    c = put_image(1)
    for nd in (16, 32, 48, 64):
        for block in (5, 21):
            p = BM.params(num_disparities=nd, block_size=block, uniqueness_ratio=0, texture_threshold=0)
            got = chip.stereo_bm(c["left"], c["right"], p)
            assert np.array_equal(got, BM.vectorised(c["left"], c["right"], p)), (nd, block)
            kept = got[got != INVALID]
            assert kept.size and kept.min() >= 0 and kept.max() < 16 * nd, (nd, block, kept.max())


# ---------------------------------------------------------------------------------------------- 4: the pair set
def load_both(chip):
    """every frame of the case set from its synthetic pair under its id, and from the mirror map of that pair under id + VIA_MAP"""
    for name, f in SC.pair_set_frames().items():
        chip.frame_put_stereo(DC.ID[name], f, f["left"], f["right"], DC.Q_PAIRS)
        chip.frame_put_disparity(DC.ID[name] + VIA_MAP, f, f["disp"], DC.Q_PAIRS)


def pairs_all(chip, modes, offset):
    a_ids, b_ids = PC.ids()
    return everything(chip, *chip.match_pairs_stored([i + offset for i in a_ids], [i + offset for i in b_ids], KINV, modes))


@pytest.mark.parametrize("modes", [0, 3])
def test_pair_set_from_stereo_pairs_equals_map_puts(clean, modes):
    chip = clean
    load_both(chip)
    valid = 0
    for name in DC.NAMES:                                             # indistinguishable afterwards: the stored frames themselves
        a, b = chip.frame_read(DC.ID[name]), chip.frame_read(DC.ID[name] + VIA_MAP)
        assert (a["n"], a["width"], a["height"]) == (b["n"], b["width"], b["height"])
        assert all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts")), name
        valid += int((a["pts"][:, 2] > 0.1).sum())
    assert valid > 3000
    got, via = pairs_all(chip, modes, 0), pairs_all(chip, modes, VIA_MAP)
    assert len(got) == len(via) == len(DC.PAIRS) == 11
    for j, (g, v) in enumerate(zip(got, via)):
        assert blob([g]) == blob([v]), (modes, j, DC.PAIRS[j])
    if modes == 0:
        assert tuple(g["summary"]["n_matches_gms"] for g in got) == DC.EXPECTED_GMS      # matching and GMS read no depths
        assert sum(g["summary"]["n_3d3d"] for g in got) > 1000


def test_batched_solvers_are_bit_identical_on_both_ways_of_putting(clean):
    chip = clean
    load_both(chip)
    a_ids, b_ids = PC.ids()

    def solve(offset):
        sms = chip.match_pairs_stored([i + offset for i in a_ids], [i + offset for i in b_ids], KINV)
        P = len(sms)
        problems = []
        for j, sm in enumerate(sms):
            problems += [(j, capi.CHIP_SET_AB, sm.n_3d2d_ab), (j, capi.CHIP_SET_BA, sm.n_3d2d_ba)]
        pp, pi = capi.default_ransac_params(), capi.default_icp_params()
        pp.seed, pi.seed = 5, 6
        ticket = chip.icp_matched_batch_enqueue([(j, sms[j].n_3d3d) for j in range(P)], pi, [900 + 3 * j for j in range(P)])
        pnp = chip.pnp_matched_batch(problems, pp, [100 + 7 * i for i in range(2 * P)])      # the ICP batch runs underneath
        return [s.as_dict() for s in sms], pnp, chip.icp_matched_batch_collect(ticket)

    sm_s, pnp_s, icp_s = solve(0)
    sm_m, pnp_m, icp_m = solve(VIA_MAP)
    assert sm_s == sm_m
    assert len(pnp_s) == len(pnp_m) == 22 and len(icp_s) == len(icp_m) == 11
    for i, (d, h) in enumerate(zip(pnp_s, pnp_m)):
        _same_estimate(d, h, ("pnp", i))
    for i, (d, h) in enumerate(zip(icp_s, icp_m)):
        _same_estimate(d, h, ("icp", i))
    assert sum(r["status"] == 0 for r in pnp_s) >= 2 and sum(r["status"] == 0 for r in icp_s) >= 1   # problems were solved, not only refused


# ---------------------------------------------------------------------------------------------- 5: buffer and slot reuse
def test_replace_across_the_three_ways_of_putting(clean):
    chip = clean
    rng = np.random.default_rng(21)
    c = put_image(0)
    w, h, nd, block = PUT_SHAPES[0]
    f = fc.frame(rng, 300, plant_at=range(0, 300, 17))                # 64 x 48, with its image
    g, e = frame_of(rng, 200, w, h, nd, block), frame_of(rng, 120, w, h, nd, block)
    rec = lambda fr: BM.records(fr["kp"], None, None, None, Q, disp=c["disp"])   # noqa: E731
    chip.frame_put(1, f)                                              # an image put ...
    chip.frame_put_stereo(1, g, c["left"], c["right"], Q, c["params"])   # ... replaced by a stereo put under the same id
    r = chip.frame_read(1)
    assert chip.frame_store_info()["n_frames"] == 1 and (r["n"], r["width"], r["height"]) == (200, w, h)
    assert same_bytes(r["desc"], g["desc"]) and same_bytes(r["kp"], g["kp"]) and BM.same_floats(r["pts"], rec(g))
    chip.frame_put_disparity(1, e, c["disp"], Q)                      # ... by a disparity put
    r = chip.frame_read(1)
    assert chip.frame_store_info()["n_frames"] == 1 and r["n"] == 120 and BM.same_floats(r["pts"], rec(e))
    chip.frame_put_stereo(1, e, c["left"], c["right"], Q, c["params"])   # ... by a stereo put of the same frame: the same records
    assert same_bytes(chip.frame_read(1)["pts"], r["pts"])
    chip.frame_put(1, f)                                              # and back to the image
    r = chip.frame_read(1)
    assert chip.frame_store_info()["n_frames"] == 1 and r["n"] == 300 and same_bytes(r["kp"], f["kp"])
    chip.frame_put_stereo(2, dict(desc=g["desc"][:0], kp=g["kp"][:0]), c["left"], c["right"], Q, c["params"])   # n == 0 is stored
    r = chip.frame_read(2)
    assert (r["n"], r["width"], r["height"]) == (0, w, h) and chip.frame_store_info()["n_frames"] == 2


def test_one_staging_buffer_serves_images_maps_and_pairs_of_any_size(clean):
    """64 x 48 (xyz), 752 x 480 (pair), 43 x 11 (pair), 752 x 480 (map), 100 x 25 (pair) through the one staging buffer and the one
    prefilter buffer, then the dense call through both: what each leaves equals what a fresh ctx gives"""
    chip = clean
    rng = np.random.default_rng(22)
    small = fc.frame(rng, 257, plant_at=(0, 63, 64, 256))
    full = SC.full_frame()
    ff = frame_of(rng, 600, *SC.FULL, 64, 21)
    c3, c0 = put_image(3), put_image(0)
    f3, f0 = frame_of(rng, 100, *PUT_SHAPES[3]), frame_of(rng, 100, *PUT_SHAPES[0])
    steps = (("xyz", 1, small, None), ("pair", 2, ff, full), ("pair", 3, f3, c3), ("map", 4, ff, full), ("pair", 10, f0, c0))

    def run(c, step):
        how, i, f, src = step
        if how == "xyz":
            c.frame_put(i, f)
        elif how == "pair":
            c.frame_put_stereo(i, f, src["left"], src["right"], Q, src["params"])
        else:
            c.frame_put_disparity(i, f, mirror_map("full"), Q)
        return c.frame_read(i)["pts"]

    got = [run(chip, s) for s in steps]
    dense = chip.stereo_bm(c3["left"], c3["right"], c3["params"])
    again = [chip.frame_read(s[1])["pts"] for s in steps]            # later puts and the dense call left the earlier slots alone
    with capi.Chip(4096) as c:                                        # a ctx that ran nothing else (its buffers grow at every step)
        c.frame_store_reserve(5, SLOT_KP)
        fresh = [run(c, s) for s in reversed(steps)][::-1]
    for s, g, a, fr in zip(steps, got, again, fresh):
        assert BM.same_floats(g, fr) and BM.same_floats(a, fr), s[:2]
    assert same_bytes(got[1], got[3])                                 # the 752 x 480 frame: pair and map give the same records
    assert np.array_equal(dense, c3["disp"])
    with capi.Chip(4096) as c:                                        # the dense call needs no store
        assert c.frame_store_info()["n_slots"] == 0 and np.array_equal(c.stereo_bm(c3["left"], c3["right"], c3["params"]), dense)


# ---------------------------------------------------------------------------------------------- 6: status codes
def test_status_codes(clean):
    chip = clean
    rng = np.random.default_rng(23)
    c = put_image(0)
    w, h, nd, block = PUT_SHAPES[0]
    f = frame_of(rng, 40, w, h, nd, block)
    Qv = np.ascontiguousarray(Q).reshape(16)
    desc, kp, left, right = (np.ascontiguousarray(a) for a in (f["desc"], f["kp"], c["left"], c["right"]))
    ptr = lambda a: None if a is None else capi._ptr(a)             # noqa: E731
    raw = lambda hd, l=left, r=right, q=Qv, p=None: chip.lib.chip_frame_put_stereo(hd, 1, ptr(desc), ptr(kp), 40, w, h, ptr(l), ptr(r), p, ptr(q))   # noqa: E731
    chip.frame_put_stereo(1, f, left, right, Q, c["params"])
    before = chip.frame_read(1)
    assert raw(None) == capi.CHIP_ERR_INVALID_ARG
    assert raw(chip.h, l=None) == raw(chip.h, r=None) == raw(chip.h, q=None) == capi.CHIP_ERR_INVALID_ARG
    for field, v in (("num_disparities", 24), ("num_disparities", 80), ("block_size", 3), ("block_size", 20), ("block_size", 23), ("prefilter_cap", 0),
                     ("prefilter_cap", 64), ("texture_threshold", -1), ("uniqueness_ratio", -1), ("uniqueness_ratio", 101)):
        assert raw(chip.h, p=C.byref(capi.default_stereo_bm_params(**{field: v}))) == capi.CHIP_ERR_UNSUPPORTED, (field, v)
        assert status_of(chip.stereo_bm, left, right, {field: v}) == capi.CHIP_ERR_UNSUPPORTED, (field, v)
    wide = frame_of(rng, SLOT_KP + 1, w, h, nd, block)
    assert status_of(chip.frame_put_stereo, 1, wide, left, right, Q) == capi.CHIP_ERR_UNSUPPORTED        # more keypoints than a slot holds
    big = np.zeros((2, 16385), np.uint8)
    assert status_of(chip.frame_put_stereo, 1, f, big, big, Q) == capi.CHIP_ERR_UNSUPPORTED
    assert status_of(chip.stereo_bm, big, big) == status_of(chip.stereo_bm, big.T, big.T) == capi.CHIP_ERR_UNSUPPORTED
    after = chip.frame_read(1)                                        # a failed put leaves the store as it was
    assert all(same_bytes(before[k], after[k]) for k in ("desc", "kp", "pts")) and chip.frame_store_info()["n_frames"] == 1
    # every accepted bound of the parameter table is accepted, and gives the mirror's map
    for kw in (dict(num_disparities=16, block_size=5, prefilter_cap=1, texture_threshold=0, uniqueness_ratio=0),
               dict(num_disparities=64, block_size=21, prefilter_cap=63, texture_threshold=2 ** 31 - 1, uniqueness_ratio=100),
               dict(num_disparities=32, block_size=19, prefilter_cap=63, texture_threshold=500, uniqueness_ratio=1)):
        assert np.array_equal(chip.stereo_bm(left, right, kw), BM.vectorised(left, right, BM.params(**kw))), kw
    # a full store: OOM, nothing evicted; a replace needs no free slot
    tiny = frame_of(rng, 5, w, h, nd, block)
    for i in range(10, 10 + N_SLOTS - 1):
        chip.frame_put_stereo(i, tiny, left, right, Q, c["params"])
    assert chip.frame_store_info()["n_frames"] == N_SLOTS
    assert status_of(chip.frame_put_stereo, 2, tiny, left, right, Q, c["params"]) == capi.CHIP_ERR_OOM
    assert chip.frame_store_info()["n_frames"] == N_SLOTS and status_of(chip.frame_read, 2) == capi.CHIP_ERR_RANGE
    chip.frame_put_stereo(10, f, left, right, Q, c["params"])
    assert same_bytes(chip.frame_read(10)["pts"], before["pts"])
    chip.frame_drop(11)
    chip.frame_put_stereo(2, tiny, left, right, Q, c["params"])
    # the dense call
    out = np.zeros((h, w), np.int16)
    bm = lambda hd, l, r, ww, hh, o: chip.lib.chip_stereo_bm(hd, l, r, ww, hh, C.byref(capi.default_stereo_bm_params(**c["params"])), o)   # noqa: E731
    lp, rp, op = capi._ptr(left), capi._ptr(right), capi._ptr(out)
    assert bm(chip.h, lp, rp, w, h, op) == capi.CHIP_OK and np.array_equal(out, c["disp"])
    assert bm(None, lp, rp, w, h, op) == bm(chip.h, None, rp, w, h, op) == bm(chip.h, lp, None, w, h, op) == bm(chip.h, lp, rp, w, h, None) == capi.CHIP_ERR_INVALID_ARG
    assert bm(chip.h, lp, rp, 0, h, op) == bm(chip.h, lp, rp, w, -1, op) == capi.CHIP_ERR_INVALID_ARG
    assert bm(chip.h, lp, rp, 16385, 1, op) == bm(chip.h, lp, rp, 1, 16385, op) == capi.CHIP_ERR_UNSUPPORTED


def test_before_a_reserve_and_on_a_group_ctx():
    rng = np.random.default_rng(24)
    c = put_image(1)
    w, h, nd, block = PUT_SHAPES[1]
    f = frame_of(rng, 40, w, h, nd, block)
    with capi.Chip(4096) as ctx:
        assert status_of(ctx.frame_put_stereo, 1, f, c["left"], c["right"], Q, c["params"]) == capi.CHIP_ERR_BUSY
        ctx.frame_store_reserve(2, 64)
        assert status_of(ctx.frame_put_stereo, 1, frame_of(rng, 65, w, h, nd, block), c["left"], c["right"], Q, c["params"]) == capi.CHIP_ERR_UNSUPPORTED
        ctx.frame_put_stereo(1, f, c["left"], c["right"], Q, c["params"])
        assert BM.same_floats(ctx.frame_read(1)["pts"], BM.records(f["kp"], None, None, None, Q, disp=c["disp"]))
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.frame_put_stereo, 1, f, c["left"], c["right"], Q, c["params"]) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.stereo_bm, c["left"], c["right"], c["params"]) == capi.CHIP_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 7: first use next to a resident scan
@pytest.mark.parametrize("first", ["dense", "put"])
def test_resident_tick_mode_allocates_inside_a_pause(monkeypatch, first):
    """with CHIP_TICK_RESIDENT=1 the first use of either call -- the stage's buffers, the staging buffer, the prefiltered pair, the
    dense map -- happens next to a resident scan instance: same values"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    c = put_image(2)
    w, h, nd, block = PUT_SHAPES[2]
    f = frame_of(np.random.default_rng(25), 300, w, h, nd, block)
    with capi.Chip(4096) as ctx:
        ctx.append_synthetic(400, 5)
        ticks = scenarios.default_schedule(400)
        for l in ticks[:8]:
            ctx.loop_tick(l)
        if first == "dense":
            dense = ctx.stereo_bm(c["left"], c["right"], c["params"])
            ctx.loop_tick(ticks[8])
            ctx.frame_store_reserve(2, 512)
            ctx.frame_put_stereo(1, f, c["left"], c["right"], Q, c["params"])
        else:
            ctx.frame_store_reserve(2, 512)
            ctx.frame_put_stereo(1, f, c["left"], c["right"], Q, c["params"])
            ctx.loop_tick(ticks[8])
            dense = ctx.stereo_bm(c["left"], c["right"], c["params"])
        pts = ctx.frame_read(1)["pts"]
        ctx.loop_tick(400)
    assert np.array_equal(dense, c["disp"])
    assert BM.same_floats(pts, BM.records(f["kp"], None, None, None, Q, disp=c["disp"]))


# ---------------------------------------------------------------------------------------------- 8: the example
def test_frame_put_stereo_example():
    exe = LIB / "frame_put_stereo"
    assert exe.exists()
    r = subprocess.run([str(exe), "1500", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== the same frames put through chip_frame_put_disparity") == 4 and "DIFFERS" not in r.stdout
