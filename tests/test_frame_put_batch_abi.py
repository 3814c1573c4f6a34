"""The batched frame puts (chip_build_has_frame_put_batch, chip_frame_put_plan, chip_frame_put_orb_stereo_batch,
chip_frame_put_raw_orb_stereo_batch, chip_frame_put_records, chip_debug_frame_put_last) at the drop-in boundary, without a GPU: declared
in include/cerebro_hip.h next to ABI 7, exported by the built library, bound by the ctypes table; chip_frame_put_plan -- which needs
neither a ctx nor a device -- gives the groups the header states; every status that needs no device is a status code."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_frame_put_batch", "chip_frame_put_plan", "chip_frame_put_orb_stereo_batch", "chip_frame_put_raw_orb_stereo_batch",
         "chip_frame_put_records", "chip_debug_frame_put_last")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
P, I32 = C.c_void_p, C.c_int32
FAKE = C.c_void_p(8)           # a handle that is never dereferenced: everything here is decided before anything touches a ctx
MAX_PUT = 256


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    flat = re.sub(r"[ \t]+", " ", raw)
    assert "#define CHIP_ABI_VERSION 7" in flat and f"#define CHIP_FRAME_MAX_PUT {MAX_PUT}" in flat   # additive


def test_library_exports_them_with_their_argument_rows(chip_lib):
    batch = [P, P, I32, I32, I32, P, P, C.POINTER(capi.OrbParams), C.POINTER(capi.StereoBmParams), P, P]
    rows = {"chip_build_has_frame_put_batch": [], "chip_frame_put_plan": [I32, I32, C.POINTER(capi.OrbParams), I32, I32, C.POINTER(I32), C.POINTER(I32)],
            "chip_frame_put_orb_stereo_batch": batch, "chip_frame_put_raw_orb_stereo_batch": batch,
            "chip_frame_put_records": [P, C.c_int64, P, P, P, I32, I32, I32],
            "chip_debug_frame_put_last": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)]}
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
        fn = getattr(chip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rows[name], name
    assert chip_lib.chip_build_has_frame_put_batch() == 1 and chip_lib.chip_abi_version() == 7


@pytest.mark.parametrize("size, group", (((160, 120), 16), ((752, 480), 16), ((1024, 768), 10), ((4096, 4096), 1), ((724, 724), 16), ((725, 724), 15)))
def test_plan_gives_the_groups_the_header_states(chip_lib, size, group):
    w, h = size
    assert group == max(1, min(16, 2 ** 23 // (w * h)))                        # level-0 pixels of a group <= 2^23, at most 16, at least 1
    for F in (1, 16, 17, MAX_PUT):
        for raw in (False, True):
            assert capi.frame_put_plan(w, h, F, raw=raw) == dict(group=group, n_groups=-(-F // group)), (F, raw)
    assert capi.frame_put_plan(w, h, 17, dict(n_levels=1, n_features=50))["group"] == group   # the parameters do not move it


def test_plan_statuses(chip_lib):
    plan = chip_lib.chip_frame_put_plan
    g, n = I32(-7), I32(-7)
    pg, pn = C.byref(g), C.byref(n)
    assert plan(160, 120, None, 0, 0, pg, pn) == plan(160, 120, None, 0, -1, pg, pn) == BAD
    assert plan(160, 120, None, 0, MAX_PUT + 1, pg, pn) == UNSUPPORTED
    assert plan(160, 120, None, 0, MAX_PUT, pg, pn) == capi.CHIP_OK and (g.value, n.value) == (16, 16)
    g.value = n.value = -7
    assert plan(160, 120, None, 0, 4, None, pn) == plan(160, 120, None, 0, 4, pg, None) == plan(160, 120, None, 2, 4, pg, pn) == BAD
    for w, h in ((0, 120), (160, 0), (-1, 120)):
        assert plan(w, h, None, 0, 4, pg, pn) == BAD
    assert plan(4097, 120, None, 0, 4, pg, pn) == plan(160, 4097, None, 1, 4, pg, pn) == UNSUPPORTED
    for field, v in (("n_features", 0), ("n_levels", 9), ("fast_threshold", 256), ("border", 15)):
        assert plan(160, 120, C.byref(capi.default_orb_params(**{field: v})), 0, 4, pg, pn) == UNSUPPORTED, (field, v)
    assert (g.value, n.value) == (-7, -7)
    with pytest.raises(capi.ChipError) as e:
        capi.frame_put_plan(160, 120, 0)
    assert e.value.status == BAD


@pytest.mark.parametrize("name", ("chip_frame_put_orb_stereo_batch", "chip_frame_put_raw_orb_stereo_batch"))
def test_batch_put_statuses_that_need_no_device(chip_lib, name):
    put = getattr(chip_lib, name)
    F = 3
    imgs = [np.zeros((70, 80), np.uint8) for _ in range(2 * F)]
    ids = np.arange(1, F + 1, dtype=np.int64)
    left = (C.c_void_p * F)(*[a.ctypes.data for a in imgs[:F]])
    right = (C.c_void_p * F)(*[a.ctypes.data for a in imgs[F:]])
    Q = np.eye(4).reshape(16)
    n = np.full(F, -7, np.int32)
    i, q, pn = capi._ptr(ids), capi._ptr(Q), capi._ptr(n)
    assert put(None, i, F, 80, 70, left, right, None, None, q, pn) == BAD
    assert put(FAKE, None, F, 80, 70, left, right, None, None, q, pn) == BAD
    assert put(FAKE, i, F, 80, 70, None, right, None, None, q, pn) == put(FAKE, i, F, 80, 70, left, None, None, None, q, pn) == BAD
    assert put(FAKE, i, F, 80, 70, left, right, None, None, None, pn) == put(FAKE, i, F, 80, 70, left, right, None, None, q, None) == BAD
    assert put(FAKE, i, 0, 80, 70, left, right, None, None, q, pn) == put(FAKE, i, -1, 80, 70, left, right, None, None, q, pn) == BAD
    hole = (C.c_void_p * F)(imgs[0].ctypes.data, None, imgs[2].ctypes.data)
    assert put(FAKE, i, F, 80, 70, hole, right, None, None, q, pn) == put(FAKE, i, F, 80, 70, left, hole, None, None, q, pn) == BAD
    twice = np.array([5, 6, 5], dtype=np.int64)
    assert put(FAKE, capi._ptr(twice), F, 80, 70, left, right, None, None, q, pn) == BAD       # an id that repeats inside the call
    many = np.arange(MAX_PUT + 1, dtype=np.int64)
    lm = (C.c_void_p * (MAX_PUT + 1))(*[imgs[0].ctypes.data] * (MAX_PUT + 1))
    nm = np.full(MAX_PUT + 1, -7, np.int32)
    assert put(FAKE, capi._ptr(many), MAX_PUT + 1, 80, 70, lm, lm, None, None, q, capi._ptr(nm)) == UNSUPPORTED
    for w, h in ((0, 70), (80, 0), (-1, 70)):
        assert put(FAKE, i, F, w, h, left, right, None, None, q, pn) == BAD
    assert put(FAKE, i, F, 4097, 70, left, right, None, None, q, pn) == put(FAKE, i, F, 80, 4097, left, right, None, None, q, pn) == UNSUPPORTED
    for field, v in (("n_features", 0), ("n_levels", 9), ("fast_threshold", 256), ("border", 15)):
        assert put(FAKE, i, F, 80, 70, left, right, C.byref(capi.default_orb_params(**{field: v})), None, q, pn) == UNSUPPORTED, (field, v)
    for field, v in (("num_disparities", 24), ("block_size", 4), ("prefilter_cap", 64), ("texture_threshold", -1), ("uniqueness_ratio", 101)):
        assert put(FAKE, i, F, 80, 70, left, right, None, C.byref(capi.default_stereo_bm_params(**{field: v})), q, pn) == UNSUPPORTED, (field, v)
    assert (n == -7).all() and (nm == -7).all()


def test_records_put_and_debug_statuses_that_need_no_device(chip_lib):
    put = chip_lib.chip_frame_put_records
    desc, kp = np.zeros((4, 32), np.uint8), np.zeros((4, 2), np.float32)
    pts = np.zeros((4, 4), np.float32)
    pts[:, 3] = (0.0, 1.0, 1.0, 0.0)
    d, k, p = capi._ptr(desc), capi._ptr(kp), capi._ptr(pts)
    assert put(None, 1, d, k, p, 4, 80, 70) == BAD
    assert put(FAKE, 1, None, k, p, 4, 80, 70) == put(FAKE, 1, d, None, p, 4, 80, 70) == put(FAKE, 1, d, k, None, 4, 80, 70) == BAD
    assert put(FAKE, 1, d, k, None, 0, 80, 70) == BAD                                          # the records stand where chip_frame_put has its image
    assert put(FAKE, 1, d, k, p, -1, 80, 70) == put(FAKE, 1, d, k, p, 4, 0, 70) == put(FAKE, 1, d, k, p, 4, 80, 0) == BAD
    assert put(FAKE, 1, d, k, p, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, 80, 70) == put(FAKE, 1, d, k, p, 4, 16385, 70) == UNSUPPORTED
    for v in (0.5, 2.0, -1.0, float("nan"), -0.0, np.float32(1.0) + np.finfo(np.float32).eps):
        bad = pts.copy()
        bad[2, 3] = v
        assert put(FAKE, 1, d, k, capi._ptr(bad), 4, 80, 70) == BAD, v                         # only the 0.0f / 1.0f the gather kernels write
    assert chip_lib.chip_debug_frame_put_last(None, None, None, None) == BAD
