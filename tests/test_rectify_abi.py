"""The rectification (chip_build_has_rectify, chip_rectify_quantize, chip_remap, chip_rectify_set_maps, chip_rectify_pair,
chip_frame_put_raw_orb_stereo) at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by
the built library, bound by the ctypes table; chip_rectify_quantize -- which needs neither a ctx nor a device -- is the quantiser of
the numpy restatement; every status that needs no device is a status code."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import np_mirror_rectify as R
import rectify_cases as RC
from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_rectify", "chip_rectify_quantize", "chip_remap", "chip_rectify_set_maps", "chip_rectify_pair",
         "chip_frame_put_raw_orb_stereo")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
P, I32 = C.c_void_p, C.c_int32
FAKE = C.c_void_p(8)           # a handle that is never dereferenced: everything here is decided before anything touches a ctx


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive
    assert "UNPINNED" in raw.split("a frame from its raw stereo pair")[1].split("chip_build_has_rectify")[0]


def test_library_exports_them_with_their_argument_rows(chip_lib):
    rows = {"chip_build_has_rectify": [], "chip_rectify_quantize": [P, C.c_int64, P], "chip_remap": [P, P, I32, I32, P, P, P],
            "chip_rectify_set_maps": [P, I32, I32] + [P] * 8, "chip_rectify_pair": [P, P, P, I32, I32, P, P],
            "chip_frame_put_raw_orb_stereo": [P, C.c_int64, I32, I32, P, P, C.POINTER(capi.OrbParams), C.POINTER(capi.StereoBmParams), P,
                                              C.POINTER(I32)]}
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
        fn = getattr(chip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rows[name], name
    assert chip_lib.chip_build_has_rectify() == 1 and chip_lib.chip_build_has_orb_describe() == 1
    assert chip_lib.chip_abi_version() == 7
    assert (1 << capi.CHIP_RECTIFY_FRACTION_BITS, capi.CHIP_RECTIFY_MAP_MIN, capi.CHIP_RECTIFY_MAP_MAX, capi.CHIP_RECTIFY_NAN_Q) == \
        (R.ONE, R.MAP_MIN, R.MAP_MAX, R.NAN_Q)


def test_quantiser_equals_the_mirror(chip_lib):
    e = RC.quantiser_edges()
    got = capi.rectify_quantize(e)
    assert got.dtype == np.int32 and got.tolist() == R.quantize(e).tolist()
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2 ** 32, 50_000, dtype=np.uint64).astype(np.uint32).view(np.float32)   # every exponent, NaNs and infinities
    near = rng.uniform(-4, 800, 50_000).astype(np.float32)
    for v in (bits, near, (np.round(near * 64) / 64).astype(np.float32)):                          # the last: half of them exact ties
        assert np.array_equal(capi.rectify_quantize(v), R.quantize(v))
    m = RC.radtan(31, 17)[0]
    assert capi.rectify_quantize(m).shape == (17, 31)
    assert capi.rectify_quantize(np.zeros(0, np.float32)).size == 0                                # count == 0 is fine
    q = np.zeros(4, np.int32)
    f = np.zeros(4, np.float32)
    assert chip_lib.chip_rectify_quantize(None, 4, capi._ptr(q)) == BAD
    assert chip_lib.chip_rectify_quantize(capi._ptr(f), 4, None) == BAD
    assert chip_lib.chip_rectify_quantize(capi._ptr(f), -1, capi._ptr(q)) == BAD


def test_remap_statuses_that_need_no_device(chip_lib):
    img, out = np.zeros((70, 80), np.uint8), np.full((70, 80), 9, np.uint8)
    mx, my = RC.identity(80, 70)
    i, x, y, o = (capi._ptr(v) for v in (img, mx, my, out))
    remap = chip_lib.chip_remap
    assert remap(None, i, 80, 70, x, y, o) == BAD
    assert remap(FAKE, None, 80, 70, x, y, o) == remap(FAKE, i, 80, 70, None, y, o) == remap(FAKE, i, 80, 70, x, None, o) == BAD
    assert remap(FAKE, i, 80, 70, x, y, None) == BAD
    for w, h in ((0, 70), (80, 0), (-1, 70), (80, -1)):
        assert remap(FAKE, i, w, h, x, y, o) == BAD
    assert remap(FAKE, i, 16385, 70, x, y, o) == remap(FAKE, i, 80, 16385, x, y, o) == UNSUPPORTED   # chip_match_pair's image limit
    assert remap(FAKE, None, 16385, 70, x, y, o) == BAD                                            # the pointers first
    assert (out == 9).all()


def test_set_maps_and_rectify_pair_statuses_that_need_no_device(chip_lib):
    mx, my = RC.identity(80, 70)
    x, y = capi._ptr(mx), capi._ptr(my)
    set_maps = chip_lib.chip_rectify_set_maps
    assert set_maps(None, 80, 70, x, y, x, y, x, y, x, y) == BAD
    for missing in (0, 1, 4, 5):                                                                   # a stage-1 map
        a = [x, y, x, y, x, y, x, y]
        a[missing] = None
        assert set_maps(FAKE, 80, 70, *a) == BAD, missing
    for present in ((2,), (3,), (6,), (7,), (2, 3), (6, 7), (2, 6), (2, 3, 6), (3, 6, 7)):          # a mix of stage-2 maps
        a = [x, y, None, None, x, y, None, None]
        for k in present:
            a[k] = x
        assert set_maps(FAKE, 80, 70, *a) == BAD, present
    for w, h in ((0, 70), (80, 0), (-1, 70), (80, -1)):
        assert set_maps(FAKE, w, h, x, y, x, y, x, y, x, y) == BAD
    assert set_maps(FAKE, capi.CHIP_ORB_MAX_SIDE + 1, 70, x, y, None, None, x, y, None, None) == UNSUPPORTED
    assert set_maps(FAKE, 80, capi.CHIP_ORB_MAX_SIDE + 1, x, y, x, y, x, y, x, y) == UNSUPPORTED
    assert set_maps(FAKE, 4097, 70, x, y, x, None, x, y, x, y) == BAD                              # the pointers first
    img, out = np.zeros((70, 80), np.uint8), np.full((70, 80), 9, np.uint8)
    i, o = capi._ptr(img), capi._ptr(out)
    pair = chip_lib.chip_rectify_pair
    assert pair(None, i, i, 80, 70, o, o) == BAD
    assert pair(FAKE, None, i, 80, 70, o, o) == pair(FAKE, i, None, 80, 70, o, o) == BAD
    assert pair(FAKE, i, i, 80, 70, None, o) == pair(FAKE, i, i, 80, 70, o, None) == BAD
    for w, h in ((0, 70), (80, 0), (-1, 70), (80, -1)):
        assert pair(FAKE, i, i, w, h, o, o) == BAD
    assert (out == 9).all()


def test_raw_put_statuses_that_need_no_device(chip_lib):
    left, right = np.zeros((70, 80), np.uint8), np.zeros((70, 80), np.uint8)
    Q = np.eye(4).reshape(16)
    n = C.c_int32(-7)
    l, r, q, pn = capi._ptr(left), capi._ptr(right), capi._ptr(Q), C.byref(n)
    put = chip_lib.chip_frame_put_raw_orb_stereo
    assert put(None, 1, 80, 70, l, r, None, None, q, pn) == BAD
    assert put(FAKE, 1, 80, 70, None, r, None, None, q, pn) == put(FAKE, 1, 80, 70, l, None, None, None, q, pn) == BAD
    assert put(FAKE, 1, 80, 70, l, r, None, None, None, pn) == put(FAKE, 1, 80, 70, l, r, None, None, q, None) == BAD
    for w, h in ((0, 70), (80, 0), (-1, 70)):
        assert put(FAKE, 1, w, h, l, r, None, None, q, pn) == BAD
    assert put(FAKE, 1, 4097, 70, l, r, None, None, q, pn) == put(FAKE, 1, 80, 4097, l, r, None, None, q, pn) == UNSUPPORTED
    for field, v in (("n_features", 0), ("n_levels", 9), ("fast_threshold", 256), ("border", 15)):
        assert put(FAKE, 1, 80, 70, l, r, C.byref(capi.default_orb_params(**{field: v})), None, q, pn) == UNSUPPORTED, (field, v)
    for field, v in (("num_disparities", 24), ("block_size", 4), ("prefilter_cap", 64), ("texture_threshold", -1), ("uniqueness_ratio", 101)):
        assert put(FAKE, 1, 80, 70, l, r, None, C.byref(capi.default_stereo_bm_params(**{field: v})), q, pn) == UNSUPPORTED, (field, v)
    assert n.value == -7
