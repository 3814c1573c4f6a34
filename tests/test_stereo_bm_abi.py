"""A frame from its rectified stereo pair (chip_stereo_bm_params_default, chip_build_has_stereo_bm, chip_stereo_bm,
chip_frame_put_stereo) at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built
library, bound by the ctypes table, and every status that needs no device is a status code."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_stereo_bm_params_default", "chip_build_has_stereo_bm", "chip_stereo_bm", "chip_frame_put_stereo")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
DEFAULTS = dict(num_disparities=64, block_size=21, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=15)
# field -> values just outside the accepted set, at both bounds (and between two accepted values)
REFUSED = dict(num_disparities=(15, 0, -16, 17, 24, 63, 65, 80, 128), block_size=(3, 4, 6, 20, 22, 23, -21), prefilter_cap=(0, 64, -1),
               texture_threshold=(-1, -(2 ** 31)), uniqueness_ratio=(-1, 101))


def test_header_declares_the_four_entries_the_struct_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bvoid\s+chip_stereo_bm_params_default\s*\(", text)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*chip_stereo_bm_params\s*;", text).group(1)
    assert re.findall(r"int32_t\s+(\w+)\s*;", body) == list(DEFAULTS)
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive


def test_struct_size_and_defaults(chip_lib):
    assert C.sizeof(capi.StereoBmParams) == 20
    assert [n for n, _ in capi.StereoBmParams._fields_] == list(DEFAULTS)
    p = capi.default_stereo_bm_params()
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    assert (capi.CHIP_STEREO_BM_NUM_DISPARITIES, capi.CHIP_STEREO_BM_BLOCK_SIZE, capi.CHIP_STEREO_BM_PREFILTER_CAP,
            capi.CHIP_STEREO_BM_TEXTURE_THRESHOLD, capi.CHIP_STEREO_BM_UNIQUENESS_RATIO) == tuple(DEFAULTS.values())
    chip_lib.chip_stereo_bm_params_default(None)                                  # a NULL is left alone


def test_library_exports_them(chip_lib):
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
    assert chip_lib.chip_build_has_stereo_bm() == 1
    assert chip_lib.chip_abi_version() == 7


def test_put_statuses_that_need_no_device(chip_lib):
    lib = chip_lib
    desc = np.zeros((4, 32), np.uint8); kp = np.zeros((4, 2), np.float32); Q = np.eye(4).reshape(16)
    left = np.zeros((3, 5), np.uint8); right = np.zeros((3, 5), np.uint8)
    d, k, l, r, q = capi._ptr(desc), capi._ptr(kp), capi._ptr(left), capi._ptr(right), capi._ptr(Q)
    put = lib.chip_frame_put_stereo
    assert put(None, 1, d, k, 4, 5, 3, l, r, None, q) == BAD
    # the frame rules and the new ones come before anything that needs a ctx's device: a fake handle is never dereferenced
    fake = C.c_void_p(8)
    assert put(fake, 1, d, k, 4, 5, 3, None, r, None, q) == BAD                   # the left image stands where xyz stood
    assert put(fake, 1, d, k, 4, 5, 3, l, None, None, q) == BAD
    assert put(fake, 1, d, k, 4, 5, 3, l, r, None, None) == BAD                   # a NULL Q
    assert put(fake, 1, None, k, 4, 5, 3, l, r, None, q) == BAD
    assert put(fake, 1, d, None, 4, 5, 3, l, r, None, q) == BAD
    assert put(fake, 1, d, k, -1, 5, 3, l, r, None, q) == BAD
    assert put(fake, 1, d, k, 4, 0, 3, l, r, None, q) == BAD
    assert put(fake, 1, d, k, 4, 5, 0, l, r, None, q) == BAD
    assert put(fake, 1, d, k, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, 5, 3, l, r, None, q) == UNSUPPORTED
    assert put(fake, 1, d, k, 4, 16385, 3, l, r, None, q) == UNSUPPORTED
    assert put(fake, 1, d, k, 4, 5, 16385, l, r, None, q) == UNSUPPORTED
    for field, values in REFUSED.items():
        for v in values:
            p = capi.default_stereo_bm_params(**{field: v})
            assert put(fake, 1, d, k, 4, 5, 3, l, r, C.byref(p), q) == UNSUPPORTED, (field, v)
            assert put(fake, 1, d, k, 4, 5, 3, l, None, C.byref(p), q) == BAD, (field, v)      # the pointers first


def test_dense_statuses_that_need_no_device(chip_lib):
    lib = chip_lib
    left = np.zeros((3, 5), np.uint8); right = np.zeros((3, 5), np.uint8); out = np.zeros((3, 5), np.int16)
    l, r, o = capi._ptr(left), capi._ptr(right), capi._ptr(out)
    bm = lib.chip_stereo_bm
    assert bm(None, l, r, 5, 3, None, o) == BAD
    fake = C.c_void_p(8)
    assert bm(fake, None, r, 5, 3, None, o) == BAD
    assert bm(fake, l, None, 5, 3, None, o) == BAD
    assert bm(fake, l, r, 5, 3, None, None) == BAD
    for w, h in ((0, 3), (5, 0), (-1, 3), (5, -1)):
        assert bm(fake, l, r, w, h, None, o) == BAD
    assert bm(fake, l, r, 16385, 3, None, o) == UNSUPPORTED                       # the limits check_frame applies to an image
    assert bm(fake, l, r, 5, 16385, None, o) == UNSUPPORTED
    for field, values in REFUSED.items():
        for v in values:
            p = capi.default_stereo_bm_params(**{field: v})
            assert bm(fake, l, r, 5, 3, C.byref(p), o) == UNSUPPORTED, (field, v)
    assert not out.any()
