"""A frame from its disparity map (chip_build_has_disparity, chip_frame_put_disparity, chip_disparity_to_xyz) at the drop-in boundary,
without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built library, bound by the ctypes table, and every
status that needs no device is a status code."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_disparity", "chip_frame_put_disparity", "chip_disparity_to_xyz")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED


def test_header_declares_the_three_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert re.search(r"enum\s*\{\s*CHIP_DISP_S16\s*=\s*0\s*,\s*CHIP_DISP_F32\s*=\s*1\s*\}", text)
    assert (capi.CHIP_DISP_S16, capi.CHIP_DISP_F32) == (0, 1)
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive


def test_library_exports_them(chip_lib):
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
    assert chip_lib.chip_build_has_disparity() == 1
    assert chip_lib.chip_abi_version() == 7


def test_put_statuses_that_need_no_device(chip_lib):
    lib = chip_lib
    desc = np.zeros((4, 32), np.uint8); kp = np.zeros((4, 2), np.float32); disp = np.zeros((3, 5), np.int16); Q = np.eye(4).reshape(16)
    d, k, s, q = capi._ptr(desc), capi._ptr(kp), capi._ptr(disp), capi._ptr(Q)
    put = lib.chip_frame_put_disparity
    assert put(None, 1, d, k, 4, 5, 3, s, capi.CHIP_DISP_S16, q) == BAD
    # the frame rules and the two new ones come before anything that needs a ctx's device: a fake handle is never dereferenced
    fake = C.c_void_p(8)
    assert put(fake, 1, d, k, 4, 5, 3, None, capi.CHIP_DISP_S16, q) == BAD      # the disparity stands where xyz stood
    assert put(fake, 1, None, k, 4, 5, 3, s, capi.CHIP_DISP_S16, q) == BAD
    assert put(fake, 1, d, None, 4, 5, 3, s, capi.CHIP_DISP_S16, q) == BAD
    assert put(fake, 1, d, k, -1, 5, 3, s, capi.CHIP_DISP_S16, q) == BAD
    assert put(fake, 1, d, k, 4, 0, 3, s, capi.CHIP_DISP_S16, q) == BAD
    assert put(fake, 1, d, k, 4, 5, 0, s, capi.CHIP_DISP_S16, q) == BAD
    assert put(fake, 1, None, None, 0, 5, 0, s, capi.CHIP_DISP_S16, q) == BAD
    for kind in (-1, 2, 16):
        assert put(fake, 1, d, k, 4, 5, 3, s, kind, q) == BAD                    # an unknown disp_type
    assert put(fake, 1, d, k, 4, 5, 3, s, capi.CHIP_DISP_F32, None) == BAD       # a NULL Q
    assert put(fake, 1, d, k, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, 5, 3, s, capi.CHIP_DISP_S16, q) == UNSUPPORTED
    assert put(fake, 1, d, k, 4, 16385, 3, s, capi.CHIP_DISP_S16, q) == UNSUPPORTED
    assert put(fake, 1, d, k, 4, 5, 16385, s, capi.CHIP_DISP_S16, q) == UNSUPPORTED


def test_dense_statuses_that_need_no_device(chip_lib):
    lib = chip_lib
    disp = np.zeros((3, 5), np.float32); Q = np.eye(4).reshape(16); out = np.zeros((3, 5, 3), np.float32)
    s, q, o = capi._ptr(disp), capi._ptr(Q), capi._ptr(out)
    dense = lib.chip_disparity_to_xyz
    assert dense(None, s, capi.CHIP_DISP_F32, 5, 3, q, o) == BAD
    fake = C.c_void_p(8)
    assert dense(fake, None, capi.CHIP_DISP_F32, 5, 3, q, o) == BAD
    assert dense(fake, s, capi.CHIP_DISP_F32, 5, 3, None, o) == BAD
    assert dense(fake, s, capi.CHIP_DISP_F32, 5, 3, q, None) == BAD
    for w, h in ((0, 3), (5, 0), (-1, 3), (5, -1)):
        assert dense(fake, s, capi.CHIP_DISP_F32, w, h, q, o) == BAD
    for kind in (-1, 2):
        assert dense(fake, s, kind, 5, 3, q, o) == BAD
    assert dense(fake, s, capi.CHIP_DISP_F32, 16385, 3, q, o) == UNSUPPORTED     # the limits check_frame applies to an image
    assert dense(fake, s, capi.CHIP_DISP_F32, 5, 16385, q, o) == UNSUPPORTED
    assert not out.any()
