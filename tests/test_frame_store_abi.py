"""The frame store (chip_frame_store_reserve / _info, chip_frame_put / _drop / _read, chip_match_batch_stored) at the drop-in boundary,
without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built library, bound by the ctypes table, and bad
arguments are status codes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_frame_store", "chip_frame_store_reserve", "chip_frame_store_info", "chip_frame_put", "chip_frame_drop",
         "chip_frame_read", "chip_match_batch_stored")


def test_header_declares_the_seven_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive


def test_library_exports_them_and_reports_the_store(chip_lib):
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
    assert chip_lib.chip_build_has_frame_store() == 1
    assert chip_lib.chip_abi_version() == 7


def test_invalid_arguments_are_status_codes(chip_lib):
    lib = chip_lib
    bad = capi.CHIP_ERR_INVALID_ARG
    v = C.c_int32()
    assert lib.chip_frame_store_reserve(None, 4, 1024) == bad
    assert lib.chip_frame_store_info(None, C.byref(v), C.byref(v), C.byref(v)) == bad
    assert lib.chip_frame_drop(None, 1) == bad
    assert lib.chip_frame_read(None, 1, C.byref(v), None, None, None, None, None) == bad
    ids = np.array([1, 2], np.int64)
    Ki = np.eye(3).reshape(9)
    sm = (capi.MatchSummary * 2)()
    assert lib.chip_match_batch_stored(None, 0, capi._ptr(ids), 2, capi._ptr(Ki), sm) == bad
    desc = np.zeros((4, 32), np.uint8); kp = np.zeros((4, 2), np.float32); xyz = np.zeros((3, 5, 3), np.float32)
    f = capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, 4, 5, 3, xyz.ctypes.data)
    assert lib.chip_frame_put(None, 1, C.byref(f)) == bad
    # the frame rules come before anything that needs a ctx's device: a fake non-null handle is never dereferenced for these
    fake = C.c_void_p(8)
    assert lib.chip_frame_put(fake, 1, None) == bad
    for broken in (capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, 4, 5, 3, None), capi.MatchFrame(None, kp.ctypes.data, 4, 5, 3, xyz.ctypes.data),
                   capi.MatchFrame(desc.ctypes.data, None, 4, 5, 3, xyz.ctypes.data), capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, -1, 5, 3, xyz.ctypes.data),
                   capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, 4, 0, 3, xyz.ctypes.data)):
        assert lib.chip_frame_put(fake, 1, C.byref(broken)) == bad
    big = capi.MatchFrame(desc.ctypes.data, kp.ctypes.data, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, 5, 3, xyz.ctypes.data)
    assert lib.chip_frame_put(fake, 1, C.byref(big)) == capi.CHIP_ERR_UNSUPPORTED
    for n_slots, slot_kp in ((0, 1024), (-1, 1024), (4, 0), (4, capi.CHIP_MATCH_MAX_KEYPOINTS + 1)):
        assert lib.chip_frame_store_reserve(fake, n_slots, slot_kp) == bad
