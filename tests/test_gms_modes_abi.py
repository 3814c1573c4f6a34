"""CPU-side checks of the additive ABI of GMS with scale / rotation (include/cerebro_hip.h): the four new symbols, the layout of
chip_gms_choice, ABI 7 unchanged, and the argument checks that answer before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
NEW = ("chip_build_has_gms_modes", "chip_gms_filter_modes", "chip_match_batch_modes", "chip_match_batch_stored_modes")


def test_new_symbols_and_struct_layout(chip_lib):
    for s in NEW:
        assert hasattr(chip_lib, s) and s in capi.declared_symbols()
    assert chip_lib.chip_build_has_gms_modes() == 1
    assert chip_lib.chip_abi_version() == 7
    assert C.sizeof(capi.GmsChoice) == 172 == 4 * (3 + 5 * 8)
    assert capi.GmsChoice.counts.offset == 12
    assert (capi.CHIP_GMS_WITH_SCALE, capi.CHIP_GMS_WITH_ROTATION) == (1, 2)


def filter_args(modes, kp1=True, kp2=True, q=True, t=True, inlier=True, n_inliers=True):
    kp = np.zeros((4, 2), np.float32)
    idx = np.zeros(4, np.int32)
    mask = np.zeros(4, np.uint8)
    cnt = C.c_int32()
    keep = (kp, idx, mask, cnt)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
    return keep, [p(kp, kp1), 4, 752, 480, p(kp, kp2), 4, 752, 480, p(idx, q), p(idx, t), 4, modes, p(mask, inlier),
                  C.byref(cnt) if n_inliers else None, None]


def test_gms_filter_modes_refuses_bad_arguments_before_touching_the_ctx(chip_lib):
    """the argument checks come first: a ctx that is only a block of zero bytes is never looked into"""
    ctx = C.create_string_buffer(1 << 16)
    h = C.cast(ctx, C.c_void_p)
    for modes in (4, 8, 7, 0x80000001):
        keep, a = filter_args(modes)
        assert chip_lib.chip_gms_filter_modes(h, *a) == capi.CHIP_ERR_INVALID_ARG, modes
    for missing in ("kp1", "kp2", "q", "t", "inlier", "n_inliers"):
        for modes in (0, 1, 2, 3):
            keep, a = filter_args(modes, **{missing: False})
            assert chip_lib.chip_gms_filter_modes(h, *a) == capi.CHIP_ERR_INVALID_ARG, (missing, modes)
    keep, a = filter_args(3)
    assert chip_lib.chip_gms_filter_modes(None, *a) == capi.CHIP_ERR_INVALID_ARG


def test_batch_calls_refuse_a_null_ctx(chip_lib):
    Ki = np.eye(3).reshape(9)
    sm = (capi.MatchSummary * 1)()
    ids = np.zeros(1, np.int64)
    for modes in (0, 3, 4):
        assert chip_lib.chip_match_batch_modes(None, None, None, 1, Ki.ctypes.data_as(C.c_void_p), modes, sm, None) == capi.CHIP_ERR_INVALID_ARG
        assert chip_lib.chip_match_batch_stored_modes(None, 1, ids.ctypes.data_as(C.c_void_p), 1, Ki.ctypes.data_as(C.c_void_p), modes, sm,
                                                      None) == capi.CHIP_ERR_INVALID_ARG
