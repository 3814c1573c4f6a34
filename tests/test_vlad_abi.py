"""The NetVLAD pooling (chip_build_has_vlad, chip_vlad_set, chip_vlad_clear, chip_vlad_info, chip_vlad, chip_db_append_vlad_f32,
chip_debug_vlad_stage) at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built
library, bound by the ctypes table; every status that is decided before a ctx is touched is a status code, in the stated order."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_vlad", "chip_vlad_set", "chip_vlad_clear", "chip_vlad_info", "chip_vlad", "chip_db_append_vlad_f32",
         "chip_debug_vlad_stage")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
FAKE = C.c_void_p(8)           # a handle that is never dereferenced: everything here is decided before anything touches a ctx


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive
    section = raw.split("NetVLAD pooling")[1].split("chip_build_has_vlad")[0]
    for word in ("UNPINNED", "orc_dot_tree_f32", "orc_dot_tree_f64", "vlad_exp", "0x1.71547652b82fep+0", "0x1.62e42fee00000p-1",
                 "0x1.a39ef35793c76p-33", "1e-12", "CHIP_VLAD_BLOCK"):
        assert word in section, word
    for name, value in (("CHIP_VLAD_NHWC", capi.CHIP_VLAD_NHWC), ("CHIP_VLAD_NCHW", capi.CHIP_VLAD_NCHW), ("CHIP_VLAD_BLOCK", capi.CHIP_VLAD_BLOCK),
                        ("CHIP_VLAD_MAX_POSITIONS", capi.CHIP_VLAD_MAX_POSITIONS)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", raw), name
    assert (capi.CHIP_VLAD_NHWC, capi.CHIP_VLAD_NCHW, capi.CHIP_VLAD_BLOCK, capi.CHIP_VLAD_MAX_POSITIONS) == (1, 2, 64, 16384)


def test_library_exports_them_with_their_argument_rows(chip_lib):
    rows = {"chip_build_has_vlad": [], "chip_vlad_set": [P, I32, I32, I32, P, P, P], "chip_vlad_clear": [P],
            "chip_vlad_info": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)], "chip_vlad": [P, P, I32, I32, P],
            "chip_db_append_vlad_f32": [P, P, I32, I32, C.c_uint32, C.POINTER(I64)], "chip_debug_vlad_stage": [P, P, P, P]}
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
        fn = getattr(chip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rows[name], name
    assert chip_lib.chip_build_has_vlad() == 1
    assert chip_lib.chip_abi_version() == 7
    for method in ("vlad_set", "vlad_clear", "vlad_info", "vlad", "append_vlad", "debug_vlad_stage"):
        assert callable(getattr(capi.Chip, method)), method


def test_set_statuses_that_need_no_device(chip_lib):
    W, b, c = np.zeros((128, 1024), np.float32), np.zeros(128, np.float32), np.zeros((128, 1024), np.float32)
    w, pb, pc = capi._ptr(W), capi._ptr(b), capi._ptr(c)
    set_ = chip_lib.chip_vlad_set
    assert set_(None, 256, 16, 0, w, pb, pc) == BAD
    assert set_(FAKE, 256, 16, 0, None, pb, pc) == set_(FAKE, 256, 16, 0, w, None, pc) == set_(FAKE, 256, 16, 0, w, pb, None) == BAD
    for ch in (0, -4, 2, 3, 5, 254, 1026, 1028, 2048, 2 ** 31 - 4):              # C % 4 == 0, 4 <= C <= 1024
        assert set_(FAKE, ch, 1, 0, w, pb, pc) == UNSUPPORTED, ch
    for K, G in ((0, 0), (-1, 2), (1, -1), (129, 0), (128, 1), (64, 65), (0, 4), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 30, 2 ** 30)):
        assert set_(FAKE, 4, K, G, w, pb, pc) == UNSUPPORTED, (K, G)
    for ch, K, G in ((260, 126, 2), (1024, 33, 0), (1024, 16, 17), (516, 64, 0), (512, 64, 1)):     # (K+G) * C <= 32768
        assert set_(FAKE, ch, K, G, w, pb, pc) == UNSUPPORTED, (ch, K, G)
    assert set_(FAKE, 3, 16, 0, None, pb, pc) == BAD                             # the pointers first
    assert set_(None, 3, 0, 0, w, pb, pc) == BAD


def test_pool_and_append_statuses_that_need_no_device(chip_lib):
    x, v = np.zeros(256, np.float32), np.full(4, 9.0, np.float32)
    px, pv = capi._ptr(x), capi._ptr(v)
    first = C.c_int64(-7)
    pool, append = chip_lib.chip_vlad, chip_lib.chip_db_append_vlad_f32
    NHWC = capi.CHIP_VLAD_NHWC
    assert pool(None, px, 1, NHWC, pv) == pool(FAKE, None, 1, NHWC, pv) == pool(FAKE, px, 1, NHWC, None) == BAD
    assert append(None, px, 1, NHWC, 0, C.byref(first)) == append(FAKE, None, 1, NHWC, 0, C.byref(first)) == BAD
    for n in (0, -1, capi.CHIP_VLAD_MAX_POSITIONS + 1, 2 ** 31 - 1):             # 1 <= positions <= CHIP_VLAD_MAX_POSITIONS
        assert pool(FAKE, px, n, NHWC, pv) == UNSUPPORTED and append(FAKE, px, n, NHWC, 0, C.byref(first)) == UNSUPPORTED, n
    for layout in (0, 3, -1, 4):
        assert pool(FAKE, px, 1, layout, pv) == UNSUPPORTED and append(FAKE, px, 1, layout, 0, C.byref(first)) == UNSUPPORTED, layout
    assert pool(FAKE, None, 0, 9, pv) == BAD and append(None, px, 0, 9, 0, None) == BAD      # the pointers first
    assert chip_lib.chip_vlad_clear(None) == BAD and chip_lib.chip_debug_vlad_stage(None, None, None, None) == BAD
    i = C.c_int32(-3)
    assert chip_lib.chip_vlad_info(None, C.byref(i), C.byref(i), C.byref(i)) == BAD
    assert first.value == -7 and i.value == -3 and (v == 9.0).all()
