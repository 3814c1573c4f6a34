"""The descriptor projection (chip_build_has_project, chip_project_set, chip_project_clear, chip_project_info, chip_project,
chip_db_append_projected_f32) at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the
built library, bound by the ctypes table; every status that is decided before a ctx is touched is a status code."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_project", "chip_project_set", "chip_project_clear", "chip_project_info", "chip_project",
         "chip_db_append_projected_f32")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
FAKE = C.c_void_p(8)           # a handle that is never dereferenced: everything here is decided before anything touches a ctx


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive
    section = raw.split("descriptor projection")[1].split("chip_build_has_project")[0]
    assert "UNPINNED" in section and "orc_dot_tree_f32" in section and "orc_dot_tree_f64" in section
    for name, value in (("CHIP_PROJ_F32", capi.CHIP_PROJ_F32), ("CHIP_PROJ_F64", capi.CHIP_PROJ_F64), ("CHIP_PROJ_MAX_IN_DIM", capi.CHIP_PROJ_MAX_IN_DIM)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", raw), name
    assert capi.CHIP_PROJ_MAX_IN_DIM * 4 == 128 * 1024                            # x as float32 in the LDS


def test_library_exports_them_with_their_argument_rows(chip_lib):
    rows = {"chip_build_has_project": [], "chip_project_set": [P, I32, P, I32, P], "chip_project_clear": [P],
            "chip_project_info": [P, C.POINTER(I32), C.POINTER(I32), C.POINTER(I32)], "chip_project": [P, P, I64, P],
            "chip_db_append_projected_f32": [P, P, I64, C.c_uint32, C.POINTER(I64)]}
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
        fn = getattr(chip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rows[name], name
    assert chip_lib.chip_build_has_project() == 1
    assert chip_lib.chip_abi_version() == 7
    for method in ("project_set", "project_clear", "project_info", "project", "append_projected"):
        assert callable(getattr(capi.Chip, method)), method


def test_set_statuses_that_need_no_device(chip_lib):
    Mt, b = np.zeros((4, 256), np.float32), np.zeros(4)
    m, pb = capi._ptr(Mt), capi._ptr(b)
    set_ = chip_lib.chip_project_set
    assert set_(None, 256, m, capi.CHIP_PROJ_F32, pb) == BAD
    assert set_(FAKE, 256, None, capi.CHIP_PROJ_F32, pb) == BAD
    for in_dim in (0, -256, 128, 255, 257, 384, 32768 + 256, 65536, 2 ** 31 - 1):
        assert set_(FAKE, in_dim, m, capi.CHIP_PROJ_F32, pb) == UNSUPPORTED, in_dim
        assert set_(FAKE, in_dim, m, capi.CHIP_PROJ_F64, None) == UNSUPPORTED, in_dim
    for t in (0, 3, 4, 8, -1):
        assert set_(FAKE, 256, m, t, pb) == UNSUPPORTED, t
    assert set_(FAKE, 100, None, 7, pb) == BAD                                    # the pointers first
    assert set_(None, 100, m, 7, pb) == BAD


def test_project_and_append_statuses_that_need_no_device(chip_lib):
    x, z = np.zeros(256, np.float32), np.full(4, 9.0)
    px, pz = capi._ptr(x), capi._ptr(z)
    first = C.c_int64(-7)
    project, append = chip_lib.chip_project, chip_lib.chip_db_append_projected_f32
    assert project(None, px, 1, pz) == project(FAKE, None, 1, pz) == project(FAKE, px, 1, None) == project(FAKE, px, -1, pz) == BAD
    assert append(None, px, 1, 0, C.byref(first)) == append(FAKE, None, 1, 0, C.byref(first)) == append(FAKE, px, -1, 0, C.byref(first)) == BAD
    assert chip_lib.chip_project_clear(None) == BAD
    i = C.c_int32(-3)
    assert chip_lib.chip_project_info(None, C.byref(i), C.byref(i), C.byref(i)) == BAD
    assert first.value == -7 and i.value == -3 and (z == 9.0).all()
