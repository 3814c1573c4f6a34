"""Batched ingest (chip_project_plan, chip_debug_project_last, chip_vlad_batch, chip_db_append_vlad_batch_f32) at the drop-in boundary,
without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built library, bound by the ctypes table; every status
that is decided before a ctx is touched is a status code, in the stated order."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_project_plan", "chip_debug_project_last", "chip_vlad_batch", "chip_db_append_vlad_batch_f32")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
FAKE = C.c_void_p(8)           # a handle that is never dereferenced: everything here is decided before anything touches a ctx


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive
    assert re.search(r"typedef\s+struct\s+chip_project_plan_out\s*\{", text)
    section = raw.split("--- batched ingest")[1].split("typedef struct chip_project_plan_out")[0]
    for word in ("ABI 7, additive", "project_pass", "ceil(n / width)", "CHIP_ERR_NONFINITE", "32768", "at most 16", "LAST map"):
        assert word in section, word


def test_library_exports_them_with_their_argument_rows(chip_lib):
    rows = {"chip_project_plan": [I32, I32, I64, P], "chip_debug_project_last": [P, C.POINTER(I64), C.POINTER(I64), C.POINTER(I32)],
            "chip_vlad_batch": [P, P, I32, I32, I32, P], "chip_db_append_vlad_batch_f32": [P, P, I32, I32, I32, C.c_uint32, C.POINTER(I64)]}
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
        fn = getattr(chip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rows[name], name
    assert chip_lib.chip_abi_version() == 7
    for method in ("vlad_batch", "append_vlad_batch", "debug_project_last"):
        assert callable(getattr(capi.Chip, method)), method
    assert callable(capi.project_plan)
    assert C.sizeof(capi.ProjectPlan) == 6 * 4 + 3 * 8


def test_statuses_that_need_no_device(chip_lib):
    x, v = np.zeros(256, np.float32), np.full(4, 9.0, np.float32)
    px, pv = capi._ptr(x), capi._ptr(v)
    first = C.c_int64(-7)
    pool, append = chip_lib.chip_vlad_batch, chip_lib.chip_db_append_vlad_batch_f32
    NHWC = capi.CHIP_VLAD_NHWC
    assert pool(None, px, 1, 1, NHWC, pv) == pool(FAKE, None, 1, 1, NHWC, pv) == pool(FAKE, px, 1, 1, NHWC, None) == BAD    # a NULL ctx first
    assert append(None, px, 1, 1, NHWC, 0, C.byref(first)) == append(FAKE, None, 1, 1, NHWC, 0, C.byref(first)) == BAD
    assert pool(FAKE, px, -1, 1, NHWC, pv) == BAD and append(FAKE, px, -1, 1, NHWC, 0, C.byref(first)) == BAD
    for n in (0, -1, capi.CHIP_VLAD_MAX_POSITIONS + 1, 2 ** 31 - 1):             # 1 <= positions <= CHIP_VLAD_MAX_POSITIONS, for every n_maps
        for b in (0, 1, 17):
            assert pool(FAKE, px, b, n, NHWC, pv) == UNSUPPORTED and append(FAKE, px, b, n, NHWC, 0, C.byref(first)) == UNSUPPORTED, (b, n)
    for layout in (0, 3, -1, 4):
        assert pool(FAKE, px, 2, 1, layout, pv) == UNSUPPORTED and append(FAKE, px, 2, 1, layout, 0, C.byref(first)) == UNSUPPORTED, layout
    assert pool(FAKE, None, 0, 0, 9, pv) == BAD and append(None, px, 0, 0, 9, 0, None) == BAD      # the pointers first
    w = C.c_int32(-3)
    n2 = (C.c_int64 * 2)(-5, -5)
    assert chip_lib.chip_debug_project_last(None, n2, n2, C.byref(w)) == BAD
    assert first.value == -7 and w.value == -3 and list(n2) == [-5, -5] and (v == 9.0).all()
    out = capi.ProjectPlan()
    plan = chip_lib.chip_project_plan
    assert plan(256, capi.CHIP_PROJ_F32, 1, None) == BAD and plan(256, capi.CHIP_PROJ_F32, -1, C.byref(out)) == BAD
    for in_dim in (0, 128, 255, 257, 32768 + 256, -256):
        assert plan(in_dim, capi.CHIP_PROJ_F32, 1, C.byref(out)) == UNSUPPORTED, in_dim
    for kind in (0, 3, -1):
        assert plan(256, kind, 1, C.byref(out)) == UNSUPPORTED, kind
