"""chip_query_batch_cast_f32 (the many-query mode on double rows, rows narrowed to float in the GEMM's loader) at the drop-in
boundary, without a GPU: declared in include/cerebro_hip.h, exported by the built library, bound by the ctypes table, and a NULL
ctx is a status code."""
import ctypes as C
import re
from pathlib import Path

import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAME = "chip_query_batch_cast_f32"


def test_header_declares_the_cast_entry():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cerebro_hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, NAME + " is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [re.sub(r"\s*\w+$", "", a).replace(" ", "") for a in args] == \
        ["chip_ctx*", "int64_t", "constfloat*", "int32_t", "int32_t", "float*", "int64_t*"]      # the signature of chip_query_batch_f32
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", (ROOT / "include" / "cerebro_hip.h").read_text())   # additive


def test_library_exports_it_and_a_null_ctx_is_a_status(chip_lib):
    assert hasattr(chip_lib, NAME)
    assert NAME in capi.declared_symbols()
    q = (C.c_float * 32)()
    sc, ix = (C.c_float * 4)(), (C.c_int64 * 4)()
    assert getattr(chip_lib, NAME)(None, 0, q, 1, 4, sc, ix) == capi.CHIP_ERR_INVALID_ARG
    assert chip_lib.chip_query_batch_f32(None, 0, q, 1, 4, sc, ix) == capi.CHIP_ERR_INVALID_ARG
