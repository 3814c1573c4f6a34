"""chip_match_pairs_stored at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built
library, bound by the ctypes table, and bad arguments are status codes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_match_pairs", "chip_match_pairs_stored")


def test_header_declares_the_two_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    flat = re.sub(r"[ \t]+", " ", raw)
    assert "#define CHIP_ABI_VERSION 7" in flat                                   # additive
    assert "#define CHIP_MATCH_MAX_PAIRS CHIP_MATCH_MAX_BATCH" in flat and "#define CHIP_MATCH_MAX_BATCH 16" in flat


def test_library_exports_them_and_reports_the_pair_list(chip_lib):
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
    assert chip_lib.chip_build_has_match_pairs() == 1
    assert chip_lib.chip_abi_version() == 7
    assert capi.CHIP_MATCH_MAX_PAIRS == capi.CHIP_MATCH_MAX_BATCH == 16
    assert hasattr(capi.Chip, "match_pairs_stored")


def test_invalid_arguments_are_status_codes(chip_lib):
    lib, bad = chip_lib, capi.CHIP_ERR_INVALID_ARG
    a, b = np.array([1, 2], np.int64), np.array([3, 4], np.int64)
    Ki = np.eye(3).reshape(9)
    sm, ch = (capi.MatchSummary * 2)(), (capi.GmsChoice * 2)()
    for modes in (0, 3):
        assert lib.chip_match_pairs_stored(None, capi._ptr(a), capi._ptr(b), 2, capi._ptr(Ki), modes, sm, ch) == bad
        assert lib.chip_match_pairs_stored(None, capi._ptr(a), capi._ptr(b), 2, capi._ptr(Ki), modes, sm, None) == bad
