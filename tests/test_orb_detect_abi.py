"""ORB keypoint detection (chip_orb_params_default, chip_build_has_orb_detect, chip_orb_plan, chip_orb_detect, chip_debug_orb_level and
the three structs) at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built
library, bound by the ctypes table, every status that needs no device is a status code, and chip_orb_plan -- which needs neither a
ctx nor a device -- gives the table of the numpy restatement."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import np_mirror_orb_detect as O
from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_orb_params_default", "chip_build_has_orb_detect", "chip_orb_plan", "chip_orb_detect", "chip_debug_orb_level")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
DEFAULTS = dict(n_features=5000, n_levels=8, fast_threshold=0, border=31)
# field -> values just outside the accepted range, at both bounds
REFUSED = dict(n_features=(0, -1, capi.CHIP_MATCH_MAX_KEYPOINTS + 1), n_levels=(0, 9, -1), fast_threshold=(-1, 256), border=(15, 65, 0))
# ... and the bounds themselves, accepted
ACCEPTED = dict(n_features=(1, capi.CHIP_MATCH_MAX_KEYPOINTS), n_levels=(1, 8), fast_threshold=(0, 255), border=(16, 64))
KEYPOINT_FIELDS = ("response", "x", "y", "m10", "m01", "x_level", "y_level", "level", "zero")
LEVEL_FIELDS = ("width", "height", "quota", "x0", "y0", "x1", "y1", "scale")


def test_header_declares_the_entries_the_structs_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bvoid\s+chip_orb_params_default\s*\(", text)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*chip_orb_params\s*;", text).group(1)
    assert re.findall(r"int32_t\s+(\w+)\s*;", body) == list(DEFAULTS)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*chip_orb_keypoint\s*;", text).group(1)
    assert tuple(n for decl in re.findall(r"\w+\s+([\w\s,]+);", body) for n in re.split(r"\s*,\s*", decl.strip())) == KEYPOINT_FIELDS
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*chip_orb_level\s*;", text).group(1)
    assert tuple(n for decl in re.findall(r"\w+\s+([\w\s,]+);", body) for n in re.split(r"\s*,\s*", decl.strip())) == LEVEL_FIELDS
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive
    assert "#define CHIP_ORB_MAX_LEVELS 8" in raw and "#define CHIP_ORB_MAX_SIDE 4096" in raw


def test_struct_sizes_field_order_and_defaults(chip_lib):
    assert C.sizeof(capi.OrbParams) == 16 and C.sizeof(capi.OrbKeypoint) == 32 and C.sizeof(capi.OrbLevel) == 40
    assert capi.ORB_KEYPOINT_DTYPE.itemsize == 32 and capi.ORB_KEYPOINT_DTYPE == O.KEYPOINT
    assert [n for n, _ in capi.OrbParams._fields_] == list(DEFAULTS)
    assert tuple(n for n, _ in capi.OrbKeypoint._fields_) == KEYPOINT_FIELDS == capi.ORB_KEYPOINT_DTYPE.names
    assert [getattr(capi.OrbKeypoint, n).offset for n in KEYPOINT_FIELDS] == [capi.ORB_KEYPOINT_DTYPE.fields[n][1] for n in KEYPOINT_FIELDS] \
        == [0, 8, 12, 16, 20, 24, 26, 28, 30]
    assert tuple(n for n, _ in capi.OrbLevel._fields_) == LEVEL_FIELDS and capi.OrbLevel.scale.offset == 32
    p = capi.default_orb_params()
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS == O.DEFAULTS
    assert (capi.CHIP_ORB_N_FEATURES, capi.CHIP_ORB_N_LEVELS, capi.CHIP_ORB_FAST_THRESHOLD, capi.CHIP_ORB_BORDER) == tuple(DEFAULTS.values())
    assert (capi.CHIP_ORB_MAX_LEVELS, capi.CHIP_ORB_MAX_SIDE) == (8, 4096)
    chip_lib.chip_orb_params_default(None)                                       # a NULL is left alone


def test_library_exports_them(chip_lib):
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
    assert chip_lib.chip_build_has_orb_detect() == 1
    assert chip_lib.chip_abi_version() == 7


def test_detect_statuses_that_need_no_device(chip_lib):
    img = np.zeros((70, 80), np.uint8)
    kp = np.zeros(5000, capi.ORB_KEYPOINT_DTYPE)
    n = C.c_int32(-7)
    i, k, pn = capi._ptr(img), capi._ptr(kp), C.byref(n)
    det = chip_lib.chip_orb_detect
    assert det(None, i, 80, 70, None, k, 5000, pn, None) == BAD
    # everything below is decided before anything touches a ctx's device: a fake handle is never dereferenced
    fake = C.c_void_p(8)
    assert det(fake, None, 80, 70, None, k, 5000, pn, None) == BAD
    assert det(fake, i, 80, 70, None, None, 5000, pn, None) == BAD
    assert det(fake, i, 80, 70, None, k, 5000, None, None) == BAD
    for w, h in ((0, 70), (80, 0), (-1, 70), (80, -1)):
        assert det(fake, i, w, h, None, k, 5000, pn, None) == BAD
    assert det(fake, i, 80, 70, None, k, 4999, pn, None) == BAD                  # capacity < n_features (the defaults' 5000)
    p = capi.default_orb_params(n_features=100)
    assert det(fake, i, 80, 70, C.byref(p), k, 99, pn, None) == BAD
    assert det(fake, i, 4097, 70, None, k, 5000, pn, None) == UNSUPPORTED
    assert det(fake, i, 80, 4097, None, k, 5000, pn, None) == UNSUPPORTED
    for field, values in REFUSED.items():
        for v in values:
            p = capi.default_orb_params(**{field: v})
            assert det(fake, i, 80, 70, C.byref(p), k, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, pn, None) == UNSUPPORTED, (field, v)
            assert det(fake, None, 80, 70, C.byref(p), k, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, pn, None) == BAD, (field, v)   # the pointers first
    assert n.value == -7 and not kp.view(np.uint8).any()
    assert chip_lib.chip_debug_orb_level(None, 0, None, None) == BAD


def test_plan_statuses_and_parameter_bounds(chip_lib):
    lv = (capi.OrbLevel * 8)()
    plan = chip_lib.chip_orb_plan
    assert plan(80, 70, None, None) == BAD
    for w, h in ((0, 70), (80, 0), (-3, 70)):
        assert plan(w, h, None, lv) == BAD
    assert plan(4097, 70, None, lv) == plan(80, 4097, None, lv) == UNSUPPORTED
    for field, values in REFUSED.items():
        for v in values:
            assert plan(80, 70, C.byref(capi.default_orb_params(**{field: v})), lv) == UNSUPPORTED, (field, v)
    for field, values in ACCEPTED.items():
        for v in values:
            assert plan(80, 70, C.byref(capi.default_orb_params(**{field: v})), lv) == capi.CHIP_OK, (field, v)
    with pytest.raises(capi.ChipError):
        capi.orb_plan(80, 70, dict(border=15))


@pytest.mark.parametrize("shape,kw", (((752, 480), {}), ((33, 33), dict(border=16)), ((1, 1), {}), ((4096, 4096), {}), ((4096, 1), dict(n_levels=3)),
                                      ((100, 90), dict(n_features=1, n_levels=1, border=16))), ids=str)
def test_plan_equals_the_mirrors_table(chip_lib, shape, kw):
    got, want = capi.orb_plan(*shape, kw or None), O.plan(*shape, O.params(**kw))
    assert got == want                                                           # ints and the double scale, exactly
    if shape == (33, 33):
        assert [(L["x0"], L["y0"], L["x1"], L["y1"]) for L in got] == [(16, 16, 16, 16)] + [(0, 0, -1, -1)] * 7   # one detection pixel, none above
    if shape == (1, 1):
        assert all(L["x1"] < L["x0"] for L in got) and [L["width"] for L in got] == [1, 1, 1, 1, 0, 0, 0, 0]
    # entries from n_levels on are zero
    lv = (capi.OrbLevel * 8)()
    p = capi.default_orb_params(**kw)
    assert chip_lib.chip_orb_plan(shape[0], shape[1], C.byref(p), lv) == capi.CHIP_OK
    assert all(not any(lv[l].as_dict().values()) for l in range(p.n_levels, 8))
