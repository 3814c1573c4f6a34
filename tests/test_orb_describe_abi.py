"""The ORB descriptor (chip_build_has_orb_describe, chip_orb_bin, chip_orb_pattern, chip_orb_detect_describe, chip_debug_orb_blur,
chip_frame_put_orb_stereo) at the drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the
built library, bound by the ctypes table; chip_orb_pattern and chip_orb_bin -- which need neither a ctx nor a device -- give the tables
and bins of the numpy restatement; every status that needs no device is a status code."""
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

import np_mirror_orb_describe as D
from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_orb_describe", "chip_orb_bin", "chip_orb_pattern", "chip_orb_detect_describe", "chip_debug_orb_blur",
         "chip_frame_put_orb_stereo")
BAD, UNSUPPORTED = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
REFUSED = dict(n_features=(0, -1, capi.CHIP_MATCH_MAX_KEYPOINTS + 1), n_levels=(0, 9, -1), fast_threshold=(-1, 256), border=(15, 65, 0))
P, I32 = C.c_void_p, C.c_int32


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    assert "#define CHIP_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", raw)           # additive
    assert "#define CHIP_ORB_BINS 32" in raw and "#define CHIP_ORB_DESC_BYTES 32" in raw
    assert "is NOT built" not in raw                                             # the detector's block said so of the descriptor half


def test_library_exports_them_with_their_argument_rows(chip_lib):
    rows = {"chip_build_has_orb_describe": [], "chip_orb_bin": [I32, I32], "chip_orb_pattern": [P, P],
            "chip_orb_detect_describe": [P, P, I32, I32, C.POINTER(capi.OrbParams), P, I32, C.POINTER(I32), C.POINTER(I32), P],
            "chip_debug_orb_blur": [P, I32, P],
            "chip_frame_put_orb_stereo": [P, C.c_int64, I32, I32, P, P, C.POINTER(capi.OrbParams), C.POINTER(capi.StereoBmParams), P, C.POINTER(I32)]}
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
        fn = getattr(chip_lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == rows[name], name
    assert chip_lib.chip_build_has_orb_describe() == 1 and chip_lib.chip_build_has_orb_detect() == 1
    assert chip_lib.chip_abi_version() == 7
    assert capi.CHIP_ORB_BINS == D.BINS == 32 and capi.CHIP_ORB_DESC_BYTES == D.DESC_BYTES


def test_pattern_and_steered_table_equal_the_mirror_byte_for_byte(chip_lib):
    pattern, steered = capi.orb_pattern()
    assert pattern.tobytes() == D.pattern().tobytes() and steered.tobytes() == D.steered().tobytes()
    assert hashlib.sha256(pattern.tobytes()).hexdigest() == "0a170a01e941c47e3dc21a502fbec04104b548ddedf269114180a0504526a179"
    assert hashlib.sha256(steered.tobytes()).hexdigest() == "489d64ba52aef79c6fa46391b51cc6fe2e3764aa946f9283360aca763ba5969f"
    # either pointer may be NULL; both is refused
    only_p, only_s = np.zeros(1024, np.int8), np.zeros(32768, np.int8)
    assert chip_lib.chip_orb_pattern(capi._ptr(only_p), None) == capi.CHIP_OK and only_p.tobytes() == pattern.tobytes()
    assert chip_lib.chip_orb_pattern(None, capi._ptr(only_s)) == capi.CHIP_OK and only_s.tobytes() == steered.tobytes()
    assert chip_lib.chip_orb_pattern(None, None) == BAD


def test_bin_equals_the_mirror(chip_lib):
    assert capi.orb_bin(3196, 315) == 0 and capi.orb_bin(0, 0) == 0 and capi.orb_bin(0, 1) == 8
    m = 2_900_000                                                                # an int32 product with the table would wrap
    cases = [(a * m, b * m) for a in (-1, 0, 1) for b in (-1, 0, 1)] + [(m, 1), (-m, -1), (m - 1, m), (-m, m - 1), (2 ** 31 - 1, 2 ** 31 - 1),
                                                                         (-2 ** 31, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]
    rng = np.random.default_rng(5)
    cases += [(int(a), int(b)) for a, b in rng.integers(-m, m + 1, (2000, 2))]
    cases += [(D.COS[k] * s, D.SIN[k] * s) for k in range(32) for s in (1, 3, 100)]    # along every bin's own direction
    assert [capi.orb_bin(a, b) for a, b in cases] == [D.orb_bin(a, b) for a, b in cases]
    assert [D.orb_bin(D.COS[k], D.SIN[k]) for k in range(32)] == list(range(32))


def test_detect_describe_statuses_that_need_no_device(chip_lib):
    img = np.zeros((70, 80), np.uint8)
    kp = np.zeros(5000, capi.ORB_KEYPOINT_DTYPE)
    desc = np.zeros((5000, 32), np.uint8)
    n = C.c_int32(-7)
    i, k, d, pn = capi._ptr(img), capi._ptr(kp), capi._ptr(desc), C.byref(n)
    det = chip_lib.chip_orb_detect_describe
    assert det(None, i, 80, 70, None, k, 5000, pn, None, d) == BAD
    # everything below is decided before anything touches a ctx's device: a fake handle is never dereferenced
    fake = C.c_void_p(8)
    assert det(fake, None, 80, 70, None, k, 5000, pn, None, d) == BAD
    assert det(fake, i, 80, 70, None, None, 5000, pn, None, d) == BAD
    assert det(fake, i, 80, 70, None, k, 5000, None, None, d) == BAD
    assert det(fake, i, 80, 70, None, k, 5000, pn, None, None) == BAD             # desc
    for w, h in ((0, 70), (80, 0), (-1, 70), (80, -1)):
        assert det(fake, i, w, h, None, k, 5000, pn, None, d) == BAD
    assert det(fake, i, 80, 70, None, k, 4999, pn, None, d) == BAD                # capacity < n_features
    assert det(fake, i, 4097, 70, None, k, 5000, pn, None, d) == det(fake, i, 80, 4097, None, k, 5000, pn, None, d) == UNSUPPORTED
    for field, values in REFUSED.items():
        for v in values:
            p = capi.default_orb_params(**{field: v})
            assert det(fake, i, 80, 70, C.byref(p), k, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, pn, None, d) == UNSUPPORTED, (field, v)
            assert det(fake, i, 80, 70, C.byref(p), k, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, pn, None, None) == BAD, (field, v)   # the pointers first
    assert n.value == -7 and not kp.view(np.uint8).any() and not desc.any()
    assert chip_lib.chip_debug_orb_blur(None, 0, None) == BAD


def test_put_statuses_that_need_no_device(chip_lib):
    left, right = np.zeros((70, 80), np.uint8), np.zeros((70, 80), np.uint8)
    Q = np.eye(4).reshape(16)
    n = C.c_int32(-7)
    l, r, q, pn = capi._ptr(left), capi._ptr(right), capi._ptr(Q), C.byref(n)
    put = chip_lib.chip_frame_put_orb_stereo
    fake = C.c_void_p(8)
    assert put(None, 1, 80, 70, l, r, None, None, q, pn) == BAD
    assert put(fake, 1, 80, 70, None, r, None, None, q, pn) == BAD
    assert put(fake, 1, 80, 70, l, None, None, None, q, pn) == BAD
    assert put(fake, 1, 80, 70, l, r, None, None, None, pn) == BAD
    assert put(fake, 1, 80, 70, l, r, None, None, q, None) == BAD
    for w, h in ((0, 70), (80, 0), (-1, 70)):
        assert put(fake, 1, w, h, l, r, None, None, q, pn) == BAD
    assert put(fake, 1, 4097, 70, l, r, None, None, q, pn) == put(fake, 1, 80, 4097, l, r, None, None, q, pn) == UNSUPPORTED
    for field, values in REFUSED.items():
        for v in values:
            assert put(fake, 1, 80, 70, l, r, C.byref(capi.default_orb_params(**{field: v})), None, q, pn) == UNSUPPORTED, (field, v)
    for field, v in (("num_disparities", 24), ("block_size", 4), ("block_size", 23), ("prefilter_cap", 0), ("prefilter_cap", 64),
                     ("texture_threshold", -1), ("uniqueness_ratio", 101)):
        bm = capi.StereoBmParams()
        chip_lib.chip_stereo_bm_params_default(C.byref(bm))
        setattr(bm, field, v)
        assert put(fake, 1, 80, 70, l, r, None, C.byref(bm), q, pn) == UNSUPPORTED, (field, v)
    assert n.value == -7
