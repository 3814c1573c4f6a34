"""ctypes loader of the reference's GMS matcher WITH its scale / rotation variants, compiled as a checker
(oracle/_ref/libgms_ref_modes.so, built by `make ref_modes` from tests/ref_gms_modes/, oracle/ref_gms/opencv2/ and the reference tree's
gms_matcher.{h,cpp}).  TEST INFRASTRUCTURE, the twin of tests/gms_ref_lib.py.  This module never opens a file of the reference tree:
where the library is missing it runs `make ref_modes`, which builds it if a reference tree is there and does nothing otherwise."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SO = ROOT / "oracle" / "_ref" / "libgms_ref_modes.so"

FLAG_NONE, FLAG_OUT_OF_BOUNDS, FLAG_NOT_RUN = 0, 1, 2
FLAG_PAIRS = ((0, 1), (1, 0), (1, 1))          # (with_scale, with_rotation)

_lib = None
_tried = False


def modes_of(with_scale, with_rotation) -> int:
    """the library's bit set: CHIP_GMS_WITH_SCALE = 1, CHIP_GMS_WITH_ROTATION = 2"""
    return (1 if with_scale else 0) | (2 if with_rotation else 0)


def load():
    """the library, or None where it has not been built and cannot be (no reference tree)"""
    global _lib, _tried
    if _lib is not None or _tried:
        return _lib
    _tried = True
    if not SO.exists():
        r = subprocess.run(["make", "ref_modes"], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("make ref_modes failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    if not SO.exists():
        return None
    lib = C.CDLL(str(SO))
    P = C.c_void_p
    I = C.POINTER(C.c_int32)
    lib.gms_ref_modes_run.restype = C.c_int
    lib.gms_ref_modes_run.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, P, C.c_int32, C.c_int32, C.c_int32, P, P, C.c_int32, C.c_int32,
                                      C.c_int32, P, I, I, I]
    _lib = lib
    return _lib


def gms_filter_modes(kp1, size1, kp2, size2, query_idx, train_idx, with_scale, with_rotation):
    """size = (width, height).  -> (uint8 mask in match order, n_inliers, mask_size, flag): what gms_matcher(kp1, size1, kp2, size2,
    matches).GetInlierMask(mask, with_scale, with_rotation) answers.  mask_size is the size of the reference's vector afterwards: 0
    where it left the vector untouched because no hypothesis kept a match (the mask here is all zero then).  flag != FLAG_NONE: the
    input is outside the reference's defined domain (it indexed a table out of bounds, or was not run); the mask means nothing."""
    lib = load()
    assert lib is not None, "libgms_ref_modes.so not available"
    kp1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
    kp2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(query_idx, dtype=np.int32)
    t = np.ascontiguousarray(train_idx, dtype=np.int32)
    assert q.shape == t.shape and q.ndim == 1
    n = len(q)
    mask = np.zeros(max(n, 1), np.uint8)
    cnt, size, flag = C.c_int32(), C.c_int32(), C.c_int32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.gms_ref_modes_run(p(kp1), len(kp1), size1[0], size1[1], p(kp2), len(kp2), size2[0], size2[1], p(q), p(t), n,
                               int(bool(with_scale)), int(bool(with_rotation)), p(mask), C.byref(cnt), C.byref(size), C.byref(flag))
    assert rc == 0, f"gms_ref_modes_run: status {rc}"
    if flag.value == FLAG_NONE:
        assert cnt.value == int(mask[:n].sum()) and size.value in (0, n) and (size.value == n or cnt.value == 0)
    return mask[:n].copy(), cnt.value, size.value, flag.value
