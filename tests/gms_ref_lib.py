"""ctypes loader of the reference's GMS matcher compiled as a checker (oracle/_ref/libgms_ref.so, built by `make ref` from
oracle/ref_gms/ and the reference tree's gms_matcher.{h,cpp}).  TEST INFRASTRUCTURE.  This module never opens a file of the reference
tree: where the library is missing it runs `make ref`, which builds it if a reference tree is there and does nothing otherwise."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SO = ROOT / "oracle" / "_ref" / "libgms_ref.so"

FLAG_NONE, FLAG_OUT_OF_BOUNDS, FLAG_NOT_RUN = 0, 1, 2

_lib = None
_tried = False


def load():
    """the library, or None where it has not been built and cannot be (no reference tree)"""
    global _lib, _tried
    if _lib is not None or _tried:
        return _lib
    _tried = True
    if not SO.exists():
        r = subprocess.run(["make", "ref"], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("make ref failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    if not SO.exists():
        return None
    lib = C.CDLL(str(SO))
    P = C.c_void_p
    lib.gms_ref_run.restype = C.c_int
    lib.gms_ref_run.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, P, C.c_int32, C.c_int32, C.c_int32, P, P, C.c_int32, P,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    _lib = lib
    return _lib


def gms_filter(kp1, size1, kp2, size2, query_idx, train_idx):
    """size = (width, height).  -> (uint8 inlier mask in match order, flag): what gms_matcher(kp1, size1, kp2, size2, matches)
    .GetInlierMask(mask, false, false) answers.  flag != FLAG_NONE: the input is outside the reference's defined domain (it indexed a
    table out of bounds, or was not run); the mask is all zero then and means nothing."""
    lib = load()
    assert lib is not None, "libgms_ref.so not available"
    kp1 = np.ascontiguousarray(kp1, dtype=np.float32).reshape(-1, 2)
    kp2 = np.ascontiguousarray(kp2, dtype=np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(query_idx, dtype=np.int32)
    t = np.ascontiguousarray(train_idx, dtype=np.int32)
    assert q.shape == t.shape and q.ndim == 1
    n = len(q)
    mask = np.zeros(max(n, 1), np.uint8)
    cnt, flag = C.c_int32(), C.c_int32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.gms_ref_run(p(kp1), len(kp1), size1[0], size1[1], p(kp2), len(kp2), size2[0], size2[1], p(q), p(t), n, p(mask),
                         C.byref(cnt), C.byref(flag))
    assert rc == 0, f"gms_ref_run: status {rc}"
    assert cnt.value == int(mask[:n].sum())
    return mask[:n].copy(), flag.value
