"""The batched ICP-RANSAC (chip_icp_ransac_batch, chip_icp_ransac_matched_batch / _enqueue / _collect, chip_build_has_icp_batch) at the
drop-in boundary, without a GPU: declared in include/cerebro_hip.h next to ABI 7, exported by the built library, bound by the ctypes
table, and bad arguments are status codes.  CHIP_ERR_BUSY of a collect before any enqueue needs a live ctx, which needs a device: it is
held on the GPU (tests/test_icp_batch_gpu.py::test_status_rules); here the collects are refused for what can be judged without one."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("chip_build_has_icp_batch", "chip_icp_ransac_batch", "chip_icp_ransac_matched_batch_enqueue", "chip_icp_ransac_matched_batch_collect",
         "chip_icp_ransac_matched_batch", "chip_icp_ransac")


def test_header_declares_the_entries_and_keeps_abi_7():
    raw = (ROOT / "include" / "cerebro_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name + " is not declared"
    flat = re.sub(r"[ \t]+", " ", raw)
    assert "#define CHIP_ABI_VERSION 7" in flat                                   # additive
    assert "#define CHIP_ICP_MAX_BATCH 16" in flat and capi.CHIP_ICP_MAX_BATCH == capi.CHIP_MATCH_MAX_BATCH == 16


def test_library_exports_them_and_reports_the_batch(chip_lib):
    for name in NAMES:
        assert hasattr(chip_lib, name), name
        assert name in capi.declared_symbols(), name
    assert chip_lib.chip_build_has_icp_batch() == 1
    assert chip_lib.chip_abi_version() == 7


def _batch_args(P, n=32):
    pts = [np.zeros((n, 3)) for _ in range(max(P, 1))]
    ptr = (C.c_void_p * max(P, 1))(*[a.ctypes.data for a in pts])
    N = np.full(max(P, 1), n, np.int32)
    T = np.zeros((max(P, 1), 16))
    conf = np.zeros(max(P, 1), np.float32)
    return pts, ptr, N, T, conf


def test_invalid_arguments_are_status_codes(chip_lib):
    lib = chip_lib
    bad, unsup = capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_UNSUPPORTED
    p = capi.default_icp_params()
    # the argument rules come before anything that needs a ctx's device: a fake non-null handle is never dereferenced for these
    fake = C.c_void_p(8)
    keep, ptr, N, T, conf = _batch_args(2)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(c=fake, P=2, A=ptr, B=ptr, N=capi._ptr(N), p=C.byref(p), seeds=None, T=capi._ptr(T),   # noqa: E731
                                                        conf=capi._ptr(conf), masks=None, summ=None).items()]
    assert lib.chip_icp_ransac_batch(*args(c=None)) == bad
    for P in (0, -1):
        assert lib.chip_icp_ransac_batch(*args(P=P)) == bad
    for k in ("A", "B", "N", "p", "T", "conf"):
        assert lib.chip_icp_ransac_batch(*args(**{k: None})) == bad, k
    keep17, ptr17, N17, T17, conf17 = _batch_args(17)
    assert lib.chip_icp_ransac_batch(fake, 17, ptr17, ptr17, capi._ptr(N17), C.byref(p), None, capi._ptr(T17), capi._ptr(conf17), None, None) == unsup
    hole = (C.c_void_p * 2)(keep[0].ctypes.data, None)
    assert lib.chip_icp_ransac_batch(*args(A=hole)) == bad                        # a NULL problem
    few = np.array([32, 19], np.int32)
    assert lib.chip_icp_ransac_batch(*args(N=capi._ptr(few))) == capi.CHIP_ERR_TOO_FEW_POINTS   # the whole call, before anything runs

    cand = np.zeros(17, np.int32)
    status = np.zeros(17, np.int32)
    enq = lambda **kw: [kw.get(k, v) for k, v in dict(c=fake, P=2, cand=capi._ptr(cand), p=C.byref(p), seeds=None, status=capi._ptr(status)).items()]   # noqa: E731
    assert lib.chip_icp_ransac_matched_batch_enqueue(*enq(c=None)) == bad
    for P in (0, -1):
        assert lib.chip_icp_ransac_matched_batch_enqueue(*enq(P=P)) == bad
    for k in ("cand", "p", "status"):
        assert lib.chip_icp_ransac_matched_batch_enqueue(*enq(**{k: None})) == bad, k
    assert lib.chip_icp_ransac_matched_batch_enqueue(*enq(P=17)) == unsup
    # the collects: without a ctx, or without somewhere to put the answers, nothing is pending that could be delivered
    assert lib.chip_icp_ransac_matched_batch_collect(None, capi._ptr(T), capi._ptr(conf), None, None) == bad
    assert lib.chip_icp_ransac_matched_batch_collect(fake, None, capi._ptr(conf), None, None) == bad
    assert lib.chip_icp_ransac_matched_batch_collect(fake, capi._ptr(T), None, None, None) == bad
    assert lib.chip_icp_ransac_collect(None, capi._ptr(T), C.byref(C.c_float()), None, None) == bad
    one = lambda **kw: [kw.get(k, v) for k, v in dict(c=fake, P=2, cand=capi._ptr(cand), p=C.byref(p), seeds=None, T=capi._ptr(T), conf=capi._ptr(conf),   # noqa: E731
                                                       masks=None, summ=None, status=capi._ptr(status)).items()]
    assert lib.chip_icp_ransac_matched_batch(*one(c=None)) == bad
    for k in ("cand", "p", "T", "conf", "status"):
        assert lib.chip_icp_ransac_matched_batch(*one(**{k: None})) == bad, k
    assert lib.chip_icp_ransac_matched_batch(*one(P=0)) == bad
    assert lib.chip_icp_ransac_matched_batch(*one(P=17)) == unsup
