"""CPU restatement in numpy scalar types of the disparity -> 3-D step (cerebro_amd/csrc/frames.hip: point_of_disparity, used by
disparity_gather and disparity_to_xyz; definitions in include/cerebro_hip.h, "a frame from its disparity map"), i.e. of
StereoGeometry::disparity_to_3DPoints, src/utils/CameraGeometry.cpp:485-523 of the reference:

    Q03, Q13, Q23, Q32, Q33 = float(Q[0,3]), float(Q[1,3]), float(Q[2,3]), float(Q[3,2]), float(Q[3,3])
    pw = float(1.0 / (double(d) / 16.0 * double(Q32) + double(Q33) + 1e-6))        every operation fp64, left to right, ONE narrowing
    x, y, z = (float(j) + Q03) * pw, (float(i) + Q13) * pw, Q23 * pw               fp32, no contraction

numpy's float64 / float32 array operations are single IEEE operations (no FMA), which is what the reference's build does.  A NaN
result is a NaN; its sign and payload are not defined."""
from __future__ import annotations

import numpy as np

import np_mirror_match as M

VARIANTS = ("exact", "f32_sum", "f32_div")     # the two float shortcuts exist so that tests can show the inputs catch them


def q5(Q) -> tuple:
    """the five entries of the 4 x 4 Q that count, each narrowed to float32 (:494-498)"""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    return tuple(np.float32(Q[r, c]) for r, c in ((0, 3), (1, 3), (2, 3), (3, 2), (3, 3)))


def as_float(disp) -> np.ndarray:
    """convertTo(CV_32FC1) (:472-473): exact for int16, the identity for float32"""
    d = np.asarray(disp)
    assert d.dtype in (np.int16, np.float32), d.dtype
    return d.astype(np.float32)


def pw_of(d32, Q, variant: str = "exact") -> np.ndarray:
    _, _, _, q32, q33 = q5(Q)
    d = np.asarray(d32, np.float32)
    with np.errstate(all="ignore"):
        prod = (d.astype(np.float64) / np.float64(16.0)) * np.float64(q32)          # exact: 24 x 24 significant bits
        if variant == "exact":
            return (np.float64(1.0) / ((prod + np.float64(q33)) + np.float64(1e-6))).astype(np.float32)
        if variant == "f32_sum":                                                     # the two additions in fp32, the divide in fp64
            return (np.float64(1.0) / ((prod.astype(np.float32) + q33) + np.float32(1e-6)).astype(np.float64)).astype(np.float32)
        if variant == "f32_div":                                                     # the divide in fp32
            return np.float32(1.0) / ((prod + np.float64(q33)) + np.float64(1e-6)).astype(np.float32)
    raise ValueError(variant)


def points(d32, j, i, Q, variant: str = "exact") -> np.ndarray:
    """-> (..., 3) float32: the points of disparities d32 (float32) at columns j, rows i (integers), broadcast together"""
    q03, q13, q23, _, _ = q5(Q)
    pw = pw_of(d32, Q, variant)
    with np.errstate(all="ignore"):
        x = (np.asarray(j).astype(np.float32) + q03) * pw
        y = (np.asarray(i).astype(np.float32) + q13) * pw
        z = q23 * pw
    return np.stack(np.broadcast_arrays(x, y, z), axis=-1).astype(np.float32)


def xyz_from_disparity(disp, Q, variant: str = "exact") -> np.ndarray:
    """the dense (H, W, 3) float32 image out3D of an (H, W) int16 / float32 disparity"""
    d = as_float(disp)
    assert d.ndim == 2
    h, w = d.shape
    return points(d, np.arange(w)[None, :], np.arange(h)[:, None], Q, variant)


def records(kp_xy, disp, Q) -> np.ndarray:
    """-> (n, 4) float32 point records of the keypoints, each from the ONE disparity at its pixel (disparity_gather); equals
    np_mirror_frame_store.gather(kp_xy, xyz_from_disparity(disp, Q))"""
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    d = as_float(disp)
    inside, x, y = M._pixel(kp, d.shape[1], d.shape[0])
    rec = np.zeros((len(kp), 4), np.float32)
    rec[inside, :3] = points(d[y[inside], x[inside]], x[inside], y[inside], Q)
    rec[inside, 3] = np.float32(1.0)
    return rec


def stored(frame: dict, disp, Q) -> dict:
    """np_mirror_frame_store.stored for a frame dict(desc, kp) that arrives with its disparity"""
    h, w = np.asarray(disp).shape
    return dict(desc=frame["desc"], kp=frame["kp"], rec=records(frame["kp"], disp, Q), size=(w, h))


def same_floats(a, b) -> bool:
    """equality on the uint32 view; a NaN matches any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))

