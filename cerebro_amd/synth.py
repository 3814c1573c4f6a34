"""Synthetic input generators shared by tests and bench.py (data only -- no reference or oracle code).
PnP scene of SURVEY.md 8d: N correspondences, points in the frustum of camera b at 0.5-20 m rounded to float32
(mirrors the CV_32FC3 depth image, PointFeatureMatching.cpp:124-141), pose yaw U(-30,30) deg, pitch/roll U(-5,5) deg,
|t| <= 1 m, pixel noise at f = 458 (EuRoC-like), a fraction of uniformly random outliers."""
from __future__ import annotations

import numpy as np


def make_scene(N=512, outlier_frac=0.3, noise_px=0.5, seed=4242, focal=458.0):
    rng = np.random.default_rng(seed)
    yaw = np.deg2rad(rng.uniform(-30, 30)); pitch = np.deg2rad(rng.uniform(-5, 5)); roll = np.deg2rad(rng.uniform(-5, 5))
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    R = Ry @ Rx @ Rz
    t = rng.standard_normal(3); t *= rng.uniform(0, 1) / np.linalg.norm(t)
    # points in the frustum of camera b, depth 0.5..20 m, expressed in frame a, rounded to float32 (CV_32FC3)
    depth = rng.uniform(0.5, 20.0, N)
    uvb = np.stack([rng.uniform(-0.8, 0.8, N), rng.uniform(-0.5, 0.5, N)], axis=1)
    Xb = np.concatenate([uvb * depth[:, None], depth[:, None]], axis=1)
    Xa = ((Xb - t) @ R).astype(np.float32).astype(np.float64)           # X_a = R^T (X_b - t)
    proj = Xa @ R.T + t
    uv = proj[:, :2] / proj[:, 2:3] + rng.standard_normal((N, 2)) * (noise_px / focal)
    out = rng.random(N) < outlier_frac
    uv[out] = np.stack([rng.uniform(-0.8, 0.8, out.sum()), rng.uniform(-0.5, 0.5, out.sum())], axis=1)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return Xa, uv, T, ~out


def make_icp_scene(N=300, outlier_frac=0.2, noise=0.02, seed=1):
    """3-D / 3-D correspondences for the Umeyama-ICP-RANSAC row (P3P_ICP, DlsPnpWithRansac.cpp:15-16: uv_X, uvd_Y): the PnP scene's
    points in frame a, the same points in frame b with Gaussian noise, a fraction displaced by up to 3 m."""
    X, uv, T, inl = make_scene(N=N, outlier_frac=0.0, noise_px=0.0, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    A = X
    B = X @ T[:3, :3].T + T[:3, 3] + rng.standard_normal((N, 3)) * noise
    out = rng.random(N) < outlier_frac
    B[out] += rng.uniform(-3, 3, (out.sum(), 3))
    return A, B, T, ~out


def pinhole(focal=458.0, width=752, height=480):
    """K and its inverse (row-major 3x3) of an EuRoC-like pinhole camera; every entry of the inverse is written down, not solved for"""
    cx, cy = width / 2.0, height / 2.0
    K = np.array([[focal, 0.0, cx], [0.0, focal, cy], [0.0, 0.0, 1.0]])
    Kinv = np.array([[1.0 / focal, 0.0, -cx / focal], [0.0, 1.0 / focal, -cy / focal], [0.0, 0.0, 1.0]])
    return K, Kinv


def make_match_scene(n_true=2000, n_outlier_a=200, n_outlier_b=200, flip_rate=0.04, n_duplicates=0, n_border=0, seed=1,
                     width=752, height=480, focal=458.0, yaw_deg=2.0, t=(0.15, 0.02, 0.05), depth=(3.0, 12.0), all_duplicate=False, roll_deg=0.0):
    """Input of the candidate verification front end (chip_match_pair): two views a, b of ONE random 3-D point cloud with a known
    relative pose b_T_a.  Per view: keypoints (float32 pixels), 256-bit descriptors, the 3-D image (H x W x 3 float32, the point of a
    keypoint stored at its truncated pixel, depth 0 elsewhere -- what the 0.1 m gate drops).
      true pairs  : a's descriptor with every bit flipped with probability flip_rate; b's keypoints are shuffled
      outliers    : keypoints with random descriptors and no depth, in both views
      duplicates  : n_duplicates extra keypoints of b that carry the exact descriptor of an earlier b keypoint (ties: the lowest index wins)
      border      : n_border of a's keypoints sit exactly on cell borders of the GMS grids (x * 20 / width integral or integral + 0.5)
      all_duplicate: every descriptor of both views is the same 32 bytes (every distance 0, every match -> train index 0)
      roll_deg    : non-zero: view b is also rolled about the optical axis, R = Ry(yaw) . Rz(roll) (what GMS needs its rotation types for)
    Returns dict(a=frame, b=frame, K, Kinv, T=b_T_a (4x4), pairs=(ia, ib) indices of the true pairs); frame = dict(desc, kp, xyz)."""
    rng = np.random.default_rng(seed)
    K, Kinv = pinhole(focal, width, height)
    yaw = np.deg2rad(yaw_deg)
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    if roll_deg != 0.0:                                              # only then: with the default every array stays byte-identical
        roll = np.deg2rad(roll_deg)
        R = R @ np.array([[np.cos(roll), -np.sin(roll), 0], [np.sin(roll), np.cos(roll), 0], [0, 0, 1]])
    tv = np.asarray(t, np.float64)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = tv
    # a's keypoints: distinct integer pixels (one 3-D point per pixel of the 3-D image) + a fraction
    n_a = n_true + n_outlier_a
    pix = rng.choice((width - 2) * (height - 2), size=n_a, replace=False)
    ka = np.stack([pix % (width - 2) + 1, pix // (width - 2) + 1], axis=1).astype(np.float64) + rng.uniform(0.0, 0.99, (n_a, 2))
    if n_border:
        bx = np.array([94.0, 188.0, 376.0, 564.0]); by = np.array([60.0, 120.0, 240.0, 360.0])
        sel = np.arange(min(n_border, n_true))
        ka[sel, 0] = bx[sel % 4]
        ka[sel, 1] = by[(sel // 4) % 4] + (sel // 16)      # distinct pixels: rows 60, 61, .. of the same border column
    ka = ka.astype(np.float32)
    z = rng.uniform(depth[0], depth[1], n_true)
    Xa = (np.concatenate([ka[:n_true].astype(np.float64), np.ones((n_true, 1))], axis=1) @ Kinv.T) * z[:, None]
    Xa = Xa.astype(np.float32).astype(np.float64)                    # the 3-D image is CV_32FC3
    Xb = Xa @ R.T + tv
    pb = (Xb / Xb[:, 2:3]) @ K.T
    kb_true = pb[:, :2].astype(np.float32)
    # a true point takes part iff it lands inside b on a pixel no other point claims
    ib_pix = np.floor(kb_true.astype(np.float64)).astype(np.int64)
    inside = (ib_pix[:, 0] >= 0) & (ib_pix[:, 0] < width) & (ib_pix[:, 1] >= 0) & (ib_pix[:, 1] < height) & (Xb[:, 2] > 0.2)
    flat = ib_pix[:, 1] * width + ib_pix[:, 0]
    _, first = np.unique(flat, return_index=True)
    keep = np.zeros(n_true, bool); keep[first] = True
    keep &= inside
    # a's pixel may also collide after the border override
    fa = np.floor(ka[:n_true, 1].astype(np.float64)).astype(np.int64) * width + np.floor(ka[:n_true, 0].astype(np.float64)).astype(np.int64)
    _, first_a = np.unique(fa, return_index=True)
    ka_keep = np.zeros(n_true, bool); ka_keep[first_a] = True
    keep &= ka_keep
    da = rng.integers(0, 256, (n_a, 32), dtype=np.uint8)
    xyz_a = np.zeros((height, width, 3), np.float32)
    va = np.nonzero(keep)[0]
    xyz_a[np.floor(ka[va, 1].astype(np.float64)).astype(np.int64), np.floor(ka[va, 0].astype(np.float64)).astype(np.int64)] = Xa[va].astype(np.float32)
    # b: the kept true points (shuffled) + outliers + duplicates
    n_keep = len(va)
    flips = np.packbits(rng.random((n_keep, 256)) < flip_rate, axis=1)
    db_true = da[va] ^ flips
    kb_out = np.stack([rng.uniform(1, width - 1, n_outlier_b), rng.uniform(1, height - 1, n_outlier_b)], axis=1).astype(np.float32)
    db_out = rng.integers(0, 256, (n_outlier_b, 32), dtype=np.uint8)
    kb = np.concatenate([kb_true[va], kb_out])
    db = np.concatenate([db_true, db_out])
    Xb_all = np.concatenate([Xb[va].astype(np.float32), np.zeros((n_outlier_b, 3), np.float32)])
    order = rng.permutation(len(kb))
    kb, db, Xb_all = kb[order], db[order], Xb_all[order]
    inv = np.empty(len(order), np.int64); inv[order] = np.arange(len(order))
    pairs_b = inv[:n_keep]
    if n_duplicates:
        src = rng.integers(0, len(kb), n_duplicates)
        kb = np.concatenate([kb, np.stack([rng.uniform(1, width - 1, n_duplicates), rng.uniform(1, height - 1, n_duplicates)], axis=1).astype(np.float32)])
        db = np.concatenate([db, db[src]])
        Xb_all = np.concatenate([Xb_all, np.zeros((n_duplicates, 3), np.float32)])
    xyz_b = np.zeros((height, width, 3), np.float32)
    has = Xb_all[:, 2] > 0
    xyz_b[np.floor(kb[has, 1].astype(np.float64)).astype(np.int64), np.floor(kb[has, 0].astype(np.float64)).astype(np.int64)] = Xb_all[has]
    if all_duplicate:
        da[:] = da[0]
        db[:] = da[0]
    return dict(a=dict(desc=da, kp=ka, xyz=xyz_a), b=dict(desc=db, kp=kb, xyz=xyz_b), K=K, Kinv=Kinv, T=T,
                pairs=(va.astype(np.int64), pairs_b.astype(np.int64)))
