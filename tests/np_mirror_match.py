"""CPU restatement in numpy of the candidate verification front end (cerebro_amd/csrc/match.hip; definitions in
include/cerebro_hip.h): brute-force Hamming matching, the GMS grid-statistics filter and the PnP / ICP correspondence sets.

Written from the definitions, with the reference's lines cited where a promotion or a comparison matters
(src/utils/GMSMatcher/gms_matcher.{h,cpp}, src/utils/PointFeatureMatching.cpp).  Every floating-point step is one IEEE
operation in the type the reference uses, so the device result must equal this one bit for bit.  No reference file is read."""
from __future__ import annotations

import numpy as np

GRID = 20                 # mGridSizeLeft = Size(20, 20) (gms_matcher.h:62); the right grid is the same at scale 0 (:230-231)
CELLS = GRID * GRID
COORD_LIM = 1.0e6         # a grid coordinate beyond this (or NaN) has no cell


# ---------------------------------------------------------------------------------------------- brute-force matching
def orb_bf_match(d1: np.ndarray, d2: np.ndarray):
    """d1 (n1, 32) uint8 queries, d2 (n2, 32) uint8 train -> (train_idx, distance) int32: minimum Hamming distance, the FIRST
    minimum in train order (np.argmin).  n2 == 0: no matches, both -1."""
    d1 = np.ascontiguousarray(d1, dtype=np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(d2, dtype=np.uint8).reshape(-1, 32)
    n1, n2 = len(d1), len(d2)
    if n2 == 0 or n1 == 0:
        return np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
    # |a xor b| = |a| + |b| - 2 a.b on the bit vectors; every number is an integer <= 512, exact in float32
    a = np.unpackbits(d1, axis=1).astype(np.float32)
    b = np.unpackbits(d2, axis=1).astype(np.float32)
    idx = np.empty(n1, np.int32)
    dist = np.empty(n1, np.int32)
    pb = b.sum(1)
    for lo in range(0, n1, 1024):
        blk = a[lo:lo + 1024]
        h = (blk.sum(1)[:, None] + pb[None, :] - 2.0 * (blk @ b.T)).astype(np.int32)
        j = np.argmin(h, axis=1)
        idx[lo:lo + 1024] = j
        dist[lo:lo + 1024] = h[np.arange(len(blk)), j]
    return idx, dist


# ---------------------------------------------------------------------------------------------- GMS
def normalise(kp_xy: np.ndarray, width: int, height: int):
    """NormalizePoints (gms_matcher.h:126-139): float / int -> ONE float division per coordinate"""
    kp = np.ascontiguousarray(kp_xy, dtype=np.float32).reshape(-1, 2)
    return kp[:, 0] / np.float32(width), kp[:, 1] / np.float32(height)


def _coord(p: np.ndarray, shifted: bool):
    """floor(pt.x * 20) resp. floor(pt.x * 20 + 0.5) (gms_matcher.h:147-173): the product is Point2f x int = float, the + 0.5 is double"""
    f = p.astype(np.float32) * np.float32(GRID)
    assert f.dtype == np.float32
    with np.errstate(invalid="ignore"):
        v = np.floor(f.astype(np.float64) + 0.5) if shifted else np.floor(f).astype(np.float64)
        ok = (v >= -COORD_LIM) & (v <= COORD_LIM)
    return ok, np.where(ok, v, 0.0).astype(np.int64)


def cell_left(px, py, grid_type: int):
    """GetGridIndexLeft (gms_matcher.h:143-182); -1 = no cell (also for an index outside [0, 400))"""
    sx, sy = grid_type in (2, 4), grid_type in (3, 4)
    okx, x = _coord(np.asarray(px, np.float32), sx)
    oky, y = _coord(np.asarray(py, np.float32), sy)
    ok = okx & oky
    if grid_type == 1:
        ok &= ~((y >= GRID) | (x >= GRID))
    if sx:
        ok &= ~((x >= GRID) | (x < 1))
    if sy:
        ok &= ~((y >= GRID) | (y < 1))
    idx = x + y * GRID
    ok &= (idx >= 0) & (idx < CELLS)
    return np.where(ok, idx, -1).astype(np.int32)


def cell_right(px, py):
    """GetGridIndexRight (gms_matcher.h:184-189): no range check; outside [0, 400) the match has no right cell"""
    okx, x = _coord(np.asarray(px, np.float32), False)
    oky, y = _coord(np.asarray(py, np.float32), False)
    idx = x + y * GRID
    ok = okx & oky & (idx >= 0) & (idx < CELLS)
    return np.where(ok, idx, -1).astype(np.int32)


def gms_pass(l: np.ndarray, r: np.ndarray):
    """one grid type: AssignMatchPairs + VerifyCellPairs (gms_matcher.cpp:73-148, rotation pattern 1) -> accepted right cell per left cell
    (-1 empty row, -2 rejected)"""
    v = (l >= 0) & (r >= 0)                                          # :92
    table = np.zeros((CELLS, CELLS), np.int32)
    np.add.at(table, (l[v], r[v]), 1)                                # :94
    cnt = np.bincount(l[v], minlength=CELLS).astype(np.int32)        # :95
    pair = np.full(CELLS, -1, np.int32)
    for i in range(CELLS):
        if cnt[i] == 0:                                              # :106
            continue
        j = int(np.argmax(table[i]))                                 # strict > from column 0 (:112-121): the first maximum
        lx, ly, rx, ry = i % GRID, i // GRID, j % GRID, j // GRID
        score = tsum = numpair = 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                a, b, c, d = lx + dx, ly + dy, rx + dx, ry + dy
                if not (0 <= a < GRID and 0 <= b < GRID and 0 <= c < GRID and 0 <= d < GRID):   # :136
                    continue
                score += int(table[a + b * GRID, c + d * GRID])
                tsum += int(cnt[a + b * GRID])
                numpair += 1
        thresh = np.float64(6.0) * np.sqrt(np.float64(tsum) / np.float64(numpair))               # :143
        pair[i] = j if not (np.float64(score) < thresh) else -2                                  # :145-146
    return pair


def gms_filter(kp1_xy, size1, kp2_xy, size2, query_idx, train_idx):
    """size = (width, height).  -> uint8 inlier mask in match order (gms_matcher.cpp:150-181 with GetInlierMask(.., false, false))"""
    q = np.asarray(query_idx, np.int64)
    t = np.asarray(train_idx, np.int64)
    inl = np.zeros(len(q), np.uint8)
    if len(q) == 0:
        return inl
    x1, y1 = normalise(kp1_xy, *size1)
    x2, y2 = normalise(kp2_xy, *size2)
    r = cell_right(x2[t], y2[t])
    for grid_type in (1, 2, 3, 4):                                   # :158
        l = cell_left(x1[q], y1[q], grid_type)
        pair = gms_pass(l, r)
        ok = (l >= 0) & (r >= 0)
        hit = np.zeros(len(q), bool)
        hit[ok] = pair[l[ok]] == r[ok]                               # :171-175
        inl |= hit.astype(np.uint8)
    return inl


# ---------------------------------------------------------------------------------------------- correspondence sets
def _pixel(p: np.ndarray, w: int, h: int):
    """(int)uv(1,k), (int)uv(0,k) (PointFeatureMatching.cpp:121,180): truncation; inside iff the float lies in (-1, w) x (-1, h)"""
    with np.errstate(invalid="ignore"):
        inside = (p[:, 0] > np.float32(-1)) & (p[:, 0] < np.float32(w)) & (p[:, 1] > np.float32(-1)) & (p[:, 1] < np.float32(h))
    safe = np.where(inside[:, None], p, 0).astype(np.float32)
    return inside, np.trunc(safe[:, 0]).astype(np.int64), np.trunc(safe[:, 1]).astype(np.int64)


def depth_ok(z: np.ndarray):
    """not (z < 0.1 || z > 25.) with the float z widened to double (:122,:182): 0.1f passes, NaN passes"""
    z = np.asarray(z, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~((z < 0.1) | (z > 25.0))


def normalise_pixels(Kinv: np.ndarray, u: np.ndarray, v: np.ndarray):
    """rows 0, 1 of Kinv (3x3, row-major) * (u, v, 1): (r0 * u + r1 * v) + r2 in fp64, no contraction (:114-115)"""
    K = np.asarray(Kinv, np.float64).reshape(9)
    return np.stack([(K[0] * u + K[1] * v) + K[2], (K[3] * u + K[4] * v) + K[5]], axis=1)


def pose_sets(kp1_xy, kp2_xy, train_idx, inlier, xyz_a, xyz_b, Kinv):
    """match i = (i, train_idx[i]); xyz_* (H, W, 3) float32.  -> dict of the arrays chip_match_read_sets returns + the summary counts"""
    kp1 = np.ascontiguousarray(kp1_xy, np.float32).reshape(-1, 2)
    kp2 = np.ascontiguousarray(kp2_xy, np.float32).reshape(-1, 2)
    xyz_a = np.asarray(xyz_a, np.float32)
    xyz_b = np.asarray(xyz_b, np.float32)
    q = np.nonzero(np.asarray(inlier) != 0)[0]
    t = np.asarray(train_idx, np.int64)[q]
    pa, pb = kp1[q], kp2[t]
    in_a, xa, ya = _pixel(pa, xyz_a.shape[1], xyz_a.shape[0])
    in_b, xb, yb = _pixel(pb, xyz_b.shape[1], xyz_b.shape[0])
    Pa = xyz_a[ya, xa].astype(np.float64)
    Pb = xyz_b[yb, xb].astype(np.float64)
    za = in_a & depth_ok(xyz_a[ya, xa, 2])
    zb = in_b & depth_ok(xyz_b[yb, xb, 2])
    uv = pa.astype(np.float64)
    uv_d = pb.astype(np.float64)
    na = normalise_pixels(Kinv, uv[:, 0], uv[:, 1])
    nb = normalise_pixels(Kinv, uv_d[:, 0], uv_d[:, 1])
    both = za & zb
    out = dict(uv=uv, uv_d=uv_d, match_query_idx=q.astype(np.int32), match_train_idx=t.astype(np.int32),
               X_ab=Pa[za], uvn_ab=nb[za], X_ba=Pb[zb], uvn_ba=na[zb], A_3d3d=Pa[both], B_3d3d=Pb[both])
    out["summary"] = dict(n_matches_gms=len(q), n_3d2d_ab=int(za.sum()), n_3d2d_ba=int(zb.sum()), n_3d3d=int(both.sum()),
                          n_out_of_image=int((~in_a | ~in_b).sum()))
    return out


def match_pair(frame_a: dict, frame_b: dict, Kinv):
    """the whole stage: frames are dicts desc (n, 32) uint8, kp (n, 2) float32, xyz (H, W, 3) float32; width / height = xyz's"""
    n1, n2 = len(frame_a["kp"]), len(frame_b["kp"])
    empty = dict(n_matches_all=0, n_matches_gms=0, n_3d2d_ab=0, n_3d2d_ba=0, n_3d3d=0, n_out_of_image=0)
    if n1 == 0 or n2 == 0:
        return dict(summary=empty, train_idx=np.zeros(0, np.int32), distance=np.zeros(0, np.int32), inlier=np.zeros(0, np.uint8))
    tidx, dist = orb_bf_match(frame_a["desc"], frame_b["desc"])
    ha, wa = frame_a["xyz"].shape[:2]
    hb, wb = frame_b["xyz"].shape[:2]
    inl = gms_filter(frame_a["kp"], (wa, ha), frame_b["kp"], (wb, hb), np.arange(n1), tidx)
    out = pose_sets(frame_a["kp"], frame_b["kp"], tidx, inl, frame_a["xyz"], frame_b["xyz"], Kinv)
    out["summary"]["n_matches_all"] = n1
    out.update(train_idx=tidx, distance=dist, inlier=inl)
    return out
