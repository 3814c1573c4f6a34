"""CPU restatement in numpy of GMS with scale and rotation (gms_grid_modes + gms_mode_select in cerebro_amd/csrc/match.hip; definitions
in include/cerebro_hip.h, "GMS with scale and rotation"): gms_matcher::GetInlierMask(mask, WithScale, WithRotation) of
src/utils/GMSMatcher/gms_matcher.{h,cpp}, built on np_mirror_match's normalise, cell_left and _coord.

Written from the definitions.  The eight rotation patterns are restated from their ring description, not copied: number the 3 x 3
neighbourhood row-major 0..8; the ring of its outer positions clockwise from the top-left is (0, 1, 2, 5, 8, 7, 6, 3); pattern r pairs
the left neighbour at ring position k with the right neighbour at ring position (k - (r - 1)) mod 8, centre with centre.
No reference file is read."""
from __future__ import annotations

import numpy as np

import np_mirror_match as M

WITH_SCALE, WITH_ROTATION = 1, 2
GRID, CELLS = M.GRID, M.CELLS
SIDES = tuple(int(20 * r) for r in (1.0, 1.0 / 2, 1.0 / np.sqrt(2.0), np.sqrt(2.0), 2.0))   # gms_matcher.h:47, :230-234
assert SIDES == (20, 10, 14, 28, 40)
RING = (0, 1, 2, 5, 8, 7, 6, 3)


def rotation_pairs(r: int):
    """[(left position, right position)] of rotation type r = 1..8, positions row-major 0..8"""
    return [(4, 4)] + [(RING[k], RING[(k - (r - 1)) % 8]) for k in range(8)]


def scales_of(modes: int):
    return range(5) if modes & WITH_SCALE else range(1)


def rotations_of(modes: int):
    return range(1, 9) if modes & WITH_ROTATION else range(1, 2)


def cell_right(px, py, side: int):
    """GetGridIndexRight under SetScale (gms_matcher.h:184-189): floorf(p * (float)side) per axis, x + y * side, no range check on x or
    y; -1 = no right cell (an index outside [0, side^2), a coordinate that is not finite or absurdly large)"""
    def coord(p):
        f = np.asarray(p, np.float32) * np.float32(side)
        assert f.dtype == np.float32
        with np.errstate(invalid="ignore"):
            v = np.floor(f).astype(np.float64)
            ok = (v >= -M.COORD_LIM) & (v <= M.COORD_LIM)
        return ok, np.where(ok, v, 0.0).astype(np.int64)
    okx, x = coord(px)
    oky, y = coord(py)
    idx = x + y * side
    ok = okx & oky & (idx >= 0) & (idx < side * side)
    return np.where(ok, idx, -1).astype(np.int32)


def grid_pass(l: np.ndarray, r: np.ndarray, side: int, rotations):
    """one (scale, grid type): the table and the first-maximum column once, then per rotation type the accepted right cell per left cell
    (-1 empty row, -2 rejected) -> {rotation: pair[400]}"""
    N = side * side
    v = (l >= 0) & (r >= 0)                                          # gms_matcher.cpp:92
    table = np.zeros((CELLS, N), np.int64)
    np.add.at(table, (l[v], r[v]), 1)                                # :94
    cnt = np.bincount(l[v], minlength=CELLS).astype(np.int64)        # :95
    first = np.where(cnt > 0, np.argmax(table, axis=1), -1)         # :106-121: the first maximum
    rows = np.nonzero(cnt > 0)[0]                                    # all non-empty left cells at once
    j = first[rows]
    lx, ly, rx, ry = rows % GRID, rows // GRID, j % side, j // side
    out = {}
    for rot in rotations:
        score = np.zeros(len(rows), np.int64)
        tsum = np.zeros(len(rows), np.int64)
        numpair = np.zeros(len(rows), np.int64)
        for lp, rp in rotation_pairs(rot):
            a, b, c, d = lx + lp % 3 - 1, ly + lp // 3 - 1, rx + rp % 3 - 1, ry + rp // 3 - 1
            ok = (0 <= a) & (a < GRID) & (0 <= b) & (b < GRID) & (0 <= c) & (c < side) & (0 <= d) & (d < side)   # :136
            ll, rr = np.where(ok, a + b * GRID, 0), np.where(ok, c + d * side, 0)
            score += np.where(ok, table[ll, rr], 0)
            tsum += np.where(ok, cnt[ll], 0)
            numpair += ok
        thresh = np.float64(6.0) * np.sqrt(tsum.astype(np.float64) / numpair.astype(np.float64))   # :143; the centre pair always remains
        pair = np.full(CELLS, -1, np.int32)
        pair[rows] = np.where(score.astype(np.float64) < thresh, -2, j)                           # :145-146
        out[rot] = pair
    return out


def gms_filter_modes(kp1_xy, size1, kp2_xy, size2, query_idx, train_idx, modes: int):
    """size = (width, height).  -> (uint8 inlier mask in match order, choice) with choice = dict(scale, rotation, n_inliers,
    counts (5, 8) int32): what chip_gms_filter_modes answers"""
    assert modes in (0, 1, 2, 3)
    q = np.asarray(query_idx, np.int64)
    t = np.asarray(train_idx, np.int64)
    n = len(q)
    counts = np.full((5, 8), -1, np.int32)
    for s in scales_of(modes):
        for rot in rotations_of(modes):
            counts[s, rot - 1] = 0
    best_mask, best, bs, br = np.zeros(n, np.uint8), 0, -1, 0
    if n == 0:
        return best_mask, dict(scale=-1, rotation=0, n_inliers=0, counts=counts)
    x1, y1 = M.normalise(kp1_xy, *size1)
    x2, y2 = M.normalise(kp2_xy, *size2)
    lefts = [M.cell_left(x1[q], y1[q], grid_type) for grid_type in (1, 2, 3, 4)]
    for s in scales_of(modes):
        side = SIDES[s]
        r = cell_right(x2[t], y2[t], side)                           # once per scale, reused by grid types 2-4
        masks = {rot: np.zeros(n, bool) for rot in rotations_of(modes)}
        for l in lefts:                                              # gms_matcher.cpp:158
            ok = (l >= 0) & (r >= 0)
            for rot, pair in grid_pass(l, r, side, rotations_of(modes)).items():
                masks[rot][ok] |= pair[l[ok]] == r[ok]               # :171-175
        for rot in rotations_of(modes):
            c = int(masks[rot].sum())
            counts[s, rot - 1] = c
            if c > best:                                             # :26-30: strictly more than every earlier hypothesis
                best_mask, best, bs, br = masks[rot].astype(np.uint8), c, s, rot
    if modes == 0:                                                   # the plain filter reports its one hypothesis even when it kept nothing
        bs, br = 0, 1
    return best_mask, dict(scale=bs, rotation=br, n_inliers=best, counts=counts)


def match_pair_modes(frame_a: dict, frame_b: dict, Kinv, modes: int):
    """np_mirror_match.match_pair with the modes filter: matcher -> gms_filter_modes -> pose_sets"""
    n1, n2 = len(frame_a["kp"]), len(frame_b["kp"])
    if n1 == 0 or n2 == 0:
        out = M.match_pair(frame_a, frame_b, Kinv)
        out["choice"] = gms_filter_modes(np.zeros((0, 2), np.float32), (1, 1), np.zeros((0, 2), np.float32), (1, 1), [], [], modes)[1]
        return out
    tidx, dist = M.orb_bf_match(frame_a["desc"], frame_b["desc"])
    ha, wa = frame_a["xyz"].shape[:2]
    hb, wb = frame_b["xyz"].shape[:2]
    inl, choice = gms_filter_modes(frame_a["kp"], (wa, ha), frame_b["kp"], (wb, hb), np.arange(n1), tidx, modes)
    out = M.pose_sets(frame_a["kp"], frame_b["kp"], tidx, inl, frame_a["xyz"], frame_b["xyz"], Kinv)
    out["summary"]["n_matches_all"] = n1
    out.update(train_idx=tidx, distance=dist, inlier=inl, choice=choice)
    return out
