"""Generators of GMS inputs (keypoints, image sizes, a match list) for the tests that compare the reference's compiled matcher, the numpy
restatement and the gms_filter kernel: tests/test_gms_ref_mirror.py (CPU), tests/golden/make_golden_gms.py and
tests/test_match_edges_gpu.py.  Every generator is a pure function of JSON-serialisable arguments, so a case is named by
(kind, arguments) and frozen by the SHA-256 of what it generates.

Cells: the grids are 20 x 20; cell (cx, cy) has column / row index cx + 20 cy in the 400 x 400 motion-statistics table.  A keypoint
"at fraction f of cell c" sits at pixel (c + f) * side / 20.  Fraction 0.25 stays in cell c in all four grid types (the shifted grids
add 0.5); fraction 0.75 is in cell c of the unshifted grid and in cell c + 1 of the shifted one."""
from __future__ import annotations

import hashlib

import numpy as np

GRID = 20
SIZES = [(752, 480), (640, 480), (1241, 376), (1280, 720), (333, 217), (100, 37), (20, 20)]


def _below(side: int) -> np.float32:
    return np.nextafter(np.float32(side), np.float32(0))


def _inside(x: np.ndarray, side: int) -> np.ndarray:
    """float32 coordinates in [0, side): a double just below side may round up to side"""
    return np.minimum(np.maximum(x.astype(np.float32), np.float32(0)), _below(side))


def _cell_pix(cell, frac, size):
    return np.array([(cell[0] + frac[0]) * size[0] / GRID, (cell[1] + frac[1]) * size[1] / GRID], np.float64)


def col_cell(col: int):
    return (col % GRID, col // GRID)


def _random_kp(rng, n, size):
    return np.stack([_inside(rng.uniform(0, size[0], n), size[0]), _inside(rng.uniform(0, size[1], n), size[1])], axis=1)


def groups(size1, size2, groups, noise=0, seed=0, shuffle=True):
    """groups: [n, [lx, ly], [fx, fy], [rx, ry]] = n matches from fraction (fx, fy) of left cell (lx, ly) to fraction 0.25 of right cell
    (rx, ry); then `noise` uniformly random matches.  Match i = (i, i) before the shuffle of the match order.
    -> also "group": the group of every match (noise: -1), for the tests' assertions"""
    rng = np.random.default_rng(seed)
    kp1, kp2, gid = [], [], []
    for g, (n, lc, lf, rc) in enumerate(groups):
        kp1.append(np.tile(_cell_pix(lc, lf, size1), (n, 1)))
        kp2.append(np.tile(_cell_pix(rc, (0.25, 0.25), size2), (n, 1)))
        gid += [g] * n
    if noise:
        kp1.append(_random_kp(rng, noise, size1))
        kp2.append(_random_kp(rng, noise, size2))
        gid += [-1] * noise
    kp1 = np.concatenate(kp1).astype(np.float32)
    kp2 = np.concatenate(kp2).astype(np.float32)
    q = np.arange(len(kp1), dtype=np.int32)
    if shuffle:
        q = rng.permutation(len(kp1)).astype(np.int32)
    return dict(kp1=kp1, size1=tuple(size1), kp2=kp2, size2=tuple(size2), q=q, t=q.copy(), group=np.asarray(gid)[q])


def border_values(side: int) -> np.ndarray:
    """every coordinate at which one of the four grids has a cell border (x * 20 / side integral or integral + 0.5), one float below
    and one above it, 0 and the last float below side.  All in [0, side)."""
    v = (np.arange(2 * GRID, dtype=np.float64) * side / (2 * GRID)).astype(np.float32)
    out = np.concatenate([v, np.nextafter(v, np.float32(side)), np.nextafter(v[1:], np.float32(0)), [_below(side)]]).astype(np.float32)
    assert (out >= 0).all() and (out < np.float32(side)).all()
    return out


def smooth(n, seed, size1=(752, 480), size2=(752, 480), motions=1, outlier_frac=0.2, border=0):
    """n matches (i, t[i]): left keypoints uniform in image 1; per motion m the right keypoint is an affine image of the left one that
    stays inside image 2; a fraction of the matches goes to a random keypoint instead.  border > 0: that many matches have both
    keypoints ON or one float either side of a cell border of the four grids."""
    rng = np.random.default_rng(seed)
    kp1 = _random_kp(rng, n, size1)
    if border:
        bx, by = border_values(size1[0]), border_values(size1[1])
        sel = rng.choice(n, min(border, n), replace=False)
        kp1[sel, 0] = rng.choice(bx, len(sel))
        kp1[sel, 1] = rng.choice(by, len(sel))
    kp2 = np.empty_like(kp1)
    which = rng.integers(0, motions, n)
    for m in range(motions):
        s = rng.uniform(0.6, 0.95, 2)
        o = rng.uniform(0, 1, 2) * (1 - s)
        sel = which == m
        for a in (0, 1):
            kp2[sel, a] = _inside((kp1[sel, a].astype(np.float64) / size1[a] * s[a] + o[a]) * size2[a], size2[a])
    if border:                                                       # right keypoints on the borders of image 2 as well
        bx, by = border_values(size2[0]), border_values(size2[1])
        sel = rng.choice(n, min(border, n), replace=False)
        kp2[sel, 0] = rng.choice(bx, len(sel))
        kp2[sel, 1] = rng.choice(by, len(sel))
    t = np.arange(n, dtype=np.int32)
    out = rng.random(n) < outlier_frac
    t[out] = rng.integers(0, n, int(out.sum()))
    return dict(kp1=kp1, size1=tuple(size1), kp2=kp2, size2=tuple(size2), q=np.arange(n, dtype=np.int32), t=t)


def random_matches(n, seed, size1=(752, 480), size2=(752, 480)):
    rng = np.random.default_rng(seed)
    return dict(kp1=_random_kp(rng, n, size1), size1=tuple(size1), kp2=_random_kp(rng, n, size2), size2=tuple(size2),
                q=np.arange(n, dtype=np.int32), t=rng.permutation(n).astype(np.int32))


def border_grid(size1=(752, 480), size2=(752, 480), seed=0, repeat=4):
    """an identity motion in normalised coordinates in which every border value of either axis occurs (against random positions of the
    other axis, `repeat` copies each, plus 400 border x border combinations and 1500 ordinary points); for every other match the
    exact border values are those of image 1 on the left keypoint, for the rest those of image 2 on the right keypoint"""
    rng = np.random.default_rng(seed)
    nb = len(border_values(size1[0]))                                 # the same count for every side: values correspond by index
    none = lambda k: np.full(k, -1)
    ix = np.concatenate([np.repeat(np.arange(nb), repeat), none(nb * repeat), rng.integers(0, nb, 400), none(1500)])
    iy = np.concatenate([none(nb * repeat), np.repeat(np.arange(nb), repeat), rng.integers(0, nb, 400), none(1500)])
    n = len(ix)
    u = rng.random((n, 2))
    unit = border_values(1 << 20).astype(np.float64) / (1 << 20)
    u[:, 0] = np.where(ix >= 0, unit[ix], u[:, 0])
    u[:, 1] = np.where(iy >= 0, unit[iy], u[:, 1])
    exact_left = np.arange(n) % 2 == 0                                # copies of one border value alternate

    def points(size, exact):
        x, y = _inside(u[:, 0] * size[0], size[0]), _inside(u[:, 1] * size[1], size[1])
        x = np.where(exact & (ix >= 0), border_values(size[0])[ix], x)
        y = np.where(exact & (iy >= 0), border_values(size[1])[iy], y)
        return np.stack([x, y], axis=1).astype(np.float32)

    q = np.arange(n, dtype=np.int32)
    return dict(kp1=points(size1, exact_left), size1=tuple(size1), kp2=points(size2, ~exact_left), size2=tuple(size2), q=q, t=q.copy())


def right_on_image_edge(seed=0, size1=(752, 480), size2=(752, 480), n=2000):
    """right keypoints with x == width exactly in the rows of cells 0..18: the reference's unchecked x + 20 y gives cell (0, y + 1),
    inside its tables ("including x + 20 y aliasing at x = width")"""
    c = smooth(n, seed, size1, size2, outlier_frac=0.1)
    rng = np.random.default_rng(seed + 1)
    sel = rng.choice(n, n // 4, replace=False)
    c["kp2"][sel, 0] = np.float32(size2[0])
    c["kp2"][sel, 1] = _inside(rng.uniform(0, size2[1] * 18.9 / GRID, len(sel)), size2[1])
    return c


def query_path(n, seed, n1=700):
    """an arbitrary match list: query indices repeated and DESCENDING, every query keypoint matched to several train keypoints that
    follow one smooth motion"""
    rng = np.random.default_rng(seed)
    size = (752, 480)
    kp1 = _random_kp(rng, n1, size)
    q = np.sort(rng.integers(0, n1, n))[::-1].astype(np.int32)
    kp2 = np.stack([_inside(kp1[q, 0].astype(np.float64) * 0.9 + 20 + rng.uniform(-2, 2, n), size[0]),
                    _inside(kp1[q, 1].astype(np.float64) * 0.9 + 11 + rng.uniform(-2, 2, n), size[1])], axis=1)
    perm = rng.permutation(n)
    t = np.empty(n, np.int32)
    t[:] = perm
    kp2s = np.empty_like(kp2)
    kp2s[perm] = kp2
    return dict(kp1=kp1, size1=size, kp2=kp2s, size2=size, q=np.ascontiguousarray(q), t=t)


KINDS = dict(groups=groups, smooth=smooth, random_matches=random_matches, border_grid=border_grid, right_on_image_edge=right_on_image_edge,
             query_path=query_path)


def generate(kind: str, args: dict) -> dict:
    return KINDS[kind](**args)


def digest(case: dict) -> str:
    h = hashlib.sha256()
    for k in ("kp1", "kp2", "q", "t"):
        a = np.ascontiguousarray(case[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())
    h.update(repr((tuple(int(v) for v in case["size1"]), tuple(int(v) for v in case["size2"]))).encode())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- the constructed cases
L0 = [10, 10]                     # an interior left cell
Q = [0.25, 0.25]


def _tie(cols, n=40, left=L0):
    """n matches from one left cell into each of the right cells `cols`, the HIGHEST column first in the match list"""
    return dict(size1=[752, 480], size2=[752, 480], groups=[[n, left, Q, list(col_cell(c))] for c in sorted(cols, reverse=True)], seed=len(cols))


FAR = [3, 17]                     # where the neighbours' matches go: no neighbour of the accepted right cells below


def _thresh(left, right, n_centre, neighbours, n_stray=0):
    """n_centre matches left -> right, n_stray more from the same left cell elsewhere, `neighbours` = [[cell, n], ..] -> FAR"""
    g = [[n_centre, left, Q, right]]
    if n_stray:
        g.append([n_stray, left, Q, FAR])
    g += [[n, c, Q, FAR] for c, n in neighbours]
    return dict(size1=[752, 480], size2=[752, 480], groups=g, seed=1)


_N8 = [[[9, 9], 3], [[10, 9], 3], [[11, 9], 3], [[9, 10], 3], [[11, 10], 3], [[9, 11], 3], [[10, 11], 3], [[11, 11], 3]]
_N3 = [[[1, 0], 2], [[0, 1], 1], [[1, 1], 1]]
_N5 = [[[9, 0], 3], [[11, 0], 3], [[9, 1], 2], [[10, 1], 2], [[11, 1], 2]]

# name -> (kind, arguments).  The expected masks of all of these are frozen in tests/golden/gms_ref.json from the compiled reference.
CONSTRUCTED = {
    # column-search ties: group 0 is the highest column, the last group the lowest
    "tie_cols_0_399": ("groups", _tie([0, 399])),
    "tie_cols_j_j1": ("groups", _tie([130, 131])),
    "tie_cols_j_j64": ("groups", _tie([130, 194])),
    "tie_cols_j_j128": ("groups", _tie([130, 258])),
    "tie_cols_63_64": ("groups", _tie([63, 64])),
    "tie_cols_127_128": ("groups", _tie([127, 128])),
    "tie_three_one_lane": ("groups", _tie([5, 69, 133])),
    "tie_three_lanes": ("groups", _tie([7, 200, 399])),
    "tie_three_adjacent": ("groups", _tie([318, 319, 320])),
    "tie_left_corner_cell": ("groups", _tie([64, 320], left=[0, 0])),
    # the tie exists in grid types 2 and 4 only: A (group 0) and B (group 2) share a left cell once x is shifted by half a cell; in
    # types 1 and 3 each loses its cell to a larger group (C, D), so nothing else marks A or B
    "tie_in_shifted_grid_only": ("groups", dict(size1=[752, 480], size2=[752, 480], seed=4, groups=[
        [24, [10, 10], [0.75, 0.25], list(col_cell(130))], [25, [10, 10], [0.25, 0.25], list(col_cell(300))],
        [24, [11, 10], [0.25, 0.25], list(col_cell(194))], [25, [11, 10], [0.75, 0.25], list(col_cell(350))]])),
    # score == thresh: mean count 4 over the neighbourhood gives 6 * sqrt(4) = 12.0 exactly, and the score is 12 (kept) or 11 (dropped)
    "thresh_equal_interior": ("groups", _thresh(L0, [5, 5], 12, _N8)),
    "thresh_short_interior": ("groups", _thresh(L0, [5, 5], 11, _N8, n_stray=1)),
    "thresh_equal_corner": ("groups", _thresh([0, 0], [0, 0], 12, _N3)),
    "thresh_short_corner": ("groups", _thresh([0, 0], [0, 0], 11, _N3, n_stray=1)),
    "thresh_equal_edge": ("groups", _thresh([10, 0], [10, 0], 12, _N5)),
    "thresh_short_edge": ("groups", _thresh([10, 0], [10, 0], 11, _N5, n_stray=1)),
    # survivor counts inside 1..149 and around 150 with non-empty masks: one consistent cluster among random matches
    "cluster_37": ("groups", dict(size1=[752, 480], size2=[752, 480], groups=[[37, [6, 12], Q, [9, 4]]], noise=600, seed=37)),
    "cluster_149": ("groups", dict(size1=[752, 480], size2=[752, 480], groups=[[149, [6, 12], Q, [9, 4]]], noise=600, seed=149)),
    "cluster_150": ("groups", dict(size1=[752, 480], size2=[752, 480], groups=[[150, [6, 12], Q, [9, 4]]], noise=600, seed=150)),
    "cluster_151": ("groups", dict(size1=[752, 480], size2=[752, 480], groups=[[151, [6, 12], Q, [9, 4]]], noise=600, seed=151)),
    # 7 + 7 matches either side of a border of the unshifted grid: each half fails grid types 1 and 3, together they pass 2 and 4
    "survives_shifted_grid_only": ("groups", dict(size1=[752, 480], size2=[752, 480], seed=2, groups=[
        [7, [10, 10], [0.75, 0.25], [5, 5]], [7, [11, 10], [0.25, 0.25], [5, 5]]])),
    # the one-workgroup loops
    **{f"smooth_n{n}": ("smooth", dict(n=n, seed=100 + n)) for n in (1, 63, 64, 65, 1023, 1024, 1025, 16384)},
    "one_cell_pair_4096": ("groups", dict(size1=[752, 480], size2=[752, 480], groups=[[4096, [4, 7], Q, [13, 2]]], shuffle=False)),
    "one_cell_pair_16384": ("groups", dict(size1=[752, 480], size2=[752, 480], groups=[[16384, [4, 7], Q, [13, 2]]], shuffle=False)),
    "query_path_3000": ("query_path", dict(n=3000, seed=6)),
    "query_path_65": ("query_path", dict(n=65, seed=7, n1=9)),
    # borders, sizes, several motions
    "border_grid_752x480": ("border_grid", dict(seed=1)),
    "border_grid_1241x376_to_640x480": ("border_grid", dict(size1=[1241, 376], size2=[640, 480], seed=2)),
    "border_grid_333x217": ("border_grid", dict(size1=[333, 217], size2=[333, 217], seed=3)),
    "three_motions_1280x720": ("smooth", dict(n=2500, seed=9, size1=[1280, 720], size2=[1280, 720], motions=3, border=200)),
    "two_sizes_borders": ("smooth", dict(n=1800, seed=10, size1=[640, 480], size2=[100, 37], motions=2, border=600)),
    "random_2000": ("random_matches", dict(n=2000, seed=11)),
    "right_x_equals_width": ("right_on_image_edge", dict(seed=12)),
}


def fuzz_case(seed: int):
    """(kind, arguments) of fuzz case `seed`: 20 .. 3000 matches, mixing smooth / several motions / random matches, image sizes and
    size1 != size2, and border keypoints"""
    rng = np.random.default_rng(1_000_003 * (seed + 1))
    n = int(rng.integers(20, 3001)) if rng.random() < 0.4 else int(rng.integers(20, 400))
    s1 = list(SIZES[rng.integers(len(SIZES))])
    s2 = s1 if rng.random() < 0.5 else list(SIZES[rng.integers(len(SIZES))])
    r = rng.random()
    if r < 0.12:
        return "random_matches", dict(n=n, seed=seed, size1=s1, size2=s2)
    if r < 0.2:
        return "right_on_image_edge", dict(n=n, seed=seed, size1=s1, size2=s2)
    return "smooth", dict(n=n, seed=seed, size1=s1, size2=s2, motions=int(rng.integers(1, 5)), outlier_frac=float(rng.choice([0.0, 0.2, 0.6])),
                          border=int(rng.choice([0, n // 4, n])))
