"""GMS inputs for the scale / rotation modes (chip_gms_filter_modes): the cases of tests/test_gms_modes_mirror.py (CPU),
tests/golden/make_golden_gms_modes.py and tests/test_gms_modes_gpu.py.  Built on tests/gms_cases.py: every case is (kind, arguments)
of a pure generator and is frozen by the SHA-256 of what it generates.

Cells as in gms_cases: a keypoint at fraction 0.25 of cell c of the 20 x 20 grid.  Such a right keypoint in cell (0, 0) or
(10, 0) sits in a corner resp. on the top edge of the right grid at EVERY scale (sides 20, 10, 14, 28, 40)."""
from __future__ import annotations

import numpy as np

import gms_cases as G

SIZE = [752, 480]
RING = (0, 1, 2, 5, 8, 7, 6, 3)          # the outer positions of a row-major 3 x 3 neighbourhood, clockwise from the top-left


def warp(n, seed, k45=0, zoom=1.0, outlier_frac=0.2, size1=SIZE, size2=SIZE):
    """n matches (i, t[i]): the right keypoint is the left one rotated by k45 * 45 degrees and zoomed about the centre, in NORMALISED
    coordinates (odd k45 shrunk by 0.7 so that the corners stay inside); the left keypoints are drawn from the part of image 1 whose
    image stays inside image 2; a fraction of the matches goes to a random keypoint instead."""
    rng = np.random.default_rng(seed)
    s = zoom * (0.7 if k45 % 2 else 1.0)
    half = 0.49 * min(1.0, 1.0 / s)
    u = rng.uniform(-half, half, (n, 2))
    a = np.deg2rad(45.0 * k45)
    v = (u @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])) * s
    pts = lambda w, size: np.stack([G._inside((w[:, 0] + 0.5) * size[0], size[0]), G._inside((w[:, 1] + 0.5) * size[1], size[1])], axis=1)
    t = np.arange(n, dtype=np.int32)
    out = rng.random(n) < outlier_frac
    t[out] = rng.integers(0, n, int(out.sum()))
    return dict(kp1=pts(u, size1), size1=tuple(size1), kp2=pts(v, size2), size2=tuple(size2), q=np.arange(n, dtype=np.int32), t=t)


KINDS = dict(G.KINDS, warp=warp)


def generate(kind: str, args: dict) -> dict:
    return KINDS[kind](**args)


def _valid(cell, pos):
    x, y = cell[0] + pos % 3 - 1, cell[1] + pos // 3 - 1
    return (x, y) if 0 <= x < G.GRID and 0 <= y < G.GRID else None


def remaining_pairs(left, right, rotation):
    """the (left cell, right cell) neighbour pairs that remain under rotation type `rotation` on two 20 x 20 grids, centre first"""
    pairs = [(4, 4)] + [(RING[k], RING[(k - (rotation - 1)) % 8]) for k in range(8)]
    return [(_valid(left, lp), _valid(right, rp)) for lp, rp in pairs if _valid(left, lp) and _valid(right, rp)]


def thresh_at_rotation(left, right, rotation, n_centre, n_stray=0):
    """n_centre matches left -> right whose score meets the threshold exactly under ONE rotation type: the left neighbours that remain
    under `rotation` hold 4 * numpair - 12 matches together (mean count 4 with a centre of 12: 6 * sqrt(4) = 12.0), every other left
    neighbour holds 7, which pushes the threshold of every other rotation type above 12.  All neighbours' matches go to FAR."""
    rem = [l for l, _ in remaining_pairs(left, right, rotation)][1:]
    total = 4 * (len(rem) + 1) - 12
    share = [total // len(rem) + (1 if i < total % len(rem) else 0) for i in range(len(rem))]
    assert min(share) >= 1
    g = [[n_centre, list(left), G.Q, list(right)]]
    if n_stray:
        g.append([n_stray, list(left), G.Q, G.FAR])
    g += [[c, list(cell), G.Q, G.FAR] for cell, c in zip(rem, share)]
    others = [_valid(left, p) for p in range(9) if p != 4 and _valid(left, p) and _valid(left, p) not in rem]
    g += [[7, list(cell), G.Q, G.FAR] for cell in others]
    return dict(size1=SIZE, size2=SIZE, groups=g, seed=1)


# the constructed score == thresh cases: (left cell, right cell, the rotation type that meets the threshold)
CORNER = ((10, 10), (0, 0), 3)             # right corner, left interior: four pairs under every rotation, the count sum differs
EDGE = ((10, 0), (10, 0), 2)               # both on the top edge: numpair = 6, 5, 4, 3, 3, 3, 4, 5 for rotation types 1..8

CASES = {
    # the synthetic motions: rotations by k * 45 degrees, zooms, one combination; 20 % wrong matches
    **{f"rotate_{45 * k}": ("warp", dict(n=3000, seed=200 + k, k45=k)) for k in range(8)},
    "zoom_2": ("warp", dict(n=3000, seed=210, zoom=2.0)),
    "zoom_sqrt2": ("warp", dict(n=3000, seed=211, zoom=float(np.sqrt(2.0)))),
    "zoom_inv_sqrt2": ("warp", dict(n=3000, seed=212, zoom=float(1.0 / np.sqrt(2.0)))),
    "zoom_half": ("warp", dict(n=3000, seed=213, zoom=0.5)),
    "rotate_90_zoom_2": ("warp", dict(n=3000, seed=214, k45=2, zoom=2.0)),
    # every constructed case of the plain filter but the one on which the reference leaves its tables under scale
    **{name: case for name, case in G.CONSTRUCTED.items() if name != "right_x_equals_width"},
    # one cell pair in an interior cell: every rotation type (and every scale) keeps all of it, so the first hypothesis (0, 1) must win
    "single_pair_interior": ("groups", dict(size1=SIZE, size2=SIZE, groups=[[40, [10, 10], G.Q, [5, 5]]], seed=3)),
    # score == thresh under one rotation type, below it under the others; one match short: below it under all
    "corner_equal_r3": ("groups", thresh_at_rotation(*CORNER, 12)),
    "corner_short_r3": ("groups", thresh_at_rotation(*CORNER, 11, n_stray=1)),
    "edge_equal_r2": ("groups", thresh_at_rotation(*EDGE, 12)),
    "edge_short_r2": ("groups", thresh_at_rotation(*EDGE, 11, n_stray=1)),
    # nothing to choose: no hypothesis keeps a match
    "random_no_choice": ("random_matches", dict(n=300, seed=5)),
}
NO_CHOICE = ("random_no_choice", "thresh_short_corner", "corner_short_r3", "edge_short_r2")
LADDER = tuple(f"smooth_n{n}" for n in (1, 63, 64, 65, 1023, 1024, 1025, 16384))
assert set(LADDER) <= set(CASES)

FLAG_PAIRS = ((0, 1), (1, 0), (1, 1))      # (with_scale, with_rotation)


def modes_of(with_scale, with_rotation) -> int:
    return (1 if with_scale else 0) | (2 if with_rotation else 0)
