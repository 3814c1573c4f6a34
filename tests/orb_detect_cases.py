"""Small named images for the ORB detector (tests/np_mirror_orb_detect.py, cerebro_amd/csrc/orb.hip): each a dict(name, img, params).
The constructed events of tests/test_orb_detect_mirror.py are built from the same helpers."""
from __future__ import annotations

import functools

import numpy as np

import np_mirror_orb_detect as O

FULL = (752, 480)
THRESHOLDS = (0, 1, 20, 255)
# compaction geometry of cerebro_amd/csrc/orb.hip, for the shapes that sit on it
SCORE_TILE_W, SCORE_TILE_H = 128, 16
WAVE, CAND_THREADS, SELECT_THREADS = 64, 256, 1024


def flat(w: int, h: int, v: int = 50) -> np.ndarray:
    return np.full((h, w), v, np.uint8)


def with_dots(w: int, h: int, dots, base: int = 50) -> np.ndarray:
    """isolated pixels: dots is a list of (x, y, value)"""
    img = flat(w, h, base)
    for x, y, v in dots:
        img[y, x] = v
    return img


def dot_grid(nx: int, ny: int, border: int = 16, pitch: int = 8, value=200, base: int = 50) -> np.ndarray:
    """nx x ny isolated pixels, `pitch` apart, the first at (border, border): identical 7 x 7 surroundings, so identical S and R.  value: an
    int, or a function (i, j) -> int"""
    w, h = 2 * border + (nx - 1) * pitch + 1, 2 * border + (ny - 1) * pitch + 1
    img = flat(w, h, base)
    for j in range(ny):
        for i in range(nx):
            img[border + j * pitch, border + i * pitch] = value(i, j) if callable(value) else value
    return img


def texture(rng, w: int, h: int, cell: int = 5) -> np.ndarray:
    """blocks of `cell` pixels of random brightness under pixel noise: corners at every scale of the pyramid"""
    blocks = rng.integers(30, 226, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    img = np.repeat(np.repeat(blocks, cell, 0), cell, 1)[:h, :w] + rng.integers(-25, 26, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def case(name: str, img, **kw) -> dict:
    return dict(name=name, img=np.ascontiguousarray(img, dtype=np.uint8), params=O.params(**kw))


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    rng = np.random.default_rng(20260)
    edge = flat(80, 72); edge[:, 40:] = 180
    square = flat(90, 84); square[30:60, 28:58] = 210
    ramp = (np.arange(96)[None, :] * 2 + np.arange(70)[:, None]).astype(np.uint8)
    adjacent = with_dots(70, 70, [(34, 35, 200), (35, 35, 200)])
    return (case("isolated", with_dots(65, 65, [(32, 32, 200)])),
            case("edge", edge, n_levels=2),
            case("square", square, n_levels=3, border=16),
            case("ramp", ramp, n_levels=2, border=16),
            case("adjacent_equal", adjacent, n_levels=1),
            case("dots", dot_grid(9, 7, border=31), n_levels=2, n_features=40),
            case("texture", texture(rng, 131, 97), n_levels=4, n_features=300, border=16),
            case("texture_odd", texture(rng, 98, 71, cell=3), n_levels=8, n_features=77, border=16),
            case("noise", rng.integers(0, 256, (75, 66)).astype(np.uint8), n_levels=3, n_features=500, border=17))


def by_name(name: str) -> dict:
    (c,) = [c for c in all_cases() if c["name"] == name]
    return c


@functools.lru_cache(maxsize=None)
def full_frame() -> np.ndarray:
    """the 752 x 480 textured frame: at the defaults every level with a detection area has more candidates than its quota"""
    img = texture(np.random.default_rng(752480), *FULL)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def full_frame_mirror() -> tuple:
    return O.detect(full_frame())
