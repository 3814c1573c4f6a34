"""Named images for the ORB descriptor (tests/np_mirror_orb_describe.py, cerebro_amd/csrc/orb.hip: orb_blur, orb_describe), next to
those of the detector (tests/orb_detect_cases.py): each a dict(name, img, params)."""
from __future__ import annotations

import functools

import numpy as np

import np_mirror_orb_describe as D
import orb_detect_cases as OC

# geometry of orb_blur in cerebro_amd/csrc/orb.hip: a workgroup makes a tile of 128 x 32 pixels, a thread 16 pixels of a row
BLUR_TILE_W, BLUR_TILE_H = 128, 32
WAVE, DESCRIBE_WAVES = 64, 4                     # orb_describe: one wave per keypoint, four waves a workgroup
DOTS = (40, 30)                                  # the detector's 1200 identical dots


def corners_of_the_rectangle(w: int = 90, h: int = 70, border: int = 16) -> np.ndarray:
    """a bright pixel on each corner pixel of the detection rectangle of a w x h image, over dim texture: a strict maximum there"""
    img = (OC.texture(np.random.default_rng(7 * w + h), w, h, cell=6) // 4 + 20).astype(np.uint8)
    for x in (border, w - 1 - border):
        for y in (border, h - 1 - border):
            img[y, x] = 255
    return img


def planted_angles(n: int = 32, pitch: int = 48, border: int = 40) -> np.ndarray:
    """n bright half planes through a point, turned by 360 / n degrees from one to the next, each inside a disc of radius 15: the
    intensity centroid of patch i points along angle i"""
    cols = 8
    rows = (n + cols - 1) // cols
    w, h = 2 * border + (cols - 1) * pitch + 1, 2 * border + (rows - 1) * pitch + 1
    img = np.full((h, w), 40, np.uint8)
    yy, xx = np.mgrid[-15:16, -15:16]
    for i in range(n):
        a = 2 * np.pi * (i + 0.5) / n            # between two bin centres' boundaries: away from every tie
        cx, cy = border + (i % cols) * pitch, border + (i // cols) * pitch
        side = xx * np.cos(a) + yy * np.sin(a) > 1.5
        patch = np.where(side & (xx * xx + yy * yy <= 15 * 15), 220, 40).astype(np.uint8)
        patch[15, 15] = 255                      # a strict FAST maximum at the centre
        img[cy - 15:cy + 16, cx - 15:cx + 16] = patch
    return img


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    rng = np.random.default_rng(20261)
    return (OC.case("corners_b16", corners_of_the_rectangle(), n_levels=1, n_features=400, border=16),
            OC.case("border64", OC.texture(rng, 171, 150), n_levels=2, n_features=200, border=64),
            OC.case("texture_w_mod4_1", OC.texture(rng, 133, 101), n_levels=3, n_features=250, border=16),
            OC.case("texture_w_mod4_2", OC.texture(rng, 134, 99, cell=4), n_levels=3, n_features=250, border=20),
            OC.case("texture_w_mod4_3", OC.texture(rng, 135, 98, cell=7), n_levels=8, n_features=120, border=16),
            OC.case("planted_angles", planted_angles(), n_levels=1, n_features=2000, border=16),
            OC.case("identical_dots", OC.dot_grid(*DOTS, border=16, pitch=8), n_levels=1, n_features=DOTS[0] * DOTS[1], border=16))


def by_name(name: str) -> dict:
    (c,) = [c for c in all_cases() if c["name"] == name]
    return c


@functools.lru_cache(maxsize=None)
def full_frame_mirror() -> tuple:
    """(records, counts, descriptors, stages) of the detector's 752 x 480 frame at the defaults"""
    st: dict = {}
    recs, counts, desc = D.detect_describe(OC.full_frame(), stages=st)
    return recs, counts, desc, st


@functools.lru_cache(maxsize=None)
def mirror_of(name: str) -> tuple:
    c = by_name(name) if any(c["name"] == name for c in all_cases()) else OC.by_name(name)
    return D.detect_describe(c["img"], c["params"])
