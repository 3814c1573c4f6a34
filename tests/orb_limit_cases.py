"""Images that drive the ORB front end (cerebro_amd/csrc/orb.hip) to the limits it is written around: a side of CHIP_ORB_MAX_SIDE, strip
segments filled to `cap`, full strips next to empty ones, keys of both signs, more than 4096 tied keys, 16384 kept keypoints.  numpy
only, seeded, every image and every mirror result made once.

All are DOTTED LINES on a flat image of 40: on chosen rows a bright pixel on every second column of the detection rectangle, x0, x0 + 2,
... <= x1, each dot random in 100 .. 255 ("distinct keys") or all of one value ("tied keys"), the lines at least 4 rows apart.  A dot's
FAST ring (radius 3) touches its own row only at x +- 3, odd offsets that hold no dot, so every dot is a strict 3 x 3 maximum of score
v - 41 and every background neighbour scores -1: a line across the rectangle gives exactly cap = ceil(width of the rectangle / 2)
candidates in its strip of two rows, and with lines every 4 rows full strips alternate with empty ones.
tests/test_orb_limits_mirror.py proves these properties from the mirror; tests/test_orb_limits_gpu.py relies on them."""
from __future__ import annotations

import functools

import numpy as np

import np_mirror_orb_describe as D
import np_mirror_orb_detect as O

BORDER = 16
BASE, TIED_VALUE = 40, 200
STRIP_ROWS = 2                                   # orb_candidates: a workgroup per strip of two rows of the detection rectangle
MAX_SIDE, MAX_KEPT = 4096, 16384                 # CHIP_ORB_MAX_SIDE, CHIP_MATCH_MAX_KEYPOINTS
SEED = 1
SEEDS = {"4096x73": 33}                          # the seed at which level 4 of 8 has the 538 candidates the tests name; every other image: SEED


def rectangle(w: int, h: int) -> tuple:
    """x0, y0, x1, y1 of level 0 at BORDER"""
    return BORDER, BORDER, w - 1 - BORDER, h - 1 - BORDER


def cap_of(w: int) -> int:
    """the candidate segment of a strip: one strict maximum per 2 x 2 block"""
    x0, _, x1, _ = rectangle(w, 1)
    return (x1 - x0 + 2) // 2


def strips_of(h: int) -> int:
    _, y0, _, y1 = rectangle(1, h)
    return (y1 - y0 + STRIP_ROWS) // STRIP_ROWS


def line_rows(h: int, second_row: bool = False) -> tuple:
    """every fourth row of the rectangle, from its first row or from the second row of the first strip"""
    _, y0, _, y1 = rectangle(1, h)
    return tuple(range(y0 + (1 if second_row else 0), y1 + 1, 4))


def dotted_lines(w: int, h: int, rows, value: int | None = None, split: bool = False, seed: int = SEED) -> np.ndarray:
    """value None: distinct keys (every dot random in 100 .. 255).  split: the left half of a line's dots on its row, the right half on
    the row below, so that a strip collects its segment over both of its rows"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), BASE, np.uint8)
    x0, _, x1, _ = rectangle(w, h)
    xs = np.arange(x0, x1 + 1, 2)
    half = len(xs) // 2
    for y in rows:
        v = rng.integers(100, 256, len(xs)) if value is None else np.full(len(xs), value)
        if split:
            img[y, xs[:half]] = v[:half]
            img[y + 1, xs[half:]] = v[half:]
        else:
            img[y, xs] = v
    img.setflags(write=False)
    return img


# a case is "<shape>" or "<shape>_<kind>", kind: row2 (the lines on the second row of their strips), split, tied
_SHAPES = {"4096x41": (4096, 41), "4095x41": (4095, 41), "41x4096": (41, 4096), "300x45": (300, 45), "301x45": (301, 45), "4096x73": (4096, 73)}
SIDES = ("4096x41", "4095x41", "41x4096")
NAMES = tuple(_SHAPES) + tuple(n + "_row2" for n in _SHAPES) + ("301x45_split", "4096x41_tied", "4096x73_tied")


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """dict(name, img, w, h, rows, cap, nstrips, full: the strips a whole line falls into, n_candidates, split, tied)"""
    base, _, kind = name.partition("_")
    w, h = _SHAPES[base]
    rows = line_rows(h, second_row=kind == "row2")
    split, tied = kind == "split", kind == "tied"
    img = dotted_lines(w, h, rows, value=TIED_VALUE if tied else None, split=split, seed=SEEDS.get(name, SEED))
    _, y0, _, y1 = rectangle(w, h)
    cap = cap_of(w)
    if split:                                    # a line's second half lies a row lower: outside the rectangle for a line on its last row
        full = tuple((y - y0) // STRIP_ROWS for y in rows if y + 1 <= y1)
        n = sum(cap if y + 1 <= y1 else cap // 2 for y in rows)
    else:
        full = tuple((y - y0) // STRIP_ROWS for y in rows)
        n = cap * len(rows)
    return dict(name=name, img=img, w=w, h=h, rows=rows, cap=cap, nstrips=strips_of(h), full=full, n_candidates=n, split=split, tied=tied)


def params(n_levels: int = 1, n_features: int = MAX_KEPT) -> dict:
    return O.params(n_levels=n_levels, n_features=n_features, border=BORDER)


@functools.lru_cache(maxsize=None)
def mirror(name: str, n_levels: int = 1, n_features: int = MAX_KEPT) -> tuple:
    """(records, counts, descriptors, stages) of the vectorised mirror; at one level and 16384 features every candidate of every case but
    4096x73 is kept"""
    st: dict = {}
    recs, counts, desc = D.detect_describe(case(name)["img"], params(n_levels, n_features), stages=st)
    for a in (recs, desc):
        a.setflags(write=False)
    return recs, counts, desc, st


def level0_candidates(name: str) -> tuple:
    """(rasters ascending, R) of level 0 from the mirror's stage functions"""
    c = case(name)
    L = O.plan(c["w"], c["h"], params())[0]
    ras = O.candidates(O.score_plane(c["img"]), L, 0)
    return ras, O.harris(c["img"], ras)


def strip_counts(c: dict, ys) -> np.ndarray:
    """candidates per strip from their level rows"""
    return np.bincount((np.asarray(ys, np.int64) - BORDER) // STRIP_ROWS, minlength=c["nstrips"])


def rasters_of(recs, w: int) -> np.ndarray:
    return recs["y_level"].astype(np.int64) * w + recs["x_level"]


def selected(recs, w: int, q: int):
    """the records a quota of q keeps of the one-level all-kept records `recs`"""
    return recs[O.select(recs["response"], rasters_of(recs, w), q)]


# quota 0 on levels that have candidates: the 160 x 120 texture of the detector's tests at 8 levels
QUOTA0_FEATURES = (1, 2, 7, 8, 9, 15, 16)
QUOTA0_COUNTS = {1: [0, 0, 0, 0, 0, 0, 0, 1], 2: [0, 0, 0, 0, 0, 0, 0, 2], 7: [2, 1, 1, 1, 1, 1, 0, 0], 8: [2, 1, 1, 1, 1, 1, 1, 0]}


@functools.lru_cache(maxsize=None)
def quota0_image() -> np.ndarray:
    import orb_detect_cases as OC
    img = OC.texture(np.random.default_rng(160120), 160, 120)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def quota0_mirror(n_features: int) -> tuple:
    return D.detect_describe(quota0_image(), params(8, n_features))
