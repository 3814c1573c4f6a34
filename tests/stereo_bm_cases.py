"""Inputs for the tests of the block matcher (tests/test_stereo_bm_mirror.py on the CPU, tests/test_stereo_bm_gpu.py on the device):
rectified 8-bit pairs of small shapes whose widths cover all four residues mod 4, one full 752 x 480 frame at the defaults, and the
pair case set of tests/disparity_cases.py with every frame carrying a synthetic stereo pair.  Everything is seeded, built once per
process and left unchanged; the properties claimed here are asserted by the CPU test."""
from __future__ import annotations

import functools

import numpy as np

import disparity_cases as DC
import np_mirror_stereo_bm as BM

# (w, h, nd, block): the smallest with one defined pixel, two with none, then widths of every residue mod 4 and every nd
SHAPES = ((20, 5, 16, 5), (19, 5, 16, 5), (20, 4, 16, 5), (37, 9, 16, 5), (41, 11, 32, 7), (90, 23, 48, 21), (101, 25, 64, 21))
N_DEFINED = (1, 0, 0, 90, 20, 69, 90)                                # defined pixels per shape
FULL = (752, 480)
MAX_ND = 64
EVENTS = ("T_at_threshold", "T_below_threshold", "thresh_at_2_filtered", "thresh_at_1_kept", "q_zero", "truncation", "equal_minima",
          "D_first", "D_last")
NOISE_SHAPE = (37, 9, 16, 5)
NOISE_TEXTURE_THRESHOLD = 100                                         # about the median T of the noise pairs
NOISE_RATIOS = (5, 0)                                                 # each noise pair under both
NOISE_SEARCH_LIMIT = 4000


def texture(rng, w: int, h: int) -> np.ndarray:
    """(h, w) uint8: a random texture, smoothed once with a 3 x 3 box (edges replicated)"""
    t = rng.integers(0, 256, (h, w)).astype(np.int32)
    p = np.pad(t, 1, mode="edge")
    s = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((s + 4) // 9).astype(np.uint8)


def planted(rng, w: int, h: int, shift) -> tuple:
    """-> (left, right): left[y][x] = right[y][x - shift] on a smoothed texture wider than the image, so every column has content;
    shift an integer, or s + 0.5: the rounded mean of the shifts s and s + 1"""
    base = texture(rng, w + MAX_ND, h)
    cut = lambda s: base[:, MAX_ND - s:MAX_ND - s + w]               # noqa: E731
    right = cut(0)
    if float(shift) == int(shift):
        return np.ascontiguousarray(cut(int(shift))), np.ascontiguousarray(right)
    s = int(np.floor(shift))
    left = (cut(s).astype(np.int32) + cut(s + 1).astype(np.int32) + 1) // 2
    return left.astype(np.uint8), np.ascontiguousarray(right)


def column_pattern(values, w: int, h: int, phase: int = 0) -> np.ndarray:
    v = np.asarray(values, np.uint8)
    return np.ascontiguousarray(np.broadcast_to(v[(np.arange(w) + phase) % len(v)], (h, w)))


def case(name, left, right, nd, block, **kw) -> dict:
    return dict(name=name, left=left, right=right, params=BM.params(num_disparities=nd, block_size=block, **kw))


@functools.lru_cache(maxsize=None)
def small_cases() -> tuple:
    """every content family on every small shape"""
    out = []
    for k, (w, h, nd, block) in enumerate(SHAPES):
        tag = f"{w}x{h}_nd{nd}_b{block}"
        rng = np.random.default_rng(7000 + k)
        for s in (0, 1, nd - 2, nd - 1):
            out.append(case(f"shift{s}_{tag}", *planted(rng, w, h, s), nd, block))
        out.append(case(f"half_{tag}", *planted(rng, w, h, nd // 2 + 0.5), nd, block))
        out.append(case(f"flat_{tag}", np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8), nd, block))
        out.append(case(f"flat_apart_{tag}", np.full((h, w), 10, np.uint8), np.full((h, w), 200, np.uint8), nd, block))
        period8 = column_pattern((0, 40, 90, 160, 250, 130, 60, 20), w, h)
        for ratio in (15, 0):                                         # equal minima at every multiple of 8: the largest wins, or none
            out.append(case(f"period8_u{ratio}_{tag}", period8, period8, nd, block, uniqueness_ratio=ratio))
        # column pairs 0, 0, 255, 255: P = 0, 126, 126, 0 at cap 63; the right image two columns on: every byte differs by 126
        out.append(case(f"swing_{tag}", column_pattern((0, 0, 255, 255), w, h), column_pattern((0, 0, 255, 255), w, h, 2), nd, block,
                        prefilter_cap=63, uniqueness_ratio=0))
    return tuple(out)


def noise_pair(seed: int) -> tuple:
    w, h, _, _ = NOISE_SHAPE
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, (h, w)).astype(np.uint8), rng.integers(0, 4, (h, w)).astype(np.uint8)


def events_of(c: dict) -> dict:
    """event -> number of defined pixels of the case at which it occurs (EVENTS; see the issue's list)"""
    det, p = BM.details(c["left"], c["right"], c["params"]), c["params"]
    if det is None:
        return dict.fromkeys(EVENTS, 0)
    nd, tex, ratio = p["num_disparities"], p["texture_threshold"], p["uniqueness_ratio"]
    sad, D, thresh, m = det["sad"], det["D"], det["thresh"], det["m"]
    kept = det["textured"] & det["unique"]
    ds = np.arange(nd)[:, None, None]
    far, at1, at2 = np.abs(ds - D[None]) > 1, np.abs(ds - D[None]) == 1, np.abs(ds - D[None]) == 2
    on = ratio > 0
    # the equality decides: a d two away sits exactly on thresh and nothing further away lies below it
    at2_decides = det["textured"] & (at2 & (sad == thresh[None])).any(0) & ~(far & (sad < thresh[None])).any(0) & ~det["unique"]
    at1_kept = kept & (at1 & (sad == thresh[None])).any(0)
    pn, q = det["p"] - det["n"], det["q"]
    return dict(T_at_threshold=int((det["T"] == tex).sum()), T_below_threshold=int((det["T"] == tex - 1).sum()),
                thresh_at_2_filtered=int(at2_decides.sum()) if on else 0, thresh_at_1_kept=int(at1_kept.sum()) if on else 0,
                q_zero=int((kept & (q == 0)).sum()),
                truncation=int((kept & (pn < 0) & (q != 0) & ((pn * 256) % np.maximum(q, 1) != 0)).sum()),
                equal_minima=int((kept & ((sad == m[None]).sum(0) > 1)).sum()),
                D_first=int((kept & (D == 0)).sum()), D_last=int((kept & (D == nd - 1)).sum()))


@functools.lru_cache(maxsize=None)
def noise_cases() -> tuple:
    """low-amplitude noise (values 0 .. 3) at block 5: seeds 0, 1, ... are searched, a seed is kept when it shows an event none before
    it has shown, until every event of EVENTS has a pixel"""
    _, _, nd, block = NOISE_SHAPE
    out, missing = [], set(EVENTS)
    for seed in range(NOISE_SEARCH_LIMIT):
        left, right = noise_pair(seed)
        cs = [case(f"noise{seed}_u{r}", left, right, nd, block, texture_threshold=NOISE_TEXTURE_THRESHOLD, uniqueness_ratio=r) for r in NOISE_RATIOS]
        for c in cs:
            new = {e for e, k in events_of(c).items() if k} & missing
            if new:
                out.append(c)
                missing -= new
        if not missing:
            return tuple(out)
    raise AssertionError(f"no noise pair with {sorted(missing)} among {NOISE_SEARCH_LIMIT} seeds")


def tiled_pair(rng, w: int, h: int, tile: int = 94, lo: int = 4, hi: int = 40) -> tuple:
    """-> (left, right, shifts): a smoothed texture seen under a piecewise-constant integer disparity, one value of lo .. hi per tile"""
    base = texture(rng, w + MAX_ND, h)
    shifts = rng.integers(lo, hi + 1, ((h + tile - 1) // tile, (w + tile - 1) // tile))
    s = np.repeat(np.repeat(shifts, tile, 0), tile, 1)[:h, :w]
    x = np.arange(w)[None, :] + MAX_ND - s
    return np.take_along_axis(base, x, 1), np.ascontiguousarray(base[:, MAX_ND:]), s


@functools.lru_cache(maxsize=None)
def full_frame() -> dict:
    """the 752 x 480 pair at the defaults"""
    left, right, shifts = tiled_pair(np.random.default_rng(752480), *FULL)
    c = case("full", left, right, 64, 21)
    c["shifts"] = shifts
    return c


@functools.lru_cache(maxsize=None)
def full_frame_map() -> np.ndarray:
    d = BM.vectorised(full_frame()["left"], full_frame()["right"], full_frame()["params"])
    d.setflags(write=False)
    return d


def all_cases() -> tuple:
    return small_cases() + noise_cases()


# ------------------------------------------------------------------------------------------------ the pair set from stereo pairs
PAIR_PARAMS = BM.params()


@functools.lru_cache(maxsize=None)
def pair_of_size(w: int, h: int) -> tuple:
    """-> (left, right, mirror map) for the frames of that image size: one synthetic pair per size, its mirror map computed once"""
    if (w, h) == FULL:
        return full_frame()["left"], full_frame()["right"], full_frame_map()
    left, right, _ = tiled_pair(np.random.default_rng(1000 * w + h), w, h, tile=max(8, min(w, h) // 2), lo=4, hi=max(4, min(40, w // 4)))
    return left, right, BM.vectorised(left, right, PAIR_PARAMS)


@functools.lru_cache(maxsize=None)
def pair_set_frames() -> dict:
    """name -> dict(desc, kp, left, right, disp): the frames of tests/disparity_cases.py, the disparity replaced by a synthetic rectified
    pair of the frame's size and by the mirror map of that pair"""
    out = {}
    for name, f in DC.frames().items():
        h, w = f["disp"].shape
        left, right, disp = pair_of_size(w, h)
        out[name] = dict(desc=f["desc"], kp=f["kp"], left=left, right=right, disp=disp)
    return out
