"""CPU restatement in integers of the ORB descriptor (cerebro_amd/csrc/orb.hip: orb_blur, orb_describe; definition in
include/cerebro_hip.h, "ORB descriptors on the device").  The definition is this project's own -- its own 256-pair pattern from a stated
generator, 32 orientation bins from the integer moments, an integer 7-tap blur with clamped borders -- and is NOT pinned against OpenCV:

    blur     : g = 9 17 24 28 24 17 9 (sum 128);  H[y][x] = sum_i g[i+3] I[y][clamp(x+i)],
               B[y][x] = (sum_j g[j+3] H[clamp(y+j)][x] + 8192) >> 14
    bin      : the k of 32 that maximises m10 C[k] + m01 S[k] (exact integers; ties to the lowest k), C[k] = round(16384 cos(2 pi k / 32))
    pattern  : s = 0x4F52425F42524945; draw: s = s * 6364136223846793005 + 1442695040888963407 mod 2^64, value (s >> 33) % 11 - 5;
               a coordinate is the sum of three draws; an attempt is x1, y1, x2, y2 (12 draws), rejected if a point has x^2 + y^2 > 169, if
               the points are closer than 3 ((dx^2 + dy^2) < 9) or if the pair, in either order, is there already; the first 256 accepted
    steered  : T[k][pair] = (rx1, ry1, rx2, ry2), rx = (x C[k] - y S[k] + 8192) >> 14, ry = (x S[k] + y C[k] + 8192) >> 14
    bit p    : B_l[y + ry1][x + rx1] < B_l[y + ry2][x + rx2] at the keypoint's level position and bin; byte j = pairs 8j .. 8j + 7, LSB first

Two forms: the `_loops` functions transcribe the definition element by element; the others are vectorised."""
from __future__ import annotations

import functools

import numpy as np

import np_mirror_orb_detect as O

I64 = np.int64
G = (9, 17, 24, 28, 24, 17, 9)
BINS = 32
DESC_BYTES = 32
N_PAIRS = 256
_Q = (16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0)          # C[0 .. 8]; S[k] = C[8 - k] there
SEED = 0x4F52425F42524945
MUL, INC, MASK = 6364136223846793005, 1442695040888963407, (1 << 64) - 1


def _tables():
    C, S = [0] * BINS, [0] * BINS
    for k in range(9):
        C[k], S[k] = _Q[k], _Q[8 - k]
    for k in range(BINS - 8):                                          # a quarter turn on: C[k + 8] = -S[k], S[k + 8] = C[k]
        C[k + 8], S[k + 8] = -S[k], C[k]
    return tuple(C), tuple(S)


COS, SIN = _tables()


# ---------------------------------------------------------------------------------------------------- blur
def blur_loops(img) -> np.ndarray:
    I = np.asarray(img)
    h, w = I.shape
    H = [[sum(G[i + 3] * int(I[y, min(max(x + i, 0), w - 1)]) for i in range(-3, 4)) for x in range(w)] for y in range(h)]
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = (sum(G[j + 3] * H[min(max(y + j, 0), h - 1)][x] for j in range(-3, 4)) + 8192) >> 14
    return out


def blur(img) -> np.ndarray:
    I = np.asarray(img).astype(I64)
    h, w = I.shape
    if h < 1 or w < 1:
        return np.zeros((max(h, 0), max(w, 0)), np.uint8)
    xs, ys = np.arange(w), np.arange(h)
    H = sum(G[i + 3] * I[:, np.clip(xs + i, 0, w - 1)] for i in range(-3, 4))
    V = sum(G[j + 3] * H[np.clip(ys + j, 0, h - 1), :] for j in range(-3, 4))
    return ((V + 8192) >> 14).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- orientation bin
def orb_bin(m10: int, m01: int) -> int:
    """Python integers: no width to overflow"""
    best, at = None, 0
    for k in range(BINS):
        v = int(m10) * COS[k] + int(m01) * SIN[k]
        if best is None or v > best:
            best, at = v, k
    return at


def bin_is_unique(m10: int, m01: int) -> bool:
    v = [int(m10) * COS[k] + int(m01) * SIN[k] for k in range(BINS)]
    return v.count(max(v)) == 1


def bins(m10, m01) -> np.ndarray:
    """int64: |m| <= 749 * 15 * 255 < 2^22 for moments of a patch, any int32 pair fits (2^31 * 2^14 * 2 < 2^63)"""
    v = np.asarray(m10, I64)[:, None] * np.array(COS, I64)[None, :] + np.asarray(m01, I64)[:, None] * np.array(SIN, I64)[None, :]
    return np.argmax(v, axis=1).astype(np.int32)                        # argmax: the first of equals


# ---------------------------------------------------------------------------------------------------- pattern, steered table
@functools.lru_cache(maxsize=None)
def pattern_with_attempts():
    """-> (the (256, 4) int8 pairs x1, y1, x2, y2, the attempts it took)"""
    s = SEED

    def draw():
        nonlocal s
        s = (s * MUL + INC) & MASK
        return (s >> 33) % 11 - 5

    def coord():
        return draw() + draw() + draw()
    pairs, seen, attempts = [], set(), 0
    while len(pairs) < N_PAIRS:
        attempts += 1
        x1 = coord(); y1 = coord(); x2 = coord(); y2 = coord()
        if x1 * x1 + y1 * y1 > 169 or x2 * x2 + y2 * y2 > 169:
            continue
        if (x1 - x2) ** 2 + (y1 - y2) ** 2 < 9:
            continue
        if (x1, y1, x2, y2) in seen or (x2, y2, x1, y1) in seen:
            continue
        seen.add((x1, y1, x2, y2))
        pairs.append((x1, y1, x2, y2))
    out = np.array(pairs, np.int8)
    out.setflags(write=False)
    return out, attempts


def pattern() -> np.ndarray:
    return pattern_with_attempts()[0]


@functools.lru_cache(maxsize=None)
def steered() -> np.ndarray:
    """(32, 256, 4) int8: rx1, ry1, rx2, ry2"""
    P = pattern().astype(I64)
    T = np.zeros((BINS, N_PAIRS, 4), np.int8)
    for k in range(BINS):
        c, s = COS[k], SIN[k]
        for j in (0, 2):
            x, y = P[:, j], P[:, j + 1]
            T[k, :, j] = (x * c - y * s + 8192) >> 14
            T[k, :, j + 1] = (x * s + y * c + 8192) >> 14
    T.setflags(write=False)
    return T


def steered_loops() -> np.ndarray:
    T = np.zeros((BINS, N_PAIRS, 4), np.int8)
    for k in range(BINS):
        for p, (x1, y1, x2, y2) in enumerate(pattern().tolist()):
            T[k, p] = ((x1 * COS[k] - y1 * SIN[k] + 8192) >> 14, (x1 * SIN[k] + y1 * COS[k] + 8192) >> 14,
                       (x2 * COS[k] - y2 * SIN[k] + 8192) >> 14, (x2 * SIN[k] + y2 * COS[k] + 8192) >> 14)
    return T


# ---------------------------------------------------------------------------------------------------- descriptors
def describe_loops(blurred: list, recs) -> np.ndarray:
    T = steered()
    out = np.zeros((len(recs), DESC_BYTES), np.uint8)
    for i, r in enumerate(recs):
        B, x, y = blurred[int(r["level"])], int(r["x_level"]), int(r["y_level"])
        k = orb_bin(int(r["m10"]), int(r["m01"]))
        for p in range(N_PAIRS):
            rx1, ry1, rx2, ry2 = (int(v) for v in T[k, p])
            if int(B[y + ry1, x + rx1]) < int(B[y + ry2, x + rx2]):
                out[i, p >> 3] |= 1 << (p & 7)
    return out


def describe(blurred: list, recs) -> np.ndarray:
    out = np.zeros((len(recs), DESC_BYTES), np.uint8)
    if not len(recs):
        return out
    T = steered().astype(I64)
    k = bins(recs["m10"], recs["m01"])
    x, y, lv = recs["x_level"].astype(I64), recs["y_level"].astype(I64), recs["level"]
    for l in np.unique(lv):
        m = np.nonzero(lv == l)[0]
        B, t = blurred[int(l)], T[k[m]]                                  # t: (n, 256, 4)
        a = B[y[m, None] + t[:, :, 1], x[m, None] + t[:, :, 0]]
        b = B[y[m, None] + t[:, :, 3], x[m, None] + t[:, :, 2]]
        out[m] = np.packbits(a < b, axis=1, bitorder="little")
    return out


# ---------------------------------------------------------------------------------------------------- the whole call
def detect_describe(img, p: dict | None = None, loops: bool = False, stages: dict | None = None):
    """chip_orb_detect_describe -> (records, level_counts[8], the (n, 32) uint8 descriptors).  stages, if given, receives the detector's
    and 'blurred'."""
    st: dict = {}
    recs, counts = O.detect(img, p, loops, st)
    blurred = [(blur_loops if loops else blur)(im) for im in st["images"]]
    if stages is not None:
        stages.update(st, blurred=blurred)
    return recs, counts, (describe_loops if loops else describe)(blurred, recs)
