"""CPU restatement in integers of the ORB detector (cerebro_amd/csrc/orb.hip; definition in include/cerebro_hip.h, "ORB keypoint
detection on the device").  The definition is this project's own, modelled on cv::ORB::detect with HARRIS_SCORE; it is NOT pinned
against OpenCV.  All image arithmetic is integer:

    levels   : s_0 = 1.0, s_l = s_(l-1) * 1.2 (double); w_l = (int)floor(w / s_l + 0.5), h_l alike
    quotas   : f = 1.0 / 1.2, g = f multiplied n_levels times, nd = n_features * (1 - f) / (1 - g); quota_l = min((int)floor(nd + 0.5),
               n_features - sum), nd *= f; the last level gets n_features - sum
    pyramid  : X = ((2x + 1) * w_(l-1) * 1024) // w_l - 1024 clamped to [0, (w_(l-1) - 1) * 2048]; x0 = X >> 11, a = X & 2047,
               x1 = min(x0 + 1, w_(l-1) - 1); y alike with b; value = (I00 (2048-a)(2048-b) + I01 a (2048-b) + I10 (2048-a) b +
               I11 a b + (1 << 21)) >> 22
    S        : b = max over the 16 cyclic arcs of 9 ring pixels of min(I_k - I_p), d = the same with I_p - I_k, S = max(b, d) - 1;
               UNDEFINED = -256 within 3 of an edge
    candidate: in the detection rectangle, S >= fast_threshold and S > the S of all eight neighbours
    R        = 25 (a bb - c c) - (a + bb)^2 with a, bb, c the 7 x 7 sums of Ix^2, Iy^2, Ix Iy (3 x 3 Sobel)
    selection: per level the quota_l largest R, ties to the lower raster index; output level ascending, raster order inside
    moments  : m10 = sum u I, m01 = sum v I over the 749 pixels |u| <= umax[|v|], |v| <= 15

Two forms: the `_loops` functions transcribe the definition pixel by pixel; the others are vectorised.  Python integers / int64."""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = dict(n_features=5000, n_levels=8, fast_threshold=0, border=31)
UNDEFINED = -256
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
# chip_orb_keypoint, 32 bytes
KEYPOINT = np.dtype([("response", "<i8"), ("x", "<f4"), ("y", "<f4"), ("m10", "<i4"), ("m01", "<i4"), ("x_level", "<u2"), ("y_level", "<u2"),
                     ("level", "<u2"), ("zero", "<u2")])
I64 = np.int64


def params(**kw) -> dict:
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def plan(width: int, height: int, p: dict) -> list:
    """chip_orb_plan: per level a dict width, height, quota, x0, y0, x1, y1, scale (an empty rectangle is 0, 0, -1, -1)"""
    nl, nf, border = p["n_levels"], p["n_features"], p["border"]
    f = 1.0 / 1.2
    g = 1.0
    for _ in range(nl):
        g *= f
    nd = float(nf) * (1.0 - f) / (1.0 - g)
    s, total, out = 1.0, 0, []
    for l in range(nl):
        if l > 0:
            s *= 1.2
        w, h = int(math.floor(width / s + 0.5)), int(math.floor(height / s + 0.5))
        if l < nl - 1:
            quota = min(int(math.floor(nd + 0.5)), nf - total)
            total += quota
            nd *= f
        else:
            quota = max(nf - total, 0)
        x0, y0, x1, y1 = border, border, w - 1 - border, h - 1 - border
        if x1 < x0 or y1 < y0:
            x0, y0, x1, y1 = 0, 0, -1, -1
        out.append(dict(width=w, height=h, quota=quota, x0=x0, y0=y0, x1=x1, y1=y1, scale=s))
    return out


# ---------------------------------------------------------------------------------------------------- pyramid
def axis(n_src: int, n_dst: int):
    """-> (i0, i1, frac) int64 arrays of n_dst entries"""
    x = np.arange(n_dst, dtype=I64)
    X = ((2 * x + 1) * n_src * 1024) // n_dst - 1024
    X = np.clip(X, 0, (n_src - 1) * 2048)
    i0 = X >> 11
    return i0, np.minimum(i0 + 1, n_src - 1), X & 2047


def downsample(img, w: int, h: int) -> np.ndarray:
    I = np.asarray(img).astype(I64)
    if w < 1 or h < 1:
        return np.zeros((max(h, 0), max(w, 0)), np.uint8)
    x0, x1, a = axis(I.shape[1], w)
    y0, y1, b = axis(I.shape[0], h)
    a, b = a[None, :], b[:, None]
    v = (I[y0][:, x0] * (2048 - a) * (2048 - b) + I[y0][:, x1] * a * (2048 - b) + I[y1][:, x0] * (2048 - a) * b + I[y1][:, x1] * a * b + (1 << 21)) >> 22
    return v.astype(np.uint8)


def downsample_loops(img, w: int, h: int) -> np.ndarray:
    I = np.asarray(img)
    hs, ws = I.shape
    out = np.zeros((max(h, 0), max(w, 0)), np.uint8)

    def ax(i, n_src, n_dst):
        X = ((2 * i + 1) * n_src * 1024) // n_dst - 1024
        X = min(max(X, 0), (n_src - 1) * 2048)
        return X >> 11, min((X >> 11) + 1, n_src - 1), X & 2047
    for y in range(h):
        y0, y1, b = ax(y, hs, h)
        for x in range(w):
            x0, x1, a = ax(x, ws, w)
            v = int(I[y0, x0]) * (2048 - a) * (2048 - b) + int(I[y0, x1]) * a * (2048 - b) + int(I[y1, x0]) * (2048 - a) * b + int(I[y1, x1]) * a * b
            out[y, x] = (v + (1 << 21)) >> 22
    return out


def pyramid(img, levels: list, loops: bool = False) -> list:
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for L in levels[1:]:
        out.append((downsample_loops if loops else downsample)(out[-1], L["width"], L["height"]))
    return out


# ---------------------------------------------------------------------------------------------------- FAST score
def score_pixel(I, x: int, y: int) -> int:
    """S at (x, y) of the 2-D integer array I; the pixel is at least 3 from every edge"""
    ip = int(I[y, x])
    d = [int(I[y + dy, x + dx]) - ip for dx, dy in RING]
    b = max(min(d[(k + j) % 16] for j in range(9)) for k in range(16))
    dd = max(min(-d[(k + j) % 16] for j in range(9)) for k in range(16))
    return max(b, dd) - 1


def score_plane_loops(img) -> np.ndarray:
    I = np.asarray(img).astype(I64)
    h, w = I.shape
    S = np.full((h, w), UNDEFINED, np.int16)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            S[y, x] = score_pixel(I, x, y)
    return S


def score_plane(img) -> np.ndarray:
    I = np.asarray(img).astype(np.int32)
    h, w = I.shape
    S = np.full((h, w), UNDEFINED, np.int16)
    if h < 7 or w < 7:
        return S
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])          # (16, h - 6, w - 6)
    d2 = np.concatenate([d, d[:8]])
    lo = np.stack([d2[k:k + 9].min(axis=0) for k in range(16)]).max(axis=0)
    hi = np.stack([(-d2[k:k + 9]).min(axis=0) for k in range(16)]).max(axis=0)
    S[3:h - 3, 3:w - 3] = np.maximum(lo, hi) - 1
    return S


# ---------------------------------------------------------------------------------------------------- candidates, Harris
def candidates(S, L: dict, threshold: int) -> np.ndarray:
    """raster indices (ascending) of the candidates of a level with score plane S"""
    if L["x1"] < L["x0"]:
        return np.zeros(0, I64)
    S = np.asarray(S).astype(np.int32)
    x0, y0, x1, y1 = L["x0"], L["y0"], L["x1"], L["y1"]
    c = S[y0:y1 + 1, x0:x1 + 1]
    ok = c >= threshold
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c > S[y0 + dy:y1 + 1 + dy, x0 + dx:x1 + 1 + dx]
    ys, xs = np.nonzero(ok)
    return (ys.astype(I64) + y0) * L["width"] + xs + x0


def candidates_loops(S, L: dict, threshold: int) -> np.ndarray:
    out = []
    for y in range(L["y0"], L["y1"] + 1):
        for x in range(L["x0"], L["x1"] + 1):
            s = int(S[y, x])
            if s >= threshold and all(s > int(S[y + dy, x + dx]) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                out.append(y * L["width"] + x)
    return np.array(out, I64)


def harris_parts(img, x: int, y: int):
    """(a, bb, c) of the 7 x 7 block centred on (x, y)"""
    I = np.asarray(img)
    a = bb = c = 0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            p = lambda j, i: int(I[y + dy + j, x + dx + i])
            ix = 2 * (p(0, 1) - p(0, -1)) + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1))
            iy = 2 * (p(1, 0) - p(-1, 0)) + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1))
            a += ix * ix; bb += iy * iy; c += ix * iy
    return a, bb, c


def harris_loops(img, x: int, y: int) -> int:
    a, bb, c = harris_parts(img, x, y)
    return 25 * (a * bb - c * c) - (a + bb) * (a + bb)


def harris(img, rasters) -> np.ndarray:
    """R (int64) at the raster indices of img"""
    I = np.asarray(img).astype(I64)
    h, w = I.shape
    rasters = np.asarray(rasters, I64)
    if not len(rasters):
        return np.zeros(0, I64)
    ix = np.zeros((h, w), I64); iy = np.zeros((h, w), I64)
    ix[1:-1, 1:-1] = 2 * (I[1:-1, 2:] - I[1:-1, :-2]) + (I[:-2, 2:] - I[:-2, :-2]) + (I[2:, 2:] - I[2:, :-2])
    iy[1:-1, 1:-1] = 2 * (I[2:, 1:-1] - I[:-2, 1:-1]) + (I[2:, :-2] - I[:-2, :-2]) + (I[2:, 2:] - I[:-2, 2:])

    def box(P):                                            # 7 x 7 sums by a summed-area table, exact in int64
        T = np.zeros((h + 1, w + 1), I64)
        T[1:, 1:] = P.cumsum(0).cumsum(1)
        ys, xs = rasters // w, rasters % w
        return T[ys + 4, xs + 4] - T[ys - 3, xs + 4] - T[ys + 4, xs - 3] + T[ys - 3, xs - 3]
    a, bb, c = box(ix * ix), box(iy * iy), box(ix * iy)
    return 25 * (a * bb - c * c) - (a + bb) * (a + bb)


def select(R, rasters, quota: int) -> np.ndarray:
    """positions (ascending) of the kept candidates: the quota largest R, ties to the lower raster index"""
    R = np.asarray(R, I64)
    if len(R) <= quota:
        return np.arange(len(R))
    order = np.lexsort((np.asarray(rasters, I64), -R))                         # primary: R descending (|R| < 2^63: the negation is exact)
    return np.sort(order[:quota])


def select_loops(R, rasters, quota: int) -> np.ndarray:
    items = sorted(range(len(R)), key=lambda i: (-int(R[i]), int(rasters[i])))
    return np.array(sorted(items[:quota]), I64)


# ---------------------------------------------------------------------------------------------------- moments
def patch_offsets():
    return [(u, v) for v in range(-15, 16) for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1)]


def moments_loops(img, x: int, y: int):
    m10 = m01 = 0
    for u, v in patch_offsets():
        i = int(img[y + v, x + u])
        m10 += u * i; m01 += v * i
    return m10, m01


_OFF = np.array(patch_offsets(), I64)


def moments(img, xs, ys):
    I = np.asarray(img).astype(I64)
    xs, ys = np.asarray(xs, I64), np.asarray(ys, I64)
    v = I[ys[:, None] + _OFF[None, :, 1], xs[:, None] + _OFF[None, :, 0]]
    return (v * _OFF[None, :, 0]).sum(1), (v * _OFF[None, :, 1]).sum(1)


# ---------------------------------------------------------------------------------------------------- the whole call
def detect(img, p: dict | None = None, loops: bool = False, stages: dict | None = None):
    """chip_orb_detect -> (records as a KEYPOINT array, level_counts[8]).  stages, if given, receives 'levels', 'images', 'scores'."""
    p = params(**(p or {}))
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    levels = plan(w, h, p)
    images = pyramid(img, levels, loops)
    scores = [(score_plane_loops if loops else score_plane)(im) for im in images]
    if stages is not None:
        stages.update(levels=levels, images=images, scores=scores)
    recs, counts = [], [0] * 8
    for l, (L, im, S) in enumerate(zip(levels, images, scores)):
        ras = (candidates_loops if loops else candidates)(S, L, p["fast_threshold"])
        if not len(ras):
            continue
        wl = L["width"]
        R = np.array([harris_loops(im, int(r % wl), int(r // wl)) for r in ras], I64) if loops else harris(im, ras)
        keep = (select_loops if loops else select)(R, ras, L["quota"])
        ras, R = ras[keep], R[keep]
        xs, ys = ras % wl, ras // wl
        if loops:
            mm = [moments_loops(im, int(x), int(y)) for x, y in zip(xs, ys)]
            m10, m01 = np.array([m[0] for m in mm], I64), np.array([m[1] for m in mm], I64)
        else:
            m10, m01 = moments(im, xs, ys)
        r = np.zeros(len(ras), KEYPOINT)
        r["response"] = R
        r["x"] = (xs.astype(np.float64) * L["scale"]).astype(np.float32)
        r["y"] = (ys.astype(np.float64) * L["scale"]).astype(np.float32)
        r["m10"], r["m01"], r["x_level"], r["y_level"], r["level"] = m10, m01, xs, ys, l
        recs.append(r)
        counts[l] = len(ras)
    return (np.concatenate(recs) if recs else np.zeros(0, KEYPOINT)), counts
