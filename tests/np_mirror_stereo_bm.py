"""CPU restatement in numpy integers of the block matcher (cerebro_amd/csrc/frames.hip: bm_prefilter, bm_pixel behind bm_keypoints and
bm_dense; definition in include/cerebro_hip.h, "a frame from its rectified stereo pair").  The definition is this project's own,
modelled on cv::StereoBM with PREFILTER_XSOBEL; it is NOT pinned against OpenCV.  All arithmetic is int32:

    P[y][x]  = clip((I[y-][x+1] - I[y-][x-1]) + 2 (I[y][x+1] - I[y][x-1]) + (I[y+][x+1] - I[y+][x-1]), -cap, cap) + cap, rows reflected
               (row -1 is row 1, row h is row h - 2, both row 0 when h == 1); columns 0 and w - 1: cap
    defined  : r <= y <= h - 1 - r and nd - 1 + r <= x <= w - 1 - r; every other pixel is INVALID = -16
    T        = sum |PL - cap|, SAD(d) = sum |PL[y+dy][x+dx] - PR[y+dy][x+dx-d]| over the (2r + 1)^2 window, d = 0 .. nd - 1
    m = min SAD, D = the LARGEST d with SAD(d) == m
    T < texture_threshold -> INVALID;  ratio > 0 and some |d - D| > 1 with SAD(d) <= m + m * ratio / 100 -> INVALID
    p, n     = SAD(D - 1), SAD(D + 1); at D == 0 both SAD(1), at D == nd - 1 both SAD(nd - 2)
    q        = p + n - 2 m + |p - n|
    value    = (D * 256 + (q ? trunc((p - n) * 256 / q) : 0) + 15) >> 4

Two forms: `loops` transcribes the definition pixel by pixel; `vectorised` takes per d a box sum over |PL - shifted PR|."""
from __future__ import annotations

import numpy as np

import np_mirror_disparity as D3
import np_mirror_match as M

INVALID = np.int16(-16)
DEFAULTS = dict(num_disparities=64, block_size=21, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=15)
I32 = np.int32


def params(**kw) -> dict:
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def prefilter(img, cap: int) -> np.ndarray:
    """(h, w) uint8 -> (h, w) int32 in [0, 2 cap]"""
    I = np.asarray(img).astype(I32)
    assert I.ndim == 2
    h, w = I.shape
    up = I[[1 if h > 1 else 0] + list(range(h - 1))]
    dn = I[list(range(1, h)) + [h - 2 if h > 1 else 0]]
    P = np.full((h, w), cap, I32)
    if w > 2:
        v = (up[:, 2:] - up[:, :-2]) + 2 * (I[:, 2:] - I[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
        P[:, 1:-1] = np.clip(v, -cap, cap) + cap
    return P


def defined_region(w: int, h: int, nd: int, block: int):
    """-> (y0, y1, x0, x1), inclusive; empty when y1 < y0 or x1 < x0"""
    r = block // 2
    return r, h - 1 - r, nd - 1 + r, w - 1 - r


def trunc_div(a, b):
    """a / b truncating toward zero (b > 0), elementwise"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return (np.sign(a) * (np.abs(a) // b)).astype(I32)


def value_of(Dd: int, p: int, m: int, n: int) -> int:
    """the sub-pixel step alone, python integers"""
    q = p + n - 2 * m + abs(p - n)
    num = (p - n) * 256
    frac = 0 if q == 0 else (abs(num) // q) * (1 if num >= 0 else -1)
    s = Dd * 256 + frac + 15
    assert s >= 0
    return s >> 4


def loops(left, right, prm: dict) -> np.ndarray:
    """the definition, one pixel at a time"""
    nd, block, cap = prm["num_disparities"], prm["block_size"], prm["prefilter_cap"]
    tex, ratio = prm["texture_threshold"], prm["uniqueness_ratio"]
    PL, PR = prefilter(left, cap), prefilter(right, cap)
    h, w = PL.shape
    r = block // 2
    out = np.full((h, w), INVALID, np.int16)
    y0, y1, x0, x1 = defined_region(w, h, nd, block)
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            wl = PL[y - r:y + r + 1, x - r:x + r + 1]
            T = int(np.abs(wl - cap).sum())
            sad = [int(np.abs(wl - PR[y - r:y + r + 1, x - r - d:x + r + 1 - d]).sum()) for d in range(nd)]
            m = min(sad)
            Dd = max(d for d in range(nd) if sad[d] == m)
            if T < tex:
                continue
            if ratio > 0:
                thresh = m + m * ratio // 100
                if any(sad[d] <= thresh for d in range(nd) if abs(d - Dd) > 1):
                    continue
            p = sad[1] if Dd == 0 else sad[nd - 2] if Dd == nd - 1 else sad[Dd - 1]
            n = sad[1] if Dd == 0 else sad[nd - 2] if Dd == nd - 1 else sad[Dd + 1]
            out[y, x] = value_of(Dd, p, m, n)
    return out


def _box(a: np.ndarray, block: int) -> np.ndarray:
    """sums over every block x block window of the (H, W) int array a -> (H - block + 1, W - block + 1) int64"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[block:, block:] - c[:-block, block:] - c[block:, :-block] + c[:-block, :-block]


def details(left, right, prm: dict):
    """-> None when no pixel is defined, else a dict over the defined region (rows y0 .. y1, columns x0 .. x1): sad (nd, H', W'), T, m, D,
    thresh, p, n, q, textured, unique (bool), value (int16, INVALID where filtered)"""
    nd, block, cap = prm["num_disparities"], prm["block_size"], prm["prefilter_cap"]
    tex, ratio = prm["texture_threshold"], prm["uniqueness_ratio"]
    PL, PR = prefilter(left, cap), prefilter(right, cap)
    h, w = PL.shape
    y0, y1, x0, x1 = defined_region(w, h, nd, block)
    if y1 < y0 or x1 < x0:
        return None
    r = block // 2
    Hd, Wd = y1 - y0 + 1, x1 - x0 + 1
    sad = np.empty((nd, Hd, Wd), I32)
    for d in range(nd):
        # window columns of the left image: x0 - r .. x1 + r = nd - 1 .. w - 1; of the right image: those minus d
        ad = np.abs(PL[:, nd - 1:] - PR[:, nd - 1 - d:w - d])
        sad[d] = _box(ad, block)
    T = _box(np.abs(PL[:, nd - 1:] - cap), block).astype(I32)
    m = sad.min(0)
    Dd = (nd - 1 - np.argmin(sad[::-1], 0)).astype(I32)
    thresh = m + (m.astype(np.int64) * ratio // 100).astype(I32)
    ds = np.arange(nd, dtype=I32)[:, None, None]
    unique = ~((np.abs(ds - Dd[None]) > 1) & (sad <= thresh[None])).any(0) if ratio > 0 else np.ones_like(m, bool)
    pi = np.where(Dd == 0, 1, np.where(Dd == nd - 1, nd - 2, Dd - 1))
    ni = np.where(Dd == 0, 1, np.where(Dd == nd - 1, nd - 2, Dd + 1))
    p = np.take_along_axis(sad, pi[None], 0)[0]
    n = np.take_along_axis(sad, ni[None], 0)[0]
    q = p + n - 2 * m + np.abs(p - n)
    frac = np.where(q != 0, trunc_div((p - n) * 256, np.maximum(q, 1)), 0).astype(I32)
    s = Dd * 256 + frac + 15
    assert (s >= 0).all()
    textured = T >= tex
    value = np.where(textured & unique, s >> 4, int(INVALID)).astype(np.int16)
    return dict(sad=sad, T=T, m=m, D=Dd, thresh=thresh, p=p, n=n, q=q, textured=textured, unique=unique, value=value,
                region=(y0, y1, x0, x1))


def vectorised(left, right, prm: dict) -> np.ndarray:
    h, w = np.asarray(left).shape
    out = np.full((h, w), INVALID, np.int16)
    det = details(left, right, prm)
    if det is not None:
        y0, y1, x0, x1 = det["region"]
        out[y0:y1 + 1, x0:x1 + 1] = det["value"]
    return out


def records(kp_xy, left, right, prm: dict, Q, disp=None) -> np.ndarray:
    """-> (n, 4) float32 point records: the mirror map (or disp, when it is given already) -> np_mirror_disparity's point -> record"""
    return D3.records(kp_xy, vectorised(left, right, prm) if disp is None else disp, Q)


same_floats = D3.same_floats
_pixel = M._pixel
