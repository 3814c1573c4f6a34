"""Inputs of the rectification tests (tests/test_rectify_mirror.py, test_rectify_abi.py, test_rectify_gpu.py): the geometry of the
rectify_pair kernel, map builders, the quantiser's edge list, tap placements at every edge of an image, images whose weighted sum
sits exactly on a rounding half, and a two-stage case in which a pixel of the undistorted image does.  Maps are float32 (H, W)."""
import functools

import numpy as np

import np_mirror_rectify as R

# cerebro_amd/csrc/frames.hip: kRectPix pixels of a row per thread, kRectLanes * kRectPix pixels of a row and kRectRows rows per workgroup
PIXELS_PER_THREAD = 4
WG_ROW_SPAN = 256
WG_ROWS = 4
F32 = np.float32


def grid(w: int, h: int) -> tuple:
    """-> (x, y): the pixel coordinates as float64 (H, W) arrays"""
    y, x = np.mgrid[0:h, 0:w]
    return x.astype(np.float64), y.astype(np.float64)


def identity(w: int, h: int) -> tuple:
    x, y = grid(w, h)
    return x.astype(F32), y.astype(F32)


def shift(w: int, h: int, dx: float, dy: float) -> tuple:
    """R[y][x] = I[y + dy][x + dx]: whole pixels, or 1/2 and 1/64 (exact in float32 at these sizes)"""
    x, y = grid(w, h)
    return (x + dx).astype(F32), (y + dy).astype(F32)


def radtan(w: int, h: int, k1=-0.28, k2=0.07, p1=2e-4, p2=-2e-5) -> tuple:
    """an undistortion map: the pixel of a radial-tangential pinhole camera that an ideal pixel of the same intrinsics comes from"""
    fx = fy = 0.61 * w
    cx, cy = 0.49 * w, 0.52 * h
    x, y = grid(w, h)
    xn, yn = (x - cx) / fx, (y - cy) / fy
    r2 = xn * xn + yn * yn
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    return (fx * xd + cx).astype(F32), (fy * yd + cy).astype(F32)


def rotation(w: int, h: int, rx=0.01, ry=-0.015, rz=0.02) -> tuple:
    """a rectification map: the homography K R K^-1 of a small rotation"""
    f, cx, cy = 0.61 * w, 0.5 * w, 0.5 * h
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    H = K @ Rz @ Ry @ Rx @ np.linalg.inv(K)
    x, y = grid(w, h)
    d = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    return ((H[0, 0] * x + H[0, 1] * y + H[0, 2]) / d).astype(F32), ((H[1, 0] * x + H[1, 1] * y + H[1, 2]) / d).astype(F32)


def random_map(w: int, h: int, seed: int) -> tuple:
    """every pixel points anywhere inside the image and up to 3 pixels outside it"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-3, w + 3, (h, w)).astype(F32), rng.uniform(-3, h + 3, (h, w)).astype(F32)


FAMILIES = ("identity", "shift_3_-2", "shift_-5_1", "half", "sixty_fourth", "radtan", "rotation", "random")


def family(name: str, w: int, h: int) -> tuple:
    if name == "identity":
        return identity(w, h)
    if name.startswith("shift_"):
        _, dx, dy = name.split("_")
        return shift(w, h, int(dx), int(dy))
    if name == "half":
        return shift(w, h, 0.5, -0.5)
    if name == "sixty_fourth":
        return shift(w, h, 1 / 64, 1 + 1 / 64)                      # every entry an exact tie of the quantiser
    if name == "radtan":
        return radtan(w, h)
    if name == "rotation":
        return rotation(w, h)
    assert name == "random"
    return random_map(w, h, 1000 * w + h)


def image(w: int, h: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(7919 * w + h + seed).integers(0, 256, (h, w)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the quantiser
def _ulps(v) -> list:
    v = F32(v)
    return [float(np.nextafter(v, F32(-np.inf))), float(v), float(np.nextafter(v, F32(np.inf)))]


@functools.lru_cache(maxsize=None)
def quantiser_edges() -> np.ndarray:
    """float32 values: the specials, the clamps and their neighbours, exact ties k/32 + 1/64 with k even and odd, positive and negative,
    and the floats one ulp either side of every tie"""
    v = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e30, -1e30, 1e-45, -1e-45, 1e-30]
    for e in (-2.0, 32768.0, 0.0, 1.0, -1.0, 4096.0, 16384.0):
        v += _ulps(e)
    for k in (0, 1, 2, 3, 96, 97, 31, 32, 33, -1, -2, -3, -63, -64, 1023, 1024, 24063, 24064, 131070, 131071, 1048574, 1048575):
        v += _ulps(k / 32 + 1 / 64)                                   # exact in float32: at most 21 + 6 significant bits ... up to 2^15
    v += [3.015625, 3.046875, -1.984375, -1.953125]
    return np.array(v, dtype=F32)


# ------------------------------------------------------------------------------------------------ taps at the edges of the image
def tap_edges(w: int, h: int) -> tuple:
    """-> (map_x, map_y) of an image with w * h >= 104: the first pixels point at every combination of x0 in (-2, -1, w-2, w-1, w)
    and y0 likewise, each with four pairs of fractions (so that every tap has weight somewhere); the rest is the identity.  The four
    corners are the combinations (-1, -1), (w-1, -1), (-1, h-1), (w-1, h-1)."""
    assert w * h >= 104
    mx, my = identity(w, h)
    fx, fy = mx.reshape(-1), my.reshape(-1)
    i = 0
    for x0 in (-2, -1, w - 2, w - 1, w):
        for y0 in (-2, -1, h - 2, h - 1, h):
            for a, b in ((0, 0), (13, 0), (0, 29), (16, 17)):
                fx[i], fy[i] = x0 + a / 32, y0 + b / 32
                i += 1
    fx[i:i + 4] = (-2.0, -2.5, 32768.0, 40000.0)                      # the clamps: every tap outside
    return mx, my


# ------------------------------------------------------------------------------------------------ sums on a rounding half
# (I[y0][x0], I[y0][x0+1], I[y0+1][x0], I[y0+1][x0+1], a, b): the weighted sum is 512 mod 1024, the exact value k + 1/2 rounds up
HALF_BLOCKS = ((0, 1, 0, 0, 16, 0), (1, 0, 0, 0, 16, 0), (1, 1, 0, 0, 16, 16), (1, 0, 1, 0, 16, 16), (0, 0, 0, 2, 16, 16), (0, 2, 0, 0, 8, 0),
               (2, 0, 0, 0, 8, 0), (254, 255, 0, 0, 16, 0), (255, 254, 255, 254, 16, 7), (7, 8, 0, 0, 16, 0), (8, 7, 0, 0, 16, 0),
               (3, 0, 0, 0, 16, 0), (200, 100, 101, 1, 16, 16), (0, 0, 0, 128, 2, 2), (128, 0, 0, 0, 30, 30))


@functools.lru_cache(maxsize=None)
def half_case() -> tuple:
    """-> (image, map_x, map_y, n): a 2-row image of one 2 x 2 block per entry of HALF_BLOCKS with a zero column between them; pixel
    (0, i) of the map points into block i with the entry's fractions (n of them), the rest of the map is the identity"""
    n = len(HALF_BLOCKS)
    img = np.zeros((2, 3 * n), np.uint8)
    mx, my = identity(3 * n, 2)
    for i, (p00, p01, p10, p11, a, b) in enumerate(HALF_BLOCKS):
        img[0, 3 * i], img[0, 3 * i + 1], img[1, 3 * i], img[1, 3 * i + 1] = p00, p01, p10, p11
        mx[0, i], my[0, i] = 3 * i + a / 32, b / 32
    return img, mx, my, n


@functools.lru_cache(maxsize=None)
def half_u_case() -> dict:
    """two stages on a 4 x 8 image with one grey level 1 at (1, 3): stage 1 shifts by half a pixel, so U[1][2] and U[1][3] are exactly
    1/2 and round to 1; stage 2 shifts by a quarter.  R[1][3] = 3/4 U[1][3] + 1/4 U[1][4] is 3/4 -> 1 with U rounded and 3/8 -> 0 with
    U kept exact: `at` is that pixel."""
    raw = np.zeros((4, 8), np.uint8)
    raw[1, 3] = 1
    return dict(raw=raw, s1=shift(8, 4, 0.5, 0.0), s2=shift(8, 4, 0.25, 0.0), at=(1, 3), rounded=1, unrounded=0)


# ------------------------------------------------------------------------------------------------ a warped textured pair
@functools.lru_cache(maxsize=None)
def warped_pair(w: int, h: int) -> dict:
    """a textured rectified pair of stereo_bm_cases warped into a `raw` pair, and the two-stage maps that bring it back (roughly: the raw
    pair is only an input that has texture where the rectified pair has).  -> dict(left_raw, right_raw, left=(x1, y1, x2, y2), right)"""
    import stereo_bm_cases as SC
    left, right, _ = SC.tiled_pair(np.random.default_rng(1000 * w + h), w, h, tile=max(8, min(w, h) // 2), lo=4, hi=max(4, min(40, w // 4)))
    lm = radtan(w, h, k1=-0.05, k2=0.01) + rotation(w, h, 0.004, -0.006, 0.008)
    rm = radtan(w, h, k1=-0.04, k2=0.008, p1=-1e-4) + rotation(w, h, -0.005, 0.004, -0.006)
    inv = lambda m: (2 * grid(w, h)[0] - m[0], 2 * grid(w, h)[1] - m[1])   # a first-order inverse of a map near the identity
    lr = R.rectify(left, *inv(lm[2:]), *inv(lm[:2]))
    rr = R.rectify(right, *inv(rm[2:]), *inv(rm[:2]))
    return dict(left_raw=lr, right_raw=rr, left=lm, right=rm)
