"""numpy restatement of the rectification's definition (include/cerebro_hip.h, "a frame from its raw stereo pair"): the quantiser of a
float map value to 1/32 pixel, the four-tap sample with a zero border and a round-half-up, one remap, and the rectification of an
image through one or two stages.  All integer behind the quantiser.  tests/test_rectify_mirror.py holds it to exact rational
arithmetic; the library (chip_rectify_quantize) and the device (chip_remap, chip_rectify_pair) are held to it bit for bit."""
import numpy as np

FRACTION_BITS = 5
ONE = 1 << FRACTION_BITS                 # 32: a pixel
MAP_MIN, MAP_MAX, NAN_Q = -2.0, 32768.0, -64


def quantize(m) -> np.ndarray:
    """Q: float map values -> int32 in 1/32 pixel.  NaN -> -64; otherwise rint(32 * clamp(m, -2, 32768)) in float32, ties to even"""
    m = np.asarray(m, dtype=np.float32)
    nan = np.isnan(m)
    c = np.minimum(np.maximum(np.where(nan, np.float32(0), m), np.float32(MAP_MIN)), np.float32(MAP_MAX))
    p = (np.float32(ONE) * c).astype(np.float32)                     # exact: a power of two, no overflow
    return np.where(nan, NAN_Q, np.rint(p).astype(np.int64)).astype(np.int32)


def taps(image, x, y) -> np.ndarray:
    """image[y][x] as int64, 0 outside the image; x and y integer arrays of one shape"""
    img = np.asarray(image)
    h, w = img.shape
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    v = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
    return np.where(inside, v, 0)


def weighted_sum(image, qx, qy) -> np.ndarray:
    """the sum S rounds: four taps times their weights, in 1/1024 of a grey level (without the + 512)"""
    qx, qy = np.asarray(qx, dtype=np.int64), np.asarray(qy, dtype=np.int64)
    x0, a, y0, b = qx >> FRACTION_BITS, qx & (ONE - 1), qy >> FRACTION_BITS, qy & (ONE - 1)
    return (taps(image, x0, y0) * (ONE - a) * (ONE - b) + taps(image, x0 + 1, y0) * a * (ONE - b)
            + taps(image, x0, y0 + 1) * (ONE - a) * b + taps(image, x0 + 1, y0 + 1) * a * b)


def sample(image, qx, qy) -> np.ndarray:
    """S(I, qx, qy): (weighted sum + 512) >> 10, a uint8 array of qx's shape"""
    return ((weighted_sum(image, qx, qy) + 512) >> 10).astype(np.uint8)


def remap(image, map_x, map_y) -> np.ndarray:
    """one stage: R[y][x] = S(image, Q(map_x[y][x]), Q(map_y[y][x]))"""
    return sample(image, quantize(map_x), quantize(map_y))


def rectify(raw, x1, y1, x2=None, y2=None) -> np.ndarray:
    """one stage (x2, y2 None) or two: U = remap(raw, x1, y1) as a uint8 image, R = remap(U, x2, y2)"""
    assert (x2 is None) == (y2 is None)
    u = remap(raw, x1, y1)
    return u if x2 is None else remap(u, x2, y2)
