"""References of the ingest tests (tests/test_ingest_cases.py on the CPU, tests/test_ingest_edges_gpu.py on the device): what the narrowing
check of K3 (kernels.hip convert_rows) has to say about a wire value, and what chip_get_info().row_norm_max has to be after an append.
Plain numpy / Python; the one call into the oracle is the row's sum of squares in the device's order.

Classes of a float64 wire value on its way into float rows:
  exact      float32-representable: stored as it is, with or without CHIP_APPEND_ALLOW_ROUNDING;
  inexact    finite, and so is the nearest float32, which differs: CHIP_ERR_NOT_F32, or rounded (to nearest, ties to even) with the flag;
  overflow   finite, but the nearest float32 is +-Inf (|x| >= 0x1.ffffffp+127, the midpoint of FLT_MAX and 2^128): CHIP_ERR_NOT_F32 without the
             flag, CHIP_ERR_NONFINITE with it -- a DB never holds an Inf;
  nonfinite  NaN / +-Inf: CHIP_ERR_NONFINITE."""
import math
import struct

import numpy as np

import oracle_lib

EXACT, INEXACT, OVERFLOW, NONFINITE = "exact", "inexact", "overflow", "nonfinite"

# magnitudes as hex literals; every one is in the table with both signs
_MAGNITUDES = {
    EXACT: ["0x0.0p+0", "0x1.0p-149", "0x1.0p-126", "0x1.000002p+0", "0x1.fffffep+127",
            "0x1.99999ap-4"],                   # float(np.float32(0.1))
    INEXACT: ["0x1.999999999999ap-4",           # 0.1
              "0x1.000001p+0",                  # 1 + 2^-24: a tie, to even = 1
              "0x1.0000010000001p+0",           # just above that tie: up, to 1 + 2^-23
              "0x1.0p-150",                     # half the smallest subnormal: a tie, to even = 0
              "0x1.0000000000001p-150",         # just above it: to 2^-149
              "0x1.8p-149",                     # 1.5 * 2^-149: a tie between subnormals 1 and 2, to even = 2^-148
              "0x0.0000000000001p-1022",        # 5e-324
              "0x1.fffffe8p+127",               # FLT_MAX + 2^102: down, to FLT_MAX
              "0x1.fffffefffffffp+127"],        # the largest double that still rounds to FLT_MAX
    OVERFLOW: ["0x1.ffffffp+127",               # the midpoint of FLT_MAX and 2^128: ties-to-even gives Inf
               "0x1.0p+128",
               "0x1.78287f49c4a1dp+129",        # 1e39
               "0x1.fffffffffffffp+1023"],      # DBL_MAX
    NONFINITE: ["inf"],
}
# NaNs by their bits: a quiet NaN; a NaN with the sign bit and a payload
_NAN_BITS = [0x7FF8000000000000, 0xFFF8000000ABCDEF]


def f64_from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _table():
    out = []
    for cls, mags in _MAGNITUDES.items():
        for h in mags:
            out.append((float.fromhex(h), cls))
            out.append((float.fromhex("-" + h), cls))
    out += [(f64_from_bits(b), NONFINITE) for b in _NAN_BITS]
    return tuple(out)


TABLE = _table()        # (value, class)


def values_of(cls):
    return [x for x, c in TABLE if c == cls]


def classify(x) -> str:
    x = float(x)
    if not math.isfinite(x):
        return NONFINITE
    with np.errstate(over="ignore"):
        f = np.float64(x).astype(np.float32)
    if np.isinf(f):
        return OVERFLOW
    return EXACT if float(f) == x else INEXACT


def stored(a) -> np.ndarray:
    """what float rows hold of float64 values: round to nearest, ties to even (numpy's conversion)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def stored_bits(x) -> int:
    return int(stored([x]).view(np.uint32)[0])


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- the norm bound
def norm_bits(row_f32) -> float:
    """the fp64 sum of squares rows_norm2_max computes for one stored row: the row's dot product with itself in the order of DESIGN.md 3
    (lane l adds elements 256 j + 4 l + c, the squares exact in fp64, one rounded add each; then the xor tree 32 .. 1)"""
    row = np.ascontiguousarray(row_f32, dtype=np.float32).reshape(-1)
    return oracle_lib.dot_tree(row, row)


def norm_bits_rows(rows_f32) -> np.ndarray:
    """norm_bits of every row of a (n, D) float32 array at once, the same order written out in numpy (tests/test_ingest_cases.py holds it to
    the oracle's): elements past D add +0.0, which changes no bit of a non-negative sum"""
    rows = np.ascontiguousarray(rows_f32, dtype=np.float32)
    n, D = rows.shape
    J = (D + 255) // 256
    sq = np.zeros((n, J * 256), dtype=np.float64)
    np.multiply(rows, rows, out=sq[:, :D], dtype=np.float64)         # exact: 24 x 24 bits
    sq = sq.reshape(n, J, 64, 4)
    acc = np.zeros((n, 64), dtype=np.float64)
    for j in range(J):
        for c in range(4):
            acc = acc + sq[:, j, :, c]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ m]
    return acc[:, 0].copy()


def norm_of(ss: float) -> float:
    """what append_publish makes of a call's largest sum of squares"""
    return math.sqrt(ss) * (1 + 2.0 ** -30)


def norm_exact(row) -> float:
    """the correctly rounded L2 norm of a float32 row: exact squares, an exactly rounded sum, a correctly rounded root"""
    x = np.asarray(row, dtype=np.float32).astype(np.float64).reshape(-1)
    return math.sqrt(math.fsum((x * x).tolist()))


# The bound is one-sided, norm_exact(row) <= N; how tight N is, is derived: the chain and the tree round at most D / 256 + 6 <= 46 times
# (D <= 10240), so ss is within a factor 1 +- 46 * 2^-53 of the true sum, its root within half of that plus one rounding, and
# N = fl(fl(sqrt(ss)) * (1 + 2^-30)) <= norm_exact * (1 + 2^-29) with room to spare (2^-30 against 2^-47).
TIGHT = 1 + 2.0 ** -29


# ---------------------------------------------------------------------------------------------- data
def f32_rows(n: int, D: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """(n, D) float32 rows of Gaussian values (what goes on the float64 wire is .astype(np.float64): float32-valued)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D), dtype=np.float32) * np.float32(scale)).astype(np.float32)


def tiled(distinct: np.ndarray, n: int) -> np.ndarray:
    """n rows that repeat the distinct ones in order (a fresh, writable array)"""
    reps = -(-n // len(distinct))
    return np.ascontiguousarray(np.tile(distinct, (reps, 1))[:n])
