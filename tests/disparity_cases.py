"""Inputs for the tests of the disparity -> 3-D step (tests/test_disparity_mirror.py on the CPU, tests/test_disparity_gpu.py on the
device): the Q matrices, the int16 image of all 65 536 values, and the pair case set of tests/match_pairs_cases.py with every frame's
3-D image replaced by an int16 disparity."""
from __future__ import annotations

import functools

import numpy as np

import match_pairs_cases as PC
import np_mirror_disparity as D
import np_mirror_frame_store as S
import np_mirror_gms_modes as MM


def make_q(f: float, cx: float, cy: float, baseline: float, q33: float = 0.0) -> np.ndarray:
    """cv::stereoRectify's Q for a horizontal pair: [1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0 1/baseline q33]"""
    Q = np.zeros((4, 4), np.float64)
    Q[0, 0] = Q[1, 1] = 1.0
    Q[0, 3], Q[1, 3], Q[2, 3], Q[3, 2], Q[3, 3] = -cx, -cy, f, 1.0 / baseline, q33
    return Q


# EuRoC-like (752 x 480, f about 458 pixels, baseline about 11 cm); none of the five doubles is a float
Q_EUROC = make_q(458.654, 367.215803962, 248.375340610, 0.110073808127)
# principal points that differ between the rectified cameras: Q33 = (cx - cx') / Tx != 0
Q_Q33 = make_q(435.2046959714599, 371.1, 239.9, 0.0997, q33=0.31415926535)
for _Q in (Q_EUROC, Q_Q33):
    assert all(float(np.float32(_Q[r, c])) != _Q[r, c] for r, c in ((0, 3), (1, 3), (2, 3), (3, 2)))
assert Q_Q33[3, 3] != 0 and float(np.float32(Q_Q33[3, 3])) != Q_Q33[3, 3]

F = np.float32
GATE_TARGETS = (("lo_below", np.nextafter(F(0.1), F(0))), ("lo", F(0.1)), ("lo_above", np.nextafter(F(0.1), F(1))),
                ("hi_below", np.nextafter(F(25.0), F(0))), ("hi", F(25.0)), ("hi_above", np.nextafter(F(25.0), F(100))))
GATE_PASSES = dict(lo_below=False, lo=True, lo_above=True, hi_below=True, hi=True, hi_above=False)   # !(z < 0.1 || z > 25.) on the widened z


@functools.lru_cache(maxsize=None)
def gate_edge_qs() -> tuple:
    """-> ((name, Q, d, target), ...): Q_EUROC with another Q23 such that z of the int16 disparity d is EXACTLY target, for the two
    edges of the depth gate and one ulp on either side of each.  Found by search: Q23 = target / pw(d) or a float neighbour of it, for
    the first d = 1, 2, ... at which one of them multiplies back to the target."""
    out = []
    for name, target in GATE_TARGETS:
        found = None
        for d in range(1, 400):
            pw = D.pw_of(F(d), Q_EUROC)
            q23 = F(np.float64(target) / np.float64(pw))
            cands = [q23]
            for _ in range(3):
                cands = [np.nextafter(cands[0], F(0))] + cands + [np.nextafter(cands[-1], F(np.inf))]
            hit = [c for c in cands if (c * pw).view(np.uint32) == target.view(np.uint32)]
            if hit:
                Q = Q_EUROC.copy()
                Q[2, 3] = float(hit[0])
                found = (name, Q, d, target)
                break
        assert found, name
        out.append(found)
    return tuple(out)


def all_qs() -> tuple:
    """every Q of the case set, named"""
    return (("euroc", Q_EUROC), ("q33", Q_Q33)) + tuple((name, Q) for name, Q, _, _ in gate_edge_qs())


def all_int16_image() -> np.ndarray:
    """256 x 256 int16 holding every one of the 65 536 values once, shuffled so that a value's pixel says nothing about it"""
    v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    return np.random.default_rng(65536).permutation(v).reshape(256, 256)


# ------------------------------------------------------------------------------------------------ the pair set from disparities
INVALID = np.int16(-16)            # StereoBM's "no disparity": (minDisparity - 1) * 16; z < 0 under a positive Q32, dropped by the depth gate
PAIRS, NAMES, ID, N_SLOTS, SLOT_KP, SET_KEYS = PC.PAIRS, PC.NAMES, PC.ID, PC.N_SLOTS, PC.SLOT_KP, PC.SET_KEYS
Q_PAIRS = Q_EUROC
# what the numpy mirror gives per pair on the disparity frames (asserted in test_disparity_mirror.py).  Brute-force matching and GMS do
# not read depths, so the survivors are those of match_pairs_cases.EXPECTED_GMS; the three set counts are the disparity version's own.
EXPECTED_GMS = PC.EXPECTED_GMS
EXPECTED_SETS = ((1035, 1035, 1035), (181, 181, 181), (790, 794, 790), (1055, 1055, 1055), (144, 144, 144), (0, 0, 0), (1197, 1197, 1197),
                 (0, 0, 0), (0, 0, 0), (173, 173, 173), (934, 934, 934))   # (n_3d2d_ab, n_3d2d_ba, n_3d3d)


def disparity_of(xyz: np.ndarray, Q=Q_PAIRS) -> np.ndarray:
    """the int16 disparity of a 3-D image: at a stored pixel (z != 0) the nearest raw value to 16 * (Q23 / z - Q33) / Q32, elsewhere
    (and where that value is no int16) INVALID"""
    _, _, q23, q32, q33 = (float(v) for v in D.q5(Q))
    z = np.asarray(xyz, np.float32)[:, :, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        raw = np.rint(16.0 * (q23 / z - q33) / q32)
    ok = (z != 0) & np.isfinite(raw) & (raw >= -32768) & (raw <= 32767)
    return np.where(ok, raw, float(INVALID)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def frames() -> dict:
    """name -> dict(desc, kp, disp (H, W) int16): the frames of match_pairs_cases with the image replaced; built once, left unchanged"""
    return {name: dict(desc=f["desc"], kp=f["kp"], disp=disparity_of(f["xyz"])) for name, f in PC.frames().items()}


@functools.lru_cache(maxsize=None)
def image_frames() -> dict:
    """the same frames as chip_frame_put takes them: xyz = the mirror's dense image of the disparity"""
    return {name: dict(desc=f["desc"], kp=f["kp"], xyz=D.xyz_from_disparity(f["disp"], Q_PAIRS)) for name, f in frames().items()}


@functools.lru_cache(maxsize=None)
def mirror(modes: int = 0) -> tuple:
    """the numpy answer per pair of PAIRS on the disparity frames (as match_pairs_cases.mirror)"""
    f = image_frames()
    return tuple(MM.match_pair_modes(f[a], f[b], PC.kinv(), modes) for a, b in PAIRS)


def mirror_records(pair) -> dict:
    """the same answer (modes 0) from records computed at the keypoints alone"""
    f = frames()
    a, b = f[pair[0]], f[pair[1]]
    return S.match_pair(D.stored(a, a["disp"], Q_PAIRS), D.stored(b, b["disp"], Q_PAIRS), PC.kinv())
