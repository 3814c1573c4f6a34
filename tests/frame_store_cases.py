"""Small frames for the tests of the frame store (tests/test_frame_store_mirror.py on the CPU, tests/test_frame_store_gpu.py on the
device): a 64 x 48 image is enough wherever the case is not about the 752 x 480 scene of tests/match_batch_cases.py."""
from __future__ import annotations

import numpy as np

W, H = 64, 48
NAN = np.float32(np.nan)
# keypoints at the image border, outside and NaN (x and y alike), then pixels with the special depths below
BORDER_KP = np.array([(-0.5, 3.0), (-1.0, 3.0), (W - 0.5, 3.0), (float(W), 3.0), (np.nan, 3.0),
                      (5.0, -0.5), (5.0, -1.0), (5.0, H - 0.5), (5.0, float(H)), (5.0, np.nan)], np.float32)
BORDER_INSIDE = (True, False, True, False, False, True, False, True, False, False)
DEPTH_PIXELS = ((10, 7, np.float32(0.1)), (11, 7, np.float32(25.0)), (12, 7, NAN), (13, 7, np.float32(0.0)),
                (0, 3, np.float32(0.1)), (W - 1, 3, NAN), (5, 0, np.float32(25.0)), (5, H - 1, np.float32(0.0)))   # the last four: where BORDER_KP lands
DEPTH_KP = np.array([(x + 0.25, y + 0.75) for x, y, _ in DEPTH_PIXELS[:4]], np.float32)
SPECIAL_KP = np.concatenate([BORDER_KP, DEPTH_KP])                  # 14 keypoints


def image(rng, w: int = W, h: int = H) -> np.ndarray:
    """(h, w, 3) float32 with depths on both sides of the 0.1 / 25 gate and, on a 64 x 48 image, the special depths planted"""
    xyz = rng.uniform(-3.0, 3.0, (h, w, 3)).astype(np.float32)
    xyz[:, :, 2] = rng.choice(np.array([0.05, 0.5, 3.0, 12.0, 24.5, 30.0], np.float32), (h, w), p=[0.1, 0.2, 0.3, 0.2, 0.1, 0.1])
    if (w, h) == (W, H):
        for x, y, z in DEPTH_PIXELS:
            xyz[y, x, 2] = z
    return xyz


def frame(rng, n: int, w: int = W, h: int = H, plant_at=()) -> dict:
    """n keypoints in the middle half of the image (ten by ten GMS cells), random descriptors; SPECIAL_KP cycled over the indices plant_at"""
    kp = np.stack([rng.uniform(0.25 * w, 0.75 * w, n), rng.uniform(0.25 * h, 0.75 * h, n)], axis=1).astype(np.float32)
    for k, i in enumerate(i for i in plant_at if 0 <= i < n):
        kp[i] = SPECIAL_KP[k % len(SPECIAL_KP)]
    return dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), kp=kp, xyz=image(rng, w, h))


def view_of(rng, a: dict, n: int | None = None, jitter: float = 0.2, extra: int = 0, w: int = W, h: int = H) -> dict:
    """another frame that sees a's first n keypoints (shuffled, moved by up to jitter pixels, one descriptor bit flipped in a tenth of
    them) and `extra` unrelated ones: brute-force matching finds them again and GMS keeps their cells"""
    n = len(a["kp"]) if n is None else n
    order = rng.permutation(n)
    kp = (a["kp"][order] * np.float32(w / a["xyz"].shape[1]) + rng.uniform(-jitter, jitter, (n, 2))).astype(np.float32)
    desc = a["desc"][order].copy()
    flip = rng.random(n) < 0.1
    desc[flip, 0] ^= np.uint8(1)
    if extra:
        more = frame(rng, extra, w, h)
        kp, desc = np.concatenate([kp, more["kp"]]), np.concatenate([desc, more["desc"]])
    return dict(desc=desc, kp=kp, xyz=image(rng, w, h))


def empty_frame(w: int = 9, h: int = 7) -> dict:
    return dict(desc=np.zeros((0, 32), np.uint8), kp=np.zeros((0, 2), np.float32), xyz=np.zeros((h, w, 3), np.float32))
