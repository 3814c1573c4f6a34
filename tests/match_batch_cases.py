"""One query frame against several candidate frames for the tests of chip_match_batch (tests/test_match_batch_mirror.py on the CPU,
tests/test_match_batch_gpu.py on the device), built from synth.make_match_scene.

Scenes made with the same seed, n_true, n_outlier_a and n_border draw a's keypoints and descriptors before anything that depends on the
candidate, so they share them byte for byte (asserted below).  a's 3-D image differs between scenes only in WHICH of its points are
stored (a point is stored iff it is visible in that scene's b): the query frame's 3-D image is the union, and overlapping pixels agree."""
from __future__ import annotations

import functools

import numpy as np

import np_mirror_match as M
from cerebro_amd import synth

BASE = dict(n_true=1200, n_outlier_a=80, n_border=16, seed=21)       # n1 = 1280: five query blocks of 256
CANDIDATES = (                                                       # 1 to 4 train tiles of 1024
    dict(yaw_deg=2.0, n_outlier_b=100),
    dict(yaw_deg=-4.0, t=(0.3, 0.0, 0.1), n_outlier_b=900, n_duplicates=50),
    dict(yaw_deg=6.0, t=(-0.2, 0.05, 0.2), n_outlier_b=0, flip_rate=0.1),
    dict(yaw_deg=1.0, n_outlier_b=2000, n_duplicates=300),
)
UNRELATED = dict(n_true=300, n_outlier_a=10, n_outlier_b=10, seed=99)   # another place: nothing survives GMS
# what the numpy mirror gives for (query, candidate j), checked in test_match_batch_mirror.py: both sides of the 150 / 20 gates occur
EXPECTED_N2 = (1248, 2100, 1112, 3471, 292)
EXPECTED_GMS = (1035, 934, 940, 1055, 0)

SET_KEYS = ("uv", "uv_d", "X_ab", "uvn_ab", "X_ba", "uvn_ba", "A_3d3d", "B_3d3d", "match_query_idx", "match_train_idx")


def query_and_candidates(base: dict, candidates) -> tuple:
    """-> (query frame, [candidate frames], Kinv) from make_match_scene(**base, **candidate)"""
    scenes = [synth.make_match_scene(**base, **c) for c in candidates]
    a0 = scenes[0]["a"]
    xyz = np.zeros_like(a0["xyz"])
    for sc in scenes:
        a = sc["a"]
        assert a["desc"].tobytes() == a0["desc"].tobytes() and a["kp"].tobytes() == a0["kp"].tobytes()
        has = a["xyz"][:, :, 2] != 0
        both = has & (xyz[:, :, 2] != 0)
        assert (a["xyz"][both] == xyz[both]).all()                   # overlapping pixels agree
        xyz[has] = a["xyz"][has]
    return dict(desc=a0["desc"], kp=a0["kp"], xyz=xyz), [sc["b"] for sc in scenes], scenes[0]["Kinv"]


@functools.lru_cache(maxsize=None)
def five_candidates() -> dict:
    """the five-candidate case and its mirror results, computed once per process and left unchanged"""
    a, cands, Kinv = query_and_candidates(BASE, CANDIDATES)
    cands = cands + [synth.make_match_scene(**UNRELATED)["b"]]
    return dict(a=a, cands=cands, Kinv=Kinv, mirror=[M.match_pair(a, b, Kinv) for b in cands])


def small_frames(n_cands: int = 2) -> tuple:
    """a smaller query frame (n1 = 330) with n_cands candidates: other data through the same buffers"""
    return query_and_candidates(dict(n_true=300, n_outlier_a=30, seed=33), [dict(yaw_deg=1.0 + j, n_outlier_b=40 * j) for j in range(n_cands)])


# ---------------------------------------------------------------------------------------------- the tile merge, restated
TILE = 1024
NO_MATCH = np.uint64(0xFFFFFFFFFFFFFFFF)


def tile_keys(d1: np.ndarray, d2: np.ndarray) -> np.ndarray:
    """[tiles, n1] uint64: per train tile of 1024 the partial minimum of every query as the key distance << 32 | train index"""
    out = []
    for base in range(0, len(d2), TILE):
        idx, dist = M.orb_bf_match(d1, d2[base:base + TILE])
        out.append((dist.astype(np.uint64) << np.uint64(32)) | (idx.astype(np.uint64) + np.uint64(base)))
    return np.array(out, dtype=np.uint64).reshape(len(out), len(d1))


def merge_keys(keys: np.ndarray, order) -> tuple:
    """unsigned minimum over the tiles taken in `order`, from the all-ones preset -> (train_idx, distance) int32"""
    acc = np.full(keys.shape[1], NO_MATCH, dtype=np.uint64)
    for t in order:
        acc = np.minimum(acc, keys[t])
    return (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), (acc >> np.uint64(32)).astype(np.uint32).view(np.int32)


_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def hamming_search(d1: np.ndarray, d2: np.ndarray) -> tuple:
    """plain integer Hamming search: xor, bit counts from a table, first minimum in train order"""
    idx = np.empty(len(d1), np.int32)
    dist = np.empty(len(d1), np.int32)
    for i, q in enumerate(d1):
        h = _POP[q[None, :] ^ d2].sum(axis=1, dtype=np.int32)
        idx[i] = int(np.argmin(h))
        dist[i] = h[idx[i]]
    return idx, dist
