"""A list of (query, candidate) pairs in which every pair has a query frame of its own, for the tests of chip_match_pairs_stored
(tests/test_match_pairs_mirror.py on the CPU, tests/test_match_pairs_gpu.py on the device), built from what the batch tests have:

  A        the five-candidate query of match_batch_cases (1280 keypoints)
  c0..c4   its candidates (1248 / 2100 / 1112 / 3471 / 292 keypoints; c4 is another place)
  S        the small query (330 keypoints), s0 / s1 its candidates (293 / 328)
  E        an empty frame

The list puts the widest query (c1, 2100) at index 2, lets four different n1 share one stride, has survivor counts on both sides of the
150 gate, a pair whose set count differs from its GMS count, an unrelated pair, a self pair, an empty frame on either side in the middle
and a candidate of four train tiles (c3)."""
from __future__ import annotations

import functools

import numpy as np

import frame_store_cases as fc
import match_batch_cases as cases
import np_mirror_frame_store as S
import np_mirror_gms_modes as MM

PAIRS = (("A", "c0"), ("S", "s0"), ("c1", "A"), ("A", "c3"), ("S", "s1"), ("S", "c0"), ("A", "A"), ("E", "c0"), ("A", "E"), ("s0", "S"), ("A", "c1"))
# what the numpy mirror gives per pair (asserted in test_match_pairs_mirror.py)
EXPECTED_N1 = (1280, 330, 2100, 1280, 330, 330, 1280, 0, 1280, 293, 1280)
EXPECTED_GMS = (1035, 181, 794, 1055, 144, 0, 1277, 0, 0, 173, 934)
EXPECTED_AB_OF_PAIR_2 = 790
NAMES = ("A", "c0", "c1", "c2", "c3", "c4", "S", "s0", "s1", "E")
ID = {name: 1000 + 7 * k for k, name in enumerate(NAMES)}           # the ids the frames are put under
N_SLOTS, SLOT_KP = 12, 3471                                          # the store of the GPU tests: the widest frame fills a slot
SET_KEYS = cases.SET_KEYS


@functools.lru_cache(maxsize=None)
def frames() -> dict:
    """name -> frame dict(desc, kp, xyz); built once per process and left unchanged"""
    five = cases.five_candidates()
    sa, sc, Kinv = cases.small_frames(2)
    assert np.array_equal(np.asarray(Kinv), np.asarray(five["Kinv"]))
    out = dict(A=five["a"], S=sa, s0=sc[0], s1=sc[1], E=fc.empty_frame())
    out.update({f"c{j}": b for j, b in enumerate(five["cands"])})
    assert sorted(out) == sorted(NAMES)
    return out


def kinv():
    return cases.five_candidates()["Kinv"]


def ids(pairs=PAIRS) -> tuple:
    """-> (a_ids, b_ids) of a pair list"""
    return [ID[a] for a, _ in pairs], [ID[b] for _, b in pairs]


@functools.lru_cache(maxsize=None)
def mirror(modes: int = 0) -> tuple:
    """the numpy answer per pair of PAIRS under the GMS modes (0: the plain filter): summary, the ten sets, train_idx, distance, inlier
    and choice; computed once per process and left unchanged"""
    f = frames()
    return tuple(MM.match_pair_modes(f[a], f[b], kinv(), modes) for a, b in PAIRS)


def mirror_records(pair) -> dict:
    """the same answer (modes 0) from the point records the store keeps in the place of the images"""
    f = frames()
    return S.match_pair(S.stored(f[pair[0]]), S.stored(f[pair[1]]), kinv())
