"""CPU checks behind the batched match stage (chip_match_batch): the merge rule of hamming_match_split restated in numpy -- partial minima
per train tile as the key distance << 32 | train index, unsigned minimum in ANY order -- equals the brute-force matcher's definition
(np_mirror_match.orb_bf_match: minimum distance, ties -> the lowest train index), and the five-candidate case of
tests/match_batch_cases.py is the one the GPU test believes it is."""
import numpy as np

import match_batch_cases as cases
import np_mirror_match as M


def _orders(n_tiles: int, rng, k: int = 6):
    return [list(range(n_tiles)), list(range(n_tiles))[::-1]] + [list(rng.permutation(n_tiles)) for _ in range(k)]


def test_key_minimum_over_tiles_in_any_order_equals_the_matcher():
    rng = np.random.default_rng(2)
    d2 = rng.integers(0, 256, (16384, 32), dtype=np.uint8)            # 16 tiles, the largest train set the library takes
    d1 = rng.integers(0, 256, (96, 32), dtype=np.uint8)
    # equal minima planted in different tiles: the query's own descriptor at two (three) train positions
    for q, pos in ((0, (1023, 1024)), (1, (0, 2048)), (2, (1024 + 1, 4096)), (3, (16383, 5000, 9000)), (4, (2047, 2049))):
        d2[list(pos)] = d1[q]
    d1[5] = d2[16383 - 1]
    d2[16383] = d2[16383 - 1]                                        # ... and 16382 / 16383 inside the last tile
    d1[6] = d2[16383]; d1[6, 0] ^= np.uint8(1)                        # distance 1 to the pair above, nothing closer
    d2[700] = d1[7]; d2[701] = d1[7]                                  # a tie inside one tile
    keys = cases.tile_keys(d1, d2)
    assert keys.shape == (16, 96)
    want = M.orb_bf_match(d1, d2)
    assert list(want[0][:6]) == [1023, 0, 1025, 5000, 2047, 16382] and (want[1][:6] == 0).all() and want[0][7] == 700
    assert want[0][6] == 16382 and want[1][6] == 1
    for order in _orders(16, rng):
        idx, dist = cases.merge_keys(keys, order)
        assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1]), order


def test_key_extremes():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    # distance 256 everywhere (every train descriptor is the complement): the largest distance, all tiles tie -> index 0
    d2 = np.repeat((~q[:1]), 2049, axis=0)
    keys = cases.tile_keys(q[:1], d2)
    for order in _orders(3, rng, 2):
        idx, dist = cases.merge_keys(keys, order)
        assert idx[0] == 0 and dist[0] == 256
    # the only exact match at the last index the library takes
    d2 = rng.integers(0, 256, (16384, 32), dtype=np.uint8)
    d2[16383] = q[1]
    keys = cases.tile_keys(q, d2)
    want = M.orb_bf_match(q, d2)
    for order in _orders(16, rng, 2):
        idx, dist = cases.merge_keys(keys, order)
        assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1]) and idx[1] == 16383 and dist[1] == 0
    # no tile at all: the preset decodes to the n2 == 0 convention
    idx, dist = cases.merge_keys(np.zeros((0, 3), np.uint64), [])
    assert (idx == -1).all() and (dist == -1).all()
    # ... and the plain integer search used by the GPU test agrees with the mirror
    a, b = cases.hamming_search(q, d2[:3000]), M.orb_bf_match(q, d2[:3000])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_five_candidate_case_spans_the_gates():
    c = cases.five_candidates()
    assert len(c["a"]["kp"]) == 1280
    assert tuple(len(b["kp"]) for b in c["cands"]) == cases.EXPECTED_N2          # 2, 3, 2, 4 and 1 train tiles
    s = [m["summary"] for m in c["mirror"]]
    assert tuple(x["n_matches_gms"] for x in s) == cases.EXPECTED_GMS
    assert s[2]["n_3d2d_ab"] == 939                                              # a GMS inlier without depth in a
    assert all(x["n_matches_gms"] >= 150 and x["n_3d2d_ab"] >= 20 and x["n_3d2d_ba"] >= 20 and x["n_3d3d"] >= 20 for x in s[:4])
    assert s[4]["n_matches_gms"] < 150 and s[4]["n_3d2d_ab"] < 20 and s[4]["n_3d2d_ba"] < 20   # the reject and the too-few-points side
    # the brute-force matches of every candidate equal the tile merge in reverse order too
    for b, m in zip(c["cands"], c["mirror"]):
        keys = cases.tile_keys(c["a"]["desc"], b["desc"])
        idx, dist = cases.merge_keys(keys, range(len(keys))[::-1])
        assert np.array_equal(idx, m["train_idx"]) and np.array_equal(dist, m["distance"])
