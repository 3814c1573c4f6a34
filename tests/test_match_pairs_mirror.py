"""CPU check of the pair-list case set (tests/match_pairs_cases.py) from the numpy mirror alone: the properties the GPU tests of
chip_match_pairs_stored rely on are properties of the generated data, so a later edit of the generators cannot quietly flatten the
case; and the sets built from the store's point records equal the ones built from the 3-D images for every pair."""
import numpy as np

import match_pairs_cases as PC


def test_the_frames_have_the_documented_sizes():
    f = PC.frames()
    assert [len(f[k]["kp"]) for k in PC.NAMES] == [1280, 1248, 2100, 1112, 3471, 292, 330, 293, 328, 0]
    assert max(len(v["kp"]) for v in f.values()) == PC.SLOT_KP and len(PC.NAMES) <= PC.N_SLOTS
    assert len(set(PC.ID.values())) == len(PC.NAMES)


def test_the_pair_list_has_its_properties():
    f, m = PC.frames(), PC.mirror(0)
    n1 = tuple(len(f[a]["kp"]) for a, _ in PC.PAIRS)
    gms = tuple(r["summary"]["n_matches_gms"] for r in m)
    assert len(PC.PAIRS) == 11 and n1 == PC.EXPECTED_N1 and gms == PC.EXPECTED_GMS
    # the widest query is not the first pair's, and four different non-zero n1 share the stride
    assert n1.index(max(n1)) == 2 and max(n1) == 2100 and len({n for n in n1 if n}) == 4
    # both sides of the "< 150 matches" gate among the related pairs
    assert any(0 < g < 150 for g in gms) and sum(g >= 150 for g in gms) >= 7
    # a pair whose set count differs from its GMS count
    assert m[2]["summary"]["n_3d2d_ab"] == PC.EXPECTED_AB_OF_PAIR_2 != gms[2]
    # an unrelated pair, a self pair, an empty frame on either side -- none of them first or last
    assert PC.PAIRS[5] == ("S", "c0") and gms[5] == 0 and m[5]["summary"]["n_matches_all"] == 330
    assert PC.PAIRS[6] == ("A", "A") and gms[6] == 1277 and np.array_equal(m[6]["train_idx"], np.arange(1280)) and not m[6]["distance"].any()
    assert PC.PAIRS[7][0] == "E" and PC.PAIRS[8][1] == "E"
    for j in (7, 8):
        assert not any(m[j]["summary"].values()) and m[j]["choice"]["scale"] == -1 and m[j]["choice"]["rotation"] == 0
    # a candidate of four train tiles of 1024, and query frames of more than one block of 256 next to ones of two
    assert len(f["c3"]["kp"]) > 3 * 1024 and PC.PAIRS[3] == ("A", "c3")
    # the same query frame with different candidates, the same candidate with different query frames, a pair and its swap
    assert sum(a == "A" for a, _ in PC.PAIRS) == 5 and sum(b == "c0" for _, b in PC.PAIRS) == 3
    assert ("A", "c1") in PC.PAIRS and ("c1", "A") in PC.PAIRS and ("S", "s0") in PC.PAIRS and ("s0", "S") in PC.PAIRS


def test_the_modes_change_some_pairs_and_not_others():
    m0, m2, m3 = PC.mirror(0), PC.mirror(2), PC.mirror(3)
    g = lambda m: [r["summary"]["n_matches_gms"] for r in m]
    assert g(m3) != g(m0) and [r["choice"]["scale"] for r in m3].count(2) >= 2      # another scale wins for some pairs
    assert g(m2) == g(m0)                                                            # rotation alone keeps the plain winner here
    for r0, r3 in zip(m0, m3):                                                       # the matcher does not depend on the modes
        assert r0["train_idx"].tobytes() == r3["train_idx"].tobytes() and r0["distance"].tobytes() == r3["distance"].tobytes()


def test_record_based_sets_equal_the_image_based_ones_for_every_pair():
    for pair, img in zip(PC.PAIRS, PC.mirror(0)):
        rec = PC.mirror_records(pair)
        assert rec["summary"] == img["summary"], pair
        for k in PC.SET_KEYS + ("train_idx", "distance", "inlier"):
            if k in img or k in rec:
                a, b = np.ascontiguousarray(rec[k]), np.ascontiguousarray(img[k])
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (pair, k)
