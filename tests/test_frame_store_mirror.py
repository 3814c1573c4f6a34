"""CPU check behind the frame store (chip_frame_put / chip_match_batch_stored): on numpy alone, the five correspondence sets built from
the point records (tests/np_mirror_frame_store.py: the gather at put time, then the sets from (x, y, z, flag)) equal the sets
np_mirror_match builds from the 3-D images, byte for byte.  With this, a device mismatch of the stored path can be placed: in the gather
(chip_frame_read against gather) or in the set kernel."""
import numpy as np

import frame_store_cases as fc
import match_batch_cases as cases
import np_mirror_frame_store as S
import np_mirror_match as M

KINV = np.linalg.inv(np.array([[40.0, 0.0, 31.5], [0.0, 41.0, 23.5], [0.0, 0.0, 1.0]]))


def same_result(got: dict, want: dict, what):
    assert got["summary"] == want["summary"], what
    for k in cases.SET_KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, k)


def test_five_candidate_case():
    c = cases.five_candidates()
    sa = S.stored(c["a"])
    for j, (b, m) in enumerate(zip(c["cands"], c["mirror"])):
        got = S.match_pair(sa, S.stored(b), c["Kinv"])
        same_result(got, m, j)
        assert got["train_idx"].tobytes() == m["train_idx"].tobytes() and got["inlier"].tobytes() == m["inlier"].tobytes()
    assert tuple(m["summary"]["n_matches_gms"] for m in c["mirror"]) == cases.EXPECTED_GMS


def test_gather_at_the_border_outside_and_nan():
    rng = np.random.default_rng(1)
    xyz = fc.image(rng)
    rec = S.gather(fc.SPECIAL_KP, xyz)
    assert tuple(rec[:10, 3] != 0) == fc.BORDER_INSIDE                # -0.5 and w - 0.5 are inside; -1.0, exactly w and NaN are not
    assert not rec[[1, 3, 4, 6, 8, 9]].any()                          # outside: (0, 0, 0, 0)
    for i, (x, y) in ((0, (0, 3)), (2, (fc.W - 1, 3)), (5, (5, 0)), (7, (5, fc.H - 1))):
        assert rec[i, :3].tobytes() == xyz[y, x].tobytes() and rec[i, 3] == 1.0   # truncation towards zero: -0.5 -> pixel 0
    assert np.isnan(rec[2, 2]) and rec[0, 2] == np.float32(0.1) and rec[5, 2] == np.float32(25.0) and rec[7, 2] == 0.0
    for k, (x, y, z) in enumerate(fc.DEPTH_PIXELS[:4]):
        assert rec[10 + k].tobytes() == np.append(xyz[y, x], np.float32(1)).astype(np.float32).tobytes()
    assert rec[10, 2] == np.float32(0.1) and rec[11, 2] == np.float32(25.0) and np.isnan(rec[12, 2]) and rec[13, 2] == 0.0


def _every_pair():
    """every special keypoint of a matched to every special keypoint of b, all of them GMS inliers"""
    n = len(fc.SPECIAL_KP)
    ia, ib = np.divmod(np.arange(n * n), n)
    return fc.SPECIAL_KP[ia], fc.SPECIAL_KP, ib


def test_sets_at_the_border_and_at_the_depth_gate():
    rng = np.random.default_rng(2)
    xa, xb = fc.image(rng), fc.image(rng)
    kp1, kp2, t = _every_pair()
    inl = np.ones(len(kp1), np.uint8)
    inl[::7] = 0                                                     # ... but for some
    want = M.pose_sets(kp1, kp2, t, inl, xa, xb, KINV)
    got = S.pose_sets(kp1, kp2, t, inl, S.gather(kp1, xa), S.gather(kp2, xb), KINV)
    same_result(got, want, "special")
    s = want["summary"]
    assert 0 < s["n_3d3d"] < s["n_3d2d_ab"] < s["n_matches_gms"] and s["n_out_of_image"] > 0
    # the gate as the reference has it: 0.1f, 25.0f and NaN pass, 0 does not -- in the records as in the images
    one = lambda k: S.pose_sets(fc.DEPTH_KP[k:k + 1], fc.DEPTH_KP[:1], [0], [1], S.gather(fc.DEPTH_KP[k:k + 1], xa), S.gather(fc.DEPTH_KP[:1], xb), KINV)   # noqa: E731
    assert [one(k)["summary"]["n_3d2d_ab"] for k in range(4)] == [1, 1, 1, 0]
    assert np.isnan(one(2)["X_ab"][0, 2]) and one(2)["X_ab"].tobytes() == M.pose_sets(fc.DEPTH_KP[2:3], fc.DEPTH_KP[:1], [0], [1], xa, xb, KINV)["X_ab"].tobytes()


def test_the_flag_bites():
    """a match with a outside its image and b inside, and the reverse: every count that depends on the flag differs from the all-inside case"""
    rng = np.random.default_rng(3)
    xa, xb = fc.image(rng), fc.image(rng)
    xa[:, :, 2] = 3.0; xb[:, :, 2] = 3.0                              # every depth passes: only the flag can drop a point
    inside = np.array([(20.5, 20.5), (21.5, 20.5), (22.5, 20.5)], np.float32)
    t, inl = np.arange(3), np.ones(3, np.uint8)

    def counts(kp1, kp2):
        want = M.pose_sets(kp1, kp2, t, inl, xa, xb, KINV)
        got = S.pose_sets(kp1, kp2, t, inl, S.gather(kp1, xa), S.gather(kp2, xb), KINV)
        same_result(got, want, "flag")
        s = got["summary"]
        return s["n_3d2d_ab"], s["n_3d2d_ba"], s["n_3d3d"], s["n_out_of_image"]

    a_out, b_out = inside.copy(), inside.copy()
    a_out[1] = (float(fc.W), 20.5)                                    # exactly w: outside
    b_out[2] = (np.nan, 20.5)
    assert counts(inside, inside) == (3, 3, 3, 0)
    assert counts(a_out, inside) == (2, 3, 2, 1)                      # a outside, b inside: ab and 33 lose the match, ba keeps it
    assert counts(inside, b_out) == (3, 2, 2, 1)                      # the reverse
    assert counts(a_out, b_out) == (2, 2, 1, 2)
    # a zero record with the flag set is a point at the origin, not "outside": z = 0 fails the depth gate but is inside
    xa[20, 20] = 0.0
    assert counts(inside, inside) == (2, 3, 2, 0)
