"""GPU parity of the candidate verification front end (cerebro_amd/csrc/match.hip) through ctypes -> C ABI: chip_orb_match,
chip_gms_filter, chip_match_pair and the solvers on the device-resident sets against the numpy restatement
(tests/np_mirror_match.py), byte for byte.  One ctx for the whole module."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_mirror_match as M
from cerebro_amd import capi, synth

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"

SET_KEYS = ("uv", "uv_d", "X_ab", "uvn_ab", "X_ba", "uvn_ba", "A_3d3d", "B_3d3d", "match_query_idx", "match_train_idx")

# name -> make_match_scene arguments.  n = 5000 / 5000 is the reference's ORB budget (PointFeatureMatching.cpp:16)
SCENES = {
    "clean_2000": dict(n_true=2000, n_outlier_a=100, n_outlier_b=100, seed=11),
    "full_5000_5000": dict(n_true=4600, n_outlier_a=400, n_outlier_b=900, flip_rate=0.05, n_duplicates=60, n_border=48, seed=12),
    "n1_lt_n2": dict(n_true=700, n_outlier_a=50, n_outlier_b=1900, n_duplicates=200, seed=13),
    "n1_gt_n2": dict(n_true=1200, n_outlier_a=2100, n_outlier_b=10, flip_rate=0.1, seed=14),
    "few_survivors": dict(n_true=100, n_outlier_a=300, n_outlier_b=300, seed=15),
    "all_duplicate": dict(n_true=900, n_outlier_a=50, n_outlier_b=50, all_duplicate=True, seed=16),
    "wide_baseline": dict(n_true=3000, n_outlier_a=500, n_outlier_b=500, yaw_deg=8.0, t=(0.6, -0.1, 0.3), depth=(1.0, 24.0), flip_rate=0.08, seed=17),
}


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


@pytest.fixture(scope="module")
def scenes():
    return {k: synth.make_match_scene(**v) for k, v in SCENES.items()}


def same_bytes(a: np.ndarray, b: np.ndarray):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_build_reports_the_stage(chip):
    assert chip.lib.chip_build_has_match() == 1
    assert chip.lib.chip_abi_version() == 7


@pytest.mark.parametrize("name", list(SCENES))
def test_orb_match_equals_mirror(chip, scenes, name):
    sc = scenes[name]
    idx, dist = chip.orb_match(sc["a"]["desc"], sc["b"]["desc"])
    m_idx, m_dist = M.orb_bf_match(sc["a"]["desc"], sc["b"]["desc"])
    assert np.array_equal(idx, m_idx) and np.array_equal(dist, m_dist)
    if name == "all_duplicate":
        assert (idx == 0).all() and (dist == 0).all()             # every distance ties: the lowest train index
    if name == "full_5000_5000":
        assert len(sc["a"]["kp"]) == 5000


def test_orb_match_sizes_at_the_edges(chip):
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, (1500, 32), dtype=np.uint8)
    for n1, n2 in ((0, 10), (1, 1), (1, 1025), (257, 1024), (300, 0), (1024, 1), (1500, 1500)):
        idx, dist = chip.orb_match(d[:n1], d[::-1][:n2])
        m_idx, m_dist = M.orb_bf_match(d[:n1], d[::-1][:n2])
        assert np.array_equal(idx, m_idx) and np.array_equal(dist, m_dist), (n1, n2)
    idx, dist = chip.orb_match(d[:300], d[:0])
    assert (idx == -1).all() and (dist == -1).all()               # no train descriptors: no matches


@pytest.mark.parametrize("name", list(SCENES))
def test_gms_filter_equals_mirror(chip, scenes, name):
    sc = scenes[name]
    a, b = sc["a"], sc["b"]
    size = (a["xyz"].shape[1], a["xyz"].shape[0])
    tidx, _ = M.orb_bf_match(a["desc"], b["desc"])
    q = np.arange(len(tidx), dtype=np.int32)
    want = M.gms_filter(a["kp"], size, b["kp"], size, q, tidx)
    got = chip.gms_filter(a["kp"], size, b["kp"], size, q, tidx)
    assert same_bytes(got, want)
    # an arbitrary match list (not one per query, not in query order) takes the query_idx path
    rng = np.random.default_rng(3)
    sel = rng.permutation(len(q))[: max(1, len(q) // 2)]
    want = M.gms_filter(a["kp"], size, b["kp"], size, q[sel], tidx[sel])
    got = chip.gms_filter(a["kp"], size, b["kp"], size, q[sel], tidx[sel])
    assert same_bytes(got, want)


def test_gms_filter_random_matches_and_border_points(chip):
    """uniformly random matches do not survive; keypoints on cell borders, on the image edge and outside it go where the mirror says"""
    rng = np.random.default_rng(8)
    w, h = 752, 480
    kp1 = np.stack([rng.uniform(0, w, 4000), rng.uniform(0, h, 4000)], axis=1).astype(np.float32)
    kp2 = np.stack([rng.uniform(0, w, 4000), rng.uniform(0, h, 4000)], axis=1).astype(np.float32)
    q = np.arange(4000, dtype=np.int32)
    t = rng.permutation(4000).astype(np.int32)
    got = chip.gms_filter(kp1, (w, h), kp2, (w, h), q, t)
    assert same_bytes(got, M.gms_filter(kp1, (w, h), kp2, (w, h), q, t)) and got.sum() < 40
    # identity motion with points ON the borders: x * 20 / w integral, integral + 0.5, x = w, y = h, negative, NaN
    xs = np.array([0.0, 94.0, 188.0, 376.0, 564.0, 751.999, 752.0, -0.5, -40.0, 800.0, np.nan], np.float32)
    ys = np.array([0.0, 60.0, 120.0, 240.0, 360.0, 479.999, 480.0, -0.5, -30.0, 500.0, np.nan], np.float32)
    gx, gy = np.meshgrid(xs, ys)
    edge = np.stack([gx.ravel(), gy.ravel()], axis=1)
    kp = np.concatenate([np.repeat(edge, 8, axis=0), kp1])
    q = np.arange(len(kp), dtype=np.int32)
    got = chip.gms_filter(kp, (w, h), kp, (w, h), q, q)
    want = M.gms_filter(kp, (w, h), kp, (w, h), q, q)
    assert same_bytes(got, want)
    assert got[len(edge) * 8:].all()                              # the regular points of an identity motion all survive


def compare_pair(chip, sc):
    g = chip.match_pair(sc["a"], sc["b"], sc["Kinv"])
    m = M.match_pair(sc["a"], sc["b"], sc["Kinv"])
    assert g["summary"] == m["summary"]
    for k in SET_KEYS:
        assert same_bytes(g[k], np.ascontiguousarray(m[k])), k
    return g, m


@pytest.mark.parametrize("name", list(SCENES))
def test_match_pair_sets_equal_mirror(chip, scenes, name):
    g, m = compare_pair(chip, scenes[name])
    s = g["summary"]
    if name == "few_survivors":
        assert s["n_matches_gms"] < 150                            # the reject of Cerebro.cpp:1487 (this scene ends with 0 survivors; non-empty
                                                                   # masks of 37 / 149 / 150 / 151: test_match_edges_gpu.py, cluster_*)
    if name in ("clean_2000", "full_5000_5000"):
        assert s["n_matches_gms"] > 800 and s["n_3d3d"] > 800
    if name == "all_duplicate":
        assert (g["match_train_idx"] == 0).all()


def test_match_pair_empty_and_single(chip, scenes):
    sc = scenes["clean_2000"]
    empty = dict(desc=np.zeros((0, 32), np.uint8), kp=np.zeros((0, 2), np.float32), xyz=sc["a"]["xyz"])
    one = dict(desc=sc["a"]["desc"][:1], kp=sc["a"]["kp"][:1], xyz=sc["a"]["xyz"])
    for fa, fb in ((empty, sc["b"]), (sc["a"], empty), (empty, empty), (one, one), (one, sc["b"])):
        g = chip.match_pair(fa, fb, sc["Kinv"])
        m = M.match_pair(fa, fb, sc["Kinv"])
        assert g["summary"] == m["summary"]
        if m["summary"]["n_matches_all"]:
            for k in SET_KEYS:
                assert same_bytes(g[k], np.ascontiguousarray(m[k])), k
    r = chip.pnp_matched(capi.CHIP_SET_AB, 0)
    assert r["status"] == capi.CHIP_ERR_TOO_FEW_POINTS            # fewer than 20 correspondences (DlsPnpWithRansac.cpp:136-139)


def test_depth_gate_out_of_image_and_different_sizes(chip):
    """z exactly 0.1f / 25.0f / NaN / just outside, keypoints outside their 3-D image, two image sizes"""
    rng = np.random.default_rng(21)
    wa, ha, wb, hb = 640, 400, 752, 480
    n = 1200
    ka = np.stack([rng.uniform(2, wa - 2, n), rng.uniform(2, ha - 2, n)], axis=1).astype(np.float32)
    ka[20:50, 0] = -1.0                                                           # outside the 3-D image ((int)-1.0 = -1), yet GMS cells by the
    ka[20:50, 1] = rng.uniform(50, 55, 30).astype(np.float32)                     # reference's unchecked x + 20 y: consistent, so they survive
    kb = (ka * np.float32(1.1)).astype(np.float32)                                # a smooth motion: GMS keeps them
    ka[:6] = [[-0.5, 10.0], [10.0, -0.999], [wa, 5.0], [5.0, ha], [-1.0, 3.0], [np.nan, 3.0]]
    kb[6:10] = [[wb, 7.0], [7.0, hb + 3.0], [-1.5, 2.0], [3.0, np.inf]]
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    za = np.float32(rng.uniform(0.5, 20, (ha, wa)))
    zb = np.float32(rng.uniform(0.5, 20, (hb, wb)))
    special = np.array([0.1, np.nextafter(np.float32(0.1), np.float32(0)), 25.0, np.nextafter(np.float32(25), np.float32(30)), np.nan, 0.0, -1.0, np.inf], np.float32)
    za.ravel()[rng.choice(za.size, za.size // 3, replace=False)] = rng.choice(special, za.size // 3)
    zb.ravel()[rng.choice(zb.size, zb.size // 3, replace=False)] = rng.choice(special, zb.size // 3)
    xa = np.stack([np.float32(rng.standard_normal((ha, wa))), np.float32(rng.standard_normal((ha, wa))), za], axis=2)
    xb = np.stack([np.float32(rng.standard_normal((hb, wb))), np.float32(rng.standard_normal((hb, wb))), zb], axis=2)
    fa, fb = dict(desc=desc, kp=ka, xyz=xa), dict(desc=desc, kp=kb, xyz=xb)
    _, Kinv = synth.pinhole()
    g = chip.match_pair(fa, fb, Kinv)
    m = M.match_pair(fa, fb, Kinv)
    assert g["summary"] == m["summary"]
    for k in SET_KEYS:
        assert same_bytes(g[k], np.ascontiguousarray(m[k])), k
    s = g["summary"]
    assert s["n_matches_gms"] > 1000 and 0 < s["n_3d3d"] < s["n_3d2d_ab"] < s["n_matches_gms"] and s["n_out_of_image"] >= 30
    assert np.isnan(g["X_ab"][:, 2]).any() and (g["X_ab"][:, 2] == np.float64(np.float32(0.1))).any()   # NaN and 0.1f pass the gate


def test_solvers_on_device_sets_equal_host_pointer_calls(chip, scenes):
    for name, seed in (("clean_2000", 7), ("wide_baseline", 9), ("n1_lt_n2", 3)):
        sc = scenes[name]
        g = chip.match_pair(sc["a"], sc["b"], sc["Kinv"])
        s = g["summary"]
        for nh, sampler in ((0, capi.CHIP_SAMPLER_FRESH), (64, capi.CHIP_SAMPLER_FRESH), (0, capi.CHIP_SAMPLER_THEIA_PERSISTENT)):
            for which, X, uv, N in ((capi.CHIP_SET_AB, g["X_ab"], g["uvn_ab"], s["n_3d2d_ab"]), (capi.CHIP_SET_BA, g["X_ba"], g["uvn_ba"], s["n_3d2d_ba"])):
                p = capi.default_ransac_params(); p.seed = seed; p.n_hypotheses = nh; p.sampler = sampler
                d = chip.pnp_matched(which, N, p)
                h = chip.pnp_ransac(X, uv, p)
                assert d["summary"] == h["summary"] and d["confidence"] == h["confidence"]
                assert same_bytes(d["T"], h["T"]) and same_bytes(d["mask"], h["mask"])
            p = capi.default_icp_params(); p.seed = seed; p.n_hypotheses = nh; p.sampler = sampler
            d = chip.icp_matched(s["n_3d3d"], p)
            h = chip.icp_ransac(g["A_3d3d"], g["B_3d3d"], p)
            assert d["summary"] == h["summary"] and d["confidence"] == h["confidence"]
            assert same_bytes(d["T"], h["T"]) and same_bytes(d["mask"], h["mask"])


def test_clean_scene_recovers_the_generator_pose(chip, scenes):
    sc = scenes["clean_2000"]
    g = chip.match_pair(sc["a"], sc["b"], sc["Kinv"], read_sets=False)
    s = g["summary"]
    p = capi.default_ransac_params(); p.seed = 7
    ab = chip.pnp_matched(capi.CHIP_SET_AB, s["n_3d2d_ab"], p)
    ba = chip.pnp_matched(capi.CHIP_SET_BA, s["n_3d2d_ba"], p)
    pi = capi.default_icp_params(); pi.seed = 7
    icp = chip.icp_matched(s["n_3d3d"], pi)
    assert np.abs(ab["T"] - sc["T"]).max() < 1e-6
    assert np.abs(ba["T"] - np.linalg.inv(sc["T"])).max() < 1e-6
    assert np.abs(icp["T"] - sc["T"]).max() < 1e-6
    assert ab["summary"]["n_inliers"] == s["n_3d2d_ab"] and icp["summary"]["n_inliers"] == s["n_3d3d"]


def test_repeat_gives_identical_bytes(chip, scenes):
    sc = scenes["full_5000_5000"]
    first = chip.match_pair(sc["a"], sc["b"], sc["Kinv"])
    chip.match_pair(scenes["n1_gt_n2"]["a"], scenes["n1_gt_n2"]["b"], sc["Kinv"])   # other data through the same scratch in between
    again = chip.match_pair(sc["a"], sc["b"], sc["Kinv"])
    assert first["summary"] == again["summary"]
    for k in SET_KEYS:
        assert same_bytes(first[k], again[k]), k


def test_invalid_arguments_are_status_codes(chip, scenes):
    lib, h = chip.lib, chip.h
    sc = scenes["clean_2000"]
    d = np.zeros((4, 32), np.uint8); out = np.zeros(4, np.int32)
    assert lib.chip_orb_match(None, capi._ptr(d), 4, capi._ptr(d), 4, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_orb_match(h, None, 4, capi._ptr(d), 4, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_orb_match(h, capi._ptr(d), -1, capi._ptr(d), 4, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_orb_match(h, capi._ptr(d), 4, capi._ptr(d), capi.CHIP_MATCH_MAX_KEYPOINTS + 1, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_UNSUPPORTED
    kp = np.zeros((4, 2), np.float32); q = np.array([0, 1, 2, 4], np.int32); m = np.zeros(4, np.uint8); cnt = C.c_int32()
    assert lib.chip_gms_filter(h, capi._ptr(kp), 4, 752, 480, capi._ptr(kp), 4, 752, 480, capi._ptr(q), capi._ptr(q), 4, capi._ptr(m), C.byref(cnt)) == capi.CHIP_ERR_RANGE
    assert lib.chip_gms_filter(h, capi._ptr(kp), 4, 0, 480, capi._ptr(kp), 4, 752, 480, capi._ptr(q), capi._ptr(q), 3, capi._ptr(m), C.byref(cnt)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_gms_filter(h, capi._ptr(kp), 4, 752, 480, capi._ptr(kp), 4, 752, 480, None, capi._ptr(q), 3, capi._ptr(m), C.byref(cnt)) == capi.CHIP_ERR_INVALID_ARG
    fa, keep_a = chip._match_frame(sc["a"]); fb, keep_b = chip._match_frame(sc["b"])
    Ki = np.ascontiguousarray(sc["Kinv"]).reshape(9); sm = capi.MatchSummary()
    assert lib.chip_match_pair(h, None, C.byref(fb), capi._ptr(Ki), C.byref(sm)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_pair(h, C.byref(fa), C.byref(fb), None, C.byref(sm)) == capi.CHIP_ERR_INVALID_ARG
    bad = capi.MatchFrame(fa.desc, fa.kp_xy, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, fa.width, fa.height, fa.xyz)
    assert lib.chip_match_pair(h, C.byref(bad), C.byref(fb), capi._ptr(Ki), C.byref(sm)) == capi.CHIP_ERR_UNSUPPORTED
    bad = capi.MatchFrame(fa.desc, fa.kp_xy, fa.n, fa.width, fa.height, None)
    assert lib.chip_match_pair(h, C.byref(bad), C.byref(fb), capi._ptr(Ki), C.byref(sm)) == capi.CHIP_ERR_INVALID_ARG
    T = np.zeros(16); conf = C.c_float(); p = capi.default_ransac_params()
    assert lib.chip_pnp_ransac_matched(h, 2, C.byref(p), capi._ptr(T), C.byref(conf), None, None) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_icp_ransac_matched(h, None, capi._ptr(T), C.byref(conf), None, None) == capi.CHIP_ERR_INVALID_ARG
    with capi.Chip(4096) as fresh:                                 # nothing matched yet on this ctx
        assert fresh.lib.chip_pnp_ransac_matched(fresh.h, 0, C.byref(p), capi._ptr(T), C.byref(conf), None, None) == capi.CHIP_ERR_BUSY
        assert fresh.lib.chip_match_read_sets(fresh.h, C.byref(capi.MatchSetsOut())) == capi.CHIP_ERR_BUSY
    with capi.Chip(4096, devices=[0, 0]) as grp:                   # not on group ctxs, as chip_set_stream
        assert grp.lib.chip_match_pair(grp.h, C.byref(fa), C.byref(fb), capi._ptr(Ki), C.byref(sm)) == capi.CHIP_ERR_UNSUPPORTED
        assert grp.lib.chip_orb_match(grp.h, capi._ptr(d), 4, capi._ptr(d), 4, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_UNSUPPORTED


def test_resident_tick_mode_allocates_inside_a_pause(scenes, monkeypatch):
    """with CHIP_TICK_RESIDENT=1 the stage's first-use allocation happens next to a resident scan instance: same results"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    sc = scenes["n1_lt_n2"]
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        for l in scenarios.default_schedule(400)[:8]:
            c.loop_tick(l)
        g = c.match_pair(sc["a"], sc["b"], sc["Kinv"])
        c.loop_tick(400)
    m = M.match_pair(sc["a"], sc["b"], sc["Kinv"])
    assert g["summary"] == m["summary"]
    for k in SET_KEYS:
        assert same_bytes(g[k], np.ascontiguousarray(m[k])), k


def test_verify_candidate_example():
    exe = LIB / "verify_candidate"
    assert exe.exists()
    r = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "LoopEdge" in r.stdout and "pf_matches=" in r.stdout
    r = subprocess.run([str(exe), "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rejected" in r.stdout and "LoopEdge" not in r.stdout
