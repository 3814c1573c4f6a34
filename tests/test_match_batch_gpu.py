"""GPU parity of the batched match stage (cerebro_amd/csrc/match.hip: chip_match_batch, chip_match_select, chip_match_batch_read_matches,
chip_pnp_ransac_matched_batch) through ctypes -> C ABI: one query frame against B candidates gives, per candidate, the bytes of the
numpy restatement (tests/np_mirror_match.py) AND of chip_match_pair on that pair.  One ctx for the whole module."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import match_batch_cases as cases
import np_mirror_match as M
from cerebro_amd import capi, synth

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
SET_KEYS = cases.SET_KEYS


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


@pytest.fixture(scope="module")
def five():
    return cases.five_candidates()


def same_bytes(a: np.ndarray, b: np.ndarray):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def batch_all(chip, a, cands, Kinv):
    """match_batch + everything it left, per candidate: dict(summary, the ten sets, train_idx, distance)"""
    sms = chip.match_batch(a, cands, Kinv)
    out = []
    for j, sm in enumerate(sms):
        chip.match_select(j)
        d = dict(summary=sm.as_dict())
        d.update(chip.match_read_sets(sm))
        d["train_idx"], d["distance"] = chip.match_batch_matches(j)
        out.append(d)
    return out


def assert_same_result(g: dict, want: dict, what):
    assert g["summary"] == want["summary"], what
    for k in SET_KEYS:
        if k in want:
            assert same_bytes(g[k], np.ascontiguousarray(want[k])), (what, k)


def blob(results) -> bytes:
    return b"".join(repr(r["summary"]).encode() + b"".join(r[k].tobytes() for k in SET_KEYS + ("train_idx", "distance")) for r in results)


def test_build_reports_the_stage(chip):
    assert chip.lib.chip_build_has_match_batch() == 1
    assert chip.lib.chip_abi_version() == 7
    assert capi.CHIP_MATCH_MAX_BATCH == 16


def test_five_candidates_equal_mirror_and_pair_call(chip, five):
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    got = batch_all(chip, a, cands, Kinv)
    assert tuple(g["summary"]["n_matches_gms"] for g in got) == cases.EXPECTED_GMS
    for j, (g, m) in enumerate(zip(got, five["mirror"])):
        assert_same_result(g, m, j)
        assert same_bytes(g["train_idx"], m["train_idx"]) and same_bytes(g["distance"], m["distance"]), j
    for j, b in enumerate(cands):                                   # after the batch: the pair call replaces what is selected
        p = chip.match_pair(a, b, Kinv)
        assert_same_result(got[j], p, j)
        idx, dist = chip.orb_match(a["desc"], b["desc"])
        assert same_bytes(got[j]["train_idx"], idx) and same_bytes(got[j]["distance"], dist), j


@pytest.fixture(scope="module")
def tile_case():
    """257 queries; candidates of 1 .. 4097 train descriptors with queries 0 / 128 / 254 planted at two positions in DIFFERENT tiles"""
    rng = np.random.default_rng(41)
    q = rng.integers(0, 256, (257, 32), dtype=np.uint8)
    plants = {1025: ((0, 1023, 1024),), 2049: ((0, 1023, 1024), (128, 0, 2048)), 4097: ((128, 0, 2048), (254, 1024, 4096))}
    trains, want = [], []
    for n2 in (1, 1023, 1024, 1025, 2049, 4097):
        t = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        for qi, lo, hi in plants.get(n2, ()):
            t[lo] = q[qi]; t[hi] = q[qi]
        trains.append(t)
        want.append(cases.hamming_search(q, t))
    return q, trains, want, plants


@pytest.mark.parametrize("n1", [255, 256, 257])
def test_tile_merge_keeps_the_lowest_index(chip, tile_case, n1):
    q, trains, want, plants = tile_case
    rng = np.random.default_rng(n1)
    xyz = np.zeros((48, 64, 3), np.float32)
    kp = lambda n: np.stack([rng.uniform(0, 64, n), rng.uniform(0, 48, n)], axis=1).astype(np.float32)   # noqa: E731
    a = dict(desc=q[:n1], kp=kp(n1), xyz=xyz)
    cands = [dict(desc=t, kp=kp(len(t)), xyz=xyz) for t in trains]
    sms = chip.match_batch(a, cands, synth.pinhole()[1])
    for j, t in enumerate(trains):
        idx, dist = chip.match_batch_matches(j)
        assert sms[j].n_matches_all == n1
        assert same_bytes(idx, want[j][0][:n1]) and same_bytes(dist, want[j][1][:n1]), (n1, len(t))
        for qi, lo, hi in plants.get(len(t), ()):
            assert idx[qi] == lo and dist[qi] == 0                  # the lower of the two positions, whichever tile arrived first


def test_all_duplicate_candidate_between_two_ordinary_ones(chip, five):
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    dup = dict(cands[0])
    dup["desc"] = np.repeat(a["desc"][:1], len(cands[0]["kp"]), axis=0)   # n2 = 1248: every distance of a query ties across two tiles
    got = batch_all(chip, a, [cands[1], dup, cands[2]], Kinv)
    assert (got[1]["train_idx"] == 0).all()
    assert same_bytes(got[1]["distance"], M.orb_bf_match(a["desc"], dup["desc"])[1])
    assert_same_result(got[1], M.match_pair(a, dup, Kinv), "dup")
    assert (got[1]["match_train_idx"] == 0).all()
    for g, j in ((got[0], 1), (got[2], 2)):                         # the neighbours are unaffected
        assert_same_result(g, five["mirror"][j], j)
        assert same_bytes(g["train_idx"], five["mirror"][j]["train_idx"])


def test_batch_sizes_1_2_16_and_17(chip, five):
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    pair = chip.match_pair(a, cands[1], Kinv)
    assert_same_result(pair, five["mirror"][1], "pair")             # the pair call is a run of one: the mirror is the independent witness
    one = batch_all(chip, a, [cands[1]], Kinv)
    assert_same_result(one[0], pair, "B=1")
    two = batch_all(chip, a, [cands[3], cands[1]], Kinv)
    assert_same_result(two[0], five["mirror"][3], "B=2/0")
    assert_same_result(two[1], pair, "B=2/1")
    sixteen = batch_all(chip, a, [cands[1]] * 16, Kinv)
    assert len({blob([r]) for r in sixteen}) == 1                   # sixteen identical byte strings ...
    assert_same_result(sixteen[15], pair, "B=16")                  # ... equal to the pair call
    assert blob(sixteen[:1]) == blob(one)
    with pytest.raises(capi.ChipError) as e:
        chip.match_batch(a, [cands[1]] * 17, Kinv)
    assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
    with pytest.raises(capi.ChipError) as e:                        # a failed call leaves nothing selected
        chip.match_select(0)
    assert e.value.status == capi.CHIP_ERR_BUSY


def test_frame_edge_cases(chip, five):
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    rng = np.random.default_rng(9)
    small = dict(desc=cands[0]["desc"][:400], kp=(cands[0]["kp"][:400] * np.float32(0.5)).astype(np.float32),
                 xyz=np.float32(rng.uniform(0.05, 30.0, (300, 400, 3))))                       # another image size, depths on both sides of the gate
    empty = dict(desc=np.zeros((0, 32), np.uint8), kp=np.zeros((0, 2), np.float32), xyz=np.zeros((7, 9, 3), np.float32))
    one = dict(desc=cands[0]["desc"][:1], kp=cands[0]["kp"][:1], xyz=cands[0]["xyz"])
    frames = [small, empty, cands[0], one]
    got = batch_all(chip, a, frames, Kinv)
    for j, b in enumerate(frames):
        m = M.match_pair(a, b, Kinv)
        assert got[j]["summary"] == m["summary"], j
        if m["summary"]["n_matches_all"]:
            assert_same_result(got[j], m, j)
            assert same_bytes(got[j]["train_idx"], m["train_idx"]) and same_bytes(got[j]["distance"], m["distance"]), j
    assert got[0]["summary"]["n_matches_gms"] > 0 and got[2]["summary"]["n_matches_gms"] == cases.EXPECTED_GMS[0]
    assert (got[1]["train_idx"] == -1).all() and (got[1]["distance"] == -1).all() and len(got[1]["train_idx"]) == len(a["kp"])
    assert not any(got[1]["summary"].values())
    assert (got[3]["train_idx"] == 0).all()
    # an empty query frame: every summary is zero, nothing to read
    q0 = dict(desc=empty["desc"], kp=empty["kp"], xyz=a["xyz"])
    for sm in chip.match_batch(q0, [cands[0], empty, one], Kinv):
        assert not any(sm.as_dict().values())
    chip.match_select(2)
    assert chip.match_batch_matches(2)[0].shape == (0,)
    assert chip.pnp_matched(capi.CHIP_SET_AB, 0)["status"] == capi.CHIP_ERR_TOO_FEW_POINTS


def test_state_across_batches_and_pair_calls(chip, five):
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    first = blob(batch_all(chip, a, cands, Kinv))
    sa, sc, sK = cases.small_frames(2)
    small = batch_all(chip, sa, sc, sK)
    for j in range(2):
        assert_same_result(small[j], M.match_pair(sa, sc[j], sK), j)
    p = chip.match_pair(a, cands[3], Kinv)
    assert_same_result(p, five["mirror"][3], "pair/mirror")
    chip.match_select(0)                                            # after a pair call there is one candidate
    assert_same_result(dict(summary=p["summary"], **chip.match_read_sets(capi.MatchSummary(**p["summary"]))), p, "pair")
    with pytest.raises(capi.ChipError) as e:
        chip.match_select(1)
    assert e.value.status == capi.CHIP_ERR_RANGE
    with pytest.raises(capi.ChipError) as e:                        # the keys belong to a batch
        chip.match_batch_matches(0)
    assert e.value.status == capi.CHIP_ERR_BUSY
    assert blob(batch_all(chip, a, cands, Kinv)) == first


def test_stand_alone_calls_leave_the_last_batch_alone(chip):
    """chip_orb_match has keys of its own and chip_gms_filter its own lists: what a batch left reads the same after them"""
    sa, sc, sK = cases.small_frames(2)
    before = batch_all(chip, sa, sc, sK)
    p = capi.default_ransac_params(); p.seed = 5
    pnp_before = {}
    for j in (1, 0):
        chip.match_select(j)
        pnp_before[j] = chip.pnp_matched(capi.CHIP_SET_AB, before[j]["summary"]["n_3d2d_ab"], p)
        assert pnp_before[j]["status"] == 0
    rng = np.random.default_rng(77)
    q = rng.integers(0, 256, (257, 32), dtype=np.uint8)             # one query block and one lane
    t = rng.integers(0, 256, (1025, 32), dtype=np.uint8)            # one train tile and one descriptor
    t[1024] = q[256]
    idx, dist = chip.orb_match(q, t)
    want = cases.hamming_search(q, t)
    assert same_bytes(idx, want[0]) and same_bytes(dist, want[1]) and idx[256] == 1024 and dist[256] == 0
    kp1 = rng.uniform(0, 64, (40, 2)).astype(np.float32)
    mask = chip.gms_filter(kp1, (64, 48), kp1[::-1].copy(), (64, 48), np.arange(40), np.arange(40)[::-1].copy())
    assert mask.shape == (40,)
    for j in (1, 0):                                                # without another run
        chip.match_select(j)
        sm = capi.MatchSummary(**before[j]["summary"])
        after = dict(summary=before[j]["summary"], **chip.match_read_sets(sm))
        after["train_idx"], after["distance"] = chip.match_batch_matches(j)
        assert blob([after]) == blob([before[j]]), j
        _same_estimate(chip.pnp_matched(capi.CHIP_SET_AB, sm.n_3d2d_ab, p), pnp_before[j], j)


def _same_estimate(d: dict, h: dict, what):
    assert d["status"] == h["status"] == 0, what
    assert d["summary"] == h["summary"] and d["confidence"] == h["confidence"], what
    assert same_bytes(d["T"], h["T"]) and same_bytes(d["mask"], h["mask"]), what


def test_pnp_batch_equals_single_calls_and_icp_after_select(chip, five):
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    sms = chip.match_batch(a, cands, Kinv)
    problems = []
    for j, sm in enumerate(sms):
        problems += [(j, capi.CHIP_SET_AB, sm.n_3d2d_ab), (j, capi.CHIP_SET_BA, sm.n_3d2d_ba)]
    seeds = [100 + 7 * i for i in range(len(problems))]             # P = 10: two launches
    for nh in (0, 64):
        for sampler in (capi.CHIP_SAMPLER_FRESH, capi.CHIP_SAMPLER_THEIA_PERSISTENT):
            p = capi.default_ransac_params(); p.n_hypotheses = nh; p.sampler = sampler; p.seed = 5
            chip.match_select(3)
            res = chip.pnp_matched_batch(problems, p, seeds)
            before = chip.match_read_sets(sms[3])                   # the call does not move the selection
            assert same_bytes(before["X_ab"], np.ascontiguousarray(five["mirror"][3]["X_ab"]))
            for i, (j, which, N) in enumerate(problems):
                if j == 4:                                          # the unrelated candidate: fewer than 20 points
                    assert res[i]["status"] == capi.CHIP_ERR_TOO_FEW_POINTS and res[i]["T"] is None, i
                    continue
                chip.match_select(j)
                q = capi.default_ransac_params(); q.n_hypotheses = nh; q.sampler = sampler; q.seed = seeds[i]
                _same_estimate(res[i], chip.pnp_matched(which, N, q), (nh, sampler, i))
    # seeds = NULL: every problem runs with params.seed
    p = capi.default_ransac_params(); p.seed = 11
    res = chip.pnp_matched_batch(problems[:3], p)
    for i, (j, which, N) in enumerate(problems[:3]):
        chip.match_select(j)
        _same_estimate(res[i], chip.pnp_matched(which, N, p), i)
    # the raw outputs of a problem left out of the launch: T NaN, confidence -1, summary zero with best_hypothesis -1, mask untouched
    cand = np.array([4, 0], np.int32); which = np.array([0, 0], np.int32)
    T = np.zeros((2, 16)); conf = np.zeros(2, np.float32); status = np.zeros(2, np.int32); summ = (capi.RansacSummary * 2)()
    masks = [np.full(max(sms[4].n_3d2d_ab, 1), 7, np.uint8), np.full(sms[0].n_3d2d_ab, 7, np.uint8)]
    mp = (C.c_void_p * 2)(*[m.ctypes.data for m in masks])
    assert chip.lib.chip_pnp_ransac_matched_batch(chip.h, 2, capi._ptr(cand), capi._ptr(which), C.byref(p), None, capi._ptr(T), capi._ptr(conf),
                                                  mp, summ, capi._ptr(status)) == capi.CHIP_OK
    assert list(status) == [capi.CHIP_ERR_TOO_FEW_POINTS, capi.CHIP_OK]
    assert np.isnan(T[0]).all() and conf[0] == -1.0 and (masks[0] == 7).all()
    assert (summ[0].n_iterations, summ[0].n_inliers, summ[0].best_hypothesis, summ[0].n_models, summ[0].best_cost) == (0, 0, -1, 0, 0.0)
    assert np.isfinite(T[1]).all() and set(masks[1].tolist()) <= {0, 1}
    # ICP stays one candidate at a time
    for j in (0, 2):
        chip.match_select(j)
        sets = chip.match_read_sets(sms[j])
        pi = capi.default_icp_params(); pi.seed = 3 + j
        _same_estimate(chip.icp_matched(sms[j].n_3d3d, pi), chip.icp_ransac(sets["A_3d3d"], sets["B_3d3d"], pi), j)


def test_verify_candidates_example():
    exe = LIB / "verify_candidates"
    assert exe.exists()
    r = subprocess.run([str(exe), "3000", "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== verify_candidate") == 6 and "DIFFERS" not in r.stdout
    assert r.stdout.count("three poses") == 4 and r.stdout.count("fewer than 150") == 2


def test_status_codes(chip, five):
    lib, h = chip.lib, chip.h
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    fa, keep_a = chip._match_frame(a)
    made = [chip._match_frame(b) for b in cands[:2]]
    fb = (capi.MatchFrame * 2)(*[m[0] for m in made])
    Ki = np.ascontiguousarray(Kinv).reshape(9); sm = (capi.MatchSummary * 2)()
    assert lib.chip_match_batch(None, C.byref(fa), fb, 2, capi._ptr(Ki), sm) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch(h, None, fb, 2, capi._ptr(Ki), sm) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch(h, C.byref(fa), None, 2, capi._ptr(Ki), sm) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch(h, C.byref(fa), fb, 2, None, sm) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch(h, C.byref(fa), fb, 2, capi._ptr(Ki), None) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch(h, C.byref(fa), fb, 0, capi._ptr(Ki), sm) == capi.CHIP_ERR_INVALID_ARG
    bad = (capi.MatchFrame * 2)(made[0][0], capi.MatchFrame(fa.desc, fa.kp_xy, capi.CHIP_MATCH_MAX_KEYPOINTS + 1, fa.width, fa.height, fa.xyz))
    assert lib.chip_match_batch(h, C.byref(fa), bad, 2, capi._ptr(Ki), sm) == capi.CHIP_ERR_UNSUPPORTED
    bad = (capi.MatchFrame * 2)(made[0][0], capi.MatchFrame(fa.desc, fa.kp_xy, fa.n, fa.width, fa.height, None))
    assert lib.chip_match_batch(h, C.byref(fa), bad, 2, capi._ptr(Ki), sm) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch(h, C.byref(fa), fb, 2, capi._ptr(Ki), sm) == capi.CHIP_OK
    out = np.zeros(fa.n, np.int32)
    assert lib.chip_match_select(None, 0) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_select(h, 2) == capi.CHIP_ERR_RANGE and lib.chip_match_select(h, -1) == capi.CHIP_ERR_RANGE
    assert lib.chip_match_select(h, 1) == capi.CHIP_OK
    assert lib.chip_match_batch_read_matches(h, 0, None, capi._ptr(out)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_match_batch_read_matches(h, 2, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_RANGE
    p = capi.default_ransac_params()
    T = np.zeros((2, 16)); conf = np.zeros(2, np.float32); status = np.zeros(2, np.int32)
    cand = np.array([0, 2], np.int32); which = np.array([0, 1], np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("h", h), ("P", 2), ("cand", capi._ptr(cand)), ("which", capi._ptr(which)), ("p", C.byref(p)), ("seeds", None),   # noqa: E731
                                                   ("T", capi._ptr(T)), ("conf", capi._ptr(conf)), ("mask", None), ("summ", None), ("status", capi._ptr(status)))]
    assert lib.chip_pnp_ransac_matched_batch(*args()) == capi.CHIP_ERR_RANGE          # cand[1] = 2 of a batch of 2
    cand[1] = 1
    assert lib.chip_pnp_ransac_matched_batch(*args()) == capi.CHIP_OK
    for k in ("cand", "which", "p", "T", "conf", "status"):
        assert lib.chip_pnp_ransac_matched_batch(*args(**{k: None})) == capi.CHIP_ERR_INVALID_ARG, k
    which[0] = 2
    assert lib.chip_pnp_ransac_matched_batch(*args()) == capi.CHIP_ERR_INVALID_ARG
    which[0] = 0
    with capi.Chip(4096) as fresh:                                  # nothing matched yet on this ctx
        assert fresh.lib.chip_match_select(fresh.h, 0) == capi.CHIP_ERR_BUSY
        assert fresh.lib.chip_match_batch_read_matches(fresh.h, 0, capi._ptr(out), capi._ptr(out)) == capi.CHIP_ERR_BUSY
        assert fresh.lib.chip_pnp_ransac_matched_batch(*args(h=fresh.h)) == capi.CHIP_ERR_BUSY
    with capi.Chip(4096, devices=[0, 0]) as grp:                    # not on group ctxs, as chip_match_pair
        assert grp.lib.chip_match_batch(grp.h, C.byref(fa), fb, 2, capi._ptr(Ki), sm) == capi.CHIP_ERR_UNSUPPORTED
        assert grp.lib.chip_match_select(grp.h, 0) == capi.CHIP_ERR_UNSUPPORTED
        assert grp.lib.chip_pnp_ransac_matched_batch(*args(h=grp.h)) == capi.CHIP_ERR_UNSUPPORTED


def test_resident_tick_mode_allocates_inside_a_pause(five, monkeypatch):
    """with CHIP_TICK_RESIDENT=1 the first batch of a ctx that is serving ticks allocates next to a resident scan instance: same bytes"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        for l in scenarios.default_schedule(400)[:8]:
            c.loop_tick(l)
        got = batch_all(c, a, cands, Kinv)
        c.loop_tick(400)
    for j, (g, m) in enumerate(zip(got, five["mirror"])):
        assert_same_result(g, m, j)
        assert same_bytes(g["train_idx"], m["train_idx"]) and same_bytes(g["distance"], m["distance"]), j
