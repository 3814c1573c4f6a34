"""GPU parity of GMS with scale / rotation (cerebro_amd/csrc/match.hip: gms_grid_modes + gms_mode_select behind chip_gms_filter_modes,
chip_match_batch_modes and chip_match_batch_stored_modes) through ctypes -> C ABI: the frozen answers of the compiled reference
(tests/golden/gms_modes_ref.json) and the numpy restatement (tests/np_mirror_gms_modes.py), byte for byte."""
import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gms_cases as G
import gms_mode_cases as MC
import match_batch_cases as cases
import np_mirror_gms_modes as MM
import np_mirror_match as M
from cerebro_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "cerebro_amd" / "lib"
GOLDEN = Path(__file__).resolve().parent / "golden" / "gms_modes_ref.json"
SET_KEYS = cases.SET_KEYS


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


@pytest.fixture(scope="module")
def gold():
    return {e["name"]: e for e in json.loads(GOLDEN.read_text())["cases"]}


def same_choice(got: dict, want: dict):
    return (got["scale"], got["rotation"], got["n_inliers"]) == (want["scale"], want["rotation"], want["n_inliers"]) and \
        np.array_equal(got["counts"], want["counts"])


def device(chip, c, modes):
    return chip.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], modes=modes)


def mirror(c, modes):
    return MM.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], modes)


# ---------------------------------------------------------------------------------------------- the explicit-list entry
@pytest.mark.parametrize("name", list(MC.CASES))
def test_filter_modes_equals_the_frozen_reference(chip, gold, name):
    """every golden case (the n = 1 .. 16384 ladder among them: waves, the 1024-thread loop, the 1600-column row search) under the three
    flag pairs: mask, count and choice; modes = 0 is chip_gms_filter byte for byte"""
    e = gold[name]
    c = MC.generate(e["kind"], e["args"])
    assert G.digest(c) == e["sha256"]
    for a in e["answers"]:
        modes = MC.modes_of(a["with_scale"], a["with_rotation"])
        want = np.unpackbits(np.frombuffer(bytes.fromhex(a["mask_hex"]), np.uint8))[: e["n"]]
        mask, ch = device(chip, c, modes)
        assert mask.dtype == np.uint8 and np.array_equal(mask, want), (name, modes, np.nonzero(mask != want)[0][:5])
        assert ch["n_inliers"] == a["n_inliers"]
        assert same_choice(ch, mirror(c, modes)[1]), (name, modes, ch)
    plain = chip.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
    mask, ch = device(chip, c, 0)
    assert mask.tobytes() == plain.tobytes()
    assert (ch["scale"], ch["rotation"], ch["n_inliers"], ch["counts"][0, 0]) == (0, 1, int(plain.sum()), int(plain.sum()))
    assert (ch["counts"].reshape(-1)[1:] == -1).all()


def outside_cases():
    """inputs on which the reference leaves its tables or is not run: the restatement still answers, and the device equals it"""
    out = {"right_x_equals_width": G.generate(*G.CONSTRUCTED["right_x_equals_width"])}
    base = G.smooth(1500, 5, outlier_frac=0.1)
    for label, vals in (("nan", (np.nan, 3.0)), ("plus_1e7", (1e7, 100.0)), ("minus_1e7", (100.0, -1e7)), ("inf", (np.inf, -np.inf))):
        for side in ("kp1", "kp2"):
            c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
            c[side][7::97] = vals
            out[f"{label}_{side}"] = c
    return out


@pytest.mark.parametrize("name", list(outside_cases()))
def test_filter_modes_equals_the_restatement_outside_the_reference(chip, name):
    c = outside_cases()[name]
    for modes in (1, 2, 3):
        mask, ch = device(chip, c, modes)
        want, wch = mirror(c, modes)
        assert np.array_equal(mask, want) and same_choice(ch, wch), (name, modes)
        assert ch["n_inliers"] > 500


def test_filter_modes_status_codes(chip):
    c = MC.generate(*MC.CASES["cluster_37"])
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)
    q, t = np.ascontiguousarray(c["q"], np.int32), np.ascontiguousarray(c["t"], np.int32)
    mask, cnt, ch = np.zeros(len(q), np.uint8), capi.C.c_int32(), capi.GmsChoice()
    call = lambda modes, n: chip.lib.chip_gms_filter_modes(chip.h, p(c["kp1"]), len(c["kp1"]), 752, 480, p(c["kp2"]), len(c["kp2"]), 752, 480,
                                                           p(q), p(t), n, modes, p(mask), capi.C.byref(cnt), capi.C.byref(ch))
    assert call(4, len(q)) == capi.CHIP_ERR_INVALID_ARG
    assert call(3, 0) == capi.CHIP_OK and (ch.scale, ch.rotation, ch.n_inliers, cnt.value) == (-1, 0, 0, 0)
    assert ch.as_dict()["counts"].tolist() == [[0] * 8] * 5
    assert call(2, 0) == capi.CHIP_OK and ch.as_dict()["counts"].tolist() == [[0] * 8] + [[-1] * 8] * 4
    t[3] = len(c["kp2"])
    assert call(3, len(q)) == capi.CHIP_ERR_RANGE


# ---------------------------------------------------------------------------------------------- one query frame, B candidates
BASE = dict(cases.BASE, depth=(6.0, 6.8))                            # n1 = 1280; the depth band lets ONE candidate be 2 x closer
CANDIDATES = (
    dict(n_outlier_b=100),
    dict(n_outlier_b=100, roll_deg=90.0),
    dict(n_outlier_b=60, roll_deg=180.0),
    dict(n_outlier_b=100, roll_deg=-90.0),
    dict(n_outlier_b=900, roll_deg=45.0),
    dict(n_outlier_b=100, t=(0.0, 0.0, -3.2)),                       # 2 x closer
)
UNRELATED, EMPTY = 6, 7


@functools.lru_cache(maxsize=None)
def scene():
    a, cands, Kinv = cases.query_and_candidates(BASE, CANDIDATES)
    assert len(a["kp"]) == 1280
    cands = cands + [synth.make_match_scene(**cases.UNRELATED)["b"]]
    cands.append(dict(desc=np.zeros((0, 32), np.uint8), kp=np.zeros((0, 2), np.float32), xyz=np.zeros_like(a["xyz"])))
    return a, cands, Kinv


@functools.lru_cache(maxsize=None)
def want(j: int, modes: int):
    """matcher -> modes filter -> pose_sets of candidate j, by the restatement; computed once and left unchanged"""
    a, cands, Kinv = scene()
    return MM.match_pair_modes(a, cands[j], Kinv, modes)


PICKS = {1: [1], 2: [1, 0], 5: [0, 1, 5, UNRELATED, EMPTY], 16: [0, 1, 2, 3, 4, 5, UNRELATED, EMPTY, 1, 0, 3, 2, EMPTY, 4, 5, 1]}


def everything(chip, sms):
    out = []
    for j, sm in enumerate(sms):
        chip.match_select(j)
        d = dict(summary=sm.as_dict())
        d.update(chip.match_read_sets(sm))
        d["train_idx"], d["distance"] = chip.match_batch_matches(j)
        out.append(d)
    return out


def assert_candidate(g, ch, w, what):
    assert g["summary"] == w["summary"], what
    assert same_choice(ch, w["choice"]), (what, ch, w["choice"])
    if not w["summary"]["n_matches_all"]:
        return
    for k in SET_KEYS + ("train_idx", "distance"):
        x, y = g[k], np.ascontiguousarray(w[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def blob(results) -> bytes:
    return b"".join(repr(r["summary"]).encode() + b"".join(np.ascontiguousarray(r[k]).tobytes() for k in SET_KEYS + ("train_idx", "distance"))
                    for r in results)


@pytest.fixture(scope="module")
def stored(chip):
    """the scene's frames in the store: the query under id 100, candidate j under id j"""
    a, cands, Kinv = scene()
    chip.frame_store_reserve(10, 4096)
    chip.frame_put(100, a)
    for j, b in enumerate(cands):
        chip.frame_put(j, b)
    return chip


@pytest.mark.parametrize("B,modes", [(1, 3), (2, 3), (5, 1), (5, 2), (5, 3), (16, 3)])
def test_batch_modes_equal_the_restatement_on_host_and_stored_frames(stored, B, modes):
    chip = stored
    a, cands, Kinv = scene()
    pick = PICKS[B]
    sms, chs = chip.match_batch(a, [cands[j] for j in pick], Kinv, modes=modes)
    host = everything(chip, sms)
    for i, j in enumerate(pick):
        assert_candidate(host[i], chs[i], want(j, modes), (B, modes, i, j))
    sms2, chs2 = chip.match_batch_stored(100, pick, Kinv, modes=modes)
    st = everything(chip, sms2)
    assert blob(st) == blob(host)                                    # host frames == stored frames byte for byte
    assert all(same_choice(x, y) for x, y in zip(chs, chs2))
    if EMPTY in pick:
        e = pick.index(EMPTY)
        assert sms[e].as_dict() == dict.fromkeys(sms[e].as_dict(), 0) and (chs[e]["scale"], chs[e]["rotation"]) == (-1, 0)


def test_the_scene_needs_the_modes():
    """the 150 gate (Cerebro.cpp:1487): plain GMS rejects the rolled and the closer candidates, the modes keep them"""
    for j in (1, 2, 3, 5):
        assert want(j, 0)["summary"]["n_matches_gms"] < 150, j
        assert want(j, 3)["summary"]["n_matches_gms"] >= 150, j
    for j in (1, 2, 3):
        assert want(j, 2)["summary"]["n_matches_gms"] >= 150, j
    assert want(5, 1)["summary"]["n_matches_gms"] >= 150
    assert want(UNRELATED, 3)["summary"]["n_matches_gms"] < 150
    assert [want(j, 2)["choice"]["rotation"] for j in (0, 1, 2, 3, 4)] == [1, 7, 5, 3, 8]


def test_modes_zero_is_the_plain_batch(stored):
    chip = stored
    a, cands, Kinv = scene()
    pick = PICKS[5]
    plain = everything(chip, chip.match_batch(a, [cands[j] for j in pick], Kinv))
    sms, chs = chip.match_batch(a, [cands[j] for j in pick], Kinv, modes=0)
    assert blob(everything(chip, sms)) == blob(plain)
    sms2, chs2 = chip.match_batch_stored(100, pick, Kinv, modes=0)
    assert blob(everything(chip, sms2)) == blob(plain)
    for i, j in enumerate(pick):
        assert same_choice(chs[i], want(j, 0)["choice"]) and same_choice(chs2[i], chs[i]), (i, j)


def test_a_rolled_candidate_between_two_ordinary_ones(stored):
    chip = stored
    a, cands, Kinv = scene()
    sms, chs = chip.match_batch_stored(100, [0, 1, 0], Kinv, modes=3)
    assert (chs[0]["scale"], chs[0]["rotation"]) == (chs[2]["scale"], chs[2]["rotation"]) != (chs[1]["scale"], chs[1]["rotation"])
    assert chs[0]["rotation"] == 1 and chs[1]["rotation"] == 7
    assert all(sm.n_matches_gms >= 150 for sm in sms)


def _same_estimate(d, h, what):
    assert d["status"] == h["status"], what
    if d["status"] != capi.CHIP_OK:
        return
    assert d["T"].tobytes() == h["T"].tobytes() and d["confidence"] == h["confidence"] and d["summary"] == h["summary"], what
    assert d["mask"].tobytes() == h["mask"].tobytes(), what


def test_state_and_solvers_across_modes_and_plain_calls(stored):
    """a modes batch, a plain pair call, a modes batch again: the second batch is the first, and the batched PnP / ICP on it are
    bit-identical to the single calls on the selected candidate"""
    chip = stored
    a, cands, Kinv = scene()
    pick = [1, 0, 5]
    first = everything(chip, chip.match_batch_stored(100, pick, Kinv, modes=3)[0])
    pair = chip.match_pair(a, cands[0], Kinv)
    assert pair["summary"] == want(0, 0)["summary"]
    sms, chs = chip.match_batch_stored(100, pick, Kinv, modes=3)
    assert blob(everything(chip, sms)) == blob(first)
    pp = capi.default_ransac_params(); pp.seed = 7
    pi = capi.default_icp_params(); pi.seed = 7
    problems = [(i, w, sms[i].n_3d2d_ab if w == capi.CHIP_SET_AB else sms[i].n_3d2d_ba) for i in range(3) for w in (capi.CHIP_SET_AB, capi.CHIP_SET_BA)]
    pnp_b = chip.pnp_matched_batch(problems, pp)
    icp_b = chip.icp_matched_batch([(i, sms[i].n_3d3d) for i in range(3)], pi)
    for k, (i, w, n) in enumerate(problems):
        chip.match_select(i)
        _same_estimate(pnp_b[k], chip.pnp_matched(w, n, pp), ("pnp", i, w))
    for i in range(3):
        chip.match_select(i)
        _same_estimate(icp_b[i], chip.icp_matched(sms[i].n_3d3d, pi), ("icp", i))
    assert pnp_b[0]["status"] == capi.CHIP_OK                        # the rolled candidate reaches PnP


def test_first_use_under_a_resident_scan_allocates_inside_a_pause(monkeypatch):
    """with CHIP_TICK_RESIDENT=1 the tables, planes and choice records of the first modes call are allocated next to a resident scan
    instance: same bytes, and the ticks go on"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    a, cands, Kinv = scene()
    pick = [0, 1, EMPTY]
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        for l in scenarios.default_schedule(400)[:8]:
            c.loop_tick(l)
        c.frame_store_reserve(4, 4096)
        c.frame_put(100, a)
        for j in pick:
            c.frame_put(j, cands[j])
        sms, chs = c.match_batch_stored(100, pick, Kinv, modes=3)
        got = everything(c, sms)
        mask, ch = device(c, MC.generate(*MC.CASES["rotate_90"]), 3)
        c.loop_tick(400)
    for i, j in enumerate(pick):
        assert_candidate(got[i], chs[i], want(j, 3), (i, j))
    assert ch["rotation"] == 7 and ch["n_inliers"] > 2000


def test_verify_candidates_modes_example():
    exe = LIB / "verify_candidates_modes"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    rolled = {}
    for l in lines:
        m = re.match(r"gms_modes=(\d) candidate 1 .*pf_matches=(\d+) choice=\(scale (-?\d+), rotation (\d+)\) accepted=(\d)", l)
        if m:
            rolled[int(m.group(1))] = (int(m.group(2)), int(m.group(4)), int(m.group(5)))
    assert rolled[0][0] < 150 and rolled[0][2] == 0                  # rejected at the gate with the plain form
    assert rolled[3][0] >= 150 and rolled[3][1] == 7 and rolled[3][2] == 1
    err = float(re.search(r"deviates from the scene's pose by at most (\S+)", r.stdout).group(1))
    assert 0 <= err < 1e-6, r.stdout                                 # the tolerance of test_clean_scene_recovers_the_generator_pose
