"""GPU parity of the frame store (cerebro_amd/csrc/frames.hip: chip_frame_store_reserve, chip_frame_put / _drop / _read; match.hip:
chip_match_batch_stored) through ctypes -> C ABI.  Frames are put once under an id; a match on stored frames gives, per candidate, the
bytes of chip_match_batch on the host frames that were put AND of the numpy restatement; chip_frame_read gives the numpy gather.
Small images (64 x 48) wherever the case is not about the 752 x 480 scene."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frame_store_cases as fc
import match_batch_cases as cases
import np_mirror_frame_store as S
import np_mirror_match as M
from cerebro_amd import capi, synth

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
SET_KEYS = cases.SET_KEYS
KINV = synth.pinhole()[1]
N_SLOTS, SLOT_KP = 8, 4096


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        c.frame_store_reserve(N_SLOTS, SLOT_KP)
        yield c


@pytest.fixture
def clean(chip):
    """the module's ctx with an empty store"""
    yield chip
    for i in list(range(-4, 64)) + [100, 2 ** 40]:               # every id the tests use
        if chip.lib.chip_frame_drop(chip.h, i) not in (capi.CHIP_OK, capi.CHIP_ERR_RANGE):
            raise AssertionError("chip_frame_drop")
    assert chip.frame_store_info() == dict(n_slots=N_SLOTS, slot_keypoints=SLOT_KP, n_frames=0)


@pytest.fixture(scope="module")
def five():
    return cases.five_candidates()


def same_bytes(a: np.ndarray, b: np.ndarray):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def everything(chip, sms):
    """what a batch left, per candidate: dict(summary, the ten sets, train_idx, distance)"""
    out = []
    for j, sm in enumerate(sms):
        chip.match_select(j)
        d = dict(summary=sm.as_dict())
        d.update(chip.match_read_sets(sm))
        d["train_idx"], d["distance"] = chip.match_batch_matches(j)
        out.append(d)
    return out


def host_all(chip, a, cands, Kinv):
    return everything(chip, chip.match_batch(a, cands, Kinv))


def stored_all(chip, a_id, b_ids, Kinv):
    return everything(chip, chip.match_batch_stored(a_id, b_ids, Kinv))


def blob(results) -> bytes:
    return b"".join(repr(r["summary"]).encode() + b"".join(np.ascontiguousarray(r[k]).tobytes() for k in SET_KEYS + ("train_idx", "distance")) for r in results)


def assert_same_result(g: dict, want: dict, what):
    assert g["summary"] == want["summary"], what
    if not want["summary"]["n_matches_all"]:
        return
    for k in SET_KEYS + ("train_idx", "distance"):
        assert same_bytes(g[k], np.ascontiguousarray(want[k])), (what, k)


def status_of(call, *args):
    with pytest.raises(capi.ChipError) as e:
        call(*args)
    return e.value.status


def test_build_reports_the_store(chip):
    assert chip.lib.chip_build_has_frame_store() == 1 and chip.lib.chip_abi_version() == 7
    assert chip.frame_store_info() == dict(n_slots=N_SLOTS, slot_keypoints=SLOT_KP, n_frames=0)


def test_five_candidates_equal_mirror_and_host_frames(clean, five):
    chip, a, cands, Kinv = clean, five["a"], five["cands"], five["Kinv"]
    chip.frame_put(100, a)
    for j, b in enumerate(cands):
        chip.frame_put(j, b)
    assert chip.frame_store_info()["n_frames"] == 6
    got = stored_all(chip, 100, list(range(5)), Kinv)
    assert tuple(g["summary"]["n_matches_gms"] for g in got) == cases.EXPECTED_GMS    # both sides of the 150 gate
    assert not any(got[4]["summary"][k] for k in ("n_matches_gms", "n_3d2d_ab", "n_3d2d_ba", "n_3d3d"))   # the unrelated candidate
    for j, (g, m) in enumerate(zip(got, five["mirror"])):
        assert_same_result(g, m, j)
    host = host_all(chip, a, cands, Kinv)
    assert blob(got) == blob(host)
    r = chip.frame_read(100)                                         # the 752 x 480 scene through the gather
    assert (r["n"], r["width"], r["height"]) == (len(a["kp"]), a["xyz"].shape[1], a["xyz"].shape[0])
    assert same_bytes(r["desc"], a["desc"]) and same_bytes(r["kp"], a["kp"]) and same_bytes(r["pts"], S.gather(a["kp"], a["xyz"]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_record_equals_the_numpy_gather(clean, n):
    rng = np.random.default_rng(n)
    edges = [0, 1, 62, 63, 64, 65, 126, 127, 128, 254, 255, 256, 257, 511, 512, 1022, 1023, 1024, n - 2, n - 1]   # first / last of a wave, of a workgroup
    f = fc.frame(rng, n, plant_at=edges + list(range(300, 300 + len(fc.SPECIAL_KP))))   # ... and every special keypoint once n > 314
    clean.frame_put(3, f)
    r = clean.frame_read(3)
    want = S.gather(f["kp"], f["xyz"])
    assert (r["n"], r["width"], r["height"]) == (n, fc.W, fc.H)
    assert same_bytes(r["desc"], f["desc"]) and same_bytes(r["kp"], f["kp"])
    assert same_bytes(r["pts"], want)
    if n >= 255:
        assert (want[:, 3] == 0).any() and np.isnan(want[:, 2]).any() and (want[:, 2] == np.float32(0.1)).any()


@pytest.mark.parametrize("n1", [1023, 1024, 1025])
@pytest.mark.parametrize("keep", ["all", "last_wave_empty"])
def test_compaction_at_the_chunk_edge(clean, n1, keep):
    """pose_sets_body walks one (n1 <= 1024) or two chunks of 1024 matches; a query keypoint outside its image has no GMS cell, so its
    match is no inlier: that empties the last wave of the first chunk"""
    rng = np.random.default_rng(1000 + n1)
    a = fc.frame(rng, n1)
    b0 = fc.view_of(rng, a, jitter=0.0)                              # the same cells on both sides: GMS keeps every match
    b1 = fc.view_of(rng, a, n=700, extra=45)
    if keep == "last_wave_empty":
        a["kp"][960:1024] = (float(fc.W) + 3.0, 5.0)
    chip = clean
    chip.frame_put(1, a); chip.frame_put(2, b0); chip.frame_put(3, b1)
    got = stored_all(chip, 1, [2, 3], KINV)
    m0 = M.match_pair(a, b0, KINV)
    if keep == "all":
        assert m0["inlier"].all() and m0["summary"]["n_matches_gms"] == n1
    else:
        assert not m0["inlier"][960:1024].any() and m0["inlier"][:960].all() and m0["inlier"][1024:].all()
    assert 0 < m0["summary"]["n_3d3d"] < m0["summary"]["n_3d2d_ab"] < n1
    assert_same_result(got[0], m0, "mirror")
    assert_same_result(got[1], M.match_pair(a, b1, KINV), "mirror 1")
    assert blob(got) == blob(host_all(chip, a, [b0, b1], KINV))


def test_ids_repeat_replace_drop_and_full_store(clean):
    chip = clean
    rng = np.random.default_rng(5)
    a = fc.frame(rng, 400, plant_at=range(0, 400, 29))
    y = fc.view_of(rng, a, extra=30)
    z = fc.view_of(rng, a, n=150, extra=400)
    for i, f in ((-3, a), (7, y), (2 ** 40, z)):
        chip.frame_put(i, f)
    # a repeated id and a_id itself
    got = stored_all(chip, -3, [7, -3, 7, 2 ** 40], KINV)
    assert blob(got) == blob(host_all(chip, a, [y, a, y, z], KINV))
    assert blob(got[:1]) == blob(got[2:3]) and got[1]["summary"]["n_matches_gms"] > 0
    # replace: the next match uses the new content (the old one gives other counts)
    my, mz = M.match_pair(a, y, KINV), M.match_pair(a, z, KINV)
    assert my["summary"] != mz["summary"] and my["summary"]["n_matches_gms"] != mz["summary"]["n_matches_gms"]
    assert_same_result(got[0], my, "y")
    chip.frame_put(7, z)
    assert chip.frame_store_info()["n_frames"] == 3
    again = stored_all(chip, -3, [7], KINV)
    assert_same_result(again[0], mz, "replaced")
    assert chip.frame_read(7)["n"] == len(z["kp"])
    # drop, then match: RANGE, and nothing is selected
    chip.frame_drop(7)
    assert status_of(chip.match_batch_stored, -3, [2 ** 40, 7], KINV) == capi.CHIP_ERR_RANGE
    assert status_of(chip.match_read_sets, capi.MatchSummary()) == capi.CHIP_ERR_BUSY
    assert status_of(chip.match_batch_stored, 7, [-3], KINV) == capi.CHIP_ERR_RANGE
    assert status_of(chip.frame_drop, 7) == capi.CHIP_ERR_RANGE and status_of(chip.frame_read, 7) == capi.CHIP_ERR_RANGE
    # what an earlier match left stays valid after the drop of its frames
    kept = stored_all(chip, -3, [2 ** 40], KINV)
    chip.frame_drop(2 ** 40)
    chip.match_select(0)
    assert same_bytes(chip.match_read_sets(capi.MatchSummary(**kept[0]["summary"]))["X_ab"], kept[0]["X_ab"])
    # fill all slots, once more: OOM; drop one: the put succeeds
    tiny = fc.frame(rng, 5)
    for i in range(10, 10 + N_SLOTS - 1):
        chip.frame_put(i, tiny)
    assert chip.frame_store_info()["n_frames"] == N_SLOTS
    assert status_of(chip.frame_put, 50, tiny) == capi.CHIP_ERR_OOM
    chip.frame_put(10, y)                                            # a replace needs no free slot
    assert status_of(chip.frame_store_reserve, N_SLOTS, SLOT_KP // 2) == capi.CHIP_ERR_BUSY
    chip.frame_store_reserve(N_SLOTS, SLOT_KP)                       # the same numbers: a no-op
    assert same_bytes(chip.frame_read(-3)["kp"], a["kp"])
    chip.frame_drop(11)
    chip.frame_put(50, z)
    assert_same_result(stored_all(chip, -3, [50, 10], KINV)[0], mz, "after the drop")
    # more keypoints than a slot holds: the store is as it was
    wide = fc.frame(rng, SLOT_KP + 1)
    assert status_of(chip.frame_put, 50, wide) == capi.CHIP_ERR_UNSUPPORTED
    assert chip.frame_read(50)["n"] == len(z["kp"])
    assert status_of(chip.match_batch_stored, -3, [10] * 17, KINV) == capi.CHIP_ERR_UNSUPPORTED
    assert status_of(chip.match_batch_stored, -3, [], KINV) == capi.CHIP_ERR_INVALID_ARG


def test_reserve_rules_on_a_fresh_ctx_and_group_ctx():
    rng = np.random.default_rng(6)
    f = fc.frame(rng, 40)
    with capi.Chip(4096) as c:
        assert c.frame_store_info() == dict(n_slots=0, slot_keypoints=0, n_frames=0)
        assert status_of(c.frame_put, 1, f) == capi.CHIP_ERR_BUSY
        assert status_of(c.frame_read, 1) == capi.CHIP_ERR_BUSY
        assert status_of(c.match_batch_stored, 1, [1], KINV) == capi.CHIP_ERR_BUSY
        assert status_of(c.frame_drop, 1) == capi.CHIP_ERR_RANGE
        c.frame_store_reserve(2, 64)
        c.frame_put(1, f)
        assert status_of(c.frame_store_reserve, 3, 64) == capi.CHIP_ERR_BUSY
        assert status_of(c.frame_put, 2, fc.frame(rng, 65)) == capi.CHIP_ERR_UNSUPPORTED
        c.frame_drop(1)
        c.frame_store_reserve(3, 128)                                # empty: other numbers are taken
        assert c.frame_store_info() == dict(n_slots=3, slot_keypoints=128, n_frames=0)
        g = fc.frame(rng, 128)
        c.frame_put(2, g)
        assert same_bytes(c.frame_read(2)["pts"], S.gather(g["kp"], g["xyz"]))
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.frame_store_reserve, 2, 64) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_put, 1, f) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_drop, 1) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_read, 1) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_store_info) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.match_batch_stored, 1, [1], KINV) == capi.CHIP_ERR_UNSUPPORTED


def test_empty_frames(clean):
    chip = clean
    rng = np.random.default_rng(7)
    a = fc.frame(rng, 300)
    b = fc.view_of(rng, a)
    chip.frame_put(0, fc.empty_frame()); chip.frame_put(1, a); chip.frame_put(2, b)
    r = chip.frame_read(0)
    assert (r["n"], r["width"], r["height"]) == (0, 9, 7) and r["pts"].shape == (0, 4)
    got = stored_all(chip, 1, [0, 2, 0], KINV)                       # an empty candidate between two calls on the same slabs
    assert blob(got) == blob(host_all(chip, a, [fc.empty_frame(), b, fc.empty_frame()], KINV))
    assert not any(got[0]["summary"].values()) and (got[0]["train_idx"] == -1).all() and got[1]["summary"]["n_matches_gms"] > 0
    for sm in chip.match_batch_stored(0, [1, 0, 2], KINV):           # an empty query frame
        assert not any(sm.as_dict().values())
    chip.match_select(2)
    assert chip.match_batch_matches(2)[0].shape == (0,)
    assert chip.pnp_matched(capi.CHIP_SET_AB, 0)["status"] == capi.CHIP_ERR_TOO_FEW_POINTS


def test_staging_does_not_leak_between_puts(clean, five):
    chip = clean
    rng = np.random.default_rng(8)
    x = five["cands"][0]                                             # 752 x 480
    w, h = 40, 30
    y = fc.view_of(rng, dict(desc=x["desc"], kp=x["kp"], xyz=x["xyz"]), n=600, jitter=0.05, w=w, h=h)   # x's keypoints on another image size
    assert y["xyz"].shape == (h, w, 3)
    chip.frame_put(1, x)
    before = chip.frame_read(1)
    chip.frame_put(2, y)
    after = chip.frame_read(1)
    assert all(same_bytes(before[k], after[k]) for k in ("desc", "kp", "pts")) and same_bytes(after["pts"], S.gather(x["kp"], x["xyz"]))
    assert same_bytes(chip.frame_read(2)["pts"], S.gather(y["kp"], y["xyz"]))
    got = stored_all(chip, 1, [2, 1], KINV)                          # two image sizes in one batch
    assert got[0]["summary"]["n_matches_gms"] > 0
    assert blob(got) == blob(host_all(chip, x, [y, x], KINV))


def _same_estimate(d: dict, h: dict, what):
    assert d["status"] == h["status"] == 0, what
    assert d["summary"] == h["summary"] and d["confidence"] == h["confidence"], what
    assert same_bytes(d["T"], h["T"]) and same_bytes(d["mask"], h["mask"]), what


def test_state_across_paths_and_the_solvers(clean, five):
    chip, a, cands, Kinv = clean, five["a"], five["cands"], five["Kinv"]
    chip.frame_put(100, a)
    for j, b in enumerate(cands):
        chip.frame_put(j, b)
    ids = list(range(5))
    host = host_all(chip, a, cands, Kinv)
    first = stored_all(chip, 100, ids, Kinv)
    assert blob(first) == blob(host)
    p = chip.match_pair(a, cands[3], Kinv)                           # host frames in between
    for k in SET_KEYS:
        assert same_bytes(p[k], np.ascontiguousarray(five["mirror"][3][k])), k
    assert status_of(chip.match_batch_matches, 0) == capi.CHIP_ERR_BUSY   # the keys belong to a batch
    assert blob(stored_all(chip, 100, ids, Kinv)) == blob(host)

    def solve(sms):
        problems = []
        for j, sm in enumerate(sms):
            if sm.n_matches_gms >= 150:                              # the survivors
                problems += [(j, capi.CHIP_SET_AB, sm.n_3d2d_ab), (j, capi.CHIP_SET_BA, sm.n_3d2d_ba)]
        prm = capi.default_ransac_params(); prm.seed = 5
        pnp = chip.pnp_matched_batch(problems, prm, [100 + 7 * i for i in range(len(problems))])
        icp = []
        for j in (0, 2):
            chip.match_select(j)
            pi = capi.default_icp_params(); pi.seed = 3 + j
            icp.append(chip.icp_matched(sms[j].n_3d3d, pi))
        return problems, pnp, icp

    ph, pnp_h, icp_h = solve(chip.match_batch(a, cands, Kinv))
    ps, pnp_s, icp_s = solve(chip.match_batch_stored(100, ids, Kinv))
    assert ph == ps and len(ph) == 8
    for i, (d, h) in enumerate(zip(pnp_s, pnp_h)):
        _same_estimate(d, h, i)
    for i, (d, h) in enumerate(zip(icp_s, icp_h)):
        _same_estimate(d, h, i)


def test_put_match_drop_back_to_back(clean):
    """50 rounds of put, match, drop of a candidate with changing content: the put is ordered before the match on the ctx stream"""
    chip = clean
    rng = np.random.default_rng(9)
    a = fc.frame(rng, 320, plant_at=(0, 63, 64, 319))
    sa = S.stored(a)
    chip.frame_put(1, a)
    seen = set()
    for r in range(50):
        b = fc.view_of(rng, a, n=200 + 2 * r, extra=r)
        chip.frame_put(2, b)
        got = stored_all(chip, 1, [2], KINV)
        chip.frame_drop(2)
        m = S.match_pair(sa, S.stored(b), KINV)
        assert_same_result(got[0], m, r)
        seen.add(m["summary"]["n_matches_gms"])
    assert len(seen) > 10 and min(seen) > 0


def test_resident_tick_mode_allocates_inside_a_pause(five, monkeypatch):
    """with CHIP_TICK_RESIDENT=1 the store, the staging image and the slabs of the first stored batch are allocated next to a resident
    scan instance: same bytes"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    a, cands, Kinv = five["a"], five["cands"], five["Kinv"]
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        for l in scenarios.default_schedule(400)[:8]:
            c.loop_tick(l)
        c.frame_store_reserve(6, 4096)
        c.frame_put(100, a)
        for j, b in enumerate(cands):
            c.frame_put(j, b)
        got = stored_all(c, 100, list(range(5)), Kinv)
        c.loop_tick(400)
    for j, (g, m) in enumerate(zip(got, five["mirror"])):
        assert_same_result(g, m, j)


@functools.lru_cache(maxsize=None)
def _first_use_calls() -> dict:
    """the four calls of test_first_use_order_of_frame_and_match_state, name -> call(ctx) -> dict of arrays / summaries; shapes of cases
    the other GPU tests use (stereo_bm: 43 x 11, rectification: 80 x 70, host frames: 64 x 48 with 257 keypoints)"""
    import rectify_cases as RC
    import stereo_bm_cases as SC
    left, right, _ = SC.tiled_pair(np.random.default_rng(43), 43, 11, tile=16, lo=0, hi=31)
    bm = SC.case("first_use", left, right, 32, 7)["params"]
    w, h = 80, 70
    lraw, rraw = RC.image(w, h), RC.image(w, h, 1)
    lm, rm = RC.radtan(w, h) + RC.rotation(w, h), RC.random_map(w, h, 3) + RC.random_map(w, h, 4)
    rng = np.random.default_rng(257)
    a = fc.frame(rng, 257, plant_at=(0, 63, 64, 256))
    b = fc.view_of(rng, a, extra=20)

    def rectify(c):
        c.rectify_set_maps(lm, rm)
        lo, ro = c.rectify_pair(lraw, rraw)
        return dict(left=lo, right=ro)

    def put(c):
        c.frame_store_reserve(2, 512)
        c.frame_put(7, a)
        return c.frame_read(7)

    return dict(stereo_bm=lambda c: dict(disp=c.stereo_bm(left, right, bm)), rectify=rectify, match_pair=lambda c: c.match_pair(a, b, KINV), put=put)


def _first_use_run(first: str) -> bytes:
    """a fresh ctx runs `first`, then the other three calls in their listed order, then the put frame against itself: every output, as bytes"""
    calls = _first_use_calls()
    got = {}
    with capi.Chip(4096) as c:
        for name in [first] + [n for n in calls if n != first]:
            got[name] = calls[name](c)
        got["stored"] = stored_all(c, 7, [7], KINV)[0]
    assert got["match_pair"]["summary"]["n_matches_gms"] > 0 and got["stored"]["summary"]["n_matches_gms"] > 0 and got["put"]["n"] == 257
    assert (got["stereo_bm"]["disp"] != -16).any() and got["rectify"]["left"].any()
    return b"".join(name.encode() + k.encode() + (np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
                    for name in sorted(got) for k, v in sorted(got[name].items()))


@pytest.fixture(scope="module")
def first_use_listed_order():
    return _first_use_run("stereo_bm")


@pytest.mark.parametrize("first", ["stereo_bm", "rectify", "match_pair", "put"])
def test_first_use_order_of_frame_and_match_state(first_use_listed_order, first):
    """The frame state and the match state of a ctx come into being apart, each on the first call that needs it: whichever call is the
    first on a fresh ctx -- a dense block matcher call or the rectification (frame state alone), a match of host frames (match state
    alone), the reserve (both) -- every later output equals, bit for bit, what one ctx running the four in the listed order returns."""
    assert _first_use_run(first) == first_use_listed_order


def test_verify_candidates_stored_example():
    exe = LIB / "verify_candidates_stored"
    assert exe.exists()
    r = subprocess.run([str(exe), "3000", "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== verify_candidates") == 6 and "DIFFERS" not in r.stdout
