"""GPU parity of chip_match_pairs_stored (cerebro_amd/csrc/match.hip: hamming_match_pairs, pairs_gms / pairs_grid_modes +
pairs_mode_select, pose_sets_stored_pairs) through ctypes -> C ABI.  A list of (query, candidate) pairs of stored frames, every pair
with a query frame of its own, gives per pair the bytes of chip_match_batch_stored[_modes] with B = 1 on that pair AND of the numpy
restatement; the batched solvers work on the result with the pair index as the candidate index.  The case set is
tests/match_pairs_cases.py; the store is 12 slots x 3471 keypoints."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import match_batch_cases as cases
import match_pairs_cases as PC
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
SET_KEYS = PC.SET_KEYS
KINV = PC.kinv()
MODES = (0, 2, 3)


def load(chip, frames: dict):
    """the store holds exactly `frames` (name -> frame) under the ids of ID / GEO_ID afterwards"""
    for i in list(PC.ID.values()) + list(GEO_ID.values()):
        if chip.lib.chip_frame_drop(chip.h, i) not in (capi.CHIP_OK, capi.CHIP_ERR_RANGE):
            raise AssertionError("chip_frame_drop")
    for name, f in frames.items():
        chip.frame_put(ALL_ID[name], f)


def new_chip():
    c = capi.Chip(4096)
    c.frame_store_reserve(PC.N_SLOTS, PC.SLOT_KP)
    return c


@pytest.fixture(scope="module")
def chip():
    with new_chip() as c:
        yield c


@pytest.fixture
def case_chip(chip):
    """the module's ctx with the frames of the case set in its store"""
    load(chip, PC.frames())
    return chip


def same_bytes(a: np.ndarray, b: np.ndarray):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_choice(got: dict, want: dict):
    return (got["scale"], got["rotation"], got["n_inliers"]) == (want["scale"], want["rotation"], want["n_inliers"]) and \
        np.array_equal(got["counts"], want["counts"])


def everything(chip, sms, choices):
    """what a run left, per candidate / pair: dict(summary, choice, the ten sets, train_idx, distance)"""
    out = []
    for j, (sm, ch) in enumerate(zip(sms, choices)):
        chip.match_select(j)
        d = dict(summary=sm.as_dict(), choice=ch)
        d.update(chip.match_read_sets(sm))
        d["train_idx"], d["distance"] = chip.match_batch_matches(j)
        out.append(d)
    return out


def pairs_all(chip, pairs, modes, id_of=None):
    id_of = id_of or ALL_ID
    return everything(chip, *chip.match_pairs_stored([id_of[a] for a, _ in pairs], [id_of[b] for _, b in pairs], KINV, modes))


def one_by_one(chip, pairs, modes):
    """the loop the call replaces: chip_match_batch_stored_modes with B = 1 per pair"""
    out = []
    for a, b in pairs:
        out += everything(chip, *chip.match_batch_stored(ALL_ID[a], [ALL_ID[b]], KINV, modes))
    return out


def blob(results) -> bytes:
    def one(r):
        ch = r["choice"]
        head = repr(r["summary"]).encode() + repr((ch["scale"], ch["rotation"], ch["n_inliers"])).encode() + np.ascontiguousarray(ch["counts"]).tobytes()
        return head + b"".join(np.ascontiguousarray(r[k]).tobytes() for k in SET_KEYS + ("train_idx", "distance"))
    return b"|".join(one(r) for r in results)


def assert_equals_mirror(g: dict, want: dict, n1: int, what):
    assert g["summary"] == want["summary"], what
    assert same_choice(g["choice"], want["choice"]), (what, g["choice"])
    assert g["train_idx"].shape == g["distance"].shape == (n1,), what     # the n of THIS pair's query frame
    if not want["summary"]["n_matches_all"]:                               # an empty frame on either side: no train descriptors
        assert (g["train_idx"] == -1).all() and (g["distance"] == -1).all(), what
        return
    for k in SET_KEYS + ("train_idx", "distance"):
        assert same_bytes(g[k], np.ascontiguousarray(want[k])), (what, k)


def status_of(call, *args):
    with pytest.raises(capi.ChipError) as e:
        call(*args)
    return e.value.status


# ---------------------------------------------------------------------------------------------- the launch-geometry frames
def _slice(f: dict, n: int) -> dict:
    return dict(desc=np.ascontiguousarray(f["desc"][:n]), kp=np.ascontiguousarray(f["kp"][:n]), xyz=f["xyz"])


def geo_frames() -> dict:
    """queries of 255 / 256 / 257 / 1 keypoints (the first keypoints of A) and candidates of 1 / 1023 / 1024 / 1025 (of c3; the
    candidate of one keypoint is the query of one): the block of 256 queries and the tile of 1024 train descriptors from both sides"""
    f = PC.frames()
    out = {f"X{n}": _slice(f["A"], n) for n in (255, 256, 257, 1)}
    out.update({f"Y{n}": _slice(f["c3"], n) for n in (1023, 1024, 1025)})
    return out


GEO_ID = {name: 5000 + k for k, name in enumerate(("X255", "X256", "X257", "X1", "Y1023", "Y1024", "Y1025"))}
ALL_ID = dict(PC.ID, **GEO_ID)
# the widest query frame (257: a second block of ONE query) at the last index
GEO_PAIRS = (("X255", "Y1023"), ("X256", "Y1024"), ("X1", "Y1025"), ("X255", "X1"), ("X256", "Y1025"), ("X1", "X1"), ("X256", "Y1023"), ("X257", "Y1025"))

_fresh = {}


def fresh(kind: str, modes):
    """the blob of the case set ("case") or of the geometry call ("geo") on a ctx that ran nothing else; computed once per process"""
    if (kind, modes) not in _fresh:
        with new_chip() as c:
            load(c, PC.frames() if kind == "case" else geo_frames())
            _fresh[kind, modes] = blob(pairs_all(c, PC.PAIRS if kind == "case" else GEO_PAIRS, modes))
    return _fresh[kind, modes]


# ---------------------------------------------------------------------------------------------- 1: the case set
@pytest.mark.parametrize("modes", MODES)
def test_case_set_equals_mirror_and_batches_of_one(case_chip, modes):
    chip = case_chip
    assert chip.lib.chip_build_has_match_pairs() == 1 and chip.lib.chip_abi_version() == 7
    got = pairs_all(chip, PC.PAIRS, modes)
    want = PC.mirror(modes)
    assert len(got) == len(want) == len(PC.PAIRS) == 11
    for j, (g, w) in enumerate(zip(got, want)):                       # every pair, none skipped
        assert_equals_mirror(g, w, PC.EXPECTED_N1[j], (modes, j, PC.PAIRS[j]))
    if modes == 0:
        assert tuple(g["summary"]["n_matches_gms"] for g in got) == PC.EXPECTED_GMS
        assert tuple(g["summary"]["n_matches_all"] for g in got) == tuple(0 if j in (7, 8) else n for j, n in enumerate(PC.EXPECTED_N1))
    chip.match_select(0)                                              # pair 0 is what a fresh result has selected
    loop = one_by_one(chip, PC.PAIRS, modes)
    for j, (g, l) in enumerate(zip(got, loop)):
        assert blob([g]) == blob([l]), (modes, j, PC.PAIRS[j])


def test_pair_zero_is_selected_and_modes_none_is_the_plain_call(case_chip):
    chip = case_chip
    a_ids, b_ids = PC.ids()
    sms = chip.match_pairs_stored(a_ids, b_ids, KINV)                 # modes None: the summaries alone
    assert [s.as_dict() for s in sms] == [m["summary"] for m in PC.mirror(0)]
    sets = chip.match_read_sets(sms[0])                               # no match_select: pair 0
    for k in SET_KEYS:
        assert same_bytes(sets[k], np.ascontiguousarray(PC.mirror(0)[0][k])), k
    assert status_of(chip.match_select, 11) == capi.CHIP_ERR_RANGE and status_of(chip.match_batch_matches, 11) == capi.CHIP_ERR_RANGE


# ---------------------------------------------------------------------------------------------- 2: edges of the launch geometry
def test_query_blocks_and_train_tiles_at_their_edges(chip):
    f = geo_frames()
    load(chip, f)
    got = pairs_all(chip, GEO_PAIRS, 0)
    for j, ((a, b), g) in enumerate(zip(GEO_PAIRS, got)):
        idx, dist = cases.hamming_search(f[a]["desc"], f[b]["desc"])
        assert same_bytes(g["train_idx"], idx) and same_bytes(g["distance"], dist), (j, a, b)
        assert g["summary"]["n_matches_all"] == len(f[a]["kp"])
    assert [len(g["train_idx"]) for g in got] == [255, 256, 1, 255, 256, 1, 256, 257]
    assert (got[3]["train_idx"] == 0).all() and (got[5]["train_idx"] == 0).all()   # one train descriptor
    loop = one_by_one(chip, GEO_PAIRS, 0)
    for j, (g, l) in enumerate(zip(got, loop)):
        assert blob([g]) == blob([l]), (j, GEO_PAIRS[j])


# ---------------------------------------------------------------------------------------------- 3: stale slabs
@pytest.mark.parametrize("modes", [0, 3])
def test_rows_of_another_stride_leave_nothing_behind(chip, modes):
    """the case set (stride 2100), the geometry call (stride 257) through the same keys, planes and slabs, the case set again"""
    load(chip, PC.frames())
    first = blob(pairs_all(chip, PC.PAIRS, modes))
    load(chip, geo_frames())
    small = blob(pairs_all(chip, GEO_PAIRS, modes))
    load(chip, PC.frames())
    again = blob(pairs_all(chip, PC.PAIRS, modes))
    assert first == fresh("case", modes)
    assert small == fresh("geo", modes)
    assert again == fresh("case", modes)


# ---------------------------------------------------------------------------------------------- 4: downstream
def _same_estimate(d: dict, h: dict, what):
    assert d["status"] == h["status"], what
    if h["status"] != 0:
        assert h["status"] == capi.CHIP_ERR_TOO_FEW_POINTS, what
        return
    assert d["summary"] == h["summary"] and d["confidence"] == h["confidence"], what
    assert same_bytes(d["T"], h["T"]) and same_bytes(d["mask"], h["mask"]), what


def _params(make, **kw):
    p = make()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw", [dict(), dict(n_hypotheses=65, sampler=capi.CHIP_SAMPLER_THEIA_PERSISTENT)], ids=["fresh", "theia_65"])
def test_batched_solvers_on_the_pairs_equal_singles_after_batches_of_one(case_chip, kw):
    chip = case_chip
    a_ids, b_ids = PC.ids()
    sms = chip.match_pairs_stored(a_ids, b_ids, KINV)
    P = len(sms)
    pnp_problems = []
    for j, sm in enumerate(sms):
        pnp_problems += [(j, capi.CHIP_SET_AB, sm.n_3d2d_ab), (j, capi.CHIP_SET_BA, sm.n_3d2d_ba)]
    pnp_seeds = [100 + 7 * i for i in range(2 * P)]
    icp_seeds = [900 + 3 * j for j in range(P)]
    chip.match_select(3)
    pnp_alone = chip.pnp_matched_batch(pnp_problems, _params(capi.default_ransac_params, seed=5, **kw), pnp_seeds)
    icp_alone = chip.icp_matched_batch([(j, sms[j].n_3d3d) for j in range(P)], _params(capi.default_icp_params, seed=6, **kw), icp_seeds)
    ticket = chip.icp_matched_batch_enqueue([(j, sms[j].n_3d3d) for j in range(P)], _params(capi.default_icp_params, seed=6, **kw), icp_seeds)
    pnp = chip.pnp_matched_batch(pnp_problems, _params(capi.default_ransac_params, seed=5, **kw), pnp_seeds)   # the ICP batch runs underneath
    icp = chip.icp_matched_batch_collect(ticket)
    sets = chip.match_read_sets(sms[3])                               # the selection is untouched: still pair 3
    for k in SET_KEYS:
        assert same_bytes(sets[k], np.ascontiguousarray(PC.mirror(0)[3][k])), k
    few = [j for j, sm in enumerate(sms) if sm.n_3d3d < 20]
    assert few == [5, 7, 8] and all(icp[j]["status"] == capi.CHIP_ERR_TOO_FEW_POINTS for j in few)
    assert all(pnp[2 * j + w]["status"] == capi.CHIP_ERR_TOO_FEW_POINTS for j in few for w in (0, 1))
    assert sum(r["status"] == 0 for r in pnp) == 2 * (P - 3) and sum(r["status"] == 0 for r in icp) == P - 3
    for j, (a, b) in enumerate(PC.PAIRS):                             # the single calls after a batch of one of that pair
        (sm,) = chip.match_batch_stored(PC.ID[a], [PC.ID[b]], KINV)
        assert sm.as_dict() == sms[j].as_dict()
        for w, n in ((capi.CHIP_SET_AB, sm.n_3d2d_ab), (capi.CHIP_SET_BA, sm.n_3d2d_ba)):
            single = chip.pnp_matched(w, n, _params(capi.default_ransac_params, seed=pnp_seeds[2 * j + w], **kw))
            _same_estimate(pnp[2 * j + w], single, ("pnp", j, w))
            _same_estimate(pnp_alone[2 * j + w], single, ("pnp alone", j, w))
        single = chip.icp_matched(sm.n_3d3d, _params(capi.default_icp_params, seed=icp_seeds[j], **kw))
        _same_estimate(icp[j], single, ("icp", j))
        _same_estimate(icp_alone[j], single, ("icp alone", j))


# ---------------------------------------------------------------------------------------------- 5: state across the entries
def test_state_across_pairs_pair_batch_and_pairs(case_chip):
    chip, f = case_chip, PC.frames()
    five = cases.five_candidates()
    want = fresh("case", 0)
    assert blob(pairs_all(chip, PC.PAIRS, 0)) == want
    p = chip.match_pair(f["A"], f["c3"], KINV)                        # host frames in between
    for k in SET_KEYS:
        assert same_bytes(p[k], np.ascontiguousarray(five["mirror"][3][k])), k
    assert status_of(chip.match_batch_matches, 0) == capi.CHIP_ERR_BUSY   # the keys belong to a batch or a pair list
    sms = chip.match_batch_stored(PC.ID["A"], [PC.ID[f"c{j}"] for j in range(5)], KINV)
    for j, sm in enumerate(sms):
        chip.match_select(j)
        assert sm.as_dict() == five["mirror"][j]["summary"]
        sets = chip.match_read_sets(sm)
        idx, dist = chip.match_batch_matches(j)
        if sm.n_matches_all:
            for k in SET_KEYS:
                assert same_bytes(sets[k], np.ascontiguousarray(five["mirror"][j][k])), (j, k)
            assert same_bytes(idx, five["mirror"][j]["train_idx"]) and same_bytes(dist, five["mirror"][j]["distance"])
    assert blob(pairs_all(chip, PC.PAIRS, 0)) == want
    assert chip.match_batch_matches(2)[0].shape == (2100,)           # ... and answers after the pairs call


# ---------------------------------------------------------------------------------------------- 6: status codes
def test_status_codes(case_chip):
    chip = case_chip
    a_ids, b_ids = PC.ids()
    ia, ib = np.array(a_ids, np.int64), np.array(b_ids, np.int64)
    Ki = np.ascontiguousarray(KINV, np.float64).reshape(9)
    sm, ch = (capi.MatchSummary * 16)(), (capi.GmsChoice * 16)()
    raw = lambda a, b, P, K, modes, s: chip.lib.chip_match_pairs_stored(chip.h, a, b, P, K, modes, s, ch)
    A, B, K = capi._ptr(ia), capi._ptr(ib), capi._ptr(Ki)
    assert raw(A, B, 0, K, 0, sm) == raw(A, B, -1, K, 0, sm) == capi.CHIP_ERR_INVALID_ARG
    assert raw(None, B, 2, K, 0, sm) == raw(A, None, 2, K, 0, sm) == raw(A, B, 2, None, 0, sm) == raw(A, B, 2, K, 0, None) == capi.CHIP_ERR_INVALID_ARG
    assert raw(A, B, 2, K, 4, sm) == raw(A, B, 2, K, 0x80000001, sm) == capi.CHIP_ERR_INVALID_ARG
    assert chip.lib.chip_match_pairs_stored(chip.h, A, B, 2, K, 3, sm, None) == capi.CHIP_OK      # choice may be NULL
    assert status_of(chip.match_pairs_stored, [PC.ID["A"]] * 17, [PC.ID["c0"]] * 17, KINV) == capi.CHIP_ERR_UNSUPPORTED
    assert len(chip.match_pairs_stored([PC.ID["A"]] * 16, [PC.ID["c0"]] * 16, KINV)) == 16
    # an unknown id in the middle of the list, on either side: RANGE, and nothing is selected afterwards
    for side in (0, 1):
        chip.match_pairs_stored(a_ids, b_ids, KINV)
        bad = [list(a_ids), list(b_ids)]
        bad[side][5] = 424242
        assert status_of(chip.match_pairs_stored, bad[0], bad[1], KINV) == capi.CHIP_ERR_RANGE
        assert status_of(chip.match_read_sets, capi.MatchSummary()) == capi.CHIP_ERR_BUSY
        assert status_of(chip.match_select, 0) == capi.CHIP_ERR_BUSY and status_of(chip.match_batch_matches, 0) == capi.CHIP_ERR_BUSY
    # refused arguments leave nothing selected either
    chip.match_pairs_stored(a_ids, b_ids, KINV)
    assert raw(A, B, 0, K, 0, sm) == capi.CHIP_ERR_INVALID_ARG
    assert status_of(chip.match_select, 0) == capi.CHIP_ERR_BUSY
    with capi.Chip(4096) as c:                                        # before any chip_frame_store_reserve
        assert status_of(c.match_pairs_stored, [1], [2], KINV) == capi.CHIP_ERR_BUSY
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.match_pairs_stored, [1], [2], KINV) == capi.CHIP_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 7: first use next to a resident scan
def test_resident_tick_mode_allocates_inside_a_pause(monkeypatch):
    """with CHIP_TICK_RESIDENT=1 the store, the slabs and the mode tables of the first pair list are allocated next to a resident scan
    instance: same bytes"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        ticks = scenarios.default_schedule(400)
        for l in ticks[:8]:
            c.loop_tick(l)
        c.frame_store_reserve(PC.N_SLOTS, PC.SLOT_KP)
        load(c, PC.frames())
        plain = pairs_all(c, PC.PAIRS, 0)
        c.loop_tick(ticks[8])
        modes = pairs_all(c, PC.PAIRS, 2)
        c.loop_tick(400)
    for j, (g, w) in enumerate(zip(plain, PC.mirror(0))):
        assert_equals_mirror(g, w, PC.EXPECTED_N1[j], j)
    for j, (g, w) in enumerate(zip(modes, PC.mirror(2))):
        assert_equals_mirror(g, w, PC.EXPECTED_N1[j], j)


# ---------------------------------------------------------------------------------------------- 8: the example
def test_verify_pairs_stored_example():
    exe = LIB / "verify_pairs_stored"
    assert exe.exists()
    r = subprocess.run([str(exe), "3000", "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== verify_candidates_stored with B = 1") == 6 and "DIFFERS" not in r.stdout
