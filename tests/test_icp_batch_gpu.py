"""GPU parity of the batched Umeyama-ICP-in-RANSAC (cerebro_amd/csrc/icp.hip: icp_models / icp_score with a problem dimension) through
ctypes -> C ABI: a problem of a batch gives the bits of chip_icp_ransac with that seed whatever the batch is, every hypothesis of every
problem equals the oracle's record, the matched batch equals chip_match_select + chip_icp_ransac_matched, it runs underneath the batched
PnP, and the pending / status rules hold.  Small shapes throughout."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import match_batch_cases as cases
import oracle_lib as O
import ransac_records as R
from cerebro_amd import capi
from cerebro_amd.synth import make_icp_scene

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
ICP = capi.CHIP_RANSAC_LEG_ICP
SET_KEYS = cases.SET_KEYS
# sixteen problems, ragged, the smallest last; problem 5 is problem 3 again (same points, same seed)
POOL_N = (1025, 63, 64, 65, 200, 65, 200, 63, 64, 1025, 200, 64, 63, 65, 200, 20)
MODES = dict(reference=dict(), one_block=dict(n_hypotheses=64), two_blocks=dict(n_hypotheses=65))


def gparams(**kw):
    p = capi.default_icp_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def status_of(call, *args):
    with pytest.raises(capi.ChipError) as e:
        call(*args)
    return e.value.status


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(64) as c:
        yield c


@pytest.fixture(scope="module")
def pool():
    """-> (problems [(A, B)], seeds), built once and left unchanged"""
    probs = []
    for i, N in enumerate(POOL_N):
        if i % 2:
            probs.append(R.half_inlier_icp_scene(N, 40 + i))
        else:
            probs.append(make_icp_scene(N=N, outlier_frac=0.2, noise=0.02, seed=40 + i)[:2])
    probs[5] = probs[3]
    seeds = [100 + 3 * i for i in range(len(probs))]
    seeds[5] = seeds[3]
    return probs, seeds


@pytest.fixture(scope="module")
def five():
    return cases.five_candidates()


def same_estimate(d: dict, h: dict, what):
    assert d["status"] == h["status"], what
    if h["status"] != 0:
        return
    R.same_summary(d, h)


def assert_left_out(r: dict, N: int, what):
    """the documented answer of a problem that was left out of the launch"""
    assert r["status"] == capi.CHIP_ERR_TOO_FEW_POINTS and r["confidence"] == -1.0 and r["T"] is None, what
    raw = r["raw"]
    assert np.isnan(raw["T"]).all() and raw["confidence"] == -1.0, what
    assert raw["summary"] == dict(n_iterations=0, n_inliers=0, best_hypothesis=-1, n_models=0, best_cost=0.0), what
    assert (raw["mask"] == 0xAB).all(), what                      # untouched


# ---------------------------------------------------------------------------------------------- batch equals singles
@pytest.mark.parametrize("sampler", [capi.CHIP_SAMPLER_FRESH, capi.CHIP_SAMPLER_THEIA_PERSISTENT])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_batch_equals_singles(chip, pool, mode, sampler):
    probs, seeds = pool
    kw = dict(MODES[mode], sampler=sampler)
    singles = [chip.icp_ransac(A, B, gparams(seed=s, **kw)) for (A, B), s in zip(probs, seeds)]
    assert any(s["summary"]["best_hypothesis"] >= 0 for s in singles)
    for lo, hi in ((0, 1), (14, 16), (1, 6), (11, 16), (0, 16)):   # P = 1, 2, 5, 5 (other positions), 16
        got = chip.icp_ransac_batch(probs[lo:hi], gparams(seed=999, **kw), seeds[lo:hi])
        assert len(got) == hi - lo
        for i, g in enumerate(got):
            same_estimate(g, singles[lo + i], (mode, sampler, lo, hi, i))
        sh = chip.ransac_record_shape(ICP, hi - lo - 1)
        assert sh["P"] == hi - lo and sh["words"] == (max(POOL_N[lo:hi]) + 63) // 64 and sh["N"] == POOL_N[hi - 1]
    got = chip.icp_ransac_batch(probs[1:6], gparams(seed=999, **kw), seeds[1:6])
    for k in ("T", "mask"):                                        # problems 3 and 5: the same points and seed
        assert got[2][k].tobytes() == got[4][k].tobytes()
    assert got[2]["summary"] == got[4]["summary"] and got[2]["confidence"] == got[4]["confidence"]
    # NULL seeds: p->seed for every problem
    one = chip.icp_ransac_batch([probs[4], probs[4]], gparams(seed=seeds[4], **kw))
    same_estimate(one[0], singles[4], "null seeds")
    same_estimate(one[1], singles[4], "null seeds")


# ---------------------------------------------------------------------------------------------- every hypothesis
@pytest.fixture(scope="module")
def ragged_five():
    A2, _ = R.half_inlier_icp_scene(70, 9)
    return [R.icp_gate_scene(0.9, 3), R.half_inlier_icp_scene(65, 8), (A2, 2.0 * A2), R.icp_gate_scene(1 / 0.901, 4), make_icp_scene(N=20, noise=0.01, seed=6)[:2]]


@pytest.mark.parametrize("sampler", [capi.CHIP_SAMPLER_FRESH, capi.CHIP_SAMPLER_THEIA_PERSISTENT])
def test_every_hypothesis_of_a_ragged_batch(chip, ragged_five, sampler):
    seeds = [11, 12, 13, 14, 15]
    kw = dict(n_hypotheses=65, sampler=sampler)
    got = chip.icp_ransac_batch(ragged_five, gparams(seed=1, **kw), seeds)
    widest = (200 + 63) // 64
    for k, (A, B) in enumerate(ragged_five):
        p = O.icp_params(seed=seeds[k], **kw)
        dev, cpu = chip.ransac_record(ICP, k), R.icp_record(A, B, p, words=widest)
        N = A.shape[0]
        assert (dev["P"], dev["H"], dev["N"], dev["words"]) == (5, 65, N, widest)
        R.assert_record_equal(dev, cpu, N, "icp", f"problem {k}")
        assert not dev["mask"][:, (N + 63) // 64:].any()           # a narrower problem: nothing beyond its own words
        R.same_summary(got[k], R.select(cpu, N, p))
        frac = cpu["valid"].mean()
        if k in (0, 3):
            assert 0.1 <= frac <= 0.9, (k, frac)                   # the gate scenes: both sides of min(s, 1 / s) > 0.9
        if k == 2:
            assert frac == 0.0 and got[k]["confidence"] == 0.0 and np.isnan(got[k]["T"]).all() and got[k]["summary"]["best_hypothesis"] == -1
    assert status_of(chip.ransac_record_shape, ICP, 5) == capi.CHIP_ERR_INVALID_ARG
    chip.icp_ransac(*ragged_five[1], gparams(seed=12, **kw))
    assert chip.ransac_record_shape(ICP, 0)["P"] == 1              # after a single call: problem 0 of 1
    assert status_of(chip.ransac_record_shape, ICP, 1) == capi.CHIP_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------- matched
CAND = (4, 0, 0, 2, 1, 3)
CAND_SEEDS = (21, 22, 23, 24, 25, 26)


def singles_matched(chip, sms, cand, seeds, **kw):
    out = []
    for j, s in zip(cand, seeds):
        chip.match_select(j)
        out.append(chip.icp_matched(sms[j].n_3d3d, gparams(seed=s, **kw)))
    return out


@pytest.fixture(scope="module")
def stored(five):
    """a ctx with the five-candidate case in its frame store (query: id 100, candidate j: id j)"""
    with capi.Chip(64) as c:
        c.frame_store_reserve(6, 4096)
        c.frame_put(100, five["a"])
        for j, b in enumerate(five["cands"]):
            c.frame_put(j, b)
        yield c


@pytest.mark.parametrize("path", ["host_frames", "stored_frames"])
def test_matched_batch_equals_select_and_single(stored, five, path):
    chip = stored
    match = (lambda: chip.match_batch(five["a"], five["cands"], five["Kinv"])) if path == "host_frames" else \
            (lambda: chip.match_batch_stored(100, list(range(5)), five["Kinv"]))
    sms = match()
    n33 = [sm.n_3d3d for sm in sms]
    assert min(n33) < 20 <= max(n33)                               # both sides of the 20-point gate
    for kw in (dict(), dict(n_hypotheses=65, sampler=capi.CHIP_SAMPLER_THEIA_PERSISTENT)):
        want = singles_matched(chip, sms, CAND, CAND_SEEDS, **kw)
        chip.match_select(2)
        got = chip.icp_matched_batch([(j, n33[j]) for j in CAND], gparams(seed=5, **kw), CAND_SEEDS)
        for i, (g, w) in enumerate(zip(got, want)):
            same_estimate(g, w, (path, i))
            if n33[CAND[i]] < 20:
                assert_left_out(g, n33[CAND[i]], (path, i))
        assert [g["status"] for g in got].count(0) == sum(n >= 20 for n in (n33[j] for j in CAND)) == chip.ransac_record_shape(ICP, 0)["P"]
        sets = chip.match_read_sets(sms[2])                        # the selection is what it was
        for k in SET_KEYS:
            assert sets[k].tobytes() == np.ascontiguousarray(five["mirror"][2][k]).tobytes(), k
    # no runnable problem: the enqueue succeeds, the collect delivers the left-out answers
    got = chip.icp_matched_batch([(4, n33[4]), (4, n33[4])], gparams(seed=5))
    for g in got:
        assert_left_out(g, n33[4], "nothing runnable")
    assert status_of(chip.ransac_record_shape, ICP, 0) == capi.CHIP_ERR_BUSY


def test_underneath_the_pnp_and_across_a_new_match(stored, five):
    chip = stored
    ids = list(range(5))
    sms = chip.match_batch_stored(100, ids, five["Kinv"])
    n33 = [sm.n_3d3d for sm in sms]
    icp_problems = [(j, n33[j]) for j in CAND]
    pnp_problems = []
    for j, sm in enumerate(sms):
        if sm.n_matches_gms >= 150:
            pnp_problems += [(j, capi.CHIP_SET_AB, sm.n_3d2d_ab), (j, capi.CHIP_SET_BA, sm.n_3d2d_ba)]
    pp = capi.default_ransac_params(); pp.seed = 5
    pnp_seeds = [100 + 7 * i for i in range(len(pnp_problems))]
    pnp_want = chip.pnp_matched_batch(pnp_problems, pp, pnp_seeds)
    icp_want = chip.icp_matched_batch(icp_problems, gparams(seed=5), CAND_SEEDS)
    # enqueue -> the PnP batch -> collect
    ticket = chip.icp_matched_batch_enqueue(icp_problems, gparams(seed=5), CAND_SEEDS)
    pnp_got = chip.pnp_matched_batch(pnp_problems, pp, pnp_seeds)
    icp_got = chip.icp_matched_batch_collect(ticket)
    assert len(pnp_got) == 8
    for i, (g, w) in enumerate(zip(pnp_got, pnp_want)):
        same_estimate(g, w, ("pnp", i))
    for i, (g, w) in enumerate(zip(icp_got, icp_want)):
        same_estimate(g, w, ("icp", i))
    # enqueue -> a NEW match that rewrites the slabs -> collect: the old batch's answers, and a correct match
    ticket = chip.icp_matched_batch_enqueue(icp_problems, gparams(seed=5), CAND_SEEDS)
    new = chip.match_batch_stored(100, [3, 1], five["Kinv"])
    old = chip.icp_matched_batch_collect(ticket)
    for i, (g, w) in enumerate(zip(old, icp_want)):
        same_estimate(g, w, ("across a match", i))
    for slot, j in enumerate((3, 1)):
        assert new[slot].as_dict() == five["mirror"][j]["summary"]
        chip.match_select(slot)
        sets = chip.match_read_sets(new[slot])
        for k in SET_KEYS:
            assert sets[k].tobytes() == np.ascontiguousarray(five["mirror"][j][k]).tobytes(), (j, k)
    # the same across chip_match_pair and chip_match_batch
    chip.match_batch_stored(100, ids, five["Kinv"])
    ticket = chip.icp_matched_batch_enqueue(icp_problems, gparams(seed=5), CAND_SEEDS)
    a, small, Kinv = cases.small_frames(2)
    chip.match_pair(a, small[0], Kinv, read_sets=False)
    chip.match_batch(a, small, Kinv)
    for i, (g, w) in enumerate(zip(chip.icp_matched_batch_collect(ticket), icp_want)):
        same_estimate(g, w, ("across host-frame matches", i))


def test_status_rules(five):
    A, B = R.half_inlier_icp_scene(64, 3)
    busy = capi.CHIP_ERR_BUSY
    with capi.Chip(64) as c:
        assert status_of(c.icp_matched_batch_enqueue, [(0, 64)]) == busy       # before any match
        assert status_of(c.icp_matched_batch, [(0, 64)]) == busy
        assert status_of(c.icp_matched_batch_collect, dict(Ns=[64], status=np.zeros(1, np.int32))) == busy
        a, small, Kinv = cases.small_frames(2)
        sms = c.match_batch(a, small, Kinv)
        n33 = [sm.n_3d3d for sm in sms]
        assert min(n33) >= 20
        for j in (-1, 2):
            assert status_of(c.icp_matched_batch_enqueue, [(0, n33[0]), (j, 64)]) == capi.CHIP_ERR_RANGE
        assert status_of(c.icp_matched_batch_collect, dict(Ns=[64], status=np.zeros(1, np.int32))) == busy   # nothing was enqueued
        want = c.icp_matched_batch([(1, n33[1]), (0, n33[0])], gparams(seed=4))
        # a pending batch excludes every other ICP call, and only the batch collect ends it
        ticket = c.icp_matched_batch_enqueue([(1, n33[1]), (0, n33[0])], gparams(seed=4))
        assert status_of(c.icp_matched_batch_enqueue, [(0, n33[0])]) == busy
        assert status_of(c.icp_matched_batch, [(0, n33[0])]) == busy
        assert status_of(c.icp_ransac_enqueue, A, B) == busy
        assert status_of(c.icp_ransac, A, B) == busy
        assert status_of(c.icp_ransac_batch, [(A, B)]) == busy
        assert status_of(c.icp_matched, n33[0]) == busy
        assert status_of(c.icp_ransac_collect, 64) == busy
        assert status_of(c.ransac_record_shape, ICP, 0) == busy
        for g, w in zip(c.icp_matched_batch_collect(ticket), want):
            same_estimate(g, w, "after the refusals")
        assert status_of(c.icp_matched_batch_collect, ticket) == busy
        # a pending single estimation excludes the batch
        single = c.icp_ransac(A, B, gparams(seed=4))
        c.icp_ransac_enqueue(A, B, gparams(seed=4))
        assert status_of(c.icp_matched_batch_enqueue, [(0, n33[0])]) == busy
        assert status_of(c.icp_matched_batch_collect, ticket) == busy
        assert status_of(c.icp_ransac_batch, [(A, B)]) == busy
        same_estimate(c.icp_ransac_collect(64), single, "single")
    with capi.Chip(64, devices=[0, 0]) as grp:
        assert status_of(grp.icp_matched_batch_enqueue, [(0, 64)]) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.icp_matched_batch, [(0, 64)]) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.icp_matched_batch_collect, dict(Ns=[64], status=np.zeros(1, np.int32))) == capi.CHIP_ERR_UNSUPPORTED
        same_estimate(grp.icp_ransac_batch([(A, B)], gparams(seed=4))[0], single, "group ctx: devices[0]")


def test_first_use_next_to_a_resident_scan_instance(pool, monkeypatch):
    """with CHIP_TICK_RESIDENT=1 the buffers of the first batch are reserved next to a resident scan instance, inside one pause: same bits"""
    import scenarios
    probs, seeds = pool
    with capi.Chip(64) as c:
        want = [c.icp_ransac(A, B, gparams(seed=s)) for (A, B), s in zip(probs[1:6], seeds[1:6])]
        want_grown = [c.icp_ransac(A, B, gparams(seed=s, n_hypotheses=65)) for (A, B), s in zip(probs, seeds)]
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        for l in scenarios.default_schedule(400)[:8]:
            c.loop_tick(l)
        got = c.icp_ransac_batch(probs[1:6], gparams(seed=1), seeds[1:6])
        grown = c.icp_ransac_batch(probs[0:16], gparams(seed=1, n_hypotheses=65), seeds)   # regrow: more points, more hypotheses, wider rows
        c.loop_tick(400)
    for i, (g, w) in enumerate(zip(got, want)):
        same_estimate(g, w, i)
    assert len(grown) == 16
    for i, (g, w) in enumerate(zip(grown, want_grown)):
        same_estimate(g, w, ("after the regrow", i))


def test_verify_candidates_composed_example():
    exe = LIB / "verify_candidates_composed"
    assert exe.exists()
    r = subprocess.run([str(exe), "3000", "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== the composition from single calls") == 6 and "DIFFERS" not in r.stdout
