"""Every hypothesis, every stage: the record both RANSAC kernel pairs leave per hypothesis (chip_debug_ransac_record) and what
pnp_build_solve hands to pnp_eig_score (chip_debug_pnp_stage) against the CPU record built from the oracle's stage functions
(tests/ransac_records.py; tests/test_ransac_records.py shows on the CPU that it is the right reference).

The other GPU tests of the two legs compare the WINNING hypothesis.  Here all of them are compared -- the 999 losers of a benchmark call,
the ones past the stopping point of an adaptive call, the rejected ones -- and the ones that lose are the ones that take the hard
paths (singular elimination, several or no cheirality-valid roots).  Rule: integers equal; cost and pose by bit pattern, pose NaN where
rejected; mask words equal to the packed oracle mask, the inlier count their popcount, no bit at positions >= N; the action matrix equal
as IEEE values with NaNs in the same places AND bit for bit (the device eliminates densely where the oracle skips zero multipliers, so a
+0 / -0 difference is possible in principle; assert_stage_equal counts such entries, and not one has shown up: the count is held to 0)."""
import numpy as np
import pytest

import np_mirror_pnp as M
import oracle_lib as O
import ransac_records as R
from cerebro_amd import capi, synth
from cerebro_amd.synth import make_icp_scene

pytestmark = pytest.mark.gpu
PNP, ICP = capi.CHIP_RANSAC_LEG_PNP, capi.CHIP_RANSAC_LEG_ICP
FRESH, PERSISTENT = capi.CHIP_SAMPLER_FRESH, capi.CHIP_SAMPLER_THEIA_PERSISTENT
COMPARED = dict(pnp=0, icp=0)   # hypotheses held to the oracle by this file (printed by the last test)


def gparams(leg, **kw):
    p = capi.default_ransac_params() if leg == PNP else capi.default_icp_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def pnp_every_hypothesis(chip, X, uv, what="", stage=True, **kw):
    """one call, then: stage 1 (a mismatch names it first), the full record, and the selection rule replayed over the DEVICE record"""
    p = O.ransac_params(**kw)
    g = chip.pnp_ransac(X, uv, gparams(PNP, **kw))
    dev, cpu = chip.ransac_record(PNP), R.pnp_record(X, uv, p, stage=stage)
    what = f"pnp {what} N={X.shape[0]} {kw}"
    assert (dev["P"], dev["H"], dev["N"], dev["S"], dev["words"]) == (1, cpu["H"], X.shape[0], p.sample_size, (X.shape[0] + 63) // 64), what
    assert np.array_equal(dev["sample"], cpu["sample"]), f"{what}: {R.first_difference(dev, cpu)}"
    if stage:
        assert R.assert_stage_equal(chip.pnp_stage(), cpu, what) == 0, f"{what}: action matrices differ in the sign of zeros"
    R.assert_record_equal(dev, cpu, X.shape[0], "pnp", what)
    R.same_summary(R.select(dev, X.shape[0], p), g)
    COMPARED["pnp"] += cpu["H"]
    return g, dev, cpu


def icp_every_hypothesis(chip, A, B, what="", **kw):
    p = O.icp_params(**kw)
    g = chip.icp_ransac(A, B, gparams(ICP, **kw))
    dev, cpu = chip.ransac_record(ICP), R.icp_record(A, B, p)
    what = f"icp {what} N={A.shape[0]} {kw}"
    assert (dev["P"], dev["H"], dev["N"], dev["S"], dev["words"]) == (1, cpu["H"], A.shape[0], p.sample_size, (A.shape[0] + 63) // 64), what
    assert np.array_equal(dev["valid"], cpu["valid"]), f"{what}: the ICP model (sample / Umeyama / scale gate) differs first at hypothesis " \
        f"{int(np.argmax(dev['valid'] != cpu['valid']))}"
    R.assert_record_equal(dev, cpu, A.shape[0], "icp", what)
    R.same_summary(R.select(dev, A.shape[0], p), g)
    COMPARED["icp"] += cpu["H"]
    return g, dev, cpu


@pytest.fixture()
def chip():
    with capi.Chip(64) as c:
        c.pnp_keep_stage(True)      # pnp_stage()'s Sg is what pnp_build_solve wrote, whatever pnp_eig_score did with the slot afterwards
        yield c


# ------------------------------------------------------------------------------------------------ PnP: every hypothesis, both stages
@pytest.mark.parametrize("sampler", [FRESH, PERSISTENT])
def test_pnp_config3_all_1000_hypotheses(chip, sampler):
    X, uv, _, _ = M.make_scene(N=512, outlier_frac=0.3, noise_px=0.5, seed=4242)
    g, dev, cpu = pnp_every_hypothesis(chip, X, uv, "config 3", seed=4242, n_hypotheses=1000, sampler=sampler)
    assert dev["valid"].sum() > 100 and (dev["nsol"] == 0).sum() > 500     # most hypotheses lose before they are ever scored
    pnp_every_hypothesis(chip, X, uv, "config 3", seed=4242, n_hypotheses=200, sampler=sampler, use_mle=0)


@pytest.mark.parametrize("N,outl,noise,seed", [(20, 0.0, 0.0, 1), (64, 0.1, 0.3, 2), (100, 0.3, 0.5, 3), (512, 0.3, 0.5, 4242),
                                                (777, 0.5, 1.0, 5), (3000, 0.2, 0.5, 6), (4500, 0.2, 0.5, 7)])
def test_pnp_random_scenes_both_modes(chip, N, outl, noise, seed):
    X, uv, _, _ = M.make_scene(N=N, outlier_frac=outl, noise_px=noise, seed=seed)
    g, dev, _ = pnp_every_hypothesis(chip, X, uv, seed=seed)                       # adaptive: the record covers all initial hypotheses ...
    assert dev["H"] == R.initial_iterations(O.ransac_params(seed=seed)) >= g["summary"]["n_iterations"]   # ... also those after the stop
    pnp_every_hypothesis(chip, X, uv, seed=seed + 100, n_hypotheses=200)
    pnp_every_hypothesis(chip, X, uv, seed=seed, use_mle=0, n_hypotheses=64)
    pnp_every_hypothesis(chip, X, uv, seed=seed, sampler=PERSISTENT)
    pnp_every_hypothesis(chip, X, uv, seed=seed, use_mle=0, n_hypotheses=64, sampler=PERSISTENT)


def test_pnp_adaptive_record_goes_past_the_stopping_point(chip):
    X, uv, _, _ = M.make_scene(N=512, outlier_frac=0.05, noise_px=0.3, seed=7)
    g, dev, _ = pnp_every_hypothesis(chip, X, uv, seed=7)
    assert g["summary"]["n_iterations"] < dev["H"] and dev["valid"][g["summary"]["n_iterations"]:].any()


def test_pnp_fuzz_kinds_every_hypothesis(chip):
    seen = set()
    for i, kind, X, uv in R.fuzz_scenes(3):
        for kw in (dict(n_hypotheses=60), dict(), dict(n_hypotheses=60, use_mle=0, sampler=PERSISTENT)):
            _, dev, _ = pnp_every_hypothesis(chip, X, uv, f"fuzz scene {i} kind {kind}", seed=5000 + i, **kw)
            seen |= set(np.minimum(dev["nsol"], 2).tolist())
    assert {-1, 0, 1, 2} <= seen, seen      # singular elimination, no root, the model, several roots: all met, all compared


def test_record_is_the_same_without_the_stage_copy():
    X, uv, _, _ = M.make_scene(N=100, outlier_frac=0.3, noise_px=0.5, seed=3)
    with capi.Chip(64) as c:                # keep_stage off (the default): the record is unchanged, Sg still equal where ok
        _, dev, cpu = pnp_every_hypothesis(c, X, uv, "no stage copy", stage=False, seed=3, n_hypotheses=64)
        stg = c.pnp_stage()
        assert np.array_equal(stg["ok"], R.pnp_record(X, uv, O.ransac_params(seed=3, n_hypotheses=64))["ok"])


# ------------------------------------------------------------------------------------------------ the sampler's modulo
SAMPLER_N = [20, 21, 31, 32, 33, 35, 63, 64, 65, 79, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537,
             2 ** 20, 2 ** 20 + 1]
SAMPLER_SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1]


def test_sampler_arithmetic_pnp():
    """ransac_sample_wave's x % (N - lane) at powers of two, their neighbours and large N: the device's sample table against the oracle's"""
    rng = np.random.default_rng(1)
    with capi.Chip(64) as chip:
        for N in SAMPLER_N:
            X = rng.uniform(-1, 1, (N, 3)) + [0, 0, 4.0]
            uv = X[:, :2] / X[:, 2:3] + rng.normal(0, 0.3, (N, 2))      # far off any pose: few models, the call stays short at 2^20 points
            for seed in SAMPLER_SEEDS:
                chip.pnp_ransac(X, uv, gparams(PNP, seed=seed, n_hypotheses=64))
                dev = chip.ransac_record(PNP)
                want = R.samples(O.ransac_params(seed=seed, n_hypotheses=64), N)
                assert np.array_equal(dev["sample"], want), (N, seed, int(np.argmax((dev["sample"] != want).any(axis=1))))
                assert (dev["sample"] >= 0).all() and (dev["sample"] < N).all()
                COMPARED["pnp"] += 64


def test_sampler_arithmetic_icp():
    """ransac_sample_lane's Barrett reduction (host-made floor(2^64 / d), two corrections): ICP keeps no sample table, so through the
    model of every hypothesis -- a wrong index gives another pose; up to 4097 points also cost, inliers and mask"""
    rng = np.random.default_rng(2)
    T = M.make_scene(N=20, seed=3)[2]
    with capi.Chip(64) as chip:
        for N in SAMPLER_N:
            A = rng.uniform(-2, 2, (N, 3)) + [0, 0, 5.0]
            B = A @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.05, (N, 3))
            for seed in SAMPLER_SEEDS:
                kw = dict(seed=seed, n_hypotheses=64)
                if N <= 4097:
                    icp_every_hypothesis(chip, A, B, "sampler", **kw)
                    continue
                chip.icp_ransac(A, B, gparams(ICP, **kw))
                dev = chip.ransac_record(ICP)
                for h in range(64):
                    ok, Th, _ = O.icp_hypothesis(A, B, seed, h)
                    assert dev["valid"][h] == ok, (N, seed, h)
                    if ok:
                        assert np.array_equal(R.bits(dev["T"][h]), R.bits(Th.T.reshape(16))), (N, seed, h)
                COMPARED["icp"] += 64


# ------------------------------------------------------------------------------------------------ sample_size
@pytest.mark.parametrize("S", [3, 4, 5, 8, 10, 14, 15, 16])
def test_pnp_sample_sizes(chip, S):
    """every sample size ransac_check_params accepts for PnP, held to the oracle: the wave-cooperative sampler, the lane < S loads, the
    cheirality loop over S points"""
    for N, seed in ((20, 1), (100, 3), (512, 4242)):
        X, uv, _, _ = M.make_scene(N=N, outlier_frac=0.2, noise_px=0.3, seed=seed)
        for sampler in (FRESH, PERSISTENT):
            pnp_every_hypothesis(chip, X, uv, f"S={S}", seed=seed, sample_size=S, sampler=sampler, n_hypotheses=32)
        pnp_every_hypothesis(chip, X, uv, f"S={S}", seed=seed, sample_size=S)


@pytest.mark.parametrize("S", [3, 4, 9, 10, 15, 16])
def test_icp_sample_sizes(chip, S):
    for N, seed in ((20, 1), (100, 2), (512, 11)):
        A, B, _, _ = make_icp_scene(N=N, outlier_frac=0.2, noise=0.02, seed=seed)
        for sampler in (FRESH, PERSISTENT):
            icp_every_hypothesis(chip, A, B, f"S={S}", seed=seed, sample_size=S, sampler=sampler, n_hypotheses=64)
            icp_every_hypothesis(chip, A, B, f"S={S}", seed=seed, sample_size=S, sampler=sampler)


def test_sample_size_outside_the_range_is_refused(chip):
    X, uv, _, _ = M.make_scene(N=64, outlier_frac=0.0, noise_px=0.0, seed=1)
    for S in (2, 17):
        with pytest.raises(capi.ChipError) as e:
            chip.pnp_ransac(X, uv, gparams(PNP, sample_size=S))
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED
        with pytest.raises(capi.ChipError) as e:
            chip.icp_ransac(X, X, gparams(ICP, sample_size=S))
        assert e.value.status == capi.CHIP_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ mask words
@pytest.mark.parametrize("N", [63, 64, 65, 127, 128, 4095, 4096, 4097, 4160, 8191, 8192, 8193])
def test_mask_words_of_every_row(chip, N):
    """pnp_eig_score keeps word w in lane w & 63 and stores 64 words at once when a group is full or at the last block: sizes where
    the two conditions coincide or a group holds one word, about half of the points inliers over the whole index range"""
    X, uv = R.half_inlier_pnp_scene(N, seed=N)
    _, dev, _ = pnp_every_hypothesis(chip, X, uv, "mask", stage=False, seed=N, n_hypotheses=64)
    v = dev["valid"] == 1
    assert v.sum() >= 8 and (dev["nin"][v] > 0.3 * N).any() and (dev["mask"][v][:, -1] != 0).any()
    A, B = R.half_inlier_icp_scene(N, seed=N)
    _, dev, _ = icp_every_hypothesis(chip, A, B, "mask", seed=N, n_hypotheses=64)
    assert (dev["valid"] == 1).sum() >= 8 and (dev["mask"][dev["valid"] == 1][:, -1] != 0).any()


# ------------------------------------------------------------------------------------------------ ICP: the scale gate on its boundary
@pytest.mark.parametrize("factor", R.ICP_GATE_FACTORS)
def test_icp_scale_gate_on_the_boundary(chip, factor):
    A, B = R.icp_gate_scene(factor, seed=31)
    _, dev, cpu = icp_every_hypothesis(chip, A, B, f"gate x{factor}", seed=5, n_hypotheses=500)
    assert 0.1 <= cpu["valid"].mean() <= 0.9            # some hypotheses pass and some fail: a differently rounded scale would show


def test_icp_scenes_and_degenerate_inputs_every_hypothesis(chip):
    for N, outl, noise, seed in [(20, 0.0, 0.0, 1), (100, 0.1, 0.01, 2), (400, 0.25, 0.02, 11), (1000, 0.5, 0.05, 4), (3001, 0.3, 0.02, 5)]:
        A, B, _, _ = make_icp_scene(N=N, outlier_frac=outl, noise=noise, seed=seed)
        for sampler in (FRESH, PERSISTENT):
            icp_every_hypothesis(chip, A, B, seed=seed, sampler=sampler)
            icp_every_hypothesis(chip, A, B, seed=seed + 7, n_hypotheses=300, sampler=sampler, use_mle=sampler)
    A, B, T, _ = make_icp_scene(N=200, outlier_frac=0.0, noise=0.0, seed=3)
    icp_every_hypothesis(chip, A, 0.85 * B, "all fail", seed=1)
    icp_every_hypothesis(chip, A, 1.05 * B, "all pass", seed=1)
    line = np.outer(np.arange(40.0), [1, 2, 3])
    icp_every_hypothesis(chip, line, line + 1.0, "collinear", seed=2)
    Ap = A.copy(); Ap[:, 2] = 1.0
    icp_every_hypothesis(chip, Ap, Ap @ T[:3, :3].T + T[:3, 3], "coplanar (rank 2)", seed=4, n_hypotheses=32)


# ------------------------------------------------------------------------------------------------ batched PnP, ragged
def same_record(a, b, N):
    """two DEVICE records of the same problem; a may have wider mask rows (the batch's stride): the extra words are zero"""
    w = b["mask"].shape[1]
    for k in ("valid", "nin", "nsol", "sample"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(R.bits(a["cost"]), R.bits(b["cost"])) and np.array_equal(R.bits(a["T"]), R.bits(b["T"]))
    assert np.array_equal(a["mask"][:, :w], b["mask"]) and not a["mask"][:, w:].any()


@pytest.mark.parametrize("sampler", [FRESH, PERSISTENT])
def test_batched_pnp_ragged(chip, sampler):
    Ns = [20, 4500, 64, 65, 1000, 129, 3000, 21]
    probs = [M.make_scene(N=n, outlier_frac=0.2, noise_px=0.5, seed=40 + i)[:2] for i, n in enumerate(Ns)]
    seeds = [900 + 17 * i for i in range(len(Ns))]
    p = gparams(PNP, n_hypotheses=48, sampler=sampler)
    wide = chip.pnp_ransac_batch([(M.make_scene(N=6000, seed=1)[:2])], p, seeds=[1])     # wider rows first: stale words beyond a problem's own
    rs = chip.pnp_ransac_batch(probs, p, seeds=seeds)
    recs = [chip.ransac_record(PNP, i) for i in range(len(Ns))]
    with pytest.raises(capi.ChipError) as e:
        chip.ransac_record(PNP, len(Ns))
    assert e.value.status == capi.CHIP_ERR_INVALID_ARG
    for i, (X, uv) in enumerate(probs):
        assert (recs[i]["P"], recs[i]["N"], recs[i]["words"]) == (8, Ns[i], (4500 + 63) // 64)
        p1 = gparams(PNP, n_hypotheses=48, sampler=sampler, seed=seeds[i])
        single = chip.pnp_ransac(X, uv, p1)
        same_record(recs[i], chip.ransac_record(PNP), Ns[i])
        assert single["summary"] == rs[i]["summary"]
        if Ns[i] in (20, 65, 4500):      # and against the oracle, at the batch's stride
            cpu = R.pnp_record(X, uv, O.ransac_params(n_hypotheses=48, sampler=sampler, seed=seeds[i]), words=recs[i]["words"], stage=False)
            R.assert_record_equal(recs[i], cpu, Ns[i], "pnp", f"batch problem {i}")
            COMPARED["pnp"] += 48
    # eleven problems: a launch of eight, then one of three -- the record is the last launch's
    probs11 = (probs + probs)[:11]
    seeds11 = [700 + i for i in range(11)]
    chip.pnp_ransac_batch(probs11, p, seeds=seeds11)
    assert chip.ransac_record_shape(PNP, 0)["P"] == 3
    for j in range(3):
        X, uv = probs11[8 + j]
        rec = chip.ransac_record(PNP, j)
        cpu = R.pnp_record(X, uv, O.ransac_params(n_hypotheses=48, sampler=sampler, seed=seeds11[8 + j]), words=rec["words"], stage=False)
        R.assert_record_equal(rec, cpu, X.shape[0], "pnp", f"second launch, problem {j}")
    with pytest.raises(capi.ChipError):
        chip.ransac_record(PNP, 3)


# ------------------------------------------------------------------------------------------------ no stale state, error codes
def test_no_stale_state_after_a_larger_call(chip):
    X, uv, _, _ = M.make_scene(N=4500, outlier_frac=0.2, noise_px=0.5, seed=7)
    chip.pnp_ransac(X, uv, gparams(PNP, seed=7, n_hypotheses=1000))
    assert chip.ransac_record_shape(PNP)["H"] == 1000
    X, uv, _, _ = M.make_scene(N=20, outlier_frac=0.1, noise_px=0.5, seed=2)
    _, dev, _ = pnp_every_hypothesis(chip, X, uv, "after 1000 x 4500", seed=2, n_hypotheses=16)
    assert (dev["valid"] == 0).any() and (dev["valid"] == 1).any() and dev["mask"].shape == (16, 1)
    A, B, _, _ = make_icp_scene(N=3001, outlier_frac=0.3, noise=0.02, seed=5)
    chip.icp_ransac(A, B, gparams(ICP, seed=5, n_hypotheses=500))
    A, B = R.icp_gate_scene(0.9, seed=31, N=20)
    _, dev, _ = icp_every_hypothesis(chip, A, B, "after 500 x 3001", seed=5, n_hypotheses=16)
    assert (dev["valid"] == 0).any() and (dev["valid"] == 1).any()


def test_the_aids_report_when_there_is_nothing_to_read():
    A, B, _, _ = make_icp_scene(N=100, outlier_frac=0.1, noise=0.01, seed=2)
    with capi.Chip(64) as c:
        for leg in (PNP, ICP):
            with pytest.raises(capi.ChipError) as e:
                c.ransac_record(leg)
            assert e.value.status == capi.CHIP_ERR_BUSY
        with pytest.raises(capi.ChipError) as e:
            c.pnp_stage()
        assert e.value.status == capi.CHIP_ERR_BUSY
        n = c.icp_ransac_enqueue(A, B, gparams(ICP, seed=2))
        with pytest.raises(capi.ChipError) as e:           # enqueued, not collected
            c.ransac_record(ICP)
        assert e.value.status == capi.CHIP_ERR_BUSY
        c.icp_ransac_collect(n)
        assert c.ransac_record(ICP)["N"] == 100
        for leg, problem in ((2, 0), (ICP, 1), (PNP, -1)):
            with pytest.raises(capi.ChipError) as e:
                c.ransac_record_shape(leg, problem)
            assert e.value.status in (capi.CHIP_ERR_INVALID_ARG, capi.CHIP_ERR_BUSY)
        sh = capi.RansacShape()
        import ctypes as C
        nsol = np.zeros(64, np.int32)
        assert c.lib.chip_debug_ransac_record(c.h, ICP, 0, C.byref(sh), None, None, None, None, None, capi._ptr(nsol), None) == capi.CHIP_ERR_INVALID_ARG
        assert c.lib.chip_debug_ransac_record(None, PNP, 0, C.byref(sh), None, None, None, None, None, None, None) == capi.CHIP_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ device-resident inputs
def test_matched_sets_give_the_record_of_the_host_pointer_call():
    sc = synth.make_match_scene(n_true=2000, n_outlier_a=100, n_outlier_b=100, seed=11)      # tests/test_match_gpu.py "clean_2000"
    with capi.Chip(4096) as chip:
        g = chip.match_pair(sc["a"], sc["b"], sc["Kinv"])
        s = g["summary"]
        for which, X, uv, N in ((capi.CHIP_SET_AB, g["X_ab"], g["uvn_ab"], s["n_3d2d_ab"]), (capi.CHIP_SET_BA, g["X_ba"], g["uvn_ba"], s["n_3d2d_ba"])):
            p = gparams(PNP, seed=7, n_hypotheses=64)
            chip.pnp_matched(which, N, p)
            d = chip.ransac_record(PNP)
            chip.pnp_ransac(X, uv, p)
            same_record(d, chip.ransac_record(PNP), N)
            R.assert_record_equal(d, R.pnp_record(X, uv, O.ransac_params(seed=7, n_hypotheses=64), stage=False), N, "pnp", f"matched set {which}")
            COMPARED["pnp"] += 64
        p = gparams(ICP, seed=7, n_hypotheses=64)
        chip.icp_matched(s["n_3d3d"], p)
        d = chip.ransac_record(ICP)
        R.assert_record_equal(d, R.icp_record(g["A_3d3d"], g["B_3d3d"], O.icp_params(seed=7, n_hypotheses=64)), s["n_3d3d"], "icp", "matched 3d3d")
        chip.icp_ransac(g["A_3d3d"], g["B_3d3d"], p)
        h = chip.ransac_record(ICP)
        for k in ("valid", "nin", "mask"):
            assert np.array_equal(d[k], h[k])
        assert np.array_equal(R.bits(d["cost"]), R.bits(h["cost"])) and np.array_equal(R.bits(d["T"]), R.bits(h["T"]))
        COMPARED["icp"] += 64


def test_zz_hypotheses_compared(capsys):
    with capsys.disabled():
        print(f"\n[per-hypothesis suite] hypotheses held to the oracle: PnP {COMPARED['pnp']}, ICP {COMPARED['icp']}")
