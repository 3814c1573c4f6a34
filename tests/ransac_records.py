"""The per-hypothesis RANSAC record on the CPU, built hypothesis by hypothesis from the oracle's STAGE functions (no test functions here).

The device computes a full record for every hypothesis (valid, cost, inlier count, pose, inlier mask; PnP also the solution count, the
sample and the first kernel's outputs) and chip_debug_ransac_record / chip_debug_pnp_stage copy it out; pnp_record / icp_record below
build the same arrays from orc_ransac_sample(_persistent) -> orc_*_hypothesis_sampled -> orc_*_score_model.  select() is a plain-Python
transcription of theia::Ransac::Estimate's sequential rule (ransac_common.h ransac_select + ransac_report): replayed over a CPU record
it must reproduce orc_pnp_ransac / orc_icp_ransac exactly (tests/test_ransac_records.py), replayed over a DEVICE record the summary
the call returned (tests/test_ransac_hypotheses_gpu.py)."""
import math

import numpy as np

import oracle_lib as O

def initial_iterations(p):
    """hypotheses the device computes for p (ransac_initial_iterations): all of them in benchmark mode, else the reference's first bound"""
    if p.n_hypotheses > 0:
        return p.n_hypotheses
    if p.min_inlier_ratio > 0:
        return O._bind_pnp().orc_ransac_max_iterations(p.sample_size, p.min_inlier_ratio, math.log(p.failure_probability),
                                                       p.min_iterations, p.max_iterations)
    return p.max_iterations


def pack_mask(mask, words):
    """N inlier bytes -> `words` uint64: bit i & 63 of word i >> 6 is point i (the kernels' ballot words)"""
    b = np.zeros(8 * words, dtype=np.uint8)
    pb = np.packbits(np.asarray(mask, dtype=np.uint8), bitorder="little")
    b[:pb.size] = pb
    return b.view("<u8").astype(np.uint64)


def unpack_mask(row, N):
    return np.unpackbits(np.ascontiguousarray(row, dtype="<u8").view(np.uint8), bitorder="little")[:N]


def samples(p, N, H=None):
    """[H, S] sample indices of hypotheses 0..H-1 under p.sampler"""
    H = initial_iterations(p) if H is None else H
    if p.sampler == 1:
        return O.ransac_sample_persistent(p.seed, H, N, p.sample_size)
    return np.stack([O.ransac_sample(p.seed, h, N, p.sample_size) for h in range(H)])


def _empty(H, words):
    return dict(valid=np.zeros(H, np.int32), cost=np.full(H, np.inf), nin=np.zeros(H, np.int32), T=np.full((H, 16), np.nan),
                mask=np.zeros((H, words), np.uint64))


def pnp_record(X, uv, p, words=None, stage=True):
    """every hypothesis of orc_pnp_ransac(X, uv, p) WITHOUT the stopping rule: valid, cost, nin, T[H, 16] column-major (NaN where rejected),
    mask[H, words], nsol (orc_dls_pnp: -1 singular D, -2 eigenvalue iteration gave up, else the cheirality-valid roots), sample[H, S];
    stage: ok[H], Tg[H, 27], Sg[H, 27, 27] (orc_dls_cubics / orc_dls_action_matrix; NaN where not ok)"""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    N, S, H = X.shape[0], p.sample_size, initial_iterations(p)
    words = (N + 63) // 64 if words is None else words
    r = _empty(H, words)
    r.update(nsol=np.zeros(H, np.int32), sample=samples(p, N, H), H=H, N=N, S=S, words=words)
    if stage:
        r.update(ok=np.zeros(H, np.int32), Tg=np.zeros((H, 27)), Sg=np.full((H, 27, 27), np.nan))
    for h in range(H):
        smp = r["sample"][h]
        ok, T = O.pnp_hypothesis_sampled(X, uv, p.seed, h, smp)
        sx, suv, u = X[smp], uv[smp], O.dls_linear_form(p.seed, h)
        r["nsol"][h] = O.dls_pnp(sx, suv, u, max_out=1)[0]
        assert ok == (r["nsol"][h] == 1)
        if ok:
            cost, nin, mask = O.score_model(T, X, uv, p.error_thresh, p.use_mle)
            r["valid"][h], r["cost"][h], r["nin"][h], r["T"][h], r["mask"][h] = 1, cost, nin, T.T.reshape(16), pack_mask(mask, words)
        if stage:
            Tfac, f = O.dls_cubics(sx, suv)
            rc, Sm = O.dls_action_matrix(f, u)
            r["Tg"][h] = Tfac.reshape(27)
            r["ok"][h] = 1 if rc == 0 else 0
            if rc == 0:
                r["Sg"][h] = Sm
    return r


def icp_record(A, B, p, words=None):
    """every hypothesis of orc_icp_ransac(A, B, p) without the stopping rule; `scale` is Umeyama's (NaN where it gave up before the gate)"""
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 3)
    B = np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 3)
    N, S, H = A.shape[0], p.sample_size, initial_iterations(p)
    words = (N + 63) // 64 if words is None else words
    r = _empty(H, words)
    r.update(sample=samples(p, N, H), scale=np.full(H, np.nan), H=H, N=N, S=S, words=words)
    for h in range(H):
        ok, T, r["scale"][h] = O.icp_hypothesis_sampled(A, B, p.seed, h, r["sample"][h] if p.sampler == 1 else None, S)
        if ok:
            cost, nin, mask = O.icp_score_model(T, A, B, p.error_thresh, p.use_mle)
            r["valid"][h], r["cost"][h], r["nin"][h], r["T"][h], r["mask"][h] = 1, cost, nin, T.T.reshape(16), pack_mask(mask, words)
    return r


def select(r, N, p):
    """theia::Ransac::Estimate's sequential rule over a record (ransac_select: strict '<', the first best wins, early termination unless
    n_hypotheses > 0) and what ransac_report makes of the winner: the dict chip.pnp_ransac / oracle_lib.pnp_ransac return."""
    bench = p.n_hypotheses > 0
    S, log_fail = p.sample_size, math.log(p.failure_probability)
    best_cost, best_h, n_models, max_it, it = np.finfo(np.float64).max, -1, 0, len(r["valid"]), 0
    while it < max_it:
        h, it = it, it + 1
        if not r["valid"][h]:
            continue
        n_models += 1
        if r["cost"][h] < best_cost:
            best_cost, best_h = float(r["cost"][h]), h
            if not bench:
                ratio = float(r["nin"][h]) / float(N)
                if ratio < float(S) / float(N):
                    continue
                max_it = min(max_it, O._bind_pnp().orc_ransac_max_iterations(S, ratio, log_fail, p.min_iterations, p.max_iterations))
    if best_h >= 0:
        nin = int(r["nin"][best_h])
        conf = float(np.float32(1.0 - math.pow(1.0 - math.pow(float(nin) / float(N), float(S)), float(it))))
        T, mask = r["T"][best_h].reshape(4, 4).T.copy(), unpack_mask(r["mask"][best_h], N)
    else:
        nin, conf, best_cost, T, mask = 0, 0.0, math.inf, np.full((4, 4), np.nan), np.zeros(N, np.uint8)
    return dict(status=0, confidence=conf, T=T, mask=mask,
                summary=dict(n_iterations=it, n_inliers=nin, best_hypothesis=best_h, n_models=n_models, best_cost=best_cost))


def same_summary(a, b):
    """two result dicts (select / chip.*_ransac / oracle_lib.*_ransac) agree in everything: integers, cost and pose bits, mask, confidence"""
    assert a["summary"].keys() == b["summary"].keys()
    for k in ("best_hypothesis", "n_iterations", "n_models", "n_inliers"):
        assert a["summary"][k] == b["summary"][k], (k, a["summary"], b["summary"])
    assert float(a["summary"]["best_cost"]).hex() == float(b["summary"]["best_cost"]).hex()
    assert np.array_equal(np.asarray(a["T"]).view(np.uint64), np.asarray(b["T"]).view(np.uint64)) or \
        (a["summary"]["best_hypothesis"] < 0 and np.isnan(a["T"]).all() and np.isnan(b["T"]).all())
    assert np.array_equal(a["mask"], b["mask"])
    assert a["confidence"] == b["confidence"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def first_difference(dev, cpu, stage=None, stage_cpu=None):
    """where a device record first leaves the CPU record, as text: the hypothesis and the earliest stage that differs there"""
    order = [("sample", "sampler"), ("Tg", "stage 1: cubics / translation factor"), ("ok", "stage 1: elimination status"),
             ("Sg", "stage 1: action matrix"), ("nsol", "stage 2: eigen-solve / roots / cheirality"), ("valid", "model accepted"),
             ("T", "pose"), ("mask", "scoring: mask"), ("nin", "scoring: inlier count"), ("cost", "scoring: cost")]
    d, c = dict(dev, **(stage or {})), dict(cpu, **(stage_cpu or {}))
    H = len(cpu["valid"])
    for h in range(H):
        for key, name in order:
            if key not in d or key not in c:
                continue
            x, y = np.asarray(d[key][h]), np.asarray(c[key][h])
            eq = np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)
            if not eq:
                return f"hypothesis {h}: first difference in {name} ({key}): device {x.ravel()[:6]} oracle {y.ravel()[:6]}"
    return None


def assert_record_equal(dev, cpu, N, leg="pnp", what=""):
    """the comparison rule of the per-hypothesis suite: integers equal, cost and T by bit pattern (T NaN where rejected), mask words equal,
    nin = popcount of the row, nothing at bit positions >= N"""
    msg = lambda: f"{what}: {first_difference(dev, cpu)}"   # noqa: E731
    H = len(cpu["valid"])
    assert len(dev["valid"]) == H and dev["mask"].shape == cpu["mask"].shape, (what, dev["mask"].shape, cpu["mask"].shape)
    assert np.array_equal(dev["valid"], cpu["valid"]), msg()
    assert np.array_equal(bits(dev["cost"]), bits(cpu["cost"])), msg()
    assert np.array_equal(dev["nin"], cpu["nin"]), msg()
    v = cpu["valid"].astype(bool)
    assert np.array_equal(bits(dev["T"][v]), bits(cpu["T"][v])), msg()
    assert np.isnan(dev["T"][~v]).all(), what
    assert np.array_equal(dev["mask"], cpu["mask"]), msg()
    pop = np.unpackbits(np.ascontiguousarray(dev["mask"], dtype="<u8").view(np.uint8), axis=1).sum(axis=1)
    assert np.array_equal(pop, dev["nin"]), what
    tail = np.unpackbits(np.ascontiguousarray(dev["mask"], dtype="<u8").view(np.uint8), axis=1, bitorder="little")[:, N:]
    assert not tail.any(), what
    if leg == "pnp":
        assert np.array_equal(dev["sample"], cpu["sample"]), msg()
        assert np.array_equal(dev["nsol"], cpu["nsol"]), msg()
        assert np.array_equal(dev["valid"], (dev["nsol"] == 1).astype(np.int32)), what


def assert_stage_equal(stg, cpu, what=""):
    """pnp_stage() against the stage part of pnp_record(): ok, Tg by bit pattern, Sg as IEEE values with NaNs in the same places -- and by
    bit pattern too.  Returns the number of entries that differ only in the sign of a zero (the device eliminates densely where the oracle
    skips zero multipliers); any other difference fails."""
    H = len(cpu["ok"])
    for h in range(H):
        if stg["ok"][h] != cpu["ok"][h]:
            raise AssertionError(f"{what}: hypothesis {h}: stage 1 (elimination status): device ok {stg['ok'][h]} oracle {cpu['ok'][h]}")
        if not np.array_equal(bits(stg["Tg"][h]), bits(cpu["Tg"][h])):
            raise AssertionError(f"{what}: hypothesis {h}: stage 1 (cubics / translation factor) differs")
    a, b = stg["Sg"], cpu["Sg"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: stage 1 (action matrix): NaNs in different places"
    neq = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    if neq.any():
        h = int(np.argwhere(neq)[0][0])
        raise AssertionError(f"{what}: hypothesis {h}: stage 1 (action matrix) differs in {int(neq[h].sum())} entries")
    return int((bits(a) != bits(b))[~np.isnan(a)].sum())


# ---------------------------------------------------------------- scenes shared by the CPU and the GPU file
def fuzz_scenes(per_kind=3):
    """(index, kind, X, uv) of the first per_kind scenes of each fuzz kind 0-11, drawn as scripts/gpu_pnp_fuzz.py draws them"""
    from pnp_fuzz_scenes import scene
    rng = np.random.default_rng(7)
    out = []
    for i in range(12 * per_kind):
        X, uv = scene(i, rng)
        rng.normal(0, 0.01, X.shape)   # (the fuzz's ICP part draws from the same generator)
        out.append((i, i % 12, X, uv))
    return out


def half_inlier_pnp_scene(N, seed):
    """noise about as large as the threshold: a model from any sample has roughly half of the correspondences within 0.03, spread over
    the whole index range (outliers would not do: with half of the points off, hardly a 15-point sample yields a model worth scoring)"""
    import np_mirror_pnp as M
    X, uv, _, _ = M.make_scene(N=N, outlier_frac=0.0, noise_px=0.0, seed=seed)
    return X, uv + np.random.default_rng(seed + 5).normal(0, 0.02, uv.shape)


def half_inlier_icp_scene(N, seed):
    from cerebro_amd.synth import make_icp_scene
    return make_icp_scene(N=N, outlier_frac=0.0, noise=0.065, seed=seed)[:2]


def icp_gate_scene(factor, seed, N=200, noise=0.2):
    """B scaled so that Umeyama's scale of a 10-point sample scatters around the gate min(s, 1 / s) > 0.9"""
    from cerebro_amd.synth import make_icp_scene
    A, B, _, _ = make_icp_scene(N=N, outlier_frac=0.0, noise=noise, seed=seed)
    return A, factor * B


ICP_GATE_FACTORS = (0.895, 0.899, 0.9, 0.901, 0.905, 1 / 0.905, 1 / 0.901, 1 / 0.9, 1 / 0.899, 1 / 0.895)
