"""The numpy restatement of GMS with scale / rotation (tests/np_mirror_gms_modes.py, what gms_grid_modes + gms_mode_select are compared
with byte for byte) against the REFERENCE's own matcher called with the other flag pairs: frozen in tests/golden/gms_modes_ref.json
and, where the compiled reference is there (`make ref_modes`: tests/ref_gms_modes/, tests/gms_modes_ref_lib.py), live.  No GPU.

A case takes no part in a comparison only if the reference reports that it left its tables; that share is capped."""
import json
from pathlib import Path

import numpy as np
import pytest

import gms_cases as G
import gms_mode_cases as MC
import gms_modes_ref_lib as R
import np_mirror_gms_modes as MM
import np_mirror_match as M
from cerebro_amd import synth

GOLDEN = Path(__file__).resolve().parent / "golden" / "gms_modes_ref.json"
needs_ref = pytest.mark.skipif(R.load() is None, reason="oracle/_ref/libgms_ref_modes.so is not built and there is no reference tree to build it from")
N_FUZZ = 300
MAX_EXCLUDED = 0.10


@pytest.fixture(scope="module")
def gold():
    return {e["name"]: e for e in json.loads(GOLDEN.read_text())["cases"]}


def mirror(c, modes):
    return MM.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], modes)


def check_choice(mask, ch, modes):
    """the choice record is consistent with the rule: the first hypothesis, scales ascending and rotations inside, with the strictly
    largest count; untried combinations -1; nothing chosen iff every count is 0"""
    S, Rn = (5 if modes & 1 else 1), (8 if modes & 2 else 1)
    counts = ch["counts"]
    assert counts.shape == (5, 8) and (counts[:S, :Rn] >= 0).all()
    untried = np.ones((5, 8), bool); untried[:S, :Rn] = False
    assert (counts[untried] == -1).all()
    flat = counts[:S, :Rn].reshape(-1)
    assert ch["n_inliers"] == flat.max() == int(mask.sum())
    if flat.max() == 0:
        assert (ch["scale"], ch["rotation"]) == (-1, 0) and not mask.any()
    else:
        k = int(np.argmax(flat))                                     # the FIRST maximum in walking order
        assert (ch["scale"], ch["rotation"]) == (k // Rn, k % Rn + 1)


# ---------------------------------------------------------------------------------------------- the frozen answers
def test_golden_holds_every_case_and_no_case_is_excluded(gold):
    assert list(gold) == list(MC.CASES)
    for name, e in gold.items():
        assert (e["kind"], e["args"]) == (MC.CASES[name][0], json.loads(json.dumps(MC.CASES[name][1]))), name
        assert [(a["with_scale"], a["with_rotation"]) for a in e["answers"]] == list(MC.FLAG_PAIRS)
    assert "right_x_equals_width" not in gold and set(G.CONSTRUCTED) - {"right_x_equals_width"} <= set(gold)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_restatement_equals_the_frozen_reference(gold, name):
    e = gold[name]
    c = MC.generate(e["kind"], e["args"])
    assert G.digest(c) == e["sha256"] and len(c["q"]) == e["n"]
    for a in e["answers"]:
        modes = MC.modes_of(a["with_scale"], a["with_rotation"])
        want = np.unpackbits(np.frombuffer(bytes.fromhex(a["mask_hex"]), np.uint8))[: e["n"]]
        assert int(want.sum()) == a["n_inliers"]
        mask, ch = mirror(c, modes)
        assert np.array_equal(mask, want), (name, modes, np.nonzero(mask != want)[0][:5])
        assert ch["n_inliers"] == a["n_inliers"]
        assert a["mask_size"] == (e["n"] if a["n_inliers"] else 0)   # the reference leaves the vector untouched iff nothing is chosen
        check_choice(mask, ch, modes)
        if R.load() is not None:
            ref, cnt, size, flag = R.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], a["with_scale"], a["with_rotation"])
            assert flag == R.FLAG_NONE and np.array_equal(ref, want) and (cnt, size) == (a["n_inliers"], a["mask_size"]), (name, modes)


def test_modes_zero_is_the_plain_restatement():
    for name in ("rotate_90", "cluster_150", "thresh_short_corner", "smooth_n1025"):
        c = MC.generate(*MC.CASES[name])
        mask, ch = mirror(c, 0)
        plain = M.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
        assert np.array_equal(mask, plain)
        assert (ch["scale"], ch["rotation"], ch["n_inliers"], ch["counts"][0, 0]) == (0, 1, int(plain.sum()), int(plain.sum()))
        assert (ch["counts"].reshape(-1)[1:] == -1).all()


# ---------------------------------------------------------------------------------------------- what the cases were built for
def test_synthetic_motions_pick_their_hypothesis(gold):
    """a rotation by k * 45 degrees is found by rotation type 1 + (8 - k) % 8 ... or its neighbour on the ring; what matters here: the
    plain form loses the scene and the mode keeps it, at the scale / rotation of the motion"""
    for k in range(2, 7):
        e = gold[f"rotate_{45 * k}"]
        c = MC.generate(e["kind"], e["args"])
        assert M.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"]).sum() == 0
        mask, ch = mirror(c, MM.WITH_ROTATION)
        assert ch["n_inliers"] > 2000 and ch["scale"] == 0 and ch["rotation"] == 1 + (8 - k) % 8, (k, ch)
    # a zoom by z spreads a left 3 x 3 neighbourhood over z times as many right cells: the right grid with ratio 1 / z fits it
    for name, scale in (("zoom_2", 1), ("zoom_half", 4)):
        c = MC.generate(*MC.CASES[name])
        mask, ch = mirror(c, MM.WITH_SCALE)
        assert (ch["scale"], ch["rotation"]) == (scale, 1) and ch["n_inliers"] > 2000, (name, ch)
        assert ch["counts"][scale, 0] > ch["counts"][0, 0]
    for name in ("zoom_sqrt2", "zoom_inv_sqrt2"):
        mask, ch = mirror(MC.generate(*MC.CASES[name]), MM.WITH_SCALE)
        assert ch["n_inliers"] > 2000 and ch["n_inliers"] >= ch["counts"][0, 0]
    mask, ch = mirror(MC.generate(*MC.CASES["rotate_90_zoom_2"]), 3)
    assert (ch["scale"], ch["rotation"]) == (1, 7) and ch["n_inliers"] > 2000


def test_all_rotations_tie_and_the_first_hypothesis_wins():
    mask, ch = mirror(MC.generate(*MC.CASES["single_pair_interior"]), 3)
    assert (ch["counts"] == 40).all() and (ch["scale"], ch["rotation"], ch["n_inliers"]) == (0, 1, 40) and mask.all()


@pytest.mark.parametrize("where,spec,numpairs", [("corner", MC.CORNER, [4] * 8), ("edge", MC.EDGE, [6, 5, 4, 3, 3, 3, 4, 5])])
def test_score_equals_the_threshold_under_one_rotation_only(where, spec, numpairs):
    """numpair and the count sum are over the pairs that remain under the rotation: 12 against 6 * sqrt(mean count 4) = 12.0 under the
    case's rotation type, a larger threshold under every other; one match short fails everywhere"""
    left, right, rot = spec
    assert [len(MC.remaining_pairs(left, right, r)) for r in range(1, 9)] == numpairs
    c = MC.generate(*MC.CASES[f"{where}_equal_r{rot}"])
    x1, y1 = M.normalise(c["kp1"], *c["size1"])
    l = M.cell_left(x1[c["q"]], y1[c["q"]], 1)
    cnt = np.bincount(l, minlength=400)
    for r in range(1, 9):
        cells = [a + 20 * b for (a, b), _ in MC.remaining_pairs(left, right, r)]
        thresh = 6.0 * np.sqrt(np.float64(cnt[cells].sum()) / np.float64(len(cells)))
        assert (thresh == 12.0) == (r == rot) and thresh >= 12.0, (r, thresh)
    for modes in (2, 3):
        mask, ch = mirror(c, modes)
        assert (ch["rotation"], ch["n_inliers"]) == (rot, 12) and mask[c["group"] == 0].all()
        assert (ch["counts"][0, :8] == np.where(np.arange(1, 9) == rot, 12, 0)).all()
        for s in range(5 if modes & 1 else 1):                       # the right cell is a corner / on the edge of the 10 x 10 and 40 x 40 grids too
            assert ch["counts"][s, rot - 1] == 12
    assert mirror(c, 1)[1]["n_inliers"] == 0 and mirror(c, 0)[1]["n_inliers"] == 0
    short = MC.generate(*MC.CASES[f"{where}_short_r{rot}"])
    assert mirror(short, 3)[1]["n_inliers"] == 0


@pytest.mark.parametrize("name", MC.NO_CHOICE)
def test_nothing_to_choose(gold, name):
    c = MC.generate(*MC.CASES[name])
    for a in gold[name]["answers"]:
        assert (a["n_inliers"], a["mask_size"]) == (0, 0)
        mask, ch = mirror(c, MC.modes_of(a["with_scale"], a["with_rotation"]))
        assert not mask.any() and (ch["scale"], ch["rotation"], ch["n_inliers"]) == (-1, 0, 0)


# ---------------------------------------------------------------------------------------------- the feature: a rolled candidate survives
ROLLED = dict(n_true=2400, n_outlier_a=80, n_border=16, seed=21, n_outlier_b=100)


@pytest.fixture(scope="module")
def rolled_90():
    sc = synth.make_match_scene(roll_deg=90.0, **ROLLED)
    a, b = sc["a"], sc["b"]
    tidx, _ = M.orb_bf_match(a["desc"], b["desc"])
    size = (a["xyz"].shape[1], a["xyz"].shape[0])
    return dict(kp1=a["kp"], size1=size, kp2=b["kp"], size2=size, q=np.arange(len(tidx), dtype=np.int32), t=tidx)


def test_rolled_candidate_passes_the_150_gate_only_with_rotation(rolled_90):
    """Cerebro.cpp:1487 rejects a candidate with fewer than 150 GMS matches: the plain form keeps none of this revisit"""
    c = rolled_90
    assert M.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"]).sum() < 150
    mask, ch = mirror(c, MM.WITH_ROTATION)
    assert ch["n_inliers"] >= 150 and (ch["scale"], ch["rotation"]) == (0, 7)
    mask, ch = mirror(c, 3)
    assert ch["n_inliers"] >= 150 and ch["rotation"] == 7
    assert mirror(c, MM.WITH_SCALE)[1]["n_inliers"] < 150


def test_roll_zero_leaves_the_scene_byte_identical():
    a, b = synth.make_match_scene(**ROLLED), synth.make_match_scene(roll_deg=0.0, **ROLLED)
    for f in ("a", "b"):
        for k in ("desc", "kp", "xyz"):
            assert a[f][k].tobytes() == b[f][k].tobytes()
    assert a["T"].tobytes() == b["T"].tobytes()
    r = synth.make_match_scene(roll_deg=90.0, **ROLLED)
    assert abs(r["T"][1, 0]) > 0.99 and np.allclose(r["T"][:3, :3] @ r["T"][:3, :3].T, np.eye(3))


@needs_ref
def test_rolled_scenes_equal_the_reference(rolled_90):
    for ws, wr in MC.FLAG_PAIRS:
        c = rolled_90
        ref, cnt, size, flag = R.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], ws, wr)
        mask, ch = mirror(c, MC.modes_of(ws, wr))
        assert flag == R.FLAG_NONE and np.array_equal(ref, mask) and cnt == ch["n_inliers"]


# ---------------------------------------------------------------------------------------------- fuzz against the compiled reference
@needs_ref
@pytest.mark.parametrize("pair", MC.FLAG_PAIRS)
def test_fuzz_equals_the_reference(pair):
    ws, wr = pair
    modes = MC.modes_of(ws, wr)
    excluded, kinds, kept = [], set(), 0
    for seed in range(N_FUZZ):
        kind, args = G.fuzz_case(seed)
        c = G.generate(kind, args)
        ref, cnt, size, flag = R.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], ws, wr)
        mask, ch = mirror(c, modes)                                  # the restatement answers on every input
        check_choice(mask, ch, modes)
        if flag != R.FLAG_NONE:
            excluded.append(kind)
            continue
        assert np.array_equal(ref, mask) and cnt == ch["n_inliers"], (seed, kind, args, np.nonzero(ref != mask)[0][:5])
        assert size == (len(mask) if cnt else 0)
        kinds.add(kind)
        kept += cnt
    assert len(excluded) <= MAX_EXCLUDED * N_FUZZ, len(excluded)
    assert set(excluded) <= {"right_on_image_edge"}                  # x = width aliases past the last row of the 10- and 14-cell grids
    if not ws:
        assert not excluded
    assert kinds >= {"smooth", "random_matches"} and kept > 50 * N_FUZZ


@needs_ref
def test_right_x_equals_width_is_outside_the_reference_under_scale_only():
    c = G.generate(*G.CONSTRUCTED["right_x_equals_width"])
    flags = {p: R.gms_filter_modes(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], *p)[3] for p in MC.FLAG_PAIRS}
    assert flags == {(0, 1): R.FLAG_NONE, (1, 0): R.FLAG_OUT_OF_BOUNDS, (1, 1): R.FLAG_OUT_OF_BOUNDS}
    for modes in (1, 2, 3):
        mask, ch = mirror(c, modes)
        check_choice(mask, ch, modes)
        assert ch["n_inliers"] > 1000
