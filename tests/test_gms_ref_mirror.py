"""The numpy restatement of the GMS filter (tests/np_mirror_match.py, what the gms_filter kernel is compared with byte for byte)
against the REFERENCE's own matcher, compiled unchanged from the reference tree against a stand-in OpenCV header (`make ref`:
oracle/ref_gms/, tests/gms_ref_lib.py): mask for mask.  No GPU.  Skipped only where the compiled reference is neither built nor
buildable (no reference tree); tests/golden/gms_ref.json carries its answers to such a machine.

Inputs on which the reference leaves its tables (flag != 0) take no part in any equality test: the stand-in detects the access and
stops the reference there."""
import json
from pathlib import Path

import numpy as np
import pytest

import gms_cases as G
import gms_ref_lib as R
import np_mirror_match as M

GOLDEN = Path(__file__).resolve().parent / "golden" / "gms_ref.json"
needs_ref = pytest.mark.skipif(R.load() is None, reason="oracle/_ref/libgms_ref.so is not built and there is no reference tree to build it from")


def both(c):
    ref, flag = R.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
    mir = M.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
    return ref, flag, mir


def assert_same(c, what):
    ref, flag, mir = both(c)
    assert flag == R.FLAG_NONE, f"{what}: the reference left its tables (flag {flag})"
    assert ref.dtype == mir.dtype and ref.shape == mir.shape
    bad = np.nonzero(ref != mir)[0]
    assert len(bad) == 0, f"{what}: reference and restatement differ on {len(bad)} of {len(ref)} matches, first {bad[:5]}"
    return ref


# ---------------------------------------------------------------------------------------------- the scenes of the GPU parity test
@needs_ref
@pytest.mark.parametrize("name", ["clean_2000", "full_5000_5000", "n1_lt_n2", "n1_gt_n2", "few_survivors", "all_duplicate", "wide_baseline"])
def test_scene_masks_equal_reference(name):
    from cerebro_amd import synth
    from test_match_gpu import SCENES
    sc = synth.make_match_scene(**SCENES[name])
    a, b = sc["a"], sc["b"]
    size = (a["xyz"].shape[1], a["xyz"].shape[0])
    tidx, _ = M.orb_bf_match(a["desc"], b["desc"])
    q = np.arange(len(tidx), dtype=np.int32)
    full = assert_same(dict(kp1=a["kp"], size1=size, kp2=b["kp"], size2=size, q=q, t=tidx), name)
    if name in ("clean_2000", "full_5000_5000"):
        assert full.sum() > 800
    sel = np.random.default_rng(3).permutation(len(q))[: max(1, len(q) // 2)]      # the permuted half list of test_match_gpu.py
    assert_same(dict(kp1=a["kp"], size1=size, kp2=b["kp"], size2=size, q=q[sel], t=tidx[sel]), name + " (half list)")


# ---------------------------------------------------------------------------------------------- fuzz
N_FUZZ = 2200


@needs_ref
def test_fuzz_masks_equal_reference():
    """small cases mixing smooth motions, random matches, several motions, image sizes, size1 != size2 and keypoints on and one float
    either side of every cell border of the four grids, at 0 and just below width / height"""
    compared = kept = border = two_sizes = 0
    kinds = set()
    for seed in range(N_FUZZ):
        kind, args = G.fuzz_case(seed)
        c = G.generate(kind, args)
        assert 20 <= len(c["q"]) <= 3000
        ref, flag, mir = both(c)
        if flag != R.FLAG_NONE:
            continue
        assert np.array_equal(ref, mir), (seed, kind, args, np.nonzero(ref != mir)[0][:5])
        compared += 1
        kept += int(ref.sum())
        kinds.add(kind)
        border += bool(args.get("border"))
        two_sizes += args["size1"] != args["size2"]
    assert compared >= 2000, compared                                # nearly every case is inside the reference's domain
    assert kinds == {"smooth", "random_matches", "right_on_image_edge"} and border > 500 and two_sizes > 500
    assert kept > 50 * compared                                       # and the masks are far from empty


@needs_ref
def test_every_border_value_reaches_the_reference():
    """the border cases put a keypoint ON, one float below and one float above every border of the four grids, on both sides"""
    for size in ((752, 480), (333, 217)):
        for side in size:
            v = G.border_values(side)
            cell = v.astype(np.float32) / np.float32(side) * np.float32(20)
            k = np.arange(1, 40) / 2.0
            for b in k:
                near = cell[np.abs(cell.astype(np.float64) - b) < 1e-4]
                assert (near < b).any() or (near == b).any()         # at or below the border ...
                assert (near >= b).any(), (side, b)                  # ... and at or above it
    for name in ("border_grid_752x480", "border_grid_1241x376_to_640x480", "border_grid_333x217"):
        kind, args = G.CONSTRUCTED[name]
        c = G.generate(kind, args)
        ref = assert_same(c, name)
        assert 2000 < ref.sum() < len(ref)
        for kp, size in ((c["kp1"], c["size1"]), (c["kp2"], c["size2"])):
            for a in (0, 1):
                assert np.isin(G.border_values(size[a]), kp[:, a]).all()


# ---------------------------------------------------------------------------------------------- the constructed cases
@needs_ref
@pytest.mark.parametrize("name", list(G.CONSTRUCTED))
def test_constructed_case_equals_reference(name):
    kind, args = G.CONSTRUCTED[name]
    assert_same(G.generate(kind, args), name)


def reference_or_golden(name):
    """the reference's mask of a constructed case: computed where the library is there, else the frozen one"""
    kind, args = G.CONSTRUCTED[name]
    c = G.generate(kind, args)
    if R.load() is not None:
        ref, flag = R.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
        assert flag == R.FLAG_NONE
    else:
        e = next(e for e in json.loads(GOLDEN.read_text())["cases"] if e["name"] == name)
        ref = np.unpackbits(np.frombuffer(bytes.fromhex(e["mask_hex"]), np.uint8))[: e["n"]]
    return c, ref


def kept_by_group(c, ref):
    return [int(ref[c["group"] == g].sum()) for g in range(int(c["group"].max()) + 1)]


@pytest.mark.parametrize("name", [n for n in G.CONSTRUCTED if n.startswith("tie_") and n != "tie_in_shifted_grid_only"])
def test_tie_cases_reach_the_tie_and_the_lower_column_wins(name):
    """the case really is a tie (equal counts into 2 or 3 right cells of ONE left cell), and the reference keeps the matches into the
    lowest column only -- what VerifyCellPairs' strict > from column 0 gives (gms_matcher.cpp:112-121)"""
    c, ref = reference_or_golden(name)
    x1, y1 = M.normalise(c["kp1"], *c["size1"])
    x2, y2 = M.normalise(c["kp2"], *c["size2"])
    l, r = M.cell_left(x1[c["q"]], y1[c["q"]], 1), M.cell_right(x2[c["t"]], y2[c["t"]])
    assert len(np.unique(l)) == 1
    cols, counts = np.unique(r, return_counts=True)
    assert len(cols) >= 2 and len(set(counts)) == 1
    per_group = kept_by_group(c, ref)
    assert per_group[-1] == counts[0] and not any(per_group[:-1])      # groups are listed from the highest column down
    assert (r[ref == 1] == cols[0]).all()


def pass_marks(c, grid_type):
    """what ONE grid type marks, by the restatement"""
    x1, y1 = M.normalise(c["kp1"], *c["size1"])
    x2, y2 = M.normalise(c["kp2"], *c["size2"])
    l, r = M.cell_left(x1[c["q"]], y1[c["q"]], grid_type), M.cell_right(x2[c["t"]], y2[c["t"]])
    pair = M.gms_pass(l, r)
    return (l >= 0) & (r >= 0) & (pair[np.maximum(l, 0)] == r), l, r


def test_tie_in_one_grid_type_only():
    c, ref = reference_or_golden("tie_in_shifted_grid_only")
    assert kept_by_group(c, ref) == [24, 25, 0, 25]                    # A kept (the lower column), B not, C and D kept
    ab = np.isin(c["group"], (0, 2))
    for grid_type in (1, 3):                                         # no tie there: A and B sit in different left cells, and lose them
        marks, l, r = pass_marks(c, grid_type)
        assert not marks[ab].any() and len(np.unique(l[ab])) == 2
    for grid_type in (2, 4):                                         # one left cell, 24 : 24
        marks, l, r = pass_marks(c, grid_type)
        assert len(np.unique(l[ab])) == 1 and marks[c["group"] == 0].all() and not marks[c["group"] == 2].any()


@pytest.mark.parametrize("where,numpair", [("interior", 9), ("corner", 4), ("edge", 6)])
def test_score_equal_to_the_threshold_is_kept_and_one_short_is_not(where, numpair):
    """score < thresh is strict (gms_matcher.cpp:145): 12 matches against 6 * sqrt(mean count 4) = 12.0 stay, 11 do not"""
    for variant, kept in (("equal", 12), ("short", 0)):
        c, ref = reference_or_golden(f"thresh_{variant}_{where}")
        x1, y1 = M.normalise(c["kp1"], *c["size1"])
        l = M.cell_left(x1[c["q"]], y1[c["q"]], 1)
        centre = l[c["group"] == 0][0]
        lx, ly = centre % 20, centre // 20
        hood = [(lx + dx) + 20 * (ly + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= lx + dx < 20 and 0 <= ly + dy < 20]
        assert len(hood) == numpair and np.isin(l, hood).sum() == 4 * numpair      # mean count exactly 4
        assert 6.0 * np.sqrt(np.float64(4 * numpair) / np.float64(numpair)) == 12.0
        assert (c["group"] == 0).sum() == (12 if variant == "equal" else 11)
        assert kept_by_group(c, ref)[0] == kept and ref.sum() == kept


def test_survivor_counts_around_the_150_gate_are_not_empty():
    for k in (37, 149, 150, 151):
        c, ref = reference_or_golden(f"cluster_{k}")
        assert ref.sum() == k and ref[c["group"] == 0].all()         # the cluster and nothing of the 600 random matches


def test_a_match_survives_through_a_shifted_grid_only():
    c, ref = reference_or_golden("survives_shifted_grid_only")
    assert ref.all() and len(ref) == 14
    assert not pass_marks(c, 1)[0].any() and not pass_marks(c, 3)[0].any()
    assert pass_marks(c, 2)[0].all() and pass_marks(c, 4)[0].all()


# ---------------------------------------------------------------------------------------------- the documented departure
def sentinel_case():
    """3000 matches of a smooth motion, plus:
      A  5 matches from left cell (3, 15), which holds nothing else, to a right keypoint one pixel left of the image in cell row 0:
         right index -1 + 20 * 0 = -1 -- the value mCellPairs keeps for an empty row
      B  5 matches from left cell (16, 3) to a right keypoint in cell (-2, 0): right index -2 -- the value VerifyCellPairs writes for a
         rejected row; 3 ordinary matches from the same left cell make the row non-empty, and far too weak to be accepted"""
    size = (752, 480)
    c = G.smooth(3000, 77, outlier_frac=0.0)
    keep = np.ones(3000, bool)
    x1, y1 = M.normalise(c["kp1"], *size)
    for grid_type in (1, 2, 3, 4):                                   # nothing else in the two left cells, in any grid type
        l = M.cell_left(x1, y1, grid_type)
        keep &= ~np.isin(l, (3 + 20 * 15, 16 + 20 * 3))
    kp1, kp2 = c["kp1"][keep], c["kp2"][keep]
    n0 = len(kp1)
    a1 = np.tile(G._cell_pix((3, 15), (0.25, 0.25), size), (5, 1)); a2 = np.tile([-1.0, 5.0], (5, 1))
    b1 = np.tile(G._cell_pix((16, 3), (0.25, 0.25), size), (8, 1))
    b2 = np.concatenate([np.tile([-1.5 * 752 / 20, 5.0], (5, 1)), np.tile(G._cell_pix((8, 8), (0.25, 0.25), size), (3, 1))])
    kp1 = np.concatenate([kp1, a1, b1]).astype(np.float32)
    kp2 = np.concatenate([kp2, a2, b2]).astype(np.float32)
    q = np.arange(len(kp1), dtype=np.int32)
    sentinel = np.zeros(len(q), bool)
    sentinel[n0:n0 + 10] = True
    return dict(kp1=kp1, size1=size, kp2=kp2, size2=size, q=q, t=q.copy()), sentinel


@needs_ref
def test_departure_negative_right_index_against_the_sentinels():
    """INTEGRATION.md section 6, "GMS with keypoints outside their image": the reference stays inside its tables here, skips the
    match in AssignMatchPairs (gms_matcher.cpp:92) and then finds its negative right index EQUAL to the -1 / -2 of mCellPairs (:172):
    an inlier.  The restatement (and the kernel) give such a match no cell.  They differ on exactly those matches."""
    c, sentinel = sentinel_case()
    ref, flag, mir = both(c)
    assert flag == R.FLAG_NONE
    x2, y2 = M.normalise(c["kp2"], *c["size2"])
    assert (M.cell_right(x2, y2)[sentinel] == -1).all()               # "no cell" in the restatement
    assert ref[sentinel].all() and not mir[sentinel].any()
    assert np.array_equal(ref != mir, sentinel)
    assert ref[~sentinel].sum() > 2000


@needs_ref
def test_departure_out_of_table_inputs_raise_the_flag():
    """where the reference would index its tables out of bounds only the flag is asserted: there is no answer to compare with"""
    size = (752, 480)
    base = G.smooth(500, 5, outlier_frac=0.0)

    def flag_of(side, xy):
        kp1, kp2 = base["kp1"].copy(), base["kp2"].copy()
        (kp1 if side == 1 else kp2)[7] = xy
        return R.gms_filter(kp1, size, kp2, size, base["q"], base["t"])[1]

    assert flag_of(1, base["kp1"][7]) == R.FLAG_NONE
    assert flag_of(2, (100.0, 480.0)) == R.FLAG_OUT_OF_BOUNDS        # right row 20: column 400 + x of the table
    assert flag_of(2, (752.0, 479.0)) == R.FLAG_OUT_OF_BOUNDS        # right cell (20, 19) = column 400
    assert flag_of(2, (752.0, 100.0)) == R.FLAG_NONE                 # right cell (20, 4) = column 100: aliased, inside the table
    assert flag_of(1, (100.0, 480.0)) == R.FLAG_OUT_OF_BOUNDS        # left row 20 passes grid type 2's check of x alone
    assert flag_of(1, (752.0, 450.0)) == R.FLAG_OUT_OF_BOUNDS        # left cell (20, 19) in grid type 3 (x unchecked, y shifted)
    assert flag_of(1, (np.nan, 3.0)) == R.FLAG_NOT_RUN and flag_of(2, (3.0, np.inf)) == R.FLAG_NOT_RUN
    mask, flag = R.gms_filter(base["kp1"], size, np.full_like(base["kp2"], 500.0), size, base["q"], base["t"])
    assert flag == R.FLAG_OUT_OF_BOUNDS and not mask.any()


# ---------------------------------------------------------------------------------------------- the frozen answers
def test_golden_inputs_regenerate_and_equal_the_restatement():
    """tests/golden/gms_ref.json: the generators still produce the frozen inputs (SHA-256), every constructed case is frozen, and the
    frozen reference masks are what the restatement computes (and what the compiled reference computes, where it is available)"""
    gold = json.loads(GOLDEN.read_text())
    names = [e["name"] for e in gold["cases"]]
    assert set(G.CONSTRUCTED) <= set(names) and len(names) == len(set(names)) and len(names) >= 40
    for e in gold["cases"]:
        c = G.generate(e["kind"], e["args"])
        assert G.digest(c) == e["sha256"], e["name"]
        assert len(c["q"]) == e["n"]
        want = np.unpackbits(np.frombuffer(bytes.fromhex(e["mask_hex"]), np.uint8))[: e["n"]]
        assert int(want.sum()) == e["n_inliers"]
        assert np.array_equal(M.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"]), want), e["name"]
        if R.load() is not None:
            ref, flag = R.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
            assert flag == R.FLAG_NONE and np.array_equal(ref, want), e["name"]
        if e["name"] in G.CONSTRUCTED:
            assert (e["kind"], e["args"]) == (G.CONSTRUCTED[e["name"]][0], json.loads(json.dumps(G.CONSTRUCTED[e["name"]][1]))), e["name"]
