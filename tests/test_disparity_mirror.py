"""CPU checks of the numpy restatement of the disparity -> 3-D step (tests/np_mirror_disparity.py) and of its case set
(tests/disparity_cases.py): the restatement against exact rational arithmetic with an explicit round-to-nearest-even at every rounding
point of the reference's expression, the inputs against the two float shortcuts they must catch, the searched gate-edge Qs, records
against the gather from the dense image, and the properties of the pair set made from disparities."""
from fractions import Fraction

import numpy as np
import pytest

import disparity_cases as DC
import frame_store_cases as fc
import np_mirror_disparity as D
import np_mirror_frame_store as S
import np_mirror_match as M

F = np.float32


# ---------------------------------------------------------------------------------------------- exact arithmetic, rounded by hand
def rne(x: Fraction, p: int, emin: int, emax: int) -> Fraction:
    """x rounded to the nearest binary floating-point number of p significant bits, exponents emin..emax, ties to even; subnormals
    have the spacing of emin.  An overflow is not a case here."""
    if x == 0:
        return x
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - p + 1)
    n, r = divmod(a / quantum, 1)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    out = n * quantum
    assert out < Fraction(2) ** (emax + 1), "overflow"
    return out if x > 0 else -out


def r32(x): return rne(Fraction(x), 24, -126, 127)
def r64(x): return rne(Fraction(x), 53, -1022, 1023)


def exact_point(d: float, j: int, i: int, Q) -> tuple:
    """CameraGeometry.cpp:494-498,511,520-522 on Fractions; d is a float32 value"""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    q03, q13, q23, q32, q33 = (r32(Fraction(float(Q[r, c]))) for r, c in ((0, 3), (1, 3), (2, 3), (3, 2), (3, 3)))
    t = r64(Fraction(d) / 16)
    t = r64(t * q32)
    t = r64(t + q33)
    t = r64(t + Fraction(1e-6))                   # the double nearest to 1e-6
    pw = r32(r64(1 / t))
    return r32(r32(Fraction(j) + q03) * pw), r32(r32(Fraction(i) + q13) * pw), r32(q23 * pw)


def bits(x) -> int:
    return int(np.asarray(x, np.float32).view(np.uint32))


GATE = {name: (Q, d) for name, Q, d, _ in DC.gate_edge_qs()}
DOZEN = ((1, 0, 0, DC.Q_EUROC), (16, 751, 479, DC.Q_EUROC), (269, 367, 248, DC.Q_EUROC), (32767, 5, 7, DC.Q_EUROC),
         (-16, 10, 20, DC.Q_EUROC), (-32768, 751, 0, DC.Q_EUROC), (33, 368, 249, DC.Q_Q33), (-5, 0, 479, DC.Q_Q33),
         (1023, 100, 100, DC.Q_Q33), (0, 3, 4, DC.Q_Q33), (100.5, 700, 13, DC.Q_EUROC), (1e-3, 1, 1, DC.Q_EUROC),
         (GATE["lo"][1], 12, 34, GATE["lo"][0]), (GATE["hi_above"][1], 750, 478, GATE["hi_above"][0]))


@pytest.mark.parametrize("k", range(len(DOZEN)))
def test_restatement_equals_exact_arithmetic_rounded_at_the_reference_points(k):
    d, j, i, Q = DOZEN[k]
    d = F(d)
    want = exact_point(float(d), j, i, Q)
    got = D.points(d, j, i, Q)
    assert [bits(v) for v in got] == [bits(F(float(v))) for v in want], (d, j, i, [float(v) for v in want], got)
    for v in want:
        assert Fraction(float(F(float(v)))) == v                       # the expected values are float32 numbers
    img = np.full((i + 1, j + 1), d, F)                                # ... and the dense image has them at (i, j)
    assert [bits(v) for v in D.xyz_from_disparity(img, Q)[i, j]] == [bits(v) for v in got]


def test_zero_disparity_without_q33_is_the_reciprocal_of_1e_6():
    p = D.points(F(0), 0, 0, DC.Q_EUROC)                               # pw = (float)(1.0 / 1e-6): the reason the reference adds it
    assert bits(p[2]) == bits(F(458.654) * F(1.0 / 1e-6)) and np.isfinite(p).all()


# ---------------------------------------------------------------------------------------------- the inputs bite
def test_all_int16_disparities_catch_both_float_shortcuts_inside_the_gate():
    d = np.arange(-32768, 32768).astype(np.int16)
    assert len(np.unique(DC.all_int16_image())) == 65536
    z = D.points(D.as_float(d), 0, 0, DC.Q_EUROC)[:, 2]
    gate = M.depth_ok(z)
    assert 4000 < gate.sum() < 65536                                   # the gate keeps a few thousand disparities and drops the rest
    for variant in ("f32_sum", "f32_div"):
        zv = D.points(D.as_float(d), 0, 0, DC.Q_EUROC, variant)[:, 2]
        differs = z.view(np.uint32) != zv.view(np.uint32)
        print(variant, "differs in", int(differs.sum()), "of 65536,", int((differs & gate).sum()), "inside the gate")
        assert differs.sum() > 10000 and (differs & gate).sum() > 100, variant


# ---------------------------------------------------------------------------------------------- the gate-edge Qs
def test_gate_edge_qs_have_the_six_properties_they_were_searched_for():
    found = DC.gate_edge_qs()
    assert [name for name, *_ in found] == ["lo_below", "lo", "lo_above", "hi_below", "hi", "hi_above"]
    lo, hi = F(0.1), F(25.0)
    want = dict(lo_below=bits(lo) - 1, lo=bits(lo), lo_above=bits(lo) + 1, hi_below=bits(hi) - 1, hi=bits(hi), hi_above=bits(hi) + 1)
    for name, Q, d, target in found:
        assert -32768 <= d <= 32767 and float(F(Q[2, 3])) == Q[2, 3]
        z = D.points(F(np.int16(d)), 3, 5, Q)[2]
        assert bits(z) == bits(target) == want[name], name
        assert bool(M.depth_ok(z)) == DC.GATE_PASSES[name], name
        assert bits(exact_point(float(d), 3, 5, Q)[2].__float__()) == want[name], name
    assert [DC.GATE_PASSES[n] for n, *_ in found] == [False, True, True, True, True, False]


# ---------------------------------------------------------------------------------------------- records
@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_records_equal_the_gather_from_the_restated_image(kind):
    rng = np.random.default_rng(7)
    w, h = fc.W, fc.H
    disp = rng.integers(-64, 2048, (h, w)).astype(np.int16) if kind == "s16" else rng.uniform(-4, 2048, (h, w)).astype(F)
    kp = np.concatenate([fc.BORDER_KP, np.stack([rng.uniform(-2, w + 2, 200), rng.uniform(-2, h + 2, 200)], axis=1).astype(F)])
    assert {(-0.5, 3.0), (-1.0, 3.0), (w - 0.5, 3.0), (float(w), 3.0)} <= {tuple(map(float, p)) for p in kp} and np.isnan(kp[4, 0])
    for _, Q in DC.all_qs()[:2]:
        rec = D.records(kp, disp, Q)
        want = S.gather(kp, D.xyz_from_disparity(disp, Q))
        assert rec.tobytes() == want.tobytes()
        assert tuple(rec[:10, 3] != 0) == fc.BORDER_INSIDE
        assert not rec[rec[:, 3] == 0].any() and 0 < (rec[:, 3] == 0).sum() < len(kp)


# ---------------------------------------------------------------------------------------------- the pair set from disparities
def test_disparity_frames_are_what_the_case_set_says():
    f, g = DC.frames(), DC.PC.frames()
    for name in DC.NAMES:
        disp, xyz = f[name]["disp"], g[name]["xyz"]
        assert disp.dtype == np.int16 and disp.shape == xyz.shape[:2]
        assert (disp[xyz[:, :, 2] == 0] == DC.INVALID).all()
    z = D.points(F(DC.INVALID), 0, 0, DC.Q_PAIRS)[2]
    assert z < 0 and not M.depth_ok(z)                                 # the invalid value is dropped by the depth gate
    a = f["A"]["disp"]
    assert (a != DC.INVALID).sum() >= 1000 and a.max() < 1024


def test_the_pair_set_keeps_its_properties_on_disparities():
    m = DC.mirror(0)
    gms = tuple(r["summary"]["n_matches_gms"] for r in m)
    sets = tuple((r["summary"]["n_3d2d_ab"], r["summary"]["n_3d2d_ba"], r["summary"]["n_3d3d"]) for r in m)
    assert gms == DC.EXPECTED_GMS and sets == DC.EXPECTED_SETS
    assert sum(g >= 150 and min(s) >= 20 for g, s in zip(gms, sets)) >= 3
    assert sum(min(s) < 20 for s in sets) >= 1
    assert any(len(set(s)) > 1 for s in sets)                          # a pair whose three sets differ in size


def test_records_at_the_keypoints_give_the_sets_of_the_dense_image_for_every_pair():
    for pair, img in zip(DC.PAIRS, DC.mirror(0)):
        rec = DC.mirror_records(pair)
        assert rec["summary"] == img["summary"], pair
        for k in DC.SET_KEYS + ("train_idx", "distance", "inlier"):
            if k in img or k in rec:
                a, b = np.ascontiguousarray(rec[k]), np.ascontiguousarray(img[k])
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (pair, k)
