"""GPU tests of tick_rescore's decision (cerebro_amd/csrc/kernels.hip) on crafted lists, for the four-tick and the five-tick
pass alike.  Every query is the one-hot row e_0 and every other row is x e_0: the pass's score of a row, staged as fp16 or not, and its exact
score are both exactly x, so a test places scores at will (background: x = -1; all |x| <= 1, so row 0, appended first, fixes the norm bound
and with it E).  What is pinned, each against the list-driven model of tests/np_mirror_rescore.py AND as an explicit expectation:
  * M < thr is strict: eight rows of score m in a workgroup that dropped something, m the largest fp32 below thr -> certified, the smallest
    fp32 at or above it -> not; and, for a norm bound and a G at which the kernel's threshold is itself an fp32 value, m == thr -> not;
  * the cap: 32 candidates certify, 33 do not;
  * ownership: a workgroup counts as having dropped something exactly from the prefix at which it owns K + 1 rows, with prefixes that end
    just below, at and just above its share -- in the second lap of the row map, in the first (the clamp of `part` from above) and in the
    third (the clamp from below);
  * windows in which some ticks certify and some do not: the counter of ticks run again alone moves by the model's count.
In every case (pass_checks.check_window): certificate words and exact lists equal the model's, every record equals the tick issued alone and
what topk_merge gives on the exact lists read back."""
import numpy as np
import pytest

import test_prefilter_bound as pb
from cerebro_amd import capi
from pass_checks import TICKS, check_window
from test_prefilter_gpu import make_chip

pytestmark = pytest.mark.gpu
D, K = 1024, 8
G_TOP = np.float32(0.9)                                # score of the planted top eight
M_HI = np.nextafter(G_TOP, np.float32(0))              # a score below G and far above G - 2 E

_GEOM = {}


def geometry(family):
    """(grid, wpb) of the pass on this device, from the function the launch sizes itself with (check_window compares with the launch)"""
    if family not in _GEOM:
        with capi.Chip(D) as c:
            n_cus = c.info()["n_cus"]
        plan = (capi.prefilter_plan if family == "prefilter" else capi.halfq_plan)(D, n_cus=n_cus)
        _GEOM[family] = (plan["grid"], plan["block"] // 64)
        assert plan["grid"] >= 64 and plan["block"] // 64 == K      # the layouts below: shares of eight rows, workgroups up to 45
    return _GEOM[family]


def rows_of(x):
    db = np.zeros((len(x), D), np.float32)
    db[:, 0] = x
    return db


def crafted(monkeypatch, family, n, w, fill, n0=1.0):
    """a chip over n rows x e_0, background x = -n0 (n0 >= 1: the largest norm).  Row 0 is appended first; fill(x, E) then places the scores, E
    being the bound of a pass over rows of that norm.  The query rows of the window w (rows k + 47 .. k + 49 of every prefix k) are e_0
    itself and lie beyond every prefix of w."""
    n0 = np.float32(n0)
    x = np.full(n, -n0, np.float32)
    span = [k + 50 - 1 - i for k in w for i in range(3)]
    assert min(span) >= max(w) and max(span) < n and n0 >= 1
    chip = make_chip(monkeypatch, D, rows_of(x[:1]))
    norm_max = chip.info()["row_norm_max"]
    assert float(n0) <= norm_max <= float(n0) * (1.0 + 1e-6)
    E = capi.halfq_bound(D, norm_max)[1] if family == "halfq" else pb.error_bound(D, norm_max)
    fill(x, E)
    assert x[0] == -n0 and (x[span] == -n0).all()
    x[span] = 1.0
    assert np.abs(x).max() == n0
    chip.append_f32(rows_of(x[1:]))
    assert chip.info()["row_norm_max"] == norm_max
    return chip, rows_of(x)


def plant_top(x, wpb, b0=10, g=G_TOP):
    """the top eight, one row in each of eight workgroups, in the first lap of the row map"""
    for b in range(b0, b0 + 8):
        x[b * wpb] = g


def tick_certs(res):
    return [int(all(q["cert"] == 1 for q in tick)) for tick in res]


@pytest.mark.parametrize("family", ["prefilter", "halfq"])
def test_m_below_threshold_is_strict(monkeypatch, family):
    grid, wpb = geometry(family)
    tw, T = grid * wpb, TICKS[family]
    b1, b2 = 40, 43                                    # their shares of the first lap hold eight rows of score m each: below thr in b1, at it in b2
    kA, kB = tw + b1 * wpb + 4, tw + b2 * wpb + 4      # prefix kA: b1 owns 12 rows (dropped some), b2 owns 8 (dropped none); prefix kB: both dropped some
    w = [kA, kB, kA + 1, kB + 1, kB + 2][:T]
    m = {}

    def fill(x, E):
        thr = np.float64(G_TOP) - 2.0 * np.float64(E)
        thr = thr - abs(thr) * 2.0 ** -51
        f = np.float32(thr)
        below, at = (np.nextafter(f, np.float32(-1)), f) if np.float64(f) >= thr else (f, np.nextafter(f, np.float32(1)))
        assert np.float64(below) < thr <= np.float64(at) and np.nextafter(below, np.float32(1)) == at and at < G_TOP
        plant_top(x, wpb)
        x[b1 * wpb:(b1 + 1) * wpb] = below
        x[b2 * wpb:(b2 + 1) * wpb] = at
        m.update(below=float(below), at=float(at))

    chip, db = crafted(monkeypatch, family, kB + 60, w, fill)
    with chip:
        _, lp, res = check_window(chip, db, w, family, expect_cert=[1, 0, 1, 0, 0][:T])
        for t, k in enumerate(w):
            r = res[t][0]
            assert r["G"] == float(G_TOP) and m["below"] < r["thr"] <= m["at"], (r["thr"], m)       # the kernel's own threshold lies between the two
            assert r["M"] == (m["below"] if k < kB else m["at"]) and r["dropped"], (t, r["M"], m)
            assert len(r["R"]) == 16                                                               # the top eight and the eight rows at the threshold


# M == thr exactly.  thr = fl(t - fl(|t| 2^-51)), t = fl(G - 2 E), is a 53-bit number whose low bits are E's, and a pass score has 24: the two are
# equal only where E's bits allow it.  E is a function of the norm bound alone, so a search over the fp32 values n0 of the largest norm
# (norm bound = n0 (1 + 2^-30)) and over G, with the library's own evaluation order of E / E_h, finds such pairs: for these (n0, G) the
# kernel's threshold IS the fp32 value `thr` below.  (Should the evaluation of the bound ever change, the assertion on r["thr"] says so and
# the constants have to be searched again.)
EQUAL = {"prefilter": dict(n0="0x1.35aacp+0", G="-0x1.8p-36", thr="-0x1.76a15cp-12"),
         "halfq": dict(n0="0x1.aab284p+4", G="0x1.19999ap-13", thr="-0x1.bc7e6ep-1")}


@pytest.mark.parametrize("family", ["prefilter", "halfq"])
def test_m_equal_to_threshold_does_not_certify(monkeypatch, family):
    grid, wpb = geometry(family)
    tw, T = grid * wpb, TICKS[family]
    n0, g, thr = (np.float32(float.fromhex(EQUAL[family][a])) for a in ("n0", "G", "thr"))
    assert all(float(v).hex() == float.fromhex(EQUAL[family][a]).hex() for v, a in ((n0, "n0"), (g, "G"), (thr, "thr")))     # fp32 values, all three
    below = np.nextafter(thr, np.float32(-np.inf))
    b1, b2 = 40, 43                                    # as in test_m_below_threshold_is_strict: `below` in b1's first-lap share, thr itself in b2's
    kA, kB = tw + b1 * wpb + 4, tw + b2 * wpb + 4
    w = [kA, kB, kA + 1, kB + 1, kB + 2][:T]

    def fill(x, E):
        plant_top(x, wpb, g=g)
        x[b1 * wpb:(b1 + 1) * wpb] = below
        x[b2 * wpb:(b2 + 1) * wpb] = thr

    chip, db = crafted(monkeypatch, family, kB + 60, w, fill, n0=n0)
    with chip:
        _, lp, res = check_window(chip, db, w, family, expect_cert=[1, 0, 1, 0, 0][:T])
        for t, k in enumerate(w):
            r = res[t][0]
            assert r["G"] == float(g) and r["thr"] == float(thr), (r["G"], float(r["thr"]).hex(), EQUAL[family])     # the kernel's threshold is that fp32 value
            assert r["M"] == (float(below) if k < kB else float(thr)) and r["dropped"] and len(r["R"]) == 16, (t, r["M"], len(r["R"]))


@pytest.mark.parametrize("family", ["prefilter", "halfq"])
def test_candidate_cap(monkeypatch, family):
    grid, wpb = geometry(family)
    tw, T = grid * wpb, TICKS[family]
    k1 = tw + 500
    w = [k1 - 1, k1, k1 + 1, k1 + 2, k1 + 3][:T]       # row k1 is the 33rd row of the query's own score

    def fill(x, E):
        slots = [b * wpb + j for b in range(20, 25) for j in range(7)]    # seven rows in each of five workgroups: no list holds eight of them
        x[slots[:32]] = 1.0
        x[k1] = 1.0

    chip, db = crafted(monkeypatch, family, k1 + 60, w, fill)
    with chip:
        _, lp, res = check_window(chip, db, w, family, expect_cert=[1, 1, 0, 0, 0][:T])
        for t, k in enumerate(w):
            r = res[t][0]
            assert (r["G"], r["M"], len(r["R"])) == (1.0, -1.0, 32 if k <= k1 else 33), (t, r["G"], r["M"], len(r["R"]))
            assert r["M"] < r["thr"]                   # only the count decides


@pytest.mark.parametrize("family", ["prefilter", "halfq"])
@pytest.mark.parametrize("lap", [1, 0, 2])
def test_ownership_switches_at_k_plus_one_rows(monkeypatch, family, lap):
    grid, wpb = geometry(family)
    tw, T = grid * wpb, TICKS[family]
    if lap == 1:       # the share's first row of the second lap is the workgroup's ninth row
        b, b0 = 30, 10
        s = tw + b * wpb
        w, want = [s - 1, s, s + 1, s + 2, s + 3][:T], [1, 1, 0, 0, 0][:T]
    elif lap == 0:     # prefixes that end inside, at the end of and beyond the share in the first lap: nobody owns more than eight rows
        b, b0 = 10, 1
        s = b * wpb
        w, want = [s + 7, s + 8, s + 9, s + 17, s + 40][:T], [1] * T
    else:              # prefixes that end in the third lap in front of the share: sixteen rows owned, whatever k mod tw - b wpb says
        b, b0 = 30, 10
        s = 2 * tw + b * wpb
        w, want = [s - 9, s - 8, s - 7, s - 1, s][:T], [0] * T

    def fill(x, E):
        plant_top(x, wpb, b0)
        x[b * wpb:(b + 1) * wpb] = M_HI                # the workgroup's first-lap share: eight rows inside (G - 2 E, G)
        assert float(M_HI) > float(G_TOP) - 2 * E

    chip, db = crafted(monkeypatch, family, max(w) + 60, w, fill)
    with chip:
        _, lp, res = check_window(chip, db, w, family, expect_cert=want)
        for t, k in enumerate(w):
            r = res[t][0]
            full = lp["cand_i"][t, b, 0, K - 1] >= 0
            assert r["G"] == float(G_TOP) and len(r["R"]) == 8 + (8 if full else 7), (t, r["G"], len(r["R"]))
            assert (r["dropped"] and r["M"] == float(M_HI)) == (not want[t]), (t, r["M"], r["dropped"])
