"""The limit cases of the ORB front end (tests/orb_limit_cases.py) are what they claim to be, from the stage functions of the numpy
restatement alone: every dotted line fills its strip's segment to `cap`, full strips lie next to empty ones, the keys have both signs and
are all distinct (or, tied, one key per line away from its ends), and the quotas leave levels with candidates and nothing to keep.
tests/test_orb_limits_gpu.py relies on these properties: if one fails here, the construction is wrong, not the kernel."""
import numpy as np
import pytest

import np_mirror_orb_detect as O
import orb_limit_cases as LC

# name -> (cap, strips, candidates) as worked out by hand for BORDER = 16
TABLE = {"4096x41": (2032, 5, 6096), "4095x41": (2032, 5, 6096), "41x4096": (5, 2032, 5080), "300x45": (134, 7, 536),
         "301x45_split": (135, 7, 3 * 135 + 67), "4096x73": (2032, 21, 22352),
         "301x45": (135, 7, 540), "4096x41_tied": (2032, 5, 6096), "4096x73_tied": (2032, 21, 22352),
         "4096x41_row2": (2032, 5, 4064), "4095x41_row2": (2032, 5, 4064), "41x4096_row2": (5, 2032, 5080), "300x45_row2": (134, 7, 402),
         "301x45_row2": (135, 7, 405), "4096x73_row2": (2032, 21, 20320)}
NEGATIVE = {"4096x41": 1974, "300x45": 168}
TIES = {"4096x41_tied": 2028, "4096x73_tied": 9 * 2028}                                      # equal keys of the lines between the first and the last


def test_the_table_names_every_case():
    assert set(TABLE) == set(LC.NAMES)
    assert LC.cap_of(LC.MAX_SIDE) == LC.strips_of(LC.MAX_SIDE) == 2032                    # kStripMaxCand, kMaxStrips of orb.hip


@pytest.mark.parametrize("name", LC.NAMES)
def test_every_line_fills_its_segment(name):
    c = LC.case(name)
    cap, nstrips, total = TABLE[name]
    L = O.plan(c["w"], c["h"], LC.params())[0]
    assert (c["cap"], c["nstrips"], c["n_candidates"]) == (cap, nstrips, total)
    assert (L["x0"], L["y0"], L["x1"], L["y1"]) == LC.rectangle(c["w"], c["h"]) and cap == (L["x1"] - L["x0"] + 2) // 2
    S = O.score_plane(c["img"])
    ras, R = LC.level0_candidates(name)
    assert len(ras) == total and (np.diff(ras) > 0).all()
    ys, xs = ras // c["w"], ras % c["w"]
    assert ((xs - L["x0"]) % 2 == 0).all()                                                 # the dots and nothing else
    assert (S[ys, xs] == c["img"][ys, xs].astype(int) - 41).all()                          # a strict maximum of score v - 41 ...
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                assert (S[ys + dy, xs + dx] == -1).all()                                   # ... among neighbours of -1
    per_strip = LC.strip_counts(c, ys)
    assert len(per_strip) == nstrips and per_strip.max() == cap
    full = np.zeros(nstrips, bool)
    full[list(c["full"])] = True
    assert (per_strip[full] == cap).all() and (per_strip[~full] < cap).all()
    if not c["split"]:
        assert (per_strip[~full] == 0).all() and full.sum() == len(c["rows"])              # full strips next to empty ones
    if name in NEGATIVE:
        assert int((R < 0).sum()) == NEGATIVE[name]
    if c["tied"]:
        # the 9 x 9 footprint of R holds the same dots away from the line ends: one key on the first and the last line, which see one
        # other line 4 rows away, and one on the lines between, which see two
        inner = (xs >= L["x0"] + 4) & (xs <= L["x0"] + 2 * (cap - 1) - 4)
        outer = (ys == c["rows"][0]) | (ys == c["rows"][-1])
        a, b = set(R[inner & outer].tolist()), set(R[inner & ~outer].tolist())
        assert len(a) == len(b) == 1 and a != b and (inner & outer).sum() == 2 * (cap - 4)
        assert (inner & ~outer).sum() == (len(c["rows"]) - 2) * (cap - 4) == TIES[name]
    else:
        assert len(set(R.tolist())) == total                                               # all keys distinct
        assert (R < 0).any() and (R > 0).any()


def test_full_and_empty_strips_alternate():
    for name, n_full in (("4096x41", 3), ("4095x41", 3), ("41x4096", 1016), ("300x45", 4), ("4096x73", 11)):
        c = LC.case(name)
        assert c["full"] == tuple(range(0, c["nstrips"], 2)) and len(c["full"]) == n_full
        assert LC.case(name + "_row2")["full"] == tuple(range(0, c["nstrips"] - 1, 2))     # the same strips, their second rows


def test_the_split_lines_cross_both_rows_of_a_strip():
    c = LC.case("301x45_split")
    ras, _ = LC.level0_candidates("301x45_split")
    ys = ras // c["w"]
    per_row = np.bincount(ys - LC.BORDER, minlength=13)
    assert per_row.tolist() == [67, 68, 0, 0] * 3 + [67]                                   # the last strip has one row in the rectangle
    assert LC.strip_counts(c, ys).tolist() == [135, 0, 135, 0, 135, 0, 67]


@pytest.mark.parametrize("name", ("300x45", "301x45_split"))
def test_both_forms_agree_on_the_45_row_images(name):
    want = LC.mirror(name)
    got, counts = O.detect(LC.case(name)["img"], LC.params(), loops=True)
    assert counts == want[1] and got.tobytes() == want[0].tobytes() and len(got) == TABLE[name][2]


def test_all_kept_mirror_records_are_the_candidates():
    for name in LC.NAMES:
        if name.startswith("4096x73"):
            continue
        recs, counts, desc, _ = LC.mirror(name)
        ras, R = LC.level0_candidates(name)
        assert counts == [len(ras)] + [0] * 7 and np.array_equal(recs["response"], R)
        assert np.array_equal(LC.rasters_of(recs, LC.case(name)["w"]), ras) and desc.shape == (len(ras), 32)


def test_ranks_select_through_both_signs():
    recs = LC.mirror("300x45")[0]
    order = np.sort(recs["response"])[::-1]
    for q in (1, 2, 367, 368, 369, 535):
        kept = LC.selected(recs, 300, q)
        assert len(kept) == q and kept["response"].min() == order[q - 1]                  # R* walks down the sorted keys
    assert order[367] > 0 > order[368]                                                     # 536 - 168 keys above zero


def test_16384_of_22352_and_the_levels_above():
    recs, counts, desc, _ = LC.mirror("4096x73")
    assert counts == [16384] + [0] * 7 and len(recs) == len(desc) == LC.MAX_KEPT
    assert LC.mirror("4096x73", 8)[1] == [3558, 2965, 2471, 2059, 538, 0, 0, 0]
    assert [L["quota"] for L in O.plan(4096, 73, LC.params(8))][:5] == [3558, 2965, 2471, 2059, 1716]


def test_quota_0_beside_candidates():
    everything = LC.quota0_mirror(LC.MAX_KEPT)[1]
    assert everything[0] == 902 and everything[7] == 2 and all(n > 0 for n in everything)
    for nf in LC.QUOTA0_FEATURES:
        counts = LC.quota0_mirror(nf)[1]
        quotas = [L["quota"] for L in O.plan(160, 120, LC.params(8, nf))]
        assert counts == quotas and sum(counts) == nf                                      # every level has more candidates than its quota
        if nf in LC.QUOTA0_COUNTS:
            assert counts == LC.QUOTA0_COUNTS[nf] and 0 in counts
