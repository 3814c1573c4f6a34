"""The three kernels of the candidate verification front end (cerebro_amd/csrc/match.hip) at the places where THESE kernels can be
subtly wrong and seeded random scenes do not go: the wave-wide first-maximum search of gms_filter at its ties, its strict threshold at
equality, the 1024-wide LDS tiles of orb_bf_match at their boundaries, and the ordered 16-wave compaction of pose_sets_build under
keep / drop patterns that are adversarial for a prefix scan.  One ctx for the module.

Expected values: for gms_filter the masks of the REFERENCE's compiled matcher, frozen in tests/golden/gms_ref.json (tests/
test_gms_ref_mirror.py checks them against the reference wherever it can be compiled); for orb_bf_match a plain integer Hamming
search; for the sets tests/np_mirror_match.py.  Every input is legal under include/cerebro_hip.h."""
import json
import time
from pathlib import Path

import numpy as np
import pytest

import gms_cases as G
import np_mirror_match as M
from cerebro_amd import capi, synth

pytestmark = pytest.mark.gpu

GOLD = {e["name"]: e for e in json.loads((Path(__file__).resolve().parent / "golden" / "gms_ref.json").read_text())["cases"]}
SET_KEYS = ("uv", "uv_d", "X_ab", "uvn_ab", "X_ba", "uvn_ba", "A_3d3d", "B_3d3d", "match_query_idx", "match_train_idx")


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


def same_bytes(a: np.ndarray, b: np.ndarray):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ================================================================================================ gms_filter
def golden_case(name):
    """(inputs, the reference's mask) of a frozen case; the inputs are regenerated and their hash checked first"""
    e = GOLD[name]
    c = G.generate(e["kind"], e["args"])
    assert G.digest(c) == e["sha256"], f"{name}: the generator no longer produces the frozen input"
    want = np.unpackbits(np.frombuffer(bytes.fromhex(e["mask_hex"]), np.uint8))[: e["n"]]
    assert len(c["q"]) == e["n"] and int(want.sum()) == e["n_inliers"]
    return c, want


def device_mask(chip, c):
    return chip.gms_filter(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])


# the 16384-increments-on-one-table-entry case runs in its own test, after the 4096 one has been timed
@pytest.mark.parametrize("name", [n for n in GOLD if n != "one_cell_pair_16384"])
def test_gms_equals_the_frozen_reference_mask(chip, name):
    c, want = golden_case(name)
    got = device_mask(chip, c)
    assert same_bytes(got, want), (name, np.nonzero(got != want)[0][:8])


def test_gms_golden_covers_what_this_module_claims():
    assert set(G.CONSTRUCTED) <= set(GOLD)
    sizes = {GOLD[f"smooth_n{n}"]["n"] for n in (1, 63, 64, 65, 1023, 1024, 1025, 16384)}
    assert sizes == {1, 63, 64, 65, 1023, 1024, 1025, 16384}
    assert all(GOLD[f"smooth_n{n}"]["n_inliers"] > 500 for n in (1023, 1024, 1025, 16384))


@pytest.mark.parametrize("name", [n for n in G.CONSTRUCTED if n.startswith("tie_") and n != "tie_in_shifted_grid_only"])
def test_gms_column_tie_keeps_the_lower_column(chip, name):
    """equal counts in 2 or 3 right cells of one left cell (columns in one lane of the strided scan, in neighbouring lanes, at 0 and
    399): the matches into the LOWEST column are marked and no others (groups are listed from the highest column down)"""
    c, want = golden_case(name)
    got = device_mask(chip, c)
    last = int(c["group"].max())
    assert got[c["group"] == last].all(), name
    assert not got[c["group"] != last].any(), name
    assert same_bytes(got, want)


def test_gms_tie_in_one_grid_type_only(chip):
    c, want = golden_case("tie_in_shifted_grid_only")
    got = device_mask(chip, c)
    assert [int(got[c["group"] == g].sum()) for g in range(4)] == [24, 25, 0, 25]
    assert same_bytes(got, want)


@pytest.mark.parametrize("where", ["interior", "corner", "edge"])
def test_gms_score_equal_to_the_threshold_is_kept(chip, where):
    """score == 6 * sqrt(mean count) == 12.0 exactly, over 9 / 4 / 6 neighbour pairs: kept; one match short: dropped"""
    c, want = golden_case(f"thresh_equal_{where}")
    got = device_mask(chip, c)
    assert got[c["group"] == 0].all() and got.sum() == 12 and same_bytes(got, want)
    c, want = golden_case(f"thresh_short_{where}")
    got = device_mask(chip, c)
    assert not got.any() and same_bytes(got, want)


def test_gms_survivor_counts_around_150_and_a_shifted_grid_survivor(chip):
    for k in (37, 149, 150, 151):
        c, want = golden_case(f"cluster_{k}")
        got = device_mask(chip, c)
        assert got.sum() == k and got[c["group"] == 0].all() and same_bytes(got, want)
    c, want = golden_case("survives_shifted_grid_only")               # kept by grid types 2 and 4 only (tests/test_gms_ref_mirror.py)
    got = device_mask(chip, c)
    assert got.all() and same_bytes(got, want)


def test_gms_every_match_in_one_cell_pair(chip):
    """one table entry takes n atomic increments per grid type, inside one workgroup: 4096 first, timed; 16384 only if that scales"""
    c, want = golden_case("one_cell_pair_4096")
    device_mask(chip, c)                                              # first use of the ctx's buffers is not what is timed
    t0 = time.perf_counter()
    got = device_mask(chip, c)
    dt = time.perf_counter() - t0
    assert same_bytes(got, want) and got.all()
    assert dt < 2.0, f"4096 increments of one entry took {dt:.3f} s: the 16384 case is not run"
    c, want = golden_case("one_cell_pair_16384")
    t0 = time.perf_counter()
    got = device_mask(chip, c)
    dt16 = time.perf_counter() - t0
    assert same_bytes(got, want) and got.all()
    print(f"\ngms_filter, every match in one cell pair: n=4096 {dt * 1e3:.2f} ms, n=16384 {dt16 * 1e3:.2f} ms (host wall, copies included)")


def test_gms_two_calls_on_one_ctx_equal_fresh_ctxs(chip):
    """the 640 KB table, the LDS counts and the inlier bytes are rewritten by every call, not reused: a large dense case, then a
    small one whose cells were all populated by the first, then the first again"""
    a, want_a = golden_case("smooth_n16384")
    b, want_b = golden_case("tie_cols_j_j64")
    d, want_d = golden_case("thresh_short_interior")
    seq = [device_mask(chip, x) for x in (a, b, d, a)]
    fresh = []
    for x in (a, b, d):
        with capi.Chip(4096) as c2:
            fresh.append(device_mask(c2, x))
    assert same_bytes(seq[0], fresh[0]) and same_bytes(seq[1], fresh[1]) and same_bytes(seq[2], fresh[2]) and same_bytes(seq[3], fresh[0])
    assert same_bytes(seq[0], want_a) and same_bytes(seq[1], want_b) and same_bytes(seq[2], want_d)


# ================================================================================================ orb_bf_match
def hamming_search(d1: np.ndarray, d2: np.ndarray):
    """plain integer search: popcount of the xor, first minimum in train order"""
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
    idx = np.empty(len(d1), np.int32)
    dist = np.empty(len(d1), np.int32)
    if hasattr(np, "bitwise_count"):
        a, b = d1.view(np.uint64), d2.view(np.uint64)
        for lo in range(0, len(a), 256):
            h = np.bitwise_count(a[lo:lo + 256, None, :] ^ b[None, :, :]).sum(2, dtype=np.int32)
            j = h.argmin(1)
            idx[lo:lo + 256], dist[lo:lo + 256] = j, h[np.arange(len(j)), j]
    else:
        for lo in range(0, len(d1), 16):
            h = np.unpackbits(d1[lo:lo + 16, None, :] ^ d2[None, :, :], axis=2).sum(2, dtype=np.int32)
            j = h.argmin(1)
            idx[lo:lo + 16], dist[lo:lo + 16] = j, h[np.arange(len(j)), j]
    return idx, dist


def test_hamming_search_is_the_plain_definition():
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 256, (40, 32), dtype=np.uint8), rng.integers(0, 256, (70, 32), dtype=np.uint8)
    b[50] = b[20] = a[3]
    idx, dist = hamming_search(a, b)
    for i in range(40):
        h = [int(np.unpackbits(a[i] ^ b[j]).sum()) for j in range(70)]
        assert idx[i] == int(np.argmin(h)) and dist[i] == min(h)
    assert idx[3] == 20 and dist[3] == 0


def near_copies(rng, base, n, max_flips=2):
    """n descriptors within max_flips bits of `base` (flips in the last 16 bytes only)"""
    d = np.tile(base, (n, 1))
    for i in range(n):
        for bit in rng.choice(128, rng.integers(0, max_flips + 1), replace=False):
            d[i, 16 + bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def check_match(chip, d1, d2):
    idx, dist = chip.orb_match(d1, d2)
    w_idx, w_dist = hamming_search(d1, d2)
    assert np.array_equal(idx, w_idx), np.nonzero(idx != w_idx)[0][:8]
    assert np.array_equal(dist, w_dist)
    return idx, dist


@pytest.mark.parametrize("n2", [1023, 1024, 1025, 2049, 16384])
def test_orb_unique_minimum_at_the_tile_edges(chip, n2):
    """the one near descriptor sits at train index 0, 1023, 1024, 1025, 2047, 2048, n2 - 1: every query (three workgroups and a
    partial one) finds it there"""
    rng = np.random.default_rng(n2)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d1 = near_copies(rng, base, 700)
    for p in sorted({p for p in (0, 1023, 1024, 1025, 2047, 2048, n2 - 1) if p < n2}):
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        d2[p] = base
        idx, dist = check_match(chip, d1, d2)
        assert (idx == p).all() and dist.max() <= 2, (n2, p)


@pytest.mark.parametrize("lo,hi,n2", [(1023, 1024, 1025), (1023, 1024, 5000), (0, 1024, 1025), (0, 1024, 3000), (2047, 4096, 4097), (2047, 4096, 16384),
                                      (1024, 2048, 2049), (5, 1023, 1024)])
def test_orb_equal_minima_across_a_tile_boundary_keep_the_lower_index(chip, lo, hi, n2):
    """the same nearest descriptor at `lo` and at `hi`, in different LDS tiles (or the last slot of one): the strict < across tiles keeps
    `lo`, for every lane of the first, a middle and the last wave of the launch"""
    rng = np.random.default_rng(lo * 7 + hi)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    n1 = 1000                                                         # 4 workgroups, the last one partial; 16 waves
    d1 = near_copies(rng, base, n1)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d2[lo] = d2[hi] = base
    idx, dist = check_match(chip, d1, d2)
    for wave in (0, 7, n1 // 64):
        assert (idx[wave * 64:(wave + 1) * 64] == lo).all(), (wave, idx[wave * 64:(wave + 1) * 64])
    assert (idx == lo).all()
    d2[hi] = base ^ np.uint8(0)                                       # and three equal minima, the third in the last slot
    d2[n2 - 1] = base
    idx, _ = check_match(chip, d1, d2)
    assert (idx == lo).all()


def test_orb_distances_0_and_256(chip):
    rng = np.random.default_rng(4)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    idx, dist = check_match(chip, base[None], (~base)[None])
    assert idx[0] == 0 and dist[0] == 256                             # the complement: every bit differs
    idx, dist = check_match(chip, base[None], base[None])
    assert idx[0] == 0 and dist[0] == 0
    d2 = np.tile(~base, (2049, 1))                                    # everything at 256 (the first wins) ...
    idx, dist = check_match(chip, np.tile(base, (300, 1)), d2)
    assert (idx == 0).all() and (dist == 256).all()
    d2[2048] = base                                                   # ... but one exact copy in the third tile
    idx, dist = check_match(chip, np.tile(base, (300, 1)), d2)
    assert (idx == 2048).all() and (dist == 0).all()
    z, o = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    assert check_match(chip, z, o)[1][0] == 256 and check_match(chip, o, np.concatenate([z, o]))[0][0] == 1


@pytest.mark.parametrize("n1", [1, 255, 256, 257, 16384])
def test_orb_query_counts_against_one_and_16384_train_descriptors(chip, n1):
    rng = np.random.default_rng(n1)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    idx, dist = check_match(chip, d1, d1[-1:])                        # n2 = 1
    assert (idx == 0).all() and dist[-1] == 0
    d2 = rng.integers(0, 256, (16384, 32), dtype=np.uint8)
    sel = rng.permutation(16384 if n1 == 16384 else 16383)[:n1]
    d2[sel] = d1                                                      # every query has its exact copy somewhere in the 16 tiles
    if n1 < 16384:
        d2[16383] = d1[0]                                             # and query 0 a second one in the last slot: the earlier one wins
    idx, dist = check_match(chip, d1, d2)
    assert (dist == 0).all() and np.array_equal(idx, sel)


# ================================================================================================ pose_sets_build
def pattern(kind: str, n: int) -> np.ndarray:
    i = np.arange(n)
    lane, wave = i % 64, (i // 64) % 16
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "wave5_dropped": wave != 5, "wave0_dropped": wave != 0,
            "alternating": lane % 2 == 0, "odd_lanes": lane % 2 == 1, "last_lane_of_wave15": (lane == 63) & (wave == 15),
            "last8_of_wave15": (lane >= 56) & (wave == 15), "first_lane_only": (lane == 0) & (wave == 0),
            "wave15_only": wave == 15}[kind]


def sets_scene(n, gms, depth_a, depth_b, wa=752, ha=480, wb=752, hb=480, seed=0):
    """n keypoints per frame, identical descriptors frame to frame (match i = (i, i), distance 0).  Match i survives GMS iff gms[i]:
    the kept ones are an identity motion on distinct pixels of a dense block in the upper part of the image (rows 50 .. 177), the
    dropped ones go from the lower part to random places.  Depth at the keypoint's pixel is valid in frame a iff depth_a[i], in frame b iff depth_b[i]."""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rank = np.cumsum(gms) - 1                                         # kept matches fill a dense 128-pixel-wide block row by row:
    ka = np.stack([80 + rank % 128, 50 + rank // 128], axis=1).astype(np.float32) + np.float32(0.5)   # distinct pixels, in match order
    kb = ka.copy()
    drop = ~gms
    nd = int(drop.sum())
    ka[drop] = np.stack([rng.uniform(2, wa - 2, nd), rng.uniform(ha * 0.62, ha - 2, nd)], axis=1).astype(np.float32)
    kb[drop] = np.stack([rng.uniform(2, wb - 2, nd), rng.uniform(2, hb - 2, nd)], axis=1).astype(np.float32)
    xa = np.zeros((ha, wa, 3), np.float32)
    xb = np.zeros((hb, wb, 3), np.float32)
    k = np.nonzero(gms)[0]
    pa, pb = ka[k].astype(np.int64), kb[k].astype(np.int64)
    xa[pa[:, 1], pa[:, 0]] = np.stack([k * 0.001, -k * 0.002, np.where(depth_a[k], 5.0 + k * 1e-4, 0.0)], axis=1).astype(np.float32)
    xb[pb[:, 1], pb[:, 0]] = np.stack([k * 0.003, k * 0.004, np.where(depth_b[k], 7.0 + k * 1e-4, 0.0)], axis=1).astype(np.float32)
    return dict(desc=desc, kp=ka, xyz=xa), dict(desc=desc, kp=kb, xyz=xb)


def compare_sets(chip, fa, fb, Kinv):
    g = chip.match_pair(fa, fb, Kinv)
    m = M.match_pair(fa, fb, Kinv)
    assert g["summary"] == m["summary"]
    for k in SET_KEYS:
        assert same_bytes(g[k], np.ascontiguousarray(m[k])), k
    assert (np.diff(g["match_query_idx"]) > 0).all()                  # in match order
    return g, m


PATTERNS = [("all", "all", "all"), ("none", "all", "all"), ("wave5_dropped", "alternating", "last_lane_of_wave15"),
            ("alternating", "wave0_dropped", "odd_lanes"), ("last8_of_wave15", "last_lane_of_wave15", "all"),
            ("wave15_only", "none", "first_lane_only"), ("all", "last_lane_of_wave15", "wave5_dropped")]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 4097, 16384])
@pytest.mark.parametrize("gms,da,db", PATTERNS)
def test_sets_keep_patterns_by_wave(chip, n, gms, da, db):
    """a different keep pattern for each of the four compactions (GMS inlier, depth in a, depth in b, both): whole waves dropped,
    one lane of the last wave kept, alternating lanes, everything, nothing; the ten arrays byte-equal and in match order"""
    pg, pa, pb = pattern(gms, n), pattern(da, n), pattern(db, n)
    if n == 1023 and gms == "last8_of_wave15":
        pg = np.arange(n) >= n - 8                                    # wave 15 has 63 lanes there
    fa, fb = sets_scene(n, pg, pa, pb, seed=n)
    _, Kinv = synth.pinhole()
    g, m = compare_sets(chip, fa, fb, Kinv)
    assert np.array_equal(m["inlier"] != 0, pg), "the scene does not produce the GMS pattern it was built for"
    s = g["summary"]
    assert s["n_matches_gms"] == pg.sum() and s["n_3d2d_ab"] == (pg & pa).sum() and s["n_3d2d_ba"] == (pg & pb).sum()
    assert s["n_3d3d"] == (pg & pa & pb).sum() and s["n_out_of_image"] == 0
    assert np.array_equal(g["match_query_idx"], np.nonzero(pg)[0])


def test_sets_odd_widths_two_sizes_last_row_and_column(chip):
    """widths that are not multiples of 4, xyz_a and xyz_b of different sizes, kept keypoints on the last row and the last column of
    both images (the 3-D image is indexed at (h - 1, x) and (y, w - 1))"""
    wa, ha, wb, hb = 751, 479, 803, 501
    n = 1500
    pg = np.ones(n, bool)
    fa, fb = sets_scene(n, pg, pattern("alternating", n), pattern("wave5_dropped", n), wa, ha, wb, hb, seed=3)
    ka, kb = fa["kp"], fb["kp"]
    xa, xb = fa["xyz"], fb["xyz"]
    k = np.arange(60)
    # 30 matches along the last row of a -> the last row of b, 30 along the last column of a -> the last column of b
    ka[:30] = np.stack([100.5 + k[:30], np.full(30, ha - 0.5)], axis=1); kb[:30] = np.stack([107.5 + k[:30], np.full(30, hb - 0.25)], axis=1)
    ka[30:60] = np.stack([np.full(30, wa - 0.75), 200.5 + k[:30]], axis=1); kb[30:60] = np.stack([np.full(30, wb - 0.5), 209.5 + k[:30]], axis=1)
    for i in k:
        xa[int(ka[i, 1]), int(ka[i, 0])] = (0.5, 0.25 * i, 3.0 + 0.125 * i)
        xb[int(kb[i, 1]), int(kb[i, 0])] = (-0.5, 0.125 * i, 4.0 + 0.125 * i)
    assert int(ka[0, 1]) == ha - 1 and int(kb[0, 1]) == hb - 1 and int(ka[30, 0]) == wa - 1 and int(kb[30, 0]) == wb - 1
    _, Kinv = synth.pinhole()
    g, m = compare_sets(chip, fa, fb, Kinv)
    s = g["summary"]
    assert s["n_out_of_image"] == 0 and s["n_matches_gms"] > 1400
    assert np.isin(k, g["match_query_idx"]).all()                     # the 60 edge matches survive GMS ...
    assert (g["A_3d3d"][:, 2] == 3.0).any() and (g["B_3d3d"][:, 2] == 4.0 + 0.125 * 59).any()   # ... and their 3-D points were read at the last row / column
