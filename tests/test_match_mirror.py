"""The numpy restatement of the candidate verification front end (tests/np_mirror_match.py) against hand-worked cases: it is what the
GPU results are compared with (tests/test_match_gpu.py), so its own corner cases are pinned here, without a GPU."""
import re
from pathlib import Path

import numpy as np

import np_mirror_match as M
from cerebro_amd import capi, synth

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("chip_build_has_match", "chip_orb_match", "chip_gms_filter", "chip_match_pair", "chip_match_read_sets",
               "chip_pnp_ransac_matched", "chip_icp_ransac_matched")


def desc(*first_bytes):
    d = np.zeros((len(first_bytes), 32), np.uint8)
    d[:, 0] = first_bytes
    return d


def test_hamming_toy_with_a_tie():
    q = desc(0b0000_0000, 0b1111_0000, 0b0000_0111)
    t = desc(0b0000_0001, 0b0000_0010, 0b1111_0001)
    idx, dist = M.orb_bf_match(q, t)
    # query 0: distances 1, 1, 5 -> the FIRST minimum; query 1: 5, 5, 1; query 2: 2, 2, 6 -> first
    assert idx.tolist() == [0, 2, 0] and dist.tolist() == [1, 1, 2]
    idx, dist = M.orb_bf_match(q, t[:0])
    assert idx.tolist() == [-1, -1, -1] and dist.tolist() == [-1, -1, -1]
    full = np.full((1, 32), 255, np.uint8)
    assert M.orb_bf_match(full, np.zeros((1, 32), np.uint8))[1].tolist() == [256]


def test_hamming_against_a_bit_loop():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (70, 32), dtype=np.uint8)
    b[50] = b[3]; a[7] = b[3]                                        # an exact duplicate in the train set: index 3 wins
    idx, dist = M.orb_bf_match(a, b)
    for i in range(40):
        d = [bin(int.from_bytes((a[i] ^ b[j]).tobytes(), "little")).count("1") for j in range(70)]
        assert dist[i] == min(d) and idx[i] == d.index(min(d))
    assert idx[7] == 3 and dist[7] == 0


def test_grid_cells_on_the_borders():
    w, h = 752, 480
    # x / w * 20 exactly integral (376 -> 10, 188 -> 5), exactly integral + 0.5 after the shift (94 -> 2.5), x = width, just inside
    xs = np.array([376.0, 188.0, 94.0, 752.0, 751.99, 0.0], np.float32)
    ys = np.full(6, 100.0, np.float32)                              # 100 / 480 * 20 = 4.1666 -> row 4; shifted 4.6666 -> row 4
    px, py = M.normalise(np.stack([xs, ys], axis=1), w, h)
    assert M.cell_left(px, py, 1).tolist() == [10 + 80, 5 + 80, 2 + 80, -1, 19 + 80, 0 + 80]
    assert M.cell_left(px, py, 2).tolist() == [10 + 80, 5 + 80, 3 + 80, -1, -1, -1]      # floor(x20 + 0.5); 0 -> index 0 < 1 and 20 >= 20 rejected
    assert M.cell_left(px, py, 3).tolist() == [10 + 80, 5 + 80, 2 + 80, 20 + 80, 19 + 80, 0 + 80]   # x not range-checked in type 3: x = width aliases
    assert M.cell_left(px, py, 4).tolist() == [10 + 80, 5 + 80, 3 + 80, -1, -1, -1]
    assert M.cell_right(px, py).tolist() == [10 + 80, 5 + 80, 2 + 80, 20 + 80, 19 + 80, 0 + 80]
    # y = height: row 20 -> index >= 400 -> no cell; type 3 / 4 reject the shifted row 20; top row: shifted row 0 < 1 rejected
    px, py = M.normalise(np.array([[100.0, 480.0], [100.0, 0.0], [100.0, 12.0]], np.float32), w, h)
    assert M.cell_left(px, py, 1).tolist() == [-1, 2, 2]
    assert M.cell_left(px, py, 2).tolist() == [-1, 3, 3]            # 100 / 752 * 20 = 2.66 -> shifted 3; row 20 -> index 403 outside the table
    assert M.cell_left(px, py, 3).tolist() == [-1, -1, 2 + 20]      # 12 / 480 * 20 = 0.5 exactly -> shifted row 1
    assert M.cell_right(px, py).tolist() == [-1, 2, 2]
    # the shift is added in DOUBLE to the FLOAT product: a float just below k + 0.5 stays below
    p = np.float32(0.125) - np.float32(2.0 ** -27)
    assert M.cell_left(np.array([p]), np.array([np.float32(0.3)]), 2).tolist() == [2 + 6 * 20]
    # not finite / absurd coordinates have no cell
    bad = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
    assert (M.cell_left(bad, np.full(4, 0.5, np.float32), 1) == -1).all() and (M.cell_right(np.full(4, 0.5, np.float32), bad) == -1).all()


def translation_scene(per_cell=4, seed=2):
    """left points in cells (2..15, 2..15), `per_cell` each, away from the cell borders; right = left shifted by (2, 1) cells"""
    rng = np.random.default_rng(seed)
    w, h = 752, 480
    cw, ch = w / 20, h / 20
    pts = []
    for cy in range(2, 16):
        for cx in range(2, 16):
            for _ in range(per_cell):
                pts.append([(cx + rng.uniform(0.3, 0.7)) * cw, (cy + rng.uniform(0.3, 0.7)) * ch])
    kp1 = np.array(pts, np.float32)
    kp2 = (kp1 + np.array([2 * cw, ch], np.float32)).astype(np.float32)
    return kp1, kp2, (w, h)


def test_gms_keeps_a_translation_and_drops_random_matches():
    kp1, kp2, size = translation_scene()
    n = len(kp1)
    q = np.arange(n)
    assert M.gms_filter(kp1, size, kp2, size, q, q).all()           # every true match survives
    rng = np.random.default_rng(4)
    t = rng.permutation(n)
    wrong = t != q
    mixed = np.where(np.arange(n) % 5 == 0, t, q)                   # a fifth of the matches point at a random keypoint
    inl = M.gms_filter(kp1, size, kp2, size, q, mixed)
    bad = (np.arange(n) % 5 == 0) & wrong
    # a random partner in the right CELL would be kept (GMS votes on cells, not points): count the ones that land elsewhere
    x2, y2 = M.normalise(kp2, *size)
    cell = M.cell_right(x2, y2)
    elsewhere = bad & (cell[mixed] != cell[q])
    assert not inl[elsewhere].any() and inl[~bad].all()
    assert M.gms_filter(kp1, size, kp2, size, q, t).sum() <= 0.02 * n     # uniformly random matches do not survive


def test_gms_pass_first_maximum_and_threshold():
    # left cell 0: two right cells with equal counts -> the LOWER index; threshold 6 * sqrt(mean count over the 4 in-grid neighbour pairs)
    l = np.array([0] * 10 + [0] * 10 + [21] * 3, np.int32)
    r = np.array([45] * 10 + [44] * 10 + [65] * 3, np.int32)
    pair = M.gms_pass(l, r)
    # cell 0 -> 44: pairs (0,44) (1,45) (20,64) (21,65): score 10 + 0 + 0 + 3 = 13; counts 20 + 0 + 0 + 3 -> thresh 6 * sqrt(23 / 4) = 14.39 -> rejected
    assert pair[0] == -2
    # cell 21 -> 65 with all 9 neighbour pairs in the grid: score 10 (0 -> 44) + 3 = 13; thresh 6 * sqrt(23 / 9) = 9.59 -> accepted
    assert pair[21] == 65 and (np.delete(pair, [0, 21]) == -1).all()
    l2 = np.array([0] * 30 + [0] * 30, np.int32); r2 = np.array([45] * 30 + [44] * 30, np.int32)
    assert M.gms_pass(l2, r2)[0] == 44                               # 30 >= 6 * sqrt(60 / 4) = 23.2; the tie goes to the lower right index
    assert M.gms_pass(np.array([-1, 5], np.int32), np.array([3, -1], np.int32)).tolist() == [-1] * 400   # either index negative: not counted


def test_depth_gate_and_pixels():
    z = np.array([0.1, np.nextafter(np.float32(0.1), np.float32(0)), 25.0, np.nextafter(np.float32(25), np.float32(26)), np.nan, 0.0, 12.0, -3.0, np.inf],
                 np.float32)
    # 0.1f = 0.100000001490116 is not < 0.1; NaN fails both comparisons and passes, as in the reference
    assert M.depth_ok(z).tolist() == [True, False, True, False, True, False, True, False, False]
    inside, x, y = M._pixel(np.array([[-0.5, 3.9], [-1.0, 3.0], [751.99, 479.5], [752.0, 1.0], [1.0, 480.0], [np.nan, 1.0]], np.float32), 752, 480)
    assert inside.tolist() == [True, False, True, False, False, False]
    assert (x[0], y[0], x[2], y[2]) == (0, 3, 751, 479)              # truncation toward zero
    # a 2 x 3 image, one match per case
    xyz = np.zeros((2, 3, 3), np.float32)
    xyz[0, 1] = [1.0, 2.0, 0.1]; xyz[1, 2] = [3.0, 4.0, np.nan]; xyz[1, 0] = [5.0, 6.0, 30.0]; xyz[0, 0] = [7.0, 8.0, 9.0]
    kp1 = np.array([[1.5, 0.5], [2.2, 1.9], [0.1, 1.0], [0.0, 0.0], [3.0, 0.0]], np.float32)
    kp2 = np.array([[0.0, 0.0]] * 5, np.float32)
    Kinv = np.array([0.5, 0.0, -1.0, 0.0, 0.25, -2.0, 0.0, 0.0, 1.0])
    o = M.pose_sets(kp1, kp2, np.zeros(5, np.int64), np.ones(5, np.uint8), xyz, xyz, Kinv)
    assert o["summary"] == dict(n_matches_gms=5, n_3d2d_ab=3, n_3d2d_ba=5, n_3d3d=3, n_out_of_image=1)
    assert o["X_ab"][:, 0].tolist() == [1.0, 3.0, 7.0] and np.isnan(o["X_ab"][1, 2]) and o["X_ab"][0, 2] == float(np.float32(0.1))
    assert o["uvn_ab"].tolist() == [[-1.0, -2.0]] * 3                # b's pixel (0, 0) normalised
    assert o["uvn_ba"][0].tolist() == [0.5 * 1.5 - 1.0, 0.25 * 0.5 - 2.0]
    assert o["match_query_idx"].tolist() == [0, 1, 2, 3, 4]


def test_scene_generator_feeds_the_stage():
    sc = synth.make_match_scene(n_true=1500, n_outlier_a=100, n_outlier_b=100, n_duplicates=30, n_border=16, seed=5)
    o = M.match_pair(sc["a"], sc["b"], sc["Kinv"])
    ia, ib = sc["pairs"]
    assert (o["train_idx"][ia] == ib).mean() > 0.99                  # 4 % flipped bits against ~128 for a random pair
    assert o["inlier"][ia].mean() > 0.8 and o["summary"]["n_matches_gms"] > 800
    outl = np.setdiff1d(np.arange(len(sc["a"]["kp"])), ia)
    assert o["inlier"][outl].mean() < 0.05
    # the sets are consistent with the generator's pose: X_b = R X_a + t on the 3d-3d set, to float32 resolution
    T = sc["T"]
    assert np.abs(o["A_3d3d"] @ T[:3, :3].T + T[:3, 3] - o["B_3d3d"]).max() < 1e-5
    few = synth.make_match_scene(n_true=100, n_outlier_a=300, n_outlier_b=300, seed=15)
    assert M.match_pair(few["a"], few["b"], few["Kinv"])["summary"]["n_matches_gms"] < 150


def test_capi_table_and_header_list_the_stage():
    assert set(NEW_SYMBOLS) <= set(capi.declared_symbols())
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cerebro_hip.h").read_text(), flags=re.S)
    assert set(NEW_SYMBOLS) <= set(re.findall(r"\b(chip_[a-z0-9_]+)\s*\(", text))
    assert "#define CHIP_ABI_VERSION 7" in text
    import ctypes as C
    assert C.sizeof(capi.MatchSummary) == 24 and C.sizeof(capi.MatchFrame) == 40 and C.sizeof(capi.MatchSetsOut) == 80
