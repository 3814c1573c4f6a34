"""GPU parity of the disparity -> 3-D step (cerebro_amd/csrc/frames.hip: disparity_gather behind chip_frame_put_disparity,
disparity_to_xyz behind chip_disparity_to_xyz) through ctypes -> C ABI against the numpy restatement (tests/np_mirror_disparity.py).
Floats are compared on their uint32 view, a NaN matches any NaN.  A frame put from its disparity must be indistinguishable from the
same frame put through chip_frame_put with the restated 3-D image: same records, same match results, same poses.  The case set is
tests/disparity_cases.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import disparity_cases as DC
import frame_store_cases as fc
import match_pairs_cases as PC
import np_mirror_disparity as D
import np_mirror_frame_store as S
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
F = np.float32
KINV = PC.kinv()
SET_KEYS = DC.SET_KEYS
N_SLOTS, SLOT_KP = 2 * len(DC.NAMES) + 4, DC.SLOT_KP                 # the case set twice (from disparities, from images) and four spare
VIA_IMAGE = 100000                                                    # id offset of the frames put through chip_frame_put
SPARE = (1, 2, 3, 4)
QS = DC.all_qs()
FLOAT_SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, 1e38, 0.0], F)   # NaN, +-inf, -0.0, a subnormal, 1e38


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        c.frame_store_reserve(N_SLOTS, SLOT_KP)
        yield c


@pytest.fixture
def clean(chip):
    """the module's ctx with an empty store"""
    yield chip
    for i in list(SPARE) + list(range(10, 10 + N_SLOTS)) + [i + o for i in DC.ID.values() for o in (0, VIA_IMAGE)]:
        if chip.lib.chip_frame_drop(chip.h, i) not in (capi.CHIP_OK, capi.CHIP_ERR_RANGE):
            raise AssertionError("chip_frame_drop")
    assert chip.frame_store_info() == dict(n_slots=N_SLOTS, slot_keypoints=SLOT_KP, n_frames=0)


def same_bytes(a: np.ndarray, b: np.ndarray):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def status_of(call, *args):
    with pytest.raises(capi.ChipError) as e:
        call(*args)
    return e.value.status


def disparity(rng, kind: str, w: int, h: int) -> np.ndarray:
    """(h, w) int16 raw disparities with invalid ones among them, or float32 ones with FLOAT_SPECIALS in the first pixels"""
    if kind == "s16":
        d = rng.integers(1, 4096, (h, w)).astype(np.int16)
        d[rng.random((h, w)) < 0.2] = DC.INVALID
        d.reshape(-1)[:3] = (0, -32768, 32767)[:min(3, d.size)]
        return d
    d = rng.uniform(-4.0, 300.0, (h, w)).astype(F)
    m = min(len(FLOAT_SPECIALS), d.size)
    d.reshape(-1)[:m] = FLOAT_SPECIALS[:m]
    return d


# ---------------------------------------------------------------------------------------------- 1: the dense image
@pytest.mark.parametrize("q", range(len(QS)), ids=[name for name, _ in QS])
def test_dense_image_of_all_int16_values_equals_mirror(chip, q):
    assert chip.lib.chip_build_has_disparity() == 1 and chip.lib.chip_abi_version() == 7
    img, Q = DC.all_int16_image(), QS[q][1]
    got = chip.disparity_to_xyz(img, Q)
    want = D.xyz_from_disparity(img, Q)
    assert got.shape == (256, 256, 3) and got.dtype == F
    assert D.same_floats(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("kind", ["s16", "f32"])
def test_dense_small_shapes_cover_tails_and_alignment(chip, kind):
    """widths that are a multiple of four (every thread on the 16-byte path), below four (none), and neither: the rows after the first
    then start at a pixel that is no multiple of four"""
    rng = np.random.default_rng(11)
    seen_specials = False
    for w in (1, 3, 4, 5, 7, 257):
        for h in (1, 2, 3):
            disp = disparity(rng, kind, w, h)
            for _, Q in QS[:2]:
                got = chip.disparity_to_xyz(disp, Q)
                want = D.xyz_from_disparity(disp, Q)
                assert got.shape == (h, w, 3) and D.same_floats(got, want), (w, h, got, want)
            if kind == "f32" and disp.size >= len(FLOAT_SPECIALS):
                seen_specials = True
                z = want.reshape(-1, 3)[:len(FLOAT_SPECIALS), 2]
                assert np.isnan(z[0]) and z[1] == 0 and z[2] == 0 and np.signbit(z[2]) and np.isfinite(z[3:]).all()
    assert seen_specials or kind == "s16"


# ---------------------------------------------------------------------------------------------- 2: put and read back
@pytest.mark.parametrize("kind", ["s16", "f32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_put_and_read_back_equals_mirror(clean, n, kind):
    rng = np.random.default_rng(100 + n)
    edges = [0, 1, 62, 63, 64, 65, 126, 127, 128, 254, 255, 256, 257, 511, 512, 1022, 1023, 1024, n - 2, n - 1]   # first / last of a wave, of a workgroup
    f = fc.frame(rng, n, plant_at=edges + list(range(300, 300 + len(fc.SPECIAL_KP))))
    disp = disparity(rng, kind, fc.W, fc.H)
    Q = QS[n % 2][1]
    clean.frame_put_disparity(3, f, disp, Q)
    r = clean.frame_read(3)
    want = D.records(f["kp"], disp, Q)
    assert (r["n"], r["width"], r["height"]) == (n, fc.W, fc.H)
    assert same_bytes(r["desc"], f["desc"]) and same_bytes(r["kp"], f["kp"])        # as put
    assert D.same_floats(r["pts"], want)
    assert D.same_floats(want, S.gather(f["kp"], D.xyz_from_disparity(disp, Q)))
    if n >= 255:
        assert (want[:, 3] == 0).any() and (want[:, 3] == 1).any() and not want[want[:, 3] == 0].any()


# ---------------------------------------------------------------------------------------------- 3: the pair set
def everything(chip, sms, choices):
    out = []
    for j, (sm, ch) in enumerate(zip(sms, choices)):
        chip.match_select(j)
        d = dict(summary=sm.as_dict(), choice=ch)
        d.update(chip.match_read_sets(sm))
        d["train_idx"], d["distance"] = chip.match_batch_matches(j)
        out.append(d)
    return out


def pairs_all(chip, modes, offset):
    a_ids, b_ids = DC.PC.ids()
    return everything(chip, *chip.match_pairs_stored([i + offset for i in a_ids], [i + offset for i in b_ids], KINV, modes))


def blob(results) -> bytes:
    def one(r):
        ch = r["choice"]
        head = repr(r["summary"]).encode() + repr((ch["scale"], ch["rotation"], ch["n_inliers"])).encode() + np.ascontiguousarray(ch["counts"]).tobytes()
        return head + b"".join(np.ascontiguousarray(r[k]).tobytes() for k in SET_KEYS + ("train_idx", "distance"))
    return b"|".join(one(r) for r in results)


def load_both(chip):
    """every frame of the case set from its disparity under its id, and through chip_frame_put with the mirror's image under id + VIA_IMAGE"""
    img = DC.image_frames()
    for name, f in DC.frames().items():
        chip.frame_put_disparity(DC.ID[name], f, f["disp"], DC.Q_PAIRS)
        chip.frame_put(DC.ID[name] + VIA_IMAGE, img[name])


@pytest.mark.parametrize("modes", [0, 3])
def test_pair_set_from_disparities_equals_image_puts_and_mirror(clean, modes):
    chip = clean
    load_both(chip)
    for name in DC.NAMES:                                             # indistinguishable afterwards: the stored frames themselves
        a, b = chip.frame_read(DC.ID[name]), chip.frame_read(DC.ID[name] + VIA_IMAGE)
        assert (a["n"], a["width"], a["height"]) == (b["n"], b["width"], b["height"])
        assert all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts")), name
    got = pairs_all(chip, modes, 0)
    via = pairs_all(chip, modes, VIA_IMAGE)
    want = DC.mirror(modes)
    assert len(got) == len(via) == len(want) == len(DC.PAIRS) == 11
    for j, (g, v, w) in enumerate(zip(got, via, want)):
        assert blob([g]) == blob([v]), (modes, j, DC.PAIRS[j])
        assert g["summary"] == w["summary"], (modes, j)
        ch = g["choice"]
        assert (ch["scale"], ch["rotation"], ch["n_inliers"]) == (w["choice"]["scale"], w["choice"]["rotation"], w["choice"]["n_inliers"]), (modes, j)
        assert np.array_equal(ch["counts"], w["choice"]["counts"]), (modes, j)
        if not w["summary"]["n_matches_all"]:
            assert (g["train_idx"] == -1).all() and (g["distance"] == -1).all()
            continue
        for k in SET_KEYS + ("train_idx", "distance"):
            assert same_bytes(g[k], np.ascontiguousarray(w[k])), (modes, j, k)
    if modes == 0:
        assert tuple(g["summary"]["n_matches_gms"] for g in got) == DC.EXPECTED_GMS
        assert tuple((g["summary"]["n_3d2d_ab"], g["summary"]["n_3d2d_ba"], g["summary"]["n_3d3d"]) for g in got) == DC.EXPECTED_SETS


def _same_estimate(d: dict, h: dict, what):
    assert d["status"] == h["status"], what
    if h["status"] != 0:
        assert h["status"] == capi.CHIP_ERR_TOO_FEW_POINTS, what
        return
    assert d["summary"] == h["summary"] and d["confidence"] == h["confidence"], what
    assert same_bytes(d["T"], h["T"]) and same_bytes(d["mask"], h["mask"]), what


def test_batched_solvers_are_bit_identical_on_both_ways_of_putting(clean):
    chip = clean
    load_both(chip)
    a_ids, b_ids = DC.PC.ids()

    def solve(offset):
        sms = chip.match_pairs_stored([i + offset for i in a_ids], [i + offset for i in b_ids], KINV)
        P = len(sms)
        problems = []
        for j, sm in enumerate(sms):
            problems += [(j, capi.CHIP_SET_AB, sm.n_3d2d_ab), (j, capi.CHIP_SET_BA, sm.n_3d2d_ba)]
        pp, pi = capi.default_ransac_params(), capi.default_icp_params()
        pp.seed, pi.seed = 5, 6
        ticket = chip.icp_matched_batch_enqueue([(j, sms[j].n_3d3d) for j in range(P)], pi, [900 + 3 * j for j in range(P)])
        pnp = chip.pnp_matched_batch(problems, pp, [100 + 7 * i for i in range(2 * P)])      # the ICP batch runs underneath
        return [s.as_dict() for s in sms], pnp, chip.icp_matched_batch_collect(ticket)

    sm_d, pnp_d, icp_d = solve(0)
    sm_i, pnp_i, icp_i = solve(VIA_IMAGE)
    assert sm_d == sm_i == [m["summary"] for m in DC.mirror(0)]
    assert len(pnp_d) == len(pnp_i) == 22 and len(icp_d) == len(icp_i) == 11
    for i, (d, h) in enumerate(zip(pnp_d, pnp_i)):
        _same_estimate(d, h, ("pnp", i))
    for i, (d, h) in enumerate(zip(icp_d, icp_i)):
        _same_estimate(d, h, ("icp", i))
    assert sum(r["status"] == 0 for r in pnp_d) == 2 * 8 and sum(r["status"] == 0 for r in icp_d) == 8   # all but the three pairs without 20 points


# ---------------------------------------------------------------------------------------------- 4: buffer and slot reuse
def test_replace_across_the_two_ways_of_putting(clean):
    chip = clean
    rng = np.random.default_rng(21)
    f, g = fc.frame(rng, 300, plant_at=range(0, 300, 17)), fc.frame(rng, 200, plant_at=range(0, 200, 13))
    disp = disparity(rng, "s16", fc.W, fc.H)
    chip.frame_put(1, f)                                              # an xyz-put frame ...
    chip.frame_put_disparity(1, g, disp, DC.Q_Q33)                    # ... replaced by a disparity put under the same id
    assert chip.frame_store_info()["n_frames"] == 1
    r = chip.frame_read(1)
    assert r["n"] == 200 and same_bytes(r["desc"], g["desc"]) and same_bytes(r["kp"], g["kp"]) and D.same_floats(r["pts"], D.records(g["kp"], disp, DC.Q_Q33))
    chip.frame_put(1, f)                                              # and the other way round
    assert chip.frame_store_info()["n_frames"] == 1
    r = chip.frame_read(1)
    assert r["n"] == 300 and same_bytes(r["kp"], f["kp"]) and same_bytes(r["pts"], S.gather(f["kp"], f["xyz"]))
    chip.frame_put_disparity(2, dict(desc=f["desc"][:0], kp=f["kp"][:0]), disp, DC.Q_Q33)   # n == 0 is stored
    r = chip.frame_read(2)
    assert (r["n"], r["width"], r["height"]) == (0, fc.W, fc.H) and chip.frame_store_info()["n_frames"] == 2


def test_one_staging_buffer_serves_images_and_disparities_of_any_size(clean):
    """64 x 48 (xyz), 752 x 480 (xyz), 752 x 480 (disparity), 64 x 48 (float disparity) through the one staging buffer, then the dense
    call through it: what each leaves equals what a fresh ctx gives"""
    chip = clean
    rng = np.random.default_rng(22)
    small = fc.frame(rng, 257, plant_at=(0, 63, 64, 256))
    big, big_d = DC.image_frames()["c0"], DC.frames()["c0"]
    small_disp = disparity(rng, "f32", fc.W, fc.H)
    steps = (("xyz", 1, small, None), ("xyz", 2, big, None), ("disp", 3, big_d, big_d["disp"]), ("disp", 4, small, small_disp))

    def run(c, step):
        how, i, f, disp = step
        if how == "xyz":
            c.frame_put(i, f)
        else:
            c.frame_put_disparity(i, f, disp, DC.Q_PAIRS)
        return c.frame_read(i)["pts"]

    got = [run(chip, s) for s in steps]
    dense = chip.disparity_to_xyz(big_d["disp"], DC.Q_PAIRS)
    again = [chip.frame_read(s[1])["pts"] for s in steps]            # later puts and the dense call left the earlier slots alone
    with capi.Chip(4096) as c:                                        # a ctx that ran nothing else (its staging buffer grows at every step)
        c.frame_store_reserve(4, SLOT_KP)
        fresh = [run(c, s) for s in reversed(steps)][::-1]
    for s, g, a, fr in zip(steps, got, again, fresh):
        assert D.same_floats(g, fr) and D.same_floats(a, fr), s[:2]
    assert same_bytes(got[1], got[2])                                 # the 752 x 480 frame: image and disparity give the same records
    assert D.same_floats(got[3], D.records(small["kp"], small_disp, DC.Q_PAIRS))
    assert D.same_floats(dense, big["xyz"])
    with capi.Chip(4096) as c:                                        # the dense call needs no store
        assert c.frame_store_info()["n_slots"] == 0 and D.same_floats(c.disparity_to_xyz(big_d["disp"], DC.Q_PAIRS), dense)


# ---------------------------------------------------------------------------------------------- 5: status codes
def test_status_codes(clean):
    chip = clean
    rng = np.random.default_rng(23)
    f = fc.frame(rng, 40)
    disp = disparity(rng, "s16", fc.W, fc.H)
    Q = np.ascontiguousarray(DC.Q_EUROC).reshape(16)
    desc, kp = np.ascontiguousarray(f["desc"]), np.ascontiguousarray(f["kp"])
    raw = lambda h, kind, q, d=disp: chip.lib.chip_frame_put_disparity(h, 1, capi._ptr(desc), capi._ptr(kp), 40, fc.W, fc.H,   # noqa: E731
                                                                        None if d is None else capi._ptr(d), kind, None if q is None else capi._ptr(q))
    chip.frame_put_disparity(1, f, disp, DC.Q_EUROC)
    before = chip.frame_read(1)
    for kind in (-1, 2, 7):
        assert raw(chip.h, kind, Q) == capi.CHIP_ERR_INVALID_ARG       # an unknown disp_type
    assert raw(chip.h, capi.CHIP_DISP_S16, None) == capi.CHIP_ERR_INVALID_ARG      # a NULL Q
    assert raw(chip.h, capi.CHIP_DISP_S16, Q, None) == capi.CHIP_ERR_INVALID_ARG   # a NULL disparity
    assert raw(None, capi.CHIP_DISP_S16, Q) == capi.CHIP_ERR_INVALID_ARG
    wide = fc.frame(rng, SLOT_KP + 1)
    assert status_of(chip.frame_put_disparity, 1, wide, disp, DC.Q_EUROC) == capi.CHIP_ERR_UNSUPPORTED   # more keypoints than a slot holds
    assert status_of(chip.frame_put_disparity, 1, f, np.zeros((2, 16385), np.int16), DC.Q_EUROC) == capi.CHIP_ERR_UNSUPPORTED
    after = chip.frame_read(1)                                        # a failed put leaves the store as it was
    assert all(same_bytes(before[k], after[k]) for k in ("desc", "kp", "pts")) and chip.frame_store_info()["n_frames"] == 1
    # a full store: OOM, nothing evicted; a replace needs no free slot
    tiny = fc.frame(rng, 5)
    for i in range(10, 10 + N_SLOTS - 1):
        chip.frame_put_disparity(i, tiny, disp, DC.Q_EUROC)
    assert chip.frame_store_info()["n_frames"] == N_SLOTS
    assert status_of(chip.frame_put_disparity, 2, tiny, disp, DC.Q_EUROC) == capi.CHIP_ERR_OOM
    assert chip.frame_store_info()["n_frames"] == N_SLOTS and status_of(chip.frame_read, 2) == capi.CHIP_ERR_RANGE
    chip.frame_put_disparity(10, f, disp.astype(F), DC.Q_EUROC)
    assert D.same_floats(chip.frame_read(10)["pts"], before["pts"])   # int16 and the same values as floats: the same records
    chip.frame_drop(11)
    chip.frame_put_disparity(2, tiny, disp, DC.Q_EUROC)
    # the dense call
    out = np.zeros((fc.H, fc.W, 3), F)
    dense = lambda h, d, kind, w, hh, q, o: chip.lib.chip_disparity_to_xyz(h, d, kind, w, hh, q, o)   # noqa: E731
    dp, qp, op = capi._ptr(disp), capi._ptr(Q), capi._ptr(out)
    assert dense(chip.h, dp, capi.CHIP_DISP_S16, fc.W, fc.H, qp, op) == capi.CHIP_OK
    assert D.same_floats(out, D.xyz_from_disparity(disp, DC.Q_EUROC))
    assert dense(None, dp, 0, fc.W, fc.H, qp, op) == dense(chip.h, None, 0, fc.W, fc.H, qp, op) == capi.CHIP_ERR_INVALID_ARG
    assert dense(chip.h, dp, 0, fc.W, fc.H, None, op) == dense(chip.h, dp, 0, fc.W, fc.H, qp, None) == capi.CHIP_ERR_INVALID_ARG
    assert dense(chip.h, dp, 2, fc.W, fc.H, qp, op) == dense(chip.h, dp, -1, fc.W, fc.H, qp, op) == capi.CHIP_ERR_INVALID_ARG
    assert dense(chip.h, dp, 0, 0, fc.H, qp, op) == dense(chip.h, dp, 0, fc.W, -1, qp, op) == capi.CHIP_ERR_INVALID_ARG
    assert dense(chip.h, dp, 0, 16385, 1, qp, op) == dense(chip.h, dp, 0, 1, 16385, qp, op) == capi.CHIP_ERR_UNSUPPORTED


def test_before_a_reserve_and_on_a_group_ctx():
    rng = np.random.default_rng(24)
    f = fc.frame(rng, 40)
    disp = disparity(rng, "s16", fc.W, fc.H)
    with capi.Chip(4096) as c:
        assert status_of(c.frame_put_disparity, 1, f, disp, DC.Q_EUROC) == capi.CHIP_ERR_BUSY
        c.frame_store_reserve(2, 64)
        assert status_of(c.frame_put_disparity, 1, fc.frame(rng, 65), disp, DC.Q_EUROC) == capi.CHIP_ERR_UNSUPPORTED
        c.frame_put_disparity(1, f, disp, DC.Q_EUROC)
        assert D.same_floats(c.frame_read(1)["pts"], D.records(f["kp"], disp, DC.Q_EUROC))
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.frame_put_disparity, 1, f, disp, DC.Q_EUROC) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.disparity_to_xyz, disp, DC.Q_EUROC) == capi.CHIP_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 6: first use next to a resident scan
@pytest.mark.parametrize("first", ["dense", "put"])
def test_resident_tick_mode_allocates_inside_a_pause(monkeypatch, first):
    """with CHIP_TICK_RESIDENT=1 the first use of either call -- the stage's buffers, the staging buffer, the dense image -- happens
    next to a resident scan instance: same floats"""
    import scenarios
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "50")
    f = DC.frames()["s0"]
    with capi.Chip(4096) as c:
        c.append_synthetic(400, 5)
        ticks = scenarios.default_schedule(400)
        for l in ticks[:8]:
            c.loop_tick(l)
        if first == "dense":
            dense = c.disparity_to_xyz(f["disp"], DC.Q_PAIRS)
            c.loop_tick(ticks[8])
            c.frame_store_reserve(2, 512)
            c.frame_put_disparity(1, f, f["disp"], DC.Q_PAIRS)
        else:
            c.frame_store_reserve(2, 512)
            c.frame_put_disparity(1, f, f["disp"], DC.Q_PAIRS)
            c.loop_tick(ticks[8])
            dense = c.disparity_to_xyz(f["disp"], DC.Q_PAIRS)
        pts = c.frame_read(1)["pts"]
        c.loop_tick(400)
    assert D.same_floats(dense, DC.image_frames()["s0"]["xyz"])
    assert D.same_floats(pts, D.records(f["kp"], f["disp"], DC.Q_PAIRS))


# ---------------------------------------------------------------------------------------------- 7: the example
def test_frame_put_disparity_example():
    exe = LIB / "frame_put_disparity"
    assert exe.exists()
    r = subprocess.run([str(exe), "3000", "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("== the same frames put through chip_frame_put") == 6 and "DIFFERS" not in r.stdout
    assert r.stdout.count("three poses") >= 3
