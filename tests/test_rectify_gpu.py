"""GPU parity of the rectification (cerebro_amd/csrc/frames.hip: rectify_pair behind chip_remap, chip_rectify_pair and
chip_frame_put_raw_orb_stereo) through ctypes -> C ABI against the numpy restatement (tests/np_mirror_rectify.py).  Everything is
compared for equality: images byte for byte, a frame put from its raw pair against the same frame put from the pair chip_rectify_pair
makes of it, row for row.  The definition is this project's own and is not pinned against OpenCV."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import disparity_cases as DSP
import np_mirror_rectify as R
import orb_detect_cases as OC
import rectify_cases as RC
import stereo_bm_cases as SC
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
Q = DSP.Q_EUROC
# widths of all residues mod the pixels of a thread around a workgroup's span of a row, heights around its rows, and the smallest images
SHAPES = tuple((w, h) for w in range(RC.WG_ROW_SPAN - 1, RC.WG_ROW_SPAN + RC.PIXELS_PER_THREAD)
               for h in (RC.WG_ROWS - 1, RC.WG_ROWS, RC.WG_ROWS + 1)) + ((1, 1), (2, 1), (1, 2), (3, 2), (5, 1), (2 * RC.WG_ROW_SPAN + 6, 9))
ORB_PUT = dict(n_levels=3, n_features=400, border=16)


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(4096) as c:
        yield c


def status_of(call, *args, **kw):
    with pytest.raises(capi.ChipError) as e:
        call(*args, **kw)
    return e.value.status


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_frames(a: dict, b: dict):
    return (a["n"], a["width"], a["height"]) == (b["n"], b["width"], b["height"]) and all(same_bytes(a[k], b[k]) for k in ("desc", "kp", "pts"))


def test_shapes_cover_every_residue():
    assert {w % RC.PIXELS_PER_THREAD for w, _ in SHAPES[:15]} == set(range(RC.PIXELS_PER_THREAD)) and RC.WG_ROW_SPAN % RC.PIXELS_PER_THREAD == 0


# ---------------------------------------------------------------------------------------------- 1: one stage, the caller's maps
@pytest.mark.parametrize("name", RC.FAMILIES)
def test_remap_equals_mirror(chip, name):
    for w, h in SHAPES:
        img = RC.image(w, h)
        mx, my = RC.family(name, w, h)
        got = chip.remap(img, mx, my)
        assert same_bytes(got, R.remap(img, mx, my)), (name, w, h)


def test_remap_at_the_edges_on_the_halves_and_through_special_values(chip):
    for w, h in ((13, 9), (104, 1), (RC.WG_ROW_SPAN + 1, 5)):
        img = np.full((h, w), 255, np.uint8) if h == 1 else RC.image(w, h)
        mx, my = RC.tap_edges(w, h)
        assert same_bytes(chip.remap(img, mx, my), R.remap(img, mx, my)), (w, h)
    img, mx, my, n = RC.half_case()
    got = chip.remap(img, mx, my)
    assert same_bytes(got, R.remap(img, mx, my)) and got[0, 0] == 1                              # taps (0, 1) at a = 16: the half goes up
    e = RC.quantiser_edges()
    w = len(e)
    img = RC.image(w, 3)
    mx, my = np.tile(e, (3, 1)), np.tile(np.float32([0.0, 1.5, float("nan")])[:, None], (1, w))
    assert same_bytes(chip.remap(img, mx, my), R.remap(img, mx, my))
    assert same_bytes(chip.remap(img, my + np.arange(w, dtype=np.float32), np.tile(e, (3, 1))), R.remap(img, my + np.arange(w, dtype=np.float32), np.tile(e, (3, 1))))


# ---------------------------------------------------------------------------------------------- 2: both eyes, both stages, one launch
def pair_cases():
    out = []
    for w, h in ((RC.WG_ROW_SPAN + 5, RC.WG_ROWS + 3), (64, 48), (13, 9)):
        out.append((f"two_stages_{w}x{h}", RC.image(w, h), RC.image(w, h, 1), RC.radtan(w, h) + RC.rotation(w, h),
                    RC.radtan(w, h, k1=-0.2, p1=-3e-4) + RC.rotation(w, h, -0.012, 0.01, -0.02)))
        out.append((f"one_stage_{w}x{h}", RC.image(w, h), RC.image(w, h, 1), RC.radtan(w, h), RC.rotation(w, h)))
        out.append((f"random_{w}x{h}", RC.image(w, h), RC.image(w, h, 1), RC.random_map(w, h, 1) + RC.random_map(w, h, 2),
                    RC.random_map(w, h, 3) + RC.random_map(w, h, 4)))
        out.append((f"tap_edges_{w}x{h}", RC.image(w, h), np.full((h, w), 255, np.uint8), RC.tap_edges(w, h) + RC.random_map(w, h, 5),
                    RC.random_map(w, h, 6) + RC.tap_edges(w, h)))
        out.append((f"tap_edges_one_stage_{w}x{h}", RC.image(w, h), np.full((h, w), 255, np.uint8), RC.tap_edges(w, h), RC.identity(w, h)))
    c = RC.half_u_case()
    out.append(("half_u", c["raw"], np.flipud(c["raw"]).copy(), c["s1"] + c["s2"], c["s2"] + c["s1"]))
    return out


@pytest.mark.parametrize("case", pair_cases(), ids=lambda c: c[0])
def test_rectify_pair_equals_remap_twice_equals_mirror(chip, case):
    name, lraw, rraw, lm, rm = case
    chip.rectify_set_maps(lm, rm)
    got = chip.rectify_pair(lraw, rraw)
    for eye, raw, m in zip(got, (lraw, rraw), (lm, rm)):
        twice = chip.remap(raw, *m[:2])
        if len(m) == 4:
            twice = chip.remap(twice, *m[2:])
        assert same_bytes(eye, twice) and same_bytes(eye, R.rectify(raw, *m)), name
    if name == "half_u":
        c = RC.half_u_case()
        assert got[0][c["at"]] == c["rounded"] != c["unrounded"]                                 # U went into stage 2 as a byte


def test_replacing_the_maps_takes_effect():
    w, h = 70, 40
    l, r = RC.image(w, h), RC.image(w, h, 1)
    a, b = RC.radtan(w, h) + RC.rotation(w, h), RC.random_map(w, h, 8) + RC.random_map(w, h, 9)
    with capi.Chip(4096) as ctx:
        ctx.rectify_set_maps(a, b)
        first = ctx.rectify_pair(l, r)
        ctx.rectify_set_maps(b, a)                                                               # other content
        second = ctx.rectify_pair(l, r)
        ctx.rectify_set_maps(a[:2], b[:2])                                                       # two stages -> one
        third = ctx.rectify_pair(l, r)
        big = (RC.radtan(150, 90), RC.rotation(150, 90))                                         # another size: the old one is refused
        ctx.rectify_set_maps(*big)
        assert status_of(ctx.rectify_pair, l, r) == capi.CHIP_ERR_INVALID_ARG
        L, Rr = RC.image(150, 90), RC.image(150, 90, 1)
        fourth = ctx.rectify_pair(L, Rr)
        ctx.rectify_set_maps(a, b)                                                               # and back to the smaller one
        assert status_of(ctx.rectify_pair, L, Rr) == capi.CHIP_ERR_INVALID_ARG
        fifth = ctx.rectify_pair(l, r)
    assert same_bytes(first[0], R.rectify(l, *a)) and same_bytes(first[1], R.rectify(r, *b))
    assert same_bytes(second[0], R.rectify(l, *b)) and same_bytes(second[1], R.rectify(r, *a))
    assert same_bytes(third[0], R.rectify(l, *a[:2])) and same_bytes(third[1], R.rectify(r, *b[:2]))
    assert same_bytes(fourth[0], R.rectify(L, *big[0])) and same_bytes(fourth[1], R.rectify(Rr, *big[1]))
    assert same_bytes(fifth[0], first[0]) and same_bytes(fifth[1], first[1]) and not same_bytes(first[0], second[0])


def test_statuses_without_maps_and_on_a_group_ctx():
    w, h = 40, 30
    l, r = RC.image(w, h), RC.image(w, h, 1)
    m = RC.identity(w, h)
    with capi.Chip(4096) as ctx:
        assert status_of(ctx.rectify_pair, l, r) == capi.CHIP_ERR_BUSY                           # no frame state at all
        assert same_bytes(ctx.remap(l, *m), l)                                                   # needs no maps and no store
        assert status_of(ctx.rectify_pair, l, r) == capi.CHIP_ERR_BUSY                           # no maps
        ctx.frame_store_reserve(2, 400)
        assert status_of(ctx.frame_put_raw_orb_stereo, 1, l, r, Q, ORB_PUT) == capi.CHIP_ERR_BUSY
        ctx.rectify_set_maps(m, m)
        assert status_of(ctx.rectify_pair, RC.image(w + 1, h), RC.image(w + 1, h)) == capi.CHIP_ERR_INVALID_ARG
        assert status_of(ctx.rectify_pair, RC.image(h, w), RC.image(h, w)) == capi.CHIP_ERR_INVALID_ARG   # the same area
        got = ctx.rectify_pair(l, r)
        assert same_bytes(got[0], l) and same_bytes(got[1], r)
        assert ctx.frame_store_info()["n_frames"] == 0
    with capi.Chip(4096, devices=[0, 0]) as grp:
        assert status_of(grp.remap, l, *m) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.rectify_set_maps, m, m) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.rectify_pair, l, r) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(grp.frame_put_raw_orb_stereo, 1, l, r, Q, ORB_PUT) == capi.CHIP_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 3: a frame straight from its raw pair
@pytest.mark.parametrize("size", ((160, 120), (320, 240)))
def test_put_from_the_raw_pair_equals_rectify_then_put(size):
    p = RC.warped_pair(*size)
    with capi.Chip(4096) as ctx:
        ctx.frame_store_reserve(3, 512)
        ctx.rectify_set_maps(p["left"], p["right"])
        n = ctx.frame_put_raw_orb_stereo(1, p["left_raw"], p["right_raw"], Q, ORB_PUT, SC.PAIR_PARAMS)
        left, right = ctx.rectify_pair(p["left_raw"], p["right_raw"])
        m = ctx.frame_put_orb_stereo(2, left, right, Q, ORB_PUT, SC.PAIR_PARAMS)
        a, b = ctx.frame_read(1), ctx.frame_read(2)
        # a replace under the same id: first by another frame, then by the raw pair again
        assert ctx.frame_put_raw_orb_stereo(1, p["right_raw"], p["left_raw"], Q, ORB_PUT, SC.PAIR_PARAMS) > 0
        swapped = ctx.frame_read(1)
        again = ctx.frame_put_raw_orb_stereo(1, p["left_raw"], p["right_raw"], Q, dict(ORB_PUT), SC.PAIR_PARAMS)
        c = ctx.frame_read(1)
        flat = OC.flat(*size)
        assert ctx.frame_put_raw_orb_stereo(3, flat, flat, Q, ORB_PUT, SC.PAIR_PARAMS) == 0      # a flat image: present and empty
        e = ctx.frame_read(3)
        assert ctx.frame_store_info()["n_frames"] == 3
    assert same_bytes(left, R.rectify(p["left_raw"], *p["left"])) and same_bytes(right, R.rectify(p["right_raw"], *p["right"]))
    assert n == m == again == a["n"] > 100 and same_frames(a, b) and same_frames(c, b) and not same_frames(swapped, b)
    assert (a["pts"][:, 3] == 1.0).any()
    assert e["n"] == 0 and (e["width"], e["height"]) == size


def test_raw_put_statuses_and_failure_rules():
    p = RC.warped_pair(160, 120)
    l, r = p["left_raw"], p["right_raw"]
    ptr, Qd = capi._ptr, np.ascontiguousarray(Q, dtype=np.float64).reshape(16)
    n = capi.C.c_int32(-7)
    with capi.Chip(4096) as ctx:
        put = ctx.frame_put_raw_orb_stereo
        assert status_of(put, 1, l, r, Q, ORB_PUT) == capi.CHIP_ERR_BUSY                        # no reserve
        ctx.rectify_set_maps(p["left"], p["right"])
        assert status_of(put, 1, l, r, Q, ORB_PUT) == capi.CHIP_ERR_BUSY                        # maps, still no reserve
        ctx.frame_store_reserve(2, 300)
        small = RC.image(80, 70)
        assert status_of(put, 1, small, small, Q, ORB_PUT) == capi.CHIP_ERR_INVALID_ARG         # not the maps' size
        assert status_of(put, 1, l, r, Q, dict(ORB_PUT, n_features=301)) == capi.CHIP_ERR_UNSUPPORTED   # more than a slot holds
        assert status_of(put, 1, l, r, Q, None) == capi.CHIP_ERR_UNSUPPORTED                    # the defaults' 5000 as well
        assert status_of(put, 1, l, r, Q, dict(ORB_PUT, border=15)) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(put, 1, l, r, Q, ORB_PUT, dict(SC.PAIR_PARAMS, block_size=4)) == capi.CHIP_ERR_UNSUPPORTED
        raw = ctx.lib.chip_frame_put_raw_orb_stereo
        o = capi.default_orb_params(**dict(ORB_PUT, n_features=300))
        assert raw(ctx.h, 1, 160, 120, ptr(l), None, capi.C.byref(o), None, ptr(Qd), capi.C.byref(n)) == capi.CHIP_ERR_INVALID_ARG
        assert raw(ctx.h, 1, 160, 120, ptr(l), ptr(r), capi.C.byref(o), None, ptr(Qd), None) == capi.CHIP_ERR_INVALID_ARG
        assert ctx.frame_store_info()["n_frames"] == 0 and n.value == -7                        # a refused put stores nothing
        orb = dict(ORB_PUT, n_features=300)
        assert put(1, l, r, Q, orb) == 300 == put(2, r, l, Q, orb)                              # the slot holds exactly what is kept
        assert status_of(put, 3, l, r, Q, orb) == capi.CHIP_ERR_OOM                             # a full store
        before = ctx.frame_read(1)
        assert status_of(put, 1, l, r, Q, dict(orb, n_features=301)) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(put, 1, small, small, Q, orb) == capi.CHIP_ERR_INVALID_ARG
        assert same_frames(ctx.frame_read(1), before)                                           # a refused replace leaves the frame
        assert put(2, l, r, Q, dict(orb, n_features=50)) == 50                                  # a known id replaces in a full store
        assert ctx.frame_store_info()["n_frames"] == 2


# ---------------------------------------------------------------------------------------------- 4: the example
def test_frame_put_raw_stereo_example():
    exe = LIB / "frame_put_raw_stereo"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout
