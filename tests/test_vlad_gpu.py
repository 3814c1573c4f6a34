"""GPU tests of the NetVLAD pooling (cerebro_amd/csrc/vlad.hip; include/cerebro_hip.h "NetVLAD pooling"): chip_vlad and
chip_db_append_vlad_f32 against the restatement tests/np_mirror_vlad.py, for equality of bits -- the stages a, V, A through
chip_debug_vlad_stage first, so that a mismatch names the stage, then v -- at the shapes of tests/vlad_cases.py, in both layouts, on the
crafted softmax cases, with non-finite maps, device-memory maps, through both append routes, the statuses that need a ctx, next to a live
resident scan instance, and the example binary."""
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import np_mirror_vlad as M
import oracle_lib
import vlad_cases as T
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
NHWC, NCHW = capi.CHIP_VLAD_NHWC, capi.CHIP_VLAD_NCHW


def status_of(fn, *a, **k):
    try:
        fn(*a, **k)
    except capi.ChipError as e:
        return e.status
    return capi.CHIP_OK


def check_stages_then_v(chip, x, want, what):
    """both layouts: a, V, A of the call, then its v, against the mirror's"""
    N = x.shape[0]
    for layout, fm in ((NHWC, x), (NCHW, np.ascontiguousarray(x.T))):
        v = chip.vlad(fm, layout, positions=N)
        st = chip.debug_vlad_stage(N)
        for key in ("a", "V", "A"):
            assert M.same_bits(st[key], want[key]), (what, layout, key, M.first_difference(st[key], want[key]))
        assert M.same_bits(v, want["v"]), (what, layout, "v", M.first_difference(v, want["v"]))


# ---------------------------------------------------------------------------------------------- 1: chip_vlad == the definition
@pytest.mark.parametrize("N,C,K,G", T.SHAPES)
def test_pooling_equals_the_definition(N, C, K, G):
    x, Wt, bias, centres, want = T.shape_case(N, C, K, G)
    assert np.isfinite(want["v"]).all() and (want["v"] != 0).any()
    with capi.Chip(256) as chip:
        chip.vlad_set(Wt, bias, centres)
        assert chip.vlad_info() == dict(channels=C, clusters=K, ghost=G)
        check_stages_then_v(chip, x, want, (N, C, K, G))
        assert chip.size() == 0                                                 # chip_vlad appends nothing


@pytest.mark.parametrize("name", T.CRAFTED)
def test_crafted_softmax_cases(name):
    x, Wt, bias, centres, want = T.crafted_case(name)
    K, C = centres.shape
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        check_stages_then_v(chip, x, want, name)
        assert chip.append_vlad(x) == 0 and chip.size() == 1                    # the all-zero vector too is appended like any finite row
        assert M.same_bits(chip.read_rows_f64([0])[0], want["v"].astype(np.float64))
        if name == "zero_map":
            assert (chip.read_rows_f64([0]) == 0).all()


# ---------------------------------------------------------------------------------------------- 2: non-finite maps
def test_nonfinite_maps_are_refused_and_leave_the_db_unchanged():
    N, C, K, G = 65, 260, 16, 0
    x, Wt, bias, centres, want = T.shape_case(N, C, K, G)
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        assert chip.append_vlad(x) == 0
        before = chip.read_rows_f64([0])
        info = chip.info()
        for value, at in ((np.nan, (64, 259)), (np.inf, (0, 0)), (-np.inf, (17, 100))):
            bad = np.array(x)
            bad[at] = value
            for layout, fm in ((NHWC, bad), (NCHW, np.ascontiguousarray(bad.T))):
                assert status_of(chip.append_vlad, fm, layout, positions=N) == capi.CHIP_ERR_NONFINITE, (value, layout)
                assert status_of(chip.vlad, fm, layout, positions=N) == capi.CHIP_ERR_NONFINITE, (value, layout)
            assert chip.size() == 1 and chip.info() == info and M.same_bits(chip.read_rows_f64([0]), before)
        assert chip.append_vlad(x) == 1                                         # and the ctx is as good as new
        assert M.same_bits(chip.read_rows_f64([1]), before) and M.same_bits(before[0], want["v"].astype(np.float64))
    bad_w = np.array(Wt)
    bad_w[3, 7] = np.nan
    bad_b = np.array(bias)
    bad_b[0] = np.inf
    bad_c = np.array(centres)
    bad_c[15, 259] = -np.inf
    with capi.Chip(K * C) as chip:                                              # chip_vlad_set: a host check
        for args in ((bad_w, bias, centres), (Wt, bad_b, centres), (Wt, bias, bad_c)):
            assert status_of(chip.vlad_set, *args) == capi.CHIP_ERR_NONFINITE
        assert chip.vlad_info()["channels"] == 0


# ---------------------------------------------------------------------------------------------- 3: device-memory maps
def test_device_memory_map_gives_the_bits_of_the_host_call():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the device-pointer form of the map cannot be made here")
    N, C, K, G = 130, 1024, 8, 2
    x, Wt, bias, centres, want = T.shape_case(N, C, K, G)
    with capi.Chip(K * C) as chip, capi.Chip(K * C) as ref:
        chip.vlad_set(Wt, bias, centres)
        ref.vlad_set(Wt, bias, centres)
        t = torch.from_numpy(np.ascontiguousarray(x.T)).to("cuda:0")           # channels first, as a torch trunk emits it
        u = torch.from_numpy(np.array(x)).to("cuda:0")
        torch.cuda.synchronize()                                                # the caller vouches that the map is complete
        assert M.same_bits(chip.vlad(t.data_ptr(), NCHW, positions=N), want["v"])
        assert M.same_bits(chip.vlad(u.data_ptr(), NHWC, positions=N), want["v"])
        assert chip.append_vlad(t.data_ptr(), NCHW, positions=N) == 0 and chip.append_vlad(u.data_ptr(), NHWC, positions=N) == 1
        assert ref.append_vlad(x) == 0
        rows = chip.read_rows_f64([0, 1])
        assert M.same_bits(rows[0], ref.read_rows_f64([0])[0]) and M.same_bits(rows[1], rows[0])
        del t, u


# ---------------------------------------------------------------------------------------------- 4: the two routes of the append
def test_default_model_shape_appends_the_rows_of_append_f64_and_ticks_like_the_oracle():
    """1410 x 512, K = 16, D = 8192, float rows: 56 ready rows, then four pooled ones (two of them noisy copies of one map, each layout
    once); the DB equals the one made by chip_db_append_f64 of chip_vlad's output, field for field, and a tick over it the oracle's"""
    N, C, K, G, D = 1410, 512, 16, 0, 8192
    x, Wt, bias, centres, want = T.shape_case(N, C, K, G)
    rng = np.random.default_rng(3)
    ready = rng.standard_normal((56, D)).astype(np.float32)
    ready /= np.linalg.norm(ready.astype(np.float64), axis=1)[:, None].astype(np.float32)
    maps = [np.array(x), np.maximum(x + 0.01 * rng.standard_normal(x.shape).astype(np.float32), 0), np.array(T.fmap(N, C, seed=1)), np.array(x)]
    with capi.Chip(D) as chip, capi.Chip(D) as ref:
        chip.vlad_set(Wt, bias, centres)
        assert chip.append_f64(ready.astype(np.float64)) == 0 and ref.append_f64(ready.astype(np.float64)) == 0
        vs = []
        for i, m in enumerate(maps):
            v = chip.vlad(m)
            vs.append(v)
            fm, layout = (m, NHWC) if i % 2 == 0 else (np.ascontiguousarray(m.T), NCHW)
            assert chip.append_vlad(fm, layout, positions=N) == 56 + i
            assert ref.append_f64(v.astype(np.float64)[None, :]) == 56 + i
        assert M.same_bits(vs[0], want["v"]) and M.same_bits(vs[3], want["v"]) and not M.same_bits(vs[1], vs[0])
        ia, ir = chip.info(), ref.info()
        assert ia["storage_bytes"] == 4 and ia["lossy_rows"] == 0                # a float32 value always passes the float-row check
        for f in ("storage_bytes", "rows_global", "rows_local", "capacity_local", "lossy_rows", "row_norm_max", "D"):
            assert ia[f] == ir[f], f
        at = list(range(54, 60))
        got = chip.read_rows(at)
        assert np.array_equal(got.view(np.uint32), ref.read_rows(at).view(np.uint32))
        assert np.array_equal(got[2:].view(np.uint32), np.stack(vs).view(np.uint32))
        db = np.concatenate([ready, np.stack(vs)])
        orc_a, orc_b = oracle_lib.LoopOracle(db), None
        g, o = chip.loop_tick(60).as_dict(), orc_a.tick(60)
        assert g == o, (g, o)
        assert ref.loop_tick(60).as_dict() == o


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_relja_shape_equals_append_projected_of_the_pooled_vector(kind):
    """130 x 512, K = 64 -> 32768 -> D = 256 through a float and a double matrix"""
    N, C, K, G, D = 130, 512, 64, 0, 256
    x, Wt, bias, centres, want = T.shape_case(N, C, K, G)
    rng = np.random.default_rng(8)
    Mt = rng.standard_normal((D, K * C), dtype=np.float32)
    Mt = Mt if kind == "f32" else Mt.astype(np.float64) * (1 + 2.0 ** -40)
    b = rng.standard_normal(D)
    with capi.Chip(D) as chip, capi.Chip(D) as ref:
        chip.vlad_set(Wt, bias, centres)
        chip.project_set(Mt, b)
        ref.project_set(Mt, b)
        v = chip.vlad(x)
        assert M.same_bits(v, want["v"])
        assert chip.append_vlad(x) == 0 and chip.append_vlad(np.ascontiguousarray(x.T), NCHW, positions=N) == 1
        assert ref.append_projected(v) == 0 and ref.append_projected(v) == 1
        ia, ir = chip.info(), ref.info()
        for f in ("storage_bytes", "rows_global", "rows_local", "lossy_rows", "row_norm_max", "D"):
            assert ia[f] == ir[f], f
        assert ia["storage_bytes"] == 8
        assert M.same_bits(chip.read_rows_f64([0, 1]), ref.read_rows_f64([0, 1]))
        import np_mirror_project as MP
        assert M.same_bits(chip.read_rows_f64([0])[0], MP.project(want["v"], Mt, b)[1])


# ---------------------------------------------------------------------------------------------- 5: statuses that need a ctx
def test_ctx_dependent_statuses():
    N, C, K, G = 64, 256, 8, 2
    x, Wt, bias, centres, want = T.shape_case(N, C, K, G)
    x2, Wt2, bias2, centres2, want2 = T.shape_case(65, 260, 16, 0)
    BUSY, UNSUPPORTED = capi.CHIP_ERR_BUSY, capi.CHIP_ERR_UNSUPPORTED
    p = capi._ptr
    out = np.zeros(K * C, np.float32)
    with capi.Chip(K * C) as chip:
        assert chip.vlad_info() == dict(channels=0, clusters=0, ghost=0)
        assert chip.lib.chip_vlad(chip.h, p(x), N, NHWC, p(out)) == BUSY        # no weights
        assert chip.lib.chip_db_append_vlad_f32(chip.h, p(x), N, NHWC, 0, None) == BUSY
        assert chip.lib.chip_debug_vlad_stage(chip.h, None, None, None) == BUSY
        chip.vlad_clear()                                                       # nothing to clear is fine
        chip.vlad_set(Wt, bias, centres)
        assert chip.lib.chip_debug_vlad_stage(chip.h, None, None, None) == BUSY  # weights, but no pooling call yet
        v1 = chip.vlad(x)
        assert chip.append_vlad(x) == 0
        chip.vlad_set(Wt2, bias2, centres2)                                     # a second set replaces the weights
        assert chip.vlad_info() == dict(channels=260, clusters=16, ghost=0)
        v2 = chip.vlad(x2)
        assert M.same_bits(v1, want["v"]) and M.same_bits(v2, want2["v"])
        assert status_of(chip.append_vlad, x2) == UNSUPPORTED and chip.size() == 1       # K * C = 4160 against D = 2048
        assert status_of(chip.vlad_set, Wt2[:, :258], bias2, centres2[:, :258]) == UNSUPPORTED   # C = 258: refused, the weights stay
        assert M.same_bits(chip.vlad(x2), v2)
        chip.vlad_set(Wt, bias, centres)
        chip.project_set(np.ones((K * C, 512), np.float32))                     # a projection whose in_dim is not K * C = 2048
        assert status_of(chip.append_vlad, x) == UNSUPPORTED and chip.size() == 1
        chip.project_clear()
        assert chip.append_vlad(x) == 1
        assert M.same_bits(chip.read_rows_f64([1])[0], want["v"].astype(np.float64))
        chip.vlad_clear()
        assert chip.vlad_info()["channels"] == 0 and status_of(chip.append_vlad, x) == BUSY and chip.size() == 2
    with capi.Chip(K * C, devices=[0, 0]) as grp:                               # a group ctx
        assert grp.lib.chip_vlad_set(grp.h, C, K, G, p(Wt), p(bias), p(centres)) == UNSUPPORTED
        assert grp.lib.chip_vlad(grp.h, p(x), N, NHWC, p(out)) == UNSUPPORTED
        assert grp.lib.chip_db_append_vlad_f32(grp.h, p(x), N, NHWC, 0, None) == UNSUPPORTED
        assert grp.lib.chip_vlad_clear(grp.h) == UNSUPPORTED and grp.lib.chip_vlad_info(grp.h, None, None, None) == UNSUPPORTED
        assert grp.lib.chip_debug_vlad_stage(grp.h, None, None, None) == UNSUPPORTED
    with capi.Chip(K * C, shard_rank=0, shard_count=2) as sh:                   # a sharded ctx
        assert sh.lib.chip_vlad_set(sh.h, C, K, G, p(Wt), p(bias), p(centres)) == UNSUPPORTED
        assert sh.lib.chip_vlad(sh.h, p(x), N, NHWC, p(out)) == UNSUPPORTED
        assert sh.lib.chip_db_append_vlad_f32(sh.h, p(x), N, NHWC, 0, None) == UNSUPPORTED
        assert sh.size() == 0


# ---------------------------------------------------------------------------------------------- 6: next to a live resident instance
def test_pooled_append_next_to_a_live_resident_instance(monkeypatch):
    """CHIP_TICK_RESIDENT=1, D = 4096 = 16 x 256: the pooled append pauses the instance for its duration (vlad.hip vlad_pool says why).
    The second append is the one that matters: it grows no buffer, so nothing but the call's own pause retires the instance.  It must
    take a small part of the lease, store the mirror's row, and leave the ticks as a run without the mode has them."""
    from test_resident_gpu import resident_stats
    D, n_rows, seed, lease_ms = 4096, 2_000, 31, 3000
    N, C, K, G = 130, 256, 16, 0
    Wt, bias, centres = T.weights(C, K, G)
    maps = [T.fmap(N, C), T.fmap(N, C, seed=2)]
    want = np.stack([M.vlad(m, Wt, bias, centres)["v"] for m in maps])
    pr = capi.default_dot_params()
    pr.min_new = -(1 << 30)
    monkeypatch.delenv("CHIP_TICK_RESIDENT", raising=False)
    with capi.Chip(D, capacity_hint=n_rows + 8) as ref:
        ref.append_synthetic(n_rows, seed, [])
        ref.append_f64(want.astype(np.float64))
        ticks = [bytes(ref.loop_tick(l, pr)) for l in (n_rows, n_rows + 1, n_rows + 2)]
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", str(lease_ms))
    with capi.Chip(D, capacity_hint=n_rows + 8) as chip:
        chip.append_synthetic(n_rows, seed, [])
        chip.vlad_set(Wt, bias, centres)
        assert bytes(chip.loop_tick(n_rows, pr)) == ticks[0]                    # an instance is alive from here on
        assert chip.append_vlad(maps[0]) == n_rows                              # (grows the pooling's buffers: pauses by itself)
        assert bytes(chip.loop_tick(n_rows + 1, pr)) == ticks[1]
        served, launched = resident_stats(chip)
        assert served == 2 and launched >= 2                                    # the ticks are commands to an instance, alive again now
        t0 = time.perf_counter()
        assert chip.append_vlad(maps[1]) == n_rows + 1                          # no reserve grows: the call's own pause
        dt = time.perf_counter() - t0
        assert dt < 1e-3 * lease_ms / 4, f"the pooled append took {dt:.3f} s next to a live instance"
        assert M.same_bits(chip.vlad(maps[1]), want[1])                         # and chip_vlad, the same way
        assert bytes(chip.loop_tick(n_rows + 2, pr)) == ticks[2]
        assert resident_stats(chip)[0] == 3
        assert np.array_equal(chip.read_rows([n_rows, n_rows + 1]).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 7: the example
def test_append_vlad_example():
    exe = LIB / "append_vlad"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout and r.stdout.count("0 differences") == 2
