"""GPU tests of the descriptor projection (cerebro_amd/csrc/project.hip; include/cerebro_hip.h "descriptor projection"): chip_project and
chip_db_append_projected_f32 against the restatement tests/np_mirror_project.py, for equality of bits -- at the shapes where the kernel
takes another path (one chunk, chunks that fill no batch of eight, whole batches, more outputs than resident waves, the LDS limit), at
the staging buffer's chunk boundary, and through the append's rules, ticks, statuses, device-memory input and the resident scan
instance."""
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import np_mirror_project as M
import oracle_lib
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"


@lru_cache(maxsize=None)
def case(in_dim, D, kind, seed=0):
    """(Mt, bias, x[4]) of one shape and matrix type: made once, shared, never written to.  x[2] is all zero: with a bias, a pure-bias row"""
    rng = np.random.default_rng(in_dim * 31 + D * 7 + seed + (kind == "f64"))
    Mt = rng.standard_normal((D, in_dim), dtype=np.float32) if kind == "f32" else rng.standard_normal((D, in_dim))
    b = rng.standard_normal(D)
    x = rng.standard_normal((4, in_dim), dtype=np.float32)
    x[2] = 0
    for a in (Mt, b, x):
        a.setflags(write=False)
    return Mt, b, x


def status_of(fn, *a, **k):
    try:
        fn(*a, **k)
    except capi.ChipError as e:
        return e.status
    return capi.CHIP_OK


# ---------------------------------------------------------------------------------------------- 1: chip_project == the definition
# (256, 4): one chunk per row (float) / two (double), fewer outputs than one workgroup's waves, the smallest D chip_create takes;
# (768, 256): three / six chunks, none of them in a batch of eight; (512, 10240): more outputs than resident waves (16 per CU);
# (32768, 256): whole batches only, the LDS limit
@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("in_dim,D", [(256, 4), (256, 68), (768, 256), (512, 10240), (32768, 256)])
def test_project_equals_the_definition(in_dim, D, kind):
    Mt, b, x = case(in_dim, D, kind)
    with capi.Chip(D) as chip:
        for bias in (None, b):
            chip.project_set(Mt, bias)
            assert chip.project_info() == dict(in_dim=in_dim, matrix_type=capi.CHIP_PROJ_F32 if kind == "f32" else capi.CHIP_PROJ_F64,
                                               has_bias=bias is not None)
            rows = x[[0, 1, 2]] if bias is not None else x[[0, 1, 3]]          # without a bias an all-zero x is NaN: test 4
            want = M.project(rows, Mt, bias)[1]
            assert np.isfinite(want).all()
            got3 = chip.project(rows)
            assert got3.shape == (3, D) and M.same_bits(got3, want), (in_dim, D, kind, bias is not None)
            assert M.same_bits(chip.project(rows[0]), want[:1])                 # n == 1
        assert chip.size() == 0                                                 # chip_project appends nothing


def test_chunk_boundary_of_the_staging_buffer():
    """n one more than the staging buffer holds at this D: 64 MiB / (10240 * 8 B) = 819 rows, so row 819 is a chunk of its own"""
    in_dim, D = 256, 10240
    n = (64 << 20) // (D * 8) + 1
    assert n == 820
    Mt, b, _ = case(in_dim, D, "f32")
    x = np.random.default_rng(5).standard_normal((n, in_dim), dtype=np.float32)
    want = M.project(x, Mt, b)[1]
    with capi.Chip(D) as chip:
        chip.project_set(Mt, b)
        assert M.same_bits(chip.project(x), want)
        assert chip.append_projected(x) == 0 and chip.size() == n
        at = [0, 1, 817, 818, 819]
        assert M.same_bits(chip.read_rows_f64(at), want[at])


# ---------------------------------------------------------------------------------------------- 2: the append
def test_append_projected_equals_append_f64_of_project():
    in_dim, D = 512, 256
    Mt, b, _ = case(in_dim, D, "f64")
    x = np.random.default_rng(9).standard_normal((7, in_dim), dtype=np.float32)
    want = M.project(x, Mt, b)[1]
    with capi.Chip(D) as a, capi.Chip(D) as ref:
        a.project_set(Mt, b)
        z = a.project(x)
        assert M.same_bits(z, want)
        assert a.append_projected(x[:3]) == 0 and a.append_projected(x[3:]) == 3
        assert a.append_projected(np.zeros((0, in_dim), np.float32)) == 7       # n == 0: CHIP_OK, first_index filled
        assert ref.append_f64(z[:3]) == 0 and ref.append_f64(z[3:]) == 3
        ia, ir = a.info(), ref.info()
        assert ia["storage_bytes"] == 8                                         # the undecided DB became a double-row DB
        for f in ("storage_bytes", "rows_global", "rows_local", "capacity_local", "lossy_rows", "row_norm_max", "D"):
            assert ia[f] == ir[f], f
        assert M.same_bits(a.read_rows_f64(range(7)), ref.read_rows_f64(range(7))) and M.same_bits(a.read_rows_f64(range(7)), want)


def test_append_edge_cases():
    in_dim, D = 256, 68
    Mt, b, x4 = case(in_dim, D, "f32")
    x = np.array(x4[[0, 1, 3]])
    want = M.project(x, Mt, b)[1]
    assert (want.astype(np.float32).astype(np.float64) != want).any()
    with capi.Chip(D, storage="f32") as chip:                                   # float rows, nothing appended: refused
        chip.project_set(Mt, b)
        assert status_of(chip.append_projected, x) == capi.CHIP_ERR_NOT_F32 and chip.size() == 0
        # the caller vouches: the rows are float32(z)
        assert chip.append_projected(x, flags=capi.CHIP_APPEND_ALLOW_ROUNDING) == 0 and chip.size() == 3
        assert chip.info()["lossy_rows"] == 3
        assert np.array_equal(chip.read_rows(range(3)).view(np.uint32), want.astype(np.float32).view(np.uint32))
    with capi.Chip(D) as chip:                                                  # an undecided DB with the flag stays a float DB
        chip.project_set(Mt, b)
        assert chip.append_projected(x, flags=capi.CHIP_APPEND_ALLOW_ROUNDING) == 0
        assert chip.info()["storage_bytes"] == 4 and chip.info()["lossy_rows"] == 3
        assert np.array_equal(chip.read_rows(range(3)).view(np.uint32), want.astype(np.float32).view(np.uint32))
    with capi.Chip(D) as chip:
        chip.project_set(Mt, None)
        bad = x.copy()
        bad[1, 100] = np.nan
        assert status_of(chip.append_projected, bad[1]) == capi.CHIP_ERR_NONFINITE and chip.size() == 0      # a NaN in x
        assert status_of(chip.append_projected, np.zeros(in_dim, np.float32)) == capi.CHIP_ERR_NONFINITE     # r == 0
        assert status_of(chip.append_projected, bad) == capi.CHIP_ERR_NONFINITE and chip.size() == 0          # the middle row of a batch
        bad[1] = 0
        assert status_of(chip.append_projected, bad) == capi.CHIP_ERR_NONFINITE and chip.size() == 0
        assert np.isnan(chip.project(bad)[1]).all() and np.isfinite(chip.project(bad)[[0, 2]]).all()           # nothing is special-cased
        assert chip.append_projected(x) == 0 and chip.size() == 3                                              # and the ctx is as good as new
        assert M.same_bits(chip.read_rows_f64(range(3)), M.project(x, Mt, None)[1])


def test_ticks_over_a_projected_db_equal_the_oracle():
    """200 raw descriptors with planted revisits (runs of four noisy copies of the descriptors 70 keyframes back): every tick over the
    projected DB equals the oracle's double-row tick over the mirror's rows"""
    in_dim, D, N = 512, 256, 200
    Mt, b, _ = case(in_dim, D, "f32", seed=1)
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, in_dim), dtype=np.float32)
    for i in range(80, N):
        if i % 20 < 4:
            x[i] = x[i - 70] + 0.05 * rng.standard_normal(in_dim, dtype=np.float32)
    want = M.project(x, Mt, b)[1]
    orc = oracle_lib.LoopOracle64(want)
    with capi.Chip(D) as chip:
        chip.project_set(Mt, b)
        for i in range(0, N, 40):
            assert chip.append_projected(x[i:i + 40]) == i
        assert chip.info()["storage_bytes"] == 8
        found = 0
        for l in range(1, N + 1):
            g, o = chip.loop_tick(l).as_dict(), orc.tick(l)
            assert g == o, (l, g, o)
            found += g["found"]
        assert found >= 3


# ---------------------------------------------------------------------------------------------- 3: statuses that need a ctx
def test_ctx_dependent_statuses():
    in_dim, D = 256, 68
    Mt, b, x4 = case(in_dim, D, "f32")
    Mt2 = case(in_dim, D, "f64")[0]
    x = x4[:2]
    BUSY, UNSUPPORTED = capi.CHIP_ERR_BUSY, capi.CHIP_ERR_UNSUPPORTED
    p = capi._ptr
    z = np.zeros((2, D))
    with capi.Chip(D) as chip:
        assert chip.project_info() == dict(in_dim=0, matrix_type=0, has_bias=False)
        assert status_of(chip.project, x) == BUSY and status_of(chip.append_projected, x) == BUSY
        assert chip.lib.chip_project(chip.h, p(x), 0, p(z)) == BUSY             # BUSY is decided before n == 0
        assert chip.lib.chip_db_append_projected_f32(chip.h, p(x), 0, 0, None) == BUSY
        chip.project_clear()                                                    # nothing to clear is fine
        chip.project_set(Mt, b)
        z1 = chip.project(x)
        chip.project_set(Mt2, None)                                             # a second set replaces the projection
        z2 = chip.project(x)
        assert M.same_bits(z1, M.project(x, Mt, b)[1]) and M.same_bits(z2, M.project(x, Mt2, None)[1]) and not M.same_bits(z1, z2)
        assert status_of(chip.project_set, Mt[:, :128]) == UNSUPPORTED          # in_dim 128: refused, the projection stays
        assert M.same_bits(chip.project(x), z2)
        chip.project_clear()
        assert chip.project_info()["in_dim"] == 0
        assert status_of(chip.project, x) == BUSY and status_of(chip.append_projected, x) == BUSY and chip.size() == 0
    with capi.Chip(D, devices=[0, 0]) as grp:                                   # a group ctx
        assert grp.lib.chip_project_set(grp.h, in_dim, p(Mt), capi.CHIP_PROJ_F32, None) == UNSUPPORTED
        assert grp.lib.chip_project(grp.h, p(x), 2, p(z)) == UNSUPPORTED
        assert grp.lib.chip_db_append_projected_f32(grp.h, p(x), 2, 0, None) == UNSUPPORTED
        assert grp.lib.chip_project_clear(grp.h) == UNSUPPORTED and grp.lib.chip_project_info(grp.h, None, None, None) == UNSUPPORTED
    with capi.Chip(D, shard_rank=0, shard_count=2) as sh:                       # a sharded ctx
        assert sh.lib.chip_project_set(sh.h, in_dim, p(Mt), capi.CHIP_PROJ_F32, None) == UNSUPPORTED
        assert sh.lib.chip_project(sh.h, p(x), 2, p(z)) == UNSUPPORTED
        assert sh.lib.chip_db_append_projected_f32(sh.h, p(x), 2, 0, None) == UNSUPPORTED
        assert sh.size() == 0


def test_device_memory_x_gives_the_bits_of_the_host_call():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the device-pointer form of x cannot be made here")
    in_dim, D = 768, 256
    Mt, b, x4 = case(in_dim, D, "f32")
    x = np.array(x4[[0, 1, 3]])
    with capi.Chip(D) as chip, capi.Chip(D) as ref:
        chip.project_set(Mt, b)
        ref.project_set(Mt, b)
        t = torch.from_numpy(x).to("cuda:0")
        torch.cuda.synchronize()                                                # the caller vouches that x is complete
        host = chip.project(x)
        assert M.same_bits(chip.project(t.data_ptr(), n=3), host) and M.same_bits(host, M.project(x, Mt, b)[1])
        assert chip.append_projected(t.data_ptr(), n=3) == 0 and ref.append_projected(x) == 0
        assert M.same_bits(chip.read_rows_f64(range(3)), ref.read_rows_f64(range(3)))
        del t


def test_project_set_pauses_the_resident_scan_instance(monkeypatch):
    """CHIP_TICK_RESIDENT=1: ticks before and after a chip_project_set (whose reserve frees and allocates device memory, which waits for
    the whole device) give the records of a run without it"""
    D, n_rows, seed = 4096, 9_000, 77
    plants = [(8_000 - j, 3_000 - j, 1) for j in range(3)]
    ls = [5_000, 8_001, 9_000]
    pr = capi.default_dot_params()
    pr.min_new = -(1 << 30)
    Mt, b, x4 = case(256, D, "f32")
    monkeypatch.delenv("CHIP_TICK_RESIDENT", raising=False)
    with capi.Chip(D, capacity_hint=n_rows) as ref:
        ref.append_synthetic(n_rows, seed, plants)
        want = [bytes(ref.loop_tick(l, pr)) for l in ls]
    assert sum(capi.TickResult.from_buffer_copy(w).found for w in want) >= 1
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", "3000")
    with capi.Chip(D, capacity_hint=n_rows) as chip:
        chip.append_synthetic(n_rows, seed, plants)
        assert [bytes(chip.loop_tick(l, pr)) for l in ls] == want
        chip.project_set(Mt, b)                                                 # the instance is alive here: the reserve pauses it
        assert [bytes(chip.loop_tick(l, pr)) for l in ls] == want
        z = chip.project(x4[:1])                                                # and a projection next to the waiting instance
        assert M.same_bits(z, M.project(x4[:1], Mt, b)[1])
        chip.project_clear()
        assert [bytes(chip.loop_tick(l, pr)) for l in ls] == want


def test_projected_append_next_to_a_live_resident_instance(monkeypatch):
    """The headline shape, 32768 -> 4096: project_rows needs 128 KiB of LDS on every CU, the resident instance's workgroup holds ~50 KiB
    there (float rows, D 4096), and 160 KiB is all a CU has -- so a projected append must PAUSE the instance, or its kernel waits until
    the instance's lease runs out (3 s here; for ever under ticks at 10 Hz).  The second append is the one that matters: it grows no
    buffer, so nothing but the call's own pause retires the instance.  It must take a small part of the lease, store the mirror's row,
    and leave the ticks as a run without the mode has them."""
    import time
    from test_resident_gpu import resident_stats
    D, in_dim, n_rows, seed, lease_ms = 4096, 32768, 2_000, 31, 3000
    rng = np.random.default_rng(4)
    Mt = np.tile(rng.standard_normal((D, 1024), dtype=np.float32), (1, in_dim // 1024))      # 512 MiB, made cheaply
    x = rng.standard_normal((2, in_dim), dtype=np.float32)
    want = M.project(x, Mt, None)[1].astype(np.float32)
    pr = capi.default_dot_params()
    pr.min_new = -(1 << 30)
    ROUND = capi.CHIP_APPEND_ALLOW_ROUNDING                                     # a float-row DB: the rows are float32(z)
    monkeypatch.delenv("CHIP_TICK_RESIDENT", raising=False)
    with capi.Chip(D, capacity_hint=n_rows + 8) as ref:
        ref.append_synthetic(n_rows, seed, [])
        ref.append_f64(want.astype(np.float64))
        ticks = [bytes(ref.loop_tick(l, pr)) for l in (n_rows, n_rows + 1, n_rows + 2)]
    monkeypatch.setenv("CHIP_TICK_RESIDENT", "1")
    monkeypatch.setenv("CHIP_RESIDENT_LEASE_MS", str(lease_ms))
    with capi.Chip(D, capacity_hint=n_rows + 8) as chip:
        chip.append_synthetic(n_rows, seed, [])
        chip.project_set(Mt, None)
        assert bytes(chip.loop_tick(n_rows, pr)) == ticks[0]                    # an instance is alive from here on
        assert chip.append_projected(x[0], flags=ROUND) == n_rows               # (grows the buffer of raw descriptors: pauses by itself)
        assert bytes(chip.loop_tick(n_rows + 1, pr)) == ticks[1]
        served, launched = resident_stats(chip)
        assert served == 2 and launched >= 2                                    # the ticks are commands to an instance, alive again now
        t0 = time.perf_counter()
        assert chip.append_projected(x[1], flags=ROUND) == n_rows + 1           # no reserve grows: the call's own pause
        dt = time.perf_counter() - t0
        assert dt < 1e-3 * lease_ms / 4, f"the projected append took {dt:.3f} s next to a live instance"
        z = chip.project(x[1])                                                  # and chip_project, the same way
        assert np.array_equal(z.astype(np.float32).view(np.uint32), want[1:].view(np.uint32))
        assert bytes(chip.loop_tick(n_rows + 2, pr)) == ticks[2]
        assert resident_stats(chip)[0] == 3
        assert np.array_equal(chip.read_rows([n_rows, n_rows + 1]).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 4: the example
def test_append_projected_example():
    exe = LIB / "append_projected"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout and r.stdout.count("0 differences") == 2
