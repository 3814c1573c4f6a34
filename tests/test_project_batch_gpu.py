"""GPU tests of the shared passes of the descriptor projection (cerebro_amd/csrc/project.hip project_pass; include/cerebro_hip.h "batched
ingest"): chip_project and chip_db_append_projected_f32 over n > 1 descriptors against the restatement tests/np_mirror_project.py, for
equality of bits -- at the counts where the walk over the groups takes another turn (2, width - 1, width, width + 1, 2 width + 3), at the
shapes where the kernel takes another path (one chunk, chunks that fill no batch, a batch plus a tail, more rows than resident waves, the
LDS limit, in_dim around the planned slab), with NaN rows in the middle of a group, through the append's rules, at the staging buffer's
chunk boundary, with device-memory input and next to a resident scan instance."""
import os
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import np_mirror_project as M
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KIND = {"f32": capi.CHIP_PROJ_F32, "f64": capi.CHIP_PROJ_F64}
INFO_FIELDS = ("storage_bytes", "rows_global", "rows_local", "capacity_local", "lossy_rows", "row_norm_max", "D")


def width():
    return capi.project_plan(256, capi.CHIP_PROJ_F32, 0)["width"]


def counts():
    w = width()
    return sorted({2, w - 1, w, w + 1, 2 * w + 3})


@lru_cache(maxsize=None)
def case(in_dim, D, kind, n):
    """(Mt, bias, x[n], the mirror's rows without and with the bias) of one shape and matrix type: made once, shared, never written to"""
    rng = np.random.default_rng(in_dim * 31 + D * 7 + (kind == "f64"))
    Mt = rng.standard_normal((D, in_dim), dtype=np.float32) if kind == "f32" else rng.standard_normal((D, in_dim))
    b = rng.standard_normal(D)
    x = rng.standard_normal((n, in_dim), dtype=np.float32)
    want = {False: M.project(x, Mt, None)[1], True: M.project(x, Mt, b)[1]}
    for a in (Mt, b, x, want[False], want[True]):
        a.setflags(write=False)
    return Mt, b, x, want


def status_of(fn, *a, **k):
    try:
        fn(*a, **k)
    except capi.ChipError as e:
        return e.status
    return capi.CHIP_OK


def check_counts(chip, Mt, b, x, want, what):
    w = width()
    for bias in (False, True):
        chip.project_set(Mt, b if bias else None)
        for n in counts():
            got = chip.project(x[:n])
            assert got.shape == want[bias][:n].shape and M.same_bits(got, want[bias][:n]), (what, bias, n)
            last = chip.debug_project_last()
            assert last["width"] == w
            assert last["shared_passes"] + last["single_launches"] == -(-n // w), (what, n, last)
            assert last["single_launches"] == (1 if n % w == 1 else 0), (what, n, last)        # a trailing group of one
            assert last["shared_descriptors"] + last["single_descriptors"] == n, (what, n, last)
        assert M.same_bits(chip.project(x[:1]), want[bias][:1])                                # n == 1: the single launch, as ever
        last = chip.debug_project_last()
        assert (last["shared_passes"], last["single_launches"]) == (0, 1), last


# ---------------------------------------------------------------------------------------------- 1: chip_project(x[:n]) == the definition
# (256, 4): one chunk per row, fewer rows than one workgroup's waves; (768, 256): chunks that fill no batch of eight; (2304, 68): a batch
# plus a tail chunk; (512, 10240): more rows than resident waves (the workgroups walk several row groups and stage x again);
# (32768, 256): the LDS limit of the single launch, sixteen / thirty-two slabs of the shared pass
@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("in_dim,D", [(256, 4), (768, 256), (2304, 68), (512, 10240), (32768, 256)])
def test_groups_equal_the_definition(in_dim, D, kind):
    Mt, b, x, want = case(in_dim, D, kind, 2 * width() + 3)
    assert np.isfinite(want[False]).all() and np.isfinite(want[True]).all()
    with capi.Chip(D) as chip:
        check_counts(chip, Mt, b, x, want, (in_dim, D, kind))
        assert chip.size() == 0


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_in_dim_around_the_planned_slab(kind):
    """one in_dim just below, at and just above the slab chip_project_plan reports, and one that is several slabs and a part of one"""
    slab = capi.project_plan(256, KIND[kind], 2)["slab"]
    assert slab % 256 == 0 and slab >= 512
    D = 68
    for in_dim in (slab - 256, slab, slab + 256, 5 * slab + 768 if slab > 768 else 5 * slab + 256):
        assert capi.project_plan(in_dim, KIND[kind], 2)["slab"] == slab
        Mt, b, x, want = case(in_dim, D, kind, 2 * width() + 3)
        with capi.Chip(D) as chip:
            check_counts(chip, Mt, b, x, want, (in_dim, D, kind))


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_a_nan_row_in_the_middle_of_a_group_leaves_its_neighbours_alone(kind):
    in_dim, D = 2304, 68
    w = width()
    Mt, b, x, want = case(in_dim, D, kind, 2 * w + 3)
    mid = w // 2
    with capi.Chip(D) as chip:
        chip.project_set(Mt, None)
        for how in ("zero", "nan"):
            bad = np.array(x[:w])
            if how == "zero":
                bad[mid] = 0                                                    # without a bias: y == 0, r == 0, 0 / 0
            else:
                bad[mid, in_dim - 1] = np.nan
            got = chip.project(bad)
            assert np.isnan(got[mid]).all(), how
            others = [i for i in range(w) if i != mid]
            assert M.same_bits(got[others], want[False][others]), how


# ---------------------------------------------------------------------------------------------- 2: the append
def test_append_of_a_batch_equals_single_appends():
    in_dim, D = 768, 256
    n = 2 * width() + 3
    Mt, b, x, want = case(in_dim, D, "f64", n)
    with capi.Chip(D) as a, capi.Chip(D) as ref:
        a.project_set(Mt, b)
        ref.project_set(Mt, b)
        assert a.append_projected(x) == 0
        last = a.debug_project_last()
        assert (last["shared_passes"], last["single_launches"], last["shared_descriptors"]) == (3, 0, n)   # 2 width + 3: three groups
        for i in range(n):
            assert ref.append_projected(x[i]) == i
        last = ref.debug_project_last()
        assert (last["shared_passes"], last["single_launches"]) == (0, 1)
        ia, ir = a.info(), ref.info()
        for f in INFO_FIELDS:
            assert ia[f] == ir[f], f
        assert ia["storage_bytes"] == 8 and ia["rows_global"] == n
        rows = a.read_rows_f64(range(n))
        assert M.same_bits(rows, ref.read_rows_f64(range(n))) and M.same_bits(rows, want[True])


def test_a_refused_batch_appends_nothing():
    in_dim, D = 768, 256
    n = 2 * width() + 3
    Mt, b, x, want = case(in_dim, D, "f32", n)
    with capi.Chip(D) as chip:
        chip.project_set(Mt, b)
        assert chip.append_projected(x[:3]) == 0
        info = chip.info()
        bad = np.array(x)
        bad[n // 2, 5] = np.nan
        assert status_of(chip.append_projected, bad) == capi.CHIP_ERR_NONFINITE
        assert chip.size() == 3 and all(chip.info()[f] == info[f] for f in INFO_FIELDS)
        assert chip.append_projected(x[3:]) == 3 and chip.size() == n           # and the ctx is as good as new
        assert M.same_bits(chip.read_rows_f64(range(n)), want[True])


def test_chunk_boundary_of_the_staging_buffer_through_passes():
    """n one more than the staging buffer holds at this D: 64 MiB / (10240 * 8 B) = 819 rows in groups, then row 819 as a chunk -- and a
    single launch -- of its own"""
    in_dim, D = 256, 10240
    n = (64 << 20) // (D * 8) + 1
    assert n == 820
    w = width()
    Mt, b, _, _ = case(in_dim, D, "f32", 2 * w + 3)
    x = np.random.default_rng(5).standard_normal((n, in_dim), dtype=np.float32)
    want = M.project(x, Mt, b)[1]
    first, rest = 819 // w, 819 % w
    with capi.Chip(D) as chip:
        chip.project_set(Mt, b)
        assert M.same_bits(chip.project(x), want)
        last = chip.debug_project_last()
        assert last["shared_passes"] == first + (1 if rest > 1 else 0) and last["single_launches"] == (1 if rest == 1 else 0) + 1, last
        assert chip.append_projected(x) == 0 and chip.size() == n
        at = [0, 1, w - 1, w, 817, 818, 819]
        assert M.same_bits(chip.read_rows_f64(at), want[at])


def test_device_memory_x_gives_the_bits_of_the_host_call():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the device-pointer form of x cannot be made here")
    in_dim, D = 768, 256
    n = 2 * width() + 3
    Mt, b, x, want = case(in_dim, D, "f32", n)
    with capi.Chip(D) as chip:
        chip.project_set(Mt, b)
        t = torch.from_numpy(np.array(x)).to("cuda:0")
        torch.cuda.synchronize()                                                # the caller vouches that x is complete
        assert M.same_bits(chip.project(t.data_ptr(), n=n), want[True])
        assert chip.append_projected(t.data_ptr(), n=n) == 0
        assert M.same_bits(chip.read_rows_f64(range(n)), want[True])
        del t


RESIDENT_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import np_mirror_project as M
from cerebro_amd import capi
D, in_dim, n_rows = 4096, 256, 2000
w = capi.project_plan(in_dim, capi.CHIP_PROJ_F32, 0)["width"]
n = 2 * w + 3
rng = np.random.default_rng(12)
Mt = rng.standard_normal((D, in_dim), dtype=np.float32)
x = rng.standard_normal((n, in_dim), dtype=np.float32)
want = M.project(x, Mt, None)[1]
pr = capi.default_dot_params()
pr.min_new = -(1 << 30)
with capi.Chip(D, capacity_hint=n_rows + 64, storage="f64") as chip:
    chip.append_synthetic(n_rows, 31, [])
    chip.project_set(Mt, None)
    before = bytes(chip.loop_tick(n_rows, pr))                                  # an instance is alive from here on
    assert chip.append_projected(x) == n_rows                                   # (grows the buffer of raw descriptors: pauses by itself)
    assert chip.append_projected(x) == n_rows + n                               # no reserve grows: the call's own pause
    assert bytes(chip.loop_tick(n_rows, pr)) == before
    assert M.same_bits(chip.project(x), want)
    rows = chip.read_rows_f64(range(n_rows, n_rows + 2 * n))
    assert M.same_bits(rows[:n], want) and M.same_bits(rows[n:], want)
    last = chip.debug_project_last()
    assert (last["shared_passes"], last["single_launches"]) == (3, 0), last
print("resident child ok")
"""


def test_batches_next_to_a_live_resident_instance():
    """CHIP_TICK_RESIDENT=1, in a process of its own: the shared pass fills every CU with a 1024-thread workgroup as the single launch
    does, so the calls pause the instance; the rows are the mirror's and a tick before and after is the same record"""
    env = dict(os.environ, CHIP_TICK_RESIDENT="1", CHIP_RESIDENT_LEASE_MS="3000")
    r = subprocess.run([sys.executable, "-c", RESIDENT_CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "resident child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
