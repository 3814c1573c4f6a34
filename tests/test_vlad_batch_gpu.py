"""GPU tests of the batched NetVLAD pooling (cerebro_amd/csrc/vlad.hip; include/cerebro_hip.h "batched ingest"): chip_vlad_batch and
chip_db_append_vlad_batch_f32 against the restatement tests/np_mirror_vlad.py, map by map, and against the single calls, for equality
of bits -- at the map counts where the walk over the groups takes another turn (1, 2, 3, 16, 17, 33), at positions where a map's last
64-position block is ragged (a block that straddled two maps would show there), in both layouts, at the largest map (groups of two and
a last group of one), through a projection with shared matrix passes, with a non-finite map in the middle, from a torch tensor."""
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import np_mirror_project as MP
import np_mirror_vlad as M
import vlad_cases as T
from cerebro_amd import capi

pytestmark = pytest.mark.gpu
LIB = Path(__file__).resolve().parent.parent / "cerebro_amd" / "lib"
NHWC, NCHW = capi.CHIP_VLAD_NHWC, capi.CHIP_VLAD_NCHW
COUNTS = (1, 2, 3, 16, 17, 33)
INFO_FIELDS = ("storage_bytes", "rows_global", "rows_local", "capacity_local", "lossy_rows", "row_norm_max", "D")


def status_of(fn, *a, **k):
    try:
        fn(*a, **k)
    except capi.ChipError as e:
        return e.status
    return capi.CHIP_OK


@lru_cache(maxsize=None)
def one_map(N, C, m):
    """map m of the batches of this shape: made once, shared, never written to"""
    return T.fmap(N, C, seed=100 + m)


@lru_cache(maxsize=None)
def mirror(N, C, K, G, m):
    return M.vlad(one_map(N, C, m), *T.weights(C, K, G))


def batch(B, N, C):
    return np.stack([one_map(N, C, m) for m in range(B)])


def as_layout(maps, layout):
    return maps if layout == NHWC else np.ascontiguousarray(maps.transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------- 1: the batch == the definition, map by map
# (4, 1, 0): one cluster, one ragged 64-channel slice; (64, 16, 0) and (512, 16, 0): the default model's K; (1024, 8, 0): four float4 per
# lane of the score tree; (64, 60, 8): more than 64 score rows, the last group of eight clusters ragged
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("C,K,G", [(4, 1, 0), (64, 16, 0), (512, 16, 0), (1024, 8, 0), (64, 60, 8)])
def test_batches_equal_the_definition_and_the_single_calls(C, K, G, N):
    Wt, bias, centres = T.weights(C, K, G)
    maps = batch(max(COUNTS), N, C)
    want = np.stack([mirror(N, C, K, G, m)["v"] for m in range(max(COUNTS))])
    assert np.isfinite(want).all() and (want != 0).any()
    with capi.Chip(K * C) as chip, capi.Chip(K * C) as ref:
        chip.vlad_set(Wt, bias, centres)
        ref.vlad_set(Wt, bias, centres)
        rows = 0
        for i, B in enumerate(COUNTS):
            layout = (NHWC, NCHW)[i % 2]
            for lay in (layout, NHWC + NCHW - layout) if B in (3, 17) else (layout,):     # both layouts at every count over the cases
                v = chip.vlad_batch(as_layout(maps[:B], lay), lay, positions=N)
                assert v.shape == (B, K * C) and M.same_bits(v, want[:B]), (B, lay, M.first_difference(v, want[:B]))
                st = chip.debug_vlad_stage(N)                                             # the stages of the call's last map
                for key in ("a", "V", "A"):
                    assert M.same_bits(st[key], mirror(N, C, K, G, B - 1)[key]), (B, lay, key)
            assert chip.append_vlad_batch(as_layout(maps[:B], layout), layout, positions=N) == rows
            rows += B
            assert chip.size() == rows
        assert chip.append_vlad_batch(np.zeros((0, N, C), np.float32), positions=N, n_maps=0) == rows      # n_maps == 0: CHIP_OK, first_index filled
        assert chip.vlad_batch(np.zeros((0, N, C), np.float32), positions=N, n_maps=0).shape == (0, K * C)
        got = chip.read_rows_f64(range(rows))
        at = 0
        for B in COUNTS:
            assert M.same_bits(got[at:at + B], want[:B].astype(np.float64)), B
            at += B
        # the loop of single calls: the same vectors, the same DB
        for m in range(3):
            assert M.same_bits(ref.vlad(maps[m]), want[m])
        for B in COUNTS:
            for m in range(B):
                ref.append_vlad(maps[m] if m % 2 else np.ascontiguousarray(maps[m].T), NHWC if m % 2 else NCHW, positions=N)
        ia, ir = chip.info(), ref.info()
        for f in INFO_FIELDS:
            assert ia[f] == ir[f], f
        assert M.same_bits(got, ref.read_rows_f64(range(rows)))


def test_the_largest_map_goes_in_groups_of_two_and_a_last_group_of_one():
    """positions 16384: 32768 / 16384 = 2 maps per group, so three maps are a group of two and a group of ONE map (more positions than
    that are refused, as the single call refuses them)"""
    N, C, K, G = capi.CHIP_VLAD_MAX_POSITIONS, 4, 1, 0
    Wt, bias, centres = T.weights(C, K, G)
    maps = batch(3, N, C)
    want = np.stack([mirror(N, C, K, G, m)["v"] for m in range(3)])
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        for layout in (NHWC, NCHW):
            assert M.same_bits(chip.vlad_batch(as_layout(maps, layout), layout, positions=N), want), layout
        st = chip.debug_vlad_stage(N)
        assert M.same_bits(st["a"], mirror(N, C, K, G, 2)["a"]) and M.same_bits(st["V"], mirror(N, C, K, G, 2)["V"])
        assert chip.append_vlad_batch(maps, positions=N) == 0 and chip.size() == 3
        assert M.same_bits(chip.read_rows_f64(range(3)), want.astype(np.float64))
        big = np.zeros((1, N + 1, C), np.float32)
        assert status_of(chip.vlad_batch, big, positions=N + 1) == capi.CHIP_ERR_UNSUPPORTED
        assert status_of(chip.append_vlad_batch, big, positions=N + 1) == capi.CHIP_ERR_UNSUPPORTED and chip.size() == 3


# ---------------------------------------------------------------------------------------------- 2: through a projection
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_a_batch_through_a_projection_shares_the_matrix_passes(kind):
    """K * C = in_dim = 1024, D = 256: a batch of 2 width + 3 maps equals append_projected of the chip_vlad vectors, in three shared passes"""
    N, C, K, G, D = 65, 64, 16, 0, 256
    w = capi.project_plan(K * C, capi.CHIP_PROJ_F32, 0)["width"]
    B = 2 * w + 3
    Wt, bias, centres = T.weights(C, K, G)
    maps = batch(B, N, C)
    want = np.stack([mirror(N, C, K, G, m)["v"] for m in range(B)])
    rng = np.random.default_rng(8)
    Mt = rng.standard_normal((D, K * C), dtype=np.float32)
    Mt = Mt if kind == "f32" else Mt.astype(np.float64) * (1 + 2.0 ** -40)
    b = rng.standard_normal(D)
    with capi.Chip(D) as chip, capi.Chip(D) as ref:
        for c in (chip, ref):
            c.vlad_set(Wt, bias, centres)
            c.project_set(Mt, b)
        v = chip.vlad_batch(maps)
        assert M.same_bits(v, want)
        assert chip.append_vlad_batch(maps) == 0 and chip.size() == B
        last = chip.debug_project_last()
        assert (last["shared_passes"], last["single_launches"], last["shared_descriptors"]) == (3, 0, B), last
        assert chip.append_vlad_batch(as_layout(maps[:w + 1], NCHW), NCHW, positions=N) == B
        last = chip.debug_project_last()
        assert (last["shared_passes"], last["single_launches"]) == (1, 1), last                    # a trailing group of one
        assert ref.append_projected(v) == 0 and ref.append_projected(v[:w + 1]) == B
        ia, ir = chip.info(), ref.info()
        for f in INFO_FIELDS:
            assert ia[f] == ir[f], f
        assert ia["storage_bytes"] == 8
        rows = chip.read_rows_f64(range(B + w + 1))
        assert M.same_bits(rows, ref.read_rows_f64(range(B + w + 1)))
        assert M.same_bits(rows[:B], MP.project(want, Mt, b)[1])
        assert chip.append_vlad(maps[0]) == B + w + 1                                              # the single call, a batch of one
        assert M.same_bits(chip.read_rows_f64([B + w + 1]), rows[:1])
        last = chip.debug_project_last()
        assert (last["shared_passes"], last["single_launches"]) == (0, 1), last


# ---------------------------------------------------------------------------------------------- 3: a non-finite map refuses the call
def test_a_nonfinite_map_in_the_middle_refuses_the_whole_batch():
    N, C, K, G = 65, 64, 16, 0
    Wt, bias, centres = T.weights(C, K, G)
    B = 19                                                                      # two groups: 16 maps and 3
    maps = batch(B, N, C)
    want = np.stack([mirror(N, C, K, G, m)["v"] for m in range(B)])
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        assert chip.append_vlad_batch(maps[:2]) == 0
        before, info = chip.read_rows_f64([0, 1]), chip.info()
        for m, value, at in ((9, np.nan, (64, 63)), (17, np.inf, (0, 0)), (0, -np.inf, (30, 5))):   # first group, second group, first map
            bad = np.array(maps)
            bad[(m,) + at] = value
            for layout in (NHWC, NCHW):
                out = np.full((B, K * C), 7.0, np.float32)
                rc = chip.lib.chip_vlad_batch(chip.h, capi._ptr(as_layout(bad, layout)), B, N, layout, capi._ptr(out))
                assert rc == capi.CHIP_ERR_NONFINITE and (out == 7.0).all(), (m, layout)       # v is not written
                assert status_of(chip.append_vlad_batch, as_layout(bad, layout), layout, positions=N) == capi.CHIP_ERR_NONFINITE
            assert chip.size() == 2 and all(chip.info()[f] == info[f] for f in INFO_FIELDS)
            assert M.same_bits(chip.read_rows_f64([0, 1]), before)
        assert chip.append_vlad_batch(maps) == 2 and chip.size() == 2 + B       # and the ctx is as good as new
        assert M.same_bits(chip.read_rows_f64(range(2, 2 + B)), want.astype(np.float64))


# ---------------------------------------------------------------------------------------------- 4: a torch tensor
def test_a_batch_from_a_torch_tensor():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device: the device-pointer form of the maps cannot be made here")
    H, W, C, K, G = 5, 13, 64, 16, 0                                            # 65 positions
    N, B = H * W, 17
    Wt, bias, centres = T.weights(C, K, G)
    maps = batch(B, N, C)
    want = np.stack([mirror(N, C, K, G, m)["v"] for m in range(B)])
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        t = torch.from_numpy(maps.reshape(B, H, W, C)).to("cuda:0").permute(0, 3, 1, 2).contiguous()     # [B, C, H, W], as a torch trunk emits it
        u = torch.from_numpy(maps.reshape(B, H, W, C)).to("cuda:0")                                      # [B, H, W, C]
        torch.cuda.synchronize()                                                # the caller vouches that the maps are complete
        assert M.same_bits(chip.vlad_batch(t.data_ptr(), NCHW, n_maps=B, positions=N), want)
        assert M.same_bits(chip.vlad_batch(u.data_ptr(), NHWC, n_maps=B, positions=N), want)
        assert chip.append_vlad_batch(t.data_ptr(), NCHW, n_maps=B, positions=N) == 0
        assert chip.append_vlad_batch(u.data_ptr(), NHWC, n_maps=B, positions=N) == B
        rows = chip.read_rows_f64(range(2 * B))
        assert M.same_bits(rows[:B], want.astype(np.float64)) and M.same_bits(rows[B:], rows[:B])
        del t, u


# ---------------------------------------------------------------------------------------------- 5: the example
def test_append_batch_example():
    exe = LIB / "append_batch"
    assert exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFER" not in r.stdout and r.stdout.count("0 differences") == 2
