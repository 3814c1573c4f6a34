"""GPU tests of the ingest path at its edges: what K3 (kernels.hip convert_rows) stores and refuses, value by value, and the row-norm bound
N = chip_get_info().row_norm_max that rows_norm2_max / append_publish make of the stored rows -- the N that the prefilter's error bounds
E and E_h are made of.  References: tests/ingest_cases.py (checked on the CPU by tests/test_ingest_cases.py).

A refused call leaves state(chip) identical; the next valid append gets the first index the refused one would have got and reads back bit
for bit.  After every accepted append check_norm holds N bit for bit to sqrt(max ss) * (1 + 2^-30), ss the tree-ordered fp64 sum of squares
of the rows read back, and every row's correctly rounded norm to N from below."""
import math
from functools import lru_cache

import numpy as np
import pytest

import ingest_cases as IC
import oracle_lib
import vlad_cases as T
from cerebro_amd import capi
from test_batch_edges_gpu import seg_rows
from test_project_gpu import case as project_case

pytestmark = pytest.mark.gpu
NOT_F32, NONFINITE = capi.CHIP_ERR_NOT_F32, capi.CHIP_ERR_NONFINITE
STAGE_BYTES = 64 << 20           # the staging buffer of an append (chip_api.hip append_pass): a call is uploaded in chunks of this size
STATE_FIELDS = ("storage_bytes", "rows_global", "rows_local", "lossy_rows", "row_norm_max")


def state(chip):
    i = chip.info()
    return (chip.size(),) + tuple(float(i[f]).hex() if f == "row_norm_max" else i[f] for f in STATE_FIELDS)


def refused(chip, status, fn, *a, **k):
    """the call fails with `status` and changes nothing that can be seen"""
    before = state(chip)
    with pytest.raises(capi.ChipError) as e:
        fn(*a, **k)
    assert e.value.status == status, (e.value.status, status)
    assert state(chip) == before, (state(chip), before)
    assert math.isfinite(chip.info()["row_norm_max"])


def check_norm(chip, first, n, running, edges=()):
    """after an append of rows [first, first + n): N == max(running, norm_of(max ss)) bit for bit, ss = norm_bits of every row read back;
    norm_exact(row) <= N for every row of a small call, for the edges, the heaviest row and a sample of a large one.  -> the new running"""
    N = chip.info()["row_norm_max"]
    assert chip.info()["storage_bytes"] == 4 and chip.size() >= first + n
    ss_max = 0.0
    for lo in range(first, first + n, 1024):
        hi = min(lo + 1024, first + n)
        rows = chip.read_rows(range(lo, hi))
        assert np.isfinite(rows).all()
        ss = IC.norm_bits_rows(rows)
        k = int(np.argmax(ss))
        assert IC.norm_bits(rows[k]).hex() == float(ss[k]).hex()              # the oracle's own tree on the row that decides
        ss_max = max(ss_max, float(ss[k]))
        pick = set(range(hi - lo)) if n <= 64 else {0, k, hi - lo - 1} | {g - lo for g in edges if lo <= g < hi} | set(range(7, hi - lo, 97))
        for i in sorted(pick):
            assert IC.norm_exact(rows[i]) <= N, (lo + i, IC.norm_exact(rows[i]).hex(), N.hex())
    running = max(running, IC.norm_of(ss_max))
    assert float(N).hex() == float(running).hex(), (first, n, N, running)
    return running


def accept_f64(chip, running, batch, allow_rounding=False, edges=()):
    """an append that must succeed: first index, length, the rows' bits, the norm bound.  -> the new running"""
    first = chip.size()
    assert chip.append_f64(batch, allow_rounding=allow_rounding) == first and chip.size() == first + len(batch)
    if len(batch) <= 64:
        assert IC.same_bits(chip.read_rows(range(first, first + len(batch))), IC.stored(batch))
    return check_norm(chip, first, len(batch), running, edges)


# ---------------------------------------------------------------------------------------------- a: the value table, float64 wire -> float rows
D_A = 256
SPOTS = ((0, 0), (2, 131), (4, D_A - 1))     # the first element; the fourth of a 4-group in a middle row; the last element of the call


@lru_cache(maxsize=None)
def base5():
    b = IC.f32_rows(5, D_A, 11).astype(np.float64)
    b.setflags(write=False)
    return b


def planted(x, at):
    b = np.array(base5())
    b[at] = x
    return b


def bits_at(chip, g, e):
    return int(chip.read_rows([g])[0, e].view(np.uint32))


def test_exact_values_are_stored_as_they_are():
    with capi.Chip(D_A, storage="f32") as chip:
        N = 0.0
        for x in IC.values_of(IC.EXACT):
            for at in SPOTS:
                for flag in (False, True):
                    first = chip.size()
                    N = accept_f64(chip, N, planted(x, at), allow_rounding=flag)
                    assert chip.info()["lossy_rows"] == 0
                    assert bits_at(chip, first + at[0], at[1]) == IC.stored_bits(x), (x.hex(), at, flag)


def test_inexact_values_are_refused_or_rounded_to_nearest_even():
    with capi.Chip(D_A, storage="f32") as chip:
        N = accept_f64(chip, 0.0, base5())
        for x in IC.values_of(IC.INEXACT):
            for at in SPOTS:
                b = planted(x, at)
                refused(chip, NOT_F32, chip.append_f64, b)
                lossy, first = chip.info()["lossy_rows"], chip.size()
                N = accept_f64(chip, N, b, allow_rounding=True)
                assert chip.info()["lossy_rows"] > lossy
                assert bits_at(chip, first + at[0], at[1]) == IC.stored_bits(x), (x.hex(), at)      # the sign of -0.0, both ties, the subnormals
        assert chip.size() == 5 + 5 * 3 * len(IC.values_of(IC.INEXACT))


def test_overflowing_values_are_never_stored():
    """a finite value whose nearest float32 is +-Inf: CHIP_ERR_NOT_F32 without the flag; with it CHIP_ERR_NONFINITE, not an Inf row"""
    with capi.Chip(D_A, storage="f32") as chip:
        N = accept_f64(chip, 0.0, base5())
        for x in IC.values_of(IC.OVERFLOW):
            for at in SPOTS:
                b = planted(x, at)
                refused(chip, NOT_F32, chip.append_f64, b)
                refused(chip, NONFINITE, chip.append_f64, b, allow_rounding=True)
        lossy = chip.info()["lossy_rows"]
        b = planted(0.1, (1, 1))
        b[3, 200] = 1e39                                            # next to a value that may be rounded
        refused(chip, NONFINITE, chip.append_f64, b, allow_rounding=True)
        assert chip.size() == 5 and chip.info()["lossy_rows"] == lossy == 0
        accept_f64(chip, N, base5())                                # the first index and the bits of a ctx nothing has happened to


def test_nonfinite_values_are_refused_with_and_without_the_flag():
    with capi.Chip(D_A, storage="f32") as chip:
        N = accept_f64(chip, 0.0, base5())
        for x in IC.values_of(IC.NONFINITE):
            for at in SPOTS:
                for flag in (False, True):
                    refused(chip, NONFINITE, chip.append_f64, planted(x, at), allow_rounding=flag)
        b = planted(0.1, (0, 0))                                    # a NaN and an inexact value: the NaN decides
        b[4, D_A - 1] = np.nan
        for flag in (False, True):
            refused(chip, NONFINITE, chip.append_f64, b, allow_rounding=flag)
        accept_f64(chip, N, base5())


# ---------------------------------------------------------------------------------------------- b: the other three instantiations
def test_float_wire_into_float_rows():
    keep = np.array([-0.0, 2.0 ** -149, -(2.0 ** -149), np.finfo(np.float32).max, -np.finfo(np.float32).max, 2.0 ** -126], dtype=np.float32)
    with capi.Chip(D_A, storage="f32") as chip:
        b = base5().astype(np.float32)
        N = 0.0
        for i, at in enumerate(SPOTS):
            for x in (np.nan, np.inf, -np.inf):
                bad = b.copy()
                bad[at] = x
                refused(chip, NONFINITE, chip.append_f32, bad)
            ok = b.copy()
            ok[at[0], :len(keep)] = keep
            ok[at] = keep[i]
            first = chip.size()
            assert chip.append_f32(ok) == first == 5 * i
            assert IC.same_bits(chip.read_rows(range(first, first + 5)), ok)
            N = check_norm(chip, first, 5, N)
        assert chip.info()["lossy_rows"] == 0


def test_float_wire_into_double_rows_widens_exactly():
    with capi.Chip(D_A, storage="f64") as chip:
        b = base5().astype(np.float32)
        b[0, 0], b[2, 131], b[4, D_A - 1], b[1, 7] = 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127, -0.0
        b[3, 3] = np.finfo(np.float32).max
        bad = b.copy()
        bad[2, 131] = np.nan
        refused(chip, NONFINITE, chip.append_f32, bad)
        assert chip.append_f32(b) == 0
        got = chip.read_rows_f64(range(5))
        assert IC.same_bits(got, b.astype(np.float64)) and got[0, 0] == 2.0 ** -149 and got[4, D_A - 1] == 2.0 ** -127
        assert chip.info()["storage_bytes"] == 8 and chip.info()["row_norm_max"] == 0.0


def test_double_wire_into_double_rows_keeps_every_bit():
    with capi.Chip(D_A, storage="f64") as chip:
        b = np.array(base5())
        b[0, 0], b[2, 131], b[4, D_A - 1], b[1, 1], b[3, 3] = 5e-324, np.finfo(np.float64).max, 0.1, -5e-324, -np.finfo(np.float64).max
        for x in IC.values_of(IC.NONFINITE):
            for at in SPOTS:
                bad = b.copy()
                bad[at] = x
                refused(chip, NONFINITE, chip.append_f64, bad)
        for flag in (False, True):
            first = chip.size()
            assert chip.append_f64(b, allow_rounding=flag) == first
            assert IC.same_bits(chip.read_rows_f64(range(first, first + 5)), b)
        assert chip.info()["lossy_rows"] == 0 and chip.info()["row_norm_max"] == 0.0


# ---------------------------------------------------------------------------------------------- c: the undecided DB
def test_undecided_db_takes_what_float_rows_cannot_hold_as_double_rows():
    for x in (0.1, 2.0 ** 128, -1e39, np.finfo(np.float64).max, 5e-324, float.fromhex("0x1.ffffffp+127"), 1 + 2.0 ** -24):
        for at in SPOTS[1:]:
            with capi.Chip(D_A) as chip:
                assert chip.info()["storage_bytes"] == 4
                b = planted(x, at)
                assert chip.append_f64(b) == 0 and chip.size() == 5
                assert chip.info()["storage_bytes"] == 8 and chip.info()["lossy_rows"] == 0 and chip.info()["row_norm_max"] == 0.0
                assert IC.same_bits(chip.read_rows_f64(range(5)), b)


def test_undecided_db_stays_undecided_after_a_refusal():
    with capi.Chip(D_A) as chip:
        for flag in (False, True):
            refused(chip, NONFINITE, chip.append_f64, planted(np.nan, SPOTS[1]), allow_rounding=flag)
        assert chip.info()["storage_bytes"] == 4 and chip.size() == 0
        accept_f64(chip, 0.0, base5())
        assert chip.info()["storage_bytes"] == 4


@pytest.mark.parametrize("then", ["same batch without the flag", "a clean batch"])
def test_undecided_db_refuses_an_overflow_under_the_flag(then):
    b = planted(2.0 ** 128, SPOTS[2])
    with capi.Chip(D_A) as chip:
        refused(chip, NONFINITE, chip.append_f64, b, allow_rounding=True)
        assert chip.info()["storage_bytes"] == 4 and chip.size() == 0
        if then == "a clean batch":
            accept_f64(chip, 0.0, base5())
            assert chip.info()["storage_bytes"] == 4
        else:
            assert chip.append_f64(b) == 0
            assert chip.info()["storage_bytes"] == 8 and IC.same_bits(chip.read_rows_f64(range(5)), b)


# ---------------------------------------------------------------------------------------------- d: chunks of the staging buffer, laps of K3
D_BIG, N_BIG = 1024, 8193


@lru_cache(maxsize=None)
def big_batch():
    """8193 float32-valued rows on the float64 wire (67 MB): 257 distinct rows, tiled"""
    b = IC.tiled(IC.f32_rows(257, D_BIG, 21), N_BIG).astype(np.float64)
    b.setflags(write=False)
    return b


def big_geometry(chip):
    """(rows of the first chunk, rows one lap of convert_rows covers) of an append of big_batch(), from the device's CU count"""
    n_cus = chip.info()["n_cus"]
    chunk_rows = STAGE_BYTES // (D_BIG * 8)
    assert chunk_rows == N_BIG - 1                                  # two chunks, the second of one row
    lap_rows = 8 * n_cus * 256 // (D_BIG // 4)                      # at most 8 n_cus blocks of 256 threads, four elements a thread
    assert 2 * lap_rows <= chunk_rows                               # the first chunk takes at least two whole laps (four at 256 CUs)
    return chunk_rows, lap_rows


def test_flags_accumulate_over_chunks_and_laps():
    b = np.array(big_batch())
    with capi.Chip(D_BIG, capacity_hint=N_BIG + 64, storage="f32") as chip:
        chunk_rows, lap_rows = big_geometry(chip)
        N = accept_f64(chip, 0.0, b[:3])
        spots = [(chunk_rows, D_BIG - 1), (chunk_rows - 1, D_BIG - 1), (0, 0), (lap_rows + 48, 230)]      # the last: inside lap 2 of chunk 1
        for at in spots:
            keep = b[at]
            for x, status in ((0.1, NOT_F32), (np.nan, NONFINITE)):
                b[at] = x
                refused(chip, status, chip.append_f64, b)
            b[at] = 2.0 ** 128
            refused(chip, NONFINITE, chip.append_f64, b, allow_rounding=True)
            b[at] = keep
        assert IC.same_bits(b, big_batch())
        edges = [3 + r for r in (0, lap_rows - 1, lap_rows, 2047, 2048, chunk_rows - 1, chunk_rows)]
        N = accept_f64(chip, N, b, edges=edges)
        assert IC.same_bits(chip.read_rows(edges), IC.stored(b[[e - 3 for e in edges]]))
        assert chip.info()["lossy_rows"] == 0


def test_a_bad_value_in_the_second_chunk_switches_an_undecided_db():
    b = np.array(big_batch())
    b[N_BIG - 1, D_BIG - 1] = 0.1
    with capi.Chip(D_BIG, capacity_hint=N_BIG + 64) as chip:
        big_geometry(chip)
        assert chip.append_f64(b) == 0 and chip.size() == N_BIG
        assert chip.info()["storage_bytes"] == 8 and chip.info()["row_norm_max"] == 0.0
        at = [0, 2047, 2048, N_BIG - 2, N_BIG - 1]
        assert IC.same_bits(chip.read_rows_f64(at), b[at])


# ---------------------------------------------------------------------------------------------- e: where the heaviest row sits in the call
@pytest.mark.parametrize("where", ["first", "last of lap 1", "first of lap 2", "last"])
def test_heaviest_row_in_either_lap_of_the_norm_kernel(where):
    D = 256
    with capi.Chip(D, capacity_hint=10_000) as chip:
        lap = 32 * chip.info()["n_cus"]                             # rows_norm2_max: at most 8 n_cus blocks of four waves, a row a wave
        n = lap + 5
        assert n * D * 4 <= STAGE_BYTES                             # one chunk
        at = {"first": 0, "last of lap 1": lap - 1, "first of lap 2": lap, "last": n - 1}[where]
        b = IC.tiled(IC.f32_rows(300, D, 31), n)
        b[at] = b[at] * np.float32(4.0)
        assert chip.append_f32(b) == 0
        N = check_norm(chip, 0, n, 0.0, edges=[0, lap - 1, lap, n - 1])
        assert N == IC.norm_of(IC.norm_bits(b[at])) and N > 3 * IC.norm_exact(b[(at + 1) % n])      # the heavy row decided
        assert IC.same_bits(chip.read_rows([at]), b[[at]])


@pytest.mark.parametrize("at", [N_BIG - 1, N_BIG - 2], ids=["the row of chunk 2", "the last row of chunk 1"])
def test_heaviest_row_in_either_chunk(at):
    b = np.array(big_batch())
    b[at] *= 4.0
    with capi.Chip(D_BIG, capacity_hint=N_BIG + 64) as chip:
        big_geometry(chip)
        N = accept_f64(chip, 0.0, b, edges=[0, N_BIG - 2, N_BIG - 1])
        assert chip.info()["storage_bytes"] == 4
        assert N == IC.norm_of(IC.norm_bits(b[at].astype(np.float32))) and N > 3 * IC.norm_exact(b[0])


# ---------------------------------------------------------------------------------------------- f: where the weight sits in the row
@pytest.mark.parametrize("wire", ["f32", "f64"])
@pytest.mark.parametrize("D", [4, 260, 1028, 10240])
def test_weight_in_the_last_elements_of_a_row(D, wire):
    """calls in the order of their norms, so that each one decides N: all zero, all 2^-149, one element at D - 1, the last 4-group, FLT_MAX"""
    def call(chip, N, row):
        b = np.zeros((3, D), dtype=np.float32)
        b[1] = row
        first = chip.size()
        assert (chip.append_f32(b) if wire == "f32" else chip.append_f64(b.astype(np.float64))) == first
        assert IC.same_bits(chip.read_rows(range(first, first + 3)), b)
        return check_norm(chip, first, 3, N)

    zero = np.zeros(D, np.float32)
    tiny = np.full(D, 2.0 ** -149, np.float32)
    last = zero.copy(); last[D - 1] = 3.0
    group = zero.copy(); group[D - 4:] = (1.0, -2.0, 0.5, 4.0)
    body = IC.f32_rows(1, D, D)[0]; body[0] = 16.0; body[D - 1] = 0.0    # ... and a full row whose last element is the FLT_MAX one
    huge = body.copy(); huge[D - 1] = np.finfo(np.float32).max
    with capi.Chip(D, storage="f32") as chip:
        N = call(chip, 0.0, zero)
        assert N == 0.0 and chip.info()["row_norm_max"] == 0.0       # exactly
        steps = [call(chip, N, tiny)]
        for row in (last, group, body, huge):
            steps.append(call(chip, steps[-1], row))
        assert all(a < b for a, b in zip([0.0] + steps, steps)), steps                                   # every call raised N
        assert steps[0] == IC.norm_of(D * 2.0 ** -298) and steps[1] == 3.0 * (1 + 2.0 ** -30)
        assert 3.4e38 < steps[-1] < 3.5e38


# ---------------------------------------------------------------------------------------------- g: N never falls; refusals do not move it
def test_n_never_falls_and_refusals_do_not_move_it():
    D = 260
    up = float.fromhex("0x1.0000010000001p+0")                      # rounds UP, to 1 + 2^-23
    with capi.Chip(D, storage="f32") as chip:
        N1 = accept_f64(chip, 0.0, IC.f32_rows(6, D, 41).astype(np.float64))
        N = accept_f64(chip, N1, IC.f32_rows(6, D, 42, scale=0.25).astype(np.float64))                   # smaller rows: N stays
        assert N == N1
        heavy = IC.f32_rows(4, D, 43).astype(np.float64)
        heavy[2] = 0.0
        heavy[2, D - 2] = float(np.float32(1e30))                   # a row of norm 1e30 ...
        for x, status, flag in ((0.1, NOT_F32, False), (np.nan, NONFINITE, False), (np.nan, NONFINITE, True), (1e39, NONFINITE, True)):
            bad = heavy.copy()
            bad[0, 5] = x                                           # ... in a call that is refused for another row
            refused(chip, status, chip.append_f64, bad, allow_rounding=flag)
        assert chip.info()["row_norm_max"] == N1 and chip.info()["lossy_rows"] == 0
        wire = np.full((3, D), up) * np.ldexp(1.0, np.arange(D) % 3 + 2)[None, :]                       # every element rounds up
        assert (IC.stored(wire).astype(np.float64) > wire).all()
        N = accept_f64(chip, N, wire, allow_rounding=True)
        wire_norm = math.sqrt(math.fsum((wire[0] * wire[0]).tolist()))
        assert N > N1 and N > wire_norm * (1 + 2.0 ** -26)           # the N of the stored floats (2^-24 above the wire's), not of the doubles
        assert chip.info()["lossy_rows"] == 3
        N = accept_f64(chip, N, heavy)                              # and the heavy row, accepted
        assert 1e30 <= N <= 1e30 * (1 + 2.0 ** -20)


# ---------------------------------------------------------------------------------------------- h: both sides of a segment boundary
SEG_D = 8224


@pytest.mark.parametrize("heavy_at", [8191, 8192], ids=["last row of segment 0", "first row of segment 1"])
def test_heaviest_row_next_to_a_segment_boundary(heavy_at):
    seed, n0 = 77, 8190
    assert seg_rows(SEG_D) == 8192
    with capi.Chip(SEG_D, capacity_hint=8300) as chip:
        chip.append_synthetic(n0, seed)
        N = check_norm(chip, 0, n0, 0.0, edges=[0, n0 - 1])
        at = [0, 1, 4095, 8188, n0 - 1]
        assert IC.same_bits(chip.read_rows(at), oracle_lib.synth_rows(seed, at, SEG_D))
        b = IC.f32_rows(6, SEG_D, 51)
        b *= np.float32(0.5 * N / IC.norm_exact(b[0]))              # rows about half as heavy as what the DB holds ...
        b[heavy_at - n0] *= np.float32(8.0)                         # ... and one about four times as heavy
        assert chip.append_f32(b) == n0
        N2 = check_norm(chip, n0, 6, N)
        assert N2 > 3 * N and N2 == IC.norm_of(IC.norm_bits(b[heavy_at - n0]))
        assert IC.same_bits(chip.read_rows(range(n0, n0 + 6)), b)                                        # rows 8191 and 8192 among them
        assert chip.info()["storage_bytes"] == 4 and chip.info()["lossy_rows"] == 0


# ---------------------------------------------------------------------------------------------- i: the other producers of rows
def test_norm_after_unit_synthetic_rows():
    D, n = 1024, 70
    with capi.Chip(D) as chip:
        chip.append_synthetic(n, 5, unit=True)
        assert IC.same_bits(chip.read_rows(range(n)), oracle_lib.synth_rows(5, range(n), D, unit=True))
        N = check_norm(chip, 0, n, 0.0)
        assert abs(N - 1.0) < 1e-6


def test_norm_after_a_projected_append():
    in_dim, D = 256, 68
    Mt, b, x4 = project_case(in_dim, D, "f32")
    with capi.Chip(D, storage="f32") as chip:
        chip.project_set(Mt, b)
        assert chip.append_projected(np.array(x4[[0, 1, 3]]), flags=capi.CHIP_APPEND_ALLOW_ROUNDING) == 0 and chip.size() == 3
        N = check_norm(chip, 0, 3, 0.0)
        assert abs(N - 1.0) < 1e-6                                  # normalised rows, rounded to float


def vlad_shape():
    N, C, K, G = 70, 8, 3, 1
    return N, C, K, G, T.weights(C, K, G, seed=5)


def test_norm_after_a_pooled_append():
    N, C, K, G, (Wt, bias, centres) = vlad_shape()
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        assert chip.append_vlad(T.fmap(N, C, seed=5)) == 0 and chip.size() == 1
        running = check_norm(chip, 0, 1, 0.0)
        assert chip.append_vlad(T.fmap(N, C, seed=6)) == 1
        check_norm(chip, 1, 1, running)


def test_norm_after_a_pooled_batch():
    N, C, K, G, (Wt, bias, centres) = vlad_shape()
    maps = np.stack([T.fmap(N, C, seed=s) for s in (5, 6, 7)])
    with capi.Chip(K * C) as chip:
        chip.vlad_set(Wt, bias, centres)
        assert chip.append_vlad_batch(maps) == 0 and chip.size() == 3
        check_norm(chip, 0, 3, 0.0)
