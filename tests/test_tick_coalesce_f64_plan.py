"""CPU tests (no GPU) of how the shared pass of pipelined ticks is sized: chip_debug_multi_plan, the function launch_scan_multi sizes
itself with (cerebro_amd/csrc/kernels.hip scan_multi_plan).  Double rows stage as many of their 3 T fp64 queries as fit the 160 KiB of
LDS next to the waves' running lists and read the rest in place; float rows stage all of theirs as fp32, as before."""
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build

LDS_PER_CU = 163840
K = capi.CHIP_DEFAULT_TOPK
LISTS = lambda T, k=K: 8 * 3 * T * k * 16          # [wave][3T][K] entries of 16 bytes


@pytest.mark.parametrize("n_cus", [256, 304, 64])
def test_double_rows_of_the_4096_model_share_a_pass_of_two_ticks(n_cus):
    f = capi.multi_plan(4096, 8, 2, K, n_cus)
    assert (f["family"], f["elem"], f["ticks"], f["nq"], f["R"], f["K"]) == ("multi", 8, 2, 6, 4, K), f
    assert f["q64"] + f["NG"] == 6 and f["q64"] >= 1 and f["NG"] >= 1, f       # 6 x 32 KiB do not fit: some are read in place
    assert f["lds_bytes"] == f["q64"] * 4096 * 8 + LISTS(2) <= LDS_PER_CU, f
    assert (f["q64"] + 1) * 4096 * 8 + LISTS(2) > LDS_PER_CU, f                # ... and not one more would
    assert f["block"] == 512 and f["grid"] == n_cus and f["wg_per_cu"] == 1, f
    assert f["launches"] == 0 and f["n_rows"] == 0


def test_narrow_double_rows_stage_every_query():
    f = capi.multi_plan(1024, 8, 2, K)
    assert (f["q64"], f["NG"], f["lds_bytes"]) == (6, 0, 6 * 1024 * 8 + LISTS(2)), f
    f = capi.multi_plan(3584, 8, 2, K)
    assert (f["q64"], f["NG"]) == (5, 1) and f["lds_bytes"] <= LDS_PER_CU, f


def test_float_rows_plan_what_they_launch_today():
    for T in (2, 3):
        f = capi.multi_plan(4096, 4, T, K)
        assert (f["family"], f["elem"], f["ticks"], f["nq"], f["R"], f["U"], f["NTL"], f["FULL"]) == ("multi", 4, T, 3 * T, 4, 4, 1, 1), f
        assert (f["q64"], f["NG"]) == (0, 0), f
        assert f["lds_bytes"] == 3 * T * 4096 * 4 + LISTS(T), f               # launch_scan_multi's size: fp32 queries + lists
        assert f["block"] == 512 and f["grid"] == 256
    rc, _ = capi.multi_plan(8192, 4, 2, K, check=False)                       # 6 x 32 KiB of fp32 queries: no shared pass
    assert rc == capi.CHIP_ERR_UNSUPPORTED


@pytest.mark.parametrize("D,elem,T", [
    (4100, 8, 2),        # rows that are not whole 4 KiB batches
    (4096 + 256, 8, 2),
    (20480, 8, 2),       # one fp64 query (160 KiB) plus the lists exceeds the LDS
    (8192, 8, 2),        # more queries in place than a kernel is built for
    (4096, 8, 3),        # double rows: two ticks per pass
    (4096, 4, 4),
    (4096, 8, 1),
])
def test_shapes_without_a_shared_pass(D, elem, T):
    rc, f = capi.multi_plan(D, elem, T, K, check=False)
    assert rc == capi.CHIP_ERR_UNSUPPORTED, (rc, f)


def test_a_longer_list_takes_its_lds_from_the_staged_queries():
    f8, f16 = capi.multi_plan(4608, 8, 2, 8), capi.multi_plan(4608, 8, 2, 16)
    assert f8["NG"] == 2 and f16["NG"] == 2 and f16["lds_bytes"] - f8["lds_bytes"] == LISTS(2, 16) - LISTS(2, 8)
    assert f16["lds_bytes"] <= LDS_PER_CU
