"""chip_query_prefix_plan (no ctx, no device): the order and the work of a many-query call with a prefix per query, from the functions
the call sizes itself with (cerebro_amd/csrc/batch.hip: prefix_order, prefix_group).  The counts are recomputed here independently:
stable sort by k, groups of CHIP_QUERY_PREFIX_GROUP, a group padded to 128 queries and tiled 256 x 256 when the padded count is a
multiple of 256 (never on double rows with topk > 8), else 128 x 128; units = sum over query tiles of ceil(max k in the tile / tile).

The triangle bound.  For k_j = j a query tile of T rows whose last query is j needs ceil(j / T) DB tiles; over one tile shape that sums
to qtiles (qtiles + 1) / 2 against the rectangle's qtiles^2, hence units <= units_rect / 2 + qtiles.  The arithmetic needs ONE tile
shape T on both sides.  At Q = 20000 that is what double rows with topk > 8 have (every group takes the 128 tile: 157 query tiles,
units 12403, units_rect 24649).  With float rows the four full groups take the 256 tile and the last group (3616 queries, padded to
3712 = 14.5 x 256) the 128 tile: its 29 small tiles hold the largest prefixes and are counted like the large ones (units 6227,
units_rect 9609, qtiles 93), so the sum of tiles of two sizes is not below half of its rectangle and the bound is not claimed there;
the float case is checked at Q = 20480, where every group is full."""
import numpy as np
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build   # loads libcerebro_hip.so (no GPU needed)
GROUP = 4096


def tile_of(count, elem, topk):
    qpad = -(-count // 128) * 128
    return qpad, (256 if qpad % 256 == 0 and not (elem == 8 and topk > 8) else 128)


def recount(k, elem, topk):
    k = np.asarray(k, dtype=np.int64)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    units = rect = qtiles = groups = 0
    for first in range(0, len(ks), GROUP):
        g = ks[first:first + GROUP]
        qpad, T = tile_of(len(g), elem, topk)
        groups += 1
        for t in range(qpad // T):
            units += -(-int(g[t * T:(t + 1) * T].max()) // T)
            rect += -(-int(ks[-1]) // T)
            qtiles += 1
    return order, groups, qtiles, units, rect


@pytest.mark.parametrize("elem,topk", [(4, 5), (4, 16), (8, 8), (8, 16)])
@pytest.mark.parametrize("Q,seed", [(1, 0), (130, 1), (600, 2), (4096, 3), (4097, 4), (9000, 5)])
def test_order_and_units_against_an_independent_count(Q, seed, elem, topk):
    k = np.random.default_rng(seed).integers(0, 50000, Q)
    k[::7] = k[0]                                               # equal prefixes: the sort is stable
    p = capi.query_prefix_plan(k, elem, topk)
    order, groups, qtiles, units, rect = recount(k, elem, topk)
    assert np.array_equal(p["order"], order)
    assert (p["groups"], p["qtiles"], p["units"], p["units_rect"]) == (groups, qtiles, units, rect)
    assert p["group_size"] == GROUP == capi.CHIP_QUERY_PREFIX_GROUP


def test_causal_self_join_walks_the_triangle():
    k = np.arange(20000)
    p = capi.query_prefix_plan(k, 8, 16)                        # one tile shape throughout (see the module docstring)
    print(p["units"], p["units_rect"], p["qtiles"])
    assert p["units"] <= p["units_rect"] / 2 + p["qtiles"]
    assert (p["units"], p["units_rect"], p["qtiles"], p["tile_full"], p["tile_last"]) == (12403, 24649, 157, 128, 128)
    p = capi.query_prefix_plan(np.arange(20480), 4, 5)          # float rows, every group full: the 256 tile throughout
    print(p["units"], p["units_rect"], p["qtiles"])
    assert p["units"] <= p["units_rect"] / 2 + p["qtiles"] and (p["tile_full"], p["tile_last"]) == (256, 256)
    p = capi.query_prefix_plan(k, 4, 5)                         # float rows at 20000: two tile shapes in one sum
    print(p["units"], p["units_rect"], p["qtiles"])
    assert (p["units"], p["units_rect"], p["qtiles"], p["tile_full"], p["tile_last"]) == (6227, 9609, 93, 256, 128)


def test_all_prefixes_equal_is_the_rectangle():
    for Q in (5, 300, 5000):
        for kk in (0, 1, 777, 100000):
            p = capi.query_prefix_plan(np.full(Q, kk), 4, 5)
            assert p["units"] == p["units_rect"]


def test_group_count():
    for Q, groups in ((1, 1), (4096, 1), (4097, 2), (8192, 2), (8193, 3)):
        assert capi.query_prefix_plan(np.zeros(Q, dtype=np.int64))["groups"] == groups


def test_tile_shape_rule():
    plan = lambda Q, elem, topk: capi.query_prefix_plan(np.arange(Q), elem, topk)   # noqa: E731
    for Q, elem, topk, full, last in ((1, 4, 5, 0, 128), (128, 4, 5, 0, 128), (129, 4, 5, 0, 256), (256, 4, 16, 0, 256), (257, 4, 5, 0, 128),
                                      (512, 8, 8, 0, 256), (512, 8, 9, 0, 128), (512, 8, 16, 0, 128), (4096, 4, 16, 256, 256),
                                      (4096, 8, 16, 128, 128), (4096 + 130, 4, 5, 256, 256), (4096 + 300, 8, 8, 256, 128), (8192 + 1, 8, 9, 128, 128)):
        p = plan(Q, elem, topk)
        assert (p["tile_full"], p["tile_last"]) == (full, last), (Q, elem, topk, p)


def test_plan_status_codes():
    lib = capi.load_library()
    k = np.arange(10, dtype=np.int64)
    out = capi.QueryPrefixPlan()
    import ctypes as C
    assert lib.chip_query_prefix_plan(None, 10, 4, 5, None, C.byref(out)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_query_prefix_plan(capi._ptr(k), 10, 4, 5, None, None) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_query_prefix_plan(capi._ptr(k), 0, 4, 5, None, C.byref(out)) == capi.CHIP_ERR_INVALID_ARG
    assert lib.chip_query_prefix_plan(capi._ptr(k), 10, 2, 5, None, C.byref(out)) == capi.CHIP_ERR_UNSUPPORTED
    assert lib.chip_query_prefix_plan(capi._ptr(k), 10, 4, 17, None, C.byref(out)) == capi.CHIP_ERR_UNSUPPORTED
    assert lib.chip_query_prefix_plan(capi._ptr(k - 1), 10, 4, 5, None, C.byref(out)) == capi.CHIP_ERR_RANGE
    assert lib.chip_query_prefix_plan(capi._ptr(k), 10, 4, 5, None, C.byref(out)) == capi.CHIP_OK and out.groups == 1   # order may be NULL
    assert lib.chip_build_has_query_prefix() == 1
