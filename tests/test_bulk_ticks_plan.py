"""chip_bulk_ticks_plan (no ctx, no device) against a Python restatement of the tick's rule (chip_api.hip tick_prepare, Cerebro.cpp:960-966,
:1019-1022): status, k and the advance of last_l over a sequence of ticks, the grouping of the scanned ticks, the argument errors."""
import numpy as np
import pytest

from cerebro_amd import capi

SKIPPED, TOO_SHORT, SCANNED = 0, 1, 2
GROUP = capi.CHIP_BULK_TICKS_GROUP


class Range(Exception):
    pass


def rule(ls, n_rows, last_l=0, locality=12, lag=50, min_new=3, min_k=5):
    """the sequence of chip_loop_tick calls, restated: (status, k) per tick and the loop state afterwards"""
    status, k = [], []
    for l in ls:
        if l < 0 or l > n_rows:
            raise Range(l)
        if l - last_l < min_new:
            status.append(SKIPPED); k.append(0)       # last_l kept
            continue
        if l < 3:
            raise Range(l)
        kk = l - lag
        scanned = kk > min_k
        status.append(SCANNED if scanned else TOO_SHORT)
        k.append(kk if scanned else 0)
        last_l = l                                     # both advance it
    return status, k, last_l


def check(ls, n_rows, last_l=0, **kw):
    p = capi.default_dot_params()
    for name, v in kw.items():
        setattr(p, name, v)
    d = capi.bulk_ticks_plan(ls, n_rows, params=p if kw else None, last_l=last_l)
    st, k, last = rule(ls, n_rows, last_l, **kw)
    assert d["status"].tolist() == st and d["k"].tolist() == k and d["last_l"] == last
    assert (d["ticks_skipped"], d["ticks_too_short"], d["ticks_scanned"]) == (st.count(SKIPPED), st.count(TOO_SHORT), st.count(SCANNED))
    assert d["group_ticks"] == GROUP and 3 * GROUP <= capi.CHIP_QUERY_PREFIX_GROUP
    assert d["groups"] == -(-st.count(SCANNED) // GROUP)     # no tick is split: groups of whole ticks
    return d, st, k


def test_defaults_are_the_ticks():
    p = capi.default_dot_params()
    assert (p.locality, p.lag, p.min_new, p.min_k) == (12, 50, 3, 5)


def test_every_l_of_a_run_interleaves_the_three_statuses():
    d, st, k = check(list(range(3, 200)), 300)
    assert st[:6] == [TOO_SHORT, SKIPPED, SKIPPED, TOO_SHORT, SKIPPED, SKIPPED]      # l = 3 runs, 4 and 5 are too close to it, 6 runs
    assert SCANNED in st and st[-3:].count(SKIPPED) == 2
    first = st.index(SCANNED)
    assert 3 + first == 57 and k[first] == 7                                      # k > 5, and of l = 55 .. 57 only 57 is far enough from the last


def test_skipped_keeps_last_l_and_too_short_advances_it():
    d, st, _ = check([10, 11, 12, 13], 100)
    assert st == [TOO_SHORT, SKIPPED, SKIPPED, TOO_SHORT] and d["last_l"] == 13
    d, st, _ = check([10, 11, 12], 100)
    assert st == [TOO_SHORT, SKIPPED, SKIPPED] and d["last_l"] == 10
    d, st, _ = check([60, 62, 63], 100, last_l=58)
    assert st == [SKIPPED, SCANNED, SKIPPED] and d["last_l"] == 62
    assert capi.bulk_ticks_plan([61], 100, last_l=58)["status"].tolist() == [SCANNED]


def test_a_repeated_l_is_skipped():
    d, st, k = check([70, 70, 73, 73, 73, 80], 100)
    assert st == [SCANNED, SKIPPED, SCANNED, SKIPPED, SKIPPED, SCANNED] and k == [20, 0, 23, 0, 0, 30]


def test_l_below_three():
    d, st, _ = check([0, 1, 2], 100, last_l=0)              # all too close to last_l = 0: skipped before the rows l-1 .. l-3 are asked for
    assert st == [SKIPPED] * 3
    for l in (0, 1, 2):
        with pytest.raises(capi.ChipError) as e:            # far enough from last_l: the tick needs three rows
            capi.bulk_ticks_plan([l], 100, last_l=-10)
        assert e.value.status == capi.CHIP_ERR_RANGE
        with pytest.raises(Range):
            rule([l], 100, last_l=-10)
    with pytest.raises(capi.ChipError) as e:
        capi.bulk_ticks_plan([-1], 100)
    assert e.value.status == capi.CHIP_ERR_RANGE


def test_l_beyond_the_db_is_a_range_error_with_nothing_written():
    ls = np.array([60, 63, 101, 66], np.int64)
    status = np.full(4, 77, np.int32)
    k = np.full(4, 77, np.int64)
    out = capi.BulkTicksPlan()
    out.groups = 77
    import ctypes as C
    rc = capi.load_library().chip_bulk_ticks_plan(ls.ctypes.data, 4, None, 0, 100, status.ctypes.data, k.ctypes.data, C.byref(out))
    assert rc == capi.CHIP_ERR_RANGE and (status == 77).all() and (k == 77).all() and out.groups == 77
    check([60, 63, 100], 100)                                # l == n_rows is the last tick there is
    with pytest.raises(Range):
        rule(ls.tolist(), 100)


def test_a_prefix_that_is_no_prefix_of_the_db_is_refused():
    """the bulk call's own refusal (header): with a negative lag k = l - lag lies beyond the rows, with min_k below -lag it is negative"""
    lib = capi.load_library()
    for kw, ls in ((dict(lag=-5), [98]), (dict(lag=70, min_k=-100), [60])):
        with pytest.raises(capi.ChipError) as e:
            capi.bulk_ticks_plan(ls, 100, params=_params(**kw))
        assert e.value.status == capi.CHIP_ERR_RANGE
    assert capi.bulk_ticks_plan([98], 100, params=_params(lag=-2))["k"].tolist() == [100]      # k == n_rows is the whole DB
    assert capi.bulk_ticks_plan([70], 100, params=_params(lag=70, min_k=-100))["k"].tolist() == [0]


def _params(**kw):
    p = capi.default_dot_params()
    for name, v in kw.items():
        setattr(p, name, v)
    return p


def test_other_params():
    d, st, k = check(list(range(3, 60)), 60, lag=10, min_new=1, min_k=2)
    assert st.count(SKIPPED) == 0 and st[:10] == [TOO_SHORT] * 10 and k[10] == 3
    check(list(range(3, 60, 2)), 60, lag=7, min_new=2, min_k=0)


@pytest.mark.parametrize("T", [1, GROUP, GROUP + 1, 2 * GROUP + 1])
def test_grouping(T):
    ls = [56 + 3 * i for i in range(T)]
    n = ls[-1] + 10
    d, st, k = check(ls, n)
    assert st == [SCANNED] * T
    last = T - GROUP * (d["groups"] - 1)                     # ticks of the last group
    qpad = -(-3 * last // 128) * 128
    assert d["groups"] == {1: 1, GROUP: 1, GROUP + 1: 2, 2 * GROUP + 1: 3}[T]
    assert d["tile_full"] == (256 if T >= GROUP else 0)     # 4095 queries pad to 4096: the wide tile
    assert d["tile_last"] == (256 if qpad % 256 == 0 else 128)
    # units as chip_query_prefix_plan counts them, group by group, over the queries in walk order
    units = rect = 0
    kq = np.repeat(np.array(k, np.int64), 3)
    for g in range(d["groups"]):
        sub = kq[3 * GROUP * g:3 * GROUP * (g + 1)]
        f = capi.query_prefix_plan(sub, elem=4, topk=16)
        assert f["groups"] == 1
        units += f["units"]
        rect += f["qtiles"] * -(-int(kq[-1]) // f["tile_last"])
    assert (d["units"], d["units_rect"]) == (units, rect)


def test_walk_order_is_by_k_whatever_the_order_of_the_ticks():
    ls = [400, 100, 300, 200]                                 # a replay may ask in any order: every tick is far from the one before
    d, st, k = check(ls, 500, min_new=-1000)
    assert st == [SCANNED] * 4 and k == [350, 50, 250, 150] and d["groups"] == 1 and d["units"] == -(-350 // d["tile_last"])


def test_argument_errors():
    lib = capi.load_library()
    import ctypes as C
    ls = np.array([60], np.int64)
    status, k, out = np.zeros(1, np.int32), np.zeros(1, np.int64), capi.BulkTicksPlan()
    ok = (ls.ctypes.data, 1, None, 0, 100, status.ctypes.data, k.ctypes.data, C.byref(out))
    assert lib.chip_bulk_ticks_plan(*ok) == capi.CHIP_OK
    for i, bad in ((0, None), (1, 0), (1, -1), (4, -1), (5, None), (6, None), (7, None)):
        args = list(ok)
        args[i] = bad
        assert lib.chip_bulk_ticks_plan(*args) == capi.CHIP_ERR_INVALID_ARG, i
    assert lib.chip_build_has_bulk_ticks() == 1
