"""The two list-merge kernels (csrc/topk_merge.h: topk_merge<NQ> and topk_merge_batch) on the crafted list sets of tests/merge_cases.py,
through chip_debug_merge_lists, against the plain reference: scores as bit patterns, indices exactly, at all K positions; the record field
by field.  tests/test_merge_cases.py shows on the CPU which paths of the kernel these inputs reach."""
import ctypes as C

import numpy as np
import pytest

import merge_cases as mc
import oracle_lib
from cerebro_amd import capi

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()
RUNS = [(c, f) for c in CASES for f in c.forms]


@pytest.fixture(scope="module")
def chip():
    with capi.Chip(64) as ch:
        yield ch


def params(case):
    p = capi.default_dot_params()
    assert (p.locality, p.thresh) == (mc.LOCALITY, mc.THRESH)
    p.locality, p.thresh = case.locality, case.thresh
    return p


def same_record(got, want):
    got = got.as_dict()
    for k in ("status", "found", "idx_curr", "idx_prev", "argmax"):
        assert got[k] == want[k], (k, got, want)
    for k in ("score", "maxv"):
        assert np.array_equal(np.array(got[k], dtype=np.float64).view(np.uint64), np.array(want[k], dtype=np.float64).view(np.uint64)), (k, got, want)


@pytest.mark.parametrize("case,form", RUNS, ids=[f"{c.name}-form{f}" for c, f in RUNS])
def test_merge_matches_reference(chip, case, form):
    sc, ix = case.arrays()
    want_s, want_i, want_rec = mc.reference(case, form)
    got_s, got_i, rec = chip.debug_merge_lists(form, sc, ix, l=case.l, params=params(case), record=form == 0)
    bad = np.argwhere((got_i != want_i) | (got_s.view(np.uint64) != want_s.view(np.uint64)))
    assert bad.size == 0, (case.name, form, bad[:4].tolist(), [(got_s[q, r], got_i[q, r], want_s[q, r], want_i[q, r]) for q, r in bad[:4]])
    if form == 0:
        same_record(rec, want_rec)
        # without a record the same kernel writes the same lists (chip_query_rows, the exchange of query lists)
        if case.kinds == ("i",):
            s2, i2, _ = chip.debug_merge_lists(0, sc, ix)
            assert np.array_equal(i2, want_i) and np.array_equal(s2.view(np.uint64), want_s.view(np.uint64))


NQ3 = [c for c in CASES if c.nq == 3 and 0 in c.forms]


@pytest.mark.parametrize("case", NQ3, ids=[c.name for c in NQ3])
def test_merge_decide_gives_the_same_record(chip, case):
    """chip_merge_decide, the product entry of the sharded tick, on the same lists in a device tensor: the record of the hook"""
    import torch
    sc, ix = case.arrays()
    lists = np.empty(sc.shape + (2,), dtype=np.float64)
    lists[..., 0] = sc
    lists[..., 1] = ix.view(np.float64)
    dev = torch.from_numpy(lists).to("cuda:0")
    torch.cuda.synchronize()
    want = mc.reference(case, 0)[2]
    _, _, hook = chip.debug_merge_lists(0, sc, ix, l=case.l, params=params(case), record=True)
    same_record(hook, want)
    if want["status"] == mc.TICK_FAILED:
        with pytest.raises(capi.ChipError) as e:
            chip.merge_decide(case.l, dev.data_ptr(), case.n_lists, case.K, params(case))
        assert e.value.status == capi.CHIP_ERR_SHARD_FAILED
    else:
        same_record(chip.merge_decide(case.l, dev.data_ptr(), case.n_lists, case.K, params(case)), want)


@pytest.mark.parametrize("K", [8, 16])
def test_many_query_merge_sees_more_than_one_wave_of_lists(K):
    """The many-query mode leaves one list per workgroup of a query tile, at most one per 128-row tile and two per compute unit: 66 tiles of
    rows give its merge 66 lists (two waves of heads) for six queries -- two workgroups, the second at query offset 4."""
    D, N = 64, 65 * 128 + 37
    db = oracle_lib.synth_rows(77 + K, range(N), D)
    q = np.concatenate([db[[N - 1, 128 * 64 + 3, 5]], oracle_lib.synth_rows(78, [1, 2, 3], D)])
    with capi.Chip(D) as chip:
        chip.append_f32(db)
        assert min(2 * chip.info()["n_cus"], 512) > 64      # batch_local_enqueue: P = min(tiles, workgroups per query tile, 512)
        for k in (N, 64 * 128 + 1, 64 * 128):                # 66 and 65 lists; 64: one full wave
            want_s, want_i = oracle_lib.scan_topk_fmaf(db, k, q, K)
            got_s, got_i = chip.query_batch(k, q, K)
            assert np.array_equal(got_i, want_i), (k, got_i[:2], want_i[:2])
            assert np.array_equal(got_s.view(np.uint32), want_s.astype(np.float32).view(np.uint32))


def test_status_codes(chip):
    lib = chip.lib

    def call(form, n_lists, nq, K, h=None, lists=True, out=True, result=False):
        buf = np.full((max(n_lists, 1), max(nq, 1), max(K, 1), 2), -np.inf)
        buf[..., 1] = np.int64(-1).view(np.float64)
        o = np.empty((max(nq, 1), max(K, 1), 2))
        p = capi.default_dot_params()
        r = capi.TickResult()
        return lib.chip_debug_merge_lists(chip.h if h is None else h, form, capi._ptr(buf) if lists else None, n_lists, nq, K, capi._ptr(o) if out else None,
                                          100, C.byref(p), C.byref(r) if result else None)
    assert call(0, 512, 4, 16, result=True) == capi.CHIP_OK and call(1, 512, 8, 8) == capi.CHIP_OK
    for form, nq in ((0, 3), (1, 4)):
        assert call(form, 513, nq, 8) == capi.CHIP_ERR_UNSUPPORTED
        assert call(form, 8, nq, 0) == capi.CHIP_ERR_UNSUPPORTED
        assert call(form, 8, nq, 17) == capi.CHIP_ERR_UNSUPPORTED
        assert call(form, 0, nq, 8) == capi.CHIP_ERR_INVALID_ARG
        assert call(form, 8, nq, 8, lists=False) == capi.CHIP_ERR_INVALID_ARG
        assert call(form, 8, nq, 8, out=False) == capi.CHIP_ERR_INVALID_ARG
    assert call(0, 8, 5, 8) == capi.CHIP_ERR_UNSUPPORTED and call(0, 8, 0, 8) == capi.CHIP_ERR_UNSUPPORTED
    assert call(1, 8, 6, 8) == capi.CHIP_ERR_UNSUPPORTED and call(1, 8, 3, 8) == capi.CHIP_ERR_UNSUPPORTED
    assert call(2, 8, 4, 8) == capi.CHIP_ERR_UNSUPPORTED
    assert lib.chip_debug_merge_lists(None, 0, None, 1, 1, 1, None, 0, None, None) == capi.CHIP_ERR_INVALID_ARG
    with capi.Chip(64, devices=[0, 0]) as group:
        assert call(0, 8, 3, 8, h=group.h) == capi.CHIP_ERR_UNSUPPORTED
    # the call leaves the ctx usable
    c = CASES[0]
    s, i, _ = chip.debug_merge_lists(0, *c.arrays())
    assert np.array_equal(i, mc.reference(c, 0)[1])
