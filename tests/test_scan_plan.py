"""CPU tests of the scan dispatcher's POLICY (no GPU): which kernel form chip_debug_scan_plan -- the functions the enqueue path itself
runs, on a ctx that exists on the host only -- chooses, at default knobs and under every documented knob.  Three claims:
  * the documented policy (the comment block of scan_rows_form) as a table, one assertion per sentence;
  * every ctx chip_create accepts has a launchable plan for every call;
  * the planner cannot reach a form that tests/scan_form_cases.py does not name, i.e. that tests/test_scan_forms_gpu.py does not
    hold against the oracle on the device."""
import pytest

import scan_form_cases as sfc
from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
Q, T, S = capi.CHIP_SCAN_CALL_QUERY, capi.CHIP_SCAN_CALL_TICK, capi.CHIP_SCAN_CALL_TICK_SYNC
MIB = 1 << 20


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in sfc.SCAN_ENV:
        monkeypatch.delenv(k, raising=False)


def plan(D, rows, call=T, nq=3, K=8, elem=4, n_cus=sfc.N_CUS):
    return capi.scan_plan(D, elem, nq, K, rows, call, n_cus)


def is_form(p, form):
    return all(p[f] == form[f] for f in sfc.FORM_FIELDS)


def shape(p):
    return p["grid"], p["block"]


# ------------------------------------------------------------------------------------------------ the documented policy
def test_policy_4096_d():
    p = plan(4096, 10_000)                                   # 164 MB: rows form, R = 1, temporal, one workgroup per CU, static rows, fused
    assert is_form(p, sfc.rows(1, fused=1)) and shape(p) == (256, 512) and p["K"] == 1
    assert is_form(plan(4096, 10_000, Q), sfc.rows(1)) and plan(4096, 10_000, Q)["K"] == 8
    p = plan(4096, 29_000)                                   # 475 MB, the reference's capacity: both workgroup slots, rows claimed
    assert is_form(p, sfc.rows(1, claimed=1, fused=1)) and shape(p) == (512, 512)
    p = plan(4096, 100_000, S)                               # 1.6 GB synchronous: one fused launch, non-temporal loads
    assert is_form(p, sfc.rows(1, ntl=1, claimed=1, fused=1)) and shape(p) == (512, 512)
    p = plan(4096, 100_000, T)                               # ... pipelined: the one-row kernel
    assert is_form(p, sfc.one(4, 6)) and shape(p) == (512, 512)
    p = plan(4096, 1_000_000)                                # 16 GB: queries staged as fp64, one 1024-thread workgroup per CU, 96 KiB
    assert is_form(p, sfc.one(4, 8)) and shape(p) == (256, 1024) and p["lds_bytes"] == 96 * 1024 and p["wg_per_cu"] == 1
    assert is_form(plan(4096, 1_000_000, S), sfc.one(4, 8))  # beyond CHIP_SCAN_SYNC_PLAIN_MIB the synchronous tick is a long scan too
    assert is_form(plan(4096, 49_152), sfc.rows(1, claimed=1, fused=1))      # exactly 768 MiB: still temporal
    assert is_form(plan(4096, 49_153), sfc.one(4, 6))
    assert shape(plan(4096, 12_288)) == (256, 512) and shape(plan(4096, 12_289)) == (512, 512)   # 192 MiB: half occupancy ends


def test_policy_8192_d():
    for call in (S, T):                                      # 0.95 GB, the reference's default model at its capacity: R = 2, non-temporal
        p = plan(8192, 29_000, call)
        assert is_form(p, sfc.rows(2, ntl=1, fused=1)) and shape(p) == (256, 1024) and p["wg_per_cu"] == 1
    assert is_form(plan(8192, 29_000, Q), sfc.rows(2, ntl=1))
    assert is_form(plan(8192, 29_000, Q, nq=4), sfc.one(4, 6))              # four queries: never R > 1 (and no temporal R = 1 beyond 768 MiB)
    assert is_form(plan(8192, 20_000), sfc.rows(1, fused=1))                # 655 MB: R = 1, temporal
    assert is_form(plan(8192, 65_536), sfc.rows(2, ntl=1, fused=1))         # exactly 2 GiB
    assert is_form(plan(8192, 65_537, T), sfc.one(4, 6))                    # beyond 2 GiB pipelined: the one-row kernel
    assert is_form(plan(8192, 65_537, S), sfc.rows(2, ntl=1, fused=1))      # synchronous: up to 4 GiB
    assert is_form(plan(8192, 131_073, S), sfc.one(4, 6))
    assert is_form(plan(7168, 40_000, S), sfc.rows(1, ntl=1, fused=1))      # rows below 32 KiB: R = 1


def test_policy_nq4_never_more_than_one_row_per_wave(monkeypatch):
    for rows_knob in (None, "1", "2", "3"):
        if rows_knob:
            monkeypatch.setenv("CHIP_SCAN_ROWS", rows_knob)
        for D, elem in ((1024, 4), (4096, 4), (8192, 4), (512, 8), (4096, 8)):
            for n in (100, 29_000, 60_000):
                p = plan(D, n, Q, nq=4, elem=elem)
                assert p["family"] != "rows" or p["R"] == 1, (rows_knob, D, elem, n, p)


def test_policy_double_rows_and_odd_row_sizes():
    assert is_form(plan(4096, 1200, Q, elem=8), sfc.rows(1)) and shape(plan(4096, 29_000, Q, elem=8)) == (256, 1024)
    assert is_form(plan(4096, 29_000, S, elem=8), sfc.rows(2, ntl=1, fused=1))     # 32 KiB rows of doubles: as 8192-D floats
    p = plan(8192, 400, Q, elem=8)                            # three double queries of 64 KiB do not fit the LDS: one is read in place
    assert is_form(p, sfc.wide(1, 1)) and p["block"] == 1024 and p["lds_bytes"] == 128 * 1024
    assert is_form(plan(8192, 400, Q, nq=4, elem=8), sfc.wide(2, 1)) and is_form(plan(8200, 400, Q, elem=8), sfc.wide(1, 0))
    assert is_form(plan(6144, 400, Q, nq=4, elem=8), sfc.wide(1, 1)) and is_form(plan(6824, 400, Q, nq=4, elem=8), sfc.wide(1, 0))
    assert is_form(plan(1536, 400, Q), sfc.one(2, 6)) and is_form(plan(768, 400, Q, elem=8), sfc.one(2, 6))    # rows of 2048 x odd bytes
    assert is_form(plan(1000, 400, Q), sfc.one(8, 1, FULL=0)) and is_form(plan(4100, 400, Q), sfc.one(8, 1, FULL=0))
    assert is_form(plan(1000, 400, Q, elem=8), sfc.one(8, 1, FULL=0))


KNOB_MOVES = [   # (knobs, plan arguments, form, shape or None): every documented knob moves the plan the way README says
    ({"CHIP_SCAN_ROWS": "-1"}, (4096, 10_000, T), sfc.one(4, 6), (256, 512)),
    ({"CHIP_SCAN_ROWS": "1"}, (4096, 100_000, T), sfc.rows(1, ntl=1, claimed=1, fused=1), (512, 512)),
    ({"CHIP_SCAN_ROWS": "2"}, (4096, 10_000, T), sfc.rows(2, fused=1), (256, 512)),
    ({"CHIP_SCAN_ROWS": "3"}, (4096, 10_000, Q), sfc.rows(3), (256, 512)),
    ({"CHIP_SCAN_CLAIM": "0"}, (4096, 29_000, T), sfc.rows(1, fused=1), (512, 512)),
    ({"CHIP_SCAN_CLAIM": "1"}, (4096, 10_000, T), sfc.rows(1, claimed=1, fused=1), (256, 512)),
    ({"CHIP_SCAN_SHORT_BPC": "0"}, (4096, 10_000, T), sfc.rows(1, claimed=1, fused=1), (512, 512)),
    ({"CHIP_SCAN_HALF_MIB": "0"}, (4096, 10_000, T), sfc.rows(1, claimed=1, fused=1), (512, 512)),
    ({"CHIP_SCAN_HALF_MIB": "512"}, (4096, 29_000, T), sfc.rows(1, fused=1), (256, 512)),
    ({"CHIP_SCAN_PLAIN_MIB": "0"}, (4096, 10_000, T), sfc.one(4, 6), (256, 512)),
    ({"CHIP_SCAN_PLAIN_MIB": "0"}, (4096, 10_000, S), sfc.rows(1, ntl=1, fused=1), (256, 512)),
    ({"CHIP_SCAN_PLAIN_MIB": "2048"}, (4096, 100_000, T), sfc.rows(1, claimed=1, fused=1), (512, 512)),
    ({"CHIP_SCAN_SYNC_PLAIN_MIB": "0"}, (4096, 100_000, S), sfc.one(4, 6), (512, 512)),
    ({"CHIP_SCAN_OVERLAP_GIB": "0"}, (4096, 10_000, T), sfc.one(4, 8), (256, 1024)),
    ({"CHIP_SCAN_OVERLAP_GIB": "32"}, (4096, 1_000_000, T), sfc.one(4, 6), (512, 512)),
    ({"CHIP_SCAN_RESERVE": "4"}, (4096, 10_000, T), sfc.rows(1, fused=1), (252, 512)),
    ({"CHIP_SCAN_RESERVE": "4"}, (4096, 29_000, T), sfc.rows(1, claimed=1, fused=1), (508, 512)),
    ({"CHIP_SCAN_RESERVE": "4"}, (8192, 29_000, T), sfc.rows(2, ntl=1, fused=1), (252, 1024)),
    ({"CHIP_SCAN_VARIANT": "1"}, (4096, 10_000, T), sfc.one(8, 1), (256, 512)),
    ({"CHIP_SCAN_VARIANT": "1"}, (4096, 1_000_000, T), sfc.one(8, 1), (512, 512)),
    ({"CHIP_SCAN_VARIANT": "7"}, (4096, 1_000_000, T), sfc.one(4, 6), (512, 512)),
    ({"CHIP_SCAN_VARIANT": "7"}, (4096, 10_000, T), sfc.rows(1, fused=1), (256, 512)),
    ({"CHIP_TICK_FUSED": "0"}, (4096, 10_000, T), sfc.rows(1), (256, 512)),
]


@pytest.mark.parametrize("knobs,args,form,grid_block", KNOB_MOVES, ids=[f"{k}-{a[1]}-{a[2]}" for k, a, _, _ in KNOB_MOVES])
def test_documented_knobs_move_the_plan(monkeypatch, knobs, args, form, grid_block):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    p = plan(*args)
    assert is_form(p, form), p
    assert shape(p) == grid_block, p


# ------------------------------------------------------------------------------------------------ every ctx can scan
CALLS = [(Q, 1), (Q, 2), (Q, 3), (Q, 4), (T, 3), (S, 3)]
ROW_COUNTS = (0, 1, 63, 4097, 29_000, 1_000_000)


def check_launchable(D, elem, nq, K, n, call):
    rc, p = capi.scan_plan(D, elem, nq, K, n, call, sfc.N_CUS, check=False)
    where = (D, elem, nq, K, n, call, p)
    assert rc == capi.CHIP_OK, where
    assert p["lds_bytes"] * p["wg_per_cu"] <= 160 * 1024 and p["wg_per_cu"] in (1, 2), where
    assert 1 <= p["grid"] <= 512 and p["block"] == (512 if p["wg_per_cu"] == 2 else 1024), where
    assert p["grid"] <= sfc.N_CUS * p["wg_per_cu"] and p["nq"] == nq and p["elem"] == elem and p["n_rows"] == n, where
    row_bytes = D * elem
    if p["family"] == "wide":
        assert elem == 8 and (nq, p["NG"]) in ((3, 1), (4, 1), (4, 2)) and p["FULL"] == (D % 512 == 0), where
        assert (nq - p["NG"]) * row_bytes <= p["lds_bytes"], where
    elif p["family"] == "rows":
        assert row_bytes % 4096 == 0 and 1 <= p["R"] <= (1 if nq == 4 else 3) and not p["q64"], where
        assert nq * row_bytes < p["lds_bytes"], where
        assert not p["claimed"] or p["R"] == 1, where
        assert not p["fused"] or (nq == 3 and p["K"] == 1 and call != Q), where
    else:
        assert p["family"] == "one_row" and (p["U"], p["NT"]) in ((4, 8), (4, 6), (2, 6), (8, 1)), where
        assert p["FULL"] == (row_bytes % (1024 * p["U"]) == 0) and (p["FULL"] or p["NT"] == 1), where
        assert (p["NT"] == 8) == bool(p["q64"]) and (not p["q64"] or elem == 4), where
        assert nq * D * (8 if p["q64"] else elem) <= p["lds_bytes"], where
        assert not p["claimed"] and not p["fused"] and not p["NTL"], where
    if not p["fused"]:
        assert p["K"] == K, where
    return p


def test_every_accepted_ctx_has_a_launchable_plan():
    """D % 4 == 0 up to 10 240 (what chip_create accepts), both storage types, every query count, K = 1 and 16, six prefix sizes, every
    call: CHIP_OK, LDS within the 160 KiB of a CU for the workgroups meant to share it, a grid K2 can merge, an instantiation that exists."""
    seen = set()
    for D in range(4, 10_240 + 1, 4):
        for elem in (4, 8):
            for call, nq in CALLS:
                for K in (1, 16):
                    for n in ROW_COUNTS:
                        p = check_launchable(D, elem, nq, K, n, call)
                        seen.add(sfc.form_key(p, elem, nq))
    named = set().union(*(c.keys() for c in sfc.CASES))
    assert seen <= named, sorted(seen - named)
    # what chip_create refuses has no plan either
    for D, elem in ((10_244, 4), (10_244, 8), (4098, 4), (12_288, 8)):
        assert capi.scan_plan(D, elem, 3, 8, 100, Q, sfc.N_CUS, check=False)[0] == capi.CHIP_ERR_UNSUPPORTED


SWEEP_D = sorted(set(range(256, 10_240 + 1, 256)) | {4, 252, 768, 1000, 1536, 4100, 6824, 6828, 8200, 10_236})


@pytest.mark.parametrize("knobs", sfc.KNOB_SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "default")
def test_no_reachable_form_without_a_gpu_parity_case(monkeypatch, knobs):
    """Every form the planner can yield -- over row sizes of every kind, both storage types, every call, six prefix sizes, each documented
    knob -- is named by a row of scan_form_cases.CASES.  A new instantiation in the dispatcher without a parity case fails here."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    named = set().union(*(c.keys() for c in sfc.CASES))
    missing = {}
    for D in SWEEP_D:
        for elem in (4, 8):
            for call, nq in CALLS:
                for n in ROW_COUNTS:
                    p = check_launchable(D, elem, nq, 8, n, call)
                    key = sfc.form_key(p, elem, nq)
                    if key not in named:
                        missing.setdefault(key, (D, elem, nq, n, call))
    assert not missing, [dict(zip(sfc.FORM_FIELDS + ("elem", "nq"), k), at=v) for k, v in sorted(missing.items(), key=str)]


# ------------------------------------------------------------------------------------------------ the case table itself
@pytest.mark.parametrize("case", sfc.CASES, ids=repr)
def test_case_rows_name_what_the_planner_chooses(monkeypatch, case):
    """Each row of the form matrix, under its knobs and at its own size: the planner chooses the form, grid and block the row names."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    N, W, R, wpb = sfc.case_geometry(case, lambda *a: capi.scan_plan(*a, sfc.N_CUS))
    assert N * case.D * case.elem <= 1.0e9 and N >= 3 * W, (N, W, R)
    for nq in case.nqs():
        p = capi.scan_plan(case.D, case.elem, nq, 8, N, sfc.CALL_CODE[case.call], sfc.N_CUS)
        assert is_form(p, case.form_for(nq)), (nq, p)
        if nq == 3:
            assert shape(p) == (case.grid, case.block), p
    ks = sfc.prefixes(W, R, wpb, N)
    assert len(ks) >= 15 and ks[-1] == N


def test_table_holds_the_rows_the_issue_names():
    names = {c.name for c in sfc.CASES}
    assert len(names) >= 55
    keys = set().union(*(c.keys() for c in sfc.CASES))
    for R in (1, 2, 3):
        for ntl in (0, 1):
            for elem in (4, 8):
                assert any(k[0] == "rows" and k[5] == R and k[6] == ntl and k[10] == elem for k in keys), (R, ntl, elem)
    bench = [c for c in sfc.CASES if c.n_rows == 29_000 and c.D == 8192 and not c.env]
    assert {c.call for c in bench} == {sfc.QUERY, sfc.TICK, sfc.SYNC} and all(c.form["R"] == 2 for c in bench)
