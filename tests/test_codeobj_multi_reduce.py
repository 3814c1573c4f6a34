"""Build-time look at the reduction block of the several-ticks-per-pass scan kernel (cerebro_amd/csrc/kernels.hip, db_scan_topk_multi<2> /
<3>) in the gfx950 code object of the built libcerebro_hip.so (no GPU needed).

When the R = 4 rows of a group are complete, their R x NQ lane sums are formed TRANSPOSED: step 32 of the pairing tree by
v_permlane32_swap on two rows at a time, step 16 by v_permlane16_swap on the two results, steps 8, 4, 2, 1 by DPP moves on the one register
that is left per query -- no LDS instruction, no wait, a quarter of the additions.  The block is the basic block between the branch that
closes a batch (the first branch after the loop body's last re-issued row load) and the first branch of the offers (the one vector
compare per query that decides whether any row of the group is offered at all).  Checked in both instantiations:
  * no ds_bpermute_b32 and no `s_waitcnt lgkmcnt(0)` (nothing crosses lanes through LDS);
  * R NQ / 2 x 2 v_permlane32_swap, R NQ / 4 x 2 v_permlane16_swap, NQ x 4 x 2 v_mov_b32_dpp, at most R NQ x 7 / 4 v_add_f64;
  * no DPP move is preceded by a `v_mov_b32 vN, 0` that fills in its destination (the controls used read a valid lane everywhere);
  * NQ vector compares (the pre-check of the offers) and not one v_readlane_b32: the scores leave the vector registers only in the walk
    behind the branch.
Register budget and the ownership of the load slots are tests/test_codeobj_multi.py's business."""
import re

import pytest

from test_codeobj_multi import _listings, _parse, _steady_loop
from test_codeobj_registers import LLVM, SO

pytestmark = pytest.mark.needs_hip_build

R = 4


def _is_branch(text):
    return _parse(text)[0].startswith(("s_cbranch", "s_branch"))


def _reduction_block(ins):
    first, last = _steady_loop(ins)
    assert first is not None and last > first
    end = next(i for i in range(last, len(ins)) if _is_branch(ins[i]))          # closes the batch: taken while the group is incomplete
    nxt = next(i for i in range(end + 1, len(ins)) if _is_branch(ins[i]))       # the first branch of the offers
    return ins[end + 1:nxt]


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_multi_scan_reduction_is_transposed_and_stays_in_registers(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        nq = 6 if "ILi2E" in name else 9
        block = _reduction_block(ins)
        ops = [_parse(t)[0] for t in block]

        def count(prefix):
            return sum(o.startswith(prefix) for o in ops)

        assert count("ds_") == 0, (name, [t for t in block if t.startswith("ds_")][:4])
        assert not any(o == "s_waitcnt" and "lgkmcnt(0)" in t for o, t in zip(ops, block)), name
        assert not any(o.startswith(("global_", "scratch_", "buffer_")) for o in ops), name
        assert count("v_permlane32_swap_b32") == R * nq // 2 * 2, (name, count("v_permlane32_swap_b32"))
        assert count("v_permlane16_swap_b32") == R * nq // 4 * 2, (name, count("v_permlane16_swap_b32"))
        assert count("v_mov_b32_dpp") == nq * 4 * 2, (name, count("v_mov_b32_dpp"))
        assert nq * 6 <= count("v_add_f64") <= R * nq * 7 // 4, (name, count("v_add_f64"))
        for i, t in enumerate(block):
            if ops[i] == "v_mov_b32_dpp":
                assert "bound_ctrl:1" in t, (name, t)
                prev = block[i - 1] if i else ""
                assert not re.fullmatch(r"v_mov_b32(_e32)? v\d+, 0", prev), (name, prev, t)
        assert count("v_cmp_") == nq and all(o.endswith(("f64_e32", "f64_e64", "f64")) for o in ops if o.startswith("v_cmp_")), \
            (name, [t for t in block if t.startswith("v_cmp_")])
        assert count("v_readlane_b32") == 0, name


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_multi_scan_kernel_has_no_cross_lane_lds_exchange_left_in_its_loop(tmp_path):
    """The only ds_bpermute_b32 of the kernel are those of the block merge behind the scan loop (once per workgroup), and the walk of the
    offers takes row rr's score from lane 16 rr."""
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        first, last = _steady_loop(ins)
        perm = [i for i, t in enumerate(ins) if _parse(t)[0] == "ds_bpermute_b32"]
        assert all(i < first or i > last for i in perm), (name, perm[:5], first, last)
        assert len(perm) <= 32, (name, len(perm))          # R x NQ x 2 x 2 of them would be the butterfly's steps 32 and 16
        # the walk of the offers reads the four rows' scores out of the four 16-lane rows of the wave
        lanes = {int(_parse(t)[1][2]) for t in ins if _parse(t)[0] == "v_readlane_b32" and len(_parse(t)[1]) == 3 and _parse(t)[1][2].isdigit()}
        assert {0, 16, 32, 48} <= lanes, (name, sorted(lanes))
