"""Build-time look at the load stream of the several-ticks-per-pass scan kernel (cerebro_amd/csrc/kernels.hip, db_scan_topk_multi<2> /
<3>) in the gfx950 code object of the built libcerebro_hip.so (no GPU needed).  What the continuous stream relies on:
  * at most 256 registers per lane, nothing spilled, no scratch (two waves per SIMD, and a scratch access would be waited for with
    vmcnt(0), which drains the stream);
  * the load slots are registers the compiler does not own: nothing but the kernel's global_load_dwordx4 writes v[192..255], nothing
    but the v_cvt_f64_f32 of the take statements reads them;
  * inside the steady-state loop every wait on the row loads is COUNTED: no `s_waitcnt vmcnt(0)` between the first and the last
    re-issued row load of the loop body, and each of those waits leaves loads in flight;
  * the query vectors are read ahead: a ds_read_b128 of the loop body is never waited for with lgkmcnt(0) within the next few
    instructions -- the wave has other arithmetic to issue while the read is in flight."""
import re

import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings, code_objects, regs_of
from test_codeobj_scan_multi import _metadata

pytestmark = pytest.mark.needs_hip_build

LO, HI = 192, 255
NEAR = 8          # "the next few instructions"


def _parse(text):
    parts = text.split(None, 1)
    op = parts[0]
    operands = [o.strip().split()[0] for o in parts[1].split(",") if o.strip()] if len(parts) > 1 else []
    return op, operands


def _listings(tmp_path):
    ks = {k: [t for t in v if t] for k, v in _kernel_listings(tmp_path, lambda k: "db_scan_topk_multi" in k).items() if not k.endswith(".kd")}
    assert len(ks) == 2, sorted(ks)
    return ks


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_multi_scan_register_budget(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    md = _metadata(tmp_path)
    assert len(md) == 2, sorted(md)
    for name, m in md.items():
        assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 256, (name, m)
        assert int(m["private_segment_fixed_size"]) == 0 and int(m.get("vgpr_spill_count", 0)) == 0 and int(m.get("sgpr_spill_count", 0)) == 0, (name, m)


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_multi_scan_load_slots_belong_to_the_asm_statements(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        n_loads = n_takes = 0
        for text in ins:
            op, operands = _parse(text)
            assert not op.startswith("scratch_"), (name, text)
            touched = [(i, r) for i, o in enumerate(operands) for r in regs_of(o) if LO <= r <= HI]
            if not touched:
                continue
            if op == "global_load_dwordx4":
                assert all(i == 0 for i, _ in touched), (name, text)        # the destination, and nothing else
                n_loads += 1
            elif op in ("v_cvt_f64_f32_e32", "v_cvt_f64_f32"):
                assert all(i == 1 for i, _ in touched), (name, text)        # the source, and nothing else
                n_takes += 1
            else:
                raise AssertionError(f"{name}: compiler-owned instruction touches a load slot: {text}")
        # every slot register is loaded (prologue and loop) and taken
        assert n_loads >= 2 * 16 and n_takes >= 4 * 16, (name, n_loads, n_takes)


def _steady_loop(ins):
    """(first, last) listing index of the loop body's re-issued row loads: the slot loads that follow a take of the same registers."""
    first = last = None
    for i, text in enumerate(ins):
        op, operands = _parse(text)
        if op != "global_load_dwordx4" or not any(LO <= r <= HI for r in regs_of(operands[0])):
            continue
        dest = set(regs_of(operands[0]))
        taken = {r for t in ins[max(0, i - 6):i] if _parse(t)[0].startswith("v_cvt_f64_f32") for o in _parse(t)[1][1:] for r in regs_of(o)}
        if dest <= taken:
            first = i if first is None else first
            last = i
    return first, last


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_multi_scan_steady_state_waits_are_counted_and_queries_are_read_ahead(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        first, last = _steady_loop(ins)
        assert first is not None and last > first, name
        end = next(i for i in range(last, len(ins)) if _parse(ins[i])[0].startswith(("s_cbranch", "s_branch")))   # the arithmetic of the last KiB
        body = ins[first - 8:end]
        assert sum(_parse(t)[0] == "global_load_dwordx4" for t in body) == 16, name       # one body: every slot is re-issued exactly once
        vm = [int(m.group(1)) for t in body for m in [re.search(r"vmcnt\((\d+)\)", t)] if m and _parse(t)[0] == "s_waitcnt"]
        assert vm and min(vm) >= 8, (name, sorted(set(vm)))        # counted waits: at least 8 KiB stay in flight behind each of them
        reads = [i for i, t in enumerate(body) if _parse(t)[0].startswith("ds_read_b128")]
        nq = 6 if "ILi2E" in name else 9
        assert len(reads) == 4 * nq, (name, len(reads))
        for i in reads:
            for t in body[i + 1:i + 1 + NEAR]:
                if _parse(t)[0].startswith(("ds_read", "global_load")):
                    break                                           # the wave goes on issuing memory operations: nothing waited for yet
                assert not (_parse(t)[0] == "s_waitcnt" and "lgkmcnt(0)" in t), f"{name}: query read at body[{i}] is waited for at once: {t}"
