"""Build-time look at the shared-pass scan kernel for DOUBLE rows (cerebro_amd/csrc/kernels.hip, db_scan_shared_f64<T, NG>: T pipelined
ticks per pass, NG of the 3 T fp64 queries read in place) in the gfx950 code object of the built libcerebro_hip.so (no GPU needed).
The checks are those of tests/test_codeobj_scan_multi.py and tests/test_codeobj_multi.py for the float kernel, with what differs:
  * the instantiations: T = 2 with NG = 0, 1, 2 (one kernel per T and per number of in-place queries the plan can ask for);
  * the asm-owned registers are the row slots v[192..255] AND the in-place query slots v[192 - 16 NG .. 191]; the compiler keeps
    below v160 in every instantiation; a slot is written by the kernel's global_load_dwordx4 only and read by the v_mov_b64 of the
    take statements only;
  * the in-place query loads are part of the in-order stream: the walk over outstanding loads runs with them in it, every wait of the
    steady loop is counted and leaves at least 8 loads in flight, and one loop body re-issues 16 row slots and 4 NG query slots;
  * arithmetic: at least 4 KiB x 2 elements x 4 rows x 3 T fp64 fma per batch body."""
import re
import subprocess

import pytest

from test_codeobj_multi import _parse
from test_codeobj_registers import LLVM, SO, _kernel_listings, code_objects, regs_of

pytestmark = pytest.mark.needs_hip_build

NAME = "db_scan_shared_f64"
ROW_LO, HI, COMPILER_TOP = 192, 255, 160
BUILT = {(2, 0), (2, 1), (2, 2)}          # (T, NG)


def _t_ng(name):
    m = re.search(NAME + r"ILi(\d+)ELi(\d+)E", name)
    assert m, name
    return int(m.group(1)), int(m.group(2))


def _listings(tmp_path):
    ks = {k: [t for t in v if t] for k, v in _kernel_listings(tmp_path, lambda k: NAME in k).items() if not k.endswith(".kd")}
    assert {_t_ng(k) for k in ks} == BUILT and len(ks) == len(BUILT), sorted(ks)
    return ks


def _metadata(tmp_path):
    """{kernel name: {key: value}} of the AMDGPU metadata notes, as test_codeobj_scan_multi._metadata reads them, for this kernel"""
    out = {}
    for co in code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        cur = {}
        for line in notes.splitlines():
            m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
            if not m:
                continue
            key, val = m.groups()
            if line.lstrip().startswith("- ."):      # first key of a new list item
                cur = {}
            cur[key] = val
            if "name" in cur:
                out[cur["name"]] = cur
    return {k: v for k, v in out.items() if NAME in k and not k.endswith(".kd")}


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_shared_f64_budget_no_scratch_no_static_lds(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    md = _metadata(tmp_path)
    assert {_t_ng(k) for k in md} == BUILT, sorted(md)
    for name, m in md.items():
        assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 256, (name, m)
        assert int(m["private_segment_fixed_size"]) == 0, (name, m)
        assert int(m.get("vgpr_spill_count", 0)) == 0 and int(m.get("sgpr_spill_count", 0)) == 0, (name, m)
        assert int(m["group_segment_fixed_size"]) == 0, name            # all LDS is the launch's: staged queries + lists
        assert int(m["max_flat_workgroup_size"]) == 512, name


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_shared_f64_slots_belong_to_the_asm_statements(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        T, NG = _t_ng(name)
        q_lo = ROW_LO - 16 * NG
        loads, takes = set(), set()
        n_fma = 0
        for text in ins:
            op, operands = _parse(text)
            assert not op.startswith("scratch_"), (name, text)
            assert not op.startswith("flat_"), (name, text)
            n_fma += op.startswith(("v_fma_f64", "v_fmac_f64"))
            touched = [(i, r) for i, o in enumerate(operands) for r in regs_of(o) if COMPILER_TOP <= r <= HI]
            if not touched:
                continue
            assert all(r >= q_lo for _, r in touched), f"{name}: v[{COMPILER_TOP}..{q_lo - 1}] belong to nobody: {text}"
            if op == "global_load_dwordx4":
                assert all(i == 0 for i, _ in touched), (name, text)        # the destination, and nothing else
                loads.update(r for _, r in touched)
                assert ("nt" in text.split()) == (min(r for _, r in touched) >= ROW_LO), (name, text)   # rows stream, queries stay cached
            elif op in ("v_mov_b64", "v_mov_b64_e32"):
                assert all(i == 1 for i, _ in touched), (name, text)        # the source, and nothing else
                takes.update(r for _, r in touched)
            else:
                raise AssertionError(f"{name}: compiler-owned instruction touches a load slot: {text}")
        assert loads == takes == set(range(q_lo, HI + 1)), (name, sorted(set(range(q_lo, HI + 1)) - loads), sorted(set(range(q_lo, HI + 1)) - takes))
        assert n_fma >= 4 * 2 * 4 * 3 * T, (name, n_fma)


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_shared_f64_loads_are_not_touched_before_their_wait(tmp_path):
    """the in-order walk of test_multi_scan_loads_are_not_touched_before_their_wait, with the in-place query loads in the stream"""
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    n_checked = 0
    for name, ins in _listings(tmp_path).items():
        pending = []          # oldest first: the VGPRs each outstanding vector-memory operation will write
        for text in ins:
            op, ops = _parse(text)
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", text)
                if m:
                    pending = pending[max(0, len(pending) - int(m.group(1))):] if int(m.group(1)) else []
                continue
            if op in ("s_branch", "s_endpgm", "s_setpc_b64"):
                pending = []
                continue
            touched = {r for o in ops for r in regs_of(o)}
            busy = set().union(*pending) if pending else set()
            assert not (touched & busy), f"{name}: `{text}` touches {sorted(touched & busy)} while their load is in flight"
            if op.startswith(("global_load", "buffer_load", "scratch_load")):
                pending.append(set(regs_of(ops[0])))
                n_checked += 1
            elif op.startswith(("global_store", "buffer_store", "scratch_store", "global_atomic")):
                pending.append(set())
    assert n_checked >= len(BUILT) * 2 * 16


def _steady_loop(ins, q_lo):
    """(first, last) listing index of the loop body's re-issued slot loads: those that follow a take of the same registers"""
    first = last = None
    for i, text in enumerate(ins):
        op, operands = _parse(text)
        if op != "global_load_dwordx4" or not any(q_lo <= r <= HI for r in regs_of(operands[0])):
            continue
        dest = set(regs_of(operands[0]))
        taken = {r for t in ins[max(0, i - 6):i] if _parse(t)[0].startswith("v_mov_b64") for o in _parse(t)[1][1:] for r in regs_of(o)}
        if dest <= taken:
            first = i if first is None else first
            last = i
    return first, last


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_shared_f64_steady_state_waits_are_counted(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        T, NG = _t_ng(name)
        first, last = _steady_loop(ins, ROW_LO - 16 * NG)
        assert first is not None and last > first, name
        end = next(i for i in range(last, len(ins)) if _parse(ins[i])[0].startswith(("s_cbranch", "s_branch")))
        body = ins[first - 8:end]
        loads = [_parse(t)[1][0] for t in body if _parse(t)[0] == "global_load_dwordx4"]
        assert len(loads) == 16 + 4 * NG, (name, len(loads))               # one body: every row and query slot is re-issued exactly once
        # the stream's order: per KiB the four row slots, then the NG query slots
        want = [(ROW_LO + 16 * u + 4 * rr) for u in range(4) for rr in range(4)]
        rows = [min(regs_of(o)) for o in loads if min(regs_of(o)) >= ROW_LO]
        assert rows == want, (name, rows)
        vm = [int(m.group(1)) for t in body for m in [re.search(r"vmcnt\((\d+)\)", t)] if m and _parse(t)[0] == "s_waitcnt"]
        assert len(vm) >= 16 + 4 * NG and min(vm) >= 8, (name, sorted(set(vm)))        # counted waits: at least 8 KiB stay in flight behind each
        assert not [t for t in body if _parse(t)[0] == "s_waitcnt" and re.search(r"vmcnt\(0\)", t)], name
        n_fma = sum(_parse(t)[0].startswith(("v_fma_f64", "v_fmac_f64")) for t in body)
        assert n_fma >= 4 * 2 * 4 * 3 * T, (name, n_fma)
        reads = sum(_parse(t)[0].startswith("ds_read_b128") for t in body)
        assert reads == 4 * (3 * T - NG), (name, reads)                   # the staged queries, 16 bytes per lane
