"""Build-time look at the several-ticks-per-pass scan kernel (cerebro_amd/csrc/kernels.hip, db_scan_topk_multi<2> / <3>) in the
gfx950 code object of the built libcerebro_hip.so (no GPU needed).  What the design relies on:
  * two waves per SIMD: at most 256 registers per lane (VGPR + AGPR, one file on gfx950), nothing spilled to scratch;
  * one workgroup per CU within the 160 KiB of LDS (the launch asks for 3 T x D x 4 bytes; the static part must be zero);
  * the staged queries are read 16 bytes per lane (ds_read_b128), the rows with global_load_dwordx4, no flat_ instruction;
  * the rows are loaded from inline asm with "=v" outputs and consumed behind counted waits, as in the one-row kernel: no
    instruction may touch a register whose load is still in flight (the walk of test_codeobj_registers.py)."""
import re
import subprocess

import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings, code_objects, regs_of

pytestmark = pytest.mark.needs_hip_build

LDS_PER_CU = 163840


def _listings(tmp_path):
    ks = {k: v for k, v in _kernel_listings(tmp_path, lambda k: "db_scan_topk_multi" in k).items() if not k.endswith(".kd")}
    assert len(ks) == 2, sorted(ks)          # T = 2 and T = 3
    return ks


def _metadata(tmp_path):
    """{kernel name: {key: int}} of the AMDGPU metadata notes (vgpr_count, agpr_count, private / group segment sizes)."""
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
            if key == "name" or "name" in cur:
                out[cur.get("name", "")] = cur
    return {k: v for k, v in out.items() if "db_scan_topk_multi" in k}


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_multi_scan_has_no_spill_no_flat_and_reads_queries_16_bytes_at_a_time(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name, ins in _listings(tmp_path).items():
        ops = [t.split(None, 1)[0] for t in ins if t]
        assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
        assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"
        nq = 6 if "ILi2E" in name else 9
        assert sum(o.startswith("ds_read_b128") for o in ops) >= 4 * nq, name        # U = 4 query vectors per query and batch
        assert sum(o.startswith("global_load_dwordx4") for o in ops) >= 16, name     # R x U row loads per batch
        assert sum(o.startswith(("v_fma_f64", "v_fmac_f64")) for o in ops) >= 4 * 4 * 4 * nq, name   # U x 4 elements x R rows x NQ


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_multi_scan_fits_two_waves_per_simd_and_one_workgroup_per_cu(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    md = _metadata(tmp_path)
    assert len(md) == 2, sorted(md)
    for name, m in md.items():
        regs = int(m["vgpr_count"]) + int(m.get("agpr_count", 0))
        assert regs <= 256, (name, regs)
        assert int(m["private_segment_fixed_size"]) == 0, (name, m["private_segment_fixed_size"])
        assert int(m.get("vgpr_spill_count", 0)) == 0 and int(m.get("sgpr_spill_count", 0)) == 0, name
        assert int(m["group_segment_fixed_size"]) == 0, name            # all LDS is the launch's dynamic 3 T x D x 4 bytes
        assert int(m["max_flat_workgroup_size"]) == 512, name           # 8 waves: two per SIMD
    assert 9 * 4096 * 4 <= LDS_PER_CU                                   # three ticks of the headline shape fit one CU's LDS


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_multi_scan_loads_are_not_touched_before_their_wait(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    n_checked = 0
    for name, ins in _listings(tmp_path).items():
        pending = []          # oldest first: the VGPRs each outstanding vector-memory operation will write
        for text in ins:
            parts = text.split(None, 1)
            if not parts:
                continue
            op = parts[0]
            ops = [o.strip().split()[0] for o in parts[1].split(",")] if len(parts) > 1 else []
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
    assert n_checked >= 2 * 16
