"""Build-time look at the double-row instantiations of the many-query kernel (cerebro_amd/csrc/batch.hip, db_gemm_topk<.., double>:
the form chip_query_batch_cast_f32 launches) in the gfx950 code object of the built libcerebro_hip.so (no GPU needed).  Only the
B-side loader differs from the float kernel: rows come in through registers (global_load_dwordx4), are narrowed with v_cvt_f32_f64
and stored into the same LDS image; the MFMA loop is the float kernel's, so the count of matrix instructions is the same; nothing
spills, and the 256 x 256 form still fits the 256 registers a wave of an 8-wave workgroup per CU can have."""
import re
import subprocess

import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings, code_objects

pytestmark = pytest.mark.needs_hip_build

# db_gemm_topk<KC = 32, WN, KL, ROW>: _ZN4chip12db_gemm_topkILi32ELi<WN>ELi<KL>E<f|d>EEvNS_9BatchArgsE
NAME = re.compile(r"db_gemm_topkILi32ELi(\d+)ELi(\d+)E([fd])EE")


def _forms(tmp_path):
    out = {}
    for k, ins in _kernel_listings(tmp_path, lambda k: "db_gemm_topk" in k and not k.endswith(".kd")).items():
        m = NAME.search(k)
        assert m, k
        out[(int(m.group(1)), int(m.group(2)), m.group(3))] = [t.split(None, 1)[0] for t in ins if t]
    return out


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_double_row_forms_of_db_gemm_topk(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    forms = _forms(tmp_path)
    dbl = {k: v for k, v in forms.items() if k[2] == "d"}
    assert {k[0] for k in dbl} == {2, 4}, sorted(dbl)                  # both tile shapes
    assert {k[1] for k in dbl} == {8, 16}, sorted(dbl)                 # both list capacities (16 entries: the small tile only -- next to
    #                                                                     128 accumulators the staging does not fit the wide form's 256 registers)
    for (wn, kl, _), ops in dbl.items():
        count = lambda prefix: sum(o.startswith(prefix) for o in ops)      # noqa: E731
        assert count("scratch_") == 0, (wn, kl, "spills")
        assert count("flat_") == 0, (wn, kl, "flat_ memory instructions")
        assert count("v_cvt_f32_f64") >= 16, (wn, kl)                   # 4 slots x 4 elements per thread and chunk
        assert count("ds_write_b128") + count("ds_write_b64") + count("ds_write2_b64") >= 1, (wn, kl)
        assert count("global_load_dwordx4") >= 8, (wn, kl)              # the rows: 2 x 16 bytes per slot
        twin = forms[(wn, kl, "f")]
        assert count("v_mfma_f32_32x32x2") == sum(o.startswith("v_mfma_f32_32x32x2") for o in twin) > 0, (wn, kl)


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_wide_double_row_form_fits_one_workgroup_of_eight_waves_per_cu(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    seen = 0
    for co in code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            m = NAME.search(name)
            if not m or m.group(3) != "d" or name.endswith(".kd"):
                continue
            get = lambda key: int(re.search(key + r":\s+(\d+)", block).group(1))   # noqa: E731
            assert get(r"\.vgpr_spill_count") == 0 and get(r"\.private_segment_fixed_size") == 0, name
            if m.group(1) == "4":
                assert get(r"\.vgpr_count") <= 256, (name, get(r"\.vgpr_count"))     # unified file: AGPRs included, 2 waves per SIMD
                seen += 1
    assert seen >= 1
