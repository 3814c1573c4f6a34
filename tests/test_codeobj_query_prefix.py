"""Build-time look at the kernels of the prefix-per-query mode (cerebro_amd/csrc/batch.hip: db_gemm_prefixed, gather_query_tiles) in the
gfx950 code object of the built libcerebro_hip.so (no GPU needed).  db_gemm_prefixed includes the body of db_gemm_topk
(db_gemm_body.inc): the MFMA loop is the same, so each form has its twin's count of matrix instructions; nothing goes through scratch,
and the wide forms fit the 256 registers a wave of an 8-wave workgroup per CU can have.  "Spill count" is what the cast test counts:
.vgpr_spill_count and the private segment (registers that went to memory); SGPRs parked in VGPR lanes are moves, not memory."""
import re
import subprocess

import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings, code_objects

pytestmark = pytest.mark.needs_hip_build

# db_gemm_prefixed<KC = 32, WN, KL, ROW> and db_gemm_topk<...>
PREFIXED = re.compile(r"db_gemm_prefixedILi32ELi(\d+)ELi(\d+)E([fd])EE")
TOPK = re.compile(r"db_gemm_topkILi32ELi(\d+)ELi(\d+)E([fd])EE")
# what the host can launch: float and double rows, both tiles, both list capacities, minus the wide double form with 16 entries
FORMS = {(2, 8, "f"), (2, 16, "f"), (4, 8, "f"), (4, 16, "f"), (2, 8, "d"), (2, 16, "d"), (4, 8, "d")}


def _ops(tmp_path, needle, pattern):
    out = {}
    for k, ins in _kernel_listings(tmp_path, lambda k: needle in k and not k.endswith(".kd")).items():
        m = pattern.search(k)
        assert m, k
        out[(int(m.group(1)), int(m.group(2)), m.group(3))] = [t.split(None, 1)[0] for t in ins if t]
    return out


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_prefix_forms_of_the_gemm(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    forms, twins = _ops(tmp_path, "db_gemm_prefixed", PREFIXED), _ops(tmp_path, "db_gemm_topk", TOPK)
    assert set(forms) == FORMS, sorted(forms)
    for key, ops in forms.items():
        count = lambda prefix, ops=ops: sum(o.startswith(prefix) for o in ops)      # noqa: E731
        assert count("scratch_") == 0, (key, "spills")
        assert count("flat_") == 0, (key, "flat_ memory instructions")
        assert count("v_mfma_f32_32x32x2") == sum(o.startswith("v_mfma_f32_32x32x2") for o in twins[key]) > 0, key


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_gather_kernel_forms(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    listings = _kernel_listings(tmp_path, lambda k: "gather_query_tiles" in k and not k.endswith(".kd"))
    seen = set()
    for k, ins in listings.items():
        m = re.search(r"gather_query_tilesI([fd])Li(\d+)EE", k)
        assert m, k
        seen.add((m.group(1), int(m.group(2))))
        ops = [t.split(None, 1)[0] for t in ins if t]
        assert not any(o.startswith("scratch_") or o.startswith("flat_") for o in ops), k
        assert any(o.startswith("v_cvt_f32_f64") for o in ops) == (m.group(1) == "d"), k   # the cast loader's own conversion
    assert seen == {("f", 128), ("f", 256), ("d", 128), ("d", 256)}, seen


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_prefix_forms_do_not_spill_and_the_wide_ones_fit(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    seen = set()
    for co in code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            m = PREFIXED.search(name) or re.search(r"gather_query_tilesI([fd])Li(\d+)EE", name)
            if not m or name.endswith(".kd"):
                continue
            get = lambda key, block=block: int(re.search(key + r":\s+(\d+)", block).group(1))   # noqa: E731
            assert get(r"\.vgpr_spill_count") == 0 and get(r"\.private_segment_fixed_size") == 0, name
            if PREFIXED.search(name):
                seen.add(name)
                if m.group(1) == "4":
                    assert get(r"\.vgpr_count") <= 256, (name, get(r"\.vgpr_count"))   # unified file: AGPRs included, 2 waves per SIMD
    assert len(seen) == len(FORMS)
