"""Build-time look at the five-tick pass (cerebro_amd/csrc/kernels.hip, db_scan_halfq) in the gfx950 code object of the built
libcerebro_hip.so (no GPU needed): two waves per SIMD (at most 256 registers per lane), nothing spilled, no scratch (a scratch access
drains the load stream), all LDS dynamic, 512 threads per workgroup.  Register and LDS facts only."""
import pytest

from test_codeobj_prefilter import LLVM, SO, _metadata

pytestmark = pytest.mark.needs_hip_build


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_halfq_fits_two_waves_per_simd_without_scratch(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    md = _metadata(tmp_path, "db_scan_halfq")
    assert len(md) == 1, sorted(md)
    for name, m in md.items():
        assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 256, (name, m)
        assert int(m["private_segment_fixed_size"]) == 0, (name, m)
        assert int(m.get("vgpr_spill_count", 0)) == 0 and int(m.get("sgpr_spill_count", 0)) == 0, (name, m)
        assert int(m["group_segment_fixed_size"]) == 0, name
        assert int(m["max_flat_workgroup_size"]) == 512, name
