"""Build-time look at the prefilter pass (cerebro_amd/csrc/kernels.hip, db_scan_prefilter<0> / <3>) in the gfx950 code object of the built
libcerebro_hip.so (no GPU needed): two waves per SIMD (at most 256 registers per lane), nothing spilled, no scratch (a scratch access
drains the load stream), all LDS dynamic and within one CU's 160 KiB as scan_prefilter_plan sizes it.  Register and LDS facts only."""
import re
import subprocess

import pytest

from cerebro_amd import capi
from test_codeobj_registers import LLVM, SO, code_objects

pytestmark = pytest.mark.needs_hip_build


def _metadata(tmp_path, want):
    out = {}
    for co in code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("  - ."):
            d = dict(re.findall(r"\.(\w+):\s*(\S+)", "." + block))
            if want in d.get("name", ""):
                out[d["name"]] = d
    return out


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_prefilter_fits_two_waves_per_simd_without_scratch(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    md = _metadata(tmp_path, "db_scan_prefilter")
    assert len(md) == 2, sorted(md)                      # NG = 0 and NG = 3
    for name, m in md.items():
        assert int(m["vgpr_count"]) + int(m.get("agpr_count", 0)) <= 256, (name, m)
        assert int(m["private_segment_fixed_size"]) == 0, (name, m)
        assert int(m.get("vgpr_spill_count", 0)) == 0 and int(m.get("sgpr_spill_count", 0)) == 0, (name, m)
        assert int(m["group_segment_fixed_size"]) == 0, name          # all LDS is the launch's dynamic size ...
        assert int(m["max_flat_workgroup_size"]) == 512, name
    for d in (1024, 2048, 3072, 4096):                                # ... which the plan keeps within one CU
        assert capi.prefilter_plan(d)["lds_bytes"] <= 163840
    rs = _metadata(tmp_path, "tick_rescore")
    assert len(rs) == 1
    for name, m in rs.items():
        assert int(m["private_segment_fixed_size"]) == 0 and int(m["group_segment_fixed_size"]) <= 4096, (name, m)
