"""Build-time look at the shared-pass kernels of the descriptor projection (cerebro_amd/csrc/project.hip project_pass) in the gfx950
code object of the built libcerebro_hip.so, from its resource metadata (no GPU needed): every instantiation is free of private memory
and spills, has no static LDS (the launch sizes it, as chip_project_plan says) and fits its 1024-thread workgroup."""
import re

import pytest

from cerebro_amd import capi
from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO

pytestmark = pytest.mark.needs_hip_build


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    return metadata(tmp_path_factory.mktemp("co"), lambda n: not n.endswith(".kd"))


def test_shared_pass_kernels_have_no_scratch_no_static_lds_and_fit_their_block(kernels):
    passes = {k: m for k, m in kernels.items() if "project_pass" in k}
    found = sorted(re.search(r"project_passI([fd])Li(\d+)E", k).groups() for k in passes)
    width = capi.project_plan(256, capi.CHIP_PROJ_F32, 0)["width"]
    # a float and a double matrix at every width the library holds; the planned width is among them
    assert found and sorted(set(t for t, _ in found)) == ["d", "f"], found
    assert [w for t, w in found if t == "f"] == [w for t, w in found if t == "d"], found
    assert str(width) in [w for _, w in found], (width, found)
    for name, m in passes.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)                     # x's slabs are ALL of the kernel's LDS, sized by the launch
        assert m["max_flat_workgroup_size"] == 1024 and m["vgpr_count"] <= 128, (name, m)   # 16 waves per CU: 512 / 4 registers a lane
    # the other kernels of the file keep their names and their count: a group of one is still project_rows, one project_finish ends a group
    assert len([k for k in kernels if "project_rows" in k]) == 2 and len([k for k in kernels if "project_finish" in k]) == 1
