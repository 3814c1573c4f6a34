"""Build-time look at the kernels of the descriptor projection (cerebro_amd/csrc/project.hip) in the gfx950 code object of the built
libcerebro_hip.so, from its resource metadata (no GPU needed): project_rows (both matrix types) and project_finish use no private
memory, project_rows has the LDS it was planned with -- and the kernels the library had before have the registers and the LDS recorded
in profiles/project.md, which are those of the commit before the projection."""
import re
from pathlib import Path

import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    return metadata(tmp_path_factory.mktemp("co"), lambda n: not n.endswith(".kd"))


def test_projection_kernels_have_no_scratch_and_the_planned_lds(kernels):
    rows = {k: m for k, m in kernels.items() if "project_rows" in k}
    finish = {k: m for k, m in kernels.items() if "project_finish" in k}
    assert len(finish) == 1, sorted(finish)
    assert sorted(re.search(r"project_rowsI([fd])E", k).group(1) for k in rows) == ["d", "f"]      # a float and a double matrix
    for name, m in {**rows, **finish}.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    for name, m in rows.items():
        # x is ALL of the kernel's LDS and is sized by the launch (in_dim * 4 bytes, up to 128 KiB): nothing static may be added to it,
        # or the 32768 case stops being launchable beside it; 1024 threads need at most 128 VGPRs
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128 and m["max_flat_workgroup_size"] == 1024, (name, m)
    (m,) = finish.values()
    assert m["group_segment_fixed_size"] == 8                                   # the one double that carries s to every wave


def test_the_earlier_kernels_keep_their_registers_and_lds(kernels):
    text = (ROOT / "profiles" / "project.md").read_text()
    table = re.findall(r"^\| `(\S+)` \| (\d+) \| (\d+) \| (\d+) \|$", text, flags=re.M)
    assert len(table) >= 150, len(table)
    # the table is the record of THIS change (the library of the commit before it): a kernel that a later change adds is not in it and
    # is not looked at, one that a later change removes or renames is skipped
    present = [row for row in table if row[0] in kernels]
    assert len(present) >= 100, len(present)
    for name, vgpr, sgpr, lds in present:
        m = kernels[name]
        assert (m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]) == (int(vgpr), int(sgpr), int(lds)), (name, m)
