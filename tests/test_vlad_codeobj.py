"""Build-time look at the kernels of the NetVLAD pooling (cerebro_amd/csrc/vlad.hip) in the gfx950 code object of the built
libcerebro_hip.so, from its resource metadata (no GPU needed): none of the vlad_* kernels uses private memory or spills, and each has the
LDS it was planned with."""
import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO

pytestmark = pytest.mark.needs_hip_build

# bytes of static LDS: the 32 x 33 float tile of the transposing stage-in; nothing (the weights are read in place out of the L2, so the
# launch is placed wherever four wave slots are free); the assignments of one block's 64 positions to eight clusters; one cluster's row as
# doubles (C <= 1024) and q_k; the one double q
PLANNED_LDS = {"vlad_transpose": 32 * 33 * 4, "vlad_assign": 0, "vlad_aggregate": 64 * 8 * 8, "vlad_reduce": 1024 * 8 + 8, "vlad_finish": 8}
BLOCK = {"vlad_transpose": 256, "vlad_assign": 256, "vlad_aggregate": 64, "vlad_reduce": 256, "vlad_finish": 1024}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    return metadata(tmp_path_factory.mktemp("co"), lambda n: not n.endswith(".kd"))


def test_pooling_kernels_have_no_scratch_and_the_planned_lds(kernels):
    found = {}
    for name, m in kernels.items():
        for short in PLANNED_LDS:
            if "4chip" in name and short in name:
                assert short not in found, (short, name)
                found[short] = m
    assert sorted(found) == sorted(PLANNED_LDS), sorted(found)
    for short, m in found.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (short, m)
        assert m["group_segment_fixed_size"] == PLANNED_LDS[short], (short, m)
        assert m["max_flat_workgroup_size"] == BLOCK[short], (short, m)
        assert m["vgpr_count"] <= 128, (short, m)                     # every one of them at eight waves per SIMD or close to it
