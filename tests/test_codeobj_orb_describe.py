"""Build-time look at the two kernels of the ORB descriptor (cerebro_amd/csrc/orb.hip: orb_blur, orb_describe) in the gfx950 code object
of the built libcerebro_hip.so (no GPU needed): each exists once, neither spills or uses a flat_ memory instruction, a descriptor
leaves in one pair of 16-byte stores, the blurred plane is written in 16-byte stores from an LDS tile read wide -- and the kernels that
were there before (the detector's five, bm_keypoints, frame_gather) have the registers they had without the descriptor."""
import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("orb_blur", "orb_describe")
# recorded on the commit before the descriptor was added
BEFORE = dict(orb_pyramid=dict(vgpr_count=34, sgpr_count=33), orb_fast_score=dict(vgpr_count=60, sgpr_count=32),
              orb_candidates=dict(vgpr_count=52, sgpr_count=50), orb_select=dict(vgpr_count=56, sgpr_count=100),
              orb_moments=dict(vgpr_count=13, sgpr_count=32), bm_keypoints=dict(vgpr_count=21, sgpr_count=66),
              frame_gather=dict(vgpr_count=10, sgpr_count=20))


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("llvm-objdump not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    ks = _kernel_listings(tmp_path_factory.mktemp("co"), lambda k: any(n in k for n in KERNELS))
    return {k: [t.split(None, 1)[0] for t in v if t] for k, v in ks.items() if not k.endswith(".kd")}


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_is_in_the_product_library_once_without_spill_or_flat(listings, name):
    mine = {k: v for k, v in listings.items() if name in k}
    assert len(mine) == 1, sorted(listings)
    (ops,) = mine.values()
    assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
    assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"


def test_a_descriptor_leaves_in_one_pair_of_16_byte_stores(listings):
    (ops,) = [v for k, v in listings.items() if "orb_describe" in k]
    stores = [o for o in ops if o.startswith("global_store")]
    assert [o for o in stores if o == "global_store_dwordx4"] == ["global_store_dwordx4"] * 2, stores
    assert sorted(set(stores) - {"global_store_dwordx4"}) in ([], ["global_store_dwordx2"]), stores   # the keypoint of a store slot
    assert len([o for o in ops if o.startswith("global_load_ubyte")]) == 8, "eight byte gathers per lane"
    assert "global_load_dwordx4" in ops, "the lane's four pairs come in one 16-byte load"


def test_blurred_plane_is_written_in_16_byte_stores_from_a_tile_read_wide(listings):
    (ops,) = [v for k, v in listings.items() if "orb_blur" in k]
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx4"}
    assert not [o for o in ops if o.startswith(("global_load_ubyte", "global_load_sbyte"))], "the tile is staged byte by byte"
    assert [o for o in ops if o.startswith("ds_read_b128") or o.startswith("ds_read2_b64")], "the horizontal sums are not read wide"


def test_no_private_memory_and_the_earlier_kernels_keep_their_registers(tmp_path):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    mine = metadata(tmp_path, lambda n: any(k in n for k in KERNELS) and not n.endswith(".kd"))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, m in mine.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)                       # eight waves per SIMD
    for kernel, want in BEFORE.items():
        md = metadata(tmp_path, lambda n: kernel in n and not n.endswith(".kd"))
        assert len(md) == 1, sorted(md)
        (m,) = md.values()
        assert {k: m[k] for k in want} == want, (kernel, m)
