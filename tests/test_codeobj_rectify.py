"""Build-time look at the kernel of the rectification (cerebro_amd/csrc/frames.hip: rectify_pair) in the gfx950 code object of the built
libcerebro_hip.so (no GPU needed): it exists once, does not spill or use a flat_ memory instruction, stores four pixels as one dword
(bytes only for tails and odd alignments) -- and the ORB and block-matcher kernels have the registers they had without it."""
import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("rectify_pair",)
# recorded on the commit before the rectification was added
BEFORE = dict(orb_pyramid=dict(vgpr_count=34, sgpr_count=33), orb_fast_score=dict(vgpr_count=60, sgpr_count=32),
              orb_candidates=dict(vgpr_count=52, sgpr_count=50), orb_select=dict(vgpr_count=56, sgpr_count=100),
              orb_moments=dict(vgpr_count=13, sgpr_count=32), orb_blur=dict(vgpr_count=55, sgpr_count=35),
              orb_describe=dict(vgpr_count=25, sgpr_count=24), bm_prefilter=dict(vgpr_count=27, sgpr_count=28),
              bm_keypoints=dict(vgpr_count=21, sgpr_count=66), bm_dense=dict(vgpr_count=16, sgpr_count=67))


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


def test_four_pixels_leave_in_one_dword_and_map_entries_arrive_in_one_load(listings):
    (ops,) = [v for k, v in listings.items() if "rectify_pair" in k]
    stores = [o for o in ops if o.startswith("global_store")]
    assert "global_store_dword" in stores and set(stores) <= {"global_store_dword", "global_store_byte"}, stores
    loads = {o for o in ops if o.startswith("global_load")}
    assert loads == {"global_load_dwordx2", "global_load_ubyte"}, loads      # an entry (qx, qy) in one load; the raw taps are bytes


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
