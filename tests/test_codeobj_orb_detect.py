"""Build-time look at the five kernels of the ORB detector (cerebro_amd/csrc/orb.hip) in the gfx950 code object of the built
libcerebro_hip.so (no GPU needed): each exists once, none spills or uses a flat_ memory instruction, a record leaves orb_moments in
one pair of 16-byte stores, the score plane is written in 16-byte stores -- and the kernels of frames.hip whose registers the other
code-object tests record have them still (they are in another translation unit and must not move)."""
import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO, _kernel_listings
from test_codeobj_stereo_bm import GATHER_REGISTERS

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("orb_pyramid", "orb_fast_score", "orb_candidates", "orb_select", "orb_moments")


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


def test_a_record_leaves_in_one_pair_of_16_byte_stores(listings):
    (ops,) = [v for k, v in listings.items() if "orb_moments" in k]
    assert [o for o in ops if o.startswith("global_store")] == ["global_store_dwordx4"] * 2
    assert not [o for o in ops if o.startswith(("global_load_ubyte", "global_load_sbyte"))], "the patch is read byte by byte"


def test_score_plane_and_lists_are_written_in_16_byte_stores(listings):
    for name in ("orb_fast_score", "orb_candidates"):
        (ops,) = [v for k, v in listings.items() if name in k]
        stores = [o for o in ops if o.startswith("global_store")]
        assert "global_store_dwordx4" in stores and set(stores) <= {"global_store_dwordx4", "global_store_dword"}, (name, stores)
    (ops,) = [v for k, v in listings.items() if "orb_fast_score" in k]
    assert not [o for o in ops if o.startswith(("global_load_ubyte", "global_load_sbyte"))], "the tile is staged byte by byte"
    assert [o for o in ops if o.startswith("ds_read_b64") or o.startswith("ds_read2_b64") or o.startswith("ds_read_b128")], "the tile rows are not read wide"


def test_no_private_memory_and_the_kernels_of_match_hip_keep_their_registers(tmp_path):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    mine = metadata(tmp_path, lambda n: any(k in n for k in KERNELS) and not n.endswith(".kd"))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, m in mine.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)                       # eight waves per SIMD
    for kernel, want in GATHER_REGISTERS.items():
        md = metadata(tmp_path, lambda n: kernel in n and not n.endswith(".kd"))
        assert len(md) == 1, sorted(md)
        (m,) = md.values()
        assert {k: m[k] for k in want} == want, (kernel, m)
