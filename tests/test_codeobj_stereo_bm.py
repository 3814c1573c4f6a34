"""Build-time look at the three kernels of the block matcher (cerebro_amd/csrc/frames.hip: bm_prefilter, bm_keypoints, bm_dense) in the
gfx950 code object of the built libcerebro_hip.so (no GPU needed): each exists once, none spills or uses a flat_ memory instruction,
the record of a keypoint leaves in ONE 16-byte store, the sums of absolute differences are byte-SAD instructions -- and frame_gather
and disparity_gather next to them have the registers they had before."""
import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("bm_prefilter", "bm_keypoints", "bm_dense")
# of the build before these kernels existed
GATHER_REGISTERS = dict(frame_gather=dict(vgpr_count=10, sgpr_count=20), disparity_gather=dict(vgpr_count=16, sgpr_count=24))
BYTE_SAD = ("v_sad_u8", "v_qsad_pk_u16_u8")


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


def test_keypoint_kernel_stores_one_record_and_sums_bytes_four_at_a_time(listings):
    (ops,) = [v for k, v in listings.items() if "bm_keypoints" in k]
    assert [o for o in ops if o.startswith("global_store")] == ["global_store_dwordx4"]      # the record leaves in one piece
    assert [o for o in ops if o.startswith(BYTE_SAD)], "no byte-SAD instruction"
    assert [o for o in ops if o.startswith("v_alignbyte_b32")], "the rows are not formed with v_alignbyte_b32"
    assert not [o for o in ops if o.startswith(("global_load_ubyte", "global_load_sbyte"))], "a window is read byte by byte"


def test_dense_kernel_runs_the_same_body(listings):
    (ops,) = [v for k, v in listings.items() if "bm_dense" in k]
    assert [o for o in ops if o.startswith("global_store")] == ["global_store_short"]        # one int16 per wave
    assert [o for o in ops if o.startswith(BYTE_SAD)]


def test_prefilter_stores_four_bytes_at_once_or_one(listings):
    (ops,) = [v for k, v in listings.items() if "bm_prefilter" in k]
    stores = {o for o in ops if o.startswith("global_store")}
    assert stores == {"global_store_dword", "global_store_byte"}, stores


def test_no_private_memory_and_the_gather_kernels_keep_their_registers(tmp_path):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    mine = metadata(tmp_path, lambda n: any(k in n for k in KERNELS) and not n.endswith(".kd"))
    assert len(mine) == 3, sorted(mine)
    for name, m in mine.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)                       # eight waves per SIMD
    for kernel, want in GATHER_REGISTERS.items():
        md = metadata(tmp_path, lambda n: kernel in n and not n.endswith(".kd"))
        assert len(md) == 1, sorted(md)
        (m,) = md.values()
        assert {k: m[k] for k in want} == want, (kernel, m)
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
