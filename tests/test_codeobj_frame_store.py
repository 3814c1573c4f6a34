"""Build-time look at the frame store's two kernels (frame_gather in cerebro_amd/csrc/frames.hip, pose_sets_stored_batch in match.hip) in the gfx950
code object of the built libcerebro_hip.so (no GPU needed): both exist, neither spills nor uses a flat_ memory instruction (every
pointer comes out of the kernel arguments as a global pointer), the gather loads a keypoint's 8 bytes and the 12 bytes of its pixel and makes ONE 16-byte store per
keypoint, and the stored set kernel reads its points as 16-byte records."""
import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("frame_gather", "pose_sets_stored_batch")


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("llvm-objdump not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    ks = _kernel_listings(tmp_path_factory.mktemp("co"), lambda k: any(n in k for n in KERNELS))
    return {k: [t.split(None, 1)[0] for t in v if t] for k, v in ks.items() if not k.endswith(".kd")}


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_is_in_the_product_library_without_spill_or_flat(listings, name):
    mine = {k: v for k, v in listings.items() if name in k}
    assert len(mine) == 1, sorted(listings)
    (ops,) = mine.values()
    assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
    assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"


def test_gather_loads_three_floats_and_stores_one_record(listings):
    (ops,) = [v for k, v in listings.items() if "frame_gather" in k]
    stores = [o for o in ops if o.startswith("global_store")]
    assert stores == ["global_store_dwordx4"], stores                # the record leaves in one piece
    loads = [o for o in ops if o.startswith("global_load")]
    words = {"global_load_dword": 1, "global_load_dwordx2": 2, "global_load_dwordx3": 3}
    assert sum(words[o] for o in loads) == 5, loads                  # the keypoint (8 bytes) and x, y, z of its pixel (12), however the compiler groups them


def test_stored_sets_read_records(listings):
    (ops,) = [v for k, v in listings.items() if "pose_sets_stored_batch" in k]
    assert sum(o.startswith("global_load_dwordx4") for o in ops) >= 2   # the record of a's keypoint and of b's
