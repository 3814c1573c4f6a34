"""Build-time look at the match stage (cerebro_amd/csrc/match.hip: hamming_match_split, gms_batch, pose_sets_batch, and gms_filter of
chip_gms_filter) in the gfx950 code object of the built libcerebro_hip.so (no GPU needed): the three kernels of the pipeline exist, none
of them spills or uses a flat_ memory instruction (the per-candidate pointers come out of the kernel arguments as global pointers), the
matcher's loop is LDS broadcast reads of 16 bytes, xor + popcount, and the kernels of the former pair-only path are gone."""
import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("hamming_match_split", "gms_batch", "pose_sets_batch")
DELETED = ("orb_bf_match", "pose_sets_build")


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("llvm-objdump not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    ks = _kernel_listings(tmp_path_factory.mktemp("co"), lambda k: any(n in k for n in KERNELS + DELETED + ("gms_filter",)))
    return {k: [t.split(None, 1)[0] for t in v if t] for k, v in ks.items() if not k.endswith(".kd")}


@pytest.mark.parametrize("name", KERNELS)
def test_batch_kernel_is_in_the_product_library_without_spill_or_flat(listings, name):
    mine = {k: v for k, v in listings.items() if name in k}
    assert len(mine) == 1, sorted(listings)
    (ops,) = mine.values()
    assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
    assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"


def test_matcher_loop_and_merge(listings):
    (ops,) = [v for k, v in listings.items() if "hamming_match_split" in k]
    assert sum(o.startswith("ds_read_b128") for o in ops) >= 2       # the tile is read 16 bytes at a time
    assert sum(o.startswith("v_bcnt_u32_b32") for o in ops) >= 8     # 8 popcounts per descriptor pair
    assert any(o.startswith("global_load_dwordx4") for o in ops)     # descriptors come in 16 bytes per lane
    assert sum(o.startswith("global_atomic_umin_x2") for o in ops) == 1   # the tile merge is ONE native 64-bit minimum, no compare-and-swap loop
    assert not [o for o in ops if "cmpswap" in o]


def test_gms_filter_is_in_the_product_library(listings):
    assert len([k for k in listings if "gms_filter" in k]) == 1, sorted(listings)


def test_no_pair_only_kernel_is_left(listings):
    assert [k for k in listings if "hamming_match_split" in k]       # the listing does see match.hip's kernels ...
    assert not [k for k in listings if any(n in k for n in DELETED)], sorted(listings)   # ... and none of the deleted ones
