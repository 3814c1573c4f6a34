"""Build-time look at the five kernels of the pair-list run (cerebro_amd/csrc/match.hip: hamming_match_pairs, pairs_gms,
pose_sets_stored_pairs, pairs_grid_modes, pairs_mode_select) in the gfx950 code object of the built libcerebro_hip.so (no GPU
needed): each exists once, none spills or uses a flat_ memory instruction (every pointer comes out of the kernel arguments as a global
pointer, the per-pair tables included), and the pairs matcher merges its tiles with ONE 64-bit unsigned atomic minimum."""
import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("hamming_match_pairs", "pairs_gms", "pose_sets_stored_pairs", "pairs_grid_modes", "pairs_mode_select")


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


def test_pairs_matcher_merges_with_one_native_minimum(listings):
    (ops,) = [v for k, v in listings.items() if "hamming_match_pairs" in k]
    assert [o for o in ops if o.startswith("global_atomic")] == ["global_atomic_umin_x2"]
    assert sum(o == "s_barrier" for o in ops) == 1                   # the tile is staged once; both early exits come before it
