"""Build-time look at the two kernels of GMS with scale / rotation (cerebro_amd/csrc/match.hip: gms_grid_modes, gms_mode_select) in the
gfx950 code object of the built libcerebro_hip.so (no GPU needed): each exists once, neither spills nor uses a flat_ memory
instruction, and the kernels of the plain filter (gms_batch, gms_filter) are still exactly one each."""
import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
NEW = ("gms_grid_modes", "gms_mode_select")
KEPT = ("gms_batch", "gms_filter")


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("llvm-objdump not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    ks = _kernel_listings(tmp_path_factory.mktemp("co"), lambda k: "gms_" in k)
    return {k: [t.split(None, 1)[0] for t in v if t] for k, v in ks.items() if not k.endswith(".kd")}


@pytest.mark.parametrize("name", NEW)
def test_mode_kernel_exists_once_without_spill_or_flat(listings, name):
    mine = {k: v for k, v in listings.items() if name in k}
    assert len(mine) == 1, sorted(listings)
    (ops,) = mine.values()
    assert len(ops) > 50
    assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
    assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"


@pytest.mark.parametrize("name", KEPT)
def test_plain_kernels_are_still_one_each(listings, name):
    assert len([k for k in listings if name in k]) == 1, sorted(listings)


def test_no_other_gms_kernel(listings):
    assert len(listings) == len(NEW) + len(KEPT), sorted(listings)
