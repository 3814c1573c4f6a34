"""Build-time look at the brute-force ORB matcher (cerebro_amd/csrc/match.hip, orb_bf_match) in the gfx950 code object of the built
libcerebro_hip.so (no GPU needed): its loop is LDS broadcast reads + xor + popcount, so it must carry no scratch (spill) traffic and no
flat_ memory instruction (the train tile is read with ds_read, the descriptors with global_load)."""
import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_orb_bf_match_has_no_spill_and_no_flat_load(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    ks = {k: v for k, v in _kernel_listings(tmp_path, lambda k: "orb_bf_match" in k).items() if not k.endswith(".kd")}
    assert len(ks) == 1, sorted(ks)
    (ins,) = ks.values()
    ops = [t.split(None, 1)[0] for t in ins if t]
    assert not [o for o in ops if o.startswith("scratch_")], "orb_bf_match spills"
    assert not [o for o in ops if o.startswith("flat_")], "orb_bf_match uses flat_ memory instructions"
    assert sum(o.startswith("ds_read_b128") for o in ops) >= 2       # the tile is read 16 bytes at a time
    assert sum(o.startswith("v_bcnt_u32_b32") for o in ops) >= 8     # 8 popcounts per descriptor pair
    assert any(o.startswith("global_load_dwordx4") for o in ops)     # descriptors come in 16 bytes per lane


@pytest.mark.skipif(not (LLVM / "llvm-objdump").exists(), reason="llvm-objdump not available")
def test_match_kernels_are_in_the_product_library(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    for name in ("gms_filter", "pose_sets_build"):
        assert [k for k in _kernel_listings(tmp_path, lambda k: name in k) if not k.endswith(".kd")], name
