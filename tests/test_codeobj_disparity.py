"""Build-time look at the two kernels of the disparity -> 3-D step (cerebro_amd/csrc/frames.hip: disparity_gather, disparity_to_xyz)
in the gfx950 code object of the built libcerebro_hip.so (no GPU needed): both exist once, neither spills nor uses a flat_ memory
instruction, the record of a keypoint leaves in ONE 16-byte store, the dense kernel loads four pixels at once and stores 16 bytes at
a time, the fp64 sum is two additions (no fused multiply-add outside the divide's own sequence) -- and frame_gather next to them has
the registers it had before."""
import re
import subprocess

import pytest

from test_codeobj_registers import LLVM, SO, _kernel_listings, code_objects

pytestmark = pytest.mark.needs_hip_build
KERNELS = ("disparity_gather", "disparity_to_xyz")
FRAME_GATHER_REGISTERS = dict(vgpr_count=10, sgpr_count=20)          # of the build before these kernels existed


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("llvm-objdump not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    ks = _kernel_listings(tmp_path_factory.mktemp("co"), lambda k: any(n in k for n in KERNELS))
    return {k: [t.split(None, 1)[0] for t in v if t] for k, v in ks.items() if not k.endswith(".kd")}


def metadata(tmp_path, want) -> dict:
    """name -> dict of the integer fields of a kernel's metadata entry"""
    out = {}
    for co in code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:             # one metadata entry per kernel (keys in alphabetical order)
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            if want(name):
                out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return out


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_is_in_the_product_library_once_without_spill_or_flat(listings, name):
    mine = {k: v for k, v in listings.items() if name in k}
    assert len(mine) == 1, sorted(listings)
    (ops,) = mine.values()
    assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
    assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"


def test_gather_stores_one_record_and_loads_one_disparity(listings):
    (ops,) = [v for k, v in listings.items() if "disparity_gather" in k]
    assert [o for o in ops if o.startswith("global_store")] == ["global_store_dwordx4"]      # the record leaves in one piece
    loads = sorted(o for o in ops if o.startswith("global_load"))
    # the keypoint (8 bytes, in one or two loads) and ONE disparity value of either type
    assert loads in (["global_load_dword", "global_load_dwordx2", "global_load_sshort"],
                     ["global_load_dword", "global_load_dword", "global_load_dword", "global_load_sshort"]), loads


def test_dense_kernel_moves_16_bytes_at_a_time(listings):
    (ops,) = [v for k, v in listings.items() if "disparity_to_xyz" in k]
    assert sum(o == "global_store_dwordx4" for o in ops) == 3, ops      # the 48 contiguous bytes of four pixels
    assert "global_load_dwordx2" in ops and "global_load_dwordx4" in ops   # four int16 / four float disparities in one load


@pytest.mark.parametrize("name", KERNELS)
def test_the_sum_is_not_fused_and_the_divide_is_the_ieee_sequence(listings, name):
    (ops,) = [v for k, v in listings.items() if name in k]
    points = 1 if name == "disparity_gather" else 5                     # the dense kernel: four pixels at once and one in the tail loop
    count = lambda prefix: sum(o.startswith(prefix) for o in ops)      # noqa: E731
    assert count("v_div_fixup_f64") == points and count("v_div_fmas_f64") == points and count("v_rcp_f64") == points
    assert count("v_add_f64") == 2 * points                             # + Q33, + 1e-6: both round
    assert count("v_fma_f64") + count("v_fmac_f64") == 5 * points       # the divide's refinement steps and nothing else
    assert not count("v_fma_f32") and not count("v_fmac_f32") and not count("v_pk_fma_f32")   # x, y, z are plain products
    assert count("v_mul_f32") + 2 * count("v_pk_mul_f32") >= 3 * points


def test_frame_gather_is_unchanged_in_register_count(tmp_path):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    md = metadata(tmp_path, lambda n: "frame_gather" in n and not n.endswith(".kd"))
    assert len(md) == 1, sorted(md)
    (m,) = md.values()
    assert {k: m[k] for k in FRAME_GATHER_REGISTERS} == FRAME_GATHER_REGISTERS
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
    mine = metadata(tmp_path, lambda n: any(k in n for k in KERNELS) and not n.endswith(".kd"))
    assert len(mine) == 2 and all(v["vgpr_count"] <= 64 and v["private_segment_fixed_size"] == 0 for v in mine.values()), mine
