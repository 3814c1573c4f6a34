"""Build-time look at the ten batch entries of the frame put (cerebro_amd/csrc/orb.hip, frames.hip: fb_*) in the gfx950 code object of
the built libcerebro_hip.so (no GPU needed): each exists once next to its single form, none uses private memory, spills or a flat_
memory instruction, none has more LDS than its single form, the stores keep the single forms' shapes -- and the registers of both are
the ones profiles/frame_put_batch.md records."""
import re
from pathlib import Path

import pytest

from test_codeobj_disparity import metadata
from test_codeobj_registers import LLVM, SO, _kernel_listings

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
# batch entry -> its single form
PAIRS = dict(fb_rectify="rectify_pair", fb_pyramid="orb_pyramid", fb_fast_score="orb_fast_score", fb_candidates="orb_candidates",
             fb_select="orb_select", fb_moments="orb_moments", fb_blur="orb_blur", fb_describe="orb_describe", fb_prefilter="bm_prefilter",
             fb_keypoints="bm_keypoints")


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("llvm-objdump not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    names = tuple(PAIRS) + tuple(PAIRS.values())
    ks = _kernel_listings(tmp_path_factory.mktemp("co"), lambda k: any(n in k for n in names))
    return {k: [t.split(None, 1)[0] for t in v if t] for k, v in ks.items() if not k.endswith(".kd")}


@pytest.fixture(scope="module")
def registers(tmp_path_factory):
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm-readelf not available")
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    names = tuple(PAIRS) + tuple(PAIRS.values())
    md = metadata(tmp_path_factory.mktemp("md"), lambda n: any(k in n for k in names) and not n.endswith(".kd"))
    out = {}
    for name in names:
        mine = [m for k, m in md.items() if name in k]
        assert len(mine) == 1, (name, sorted(md))
        out[name] = mine[0]
    return out


def ops_of(listings, name):
    mine = [v for k, v in listings.items() if name in k]
    assert len(mine) == 1, (name, sorted(listings))
    return mine[0]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_batch_entry_is_in_the_product_library_once_without_spill_or_flat(listings, name):
    ops = ops_of(listings, name)
    assert not [o for o in ops if o.startswith("scratch_")], f"{name} spills"
    assert not [o for o in ops if o.startswith("flat_")], f"{name} uses flat_ memory instructions"


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_no_private_memory_no_more_lds_than_the_single_form_and_eight_waves(registers, name):
    m, single = registers[name], registers[PAIRS[name]]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert single["private_segment_fixed_size"] == 0, single
    assert m["group_segment_fixed_size"] == single["group_segment_fixed_size"], (m, single)   # the one body's LDS, nothing for the frame axis
    assert m["vgpr_count"] <= 64, m                                                             # eight waves per SIMD, as the single forms
    assert m["max_flat_workgroup_size"] == single["max_flat_workgroup_size"]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_the_frame_axis_leaves_the_memory_instructions_of_the_body_alone(listings, name):
    """one body, two entries: the batch entry stores and loads global memory with the instructions the single form uses (the kept counts
    that fb_keypoints reads are scalar loads)"""
    mem = lambda ops: sorted({o for o in ops if o.startswith(("global_store", "global_load", "ds_"))})
    assert mem(ops_of(listings, name)) == mem(ops_of(listings, PAIRS[name])), name


def test_profile_records_the_registers_of_both_forms(registers):
    text = (ROOT / "profiles" / "frame_put_batch.md").read_text()
    for name, single in PAIRS.items():
        row = re.search(r"^\|\s*`" + name + r"`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*`" + single + r"`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", text, flags=re.M)
        assert row, f"profiles/frame_put_batch.md has no row for {name}"
        want = (registers[name]["vgpr_count"], registers[name]["sgpr_count"], registers[single]["vgpr_count"], registers[single]["sgpr_count"])
        assert tuple(int(v) for v in row.groups()) == want, (name, row.groups(), want)
