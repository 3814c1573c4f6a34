"""Build-time guard for the ICP kernels (cerebro_amd/csrc/icp.hip).  icp_models_batch / icp_score_batch are icp_models / icp_score with a
problem dimension (blockIdx.y and a per-problem table in device memory); both pairs share their bodies.  Neither pair may need more VGPRs
or scratch than the parent commit's single-problem pair -- built from the parent's icp.hip with the Makefile's flags, recorded in
profiles/icp_batch.md.  Read from the built library's code-object metadata (no GPU needed)."""
import re
import subprocess
from pathlib import Path

import pytest

from test_codeobj_registers import LLVM, SO, code_objects

pytestmark = pytest.mark.needs_hip_build
ROOT = Path(__file__).resolve().parent.parent
# the single-problem pair of the parent commit (profiles/icp_batch.md, "Code objects"): kernel -> (VGPRs, scratch bytes)
PARENT = {"icp_models": (92, 0), "icp_score": (32, 0)}


def kernel_metadata(tmp_path):
    out = {}
    for co in code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:          # one metadata entry per kernel (keys in alphabetical order)
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            get = lambda key: int(re.search(key + r":\s+(\d+)", block).group(1))   # noqa: E731
            out[name] = dict(vgpr=get(r"\.vgpr_count"), scratch=get(r"\.private_segment_fixed_size"), spill=get(r"\.vgpr_spill_count"),
                             kernarg=get(r"\.kernarg_segment_size"))
    return out


@pytest.mark.skipif(not (LLVM / "llvm-readelf").exists(), reason="llvm-readelf not available")
def test_both_icp_pairs_cost_no_more_registers_than_the_parents_pair(tmp_path):
    if not SO.exists():
        pytest.skip("libcerebro_hip.so not built")
    meta = kernel_metadata(tmp_path)
    for kernel, (vgpr, scratch) in PARENT.items():
        for name in (kernel, kernel + "_batch"):
            mine = [m for full, m in meta.items() if re.search(r"\d+" + name + r"E", full)]
            assert len(mine) == 1, (name, sorted(meta))
            m = mine[0]
            print(name, m)
            assert m["vgpr"] <= vgpr, (name, m)
            assert m["scratch"] <= scratch and m["spill"] == 0, (name, m)
            if name.endswith("_batch"):
                # the per-problem values live in a table, not in the argument block: sixteen problems' worth would be > 2 KiB
                assert m["kernarg"] <= 128, (name, m)


def test_the_profile_records_the_figures_the_test_holds_the_kernels_to():
    text = (ROOT / "profiles" / "icp_batch.md").read_text()
    for kernel, (vgpr, scratch) in PARENT.items():
        assert re.search(r"\|\s*`" + kernel + r"`\s*\|\s*" + str(vgpr) + r"\s*\|\s*" + str(scratch) + r"\s*\|", text), kernel
