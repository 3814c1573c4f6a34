"""chip_project_plan without a GPU: what a projecting call over n descriptors launches -- the group width, the reads of the matrix
(shared passes and single launches), the slab of x a shared pass keeps in the LDS and what that costs -- over the shapes and counts at
which the walk over the groups takes another turn."""
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
KINDS = {"f32": (capi.CHIP_PROJ_F32, 4), "f64": (capi.CHIP_PROJ_F64, 8)}
LDS_LIMIT = 163840


def width():
    return capi.project_plan(256, capi.CHIP_PROJ_F32, 0)["width"]


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("in_dim", [256, 768, 2048, 2304, 32768])
def test_plan_over_the_group_boundaries(in_dim, kind):
    matrix_type, elem = KINDS[kind]
    w = width()
    assert w >= 2
    for n in (0, 1, 2, w - 1, w, w + 1, 2 * w + 3):
        f = capi.project_plan(in_dim, matrix_type, n)
        assert f["width"] == w
        assert f["passes"] == -(-n // w) == f["shared_passes"] + f["single_launches"], (n, f)
        if n <= 1:
            assert f["shared_passes"] == 0 and f["single_launches"] == n, (n, f)       # n <= 1 plans no shared pass
        else:
            assert f["single_launches"] == (1 if n % w == 1 else 0), (n, f)            # a trailing group of one is a single launch
        assert 0 < f["lds_bytes"] <= LDS_LIMIT and f["lds_bytes"] == 2 * w * f["slab"] * 4, f   # two slabs of every descriptor, float32
        assert f["single_lds_bytes"] == in_dim * 4 <= LDS_LIMIT
        assert f["slab"] > 0 and (f["slab"] * elem) % 1024 == 0, f                     # a whole number of 1-KiB chunks of a matrix row
        assert f["block"] == 1024


def test_large_counts_do_not_wrap():
    w = width()
    n = (1 << 40) + 1
    f = capi.project_plan(32768, capi.CHIP_PROJ_F64, n)
    assert f["passes"] == -(-n // w) and f["shared_passes"] + f["single_launches"] == f["passes"]
