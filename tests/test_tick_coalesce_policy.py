"""The parking policy of pipelined ticks that share a DB pass, without a device (chip_debug_coalesce_decide is the function the
library's enqueue path calls: cerebro_amd/csrc/chip_api.hip coalesce_decide).  0 = launch now, alone; 1 = park; 2 = park and
release everything parked as one pass."""
import pytest

from cerebro_amd import capi

pytestmark = pytest.mark.needs_hip_build
LAUNCH, PARK, PARK_FLUSH = 0, 1, 2


def passes_of(decide, n_ticks, t_max, running_after_first=True):
    """Ticks 0 .. n-1 enqueued back to back behind a scan that keeps running; the caller's collects release the rest."""
    passes, parked, running = [], [], False
    for i in range(n_ticks):
        act = decide(len(parked), t_max, 1 if running else 0)
        if act == LAUNCH:
            assert not parked
            passes.append([i])
        else:
            parked.append(i)
            if act == PARK_FLUSH:
                passes.append(parked)
                parked = []
        running = running_after_first
    if parked:
        passes.append(parked)      # chip_loop_tick_collect of a parked slot
    return passes


def test_policy_table(chip_lib):
    d = chip_lib.chip_debug_coalesce_decide
    for t_max in (0, 1):
        assert [d(n, t_max, r) for n in range(3) for r in (0, 1)] == [LAUNCH] * 6       # coalescing off
    for t_max in (2, 3):
        assert d(0, t_max, 0) == LAUNCH                       # nothing running, nothing parked: at once, alone
        assert d(1, t_max, 0) == PARK_FLUSH                   # the scan they waited behind has ended: leave together now
        assert d(t_max - 1, t_max, 1) == PARK_FLUSH           # the T_max-th tick sends all of them off
    assert d(0, 2, 1) == PARK and d(0, 3, 1) == PARK and d(1, 3, 1) == PARK and d(1, 2, 1) == PARK_FLUSH


@pytest.mark.parametrize("t_max", [2, 3])
def test_sixteen_ticks_ahead_leave_in_full_passes(chip_lib, t_max):
    passes = passes_of(chip_lib.chip_debug_coalesce_decide, 16, t_max)
    assert passes[0] == [0]                                   # the first tick finds the GPU idle
    assert [t for p in passes for t in p] == list(range(16))  # every tick leaves once, in order
    assert all(len(p) == t_max for p in passes[1:-1]) and 1 <= len(passes[-1]) <= t_max
    assert len(passes) == 1 + -(-15 // t_max)


def test_a_caller_that_never_outruns_the_gpu_never_parks(chip_lib):
    assert passes_of(chip_lib.chip_debug_coalesce_decide, 8, 3, running_after_first=False) == [[i] for i in range(8)]
