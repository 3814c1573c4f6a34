"""examples/bulk_ticks.cc (built by `make`): one chip_loop_ticks_bulk over a whole schedule against the loop of chip_loop_tick and
chip_query_rows, every field compared by the program itself."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_bulk_ticks_example_prints_all_equal():
    exe = ROOT / "cerebro_amd" / "lib" / "bulk_ticks"
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout, r.stdout
    m = re.search(r"\((\d+) scanned, (\d+) loops found\).*certified (\d+), uncertified (\d+) \(run again exactly: (\d+)\)", r.stdout)
    assert m, r.stdout
    scanned, found, cert, unc, rerun = (int(x) for x in m.groups())
    assert scanned > 900 and 0 < found < scanned and cert + unc == scanned and rerun == unc


def test_replay_bulk_writes_the_file_of_the_plain_replay(tmp_path):
    """cerebro_replay --bulk --state: the cold start's ticks in one chip_loop_ticks_bulk, through Cerebro::descrip_N__dot__descrip_0_N_bulk,
    against the loop of ticks on the small state.json of tests/test_host_replay.py: byte-identical dumps, with candidates in them"""
    import scenarios
    from test_host_replay import LIB, write_state_json
    D, N = 1024, 700
    plants, loops, ties = scenarios.loop_plants(N, 4, seed=8)
    db = scenarios.build_db(19, N, D, plants)
    write_state_json(tmp_path / "state.json", db, [1403636579_000000000 + i * 50_000_000 for i in range(N)])
    outs = []
    for opt in ([], ["--bulk"]):
        out = tmp_path / ("bulk.json" if opt else "plain.json")
        r = subprocess.run(["timeout", "-k", "10", "120", str(LIB / "cerebro_replay")] + opt + ["--state", str(tmp_path / "state.json"), str(out)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and outs[0].count(b"global_a") >= len(loops) >= 1
