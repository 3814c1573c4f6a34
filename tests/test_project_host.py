"""The host mirror's raw-descriptor path (Cerebro::set_descriptor_projection / raw_descriptor_available), compiled and run: a value
that is no float32 is refused before anything is touched and nothing is registered; without a device every call fails with a status,
not a crash.  (On a machine with a device the same program finds a ctx without a projection: CHIP_ERR_BUSY.)"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.needs_hip_build

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "cerebro_host.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (status %d)\n", __LINE__, #c, cer.last_status()); return 1; } } while (0)
int main()
{
    cerebro_hip::Cerebro cer(4);
    cerebro_hip::Time t; t.sec = 5; t.nsec = 6;
    std::vector<double> raw(256, 0.5);
    const int no_ctx = cer.ok() ? CHIP_ERR_BUSY : CHIP_ERR_NO_DEVICE;      // with a ctx: no projection is set
    CHECK(cer.projection_in_dim() == 0);
    raw[100] = 0.1;                                                          // not a float32
    CHECK(!cer.raw_descriptor_available(t, raw.data(), 256) && cer.last_status() == CHIP_ERR_NOT_F32);
    raw[100] = std::nan("");
    CHECK(!cer.raw_descriptor_available(t, raw.data(), 256) && cer.last_status() == CHIP_ERR_NOT_F32);
    raw[100] = 1e300;                                                        // overflows to inf
    CHECK(!cer.raw_descriptor_available(t, raw.data(), 256) && cer.last_status() == CHIP_ERR_NOT_F32);
    raw[100] = (double)0.1f;
    CHECK(!cer.raw_descriptor_available(t, raw.data(), 256) && cer.last_status() == no_ctx);
    CHECK(!cer.raw_descriptor_available(t, nullptr, 256) && cer.last_status() == CHIP_ERR_INVALID_ARG);
    CHECK(!cer.raw_descriptor_available(t, raw.data(), 0) && cer.last_status() == CHIP_ERR_INVALID_ARG);
    CHECK(cer.wholeImageComputedList_size() == 0);                           // nothing was registered
    std::vector<float> Mt(4 * 256, 1.0f);
    if (!cer.ok()) CHECK(!cer.set_descriptor_projection(256, Mt.data(), CHIP_PROJ_F32, nullptr) && cer.last_status() == CHIP_ERR_NO_DEVICE);
    CHECK(!cer.set_descriptor_projection(100, Mt.data(), CHIP_PROJ_F32, nullptr) && cer.last_status() == (cer.ok() ? CHIP_ERR_UNSUPPORTED : CHIP_ERR_NO_DEVICE));
    CHECK(cer.projection_in_dim() == 0);
    std::puts("raw descriptor path ok");
    return 0;
}
"""


def test_raw_descriptor_path_of_the_host_mirror(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    lib = ROOT / "cerebro_amd" / "lib"
    assert (lib / "libcerebro_host.so").exists()
    syms = subprocess.run(["nm", "-DC", str(lib / "libcerebro_host.so")], capture_output=True, text=True).stdout
    for name in ("cerebro_hip::Cerebro::set_descriptor_projection", "cerebro_hip::Cerebro::raw_descriptor_available"):
        assert name in syms, name
    (tmp_path / "driver.cc").write_text(DRIVER)
    exe = tmp_path / "raw_descriptor_check"
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "cerebro_amd/host"), "-I", str(ROOT / "include"), str(tmp_path / "driver.cc"),
           "-o", str(exe), "-L", str(lib), "-lcerebro_host", "-lcerebro_hip", f"-Wl,-rpath,{lib}", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "raw descriptor path ok" in r.stdout, (r.stdout, r.stderr[-1500:])
