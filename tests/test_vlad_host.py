"""The host mirror's feature-map path (Cerebro::set_descriptor_pooling / feature_map_available), compiled and run: bad arguments are
refused before anything is touched and nothing is registered; without a device every call fails with a status, not a crash.  (On a
machine with a device the same program finds a ctx without weights: CHIP_ERR_BUSY, and shapes outside the limits CHIP_ERR_UNSUPPORTED.)"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.needs_hip_build

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "cerebro_host.h"
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (status %d)\n", __LINE__, #c, cer.last_status()); return 1; } } while (0)
int main()
{
    cerebro_hip::Cerebro cer(256);
    cerebro_hip::Time t; t.sec = 5; t.nsec = 6;
    std::vector<float> map(130 * 64, 0.5f), Wt(4 * 64, 0.1f), bias(4, 0.f), centres(4 * 64, 0.2f);
    const int no_ctx = cer.ok() ? CHIP_ERR_BUSY : CHIP_ERR_NO_DEVICE;      // with a ctx: no weights are set
    CHECK(cer.pooling_vector_dim() == 0);
    CHECK(!cer.feature_map_available(t, nullptr, 130, CHIP_VLAD_NHWC) && cer.last_status() == CHIP_ERR_INVALID_ARG);
    CHECK(!cer.feature_map_available(t, map.data(), 0, CHIP_VLAD_NHWC) && cer.last_status() == CHIP_ERR_INVALID_ARG);
    CHECK(!cer.feature_map_available(t, map.data(), 130, CHIP_VLAD_NHWC) && cer.last_status() == no_ctx);
    CHECK(cer.wholeImageComputedList_size() == 0);                           // nothing was registered
    if (!cer.ok()) CHECK(!cer.set_descriptor_pooling(64, 4, 0, Wt.data(), bias.data(), centres.data()) && cer.last_status() == CHIP_ERR_NO_DEVICE);
    CHECK(!cer.set_descriptor_pooling(66, 4, 0, Wt.data(), bias.data(), centres.data()) && cer.last_status() == (cer.ok() ? CHIP_ERR_UNSUPPORTED : CHIP_ERR_NO_DEVICE));
    CHECK(cer.pooling_vector_dim() == 0);
    std::puts("feature map path ok");
    return 0;
}
"""


def test_feature_map_path_of_the_host_mirror(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    lib = ROOT / "cerebro_amd" / "lib"
    assert (lib / "libcerebro_host.so").exists()
    syms = subprocess.run(["nm", "-DC", str(lib / "libcerebro_host.so")], capture_output=True, text=True).stdout
    for name in ("cerebro_hip::Cerebro::set_descriptor_pooling", "cerebro_hip::Cerebro::feature_map_available"):
        assert name in syms, name
    (tmp_path / "driver.cc").write_text(DRIVER)
    exe = tmp_path / "feature_map_check"
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "cerebro_amd/host"), "-I", str(ROOT / "include"), str(tmp_path / "driver.cc"),
           "-o", str(exe), "-L", str(lib), "-lcerebro_host", "-lcerebro_hip", f"-Wl,-rpath,{lib}", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "feature map path ok" in r.stdout, (r.stdout, r.stderr[-1500:])
