"""The asset impulse-response tests (tests/test_ir_assets_gpu.py, `-m gpu`) on the host simulator (tests/hostsim/, TEST
INFRASTRUCTURE): the kernels of csrc/og_bus_conv.hip.h with their per-channel tap planes, the plane mapping, the resampler in
front of it and the engine's host code around them -- registry, publishing, read-back, the snapshot section -- compiled for
x86, every lane a fibre, the same C ABI and the same bit-for-bit comparisons as on the MI355X.  A subprocess, like
tests/test_sample_player_hostsim_cpu.py: the simulator is reached through OSCEN_GPU_LIB only.  One simulated device."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CASES = 20  # tests in the file, the parametrised ones counted per case


@pytest.mark.timeout(900)
def test_ir_asset_tests_on_the_host_simulator():
    sys.path.insert(0, HOSTSIM)
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    lib = build_hostsim.build()
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = lib
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(lib), "fake_rccl") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    env.pop("OG_HOSTSIM_DEVICES", None)
    env.pop("OSCEN_GPU_SPLIT", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "300", "-p", "no:cacheprovider",
                        "tests/test_ir_assets_gpu.py"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = r.stdout[-4000:]
    assert r.returncode == 0 and "%d passed" % CASES in tail and "failed" not in tail and "skipped" not in tail, tail
