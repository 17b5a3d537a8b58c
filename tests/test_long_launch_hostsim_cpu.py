"""The long-launch tests (tests/test_long_launch_gpu.py, `-m gpu`) on the host simulator (tests/hostsim/, TEST INFRASTRUCTURE):
the engine's queue -- the frame capacity, the automatic rule, the limits, the early launches -- and the kernels it launches
over more than 32 blocks, compiled for x86, every lane a fibre, the same C ABI and the same bit-for-bit comparisons as on the
MI355X.  A subprocess, like tests/test_ir_assets_hostsim_cpu.py: the simulator is reached through OSCEN_GPU_LIB only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CASES = 9  # tests in the file, the parametrised ones counted per case


@pytest.mark.timeout(900)
def test_long_launch_tests_on_the_host_simulator():
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
                        "tests/test_long_launch_gpu.py"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = r.stdout[-4000:]
    assert r.returncode == 0 and "%d passed" % CASES in tail and "failed" not in tail and "skipped" not in tail, tail
