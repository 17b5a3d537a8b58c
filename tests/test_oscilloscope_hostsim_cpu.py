"""The Oscilloscope tests (tests/test_oscilloscope_gpu.py, `-m gpu`) on the host simulator (tests/hostsim/, TEST
INFRASTRUCTURE): csrc/og_scope.hip.h and the engine's host code -- planes in the node-array pool, the reconstruction of a read,
the clear, snapshots, grouped voices -- compiled for x86, every lane a fibre, the same C ABI and the same numpy witness as on
the MI355X.  A subprocess, like tests/test_sample_player_hostsim_cpu.py: the simulator is reached through OSCEN_GPU_LIB only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CASES = 24  # tests in the file, the parametrised ones counted per case


@pytest.mark.timeout(900)
def test_oscilloscope_tests_on_the_host_simulator():
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
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "600", "-p", "no:cacheprovider",
                        "tests/test_oscilloscope_gpu.py"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = r.stdout[-4000:]
    assert r.returncode == 0 and "%d passed" % CASES in tail and "skipped" not in tail and "failed" not in tail, tail
