"""The moving-parameter envelope tests (tests/test_adsr_params_gpu.py, `-m gpu`) on the host simulator (tests/hostsim/,
TEST INFRASTRUCTURE): the generated og::AdsrP kernels and the engine's host code compiled for x86, every lane a fibre, the
same C ABI and the same oracle as on the MI355X.  Checks the body's control flow -- the gate queue, the lazy block begin,
the samples_remaining clamp, the pipelined shape of the equivalence case, snapshots -- without a GPU; og_expf_exact is plain
C++, so the coefficient case holds bit for bit here too.  A subprocess, like tests/test_hostsim_cpu.py: the simulator is
reached through OSCEN_GPU_LIB only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")


@pytest.mark.timeout(900)
def test_moving_parameter_envelope_tests_on_the_host_simulator():
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
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "--timeout", "300", "-p", "no:cacheprovider",
                        "tests/test_adsr_params_gpu.py"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "6 passed" in r.stdout[-2000:], r.stdout[-4000:]
