"""The post-mix graph tests (tests/test_post_mix_graph_gpu.py, `-m gpu`) on the host simulator (tests/hostsim/, TEST
INFRASTRUCTURE): the generated post-mix units with csrc/og_post_mix.hip.h and the engine's host code -- the second state
image, the planar reduce, the launch order, the snapshot section, the cluster refusal -- compiled for x86, every lane a
fibre, the same C ABI and the same oracle nodes as on the MI355X.  A subprocess, like tests/test_sample_player_hostsim_cpu.py:
the simulator is reached through OSCEN_GPU_LIB only.  Once with one simulated device (the cluster case skips, as on a one-GPU
machine) and once with two, so that it executes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")
CASES = 22  # tests in the file, the parametrised ones counted per case


def run(devices):
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
    if devices > 1:
        env["OG_HOSTSIM_DEVICES"] = str(devices)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "300", "-p", "no:cacheprovider",
                        "tests/test_post_mix_graph_gpu.py"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout[-4000:]


@pytest.mark.timeout(900)
def test_post_mix_graph_tests_on_the_host_simulator():
    rc, tail = run(1)
    assert rc == 0 and "%d passed, 1 skipped" % (CASES - 1) in tail and "failed" not in tail, tail


@pytest.mark.timeout(900)
def test_post_mix_graph_tests_on_two_simulated_devices():
    rc, tail = run(2)
    assert rc == 0 and "%d passed" % CASES in tail and "skipped" not in tail and "failed" not in tail, tail
