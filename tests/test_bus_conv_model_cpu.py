"""BusConvolver (csrc/og_bus_conv_host.h: the post-mix Convolver's host bookkeeping) against a naive model, on the CPU:
tests/standalone/bus_conv_model_main.cpp drives the class beside a frame-by-frame model of the reference's swap and fade rules
and a shadow of the history buffer, and checks after every planned launch that every sample a response is entitled to is
readable and in the slot it is read from -- through wraps, growth and re-sizing.  The header is host C++ without HIP: it is
compiled alone first.  The program counts the branches it took; a run that missed one fails.  The same program runs under the
address and undefined-behaviour sanitizers (it has its own main: nothing is preloaded, nothing is loaded into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oscen_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "standalone", "bus_conv_model_main.cpp")
PATHS = ["history_wrap", "growth_by_taps", "resize_by_capacity", "retire_by_time", "swap_during_fade", "pending_replaced", "empty_response",
         "multi_run_launch", "tight_response", "growth_during_fade"]
SEEDS = [1, 2, 3, 4]


def clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if os.path.exists(c) or "/" not in c:
            return c


def run_and_check(exe):
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(exe)] + [str(s) for s in SEEDS], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.rstrip().endswith("ok")
    counts = {(int(s), name): int(n) for s, name, n in re.findall(r"^path seed (\d+) (\w+) (\d+)$", r.stdout, flags=re.M)}
    assert sorted(counts) == sorted((s, p) for s in SEEDS for p in PATHS)
    assert all(n > 0 for n in counts.values()), {k: n for k, n in counts.items() if n == 0}


def test_bus_conv_host_header_compiles_without_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "og_bus_conv_host.h")], check=True)
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "og_bus_conv_host.h")).read()).lower()


def test_bus_convolver_matches_the_model_and_takes_every_branch(tmp_path):
    exe = tmp_path / "bus_conv_model_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, MAIN, "-o", str(exe)], check=True)
    run_and_check(exe)


@pytest.mark.timeout(600)
def test_the_same_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "bus_conv_model_main_san"
    r = subprocess.run([clangxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + CSRC, MAIN, "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    run_and_check(exe)
