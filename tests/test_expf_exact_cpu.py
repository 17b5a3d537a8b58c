"""og_expf_exact (csrc/og_adsr_params.hip.h) against the host libm's expf on EVERY argument an envelope can form:
x = -4.6051702f / (float)n with the division in f32, n = 1 .. 2^24.  The coefficient 1 - expf(x) is applied n times, so
one ulp in expf is 2e-5 of level at n = 4 800: the lanes of og::AdsrP need the host's bits.  CPU only.

The routine aims at the correctly rounded value.  Condition: wherever it differs from libm, libm itself differs from
(float)exp((double)x) -- and libm does that on at most 2 of the 16 777 216 arguments (glibc 2.3x: n = 757 and n = 912)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 1 << 24
SRC = r'''
#include "og_adsr_params.hip.h"
// out_ours[]: n where og_expf_exact != expf; out_libm[]: n where expf != (float)exp((double)x); both capped at `cap`
extern "C" void sweep(unsigned n_max, unsigned cap, unsigned* n_ours, unsigned* out_ours, unsigned* n_libm, unsigned* out_libm)
{
    unsigned a = 0, b = 0;
    for (unsigned n = 1; n <= n_max; ++n) {
        const float x = -4.6051702f / (float)n;
        const float mine = og_expf_exact(x), lm = expf(x), cr = (float)exp((double)x);
        if (mine != lm) { if (a < cap) out_ours[a] = n; ++a; }
        if (lm != cr) { if (b < cap) out_libm[b] = n; ++b; }
    }
    *n_ours = a;
    *n_libm = b;
}
extern "C" float one(float x) { return og_expf_exact(x); }
'''


@pytest.fixture(scope="module")
def elib(tmp_path_factory):
    # built the way tests/test_og_math.py builds og_math.h
    d = tmp_path_factory.mktemp("ogexpf")
    src = d / "e.cpp"
    src.write_text(SRC)
    so = d / "libexpf_test.so"
    flags = ["-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "oscen_amd", "csrc")]
    if "fma" in open("/proc/cpuinfo").read():
        flags.append("-mfma")
    subprocess.run(["g++"] + flags + [str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.one.restype = C.c_float
    lib.one.argtypes = [C.c_float]
    return lib


def irregular(lib, n_max=N_MAX):
    """(n where og_expf_exact differs from libm, n where libm differs from the correctly rounded value)"""
    cap = 64
    ours, libm = (C.c_uint * cap)(), (C.c_uint * cap)()
    n_ours, n_libm = C.c_uint(), C.c_uint()
    lib.sweep(n_max, cap, C.byref(n_ours), ours, C.byref(n_libm), libm)
    assert n_ours.value <= cap and n_libm.value <= cap, (n_ours.value, n_libm.value)
    return list(ours[:n_ours.value]), list(libm[:n_libm.value])


def test_expf_exact_equals_libm_wherever_libm_is_correctly_rounded(elib):
    ours, libm = irregular(elib)
    print("og_expf_exact != expf at n =", ours, "; expf != (float)exp((double)x) at n =", libm)
    assert len(libm) <= 2, libm
    assert set(ours) <= set(libm), (ours, libm)


def test_expf_exact_end_points(elib):
    assert elib.one(-0.0) == 1.0
    assert elib.one(-4.6051702) == pytest.approx(0.01, rel=1e-6)
