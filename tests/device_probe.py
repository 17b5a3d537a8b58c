"""Probes of single device helpers (test infrastructure; no conftest, no pytest settings).

A probe is a one-node graph around a plug-in node (oscen_amd.register_node) whose process() body calls the helper under
test: a run-time unit always includes og_nodes.hip.h and og_math.h, so og::div_near, og::fract_floor, og_sinf, ... are in
reach of the body.  Every lane forms its own arguments from per-voice value inputs, which carry raw f32 bits:

    x = __uint_as_float(__float_as_uint(a) + tick * __float_as_uint(sa))      (tick: a u32 state counter, one step per frame)
    y = __uint_as_float(__float_as_uint(b) + tick * __float_as_uint(sb))
    c, d: per-voice constants;   sel, u0 .. u3: block-uniform values (scalar registers)

i.e. a walk over bit patterns that numpy reproduces with integer arithmetic, bit for bit.  The body assigns r0 .. r3; they
leave the kernel as one Frame<4> voice output and are read through the voice taps.  `Probe.run` returns the arguments
together with the results; `host_eval` compiles the very same body text with g++ against og_math.h -- the flags of
tests/test_og_math.py -- for the helpers that are plain IEEE arithmetic (the "host build")."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FRAMES = 256
VOICES = 256
PER_VOICE = ("a", "sa", "b", "sb", "c", "d")
UNIFORM = ("sel", "u0", "u1", "u2", "u3")

# ---- the bodies: one run-time unit each ------------------------------------------------------------------------------
BODIES = {
    # r3 = x: the argument as the lane formed it (the witness that the walk on the host is the walk on the device)
    "sine": """
    r0 = og_sinf(x);
    r1 = og_sin_turns_poly(x);
    r2 = og_sin_turns(x);
    r3 = x;
""",
    "tangent": """
    r0 = og_tan_poly(x);
    r1 = og_tanf_q1(x);
    r2 = og::div_near(1.0f, og_tan_poly(x));
    r3 = x;
""",
    "exact": """
    r0 = og_sinf_exact(x);
    r1 = og_cosf_exact(x);
""",
    "divide": """
    r0 = og::div_near(x, y);
    r1 = og::div_rcp(x, y, __builtin_amdgcn_rcpf(y));
    r2 = __builtin_amdgcn_rcpf(y);
""",
    "fract": """
    r0 = og::fract_floor(x);
    r1 = og::wrap_phase(x);
    r2 = og::fract_keep_sign(x);
    r3 = (sel > 0.5f) ? og::fract_phase(x) : og::fmod1(x);
""",
    # Every float of a range, compared where it is formed: the lane walks the __float_as_uint(c) patterns from x on and counts
    # the ones at which a helper is not the value of the Rust semantics restated beside it (IEEE subtract, trunc, add; `==`
    # takes +0 for -0), 0.99999994 standing in where rem_euclid gives 1.0.  r2 counts those; r3 is the restated rem_euclid at
    # x itself, which the host holds against numpy -- the restatement is checked too.
    "fract_all": """
    const uint32_t first = __float_as_uint(x), count = __float_as_uint(c);
    uint32_t bad_floor = 0u, bad_keep = 0u, ones = 0u;
    for (uint32_t i = 0u; i < count; ++i) {
        const float v = __uint_as_float(first + i);
        const float r = v - truncf(v);
        const float w = (r < 0.0f) ? r + 1.0f : r;
        const float want = (w == 1.0f) ? 0.99999994f : w;
        ones += (w == 1.0f) ? 1u : 0u;
        bad_floor += (og::fract_floor(v) == want && og::wrap_phase(v) == want && og::fract_phase(v) == want) ? 0u : 1u;
        bad_keep += (og::fract_keep_sign(v) == r && og::fmod1(v) == r) ? 0u : 1u;
        if (i == 0u) r3 = w;
    }
    r0 = (float)bad_floor;
    r1 = (float)bad_keep;
    r2 = (float)ones;
""",
    "clamp": """
    r0 = og::clampf(x, c, d);
    r1 = og::clamp01(x);
""",
    # x = t, y = dt; rdt as polyblep_tick forms it
    "blep": """
    const float rdt = __builtin_amdgcn_rcpf(y);
    r0 = og::poly_blep(x, y, rdt);
    r1 = og::poly_blamp(x, y, rdt);
""",
    # x = cutoff input, c = q; u0 .. u3 = two_sr, period, nyquist, max_cutoff; sel picks the form (block-uniform: the branch
    # around the call is a scalar one, as in the kernels, so tpt_update_coefficients_iq's __any sees whole waves)
    "tpt": """
    const float cutoff = og::clampf(x, 20.0f, u3);
    float cc = -1.0f, cq = -1.0f, h = 0.0f, g = 0.0f, kq = 0.0f;
    if (sel < 0.5f) og::tpt_update_coefficients(cutoff, c, u0, u1, u2, cc, cq, h, g, kq);
    else if (sel < 1.5f) og::tpt_update_coefficients_iq(cutoff, c, 1.0f / c, u0, u1, u2, cc, cq, h, g, kq);
    else og::tpt_params_nomod_flat(x, c, 1.0f / c, u3, u0, u1, u2, cc, cq, h, g, kq);
    r0 = h;
    r1 = g;
    r2 = kq;
    r3 = sel;
""",
}

HEAD = """
    const uint32_t t_ = tick;
    tick += 1u;
    const float x = __uint_as_float(__float_as_uint(a) + t_ * __float_as_uint(sa));
    const float y = __uint_as_float(__float_as_uint(b) + t_ * __float_as_uint(sb));
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
"""
TAIL = """
    o0 = r0;
    o1 = r1;
    o2 = r2;
    o3 = r3;
"""


# ---- bit patterns ----------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(f32)


def walk(base, stride, frames=FRAMES, tick0=0):
    """what the lanes form: (voices, frames) f32 with bits base + (tick0 + frame) * stride, modulo 2^32"""
    base = np.atleast_1d(np.asarray(base)).astype(np.uint64)
    stride = np.broadcast_to(np.atleast_1d(np.asarray(stride)).astype(np.uint64), base.shape)
    t = np.arange(tick0, tick0 + frames, dtype=np.uint64)[None, :]
    return from_bits(((base[:, None] + t * stride[:, None]) & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def around(centres, half=64):
    """base patterns of the walks with stride 1 that visit `half` floats either side of each centre (2 * half + 1 <= frames)"""
    return (bits(centres).astype(np.int64) - half).astype(np.uint64)


def ordered(x):
    """f32 -> int64 that counts floats: ordered(nextafter(x)) = ordered(x) + 1 across zero, ordered(-0) = ordered(+0)"""
    u = bits(x).astype(np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)


def ulp_distance(a, b):
    return np.abs(ordered(a) - ordered(b))


def same_value(a, b):
    """bit-equal with +0 = -0"""
    return ordered(a) == ordered(b)


# ---- the device side -------------------------------------------------------------------------------------------------
class Probe:
    """one engine of `voices` lanes around BODIES[name]; every run() is a launch of `frames` frames"""

    def __init__(self, name, voices=VOICES):
        import oscen_amd

        self.name, self.voices, self.tick = name, voices, 0
        ctor = "DeviceProbe_%s::new" % name
        if ctor not in _registered:
            oscen_amd.register_node(
                ctor, inputs=[(p, "value", 0.0, -1) for p in PER_VOICE + UNIFORM], outputs=["o0", "o1", "o2", "o3"],
                state=[("tick", "u32", 0, -1)], process=HEAD + BODIES[name] + TAIL)
            _registered.add(ctor)
        ins = " ".join("input %s: value = 0.0;" % p for p in PER_VOICE + UNIFORM)
        con = " ".join("%s -> p.%s;" % (p, p) for p in PER_VOICE + UNIFORM)
        g = oscen_amd.Graph(dsl="name: DeviceProbe_%s; %s output out: stream: Frame<4>; nodes { p = %s(); } "
                                "connections { %s Frame(p.o0, p.o1, p.o2, p.o3) -> out; }" % (name, ins, ctor, con),
                            per_voice=list(PER_VOICE))
        self.eng = oscen_amd.Engine(g, voices, sample_rate=48000.0)
        self.eng.set_voice_taps(np.arange(voices, dtype=np.uint32))

    def run(self, a, sa=0, b=0, sb=0, c=0.0, d=0.0, frames=FRAMES, **uniform):
        """a, b: base bit patterns (integers) per voice; sa, sb: strides in bit patterns; c, d: f32 per voice.  Any number
        of voices: they are spread over launches of the engine's size (the last one padded with its last voice).
        Returns {"x", "y": (voices, frames) f32 as the lanes formed them, "c", "d": (voices,), "out": (voices, frames, 4)}."""
        a = np.atleast_1d(np.asarray(a)).astype(np.uint64)
        n = len(a)
        full = lambda v, ty: np.ascontiguousarray(np.broadcast_to(np.atleast_1d(np.asarray(v)).astype(ty), (n,)))
        sa, b, sb = full(sa, np.uint64), full(b, np.uint64), full(sb, np.uint64)
        c, d = full(c, f32), full(d, f32)
        for name, v in uniform.items():
            self.eng.set_value(name, float(v))
        out = np.empty((n, frames, 4), dtype=f32)
        mask = np.uint64(0xFFFFFFFF)
        for lo in range(0, n, self.voices):
            idx = np.minimum(np.arange(lo, lo + self.voices), n - 1)
            # the counter keeps running from launch to launch: start the walk that many steps back
            t0 = np.uint64(self.tick)
            self.eng.set_voice_values("a", from_bits(((a[idx] - t0 * sa[idx]) & mask).astype(np.uint32)))
            self.eng.set_voice_values("sa", from_bits((sa[idx] & mask).astype(np.uint32)))
            self.eng.set_voice_values("b", from_bits(((b[idx] - t0 * sb[idx]) & mask).astype(np.uint32)))
            self.eng.set_voice_values("sb", from_bits((sb[idx] & mask).astype(np.uint32)))
            self.eng.set_voice_values("c", c[idx])
            self.eng.set_voice_values("d", d[idx])
            self.eng.process_block(frames)
            self.tick += frames
            hi = min(n, lo + self.voices)
            out[lo:hi] = self.eng.read_voice_taps(frames)[:hi - lo]
        return {"x": walk(a, sa, frames), "y": walk(b, sb, frames), "c": c, "d": d, "out": out}

    def points(self, x, y=0.0, c=0.0, d=0.0, **uniform):
        """arbitrary arguments, one per lane (a launch of one frame): {"x", "y", "c", "d": (n,), "out": (n, 4)}"""
        x = np.ascontiguousarray(x, dtype=f32)
        y = np.ascontiguousarray(np.broadcast_to(np.asarray(y, dtype=f32), x.shape))
        r = self.run(bits(x), 0, bits(y), 0, c, d, frames=1, **uniform)
        return {"x": r["x"][:, 0], "y": r["y"][:, 0], "c": r["c"], "d": r["d"], "out": r["out"][:, 0]}


_registered = set()
_probes = {}


def probe(name, voices=VOICES):
    """the shared engine of a body (one run-time compilation per body and test session)"""
    if (name, voices) not in _probes:
        _probes[(name, voices)] = Probe(name, voices)
    return _probes[(name, voices)]


# ---- the host build --------------------------------------------------------------------------------------------------
HOST_EXTRA = """
extern "C" void ref_sinf(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = sinf(x[i]); }
extern "C" void ref_cosf(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = cosf(x[i]); }
extern "C" void ref_tanf(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = tanf(x[i]); }
extern "C" void ref_fmaf(const float* a, const float* b, const float* c, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = fmaf(a[i], b[i], c[i]); }
"""
HOST_BODIES = ("sine", "tangent", "exact")  # plain IEEE arithmetic: no device builtin behind them on the host
HOST_STANDINS = """
namespace og { static inline float div_near(float a, float b) { return a / b; } }  // the reference formula: the IEEE quotient
"""
_host = {}


def host_has_fma():
    return "fma" in open("/proc/cpuinfo").read()


def host_lib():
    """og_math.h and the probe bodies of HOST_BODIES compiled with g++: -O2 -ffp-contract=off, -mfma where the CPU has it"""
    if "lib" in _host:
        return _host["lib"]
    src = '#include "og_math.h"\n' + HOST_STANDINS + HOST_EXTRA
    for name in HOST_BODIES:
        src += ('extern "C" void probe_%s(const float* X, float* out, long n)\n{\n    for (long i = 0; i < n; ++i) {\n'
                '        const float x = X[i];\n        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;\n%s'
                '        out[4 * i] = r0; out[4 * i + 1] = r1; out[4 * i + 2] = r2; out[4 * i + 3] = r3;\n    }\n}\n'
                % (name, BODIES[name]))
    d = tempfile.mkdtemp(prefix="device_probe_")
    tag = hashlib.sha256(src.encode()).hexdigest()[:12]
    cpp, so = os.path.join(d, "host_%s.cpp" % tag), os.path.join(d, "libhost_%s.so" % tag)
    with open(cpp, "w") as f:
        f.write(src)
    flags = ["-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "oscen_amd", "csrc")]
    if host_has_fma():
        flags.append("-mfma")
    subprocess.run(["g++"] + flags + [cpp, "-o", so, "-lm"], check=True)
    _host["lib"] = C.CDLL(so)
    return _host["lib"]


def host_eval(name, x):
    """the host build of BODIES[name] at the arguments x: (len(x), 4) f32"""
    x = np.ascontiguousarray(x, dtype=f32).ravel()
    out = np.empty((len(x), 4), dtype=f32)
    fp = C.POINTER(C.c_float)
    getattr(host_lib(), "probe_" + name)(x.ctypes.data_as(fp), out.ctypes.data_as(fp), C.c_long(len(x)))
    return out


def host_libm(fn, *args):
    """sinf / cosf / tanf / fmaf of the host libm, elementwise"""
    args = [np.ascontiguousarray(a, dtype=f32).ravel() for a in args]
    y = np.empty_like(args[0])
    fp = C.POINTER(C.c_float)
    getattr(host_lib(), "ref_" + fn)(*([a.ctypes.data_as(fp) for a in args] + [y.ctypes.data_as(fp), C.c_long(len(y))]))
    return y


# ---- references in numpy f32 -----------------------------------------------------------------------------------------
def rem_euclid1(x):
    """f32::rem_euclid(1.0): r = x % 1.0; if r < 0 { r + 1.0 } else { r }"""
    x = np.asarray(x, dtype=f32)
    r = (x - np.trunc(x)).astype(f32)
    return np.where(r < 0, (r + f32(1.0)).astype(f32), r).astype(f32)


def fmod1(x):
    """`x % 1.0` = f32::fract: x - trunc(x)"""
    x = np.asarray(x, dtype=f32)
    return (x - np.trunc(x)).astype(f32)


def clamp(x, lo, hi):
    return np.clip(np.asarray(x, dtype=f32), np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)).astype(f32)


EPSILON = f32(1.1920929e-7)


def poly_blep(t, dt):
    """oscillators/mod.rs:139-153 in f32 with true division"""
    t, dt = np.asarray(t, dtype=f32), np.asarray(dt, dtype=f32)
    with np.errstate(all="ignore"):
        x1 = (t / dt).astype(f32)
        r1 = ((((x1 + x1).astype(f32) - (x1 * x1).astype(f32)).astype(f32)) - f32(1.0)).astype(f32)
        x2 = ((t - f32(1.0)).astype(f32) / dt).astype(f32)
        r2 = (((((x2 * x2).astype(f32) + x2).astype(f32) + x2).astype(f32)) + f32(1.0)).astype(f32)
        res = np.where(t < dt, r1, np.where(t > (f32(1.0) - dt).astype(f32), r2, f32(0.0)))
    return np.where(dt <= EPSILON, f32(0.0), res).astype(f32)


def poly_blamp(t, dt):
    """oscillators/mod.rs:155-169 in f32 with true division"""
    t, dt = np.asarray(t, dtype=f32), np.asarray(dt, dtype=f32)
    with np.errstate(all="ignore"):
        x1 = ((t / dt).astype(f32) - f32(1.0)).astype(f32)
        r1 = (-((x1 * x1).astype(f32) * x1).astype(f32) / f32(3.0)).astype(f32)
        x2 = (((t - f32(1.0)).astype(f32) / dt).astype(f32) + f32(1.0)).astype(f32)
        r2 = (((x2 * x2).astype(f32) * x2).astype(f32) / f32(3.0)).astype(f32)
        res = np.where(t < dt, r1, np.where(t > (f32(1.0) - dt).astype(f32), r2, f32(0.0)))
    return np.where(dt <= EPSILON, f32(0.0), res).astype(f32)


# ---- the TPT cases ---------------------------------------------------------------------------------------------------
TPT_RATES = (48000.0, 44100.0, 32000.0, 22050.0, 8000.0)
TPT_QS = (0.1, 0.70710678, 10.0)
TAU = f32(6.28318548202514648)
PIO4 = f32(float.fromhex("0x1.921fb6p-1"))


def tpt_slots(sr):
    """the block-uniform host slots as the engine forms them (og_graph.cpp, emit_tpt)"""
    sr = f32(sr)
    nyquist = f32(f32(sr * f32(0.5)) - EPSILON)
    return {"two_sr": f32(f32(2.0) * sr), "period": f32(f32(0.5) / sr), "nyquist": nyquist,
            "max_cutoff": f32(min(nyquist, f32(20000.0)))}


def tpt_x(cutoff, slots):
    """the argument of the tangent: F32_TAU * clamp(cutoff) * period, two f32 products"""
    c = clamp(clamp(cutoff, 20.0, slots["max_cutoff"]), 20.0, slots["nyquist"])
    return ((TAU * c).astype(f32) * slots["period"]).astype(f32)


def tpt_cutoffs(sr):
    """a geometric run from 20 Hz to max_cutoff with both ends, the two floats either side of the cutoff where x crosses
    pi/4, and the 64 floats below max_cutoff"""
    s = tpt_slots(sr)
    top = s["max_cutoff"]
    run = np.geomspace(20.0, float(top), 160).astype(f32)
    run[0], run[-1] = f32(20.0), top
    # the crossing: the largest cutoff with x <= pi/4 (x is monotone in the cutoff), found by bisection over bit patterns
    lo, hi = int(bits(f32(20.0))[0]), int(bits(top)[0])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tpt_x(from_bits([mid]), s)[0] <= PIO4:
            lo = mid
        else:
            hi = mid
    cross = from_bits(np.array([lo - 1, lo, hi, hi + 1], dtype=np.uint32))
    below = from_bits(int(bits(top)[0]) - np.arange(0, 65, dtype=np.uint32))
    return np.unique(np.concatenate([run, cross, below]))


def tpt_layout(cutoffs, slots):
    """The lanes of the three layouts for tpt_update_coefficients_iq's wave-uniform test, in blocks of 64 consecutive
    voices starting at a multiple of 64 (a wave, or a whole number of narrower ones): blocks wholly at or below pi/4, blocks
    wholly above, blocks with even lanes below and odd lanes above.  Returns (cutoff per lane, layout code per lane)."""
    x = tpt_x(cutoffs, slots)
    lo, hi = cutoffs[x <= PIO4], cutoffs[x > PIO4]
    assert len(lo) and len(hi)
    pad = lambda v: np.concatenate([v, np.repeat(v[-1], (-len(v)) % 64)])
    n = -(-max(len(lo), len(hi)) // 32) * 32
    mixed = np.empty(2 * n, dtype=f32)
    mixed[0::2] = np.resize(lo, n)
    mixed[1::2] = np.resize(hi, n)
    parts = [pad(lo), pad(hi), mixed]
    return np.concatenate(parts), np.concatenate([np.full(len(p), i) for i, p in enumerate(parts)])


def tpt_reference(cutoff, q, slots):
    """(h, g, k) of tpt/mod.rs:69-82 in f64 on the f32 argument x the three f32 products give and the f32 1/q"""
    x = tpt_x(cutoff, slots).astype(np.float64)
    inv_q = (f32(1.0) / np.asarray(q, dtype=f32)).astype(f32).astype(np.float64)
    g = float(slots["two_sr"]) * np.tan(x) * float(slots["period"])
    return 1.0 / (1.0 + inv_q * g + g * g), g, g + inv_q
