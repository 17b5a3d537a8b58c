"""AdsrEnvelope whose attack / decay / sustain / release move: per voice (og_set_voice_values), ramped (`[ramp: N]`) and
as an expression of both -- the second envelope body, og::AdsrP (csrc/og_adsr_params.hip.h).  `-m gpu`.

Reference: the oracle's oo_adsr, one struct per voice, its attack / decay / sustain / release fields written on every frame
before oo_adsr_process exactly as the graph feeds them, gate events handled between the write and the process() (the
reference's order at the outer rate: codegen/emit_frame.rs:219-229).  Tolerance: the suite's 1e-5 on the level.

Largest error of each case, MI355X: profiles/adsr_params_observed.md."""
import ctypes as C
import math

import numpy as np
import pytest

import oscen_amd
from tests import oracle_lib as ol
from tests.test_bench_entry_points_gpu import DeviceBuffer

pytestmark = pytest.mark.gpu
SR = 48000.0
TOL = 1e-5
BLOCK = 256
CTOR = (0.01, 0.02, 0.6, 0.05)

# attack, decay per voice; sustain ramped; release = (per voice) * (ramped factor): a per-sample value of the kernel
ENV = """
name: EnvMoving;
input gate: event;
input att: value = 0.01;
input dec: value = 0.02;
input sus: value = 0.6 [ramp: 300];
input relv: value = 0.05;
input relk: value = 1.0 [ramp: 200];
output out: stream;
nodes { env = AdsrEnvelope::new(0.01, 0.02, 0.6, 0.05); }
connections { gate -> env.gate; att -> env.attack; dec -> env.decay; sus -> env.sustain; relv * relk -> env.release; env.output -> out; }
"""


@pytest.fixture(scope="module")
def graph():
    return oscen_amd.Graph(dsl=ENV, per_voice=["att", "dec", "relv"])


class Ramp:
    """ValueRampState in f32 (oracle: oo_ramp_*): ticked at the top of every frame"""

    def __init__(self, v):
        self.cur = self.tgt = np.float32(v)
        self.inc = np.float32(0)
        self.rem = 0

    def set(self, v, frames):
        v = np.float32(v)
        if v == self.tgt:
            return
        self.tgt, self.inc, self.rem = v, np.float32((v - self.cur) / np.float32(frames)), frames

    def tick(self):
        if self.rem > 0:
            self.rem -= 1
            self.cur = self.tgt if self.rem == 0 else np.float32(self.cur + self.inc)
        return self.cur


def oracle(n, frames, att, dec, relv, events, sus_sets=(), relk_sets=(), relv_sets=()):
    """level [n, frames] of n oo_adsr structs.
    events: {voice: [(frame, value)]}; sus_sets / relk_sets: [(frame, target, ramp frames)]; relv_sets: [(frame, array)]"""
    lib = ol.load()
    sus, relk = Ramp(CTOR[2]), Ramp(1.0)
    s_f, k_f = np.empty(frames, np.float32), np.empty(frames, np.float32)
    for i in range(frames):
        for f, v, fr in sus_sets:
            if f == i:
                sus.set(v, fr)
        for f, v, fr in relk_sets:
            if f == i:
                relk.set(v, fr)
        s_f[i], k_f[i] = sus.tick(), relk.tick()
    relv = np.array(relv, np.float32)
    rel = np.empty((n, frames), np.float32)
    start = 0
    for f, arr in list(relv_sets) + [(frames, None)]:
        rel[:, start:f] = relv[:, None] * k_f[None, start:f]
        start = f
        if arr is not None:
            relv = np.array(arr, np.float32)
    out = np.zeros((n, frames), np.float32)
    for v in range(n):
        e = ol.Adsr()
        lib.oo_adsr_new(C.byref(e), *CTOR)
        e.sample_rate = SR
        lib.oo_adsr_prepare(C.byref(e))
        evs = dict()
        for f, val in events.get(v, ()):
            evs.setdefault(f, []).append(val)
        ref, proc, gate = C.byref(e), lib.oo_adsr_process, lib.oo_adsr_handle_gate_event
        a_v, d_v = float(att[v]), float(dec[v])
        for i in range(frames):
            e.attack, e.decay, e.sustain, e.release = a_v, d_v, s_f[i], rel[v, i]
            if i in evs:
                for val in evs[i]:
                    gate(ref, C.byref(ol.Event(0, val, 0)))
            proc(ref)
            out[v, i] = e.output
    return out


def engine(graph, n, att, dec, relv, events, taps=True):
    eng = oscen_amd.Engine(graph, n, sample_rate=SR)
    eng.set_voice_values("att", att)
    eng.set_voice_values("dec", dec)
    eng.set_voice_values("relv", relv)
    vs, fs, xs = [], [], []
    for v, lst in events.items():
        for f, val in lst:
            vs.append(v), fs.append(f), xs.append(val)
    eng.schedule_voice_events("gate", vs, fs, xs)
    if taps:
        eng.set_voice_taps(list(range(n)))
    return eng


def run(eng, blocks, between=None):
    got = []
    for b in range(blocks):
        if between:
            between(eng, b)
        eng.process_block(BLOCK)
        got.append(eng.read_voice_taps(BLOCK).copy())
    return np.concatenate(got, axis=1)


def check(got, ref, what):
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print("%s: max |level - oracle| = %.3g" % (what, err))
    assert err <= TOL, (what, err)


# ---- case 1: per-voice attack and decay --------------------------------------------------------------------------
N1, BLOCKS1 = 200, 8


def case1():
    att = np.concatenate([[0.0], np.geomspace(1e-3, 0.04, N1 - 1)]).astype(np.float32)  # 0 = the instant-attack branch
    dec = att[::-1].copy()
    relv = np.full(N1, 0.01, np.float32)
    # note-on at frame 3; note-off inside a voice-dependent stage (Attack / Decay / Sustain); some voices strike again
    events = {v: [(3, 0.8), (300 + 6 * v, 0.0)] + ([(1600, 1.0)] if v % 3 == 0 else []) for v in range(N1)}
    return att, dec, relv, events


@pytest.fixture(scope="module")
def ref1():
    att, dec, relv, events = case1()
    return oracle(N1, BLOCK * BLOCKS1, att, dec, relv, events)


def test_per_voice_attack_and_decay(graph, ref1):
    att, dec, relv, events = case1()
    got = run(engine(graph, N1, att, dec, relv, events), BLOCKS1)
    assert len(np.unique(np.argmax(got[:, :300] >= 0.79, axis=1))) > 50  # the voices really rise at their own rates
    check(got, ref1, "case 1 (per-voice attack / decay, 200 voices)")


# ---- case 2: per-voice release changed while the voice is mid-Release ------------------------------------------------
def test_release_changed_mid_release_reclamps_samples_remaining(graph):
    n, blocks = 192, 8
    att = dec = np.full(n, 0.001, np.float32)
    relv = np.full(n, 0.02, np.float32)  # 960 frames; the gate-off is at 300, the change in front of frame 512: 748 left
    new = (0.002 + 0.0004 * np.arange(n)).astype(np.float32)  # 96 .. 3763 frames: shorter than what is left, and longer
    events = {v: [(3, 1.0), (300, 0.0)] for v in range(n)}
    ref = oracle(n, BLOCK * blocks, att, dec, relv, events, relv_sets=[(512, new)])
    got = run(engine(graph, n, att, dec, relv, events), blocks, lambda eng, b: b == 2 and eng.set_voice_values("relv", new))
    ends = np.argmax(got[:, 512:] == 0.0, axis=1)
    assert ends.min() < 110 and ends.max() > 700 and len(np.unique(ends)) > 20  # cut short, and left alone
    check(got, ref, "case 2 (release changed mid-Release, 192 voices)")


# ---- case 3: ramped sustain across a block boundary, ramped release started mid-Release -----------------------------------
def test_ramped_sustain_and_ramped_release(graph):
    n, blocks = 200, 10
    att = np.full(n, 0.001, np.float32)
    dec = np.where(np.arange(n) % 2 == 0, 0.001, 0.03).astype(np.float32)  # half in Sustain, half still in Decay at frame 256
    relv = np.full(n, 0.03, np.float32)
    events = {v: [(3, 0.9), (700 + v, 0.0)] for v in range(n)}
    sus_sets, relk_sets = [(256, 0.2, 300)], [(1024, 0.5, 200)]  # sustain glides over 256 .. 555; release shrinks from 1024 on
    ref = oracle(n, BLOCK * blocks, att, dec, relv, events, sus_sets=sus_sets, relk_sets=relk_sets)

    def between(eng, b):
        if b == 1:
            eng.set_value_with_ramp("sus", 0.2, 300)
        if b == 4:
            eng.set_value_with_ramp("relk", 0.5, 200)

    got = run(engine(graph, n, att, dec, relv, events), blocks, between)
    assert abs(got[0, 400] - got[0, 300]) > 0.05  # a voice in Sustain follows the glide
    check(got, ref, "case 3 (ramped sustain / release, 200 voices)")


# ---- case 4: the coefficient's bits ----------------------------------------------------------------------------------
def test_attack_coefficient_has_the_host_libms_bits(graph):
    libm = C.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
    ns = np.unique(np.geomspace(2, 2.0e6, 4096).astype(np.int64))
    att = ((ns + 0.5) / SR).astype(np.float32)
    assert np.array_equal((att * np.float32(SR)).astype(np.uint32), ns)  # attack_samples really is n
    x = (np.float32(-4.6051702) / ns.astype(np.float32)).astype(np.float32)
    e = np.array([libm.expf(float(v)) for v in x], np.float32)
    regular = e == np.array([math.exp(float(v)) for v in x]).astype(np.float32)  # (libm's own irregular n: tests/test_expf_exact_cpu.py)
    assert regular.sum() >= len(ns) - 2
    want = (np.float32(1.0) - e).astype(np.float32)
    n = len(ns)
    eng = engine(graph, n, att, np.full(n, 0.02, np.float32), np.full(n, 0.05, np.float32), {v: [(0, 1.0)] for v in range(n)})
    eng.process_block(16)
    got = eng.read_voice_taps(16)[:, 0]  # frame 0: 0 + (1 - 0) * attack_coeff
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & regular)[0]
    print("case 4: %d attack lengths n = %d .. %d, %d skipped, %d differ from the host's bits" % (n, ns[0], ns[-1], n - regular.sum(), len(bad)))
    assert len(bad) == 0, [(int(ns[i]), float(got[i]), float(want[i])) for i in bad[:8]]


# ---- case 5: per-voice inputs that all hold the constants == the constant-parameter graph ------------------------------
SUB = """
name: SubEnv%(tag)s;
input frequency: value = 220.0;
input gate: event;
%(inputs)s
output out: stream;
nodes {
    osc = PolyBlepOscillator::saw(220.0, 0.7);
    env = AdsrEnvelope::new(0.005, 0.02, 0.6, 0.03);
    filter = TptFilter::new(1800.0, 0.9);
}
connections {
    frequency -> osc.frequency; gate -> env.gate; %(wires)s
    osc.output -> filter.input;
    filter.output * env.output -> out;
}
"""
SUB_PV = dict(tag="PerVoice", inputs="input a: value = 0.005; input d: value = 0.02; input s: value = 0.6; input r: value = 0.03;",
              wires="a -> env.attack; d -> env.decay; s -> env.sustain; r -> env.release;")


def test_per_voice_inputs_holding_the_constants_equal_the_constant_graph():
    n, blocks = 200, 8
    freqs = np.geomspace(80.0, 2000.0, n).astype(np.float32)
    events = {v: [(3 + v % 5, 0.7), (500 + 4 * v, 0.0)] for v in range(n)}
    engs = []
    for kw, pv in ((dict(tag="Const", inputs="", wires=""), ["frequency"]), (SUB_PV, ["frequency", "a", "d", "s", "r"])):
        e = oscen_amd.Engine(oscen_amd.Graph(dsl=SUB % kw, per_voice=pv), n, sample_rate=SR)
        e.set_voice_values("frequency", freqs)
        vs, fs, xs = zip(*[(v, f, x) for v, l in events.items() for f, x in l])
        e.schedule_voice_events("gate", vs, fs, xs)
        e.set_voice_taps(list(range(n)))
        engs.append(e)
    for name, val in zip("adsr", (0.005, 0.02, 0.6, 0.03)):
        engs[1].set_voice_values(name, np.full(n, val, np.float32))
    worst = 0.0
    for b in range(blocks):
        outs = []
        for e in engs:
            e.process_block(BLOCK)
            outs.append(e.read_voice_taps(BLOCK).astype(np.float64))
        worst = max(worst, float(np.max(np.abs(outs[0] - outs[1]))))
        for field in ("env.stage", "env.samples_remaining"):
            assert np.array_equal(engs[0].read_state_field(field, dtype=np.uint32), engs[1].read_state_field(field, dtype=np.uint32)), (field, b)
    print("case 5: max |per-voice-parameter graph - constant graph| = %.3g" % worst)
    assert worst <= TOL, worst


# ---- case 6: the queued path and a snapshot ----------------------------------------------------------------------------
def test_queued_blocks_and_a_restored_snapshot_are_bit_identical(graph, ref1):
    att, dec, relv, events = case1()
    a = engine(graph, N1, att, dec, relv, events, taps=False)
    want = np.concatenate([a.process_block(BLOCK).copy() for _ in range(BLOCKS1)], axis=0)
    q = engine(graph, N1, att, dec, relv, events, taps=False)
    ch = q.channels
    buf = DeviceBuffer(BLOCKS1 * BLOCK * ch * 4)
    try:
        q.process_blocks_async(BLOCK, BLOCKS1, buf.ptr.value, BLOCK * ch * 4)
        q.synchronize()
        assert np.array_equal(buf.to_host().reshape(BLOCKS1 * BLOCK, ch), want)
    finally:
        buf.free()
    # a snapshot in front of block 1: most voices are in Decay (attack <= 40 ms ... their note-off comes at 300 + 6 v)
    s = engine(graph, N1, att, dec, relv, events)
    s.process_block(BLOCK)
    assert (s.read_state_field("env.stage", dtype=np.uint32) == 2).sum() > 20
    blob = s.save_state()
    r = oscen_amd.Engine(graph, N1, sample_rate=SR)
    r.load_state(blob)
    r.set_voice_taps(list(range(N1)))
    rest = np.concatenate([(r.process_block(BLOCK), r.read_voice_taps(BLOCK).copy())[1] for _ in range(BLOCKS1 - 1)], axis=1)
    cont = np.concatenate([(s.process_block(BLOCK), s.read_voice_taps(BLOCK).copy())[1] for _ in range(BLOCKS1 - 1)], axis=1)
    assert np.array_equal(rest, cont)
    check(cont, ref1[:, BLOCK:], "case 6 (restored snapshot against the oracle)")
