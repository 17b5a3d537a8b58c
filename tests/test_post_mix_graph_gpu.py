"""Post-mix graphs: wrapper-level nodes behind the voice sum (og_graph_add_bus_node with any constructor), compiled as a
second graph of one voice and run by the one-wave post-mix kernel (og_kp_<hash>_{00,10}, csrc/og_post_mix.hip.h) between the
bus reduce and the copies.

The voices are the built-in sub_voice with its oscillator turned down (70 of them: one full wave and a partial one; or 1),
or a small stereo voice, so that the dry sum stays inside [-1, 1] (asserted).  Parity is checked by stepping the oracle's nodes in
f32 over THE DEVICE'S OWN dry sum (Engine.post_mix_input), so the summation order of the voice tree is not part of the
comparison; the tolerance is the project's per-sample 1e-5, |got - ref| / max(1, |ref|).  Every graph here has the same voice kernel and the library keeps a compiled unit by its hash, so hiprtc runs once per
distinct unit of the module; a dry render per voice count is made once and never modified."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oscen_amd
from tests import observed
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
SR = 48000.0
N = 70
BLOCK = 256
TOTAL = 2048
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- graphs ------------------------------------------------------------------------------------------------------------
def sub_voice(params=True):
    """sub_voice turned down, plus the three wrapper inputs the parametrised post-mix graphs use: every graph of this file has
    the same voice kernel (the library keeps a compiled unit by its hash)"""
    dsl = oscen_amd.Graph(builtin="sub_voice").to_dsl()
    quiet = dsl.replace("PolyBlepOscillator::saw(440.0, 0.600000024)", "PolyBlepOscillator::saw(440.0, 0.03)")  # 70 voices sum to < 1
    assert quiet != dsl
    g = oscen_amd.Graph(dsl=quiet, per_voice=("frequency",))
    if params:
        g.input_value("cut", 1200.0, ramp=300)
        g.input_value("dly", 0.0)
        g.input_value("vol", 0.5)
    return g


def chain(g, nodes, edges, out="wet"):
    g.output_stream(out)
    for name, ctor, *args in nodes:
        g.bus_node(name, ctor, *args)
    for e in edges:
        if len(e) == 3:
            g.connect_via(*e)
        else:
            g.connect(*e)
    return g


def g_identity():
    return chain(sub_voice(), [("unity", "Gain::new", 1.0)], [("audio", "unity.input"), ("unity.output", "wet")])


def g_tpt_gain():
    return chain(sub_voice(), [("master", "TptFilter::new", 1200.0, 0.707), ("trim", "Gain::new", 0.5)],
                 [("audio", "master.input"), ("cut", "master.cutoff"), ("master.output", "trim.input"), ("vol", "trim.gain"), ("trim.output", "wet")])


def g_delay():
    return chain(sub_voice(), [("echo", "Delay::new", 0.0, 0.0)], [("audio", "echo.input"), ("dly", "echo.delay_samples"), ("echo.output", "wet")])


def g_iir():
    return chain(sub_voice(), [("lp", "IirLowpass::new", 1000.0, 0.707)], [("audio", "lp.input"), ("lp.output", "wet")])


def g_echo():
    return chain(sub_voice(), [("master", "TptFilter::new", 1200.0, 0.707), ("echo", "Delay::new", 37.0, 0.4), ("trim", "Gain::new", 0.5)],
                 [("audio", "master.input"), ("cut", "master.cutoff"), ("master.output", "echo", "trim.input"), ("trim.output", "wet")])


def g_lfo():
    return chain(sub_voice(), [("lfo", "Oscillator::sine", 30.0, 1.0), ("master", "TptFilter::new", 1200.0, 0.707)],
                 [("audio", "master.input"), ("lfo.output * 800.0 + 1200.0", "master.cutoff"), ("master.output", "wet")])


PAN_VOICE = """
name: PanVoice;
input frequency: value = 220.0;
input gate: event;
output out: stream;
nodes {
    osc = PolyBlepOscillator::saw(220.0, 0.02);
    env = AdsrEnvelope::new(0.005, 0.05, 0.7, 0.05);
    p = PmPan::new(0.3);
}
connections {
    frequency -> osc.frequency;
    gate -> env.gate;
    osc.output * env.output -> p.input;
    p.output -> out;
}
"""


def register_nodes():
    oscen_amd.register_node("PmPan::new", inputs=[("input", "stream", 0.0, -1), ("pan", "value", 0.5, 0)], outputs=[("output", 2)], n_ctor_args=1,
                            process="    output.v[0] = input * (1.0f - pan);\n    output.v[1] = input * pan;\n")
    oscen_amd.register_node("PmClip::new", inputs=[("input", "stream", 0.0, -1)], outputs=["output"],
                            process="    output = og::clampf(input * 4.0f, -0.25f, 0.25f);\n")


def g_stereo():
    register_nodes()
    g = oscen_amd.Graph(dsl=PAN_VOICE, per_voice=("frequency",))
    return chain(g, [("master", "TptFilter::<Frame<2>>::new", 1500.0, 0.9)], [("out", "master.input"), ("master.output", "wet")])


def g_pan():
    register_nodes()
    return chain(sub_voice(), [("pan", "PmPan::new", 0.25)], [("audio", "pan.input"), ("pan.output", "wet")])


def g_clip():
    register_nodes()
    return chain(sub_voice(), [("master", "TptFilter::new", 1200.0, 0.707), ("clip", "PmClip::new")],
                 [("audio", "master.input"), ("master.output", "clip.input"), ("clip.output", "wet")])


# ---- engines -----------------------------------------------------------------------------------------------------------
def feed(eng, n=N, total=TOTAL):
    plans = oscen_amd.note_plans(n, span=total)
    eng.set_voice_values("frequency", plans["frequency"])
    ev_v, ev_f, ev_x = plans["events"]
    keep = ev_f < total
    eng.schedule_voice_events(eng.index("gate"), ev_v[keep], ev_f[keep], ev_x[keep])
    return eng


def engine(graph, n=N):
    return feed(oscen_amd.Engine(graph, n, sample_rate=SR), n)


def render(eng, cuts):
    """(bus, dry sum) over the blocks `cuts`, block by block through the blocking entry"""
    bus, dry = [], []
    for c in cuts:
        bus.append(eng.process_block(c).copy())
        dry.append(eng.post_mix_input(c).copy())
    return np.concatenate(bus, axis=0), np.concatenate(dry, axis=0)


EIGHT = [BLOCK] * (TOTAL // BLOCK)
_twin = {}


def twin_bus(n):
    """the bus of the same voices without post-mix nodes: rendered once per voice count, read-only"""
    if n not in _twin:
        eng = engine(sub_voice(), n)
        bus = np.concatenate([eng.process_block(c).copy() for c in EIGHT], axis=0)
        assert bus.shape == (TOTAL, 1) and 1e-3 < float(np.abs(bus).max()) <= 1.0
        bus.setflags(write=False)
        _twin[n] = bus
    return _twin[n]


def close(got, ref, tag=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    worst = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    observed.note(worst, tag)
    print("post-mix parity %s: max error %.3e" % (tag, worst))
    assert worst <= 1e-5, (tag, worst)
    return worst


# ---- the oracle's nodes, stepped in f32 ---------------------------------------------------------------------------------
class Nodes:
    def __init__(self):
        self.lib = ol.load()
        self.delays = []

    def tpt(self, cutoff, q, channels=1):
        f = ol.Tpt()
        self.lib.oo_tpt_new(C.byref(f), cutoff, q, channels)
        f.sample_rate = SR
        self.lib.oo_tpt_prepare(C.byref(f))
        return f

    def delay(self, samples, feedback):
        d = ol.Delay()
        self.lib.oo_delay_new(C.byref(d), samples, feedback)
        d.sample_rate = SR
        self.lib.oo_delay_prepare(C.byref(d))
        self.delays.append(d)
        return d

    def iir(self, cutoff, q):
        f = ol.IirLowpass()
        self.lib.oo_iir_lowpass_new(C.byref(f), cutoff, q)
        f.sample_rate = SR
        self.lib.oo_iir_lowpass_prepare(C.byref(f))
        return f

    def osc(self, freq, amp):
        o = ol.Oscillator()
        self.lib.oo_oscillator_new(C.byref(o), freq, amp, ol.WAVE_SINE)
        o.sample_rate = SR
        return o

    def gain(self, x, g):
        k = ol.Gain()
        k.input, k.gain = float(x), float(g)
        self.lib.oo_gain_process(C.byref(k))
        return f32(k.output)

    def run_tpt(self, f, x, cutoff=None):
        if cutoff is not None:
            f.cutoff = float(cutoff)
        f.input[0] = float(x)
        self.lib.oo_tpt_process(C.byref(f))
        return f32(f.output[0])

    def run_delay(self, d, x):
        d.input = float(x)
        self.lib.oo_delay_process(C.byref(d))
        return f32(d.output)

    def close(self):
        for d in self.delays:
            self.lib.oo_delay_free(C.byref(d))


def ramp_values(start, target, frames, n):
    """ValueRampState (graph/types.rs:300-373): the value frame f sees is the one after f + 1 ticks"""
    cur, out = f32(start), np.empty(n, f32)
    inc = f32(f32(f32(target) - cur) / f32(frames))
    left = frames
    for i in range(n):
        if left > 0:
            left -= 1
            cur = f32(target) if left == 0 else f32(cur + inc)
        out[i] = cur
    return out


# ---- 1: identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N, 1])
def test_unity_gain_is_the_twin_bus_bit_for_bit(n):
    eng = engine(g_identity(), n)
    assert eng.post_mix_kind == 2 and eng.channels == 1
    bus, dry = render(eng, EIGHT)
    assert np.array_equal(bus, twin_bus(n))
    assert np.array_equal(dry.reshape(-1, 1), twin_bus(n))


# ---- 2: parity -----------------------------------------------------------------------------------------------------------
def test_tpt_into_gain_matches_the_oracle_over_the_device_sum():
    eng = engine(g_tpt_gain())
    bus, dry = render(eng, EIGHT)
    assert float(np.abs(dry).max()) <= 1.0
    o = Nodes()
    f = o.tpt(1200.0, 0.707)
    ref = np.array([o.gain(o.run_tpt(f, x, 1200.0), 0.5) for x in dry], f32)
    close(bus[:, 0], ref, "tpt->gain")
    # state: the filter's first integrator, as the oracle's node holds it
    z0 = eng.read_state_field("master.z0", 0, 1)
    assert abs(float(z0[0]) - float(f.z[0][0])) <= 1e-5 * max(1.0, abs(float(f.z[0][0])))
    with pytest.raises(oscen_amd.OscenError, match="post-mix node"):
        eng.read_state_field("master.z0", 0, 2)
    with pytest.raises(oscen_amd.OscenError, match="post-mix node"):
        eng.read_state_field("master.z0", 1, 1)
    assert eng.lib.og_state_field_index(eng.h, b"master.z0") >= eng.state_words_per_voice


@pytest.mark.parametrize("d", [0, 5, 16, 37])
def test_delay_alone_is_exact(d):
    eng = engine(g_delay())
    eng.set_value("dly", float(d))
    bus, dry = render(eng, [BLOCK] * 4)
    assert float(np.abs(dry).max()) <= 1.0
    o = Nodes()
    line = o.delay(float(d), 0.0)
    ref = np.array([o.run_delay(line, x) for x in dry], f32)
    o.close()
    assert np.array_equal(bus[:, 0], ref), d


def test_iir_lowpass_matches_the_oracle():
    eng = engine(g_iir())
    bus, dry = render(eng, EIGHT)
    o = Nodes()
    f = o.iir(1000.0, 0.707)
    ref = np.array([o.lib.oo_iir_lowpass_process_sample(C.byref(f), float(x)) for x in dry], f32)
    close(bus[:, 0], ref, "iir")


def echo_reference(dry, cutoffs, gain=0.5):
    """master -> [echo] -> trim: the reference's order is master, trim, echo -- trim reads what the echo put out a frame ago"""
    o = Nodes()
    f, line = o.tpt(1200.0, 0.707), o.delay(37.0, 0.4)
    prev, ref = f32(0.0), np.empty(len(dry), f32)
    for i, x in enumerate(dry):
        m = o.run_tpt(f, x, cutoffs[i])
        ref[i] = o.gain(prev, gain)
        prev = o.run_delay(line, m)
    o.close()
    return ref


def test_filter_echo_gain_matches_the_oracle():
    eng = engine(g_echo())
    bus, dry = render(eng, EIGHT)
    assert float(np.abs(dry).max()) <= 1.0 and float(np.abs(bus).max()) > 1e-4
    close(bus[:, 0], echo_reference(dry, np.full(TOTAL, 1200.0, f32)), "tpt->[delay 0.4]->gain")


# ---- 3: block cuts -------------------------------------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, nbytes):
        self.rt = oscen_amd.load_library()
        self.ptr = C.c_void_p()
        self.nbytes = nbytes
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]
        assert self.rt.hipMalloc(C.byref(self.ptr), nbytes) == 0
        assert self.rt.hipMemset(self.ptr, 0, nbytes) == 0

    def to_host(self):
        out = np.empty(self.nbytes // 4, dtype=np.float32)
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, self.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.ptr:
            self.rt.hipFree(self.ptr)
            self.ptr = None


RAGGED = [1, 15, 16, 17, 256, 512, 207]
CUT_TOTAL = 1024


def queued(eng, batching, gap=0):
    """four 256-frame blocks through the asynchronous entry; gap > 0: their device destinations are `gap` floats apart"""
    eng.set_bus_batching(batching)
    stride = BLOCK + gap
    buf = DeviceBuffer(4 * stride * 4)
    try:
        for b in range(4):
            eng.process_block_async(BLOCK, buf.ptr.value + b * stride * 4)
        eng.flush()
        eng.synchronize()
        got = buf.to_host().reshape(4, stride)
    finally:
        buf.free()
    if gap:
        assert not got[:, BLOCK:].any()  # (nothing is written between the destinations)
    return got[:, :BLOCK].reshape(CUT_TOTAL, 1)


def test_block_cuts_are_bit_identical():
    assert sum(RAGGED) == CUT_TOTAL
    g = g_echo()
    want = engine(g).render(CUT_TOTAL, block=512)
    assert float(np.abs(want).max()) > 1e-4
    eng = engine(g)
    assert np.array_equal(np.concatenate([eng.process_block(BLOCK).copy() for _ in range(4)]), want)
    eng = engine(g)
    assert np.array_equal(np.concatenate([eng.process_block(c).copy() for c in RAGGED]), want)
    assert np.array_equal(queued(engine(g), 4), want)
    assert np.array_equal(queued(engine(g), 0), want)


def test_block_cuts_with_destinations_that_are_not_contiguous():
    g = g_echo()
    want = engine(g).render(CUT_TOTAL, block=BLOCK)
    assert np.array_equal(queued(engine(g), 4, gap=48), want)
    assert np.array_equal(queued(engine(g), 0, gap=3), want)


# ---- 4: parameters -------------------------------------------------------------------------------------------------------
def test_ramped_wrapper_input_moves_the_cutoff_every_frame():
    eng = engine(g_echo())
    bus, dry = [], []
    for b in range(4):
        if b == 1:
            eng.set_value("cut", 4000.0)  # [ramp: 300]: frames 256 .. 555, across the block boundary at 512
        bus.append(eng.process_block(BLOCK).copy())
        dry.append(eng.post_mix_input(BLOCK).copy())
    bus, dry = np.concatenate(bus), np.concatenate(dry)
    cut = np.concatenate([np.full(BLOCK, 1200.0, f32), ramp_values(1200.0, 4000.0, 300, 3 * BLOCK)])
    assert cut[BLOCK + 299] == f32(4000.0) and cut[BLOCK + 298] != f32(4000.0)
    close(bus[:, 0], echo_reference(dry, cut), "ramped cutoff")


def test_set_value_between_queued_blocks_lands_on_that_blocks_first_frame():
    g = g_tpt_gain()
    eng = engine(g)
    eng.set_bus_batching(4)
    buf = DeviceBuffer(4 * BLOCK * 4)
    try:
        for b in range(4):
            if b == 2:
                eng.set_value("vol", 0.25)  # (launches the two queued blocks first)
            eng.process_block_async(BLOCK, buf.ptr.value + b * BLOCK * 4)
        eng.flush()
        eng.synchronize()
        got = buf.to_host()
    finally:
        buf.free()
    plain = engine(g)
    _, dry = render(plain, [BLOCK] * 4)
    o = Nodes()
    f = o.tpt(1200.0, 0.707)
    ref = np.array([o.gain(o.run_tpt(f, x, 1200.0), 0.5 if i < 2 * BLOCK else 0.25) for i, x in enumerate(dry)], f32)
    close(got, ref, "set_value between queued blocks")
    # gains that are powers of two: the step is exact
    mid = np.array([o.gain(1.0, 0.5), o.gain(1.0, 0.25)], f32)
    assert mid[0] == f32(0.5) and mid[1] == f32(0.25)


def test_an_lfo_inside_the_post_mix_graph_drives_the_cutoff():
    eng = engine(g_lfo())
    assert eng.post_mix_info()["nodes"] == 2
    bus, dry = render(eng, EIGHT)
    o = Nodes()
    lfo, f = o.osc(30.0, 1.0), o.tpt(1200.0, 0.707)
    ref = np.empty(TOTAL, f32)
    for i, x in enumerate(dry):
        o.lib.oo_oscillator_process(C.byref(lfo))
        ref[i] = o.run_tpt(f, x, f32(f32(f32(lfo.output) * f32(800.0)) + f32(1200.0)))
    close(bus[:, 0], ref, "lfo -> cutoff")


# ---- 5: width ------------------------------------------------------------------------------------------------------------
def test_stereo_voices_into_a_stereo_filter():
    eng = engine(g_stereo())
    assert eng.channels == 2 and eng.lib.og_voice_channels(eng.h) == 2 and eng.post_mix_kind == 2
    assert eng.post_mix_info() == {"nodes": 1, "in_channels": 2, "out_channels": 2, "state_words": eng.post_mix_info()["state_words"]}
    bus, dry = render(eng, [BLOCK] * 4)
    assert dry.shape == (4 * BLOCK, 2) and float(np.abs(dry).max()) <= 1.0 and float(np.abs(dry[:, 1]).max()) > 1e-4
    o = Nodes()
    f = o.tpt(1500.0, 0.9, 2)
    ref = np.empty_like(bus)
    for i in range(len(dry)):
        f.input[0], f.input[1] = float(dry[i, 0]), float(dry[i, 1])
        o.lib.oo_tpt_process(C.byref(f))
        ref[i] = (f.output[0], f.output[1])
    close(bus, ref, "Frame<2> tpt")


def test_mono_sum_into_a_pan_node_gives_two_channels():
    eng = engine(g_pan())
    assert eng.channels == 2 and eng.lib.og_voice_channels(eng.h) == 1 and eng.post_mix_kind == 2
    info = eng.post_mix_info()
    assert (info["nodes"], info["in_channels"], info["out_channels"]) == (1, 1, 2)
    bus, dry = render(eng, [BLOCK, 100, 156])
    assert np.array_equal(dry.reshape(-1, 1), twin_bus(N)[:2 * BLOCK])
    pan = f32(0.25)
    assert np.array_equal(bus[:, 0], dry * f32(f32(1.0) - pan)) and np.array_equal(bus[:, 1], dry * pan)


def test_a_hard_clip_behind_the_filter():
    eng = engine(g_clip())
    assert eng.post_mix_kind == 2  # (linearity is never assumed)
    bus, dry = render(eng, [BLOCK] * 4)
    o = Nodes()
    f = o.tpt(1200.0, 0.707)
    ref = np.array([np.clip(f32(o.run_tpt(f, x, 1200.0) * f32(4.0)), f32(-0.25), f32(0.25)) for x in dry], f32)
    assert float(np.abs(ref).max()) == 0.25 and float(np.abs(ref).min()) < 0.25  # (it clips, and not everywhere)
    close(bus[:, 0], ref, "tpt->clip")


# ---- 6: state ------------------------------------------------------------------------------------------------------------
def test_init_resets_the_post_mix_state():
    eng = engine(g_echo())
    first = np.concatenate([eng.process_block(BLOCK).copy() for _ in range(4)])
    assert eng.read_state_field("echo.write_pos", 0, 1, dtype=np.uint32)[0] != 0
    eng.init(SR)
    assert eng.read_state_field("echo.write_pos", 0, 1, dtype=np.uint32)[0] == 0
    feed(eng)
    again = np.concatenate([eng.process_block(BLOCK).copy() for _ in range(4)])
    assert float(np.abs(first).max()) > 1e-4 and np.array_equal(first, again)


def test_snapshot_in_mid_render_continues_bit_for_bit():
    g = g_echo()
    a = engine(g)
    want = np.concatenate([a.process_block(BLOCK).copy() for _ in range(6)])
    b = engine(g)
    head = np.concatenate([b.process_block(BLOCK).copy() for _ in range(3)])
    blob = b.save_state()
    c = oscen_amd.Engine(g, N, sample_rate=SR)
    c.load_state(blob)
    tail = np.concatenate([c.process_block(BLOCK).copy() for _ in range(3)])
    assert np.array_equal(np.concatenate([head, tail]), want)
    # the section closes the blob, and is refused when it is not this graph's
    info = c.post_mix_info()
    plain = engine(sub_voice())
    plain.process_block(BLOCK)
    with pytest.raises(oscen_amd.OscenError, match="post-mix graph's section"):
        c.load_state(plain.save_state())
    same = engine(sub_voice())  # the same voices after the same three blocks, without the post-mix nodes
    for _ in range(3):
        same.process_block(BLOCK)
    ring, head = 1 << 17, 40  # next_power_of_two(min(2 sr, 88200)) samples of the echo's line; the section's head
    assert len(blob) - len(same.save_state()) == head + 4 * (info["state_words"] + ring)
    with pytest.raises(oscen_amd.OscenError):
        plain.load_state(blob)


def test_a_blob_without_a_post_mix_graph_keeps_its_length():
    eng = engine(sub_voice())
    eng.process_block(BLOCK)
    blob = eng.save_state()
    n_inputs, header, ramp, event = eng.lib.og_num_inputs(eng.h), 32, 16, 24
    events = (len(blob) - eng.state_words_per_voice * N * 4 - header - n_inputs * (4 + ramp))
    assert events >= 0 and events % event == 0  # state planes + control block + unfired events, and nothing behind them
    assert len(blob) == eng.state_bytes


# ---- 7: legacy -----------------------------------------------------------------------------------------------------------
def test_a_lone_tremolo_keeps_its_stage_and_its_kernel():
    g = oscen_amd.Graph(builtin="epiano_voice")
    assert g.post_mix_source() == ""
    eng = oscen_amd.Engine(g, 8, sample_rate=SR)
    assert eng.post_mix_kind == 1 and eng.channels == 2
    committed = open(os.path.join(ROOT, "oscen_amd", "csrc", "gen", "epiano_voice.hip")).read()
    name = eng.lib.og_kernel_name(eng.h).decode()
    assert re.fullmatch(r"og_k\d?w?_[0-9a-f]{16}", name) and name.split("_")[-1] in committed
    with pytest.raises(oscen_amd.OscenError):
        eng.post_mix_info()
    with pytest.raises(oscen_amd.OscenError):
        eng.post_mix_input(1)


# ---- 8: cluster ----------------------------------------------------------------------------------------------------------
def test_a_cluster_over_a_post_mix_graph_is_refused():
    n_dev = C.c_int(0)
    if oscen_amd.load_library().hipGetDeviceCount(C.byref(n_dev)) != 0 or n_dev.value < 2:
        pytest.skip("needs two visible devices")
    with pytest.raises(oscen_amd.OscenError, match="post-mix graph"):
        oscen_amd.Cluster(g_identity(), N, [0, 1], sample_rate=SR)
