"""The post-mix Convolver (og_graph_add_bus_convolver / `Convolver::with_ir(name())` behind the voice sum; the kernels of
csrc/og_bus_conv.hip.h): y[t] = sum_k h[k] x[t-k] on the summed bus with zero latency, exact history across blocks and
batches, a summation order that depends on k alone, the reference's crossfade on a live response swap, snapshots.

Every test renders a DRY engine (built-in sub_voice, 70 voices) and a WET one (the same graph plus the bus Convolver) fed
the same notes; the first test establishes that the dry bus IS the convolver's input, bit for bit.  S = taps per segment
and F = frames per tile of the kernel's decomposition: the response lengths and delays sit on both sides of them."""
import ctypes as C

import numpy as np
import pytest

import oscen_amd
from tests import observed

pytestmark = pytest.mark.gpu
SR = 48000.0
N = 70
BLOCK = 256
TOTAL = 2048
S = oscen_amd.CONV_SEGMENT_TAPS
F = oscen_amd.CONV_TILE_FRAMES
FADE = 960  # max(1, round(0.02 * 48000))
f32 = np.float32


def wet_graph(ir_name, builtin="sub_voice"):
    g = oscen_amd.Graph(builtin=builtin)
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.output_stream("wet")
    g.bus_convolver("reverb", ir_name)
    g.connect(out, "reverb.input")
    g.connect("reverb.output", "wet")
    return g


def feed(eng):
    oscen_amd.schedule_note_plans(eng, oscen_amd.note_plans(N, span=TOTAL), total_frames=TOTAL)
    return eng


def engine(graph):
    return feed(oscen_amd.Engine(graph, N, sample_rate=SR))


def blocks(eng, n_blocks, block=BLOCK):
    return np.concatenate([eng.process_block(block).copy() for _ in range(n_blocks)], axis=0)


_dry = {}


def dry_bus():
    """2048 frames of the dry bank, rendered once and never modified"""
    if "bus" not in _dry:
        bus = blocks(engine("sub_voice"), TOTAL // BLOCK)
        assert bus.shape == (TOTAL, 1) and float(np.abs(bus).max()) > 1e-2
        bus.setflags(write=False)
        _dry["bus"] = bus
    return _dry["bus"]


class DeviceBuffer:
    """device memory for the asynchronous entry, through the HIP runtime the library is linked against"""

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


class registered:
    def __init__(self, **irs):
        self.irs = irs

    def __enter__(self):
        for k, v in self.irs.items():
            oscen_amd.register_ir(k, v)

    def __exit__(self, *a):
        for k in self.irs:
            oscen_amd.unregister_ir(k)


def noise_ir(k, seed):
    rng = np.random.default_rng(seed)
    h = (rng.uniform(-1.0, 1.0, k) * np.exp(-np.arange(k) * (6.0 / max(k, 16))) * 0.3).astype(f32)
    h[0] = 1.0
    return h


def conv64(h, x, since=0):
    """(float64 convolution of x[t >= since], the sum of the magnitudes of its products) over len(x) frames"""
    x = np.asarray(x, np.float64).copy()
    x[:since] = 0.0
    h = np.asarray(h, np.float64)
    if len(h) == 0:
        return np.zeros(len(x)), np.zeros(len(x))
    return np.convolve(x, h)[:len(x)], np.convolve(np.abs(x), np.abs(h))[:len(x)]


def check_rule(got, ref, base, tag=None):
    """the project's bus rule: |got - ref| <= 2e-6 * sum |products|, per sample, bound in float64"""
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(base, 1e-30) * (base > 0))) if np.any(base > 0) else 0.0
    observed.note(ratio, tag)
    assert np.all(err <= 2e-6 * base), (tag, ratio, float(err.max()))
    return ratio


def test_unit_tap_is_the_dry_bus_bit_for_bit():
    dry = dry_bus()
    with registered(unit=[1.0]):
        eng = engine(wet_graph("unit"))
        assert eng.channels == 1 and eng.post_mix_kind == 1
        wet = blocks(eng, TOTAL // BLOCK)
    assert np.array_equal(wet, dry)


DELAYS = sorted({1, 31, 32, 255, 256, 257, 511, 512, 513, S - 1, S, S + 1, 2 * S + 3})


@pytest.mark.parametrize("d", DELAYS)
def test_delayed_unit_tap(d):
    """wet[t] == dry[t - d], zeros before: every d crosses a block edge, the larger ones segment and tile edges"""
    dry = dry_bus()
    h = np.zeros(d + 1, f32)
    h[d] = 1.0
    with registered(delay=h):
        wet = blocks(engine(wet_graph("delay")), TOTAL // BLOCK)
    assert np.array_equal(wet[d:], dry[:TOTAL - d])
    assert not np.any(wet[:d])


@pytest.mark.parametrize("k", [2, S - 1, S + 1, 2 * S + 3, 1500])
def test_general_response_against_float64(k):
    dry = dry_bus()
    h = noise_ir(k, 100 + k)
    with registered(room=h):
        wet = blocks(engine(wet_graph("room")), TOTAL // BLOCK)
    ref, base = conv64(h, dry[:, 0])
    assert float(np.abs(ref).max()) > 1e-3
    check_rule(wet[:, 0], ref, base, "K=%d" % k)


def test_cutting_independence():
    """the same 2048 frames as 8 blocks of 256, as irregular blocks, and as one batched launch: bit-identical"""
    h = noise_ir(2 * S + 3, 7)
    with registered(room=h):
        g = wet_graph("room")
        a = blocks(engine(g), TOTAL // BLOCK)
        eng = engine(g)
        cuts = [64, 100, 256, 37, 255, 1, 256, 3, 256, 200, 256, 256]
        cuts.append(TOTAL - sum(cuts))
        assert cuts[-1] > 0 and max(cuts) <= 256
        b = np.concatenate([eng.process_block(c).copy() for c in cuts], axis=0)
        eng = engine(g)
        eng.set_bus_batching(8)
        c = eng.render(TOTAL, block=BLOCK).reshape(TOTAL, -1)
    assert float(np.abs(a).max()) > 1e-3
    assert np.array_equal(a, b)
    assert np.array_equal(a, c)


STEREO_VOICE = """
name: PanVoice;
input frequency: value = 220.0;
input gate: event;
output out: stream;
nodes {
    osc = PolyBlepOscillator::saw(220.0, 0.25);
    env = AdsrEnvelope::new(0.005, 0.05, 0.7, 0.05);
    p = ConvPan::new(0.3);
}
connections {
    frequency -> osc.frequency;
    gate -> env.gate;
    osc.output * env.output -> p.input;
    p.output -> out;
}
"""


def wrapper_text(voice_type, voice_out, n, params=(), post=None, out_type=""):
    """a poly wrapper in the reference's DSL (the shape of examples/fm-synth/src/lib.rs:22-131): MidiParser ->
    VoiceAllocator<n> -> [MidiVoiceHandler; n] -> [voice_type; n] -> sum [-> post-mix node]"""
    t = ["name: GeneratedPoly;", "input midi_in: event;"] + ["input %s;" % decl for _, decl in params]
    t += ["output out: stream%s;" % out_type]
    t += ["nodes {", "  midi_parser = MidiParser::new();", "  voice_allocator = VoiceAllocator::<%d>::new();" % n,
          "  voice_handlers = [MidiVoiceHandler::new(); %d];" % n, "  voices = [%s::new(); %d];" % (voice_type, n)]
    if post:
        t += ["  reverb = %s;" % post]
    t += ["}", "connections {", "  midi_in -> midi_parser.midi_in;", "  midi_parser.note_on -> voice_allocator.note_on;",
          "  midi_parser.note_off -> voice_allocator.note_off;", "  voice_allocator.voices -> voice_handlers.note_on;",
          "  voice_allocator.voices -> voice_handlers.note_off;", "  voice_handlers.frequency -> voices.frequency;",
          "  voice_handlers.gate -> voices.gate;"]
    t += ["  %s -> voices.%s;" % (nm, nm) for nm, _ in params]
    t += ["  voices.%s -> reverb.input;" % voice_out, "  reverb.output -> out;"] if post else ["  voices.%s -> out;" % voice_out]
    return "\n".join(t + ["}"])


def builtin_params(builtin):
    import re

    decl = oscen_amd.Graph(builtin=builtin).to_dsl()
    out = [ln.split()[1].rstrip(":;") for ln in decl.splitlines() if ln.startswith("output ")][0]
    ins = [ln.split("//")[0].strip().rstrip(";")[len("input "):] for ln in decl.splitlines() if ln.startswith("input ")]
    ins = [d for d in ins if not re.match(r"(frequency|gate)\b", d)]
    return out, [(re.match(r"(\w+)", d).group(1), d) for d in ins]


def test_stereo_voices_convolve_each_channel():
    """`Convolver::<Frame<2>>::with_ir` behind Frame<2> voices: the mono response on both channels, L -> L and R -> R"""
    oscen_amd.register_node("ConvPan::new", inputs=[("input", "stream", 0.0, -1), ("pan", "value", 0.5, 0)], outputs=[("output", 2)],
                            n_ctor_args=1, process="    output.v[0] = input * (1.0f - pan);\n    output.v[1] = input * pan;\n")
    oscen_amd.register_graph_type("PanVoice", oscen_amd.Graph(dsl=STEREO_VOICE))
    h = noise_ir(S + 1, 5)
    try:
        with registered(room=h):
            dry = engine(oscen_amd.Graph(dsl=wrapper_text("PanVoice", "out", 8, out_type=": Frame<2>")))
            wet = engine(oscen_amd.Graph(dsl=wrapper_text("PanVoice", "out", 8, post="Convolver::<Frame<2>>::with_ir(room())", out_type=": Frame<2>")))
            assert dry.channels == 2 and wet.channels == 2
            x, y = blocks(dry, 4), blocks(wet, 4)
            with pytest.raises(oscen_amd.OscenError, match="Frame<3>"):
                oscen_amd.Engine(oscen_amd.Graph(dsl=wrapper_text("PanVoice", "out", 8, post="Convolver::<Frame<3>>::with_ir(room())",
                                                                  out_type=": Frame<2>")), N, sample_rate=SR)
    finally:
        oscen_amd.unregister_graph_type("PanVoice")
        oscen_amd.unregister_node("ConvPan::new")
    assert x.shape == y.shape == (4 * BLOCK, 2)
    assert not np.array_equal(x[:, 0], x[:, 1])
    for c in range(2):
        ref, base = conv64(h, x[:, c])
        assert float(np.abs(ref).max()) > 1e-3
        check_rule(y[:, c], ref, base, "channel %d" % c)


def test_wrapper_text_gives_the_explicit_engine_bit_for_bit():
    """`voices.output -> reverb.input; reverb.output -> out` in DSL text, the response named by a path with arguments"""
    h = noise_ir(S + 1, 11)
    with registered(room=h):
        out, params = builtin_params("fm_voice")
        text = wrapper_text("FMVoice", out, 8, params=params, post="Convolver::with_ir(rooms::room(48000.0))")
        g = oscen_amd.Graph(dsl=text)
        assert g.poly_info() is not None
        a = blocks(engine(g), 4)
        b = blocks(engine(wet_graph("room", "fm_voice")), 4)
    assert float(np.abs(a).max()) > 1e-3 and a.shape == (4 * BLOCK, 1)
    assert np.array_equal(a, b)


def fade_gains(n):
    g = (np.arange(n, dtype=f32) / f32(FADE)).astype(f32)
    a = (g * f32(np.pi / 2)).astype(f32)
    return np.sin(a).astype(f32).astype(np.float64), np.cos(a).astype(f32).astype(np.float64)


def test_swap_crossfades_as_the_reference_does():
    """A (700 taps) -> B (300 taps) before the third block: fade_len = 960 is no multiple of the block.  Model in float64,
    gains in f32: B on empty history from the swap frame, A on its full history for 960 samples, new sin + old cos; then B
    alone.  The gain term of the bound (1e-6 (|new| + |old|)) covers the f32 sine / cosine: numpy's against the kernel's
    restatement of libm's differ by an ulp (6e-8) at most."""
    dry = dry_bus()[:, 0]
    hA, hB = noise_ir(700, 1), noise_ir(300, 2)
    ts = 2 * BLOCK
    with registered(A=hA, B=hB):
        eng = engine(wet_graph("A"))
        got = [blocks(eng, 2)]
        eng.set_bus_ir("B")
        got.append(blocks(eng, TOTAL // BLOCK - 2))
    got = np.concatenate(got)[:, 0].astype(np.float64)
    old, old_base = conv64(hA, dry)
    new, new_base = conv64(hB, dry, since=ts)
    gn, go = fade_gains(FADE)
    assert np.max(np.abs(old)) > 1e-3 and np.max(np.abs(new[ts:])) > 1e-3
    check_rule(got[:ts], old[:ts], old_base[:ts], "before")
    fade = slice(ts, ts + FADE)
    ref = new[fade] * gn + old[fade] * go
    bound = 2e-6 * (old_base[fade] + new_base[fade]) + 1e-6 * (np.abs(new[fade]) + np.abs(old[fade]))
    err = np.abs(got[fade] - ref)
    observed.note(float(np.max(err / np.maximum(bound, 1e-30))), "fade")
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-30)))
    assert got[ts] == pytest.approx(old[ts], abs=float(bound[0]))  # pos = 0: the old response alone
    check_rule(got[ts + FADE:], new[ts + FADE:], new_base[ts + FADE:], "after")  # the tail of pre-swap input ends with the fade
    assert np.max(np.abs(old[ts + FADE:] - new[ts + FADE:])) > 1e-4


def test_second_swap_during_a_fade_restarts_from_the_current_response():
    """B at frame 512, C at frame 1024 (pos = 512 of 960): A is dropped at once, B -- history from 512 -- fades into C"""
    dry = dry_bus()[:, 0]
    hA, hB, hC = noise_ir(700, 1), noise_ir(300, 2), noise_ir(S + 40, 3)
    t1, t2 = 2 * BLOCK, 4 * BLOCK
    with registered(A=hA, B=hB, C=hC):
        eng = engine(wet_graph("A"))
        eng.set_bus_batching(4)  # the swaps travel with the queued blocks
        buf = DeviceBuffer(TOTAL * 4)
        try:
            for b in range(TOTAL // BLOCK):
                if b == 2:
                    eng.set_bus_ir("B")
                if b == 4:
                    eng.set_bus_ir("C")
                eng.process_block_async(BLOCK, buf.ptr.value + b * BLOCK * 4)
            eng.flush()
            eng.synchronize()
            got = buf.to_host().reshape(TOTAL, 1)
        finally:
            buf.free()
    got = got[:, 0].astype(np.float64)
    a, a_base = conv64(hA, dry)
    b, b_base = conv64(hB, dry, since=t1)
    c, c_base = conv64(hC, dry, since=t2)
    gn, go = fade_gains(FADE)
    n1 = t2 - t1
    ref = b[t1:t2] * gn[:n1] + a[t1:t2] * go[:n1]
    bound = 2e-6 * (a_base[t1:t2] + b_base[t1:t2]) + 1e-6 * (np.abs(b[t1:t2]) + np.abs(a[t1:t2]))
    assert np.all(np.abs(got[t1:t2] - ref) <= bound)
    fade = slice(t2, t2 + FADE)
    ref = c[fade] * gn + b[fade] * go
    bound = 2e-6 * (b_base[fade] + c_base[fade]) + 1e-6 * (np.abs(c[fade]) + np.abs(b[fade]))
    assert np.all(np.abs(got[fade] - ref) <= bound)
    check_rule(got[t2 + FADE:], c[t2 + FADE:], c_base[t2 + FADE:], "after")
    assert np.max(np.abs(c[t2 + FADE:])) > 1e-3


def test_swap_to_a_longer_response_keeps_the_outgoing_history():
    """A (300 taps: the history is sized for 512 frames) -> B (700 taps: 768) before the third block.  The history is
    reallocated at the publish; A must still see its full pre-swap input for the 960 frames it fades over.  The model and
    the bounds are those of test_swap_crossfades_as_the_reference_does."""
    dry = dry_bus()[:, 0]
    hA, hB = noise_ir(300, 1), noise_ir(700, 2)
    assert -(-len(hA) // S) * S == 512 and -(-len(hB) // S) * S == 768
    ts = 2 * BLOCK
    with registered(A=hA, B=hB):
        eng = engine(wet_graph("A"))
        got = [blocks(eng, 2)]
        eng.set_bus_ir("B")
        got.append(blocks(eng, TOTAL // BLOCK - 2))
    got = np.concatenate(got)[:, 0].astype(np.float64)
    old, old_base = conv64(hA, dry)
    new, new_base = conv64(hB, dry, since=ts)
    gn, go = fade_gains(FADE)
    assert np.max(np.abs(old)) > 1e-3 and np.max(np.abs(new[ts:])) > 1e-3
    check_rule(got[:ts], old[:ts], old_base[:ts], "before")
    fade = slice(ts, ts + FADE)
    ref = new[fade] * gn + old[fade] * go
    bound = 2e-6 * (old_base[fade] + new_base[fade]) + 1e-6 * (np.abs(new[fade]) + np.abs(old[fade]))
    err = np.abs(got[fade] - ref)
    observed.note(float(np.max(err / np.maximum(bound, 1e-30))), "fade")
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-30)))
    # A's part of the fade comes from input before the swap: without it the error would be far outside the bound
    lost, _ = conv64(hA, dry, since=ts)
    assert np.max(np.abs((old[fade] - lost[fade]) * go) - bound) > 1e-3
    check_rule(got[ts + FADE:], new[ts + FADE:], new_base[ts + FADE:], "after")


def test_batching_changed_in_mid_stream():
    """three blocks at a queue of 1, then set_bus_batching(8) -- the history and the rows are re-sized for the longer
    launch -- and the remaining blocks in one launch: bit-identical to eight plain blocks"""
    h = noise_ir(2 * S + 3, 7)
    with registered(room=h):
        g = wet_graph("room")
        want = blocks(engine(g), TOTAL // BLOCK)
        eng = engine(g)
        head = blocks(eng, 3)
        eng.set_bus_batching(8)
        rest = TOTAL // BLOCK - 3
        buf = DeviceBuffer(rest * BLOCK * 4)
        try:
            for b in range(rest):
                eng.process_block_async(BLOCK, buf.ptr.value + b * BLOCK * 4)
            eng.flush()
            eng.synchronize()
            tail = buf.to_host().reshape(rest * BLOCK, 1)
        finally:
            buf.free()
    assert float(np.abs(want).max()) > 1e-3
    assert np.array_equal(np.concatenate([head, tail]), want)


def test_empty_convolver_is_silent_until_a_response_is_set():
    dry = dry_bus()[:, 0]
    hB = noise_ir(300, 2)
    ts = 3 * BLOCK
    with registered(B=hB, nothing=[]):
        eng = engine(wet_graph(None))
        head = blocks(eng, 3)
        eng.set_bus_ir("B")
        tail = blocks(eng, TOTAL // BLOCK - 3)[:, 0].astype(np.float64)
        silent = blocks(engine(wet_graph("nothing")), 2)
    assert head.shape == (ts, 1) and not np.any(head) and not np.any(silent)
    new, base = conv64(hB, dry, since=ts)
    gn, _ = fade_gains(FADE)
    ref = new[ts:].copy()
    ref[:FADE] *= gn
    assert np.all(np.abs(tail - ref) <= 2e-6 * base[ts:] + 1e-6 * np.abs(new[ts:]))
    assert np.max(np.abs(ref)) > 1e-3


def test_snapshot_mid_fade_continues_sample_for_sample():
    hA, hB = noise_ir(700, 1), noise_ir(300, 2)
    with registered(A=hA, B=hB):
        g = wet_graph("A")
        eng = engine(g)
        blocks(eng, 2)
        eng.set_bus_ir("B")
        blocks(eng, 1)  # pos = 256 of 960
        assert eng.state_bytes > 0
        blob = eng.save_state()
        assert blob.nbytes == eng.state_bytes
        want = blocks(eng, 4)
        fresh = oscen_amd.Engine(g, N, sample_rate=SR)
        fresh.load_state(blob)
        got = blocks(fresh, 4)
        assert float(np.abs(want).max()) > 1e-3
        assert np.array_equal(got, want)
        # a blob without the convolver's section does not load into an engine that has one, and the other way round
        plain = oscen_amd.Engine("sub_voice", N, sample_rate=SR)
        with pytest.raises(oscen_amd.OscenError):
            fresh.load_state(plain.save_state())
        with pytest.raises(oscen_amd.OscenError):
            plain.load_state(blob)
    # a graph without a Convolver: the blob is what it was -- state planes, header (32 bytes), value + ramp per input
    plain = oscen_amd.Engine("sub_voice", N, sample_rate=SR)
    assert plain.state_bytes == plain.state_words_per_voice * N * 4 + 32 + 20 * plain.lib.og_num_inputs(plain.h)


def test_refusals():
    with registered(room=[1.0, 0.5]):
        with pytest.raises(oscen_amd.OscenError, match="unknown impulse response 'nowhere'"):
            oscen_amd.Engine(wet_graph("nowhere"), N, sample_rate=SR)
        # a Convolver as a voice node
        g = oscen_amd.Graph(dsl="""
            name: ReverbVoice; input frequency: value = 220.0; input gate: event; output out: stream;
            nodes { osc = PolyBlepOscillator::saw(220.0, 0.2); reverb = Convolver::with_ir(room()); }
            connections { frequency -> osc.frequency; osc.output -> reverb.input; reverb.output -> out; }""")
        with pytest.raises(oscen_amd.OscenError, match="only available as the post-mix") as ei:
            oscen_amd.Engine(g, N, sample_rate=SR)
        assert ei.value.code == oscen_amd.OG_E_UNSUPPORTED
        # a second bus node
        g = wet_graph("room")
        g.bus_convolver("again", "room")
        with pytest.raises(oscen_amd.OscenError, match="only one post-mix"):
            oscen_amd.Engine(g, N, sample_rate=SR)
        # set_bus_ir without a bus Convolver, and with an unregistered name
        with pytest.raises(oscen_amd.OscenError, match="no post-mix Convolver"):
            oscen_amd.Engine("sub_voice", N, sample_rate=SR).set_bus_ir("room")
        with pytest.raises(oscen_amd.OscenError, match="unknown impulse response 'nowhere'"):
            oscen_amd.Engine(wet_graph("room"), N, sample_rate=SR).set_bus_ir("nowhere")
        with pytest.raises(oscen_amd.OscenError, match="cluster over a graph with a post-mix Convolver") as ei:
            oscen_amd.Cluster(wet_graph("room"), N, [0], sample_rate=SR)
        assert ei.value.code == oscen_amd.OG_E_UNSUPPORTED
