"""Asset impulse responses on the post-mix Convolver: multi-channel, rate-tagged responses (og_register_ir_asset /
og_register_ir_wav) published with og_set_bus_ir -- conformed to the engine's rate by the load path's resampler, mapped onto
the bus's channels as MultiConvolverEngine::from_asset does, one tap plane per channel in the kernels of
csrc/og_bus_conv.hip.h -- read-back, swaps, batching, block cuts, snapshots, refusals.

Every comparison is BIT EQUALITY: channels are independent and the order in which an output sample's products are summed
depends on k alone, so channel c of a run under a per-channel response is channel c of the same bus run under the MONO
response `plane[c]` (the path the existing bus tests hold against float64).  70 voices (a full wave and a 6-lane remainder),
48 000 Hz, 2048 frames; a mono bus (built-in sub_voice), a Frame<2> and a Frame<4> bus (wrapper graphs around a panning
voice)."""
import ctypes as C
import struct

import numpy as np
import pytest

import oscen_amd

pytestmark = pytest.mark.gpu
SR = 48000
N = 70
BLOCK = 256
TOTAL = 2048
FADE = 960  # max(1, round(0.02 * 48000))
f32 = np.float32

PAN_VOICE = """
name: %s;
input frequency: value = 220.0;
input gate: event;
output out: stream;
nodes {
    osc = PolyBlepOscillator::saw(220.0, 0.25);
    env = AdsrEnvelope::new(0.005, 0.05, 0.7, 0.05);
    p = %s::new(0.3);
}
connections {
    frequency -> osc.frequency;
    gate -> env.gate;
    osc.output * env.output -> p.input;
    p.output -> out;
}
"""
# kind -> (voice graph type, pan node type, channels, the pan node's process body)
WIDE = {
    "st": ("IraPanVoice2", "IraPan2", 2, "    output.v[0] = input * (1.0f - pan);\n    output.v[1] = input * pan;\n"),
    "quad": ("IraPanVoice4", "IraPan4", 4, "    output.v[0] = input * (1.0f - pan);\n    output.v[1] = input * pan;\n"
                                           "    output.v[2] = input * 0.5f;\n    output.v[3] = input * (pan - 1.0f);\n"),
}
CHANNELS = {"mono": 1, "st": 2, "quad": 4}


def wrapper_text(voice_type, n, width, wet=True):
    """a poly wrapper in the reference's DSL around `voice_type`, its Frame<width> sum through an empty Convolver (wet) or
    straight to the output"""
    t = ["name: IraPoly;", "input midi_in: event;", "output out: stream: Frame<%d>;" % width, "nodes {", "  midi_parser = MidiParser::new();",
         "  voice_allocator = VoiceAllocator::<%d>::new();" % n, "  voice_handlers = [MidiVoiceHandler::new(); %d];" % n,
         "  voices = [%s::new(); %d];" % (voice_type, n)] + (["  reverb = Convolver::<Frame<%d>>::new();" % width] if wet else []) + ["}", "connections {",
         "  midi_in -> midi_parser.midi_in;", "  midi_parser.note_on -> voice_allocator.note_on;", "  midi_parser.note_off -> voice_allocator.note_off;",
         "  voice_allocator.voices -> voice_handlers.note_on;", "  voice_allocator.voices -> voice_handlers.note_off;",
         "  voice_handlers.frequency -> voices.frequency;", "  voice_handlers.gate -> voices.gate;"]
    t += ["  voices.out -> reverb.input;", "  reverb.output -> out;", "}"] if wet else ["  voices.out -> out;", "}"]
    return "\n".join(t)


def mono_graph(ir_name=None):
    g = oscen_amd.Graph(builtin="sub_voice")
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.output_stream("wet")
    g.bus_convolver("reverb", ir_name)
    g.connect(out, "reverb.input")
    g.connect("reverb.output", "wet")
    return g


def noise(frames, channels, seed):
    rng = np.random.default_rng(seed)
    h = (rng.uniform(-1.0, 1.0, (frames, channels)) * np.exp(-np.arange(frames) * (6.0 / frames))[:, None] * 0.3).astype(f32)
    h[0] = 1.0 - 0.125 * np.arange(channels)  # the channels differ from the first tap on
    return h


# the asset responses: name -> (frames x channels, rate).  300 frames at 44 100 Hz are 327 taps at 48 000: across the 256-tap segment
ASSETS = {
    "ira::m44": (noise(300, 1, 1), 44100),
    "ira::m96": (noise(700, 1, 2), 96000),  # downsampling: the kernel widened by 1 / cutoff
    "ira::m48": (noise(300, 1, 3), 48000),  # equal rates: a copy
    "ira::st44": (noise(300, 2, 4), 44100),
    "ira::tri44": (noise(290, 3, 5), 44100),
    "ira::st48": (noise(520, 2, 6), 48000),
}
MONO = {"ira::a": noise(700, 1, 7)[:, 0], "ira::b": noise(300, 1, 8)[:, 0]}  # og_register_ir: mono, at the session rate
_planes = {}
_derived = []


@pytest.fixture(scope="module", autouse=True)
def registrations():
    for kind, (vt, node, width, body) in WIDE.items():
        oscen_amd.register_node(node + "::new", inputs=[("input", "stream", 0.0, -1), ("pan", "value", 0.5, 0)], outputs=[("output", width)],
                                n_ctor_args=1, process=body)
        oscen_amd.register_graph_type(vt, oscen_amd.Graph(dsl=PAN_VOICE % (vt, node)))
    for name, (a, rate) in ASSETS.items():
        oscen_amd.register_ir(name, a, sample_rate=rate)
    for name, h in MONO.items():
        oscen_amd.register_ir(name, h)
    yield
    for name in list(ASSETS) + list(MONO) + _derived:
        oscen_amd.unregister_ir(name)
    for kind, (vt, node, width, body) in WIDE.items():
        oscen_amd.unregister_graph_type(vt)
        oscen_amd.unregister_node(node + "::new")


def planes(name):
    """the asset conformed to 48 000 Hz by og_resample, [taps, source channels]: computed once, never modified"""
    if name not in _planes:
        a, rate = ASSETS[name]
        p = oscen_amd.resample(a, rate, SR) if rate != SR else a.copy()
        p.setflags(write=False)
        _planes[name] = p
    return _planes[name]


def as_mono(name, channel):
    """the name of the mono, session-rate response (og_register_ir) that holds the conformed source channel `channel`
    (channel "avg": the f32 average in the stated order: channels 0, 1, .. added into 0.0f, times 1.0f / channels)"""
    if name in MONO:
        return name
    derived = "%s_%s" % (name, channel)
    if derived not in _derived:
        p = planes(name)
        if channel == "avg":
            acc = np.zeros(p.shape[0], f32)
            for c in range(p.shape[1]):
                acc = (acc + p[:, c]).astype(f32)
            taps = (acc * (f32(1.0) / f32(p.shape[1]))).astype(f32)
        else:
            taps = p[:, channel]
        oscen_amd.register_ir(derived, taps)
        _derived.append(derived)
    return derived


def source_channel(name, kind, c):
    """from_asset: which conformed source channel bus channel c of a `kind` bus is convolved with"""
    if name in MONO:
        return 0
    src = ASSETS[name][0].shape[1]
    if CHANNELS[kind] == 1 and src > 1:
        return "avg"
    return 0 if src == 1 else min(c, src - 1)


def engine(kind):
    g = mono_graph() if kind == "mono" else oscen_amd.Graph(dsl=wrapper_text(WIDE[kind][0], 8, WIDE[kind][2]))
    eng = oscen_amd.Engine(g, N, sample_rate=float(SR))
    oscen_amd.schedule_note_plans(eng, oscen_amd.note_plans(N, span=TOTAL), total_frames=TOTAL)
    assert eng.channels == CHANNELS[kind]
    return eng


class DeviceBuffer:
    """device memory for the asynchronous entries, through the HIP runtime the library is linked against"""

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


_runs = {}


def render(kind, script, block=BLOCK, mode="blocking"):
    """TOTAL frames of a `kind` bus; script: ((frame, response name), ..) -- set_bus_ir in front of the block that starts at
    `frame`.  Blocks of `block` frames, cut at the swap frames.  mode: "blocking" (process_block), "async" (one
    process_block_async per block under set_bus_batching(8)), "many" (process_blocks_async per run of blocks)."""
    eng = engine(kind)
    ch = eng.channels
    swaps = dict(script)
    edges = sorted(set(swaps) | {0, TOTAL})
    buf = None
    if mode != "blocking":
        eng.set_bus_batching(8)
        buf = DeviceBuffer(TOTAL * ch * 4)
    out = []
    try:
        for f0, f1 in zip(edges[:-1], edges[1:]):
            if f0 in swaps:
                eng.set_bus_ir(swaps[f0])
            f = f0
            if mode == "many":
                assert (f1 - f0) % block == 0
                eng.process_blocks_async(block, (f1 - f0) // block, buf.ptr.value + f0 * ch * 4, block * ch * 4)
                continue
            while f < f1:
                n = min(block, f1 - f)
                if mode == "blocking":
                    out.append(eng.process_block(n).copy())
                else:
                    eng.process_block_async(n, buf.ptr.value + f * ch * 4)
                f += n
        if mode != "blocking":
            eng.flush()
            eng.synchronize()
            return buf.to_host().reshape(TOTAL, ch)
    finally:
        if buf:
            buf.free()
    return np.concatenate(out, axis=0)


def run(kind, script):
    """render(kind, script) in 256-frame blocking blocks: computed once per (bus, script), shared, never modified"""
    key = (kind, tuple(script))
    if key not in _runs:
        got = render(kind, script)
        assert got.shape == (TOTAL, CHANNELS[kind])
        got.setflags(write=False)
        _runs[key] = got
    return _runs[key]


def check_against_mono_runs(kind, script, got=None):
    """channel c of the run under `script` == channel c of the run on the same bus that publishes, at the same frames, the MONO
    responses holding the source channels from_asset maps onto bus channel c"""
    got = run(kind, script) if got is None else got
    assert float(np.abs(got).max()) > 1e-3
    for c in range(CHANNELS[kind]):
        mono_script = tuple((f, as_mono(name, source_channel(name, kind, c))) for f, name in script)
        ref = run(kind, mono_script)
        assert float(np.abs(ref[:, c]).max()) > 1e-3
        assert np.array_equal(got[:, c], ref[:, c]), (kind, script, c)
    return got


# ---- conform ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,taps", [("ira::m44", 327), ("ira::m96", 350), ("ira::m48", 300)])
def test_a_rate_tagged_mono_response_is_conformed_on_publishing(name, taps):
    a, rate = ASSETS[name]
    assert oscen_amd.registered_ir(name) == (a.shape[0], 1, rate)
    eng = engine("mono")
    eng.set_bus_ir(name)
    got = eng.bus_ir()
    want = oscen_amd.resample(a[:, 0], rate, SR)
    assert got.shape == (taps, 1) and want.shape == (taps,)
    assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32))
    if rate == SR:
        assert np.array_equal(want, a[:, 0])
    # the wet bus is that of an engine given register_ir(resample(..)) at the same block
    script = ((BLOCK, name),)
    wet = check_against_mono_runs("mono", script)
    assert not np.any(wet[:BLOCK]) and np.any(wet[BLOCK:])  # Convolver::new() is silent until the response arrives


def test_a_wav_file_is_registered_at_its_rate_and_conformed(tmp_path):
    a, rate = ASSETS["ira::st44"]
    path = str(tmp_path / "hall.wav")
    oscen_amd.write_wav(path, a, sample_rate=rate, bits=32)
    oscen_amd.register_ir_wav("ira::wav", path)
    try:
        assert oscen_amd.registered_ir("ira::wav") == (300, 2, 44100)
        eng = engine("st")
        eng.set_bus_ir("ira::wav")
        assert np.array_equal(eng.bus_ir().view(np.uint32), planes("ira::st44").view(np.uint32))
    finally:
        oscen_amd.unregister_ir("ira::wav")


# ---- per-channel taps and the channel mapping ---------------------------------------------------------------------------------
def info(eng):
    taps, ch = C.c_uint32(), C.c_uint32()
    assert eng.lib.og_bus_ir_info(eng.h, C.byref(taps), C.byref(ch)) == 0
    return taps.value, ch.value


def test_a_stereo_response_convolves_each_channel_with_its_own_taps():
    p = planes("ira::st44")
    assert p.shape == (327, 2) and not np.array_equal(p[:, 0], p[:, 1])
    eng = engine("st")
    eng.set_bus_ir("ira::st44")
    assert info(eng) == (327, 2)
    assert np.array_equal(eng.bus_ir().view(np.uint32), p.view(np.uint32))
    wet = check_against_mono_runs("st", ((BLOCK, "ira::st44"),))
    # ... and the two channels did not get the same taps: channel 1 under channel 0's response is something else
    other = run("st", ((BLOCK, as_mono("ira::st44", 0)),))
    assert not np.array_equal(wet[:, 1], other[:, 1])


MAPPING = [("ira::tri44", "st", [0, 1]),           # more source channels than the bus: the first two
           ("ira::st44", "quad", [0, 1, 1, 1]),     # fewer: channels 2 and 3 take the last source channel
           ("ira::st44", "mono", "avg"),            # a mono bus: the f32 average, channels added in order
           ("ira::tri44", "mono", "avg"),
           ("ira::m44", "st", None)]                # one source channel: ONE plane shared by both bus channels


@pytest.mark.parametrize("name,kind,want", MAPPING, ids=["%s-on-%s" % (n.split("::")[1], k) for n, k, _ in MAPPING])
def test_channel_mapping(name, kind, want):
    p = planes(name)
    eng = engine(kind)
    eng.set_bus_ir(name)
    got = eng.bus_ir()
    if want == "avg":
        acc = np.zeros(p.shape[0], f32)
        for c in range(p.shape[1]):
            acc = (acc + p[:, c]).astype(f32)
        ref = (acc * (f32(1.0) / f32(p.shape[1]))).astype(f32)[:, None]
        assert not np.array_equal(ref[:, 0], p[:, 0])
    elif want is None:
        ref = p
    else:
        ref = p[:, want]
    assert info(eng) == (p.shape[0], ref.shape[1]) and (ref.shape[1] == 1 or ref.shape[1] == CHANNELS[kind])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    for c in range(CHANNELS[kind]):  # og_read_bus_ir by BUS channel: a shared plane answers for every channel
        one = np.zeros(p.shape[0], f32)
        assert eng.lib.og_read_bus_ir(eng.h, c, one.ctypes.data_as(C.POINTER(C.c_float)), len(one)) == 0
        assert np.array_equal(one, ref[:, c if ref.shape[1] > 1 else 0])
    check_against_mono_runs(kind, ((BLOCK, name),))


# ---- swaps ------------------------------------------------------------------------------------------------------------------
SWAPS = ((0, "ira::a"), (2 * BLOCK, "ira::st44"), (5 * BLOCK, "ira::b"))  # mono -> stereo asset -> mono; 960-frame fades


def test_swaps_between_shared_and_per_channel_responses_crossfade_per_channel():
    """the fade that starts at frame 512 spans three block cuts and is cut short by the swap at 1280; the one that starts there
    runs to the end"""
    assert 2 * BLOCK + FADE > 5 * BLOCK
    check_against_mono_runs("st", SWAPS)


def test_a_second_swap_during_a_fade_between_per_channel_responses():
    """stereo (327 taps) at 512, three channels (316 taps) at 768 -- pos = 256 of 960: the first is dropped at once"""
    assert planes("ira::tri44").shape[0] != planes("ira::st44").shape[0]
    check_against_mono_runs("st", ((0, "ira::a"), (2 * BLOCK, "ira::st44"), (3 * BLOCK, "ira::tri44")))
    check_against_mono_runs("st", ((0, "ira::st48"), (2 * BLOCK, "ira::a"), (3 * BLOCK, "ira::st44")))


@pytest.mark.parametrize("mode", ["async", "many"])
def test_a_swap_queued_under_batching_equals_the_blocking_run(mode):
    assert np.array_equal(render("st", SWAPS, mode=mode), run("st", SWAPS))


@pytest.mark.parametrize("block", [100, 7])
def test_block_cuts_do_not_change_a_bit(block):
    assert np.array_equal(render("st", SWAPS, block=block), run("st", SWAPS))


# ---- snapshots --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [("ira::st44", "ira::b"), ("ira::a", "ira::st48")], ids=["stereo-to-mono", "mono-to-stereo"])
def test_snapshot_mid_fade_restores_per_channel_responses(first, second):
    eng = engine("st")
    eng.set_bus_ir(first)
    for _ in range(2):
        eng.process_block(BLOCK)
    eng.set_bus_ir(second)
    eng.process_block(BLOCK)  # pos = 256 of 960
    blob = eng.save_state()
    assert blob.nbytes == eng.state_bytes
    want = np.concatenate([eng.process_block(BLOCK).copy() for _ in range(5)])
    fresh = engine("st")
    fresh.load_state(blob)
    got = np.concatenate([fresh.process_block(BLOCK).copy() for _ in range(5)])
    assert float(np.abs(want).max()) > 1e-3 and not np.array_equal(want[:, 0], want[:, 1])
    assert np.array_equal(got, want)
    k1, k2 = planes(first).shape[0] if first in ASSETS else len(MONO[first]), planes(second).shape[0] if second in ASSETS else len(MONO[second])
    p1, p2 = (2 if first in ASSETS else 1), (2 if second in ASSETS else 1)
    # the section: its 48-byte header, the planes of both responses, max(K) - 1 frames of two-channel history -- behind what
    # the same bank without a Convolver saves at the same frame
    plain = oscen_amd.Engine(oscen_amd.Graph(dsl=wrapper_text(WIDE["st"][0], 8, 2, wet=False)), N, sample_rate=float(SR))
    oscen_amd.schedule_note_plans(plain, oscen_amd.note_plans(N, span=TOTAL), total_frames=TOTAL)
    for _ in range(3):
        plain.process_block(BLOCK)
    assert blob.nbytes - plain.state_bytes == 48 + 4 * (k1 * p1 + k2 * p2 + (max(k1, k2) - 1) * 2)
    with pytest.raises(oscen_amd.OscenError):  # an engine without a Convolver does not take it
        plain.load_state(blob)
    cut = blob[:-4].copy()
    with pytest.raises(oscen_amd.OscenError):
        fresh.load_state(cut)


def test_blobs_without_a_per_channel_response_keep_their_size():
    # a graph without a Convolver: state planes, header (32 bytes), value + ramp per input
    plain = oscen_amd.Engine("sub_voice", N, sample_rate=float(SR))
    assert plain.state_bytes == plain.state_words_per_voice * N * 4 + 32 + 20 * plain.lib.og_num_inputs(plain.h)
    # a Convolver under shared planes only (a one-channel asset included): header, one plane per response, history
    eng = oscen_amd.Engine(oscen_amd.Graph(dsl=wrapper_text(WIDE["st"][0], 8, 2)), N, sample_rate=float(SR))  # (no notes: no events in the blob)
    empty = eng.state_bytes
    eng.set_bus_ir("ira::a")
    eng.process_block(BLOCK)
    eng.set_bus_ir("ira::m44")
    eng.process_block(BLOCK)
    assert eng.state_bytes - empty == 4 * (700 + 327 + 699 * 2)
    blob = eng.save_state()
    assert struct.unpack_from("<I", blob, blob.nbytes - (eng.state_bytes - empty) - 48)[0] == 0x56434E4F  # the section's magic is the old one


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    with pytest.raises(oscen_amd.OscenError, match="og_set_bus_ir") as ei:  # with_ir is the mono, session-rate constructor
        oscen_amd.Engine(mono_graph("ira::st44"), N, sample_rate=float(SR))
    assert ei.value.code == oscen_amd.OG_E_INVALID
    # a conformed length over 2^20: 64 frames at 1 Hz are 3 072 000 taps at 48 000 Hz; the engine keeps what it had
    oscen_amd.register_ir("ira::slow", noise(64, 2, 9), sample_rate=1)
    try:
        eng = engine("st")
        eng.set_bus_ir("ira::st44")
        eng.process_block(BLOCK)
        with pytest.raises(oscen_amd.OscenError, match="3072000 taps") as ei:
            eng.set_bus_ir("ira::slow")
        assert ei.value.code == oscen_amd.OG_E_UNSUPPORTED
        assert np.array_equal(eng.bus_ir(), planes("ira::st44"))
        rest = np.concatenate([eng.process_block(BLOCK).copy() for _ in range(TOTAL // BLOCK - 1)])
        assert np.array_equal(rest, run("st", ((0, "ira::st44"),))[BLOCK:])
    finally:
        oscen_amd.unregister_ir("ira::slow")
    with pytest.raises(oscen_amd.OscenError, match="unknown impulse response"):
        engine("st").set_bus_ir("ira::nowhere")
    # bad WAV files: nothing is registered
    def chunk(tag, data):
        return tag + struct.pack("<I", len(data)) + data

    def wav(bits, data):
        body = b"WAVE" + chunk(b"fmt ", struct.pack("<HHIIHH", 1, 1, 8000, 8000 * bits // 8, bits // 8, bits)) + chunk(b"data", data)
        return b"RIFF" + struct.pack("<I", len(body)) + body

    for fname, image, code in (("u8.wav", wav(8, bytes(8)), oscen_amd.OG_E_UNSUPPORTED), ("cut.wav", wav(16, bytes(16))[:-5], oscen_amd.OG_E_INVALID)):
        (tmp_path / fname).write_bytes(image)
        with pytest.raises(oscen_amd.OscenError) as ei:
            oscen_amd.register_ir_wav("ira::bad", str(tmp_path / fname))
        assert ei.value.code == code, fname
        with pytest.raises(oscen_amd.OscenError):
            oscen_amd.registered_ir("ira::bad")
