"""SamplePlayer inside a voice (csrc/og_sample_player.hip.h): looping playback from the engine's device sample pool, one
buffer choice and one playhead per voice.  `-m gpu`.

Witness: numpy, here -- out[v][t] = buf_v[(t - t_publish_v) mod len_v], zeros while unloaded.  The node copies floats, so
every per-voice comparison is EXACT (np.array_equal); the summed bus is held to the suite's 2e-6 * sum |x_i|.  All banks
have 70 voices: one full wave and a partial one (voices 0, 63, 64, 69 are always among the tapped: every voice is tapped)."""
import ctypes as C

import numpy as np
import pytest

import oscen_amd
from tests import oracle_lib as ol
from tests.test_bench_entry_points_gpu import DeviceBuffer

pytestmark = pytest.mark.gpu
SR = 48000.0
N = 70
BUS_TOL = 2e-6
NONE = oscen_amd.SAMPLE_NONE if hasattr(oscen_amd, "SAMPLE_NONE") else 0xFFFFFFFF


def player_graph(width=1, tag=""):
    ctor = "SamplePlayer::new()" if width == 1 else "SamplePlayer::<Frame<%d>>::new()" % width
    return oscen_amd.Graph(dsl="name: Player%d%s; output out: stream; nodes { player = %s; } connections { player.output -> out; }"
                           % (width, tag, ctor))


def bank(graph=None, taps=True):
    eng = oscen_amd.Engine(graph or player_graph(), N, sample_rate=SR)
    if taps:
        eng.set_voice_taps(list(range(N)))
    return eng


def noise(seed, frames, channels=1):
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, (frames, channels)).astype(np.float32)
    return a[:, 0] if channels == 1 else a


def load(eng, name, data):
    oscen_amd.register_sample(name, data)
    return eng.load_sample(name)


def loop(buf, start, t0, t1):
    """frames t0..t1 of a buffer published at frame `start` ([frames] or [frames, C]); zeros for None / an empty one"""
    if buf is None or len(buf) == 0:
        return None
    return buf[(np.arange(t0, t1) - start) % len(buf)]


def render(eng, blocks, between=None):
    """process the blocks one by one; `between(b)` runs in front of block b.  Returns (taps [N, frames(, C)], bus [frames, ch])"""
    taps, bus = [], []
    for b, frames in enumerate(blocks):
        if between:
            between(b)
        bus.append(eng.process_block(frames).copy())
        taps.append(eng.read_voice_taps(frames).copy())
    return np.concatenate(taps, axis=1), np.concatenate(bus, axis=0)


# ---- 1: silent before load --------------------------------------------------------------------------------------------
def test_an_unloaded_bank_is_exactly_silent():
    eng = bank()
    taps, bus = render(eng, [1, 16, 17, 256])
    assert taps.shape == (N, 290) and not taps.any() and not bus.any()
    assert np.array_equal(eng.read_state_field("player.sample", dtype=np.uint32), np.full(N, NONE, np.uint32))
    assert not eng.read_state_field("player.playhead", dtype=np.uint32).any()
    # an empty registered sample plays as silence too, and its playhead stays at 0
    i = load(eng, "sp_empty", np.zeros(0, np.float32))
    eng.set_sample("player", i)
    taps, bus = render(eng, [33])
    assert not taps.any() and not bus.any()
    assert not eng.read_state_field("player.playhead", dtype=np.uint32).any()


# ---- 2: the reference's known answers ---------------------------------------------------------------------------------
def known_answers(eng, sizes):
    """sample_player/tests.rs + tests/sample_player_graph.rs as one timeline; `sizes(n)` cuts n frames into blocks"""
    f32 = lambda *x: np.array(x, np.float32)  # noqa: E731
    got = []

    def run(n):
        t, _ = render(eng, sizes(n))
        assert all(np.array_equal(t[v], t[0]) for v in range(N))
        got.append(t[0])
        return t[0]

    ia = load(eng, "sp_ka_a", f32(0.1, 0.2, 0.3))
    eng.set_sample("player", ia)
    assert np.array_equal(run(7), f32(0.1, 0.2, 0.3, 0.1, 0.2, 0.3, 0.1))  # plays_buffer_in_order_then_loops
    eng.set_sample("player", load(eng, "sp_ka_b", f32(0.1, 0.2, 0.3, 0.4)))
    assert np.array_equal(run(2), f32(0.1, 0.2))  # swap_resets_playhead
    eng.set_sample("player", load(eng, "sp_ka_c", f32(0.8, 0.9)))
    assert np.array_equal(run(3), f32(0.8, 0.9, 0.8))
    eng.set_sample("player", None)
    assert not run(8).any()  # silent_before_load_then_plays_then_swaps
    a, b = f32(0.1, -0.2, 0.3, -0.4, 0.5), f32(0.9, 0.8, 0.7)
    eng.set_sample("player", load(eng, "sp_ka_A", a))
    assert np.array_equal(run(10), np.tile(a, 2))
    eng.set_sample("player", load(eng, "sp_ka_B", b))
    assert np.array_equal(run(6), np.tile(b, 2))
    return np.concatenate(got)


def test_the_references_known_answers_at_block_size_1_and_as_one_block():
    one = known_answers(bank(), lambda n: [1] * n)
    whole = known_answers(bank(), lambda n: [n])
    assert np.array_equal(one, whole)


# ---- 3: lengths around the chunk ---------------------------------------------------------------------------------------
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 1000]
BLOCKS = [1, 16, 17, 256, 512]
# every length meets a block size that puts a wrap at every position of a 16-frame chunk (a launch restarts the chunk grid):
#   lengths coprime to 16 walk through all positions under any block size; 2, 16 and 32 need a block size that shifts the
#   grid (17, or 1); lengths 1 and 17 run at every block size
PAIRS = [(n, b) for n in (1, 17) for b in BLOCKS] + [(2, 17), (2, 1), (15, 16), (15, 256), (16, 17), (16, 1), (31, 512), (31, 17),
                                                     (32, 17), (32, 256), (33, 16), (33, 512), (1000, 17), (1000, 512)]
TOTAL = 2048


@pytest.fixture(scope="module")
def length_bank():
    eng = bank()
    idx = {n: load(eng, "sp_len_%d" % n, noise(100 + n, n)) for n in LENGTHS}
    return eng, idx


@pytest.mark.parametrize("length,block", PAIRS)
def test_lengths_around_the_chunk(length_bank, length, block):
    eng, idx = length_bank
    buf = noise(100 + length, length)
    eng.set_sample("player", idx[length])
    sizes = [block] * (TOTAL // block) + ([TOTAL % block] if TOTAL % block else [])
    taps, bus = render(eng, sizes)
    want = loop(buf, 0, 0, TOTAL)
    assert np.array_equal(taps, np.broadcast_to(want, (N, TOTAL)))
    ph = eng.read_state_field("player.playhead", dtype=np.uint32)
    assert np.array_equal(ph, np.full(N, TOTAL % length, np.uint32))
    err = np.abs(bus[:, 0].astype(np.float64) - N * want.astype(np.float64))
    bound = BUS_TOL * N * np.abs(want.astype(np.float64))
    print("length %d block %d: max bus error %.3g (bound %.3g)" % (length, block, err.max(), bound.max()))
    assert np.all(err <= bound)


# ---- 4: staggered voices ---------------------------------------------------------------------------------------------
STAG_LENS = [1, 3, 16, 17, 1000]


def staggered(eng, prefix="sp_stag"):
    bufs = [noise(200 + n, n) for n in STAG_LENS]
    idx = [load(eng, "%s_%d" % (prefix, n), b) for n, b in zip(STAG_LENS, bufs)]
    return bufs, idx


def staggered_want(bufs, block, total):
    want = np.zeros((N, total), np.float32)
    for v in range(N):
        start = (v % 4) * block
        want[v, start:] = loop(bufs[v % 5], start, start, total)
    return want


def staggered_publish(eng, idx, b):
    """in front of block b: the voices with v mod 4 == b get sample v mod 5"""
    for v in range(N):
        if v % 4 == b:
            eng.set_voice_samples("player", [idx[v % 5]], first=v)


def test_staggered_voices_hold_their_own_buffers_and_playheads():
    eng = bank()
    bufs, idx = staggered(eng)
    block, blocks = 100, 6  # (100: launches start inside a chunk of the previous one's grid)
    taps, bus = render(eng, [block] * blocks, lambda b: staggered_publish(eng, idx, b))
    want = staggered_want(bufs, block, block * blocks)
    assert np.array_equal(taps, want)
    ph = eng.read_state_field("player.playhead", dtype=np.uint32)
    assert np.array_equal(ph, np.array([(block * blocks - (v % 4) * block) % STAG_LENS[v % 5] for v in range(N)], np.uint32))
    smp = eng.read_state_field("player.sample", dtype=np.uint32)
    assert np.array_equal(smp, np.array([idx[v % 5] for v in range(N)], np.uint32))
    w64 = want.astype(np.float64)
    assert np.all(np.abs(bus[:, 0] - w64.sum(axis=0)) <= BUS_TOL * np.abs(w64).sum(axis=0))


# ---- 5: re-publish ---------------------------------------------------------------------------------------------------
def test_republishing_resets_the_playhead_and_a_sub_range_leaves_the_others_alone():
    eng = bank()
    buf = noise(300, 37)
    i = load(eng, "sp_repub", buf)
    eng.set_sample("player", i)
    t0, _ = render(eng, [50])
    assert np.array_equal(t0, np.broadcast_to(loop(buf, 0, 0, 50), (N, 50)))
    eng.set_voice_samples("player", [i] * 10, first=60)  # voices 60..69: the playing index again (crosses the wave boundary)
    ph = eng.read_state_field("player.playhead", dtype=np.uint32)
    assert np.array_equal(ph, np.array([50 % 37] * 60 + [0] * 10, np.uint32))
    t1, _ = render(eng, [40])
    assert np.array_equal(t1[:60], np.broadcast_to(loop(buf, 0, 50, 90), (60, 40)))
    assert np.array_equal(t1[60:], np.broadcast_to(loop(buf, 50, 50, 90), (10, 40)))
    eng.set_sample("player", i)  # everybody
    t2, _ = render(eng, [20])
    assert np.array_equal(t2, np.broadcast_to(loop(buf, 90, 90, 110), (N, 20)))


# ---- 6: channel mapping ----------------------------------------------------------------------------------------------
def mapped(src, width):
    """SamplePlayerConsumer::build"""
    src = src.reshape(len(src), -1)
    ch = src.shape[1]
    return np.stack([src[:, 0 if ch == 1 else min(c, ch - 1)] for c in range(width)], axis=1)


@pytest.mark.parametrize("src_ch,width", [(2, 2), (1, 2), (2, 1), (3, 2), (2, 4)])
def test_channel_mapping(src_ch, width):
    g = player_graph(width) if width <= 2 else oscen_amd.Graph(
        dsl="name: Player4; output a: stream; output b: stream; nodes { player = SamplePlayer::<Frame<4>>::new(); } "
            "connections { Frame(player.output[0], player.output[1]) -> a; Frame(player.output[2], player.output[3]) -> b; }")
    eng = bank(g)
    src = noise(400 + 10 * src_ch + width, 21, src_ch)
    eng.set_sample("player", load(eng, "sp_map_%d_%d" % (src_ch, width), src))
    taps, bus = render(eng, [1, 16, 40])
    want = loop(mapped(src, width), 0, 0, 57)
    if width == 1:
        want = want[:, 0]
    assert taps.shape == (N,) + want.shape
    assert np.array_equal(taps, np.broadcast_to(want, taps.shape))
    if (src_ch, width) == (2, 4):
        assert np.array_equal(taps[0, :, 1], taps[0, :, 2]) and np.array_equal(taps[0, :, 1], taps[0, :, 3])  # [L, R, R, R]
        assert not np.array_equal(taps[0, :, 0], taps[0, :, 1])


def test_the_stereo_graph_answer():
    """tests/stereo_sample_player_graph.rs: silent, then each channel reproduced over two loops"""
    eng = bank(player_graph(2))
    before, _ = render(eng, [8])
    assert before.shape == (N, 8, 2) and not before.any()
    left, right = np.array([0.1, -0.2, 0.3, -0.4], np.float32), np.array([-0.1, 0.2, -0.3, 0.4], np.float32)
    eng.set_sample("player", load(eng, "sp_stereo_answer", np.stack([left, right], axis=1)))
    out, _ = render(eng, [1] * 8)
    want = np.stack([np.tile(left, 2), np.tile(right, 2)], axis=1)
    assert np.array_equal(out, np.broadcast_to(want, (N, 8, 2)))


# ---- 7: cutting ------------------------------------------------------------------------------------------------------
def test_the_same_frames_cut_five_ways_are_bit_identical():
    """case 4's voices at block 512 (publishes in front of frames 0, 512, 1024, 1536), rendered five ways.  A publish launches
    what is queued, so the cuts differ in how the 512 frames BETWEEN two publishes are processed.  The three block-by-block cuts
    compare every tap of every frame.  A launch that covers several blocks keeps the taps of no block but its last (and a
    tapped engine launches block by block), so the two queued forms run UNTAPPED -- one launch over 32 blocks -- and are
    compared through everything they leave behind: both state words of every voice after every span, the bus of every
    frame, and the taps of the 64 frames that follow, against the block-by-block engine and the witness."""
    span, spans = 512, 4

    def run(cut):
        eng = bank()
        bufs, idx = staggered(eng, "sp_cut")
        taps = []
        for b in range(spans):
            staggered_publish(eng, idx, b)
            taps.append(cut(eng))
        return bufs, np.concatenate(taps, axis=1)

    def blocks(size):
        return lambda eng: render(eng, [size] * (span // size))[0]

    bufs, a = run(blocks(256))
    want = staggered_want(bufs, span, span * spans)
    assert np.array_equal(a, want)
    for size in (512, 16):
        assert np.array_equal(run(blocks(size))[1], a), size
    # the two queued forms keep taps of the last block only: compare what they leave behind -- every voice's state words
    # after each span and the bus -- with the block-by-block engine
    for cut in ("render under set_bus_batching(32)", "og_process_blocks_async"):
        ref, eng = bank(), bank(taps=False)
        _, ridx = staggered(ref, "sp_cut")
        _, eidx = staggered(eng, "sp_cut")
        assert ridx == eidx
        for b in range(spans):
            staggered_publish(ref, ridx, b)
            staggered_publish(eng, eidx, b)
            ref_bus = render(ref, [16] * (span // 16))[1]
            if cut.startswith("render"):
                eng.set_bus_batching(32)
                got_bus = eng.render(span, block=16)
                eng.set_bus_batching(1)
            else:
                buf = DeviceBuffer(span * 4)
                try:
                    eng.set_bus_batching(32)
                    eng.process_blocks_async(16, span // 16, buf.ptr.value, 16 * 4)
                    eng.synchronize()
                    eng.set_bus_batching(1)
                    got_bus = buf.to_host().reshape(span, 1)
                finally:
                    buf.free()
            w64 = want[:, b * span:(b + 1) * span].astype(np.float64)
            assert np.all(np.abs(got_bus[:, 0] - w64.sum(axis=0)) <= BUS_TOL * np.abs(w64).sum(axis=0))
            assert np.all(np.abs(ref_bus[:, 0] - w64.sum(axis=0)) <= BUS_TOL * np.abs(w64).sum(axis=0))
            for field in ("player.playhead", "player.sample"):
                assert np.array_equal(eng.read_state_field(field, dtype=np.uint32), ref.read_state_field(field, dtype=np.uint32)), (cut, b, field)
        # ... and the taps of the frames that follow are the witness's: the queued launches left every voice where it belongs
        eng.set_voice_taps(list(range(N)))
        tail = render(eng, [64])[0]
        total = span * spans
        more = np.stack([loop(bufs[v % 5], (v % 4) * span, total, total + 64) for v in range(N)])
        assert np.array_equal(tail, more), cut


# ---- 8: a sampler voice ----------------------------------------------------------------------------------------------
ADSR_CTOR = (0.004, 0.01, 0.5, 0.02)
SAMPLER = """
name: Sampler;
input gate: event;
output out: stream;
nodes { player = SamplePlayer::new(); env = AdsrEnvelope::new(%r, %r, %r, %r); }
connections { gate -> env.gate; player.output * env.output -> out; }
""" % ADSR_CTOR


def adsr_levels(events, frames):
    lib = ol.load()
    out = np.zeros((N, frames), np.float32)
    for v in range(N):
        e = ol.Adsr()
        lib.oo_adsr_new(C.byref(e), *ADSR_CTOR)
        e.sample_rate = SR
        lib.oo_adsr_prepare(C.byref(e))
        evs = {}
        for f, val in events[v]:
            evs.setdefault(f, []).append(val)
        for i in range(frames):
            for val in evs.get(i, ()):
                lib.oo_adsr_handle_gate_event(C.byref(e), C.byref(ol.Event(0, val, 0)))
            lib.oo_adsr_process(C.byref(e))
            out[v, i] = e.output
    return out


@pytest.fixture(scope="module")
def sampler_case():
    frames = 1536
    events = {v: [(3 + v % 7, 0.9), (500 + 5 * v, 0.0)] + ([(1100, 0.6)] if v % 3 == 0 else []) for v in range(N)}
    buf = noise(500, 777)
    env = adsr_levels(events, frames).astype(np.float64)
    return frames, events, buf, env


@pytest.mark.parametrize("split", [0, 2, 4])
def test_a_sampler_voice_under_every_kernel_shape_the_knobs_can_force(monkeypatch, sampler_case, split):
    frames, events, buf, env = sampler_case
    monkeypatch.setenv("OSCEN_GPU_SPLIT", str(split))
    eng = bank(oscen_amd.Graph(dsl=SAMPLER))
    assert eng.pipeline_depth in (0, 1)  # (a graph with a SamplePlayer has the ordinary kernel only, as one with a Delay)
    eng.set_sample("player", load(eng, "sp_sampler", buf))
    vs, fs, xs = zip(*[(v, f, x) for v, l in events.items() for f, x in l])
    eng.schedule_voice_events("gate", vs, fs, xs)
    taps, _ = render(eng, [256] * (frames // 256))
    want = loop(buf, 0, 0, frames).astype(np.float64)[None, :] * env
    err = float(np.max(np.abs(taps.astype(np.float64) - want)))
    print("sampler voice, OSCEN_GPU_SPLIT=%d: max |out - player * oracle envelope| = %.3g" % (split, err))
    assert err <= 1e-5


# ---- 9: grouping -----------------------------------------------------------------------------------------------------
def test_grouped_voices_publish_and_read_by_logical_voice():
    eng = oscen_amd.Engine(oscen_amd.Graph(dsl=SAMPLER), N, sample_rate=SR)
    bufs, idx = staggered(eng, "sp_grp")
    # note-offs in reverse voice order: policy 1 re-orders the slots
    events = {v: [(0, 1.0), (1000 - 10 * v, 0.0)] for v in range(N)}
    vs, fs, xs = zip(*[(v, f, x) for v, l in events.items() for f, x in l])
    eng.schedule_voice_events("gate", vs, fs, xs)
    eng.group_voices(1)
    assert any(eng.voice_slot(v) != v for v in range(N))
    eng.set_voice_taps(list(range(N)))
    eng.set_voice_samples("player", [idx[v % 5] for v in range(N)])
    eng.set_voice_samples("player", [idx[4]] * 3, first=62)  # a few voices, across the wave boundary
    chosen = [4 if 62 <= v < 65 else v % 5 for v in range(N)]
    assert np.array_equal(eng.read_state_field("player.sample", dtype=np.uint32), np.array([idx[c] for c in chosen], np.uint32))
    taps, _ = render(eng, [48])
    ph = eng.read_state_field("player.playhead", dtype=np.uint32)
    assert np.array_equal(ph, np.array([48 % STAG_LENS[c] for c in chosen], np.uint32))
    env = adsr_levels(events, 48).astype(np.float64)
    want = np.stack([loop(bufs[c], 0, 0, 48) for c in chosen]).astype(np.float64) * env
    assert float(np.max(np.abs(taps - want))) <= 1e-5
    eng.set_voice_samples("player", [None], first=69)
    taps, _ = render(eng, [16])
    assert not taps[69].any() and taps[68].any()


# ---- 10: snapshot ----------------------------------------------------------------------------------------------------
def test_a_snapshot_in_mid_loop_continues_bit_for_bit_and_needs_its_samples():
    eng = bank()
    bufs, idx = staggered(eng, "sp_snap")
    render(eng, [100] * 4, lambda b: staggered_publish(eng, idx, b))
    assert eng.read_state_field("player.playhead", dtype=np.uint32).any()
    blob = eng.save_state()
    assert len(blob) == eng.state_bytes
    fresh = bank()
    fresh.load_state(blob)  # resolves the names through the registry and loads the samples in index order
    assert [fresh.load_sample("sp_snap_%d" % n) for n in STAG_LENS] == idx
    a, bus_a = render(eng, [100, 33])
    b, bus_b = render(fresh, [100, 33])
    assert np.array_equal(a, b) and np.array_equal(bus_a, bus_b)
    assert np.array_equal(a, np.stack([loop(bufs[v % 5], (v % 4) * 100, 400, 533) for v in range(N)]))
    oscen_amd.unregister_sample("sp_snap_17")
    try:
        with pytest.raises(oscen_amd.OscenError) as ei:
            bank().load_state(blob)
        assert ei.value.code == -1 and "sp_snap_17" in str(ei.value)  # OG_E_INVALID
        oscen_amd.register_sample("sp_snap_17", noise(1, 18))  # another shape
        with pytest.raises(oscen_amd.OscenError) as ei:
            bank().load_state(blob)
        assert ei.value.code == -1
    finally:
        oscen_amd.register_sample("sp_snap_17", bufs[3])


# ---- argument validation on an engine (tests/test_sample_player_cpu.py has what needs none) -------------------------------
def test_engine_entry_points_refuse_bad_arguments():
    lib = oscen_amd.load_library()
    eng = bank(taps=False)
    u32p = C.POINTER(C.c_uint32)
    out = C.c_uint32(7)
    one = (C.c_uint32 * 2)(0, 0)
    oscen_amd.register_sample("sp_args", noise(7, 9))
    assert lib.og_load_sample(eng.h, None, C.byref(out)) == -1 and lib.og_load_sample(eng.h, b"sp_args", None) == -1
    assert lib.og_load_sample(eng.h, b"sp_never_registered", C.byref(out)) == -1 and b"sp_never_registered" in lib.og_last_error()
    i = eng.load_sample("sp_args")
    assert eng.load_sample("sp_args") == i  # idempotent per name
    assert lib.og_set_sample(eng.h, None, i) == -1 and lib.og_set_voice_samples(eng.h, b"player", 0, 1, None) == -1
    assert lib.og_set_sample(eng.h, b"nobody", i) == -1 and b"no SamplePlayer named 'nobody'" in lib.og_last_error()
    assert lib.og_set_sample(eng.h, b"player", i + 1) == -1 and b"og_load_sample" in lib.og_last_error()  # unknown index
    assert lib.og_set_voice_samples(eng.h, b"player", N - 1, 2, C.cast(one, u32p)) == -1 and b"voice range out of bounds" in lib.og_last_error()
    assert lib.og_set_voice_samples(eng.h, b"player", N, 0, None) == 0  # an empty range at the end is legal
    assert not eng.read_state_field("player.playhead", dtype=np.uint32).any()  # nothing was published by the refused calls
    assert np.array_equal(eng.read_state_field("player.sample", dtype=np.uint32), np.full(N, NONE, np.uint32))
    plain = oscen_amd.Engine("sub_voice", N, sample_rate=SR)  # a graph without a player
    assert lib.og_load_sample(plain.h, b"sp_args", C.byref(out)) == -1 and b"no SamplePlayer" in lib.og_last_error()
    assert lib.og_set_sample(plain.h, b"player", 0) == -1


# ---- 11: cluster -----------------------------------------------------------------------------------------------------
def test_a_two_shard_cluster_equals_the_single_engine():
    n_dev = C.c_int(0)  # (asked of the runtime the loaded library is linked against: the host simulator's, on the simulator)
    if oscen_amd.load_library().hipGetDeviceCount(C.byref(n_dev)) != 0 or n_dev.value < 2:
        pytest.skip("needs two visible devices")
    g = player_graph()
    single = bank(g)
    bufs, idx = staggered(single, "sp_clu")
    cl = oscen_amd.Cluster(g, N, [0, 1], sample_rate=SR)
    cidx = [cl.load_sample("sp_clu_%d" % n) for n in STAG_LENS]
    assert cidx == idx
    shards = [cl.shard(s) for s in range(2)]
    for e in shards:
        e.set_voice_taps(list(range(e.n_voices)))
    block, blocks = 100, 6
    want = staggered_want(bufs, block, block * blocks)
    for b in range(blocks):
        staggered_publish(single, idx, b)
        for v in range(N):
            if v % 4 == b:
                cl.set_voice_samples("player", [cidx[v % 5]], first=v)
        bus_s = single.process_block(block)
        bus_c = cl.process_block(block)
        taps_c = np.concatenate([e.read_voice_taps(block) for e in shards], axis=0)
        assert np.array_equal(taps_c, single.read_voice_taps(block))
        assert np.array_equal(taps_c, want[:, b * block:(b + 1) * block])
        w64 = want[:, b * block:(b + 1) * block].astype(np.float64)
        for bus in (bus_s, bus_c):
            assert np.all(np.abs(bus[:, 0] - w64.sum(axis=0)) <= BUS_TOL * np.abs(w64).sum(axis=0))
    ph = np.concatenate([e.read_state_field("player.playhead", dtype=np.uint32) for e in shards])
    assert np.array_equal(ph, single.read_state_field("player.playhead", dtype=np.uint32))
    cl.set_sample("player", None)
    assert not cl.process_block(32).any()
