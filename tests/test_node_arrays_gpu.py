"""Per-voice ARRAY fields of custom nodes (og_node_array, csrc/og_node_array.hip.h) on the device: delay lines, histories
and tables a registered node type keeps per voice.  The witnesses are numpy float32 models written here; the nodes' arithmetic
(tests/node_array_nodes.py) is adds of two f32 and multiplies by a power of two, so every comparison of per-voice samples is
np.array_equal.  V = 70: one full wave and a partial one of 6 lanes."""
import ctypes as C

import numpy as np
import pytest

import oscen_amd
from tests import node_array_nodes as nn

pytestmark = pytest.mark.gpu
SR = 48000.0
V = 70
FRAMES = 1536
f32 = np.float32
DELAYS = (0, 1, 63, 64, 1022)


@pytest.fixture(scope="module", autouse=True)
def _nodes():
    nn.register_all()
    yield
    for name in nn.ALL:
        oscen_amd.unregister_node(name)


def freqs(n):
    return np.linspace(55.0, 1760.0, n).astype(f32)


def delays(n):
    return np.array([DELAYS[v % len(DELAYS)] for v in range(n)], dtype=f32)


def engine(g, n=V, delay=None, group=False):
    eng = oscen_amd.Engine(g, n, sample_rate=SR)
    eng.set_voice_values("frequency", freqs(n))
    if delay is not None:
        eng.set_voice_values("delay", delay)
    if group:
        eng.group_voices(1)
    eng.set_voice_taps(np.arange(n, dtype=np.uint32))
    return eng


def run(eng, cuts):
    """process_block over `cuts`; the taps of all voices, [voice][frame]"""
    out = []
    for c in cuts:
        eng.process_block(c)
        out.append(eng.read_voice_taps(c))
    return np.concatenate(out, axis=1)


_source = {}


def source(n=V, frames=FRAMES):
    """the oscillator's samples, [voice][frame]: computed once per shape, never changed"""
    if (n, frames) not in _source:
        x = run(engine(nn.source_graph(), n), [512] * (frames // 512) + ([frames % 512] if frames % 512 else []))
        assert np.abs(x).max() > 0.1
        x.setflags(write=False)
        _source[(n, frames)] = x
    return _source[(n, frames)]


def comb_model(x, delay, line=None, wp=None):
    """UComb over x[voice][frame] -> (output, line, write positions)"""
    n, frames = x.shape
    line = np.zeros((n, nn.N_LINE), dtype=f32) if line is None else line.copy()
    wp = np.zeros(n, dtype=np.int64) if wp is None else wp.copy()
    dl = np.asarray(delay, dtype=np.int64)
    rows = np.arange(n)
    out = np.zeros((n, frames), dtype=f32)
    for f in range(frames):
        d = line[rows, (wp + 1024 - dl - 1) & 1023]
        line[rows, wp] = x[:, f] + d * f32(0.5)
        wp = (wp + 1) & 1023
        out[:, f] = d
    return out, line, wp


# ---- 1. the comb ---------------------------------------------------------------------------------------------------------------
def test_comb_matches_the_model_over_a_wrapping_line():
    eng = engine(nn.comb_graph(), delay=delays(V))
    assert eng.lib.og_kernel_is_jit(eng.h) == 1 and eng.lib.og_uses_split_kernel(eng.h) == 0
    got = run(eng, [512, 512, 512])
    want, line, wp = comb_model(source(), delays(V))
    assert np.array_equal(got, want) and np.abs(want).max() > 0.1
    assert np.array_equal(eng.read_node_array("comb.buf"), line)
    assert np.array_equal(eng.read_state_field("comb.wp", dtype=np.uint32), wp.astype(np.uint32))


# ---- 2. the twin of the built-in Delay -----------------------------------------------------------------------------------------
def test_comb_is_the_bit_equal_twin_of_the_builtin_delay():
    got = run(engine(nn.comb_graph(delay_arg=100)), [512, 512, 512])
    twin = run(engine(nn.delay_twin_graph(100)), [512, 512, 512])
    assert np.array_equal(got, twin) and np.abs(twin).max() > 0.1


# ---- 3. block cuts --------------------------------------------------------------------------------------------------------------
def test_block_cuts_and_queued_launches_leave_samples_and_lines_bit_identical():
    """(a block of this engine is at most 512 frames: the 1536 frames in one piece are three 512-frame blocks in ONE launch)"""
    want, line, wp = comb_model(source(), delays(V))
    for cuts in ([512] * 3, [256] * 6, [37] * (FRAMES // 37) + [FRAMES % 37]):
        eng = engine(nn.comb_graph(), delay=delays(V))
        assert np.array_equal(run(eng, cuts), want), cuts[0]
        assert np.array_equal(eng.read_node_array("comb.buf"), line), cuts[0]
    # one launch over all 1536 frames (no taps while blocks are queued: the lines and the write positions are the witnesses)
    eng = engine(nn.comb_graph(), delay=delays(V))
    eng.set_voice_taps(np.zeros(0, dtype=np.uint32))
    eng.set_bus_batching(4)
    eng.process_blocks_async(512, 3)
    assert np.array_equal(eng.read_node_array("comb.buf"), line)
    assert np.array_equal(eng.read_state_field("comb.wp", dtype=np.uint32), wp.astype(np.uint32))
    # render(): 256-frame blocks queued four to a launch
    eng = engine(nn.comb_graph(), delay=delays(V))
    eng.set_voice_taps(np.zeros(0, dtype=np.uint32))
    eng.set_bus_batching(4)
    bus = eng.render(FRAMES, 256)
    assert np.array_equal(eng.read_node_array("comb.buf"), line)
    w64 = want.astype(np.float64)
    assert np.all(np.abs(bus[:, 0] - w64.sum(axis=0)) <= 2e-6 * np.abs(w64).sum(axis=0) + 1e-30)
    # ... and the last block of a queue with its taps
    eng = engine(nn.comb_graph(), delay=delays(V))
    eng.set_bus_batching(4)
    eng.process_blocks_async(256, 5)
    assert np.array_equal(run(eng, [256]), want[:, 1280:]) and np.array_equal(eng.read_node_array("comb.buf"), line)


# ---- 4. lengths and element types ------------------------------------------------------------------------------------------------
def test_lengths_one_and_five_a_u32_array_and_read_after_write_in_one_tick():
    frames = 300
    eng = engine(nn.one_node_graph("narr_multi", "UMulti::new()"))
    assert eng.node_array_info("n.one") == (1, "f32") and eng.node_array_info("n.five") == (5, "f32") and eng.node_array_info("n.cnt") == (3, "u32")
    assert np.array_equal(eng.read_node_array("n.one"), np.full((V, 1), 0.25, f32))
    assert np.array_equal(eng.read_node_array("n.cnt"), np.full((V, 3), 7, np.uint32))
    got = run(eng, [256, 44])
    x = source()[:, :frames]
    five = np.full((V, 5), 1.5, dtype=f32)
    cnt = np.full((V, 3), 7, dtype=np.uint32)
    one = np.zeros((V, 1), dtype=f32)
    want = np.zeros((V, frames), dtype=f32)
    for f in range(frames):
        t0 = five[:, 0].copy()
        five[:, :4] = five[:, 1:].copy()
        five[:, 4] = t0 + x[:, f]
        cnt[:, f % 3] += 1
        one[:, 0] = x[:, f] * f32(2.0)
        want[:, f] = one[:, 0] + five[:, 0]
    assert np.array_equal(got, want)
    assert np.array_equal(eng.read_node_array("n.one"), one) and np.array_equal(eng.read_node_array("n.five"), five)
    assert np.array_equal(eng.read_node_array("n.cnt"), cnt)


# ---- 5. the clamp ----------------------------------------------------------------------------------------------------------------
def test_an_index_past_the_end_is_clamped_to_the_last_element_and_leaves_the_neighbours_alone():
    frames = 64
    eng = engine(nn.one_node_graph("narr_clamp", "UClamp::new()"))
    got = run(eng, [frames])
    x = source()[:, :frames]
    assert np.array_equal(got, x)  # get(0xFFFFFFFF) reads what set(length + 3, x) wrote: both are element length - 1
    mid = np.full((V, 4), 1.0, dtype=f32)
    mid[:, 3] = x[:, frames - 1]
    assert np.array_equal(eng.read_node_array("n.mid"), mid)
    assert np.array_equal(eng.read_node_array("n.below"), np.full((V, 2), 3.0, f32))
    assert np.array_equal(eng.read_node_array("n.above"), np.full((V, 4), 2.0, f32))
    ids = np.full((V, 3), 5, dtype=np.uint32)
    ids[:, 2] += frames
    assert np.array_equal(eng.read_node_array("n.ids"), ids)


# ---- 6. instances ----------------------------------------------------------------------------------------------------------------
def test_every_instance_and_every_element_of_a_node_array_has_its_own_line():
    n = 130  # three waves
    eng = engine(nn.instances_graph(), n)
    got = run(eng, [512, 512, 512])
    x = source(n)
    names = ["combs[0]", "combs[1]", "combs[2]", "first", "second"]
    acc = None
    for name in names:
        out, line, _ = comb_model(x, np.full(n, nn.INSTANCE_DELAYS[name]))
        assert np.array_equal(eng.read_node_array(name + ".buf"), line), name
        acc = out if acc is None else (acc + out).astype(f32)
    assert np.array_equal(got, acc)


# ---- 7. handler access -----------------------------------------------------------------------------------------------------------
def test_a_gate_handler_clears_the_line_and_writes_a_burst():
    eng = engine(nn.one_node_graph("narr_burst", "UBurst::new()", feeds_input=False, gate=True))
    when = {0: [(0, 0.75)], 1: [(255, 0.5)], 2: [(100, 1.0), (300, 0.25)], 64: [(0, 0.5), (255, 1.0)], 69: [(400, 0.75)]}
    for v, evs in when.items():
        for frame, vel in evs:
            eng.schedule_voice_event("gate", v, frame, vel)
    got = run(eng, [256, 256])
    want = np.zeros((V, 512), dtype=f32)
    for v in range(V):
        line, wp = np.zeros(64, dtype=f32), 0
        evs = dict(when.get(v, []))
        for f in range(512):
            if f in evs:
                line[:] = 0
                line[0], line[1], line[2], wp = f32(evs[f]), f32(evs[f]) * f32(0.5), f32(evs[f]) * f32(0.25), 0
            want[v, f] = line[wp]
            line[wp] = want[v, f] * f32(0.5)
            wp = (wp + 1) & 63
    assert np.array_equal(got, want) and np.count_nonzero(want) > 20


# ---- 8. oversampled --------------------------------------------------------------------------------------------------------------
def test_an_oversampled_comb_ticks_twice_per_frame():
    a = engine(nn.comb_graph(delay_arg=0, factor=2))
    got = run(a, [256, 256])
    want = run(engine(nn.comb0_scalar_graph(2)), [256, 256])
    assert np.array_equal(got, want) and np.abs(want).max() > 0.1
    assert np.array_equal(a.read_state_field("comb.wp", dtype=np.uint32), np.full(V, 1024 % 1024, np.uint32))  # 2 x 512 ticks


# ---- 9. og_init -------------------------------------------------------------------------------------------------------------------
def test_init_resets_the_arrays():
    eng = engine(nn.comb_graph(), delay=delays(V))
    first = run(eng, [300])
    assert np.abs(eng.read_node_array("comb.buf")).max() > 0
    eng.init(SR)
    assert np.array_equal(eng.read_node_array("comb.buf"), np.zeros((V, nn.N_LINE), f32))
    eng.set_voice_values("frequency", freqs(V))
    eng.set_voice_values("delay", delays(V))
    eng.set_voice_taps(np.arange(V, dtype=np.uint32))
    assert np.array_equal(run(eng, [300]), first)
    multi = engine(nn.one_node_graph("narr_multi", "UMulti::new()"))
    run(multi, [10])
    multi.init(SR)
    assert np.array_equal(multi.read_node_array("n.five"), np.full((V, 5), 1.5, f32)) and np.array_equal(multi.read_node_array("n.cnt"), np.full((V, 3), 7, np.uint32))


# ---- 10. write --------------------------------------------------------------------------------------------------------------------
def test_write_gives_every_voice_its_own_table_and_lands_behind_queued_blocks():
    eng = engine(nn.one_node_graph("narr_table", "UTable::new()", feeds_input=False))
    tables = (np.arange(V * 64, dtype=f32).reshape(V, 64) * f32(0.25)).astype(f32)
    eng.write_node_array("n.table", tables)
    assert np.array_equal(eng.read_node_array("n.table"), tables)
    got = run(eng, [100])
    assert np.array_equal(got, tables[:, np.arange(100) & 63])
    # a range of voices, others untouched
    eng.write_node_array("n.table", -tables[64:67], first=64)
    tables2 = tables.copy()
    tables2[64:67] = -tables[64:67]
    assert np.array_equal(eng.read_node_array("n.table", first=60, n=10), tables2[60:70])
    # between two queued blocks and the next: the queued ones play the old tables
    eng.set_bus_batching(4)
    eng.set_voice_taps(np.zeros(0, dtype=np.uint32))
    eng.process_blocks_async(28, 1)  # phase 100 .. 127
    eng.write_node_array("n.table", np.zeros((V, 64), f32))
    assert np.array_equal(eng.read_state_field("n.ph", dtype=np.uint32), np.full(V, 128, np.uint32))
    eng.set_voice_taps(np.arange(V, dtype=np.uint32))
    assert np.array_equal(run(eng, [64]), np.zeros((V, 64), f32))


def test_a_write_between_queued_blocks_takes_effect_after_them():
    """the node sums what it plays (small integers: exact): queued blocks that played the new table early would show in the sum"""
    eng = engine(nn.one_node_graph("narr_table", "UTable::new()", feeds_input=False), 3)
    eng.set_voice_taps(np.zeros(0, dtype=np.uint32))
    eng.set_bus_batching(4)
    ramp = np.tile(np.arange(64, dtype=f32), (3, 1))
    eng.write_node_array("n.table", ramp)
    eng.process_blocks_async(64, 2)  # queued, not launched
    eng.write_node_array("n.table", ramp * f32(2.0))
    assert np.array_equal(eng.read_state_field("n.acc"), np.full(3, 2 * 2016.0, f32))
    bus = eng.process_block(64)
    assert np.array_equal(bus[:, 0], (ramp[0] * f32(2.0)) * f32(3.0))
    assert np.array_equal(eng.read_state_field("n.acc"), np.full(3, 4 * 2016.0, f32))


# ---- 11. snapshots -----------------------------------------------------------------------------------------------------------------
def test_snapshots_carry_the_pool_and_refuse_another_layout():
    eng = engine(nn.comb_graph(), delay=delays(V))
    run(eng, [300])
    blob = eng.save_state()
    assert blob.nbytes == eng.state_bytes
    want = run(eng, [400])
    fresh = engine(nn.comb_graph())
    fresh.load_state(blob)
    assert np.array_equal(run(fresh, [400]), want)
    assert np.array_equal(fresh.read_node_array("comb.buf"), eng.read_node_array("comb.buf"))
    # the section: a head of 2 + n_fields words, then the pool
    words = eng.state_words_per_voice * V * 4 + 32 + 20 * eng.lib.og_num_inputs(eng.h)
    assert eng.state_bytes == words + (2 + 1) * 4 + nn.N_LINE * V * 4
    # graphs without array fields: byte for byte what they were
    plain = oscen_amd.Engine("sub_voice", V, sample_rate=SR)
    assert plain.state_bytes == plain.state_words_per_voice * V * 4 + 32 + 20 * plain.lib.og_num_inputs(plain.h)
    # another array length: refused, the engine untouched
    short = dict(nn.COMB, arrays=[("buf", 512, "f32", 0.0)])
    nn.register("UCombShort::new", short)
    try:
        g = nn.graph("narr_comb", "    comb = UCombShort::new(0.0);\n", "    osc.output -> comb.input;\n    delay -> comb.delay;\n    comb.output -> out;\n")
        other = engine(g, delay=delays(V))
        run(other, [50])
        before = other.read_node_array("comb.buf")
        with pytest.raises(oscen_amd.OscenError) as ei:
            other.load_state(blob)
        assert ei.value.code == oscen_amd.OG_E_INVALID and "node-array" in str(ei.value)
        assert np.array_equal(other.read_node_array("comb.buf"), before) and other.frames_processed == 50
        with pytest.raises(oscen_amd.OscenError):
            fresh.load_state(other.save_state())
    finally:
        oscen_amd.unregister_node("UCombShort::new")


# ---- 12. grouping -------------------------------------------------------------------------------------------------------------------
def test_grouped_voices_read_and_write_by_the_callers_numbers():
    rows = (np.arange(2 * nn.N_LINE, dtype=f32).reshape(2, nn.N_LINE) * f32(0.5)).astype(f32)

    def make(group, prewrite=False):
        eng = oscen_amd.Engine(nn.comb_graph(), V, sample_rate=SR)
        eng.set_voice_values("frequency", freqs(V))
        eng.set_voice_values("delay", delays(V))
        if prewrite:  # written BEFORE the slots are re-ordered: the columns move with their voices
            eng.write_node_array("comb.buf", rows, first=7)
        for v in range(V):  # note-offs in reverse voice order: policy 1 reverses the slots
            eng.schedule_voice_event("gate", v, 2000 - 3 * v, 0.0)
        if group:
            eng.group_voices(1)
            assert eng.voice_slot(0) != 0
        eng.set_voice_taps(np.arange(V, dtype=np.uint32))
        return eng
    a, b = make(False), make(True)
    ta, tb = run(a, [512]), run(b, [512])
    assert np.array_equal(ta, tb) and np.array_equal(a.read_node_array("comb.buf"), b.read_node_array("comb.buf"))
    assert np.array_equal(b.read_node_array("comb.buf", first=5, n=3), a.read_node_array("comb.buf")[5:8])
    for e in (a, b):
        e.write_node_array("comb.buf", rows, first=7)
    assert np.array_equal(b.read_node_array("comb.buf"), a.read_node_array("comb.buf")) and np.array_equal(b.read_node_array("comb.buf")[7:9], rows)
    assert np.array_equal(run(a, [100]), run(b, [100]))
    c, d = make(False, prewrite=True), make(True, prewrite=True)
    assert np.array_equal(d.read_node_array("comb.buf")[7:9], rows) and np.count_nonzero(d.read_node_array("comb.buf")) == np.count_nonzero(rows)
    assert np.array_equal(run(c, [100]), run(d, [100])) and np.array_equal(c.read_node_array("comb.buf"), d.read_node_array("comb.buf"))


# ---- 13. bad arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_to_the_entry_points():
    eng = engine(nn.comb_graph())
    lib, INVALID = eng.lib, oscen_amd.OG_E_INVALID
    length, is_uint = C.c_uint32(), C.c_int()
    buf = np.zeros((2, nn.N_LINE), f32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.og_node_array_info(None, b"comb.buf", C.byref(length), C.byref(is_uint)) == INVALID
    assert lib.og_node_array_info(eng.h, None, C.byref(length), C.byref(is_uint)) == INVALID
    assert lib.og_node_array_info(eng.h, b"comb.nothing", C.byref(length), C.byref(is_uint)) == INVALID and b"no array field" in lib.og_last_error()
    assert lib.og_node_array_info(eng.h, b"comb.wp", None, None) == INVALID  # a scalar field is not an array
    assert lib.og_node_array_info(eng.h, b"comb.buf", None, None) == 0
    for fn in (lib.og_read_node_array, lib.og_write_node_array):
        assert fn(None, b"comb.buf", 0, 1, p) == INVALID and fn(eng.h, None, 0, 1, p) == INVALID and fn(eng.h, b"comb.buf", 0, 1, None) == INVALID
        assert fn(eng.h, b"osc.buf", 0, 1, p) == INVALID
        assert fn(eng.h, b"comb.buf", V - 1, 2, p) == INVALID and b"voice range out of bounds" in lib.og_last_error()
        assert fn(eng.h, b"comb.buf", V, 1, p) == INVALID and fn(eng.h, b"comb.buf", 0xFFFFFFFF, 2, p) == INVALID
        assert fn(eng.h, b"comb.buf", V, 0, None) == 0  # an empty range at the end is legal
    with pytest.raises(ValueError):
        eng.write_node_array("comb.buf", np.zeros((1, 5), f32))
    plain = oscen_amd.Engine("sub_voice", 4, sample_rate=SR)
    assert lib.og_read_node_array(plain.h, b"osc.buf", 0, 1, p) == INVALID
