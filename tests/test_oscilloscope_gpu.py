"""Oscilloscope in a voice (csrc/og_scope.hip.h) on the device: the pass-through, the ring of the last samples, the window a
rising zero crossing freezes -- manual and auto-detected length -- and the deferred copy behind it, against the numpy restatement
of the reference's node (tests/scope_model.py) run over the device's own samples.  The node copies floats, so every comparison
is np.array_equal.  V = 70: one full wave and a partial one of 6 lanes; 1536 frames at 48 kHz."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oscen_amd
from oscen_amd import build as b
from tests import scope_model as sm

pytestmark = pytest.mark.gpu
SR = 48000.0
V = 70
FRAMES = 1536
f32 = np.float32
INVALID = oscen_amd.OG_E_INVALID
WORDS = (("written", np.uint32), ("triggered_length", np.uint32), ("last_sample", f32), ("detected_period", np.uint32))

HEAD = """
name: %s;
input frequency: value = 220.0;
input amp: value = 0.3;
input period: value = 64.0;
input enabled: value = 1.0;
input en_ramp: value = 0.0 [ramp: 100];
output out: stream;
"""


def graph(name, nodes, connections):
    dsl = HEAD % name + "nodes {\n    osc = PolyBlepOscillator::saw(220.0, 0.3);\n" + nodes + "}\nconnections {\n    frequency -> osc.frequency;\n" + \
        "    amp -> osc.amplitude;\n" + connections + "}\n"
    return oscen_amd.Graph(dsl=dsl, per_voice=("frequency", "period"))


def scope_graph(ctor, extra="", name="scope_voice"):
    return graph(name, "    scope = %s;\n" % ctor, "    osc.output -> scope.input;\n" + extra + "    scope.output -> out;\n")


def source_graph():
    """the same voice without the scope: the bit-equal input of every model"""
    return graph("scope_source", "", "    osc.output -> out;\n")


def freqs(n=V):
    return np.linspace(55.0, 1760.0, n).astype(f32)


def engine(g, n=V, period=None, group=False, taps=True):
    eng = oscen_amd.Engine(g, n, sample_rate=SR)
    eng.set_voice_values("frequency", freqs(n))
    if period is not None:
        eng.set_voice_values("period", period)
    if group:
        eng.group_voices(1)
    if taps:
        eng.set_voice_taps(np.arange(n, dtype=np.uint32))
    return eng


def run(eng, cuts, before=None):
    """process_block over `cuts` (before(eng, k) ahead of block k); the taps of all voices, [voice][frame]"""
    out = []
    for k, c in enumerate(cuts):
        if before:
            before(eng, k)
        eng.process_block(c)
        out.append(eng.read_voice_taps(c))
    return np.concatenate(out, axis=1)


_cache = {}


def source(silence_after=None):
    """the oscillator's samples, [voice][frame]: computed once per pattern, never changed.  silence_after: amplitude 0 from
    that block on"""
    if silence_after not in _cache:
        x = run(engine(source_graph()), [512] * 3, (lambda e, k: e.set_value("amp", 0.0) if k == silence_after else None) if silence_after else None)
        assert np.abs(x[:, :512]).max() > 0.1
        x.setflags(write=False)
        _cache[silence_after] = x
    return _cache[silence_after]


def periods():
    return SR / freqs().astype(np.float64)


def check(eng, scopes, path="scope", voices=None, words=True):
    """read_scope at sample_count 0, 5, capacity and 10 x capacity, and the state words, against the model, voice by voice"""
    cap = scopes[0].capacity
    voices = range(len(scopes)) if voices is None else voices
    for count in (0, 5, cap, 10 * cap):
        s, t = eng.read_scope(path, count)
        for v in voices:
            ws, wt = scopes[v].snapshot(count)
            assert np.array_equal(s[v], ws), (count, v, s[v], ws)
            assert np.array_equal(t[v], wt), (count, v, t[v], wt)
    if words:
        for name, ty in WORDS:
            got = eng.read_state_field(path + "." + name, dtype=ty)
            want = np.array([getattr(sc, name) for sc in scopes], dtype=ty)
            assert np.array_equal(got[list(voices)], want[list(voices)]), name


def results(eng, path="scope", cap=64):
    """everything a caller can see of a scope that does not depend on where launches are cut"""
    out = []
    for count in (0, 5, cap, 10 * cap):
        s, t = eng.read_scope(path, count)
        out += [np.concatenate(s), np.array([len(a) for a in s]), np.concatenate(t), np.array([len(a) for a in t])]
    out += [eng.read_state_field(path + "." + name, dtype=ty) for name, ty in WORDS]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. pass-through ---------------------------------------------------------------------------------------------------------
def test_the_scope_passes_its_input_through_bit_for_bit():
    eng = engine(scope_graph("Oscilloscope::new(64)"))
    assert eng.scope_info("scope") == (64, False)
    assert eng.lib.og_uses_split_kernel(eng.h) == 0  # the ordinary kernel only
    got = run(eng, [512] * 3)
    assert np.array_equal(got.view(np.uint32), source().view(np.uint32))


# ---- 2. the reference's own known answers (mod.rs:293-323) -------------------------------------------------------------------
def stream_graph(cap):
    return oscen_amd.Graph(dsl="""
name: scope_stream_%d;
input x: stream;
output out: stream;
nodes { scope = Oscilloscope::new(%d); }
connections { x -> scope.input; 0.0 -> scope.trigger_enabled; scope.output -> out; }
""" % (cap, cap))


def test_the_three_known_answers_on_every_voice():
    assert sm.known_answers()
    eng = oscen_amd.Engine(stream_graph(8), V, sample_rate=SR)
    eng.render_inputs([np.arange(10, dtype=f32)])
    s, t = eng.read_scope("scope", 4)
    assert len(s) == V and all(np.array_equal(a, np.array([6, 7, 8, 9], f32)) for a in s) and all(a.size == 0 for a in t)
    eng = oscen_amd.Engine(stream_graph(16), V, sample_rate=SR)
    s, t = eng.read_scope("scope", 8)
    assert all(a.size == 0 for a in s) and all(a.size == 0 for a in t)
    eng = oscen_amd.Engine(stream_graph(4), V, sample_rate=SR)
    eng.render_inputs([np.arange(4, dtype=f32)])
    s, t = eng.read_scope("scope", 16)
    assert all(np.array_equal(a, np.array([0, 1, 2, 3], f32)) for a in s) and all(a.size == 0 for a in t)


# ---- 3. manual mode, the default period ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [64, 7, 1])
def test_manual_mode_at_the_default_period(cap):
    eng = engine(scope_graph("Oscilloscope::new(%d)" % cap))
    assert eng.scope_info("scope") == (cap, False)
    assert np.array_equal(run(eng, [512] * 3), source())
    scopes = sm.run(source(), cap)
    assert all(sc.triggered_length == cap for sc in scopes)  # every voice crossed zero; the window is the capacity
    if cap == 64:  # both kinds of voice: a window that was superseded in time, and one that waited longer than a capacity
        assert (periods() < cap - 1).sum() >= 20 and (periods() > cap + 1).sum() >= 10
    check(eng, scopes)


def test_capacity_zero_is_one_and_with_handle_is_new():
    a = engine(scope_graph("Oscilloscope::new(0)"))
    assert a.scope_info("scope") == (1, False)
    run(a, [512])
    check(a, sm.run(source()[:, :512], 0))
    b1, b2 = engine(scope_graph("Oscilloscope::new(16)")), engine(scope_graph("Oscilloscope::with_handle(OscilloscopeHandle::new(16))"))
    run(b1, [512])
    run(b2, [512])
    assert same(results(b1, cap=16), results(b2, cap=16))


# ---- 4. manual mode, per-voice trigger_period --------------------------------------------------------------------------------
PERIODS = (0.4, 1.0, 2.5, 3.5, 17.0, 64.0, 1e9, np.inf, np.nan)
LENGTHS = (1, 1, 3, 4, 17, 64, 64, 64, 1)


def test_manual_mode_with_a_period_per_voice():
    per = np.array([PERIODS[v % len(PERIODS)] for v in range(V)], dtype=f32)
    eng = engine(scope_graph("Oscilloscope::new(64)", "    period -> scope.trigger_period;\n"), period=per)
    assert np.array_equal(run(eng, [512] * 3), source())
    scopes = sm.run(source(), 64, trigger_period=per)
    assert [sc.triggered_length for sc in scopes] == [LENGTHS[v % len(LENGTHS)] for v in range(V)]
    check(eng, scopes)


# ---- 5. auto-detect ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [64, 7])
def test_auto_detect(cap):
    eng = engine(scope_graph("Oscilloscope::with_auto_detect(OscilloscopeHandle::new(%d))" % cap))
    assert eng.scope_info("scope") == (cap, True)
    assert np.array_equal(run(eng, [512] * 3), source())
    scopes = sm.run(source(), cap, auto_detect=True)
    det = np.array([sc.detected_period for sc in scopes])
    if cap == 64:  # counted periods below the capacity, and at or above it (clamped to it)
        assert ((det >= 10) & (det < cap)).sum() >= 20 and (det == cap).sum() >= 10 and (periods() > cap + 1).sum() >= 10
    else:  # max(min(count, 7), 10) = 10, and the window is the capacity
        assert np.all(det == 10) and all(sc.triggered_length == cap for sc in scopes)
    check(eng, scopes)
    got = eng.read_state_field("scope.period_sample_count", dtype=np.uint32)
    assert np.array_equal(got, np.array([sc.period_sample_count for sc in scopes], dtype=np.uint32))


# ---- 6. trigger_enabled --------------------------------------------------------------------------------------------------------------
def test_trigger_disabled_from_the_start():
    eng = engine(scope_graph("Oscilloscope::with_auto_detect(OscilloscopeHandle::new(64))", "    0.0 -> scope.trigger_enabled;\n"))
    run(eng, [512] * 3)
    scopes = sm.run(source(), 64, auto_detect=True, trigger_enabled=0.0)
    assert all(sc.triggered_length == 0 and sc.period_sample_count == 0 for sc in scopes)
    check(eng, scopes)
    assert np.all(eng.read_state_field("scope.period_sample_count", dtype=np.uint32) == 0)
    assert np.array_equal(eng.read_state_field("scope.last_sample"), source()[:, -1]) and np.abs(source()[:, -1]).max() > 0


def test_trigger_switched_between_blocks():
    eng = engine(scope_graph("Oscilloscope::with_auto_detect(OscilloscopeHandle::new(64))", "    enabled -> scope.trigger_enabled;\n"))
    values = (1.0, 0.0, 0.6, 0.5, 1.0, 0.0)
    run(eng, [256] * 6, lambda e, k: e.set_value("enabled", values[k]))
    en = np.repeat(np.array(values, dtype=f32), 256)[None, :].repeat(V, axis=0)
    scopes = sm.run(source(), 64, auto_detect=True, trigger_enabled=en)
    check(eng, scopes)
    got = eng.read_state_field("scope.period_sample_count", dtype=np.uint32)
    assert np.array_equal(got, np.array([sc.period_sample_count for sc in scopes], dtype=np.uint32))


def test_trigger_enabled_as_a_ramp_crossing_one_half_inside_a_block():
    def drive(e, k):
        if k == 1:
            e.set_value("en_ramp", 1.0)
        if k == 2:
            e.set_value("en_ramp", 0.0)
    # the ramp's own per-frame values, from a twin whose output is the ramp (0.0 + value)
    twin = oscen_amd.Graph(dsl=HEAD % "scope_ramp_twin" + "nodes { a = AddValue::new(0.0); }\nconnections { en_ramp -> a.value; a.output -> out; }\n",
                           per_voice=("frequency", "period"))
    te = oscen_amd.Engine(twin, 1, sample_rate=SR)
    te.set_voice_taps(np.zeros(1, dtype=np.uint32))
    ramp = run(te, [512] * 3, drive)[0]
    inside = np.flatnonzero((ramp[:-1] > 0.5) != (ramp[1:] > 0.5)) + 1
    assert len(inside) == 2 and all(k % 512 not in (0, 511) for k in inside)  # on at frame 5xx, off at frame 10xx: inside blocks
    eng = engine(scope_graph("Oscilloscope::new(64)", "    en_ramp -> scope.trigger_enabled;\n"))
    run(eng, [512] * 3, drive)
    scopes = sm.run(source(), 64, trigger_enabled=ramp[None, :].repeat(V, axis=0))
    assert sum(sc.triggered_length > 0 for sc in scopes) >= 60
    check(eng, scopes)


# ---- 7. the deferred path ----------------------------------------------------------------------------------------------------------
def test_a_steady_tone_never_copies_a_window_it_supersedes_in_time():
    eng = engine(scope_graph("Oscilloscope::new(64)"))
    run(eng, [512] * 3)
    scopes = sm.run(source(), 64)
    short = np.flatnonzero(periods() < 63)
    assert len(short) >= 20
    copies = eng.read_state_field("scope.copies", dtype=np.uint32)
    assert np.all(copies[short] == 0)
    assert np.all(eng.read_state_field("scope.pending", dtype=np.uint32)[short] == 1)  # read while pending
    check(eng, scopes)
    assert np.any(copies[np.flatnonzero(periods() > 200)] >= 1)  # ... and a slow voice had to copy


def test_a_window_is_copied_once_crossings_stop_and_stays_frozen():
    eng = engine(scope_graph("Oscilloscope::new(64)"))
    got = run(eng, [512] * 3, lambda e, k: e.set_value("amp", 0.0) if k == 1 else None)
    x = source(silence_after=1)
    assert np.array_equal(got, x) and not np.any(x[:, 512:])
    scopes = sm.run(x, 64)
    hit = np.array([sc.triggered_length > 0 for sc in scopes])
    assert hit.sum() >= 60
    copies = eng.read_state_field("scope.copies", dtype=np.uint32)
    assert np.all(copies[hit] >= 1) and np.all(eng.read_state_field("scope.pending", dtype=np.uint32) == 0)
    assert all(np.any(sc.triggered[:sc.triggered_length]) for sc in np.array(scopes, dtype=object)[hit])
    check(eng, scopes)


# ---- 8. cuts -------------------------------------------------------------------------------------------------------------------------
def test_block_cuts_queued_launches_and_render_leave_the_scope_bit_identical():
    """(`copies` and `pending` say where a window lies, which depends on where chunks begin; what a read returns does not)"""
    scopes = sm.run(source(), 64, auto_detect=True)
    ctor = "Oscilloscope::with_auto_detect(OscilloscopeHandle::new(64))"
    want = None
    for cuts in ([512] * 3, [256] * 6, [37] * (FRAMES // 37) + [FRAMES % 37]):
        eng = engine(scope_graph(ctor))
        assert np.array_equal(run(eng, cuts), source()), cuts[0]
        check(eng, scopes)
        want = want or results(eng)
        assert same(results(eng), want), cuts[0]
    eng = engine(scope_graph(ctor), taps=False)
    eng.set_bus_batching(4)
    eng.process_blocks_async(512, 3)
    assert same(results(eng), want)
    eng = engine(scope_graph(ctor), taps=False)
    eng.set_bus_batching(4)
    eng.render(FRAMES, 256)
    assert same(results(eng), want)


# ---- 9. snapshots ------------------------------------------------------------------------------------------------------------------
def test_save_with_pending_windows_and_load_into_a_fresh_engine():
    g = scope_graph("Oscilloscope::new(64)")
    a = engine(g)
    run(a, [512, 188])
    assert 0 < a.read_state_field("scope.pending", dtype=np.uint32).sum()
    blob = a.save_state()
    fresh = engine(g)
    fresh.load_state(blob)
    tail = run(fresh, [324, 512])
    assert np.array_equal(tail, source()[:, 700:])
    check(fresh, sm.run(source(), 64))
    assert same(results(fresh), results_of_uninterrupted())


def results_of_uninterrupted():
    if "uninterrupted" not in _cache:
        eng = engine(scope_graph("Oscilloscope::new(64)"))
        run(eng, [512] * 3)
        _cache["uninterrupted"] = results(eng)
    return _cache["uninterrupted"]


def test_blobs_of_graphs_without_a_scope_keep_their_size():
    plain = engine(source_graph())
    words = plain.lib.og_state_bytes(plain.h)
    with_scope = engine(scope_graph("Oscilloscope::new(64)"))
    # 9 state words, the ring (2 x 64 + 16) and the window (64) per voice, and the node-array section's head (2 + 2 words)
    assert with_scope.lib.og_state_bytes(with_scope.h) - words == V * 4 * (9 + 144 + 64) + 16


# ---- 10. grouped voices ----------------------------------------------------------------------------------------------------------
def test_grouped_voices_read_through_the_slot_map():
    eng = engine(scope_graph("Oscilloscope::new(64)"), group=True)
    assert np.array_equal(run(eng, [512] * 3), source())
    check(eng, sm.run(source(), 64))
    eng.clear_scope_triggered("scope", [3, 69])
    assert [len(t) for t in eng.read_scope("scope", 1, first=2, n=3)[1]] == [64, 0, 64]


# ---- 11. clear_triggered -------------------------------------------------------------------------------------------------------------
def test_clear_on_a_subset_drops_pending_windows_and_the_next_crossing_fills_them_again():
    eng = engine(scope_graph("Oscilloscope::new(64)"))
    run(eng, [512, 512])
    scopes = sm.run(source()[:, :1024], 64)
    pending = eng.read_state_field("scope.pending", dtype=np.uint32)
    subset = [0, 5, 40, 63, 64, 69]
    assert any(pending[v] for v in subset) and any(not pending[v] for v in subset)
    eng.clear_scope_triggered("scope", subset)
    for v in subset:
        scopes[v].clear_triggered()
    assert all(len(t) == 0 for t in np.array(eng.read_scope("scope", 4)[1], dtype=object)[subset])
    check(eng, scopes)  # at once, and the others untouched
    run(eng, [512])
    sm.run(source()[:, 1024:], 64, scopes=scopes)
    assert all(scopes[v].triggered_length == 64 for v in subset)
    check(eng, scopes)
    eng.clear_scope_triggered("scope")
    assert all(len(t) == 0 for t in eng.read_scope("scope", 4)[1]) and all(len(s) == 4 for s in eng.read_scope("scope", 4)[0])


# ---- 12. og_init -------------------------------------------------------------------------------------------------------------------
def test_init_empties_everything():
    eng = engine(scope_graph("Oscilloscope::new(64)"))
    run(eng, [512])
    eng.init(SR)
    s, t = eng.read_scope("scope", 64)
    assert all(a.size == 0 for a in s) and all(a.size == 0 for a in t)
    for name in ("written", "triggered_length", "copies", "pending", "write_pos"):
        assert not np.any(eng.read_state_field("scope." + name, dtype=np.uint32)), name
    assert not np.any(eng.read_node_array("scope.ring")) and not np.any(eng.read_node_array("scope.triggered"))
    eng.set_voice_values("frequency", freqs())
    eng.set_voice_taps(np.arange(V, dtype=np.uint32))
    assert np.array_equal(run(eng, [512] * 3), source())
    check(eng, sm.run(source(), 64))


# ---- 13. node arrays and nested graph types ----------------------------------------------------------------------------------------
def test_a_node_array_of_scopes_and_a_scope_in_a_nested_graph_type():
    g = graph("scope_array", "    scopes = [Oscilloscope::new(16); 2];\n    g = Gain::new(-1.0);\n    m = Mixer::new();\n",
              "    osc.output -> scopes[0].input;\n    osc.output -> g.input;\n    g.output -> scopes[1].input;\n"
              "    scopes[0].output -> m.input_a;\n    scopes[1].output -> m.input_b;\n    m.output -> out;\n")
    eng = engine(g)
    run(eng, [512] * 3)
    assert eng.scope_info("scopes[0]") == (16, False) and eng.scope_info("scopes[1]") == (16, False)
    check(eng, sm.run(source(), 16), path="scopes[0]")
    check(eng, sm.run(-source(), 16), path="scopes[1]")
    oscen_amd.register_graph_type("ScopeInner", oscen_amd.Graph(dsl="""
name: scope_inner;
input frequency: value = 220.0;
output out: stream;
nodes { osc = PolyBlepOscillator::saw(220.0, 0.3); scope = Oscilloscope::with_auto_detect(OscilloscopeHandle::new(32)); }
connections { frequency -> osc.frequency; osc.output -> scope.input; scope.output -> out; }
""", per_voice=("frequency",)))
    try:
        outer = oscen_amd.Graph(dsl="""
name: scope_outer;
input frequency: value = 220.0;
output out: stream;
nodes { nested = ScopeInner::new(); }
connections { frequency -> nested.frequency; nested.out -> out; }
""", per_voice=("frequency",))
        eng = engine(outer)
        assert eng.scope_info("nested.scope") == (32, True)
        assert np.array_equal(run(eng, [512] * 3), source())
        check(eng, sm.run(source(), 32, auto_detect=True), path="nested.scope")
    finally:
        oscen_amd.unregister_graph_type("ScopeInner")


# ---- 14. the built-in kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fm_voice", "echo_voice"])
def test_builtin_kernels_keep_their_hashes(name):
    text = open(os.path.join(b.GEN, name + ".hip")).read()
    committed = re.search(r"OgKernelRegistrar og_reg_([0-9a-f]{16})\(", text).group(1)
    eng = oscen_amd.Engine(name, 64, sample_rate=SR)
    assert eng.kernel_hash == committed and eng.lib.og_kernel_is_jit(eng.h) == 0


# ---- argument errors on a live engine ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    eng = engine(scope_graph("Oscilloscope::new(64)"))
    lib = eng.lib
    cap, auto = C.c_uint32(), C.c_int()
    assert lib.og_scope_info(eng.h, b"osc", C.byref(cap), C.byref(auto)) == INVALID and b"no Oscilloscope" in lib.og_last_error()
    assert lib.og_scope_info(eng.h, b"nothing", None, None) == INVALID
    assert lib.og_scope_info(eng.h, None, None, None) == INVALID
    assert lib.og_scope_info(eng.h, b"scope", None, None) == 0
    buf = np.zeros((V, 64), f32)
    n = np.zeros(V, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.og_read_scope(eng.h, b"scope", V - 1, 2, 4, p(buf), p(n), None, None) == INVALID  # past the bank
    assert lib.og_read_scope(eng.h, b"scope", 0, V, 4, p(buf), None, None, None) == INVALID     # rows without their lengths
    assert lib.og_read_scope(eng.h, b"osc", 0, V, 4, p(buf), p(n), None, None) == INVALID
    assert lib.og_read_scope(eng.h, b"scope", 0, V, 4, None, None, None, None) == 0              # both pairs may be null
    assert lib.og_read_scope(eng.h, b"scope", 0, V, 4, None, p(n), None, None) == 0 and not np.any(n)  # lengths alone
    bad = np.array([V], dtype=np.uint32)
    assert lib.og_clear_scope_triggered(eng.h, b"scope", p(bad), 1) == INVALID
    assert lib.og_clear_scope_triggered(eng.h, b"osc", None, 0) == INVALID
    plain = engine(source_graph())
    assert lib.og_read_scope(plain.h, b"scope", 0, 1, 4, None, None, None, None) == INVALID
