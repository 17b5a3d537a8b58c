"""The edges of the Delay's chunk-ahead staging (og::ring_chunk_begin / og::delay_tick): the staging limits 16 and 32, the
ring wrap, offsets above the capacity, mixed lanes in one wave, set-value events inside a staged chunk, queued launches,
several lines in one graph, a snapshot across a wrap -- and the built-in echo_voice, sample by sample.

Every case is saw -> Delay with the output `d.output + osc.output`, against the oracle's oo_polyblep_process +
oo_delay_process driven sample by sample.  Tolerance: the project's contract, 1e-5 * max(1, |ref|) per sample.  70 voices
(two waves, the second ragged); the taps compared are voices of both waves and of the ragged tail.  The block sizes cut
chunks short, start launches in the middle of a line and end them on and off a chunk boundary (the `more` flag of
ring_chunk_begin goes both ways).

The ring of a Delay holds 2 * sample_rate slots, rounded up to a power of two: 131 072 at 48 kHz, 256 at a sample rate of
100 Hz, where a test of a few hundred frames wraps it."""
import ctypes as C

import numpy as np
import pytest

import oscen_amd
from tests import observed
from tests import oracle_lib as ol
from tests.test_bench_entry_points_gpu import DeviceBuffer
from tests.test_n3_gpu import _delay, _saw

pytestmark = pytest.mark.gpu

SR = 48000.0
SR_LOW = 100.0  # RingSpec::capacity: 256 slots
CAP_LOW = 256
TOL = 1e-5
N = 70
TAPS = [0, 1, 33, 63, 64, 69]
BLOCKS = (37, 16, 1, 15, 17, 33, 128)
BLOCKS_WRAP = BLOCKS + (256, 200, 100)  # 803 frames: write_pos passes the top of a 256-slot ring three times
f32 = np.float32


def _freqs(sr):
    if sr == SR:
        return np.geomspace(55.0, 1760.0, N).astype(f32)
    return np.geomspace(sr / 900.0, sr / 27.0, N).astype(f32)


def _graph(name, lines, dly=None, fb=None):
    """saw -> one Delay per (delay_samples, feedback) of `lines`, summed with the dry signal.  dly / fb: None (the
    constructor's field stays), "uniform" (a broadcast value input) or "voice" (a per-voice value input) on line 0."""
    g = oscen_amd.Graph(name)
    g.input_value("frequency", 440.0, per_voice=True)
    if dly:
        g.input_value("dly", lines[0][0], per_voice=dly == "voice")
    if fb:
        g.input_value("fb", lines[0][1], per_voice=fb == "voice")
    g.output_stream("out")
    g.node("osc", "PolyBlepOscillator::saw", 440.0, 0.5)
    g.connect("frequency", "osc.frequency")
    names = ["d"] if len(lines) == 1 else ["d%d" % k for k in range(len(lines))]
    for nm, (ds, f) in zip(names, lines):
        g.node(nm, "Delay::new", ds, f)
        g.connect("osc.output", nm + ".input")
    if dly:
        g.connect("dly", names[0] + ".delay_samples")
    if fb:
        g.connect("fb", names[0] + ".feedback")
    g.connect(" + ".join(nm + ".output" for nm in names) + " + osc.output", "out")
    return g


def _engine(graph, sr, taps=TAPS):
    eng = oscen_amd.Engine(graph, N, sample_rate=sr)
    eng.set_voice_values("frequency", _freqs(sr))
    eng.set_voice_taps(taps)
    return eng


def _render(eng, blocks, before_block=None):
    got = []
    for b, frames in enumerate(blocks):
        if before_block:
            before_block(eng, b)
        eng.process_block(frames)
        got.append(eng.read_voice_taps(frames))
    return np.concatenate(got, axis=1)


def _ref_voice(lib, sr, freq, total, lines, dly=None, fb=None):
    """One voice of _graph on the oracle.  dly / fb: what the connected input of line 0 holds on every frame (a scalar or
    an array of `total`); the generated edge copy writes it into the field before every process()."""
    o = _saw(lib, freq)
    o.sample_rate = sr
    ds = []
    for s, f in lines:
        d = _delay(lib, s, f)
        d.sample_rate = sr
        lib.oo_delay_prepare(C.byref(d))
        ds.append(d)
    dly = None if dly is None else np.broadcast_to(np.asarray(dly, dtype=f32), (total,))
    fb = None if fb is None else np.broadcast_to(np.asarray(fb, dtype=f32), (total,))
    out = np.zeros(total, dtype=f32)
    for i in range(total):
        lib.oo_polyblep_process(C.byref(o))
        if dly is not None:
            ds[0].delay_samples = float(dly[i])
        if fb is not None:
            ds[0].feedback = float(fb[i])
        acc = None
        for d in ds:
            d.input = o.output
            lib.oo_delay_process(C.byref(d))
            acc = f32(d.output) if acc is None else acc + f32(d.output)
        out[i] = acc + f32(o.output)
    for d in ds:
        lib.oo_delay_free(C.byref(d))
    return out


def _ref(lib, sr, total, lines, taps=TAPS, dly=None, fb=None):
    """dly / fb: None, a scalar, or {voice: per-frame array or scalar}"""
    fr = _freqs(sr)
    pick = lambda x, v: x[v] if isinstance(x, dict) else x
    return np.stack([_ref_voice(lib, sr, fr[v], total, lines, pick(dly, v), pick(fb, v)) for v in taps])


def _err(got, ref):
    assert np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def _is_exact_sample_read(x):
    """the test of RingBuffer::get (ring_buffer/mod.rs:178), in f32 as there"""
    o = max(f32(x), f32(0.0))
    fr = f32(o - np.trunc(o))
    return bool(fr < f32(1e-6) or f32(f32(1.0) - fr) < f32(1e-6))


# ---- a. the staging limits: offsets below 16 are never staged, 16..31 for the chunk at hand, 32 and up a chunk ahead ----
A_CASES = [(d, f) for d in (1.0, 15.0, 16.0, 17.0, 31.0, 32.0, 33.0, 48.0) for f in (0.0, 0.6, 1.7)]
A_CASES += [(0.9999995, 0.6), (3.0000005, 0.6), (0.999998, 0.6), (0.5, 0.6)]  # two (almost) whole, two just outside


@pytest.mark.parametrize("delay_samples,feedback", A_CASES)
def test_staging_limits(delay_samples, feedback):
    """Unconnected fields (fixed_params): feedback 1.7 keeps the fast path off until the first tick has clamped the field
    to 0.99, then lets it turn on.  0.9999995 and 3.0000005 are whole samples to RingBuffer::get, 0.999998 and 0.5 are not."""
    lib = ol.load()
    assert _is_exact_sample_read(delay_samples) == (delay_samples not in (0.999998, 0.5))
    lines = [(delay_samples, feedback)]
    eng = _engine(_graph("dedge_a_%d_%d" % (round(delay_samples * 1e7), round(feedback * 10)), lines), SR)
    got = _render(eng, BLOCKS)
    ref = _ref(lib, SR, sum(BLOCKS), lines)
    assert np.max(np.abs(ref)) > 0.4
    err = _err(got, ref)
    observed.note(err)
    assert err <= TOL, err


# ---- b. the ring wraps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delay_samples", [255.0, 254.0, 240.0, 239.0, 224.0, 32.0, 16.0, 0.5, 1.5, 253.25, 254.5])
def test_ring_wrap(delay_samples):
    """100 Hz: a 256-slot ring, 803 frames.  write_pos passes the top three times; a delay of capacity - 1 reads the slot
    the tick is about to overwrite, the cubic reads near it touch the slots written longest ago."""
    lib = ol.load()
    lines = [(delay_samples, 0.6)]
    eng = _engine(_graph("dedge_b_%d" % round(delay_samples * 100), lines), SR_LOW)
    got = _render(eng, BLOCKS_WRAP)
    ref = _ref(lib, SR_LOW, sum(BLOCKS_WRAP), lines)
    assert np.max(np.abs(ref)) > 0.4
    err = _err(got, ref)
    observed.note(err)
    assert err <= TOL, err
    # the saved state holds a 256-slot line per voice (and, beside it, a few dozen words per voice)
    assert CAP_LOW * N * 4 <= eng.state_bytes < 2 * CAP_LOW * N * 4


# ---- c. an offset above the capacity ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dly", [300.0, 296.0, 1000.0, 255.0, 40.0])
def test_offset_above_capacity(dly):
    """A broadcast input overwrites the field every frame; the clamp to capacity - 1 runs on every 32nd tick only and
    holds for that tick alone.  On the other 31 the offset is taken modulo the capacity (300 reads 44 back, 1000 reads 232)."""
    lib = ol.load()
    lines = [(40.0, 0.6)]
    eng = _engine(_graph("dedge_c", lines, dly="uniform"), SR_LOW)
    eng.set_value("dly", dly)
    got = _render(eng, BLOCKS_WRAP)
    ref = _ref(lib, SR_LOW, sum(BLOCKS_WRAP), lines, dly=dly)
    assert np.max(np.abs(ref)) > 0.4
    err = _err(got, ref)
    observed.note(err)
    assert err <= TOL, err


# ---- d. staged, unstaged, cubic and clamped lanes in one wave -----------------------------------------------------------
def test_mixed_lanes_in_one_wave():
    """Per-voice delay_samples and feedback.  Every wave holds lanes of each kind, so the wave-uniform fast path must stay
    off and every lane must still be right.  The delay cycles with the voice number, the feedback with every sixth voice,
    so each delay meets each feedback within the first 18 voices.  One pairing is left out of the comparison: a one-sample
    delay with feedback 1.5 (unclamped on 31 ticks of 32) leaves the f32 range within the test's frames."""
    lib = ol.load()
    delays = [8.0, 16.0, 40.0, 40.5, 300.0, 1.0000005]  # 300: above the capacity at 100 Hz
    fbs = [0.0, 0.6, 1.5]
    dly = np.array([delays[v % 6] for v in range(N)], dtype=f32)
    fb = np.array([fbs[(v // 6) % 3] for v in range(N)], dtype=f32)
    taps = [v for v in range(18) if not (dly[v] == f32(1.0000005) and fb[v] == f32(1.5))] + [33, 63, 64, 69]
    lines = [(40.0, 0.5)]
    eng = _engine(_graph("dedge_d", lines, dly="voice", fb="voice"), SR_LOW, taps)
    eng.set_voice_values("dly", dly)
    eng.set_voice_values("fb", fb)
    got = _render(eng, BLOCKS)
    ref = _ref(lib, SR_LOW, sum(BLOCKS), lines, taps, dly={v: dly[v] for v in taps}, fb={v: fb[v] for v in taps})
    assert len({(dly[v], fb[v]) for v in taps}) == 17 and np.max(np.abs(ref)) > 0.4
    err = _err(got, ref)
    observed.note(err)
    assert err <= TOL, err


# ---- e. set-value events inside a staged chunk ----------------------------------------------------------------------------
E_TAPS = [0, 1, 3, 33, 63, 64, 69]
E_FRAMES = 256
E_LINES = [(40.0, 0.5)]
E_CASES = [("dly", at, to) for to in (24.0, 8.0, 40.5) for at in (80, 85, 95)]  # staged -> staged, -> unstaged, -> cubic
E_CASES += [("fb", 96, 1.5), ("fb", 97, 1.5)]  # on a tick that clamps (frame_counter 0) and on one that does not
_e_cache = {}


def _e_ref(lib, name, voices, at, to):
    """oracle run of case e (shared between the two voice sets: a voice without the event is the plain run)"""
    def one(key):
        if key not in _e_cache:
            n, a, t = key
            sched = np.full(E_FRAMES, E_LINES[0][0 if n == "dly" else 1], dtype=f32)
            if a is not None:
                sched[a:] = t
            other = E_LINES[0][1 if n == "dly" else 0]
            kw = {"dly": sched, "fb": other} if n == "dly" else {"dly": other, "fb": sched}
            _e_cache[key] = _ref(lib, SR, E_FRAMES, E_LINES, E_TAPS, **kw)
        return _e_cache[key]

    plain, changed = one((name, None, None)), one((name, at, to))
    hit = np.array([v in voices for v in E_TAPS])
    return np.where(hit[:, None], changed, plain), plain, hit


@pytest.mark.parametrize("voices", ["all", "3,64"])
@pytest.mark.parametrize("name,at,to", E_CASES)
def test_set_value_event_inside_a_staged_chunk(name, at, to, voices):
    """`dly` (40) and `fb` (0.5) are per-voice inputs: block-constant to the compiler, so the chunk of frames 80..95 is
    staged for an offset of 40 and takes the fast path -- until og_schedule_voice_value changes one of them on frame `at`.
    The new value holds from that very frame on, as it does when the block is cut at `at` and set_voice_values is called."""
    lib = ol.load()
    vs = list(range(N)) if voices == "all" else [3, 64]
    ref, plain, hit = _e_ref(lib, name, vs, at, to)
    assert np.max(np.abs(ref[hit] - plain[hit])) > 1e-2  # the event is audible: the case cannot pass without it
    graph = _graph("dedge_e", E_LINES, dly="voice", fb="voice")

    eng = _engine(graph, SR, E_TAPS)
    for v in vs:
        eng.schedule_voice_value(name, v, at, to)
    got = _render(eng, (E_FRAMES,))
    bad = np.flatnonzero(np.any(np.abs(got - ref) > TOL * np.maximum(1.0, np.abs(ref)), axis=0))
    err = _err(got, ref)
    observed.note(err)
    assert err <= TOL, (err, "frames %d..%d" % (bad[0], bad[-1]))

    cut = _engine(graph, SR, E_TAPS)

    def between(e, b):
        if b == 1:
            for v in ([0] if voices == "all" else vs):
                e.set_voice_values(name, np.full(N if voices == "all" else 1, to, dtype=f32), first=v)

    got2 = _render(cut, (at, E_FRAMES - at), between)
    err2 = _err(got2, ref)
    observed.note(err2)
    assert err2 <= TOL, err2


# ---- f. queued launches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", [False, True])
def test_queued_launches_equal_blocking_blocks(change):
    """Eight 64-frame blocks queued behind one another (one launch covers them) against eight blocking blocks: the staging
    restarts at every launch, so the bus must be the same bit for bit.  `change`: a broadcast dly 40 -> 24 between the halves."""
    lines = [(40.0, 0.6)]
    graph = _graph("dedge_f%d" % change, lines, dly="uniform" if change else None)
    block, nb = 64, 8

    def halfway(e):
        if change:
            e.set_value("dly", 24.0)

    a = _engine(graph, SR)
    want = []
    for b in range(nb):
        if b == nb // 2:
            halfway(a)
        want.append(a.process_block(block).copy())
    want = np.concatenate(want, axis=0)

    q = _engine(graph, SR)
    q.set_bus_batching(8)
    ch = q.channels
    buf = DeviceBuffer(nb * block * ch * 4)
    try:
        if change:
            q.process_blocks_async(block, nb // 2, buf.ptr.value, block * ch * 4)
            halfway(q)
            q.process_blocks_async(block, nb // 2, buf.ptr.value + (nb // 2) * block * ch * 4, block * ch * 4)
        else:
            q.process_blocks_async(block, nb, buf.ptr.value, block * ch * 4)
        q.synchronize()
        got = buf.to_host().reshape(nb * block, ch)
    finally:
        buf.free()
    assert np.max(np.abs(want)) > 1.0  # 70 voices on the bus
    assert np.array_equal(got, want)
    if change:  # ... and the change is in there
        plain = _engine(_graph("dedge_f0", lines), SR)
        assert not np.array_equal(np.concatenate([plain.process_block(block).copy() for _ in range(nb)], axis=0), want)


# ---- g. several lines in one graph --------------------------------------------------------------------------------------------
def test_four_lines_in_one_graph_and_a_fifth_is_refused():
    """Every Delay has its own ring and its own LDS column (ring_lds[k]): unstaged, staged a chunk ahead, cubic, and long."""
    lib = ol.load()
    lines = [(16.0, 0.3), (33.0, 0.6), (0.5, 0.0), (100.0, 0.5)]
    eng = _engine(_graph("dedge_g4", lines), SR)
    got = _render(eng, BLOCKS)
    ref = _ref(lib, SR, sum(BLOCKS), lines)
    assert np.max(np.abs(ref)) > 1.0
    err = _err(got, ref)
    observed.note(err)
    assert err <= TOL, err
    with pytest.raises(oscen_amd.OscenError, match="at most 4 Delay nodes"):
        oscen_amd.Engine(_graph("dedge_g5", lines + [(7.0, 0.1)]), N, sample_rate=SR)


# ---- h. a snapshot across the wrap -----------------------------------------------------------------------------------------------
def test_snapshot_just_below_the_wrap():
    """save_state after 250 of a 256-slot ring's frames; the restored engine's next 64 frames cross the top of the ring
    with cubic reads (delay 254.5) that reach back over it."""
    graph = _graph("dedge_h", [(254.5, 0.6)])
    a = _engine(graph, SR_LOW)
    _render(a, (128, 122))
    blob = a.save_state()
    want_bus = a.process_block(64).copy()
    want = a.read_voice_taps(64)
    b = oscen_amd.Engine(graph, N, sample_rate=SR_LOW)
    b.load_state(blob)
    b.set_voice_taps(TAPS)
    got_bus = b.process_block(64).copy()
    got = b.read_voice_taps(64)
    assert np.max(np.abs(want)) > 0.4
    assert np.array_equal(got_bus, want_bus) and np.array_equal(got, want)


# ---- the built-in echo_voice against the oracle's nodes ---------------------------------------------------------------------------
def _echo_ref_voice(lib, freq, total, delay_samples, feedback, on=5, off=3000):
    """og_builtin.cpp echo_voice(): saw 0.6 x ADSR(0.01, 0.1, 0.7, 0.2) -> Mixer -> Delay(11025, 0) -> feedback edge ->
    TptFilter(4000, 0.7); `filter.output * feedback` back into the mixer; dry 0.65 / wet 0.35.  The filter sits behind a
    feedback edge: it runs before the Delay and reads the sample the Delay produced on the previous frame
    (test_n3_gpu.py::test_feedback_edge_through_delay_node models the same ordering).  The reference's hand-written
    EchoChannel (examples/simple-echo/src/lib.rs:33-61) also feeds the previous sample's `filter.output * feedback` into
    the delay's input, but runs its filter behind the delay within the sample and soft-clips the sum; the built-in is
    the graph form, so the generated schedule of a feedback edge is what is modelled here."""
    o = _saw(lib, freq, amp=0.6)
    e = ol.Adsr()
    lib.oo_adsr_new(C.byref(e), 0.01, 0.1, 0.7, 0.2)
    e.sample_rate = SR
    lib.oo_adsr_prepare(C.byref(e))
    d = _delay(lib, 11025.0, 0.0)
    t = ol.Tpt()
    lib.oo_tpt_new(C.byref(t), 4000.0, 0.7, 1)
    t.sample_rate = SR
    lib.oo_tpt_prepare(C.byref(t))
    fbk, dry, wet = f32(feedback), f32(0.65), f32(0.35)
    out, echo = np.zeros(total, dtype=f32), np.zeros(total, dtype=f32)
    for i in range(total):
        if i == on or i == off:
            ev = ol.Event(0, 1.0 if i == on else 0.0, 0)
            lib.oo_adsr_handle_gate_event(C.byref(e), C.byref(ev))
        lib.oo_polyblep_process(C.byref(o))
        lib.oo_adsr_process(C.byref(e))
        t.cutoff = 4000.0
        t.input[0] = d.output  # still last frame's
        lib.oo_tpt_process(C.byref(t))
        voiced = f32(o.output) * f32(e.output)
        d.delay_samples = delay_samples
        d.input = float(voiced + f32(t.output[0]) * fbk)
        lib.oo_delay_process(C.byref(d))
        out[i] = voiced * dry + f32(t.output[0]) * wet
        echo[i] = t.output[0]
    lib.oo_delay_free(C.byref(d))
    return out, echo


@pytest.mark.parametrize("delay_samples,feedback,total", [(None, None, 12288), (100.0, 0.9, 2048)])
def test_echo_voice_against_the_oracle(delay_samples, feedback, total):
    """The built-in's samples: the defaults (delay 11025, feedback 0.4) until the first echo is out, and a 100-sample
    line with feedback 0.9, where the loop through the filter is heard many times over."""
    lib = ol.load()
    freqs = _freqs(SR)
    eng = oscen_amd.Engine("echo_voice", N, sample_rate=SR)
    eng.set_voice_values("frequency", freqs)
    if delay_samples is not None:
        eng.set_value("delay_samples", delay_samples)
        eng.set_value("feedback", feedback)
    for v in range(N):
        eng.schedule_voice_event("gate", v, 5, 1.0)
        eng.schedule_voice_event("gate", v, 3000, 0.0)
    eng.set_voice_taps(list(range(N)))
    bus, taps = [], []
    for _ in range(total // 256):
        bus.append(eng.process_block(256).copy())
        taps.append(eng.read_voice_taps(256))
    bus, taps = np.concatenate(bus, axis=0), np.concatenate(taps, axis=1)
    ds, fb = (11025.0, 0.4) if delay_samples is None else (delay_samples, feedback)
    ref, echo = map(np.stack, zip(*[_echo_ref_voice(lib, freqs[v], total, ds, fb) for v in TAPS]))
    if delay_samples is None:  # the note comes back from frame 5 + 11025 on, and not before
        assert np.max(np.abs(echo[:, 11100:])) > 0.1 and not echo[:, :11025].any()
    else:
        assert np.max(np.abs(echo[:, 1000:])) > 0.1
    err = _err(taps[TAPS], ref)
    observed.note(err)
    assert err <= TOL, err
    # the bus is the sum of the voices: the project's bus rule, 2e-6 * sum |x_i| per sample, against the float64 sum
    want = taps.astype(np.float64).sum(axis=0)
    scale = np.abs(taps.astype(np.float64)).sum(axis=0)
    assert bus.shape == (total, 1) and np.max(np.abs(want)) > 1.0
    assert np.all(np.abs(bus[:, 0] - want) <= 2e-6 * scale)
