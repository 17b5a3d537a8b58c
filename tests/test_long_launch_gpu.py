"""One launch over everything the caller queued (og_set_bus_batching above 32 blocks; the automatic rule of the wide
four-wave form): the results are those of block-by-block launches, bit for bit.

A small fm_voice bank takes the kernel of the headline run -- the cost model picks four waves and the wide form where a CU
holds one workgroup -- so the shapes are tiny: 200 voices (four workgroups, the last with 8 live lanes), 45 blocks of 96 frames
(blocks straddle the 16-frame chunks, the launch ends on a short chunk, more than 32 blocks), envelope times short enough for
the 4 320 frames to hold every stage, stage ends, ends of Release into Idle and retriggers.

The score goes to the device with the first launch, and a queue that has more events waiting on the host than the staging
bound is launched early (process_async; unchanged).  So every run first renders one pre-roll block, as bench.py's warm-up
does: the launches counted afterwards are cut by the queue limit alone.
"""
import numpy as np
import pytest

import oscen_amd
from tests.test_bench_entry_points_gpu import DeviceBuffer

pytestmark = pytest.mark.gpu

SR = 48000.0
N, FR, NB = 200, 96, 45
T0 = FR  # the pre-roll block
LIMIT = 256  # OG_MAX_QUEUE_BLOCKS
ENV = {"%s_%s" % (op, k): v for op in ("op3", "op2", "op1", "filter") for k, v in (("attack", 0.002), ("decay", 0.01), ("release", 0.02))}


def _score():
    rng = np.random.default_rng(0x13C0)
    on, off, re = rng.integers(0, 64, N), rng.integers(600, 1501, N), rng.integers(2500, 3501, N)
    v = np.tile(np.arange(N), 3)
    f = np.concatenate([on, off, re]) + T0
    x = np.concatenate([0.5 + 0.5 * rng.random(N), np.zeros(N), 0.5 + 0.5 * rng.random(N)])
    freq = (110.0 * 2.0 ** (rng.integers(0, 48, N) / 12.0)).astype(np.float32)
    return v, f, x, freq


SCORE_V, SCORE_F, SCORE_X, FREQ = _score()
# events for frames inside blocks 25..44, pushed while 20 blocks are queued (fewer than the staging bound of 200 / 4 + 32)
LATE_V = np.array([3, 64, 65, 127, 128, 191, 192, 199, 7, 150])
LATE_F = T0 + np.array([25 * FR, 25 * FR + 95, 30 * FR + 17, 31 * FR, 33 * FR + 1, 38 * FR + 50, 40 * FR + 15, 44 * FR + 95, 44 * FR, 27 * FR + 16])
LATE_X = np.array([0.9, 0.0, 0.7, 0.0, 0.6, 0.0, 0.8, 0.5, 0.0, 1.0])


def engine(sets=(), grouped=False, extra=None):
    eng = oscen_amd.Engine("fm_voice", N, sample_rate=SR)
    for k, v in list(ENV.items()) + list(sets):
        eng.set_value_immediate(k, v)
    eng.set_voice_values("frequency", FREQ)
    v, f, x = SCORE_V, SCORE_F, SCORE_X
    if extra is not None:
        v, f, x = np.concatenate([v, extra[0]]), np.concatenate([f, extra[1]]), np.concatenate([x, extra[2]])
    order = np.argsort(f, kind="stable")
    eng.schedule_voice_events("gate", v[order], f[order], x[order])
    if grouped:
        eng.group_voices(1)
    return eng


def run(batching, sets=(), grouped=False, ramp_block=None, late=None, dest="dense", split=None):
    """pre-roll, then NB blocks under `batching`; `split`: blocks handed over by the first call (the timers are read after it).
    late = "queued": LATE_* scheduled once 20 blocks are queued; "upfront": with the score."""
    eng = engine(sets, grouped, (LATE_V, LATE_F, LATE_X) if late == "upfront" else None)
    ch = eng.channels
    eng.process_block(FR)
    if batching != 1:
        eng.set_bus_batching(batching)
    eng.enable_kernel_timing(True)
    stride = (FR + (32 if dest == "strided" else 0)) * ch
    buf = DeviceBuffer(NB * stride * 4)
    out = {}
    try:
        def go(b0, b1):
            if b1 > b0:
                eng.process_blocks_async(FR, b1 - b0, None if dest == "null" else buf.ptr.value + b0 * stride * 4, 0 if dest == "null" else stride * 4)

        cuts = sorted({0, NB} | ({ramp_block} if ramp_block is not None else set()) | ({20} if late == "queued" else set()) | ({split} if split else set()))
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            if b0 == ramp_block:
                eng.set_value("filter_cutoff", 6000.0)  # `[ramp: 2205]`: launches what is queued, then ramps over 23 blocks
            if late == "queued" and b0 == 20:
                eng.schedule_voice_events("gate", LATE_V, LATE_F, LATE_X)
            go(b0, b1)
            if b1 == split:
                out["timed_after_split"] = eng.kernel_blocks_timed
        eng.flush()
        eng.synchronize()
        out["launches"] = eng.kernel_time_ms()[1]
        out["blocks_timed"] = eng.kernel_blocks_timed
        out["variant"], out["tier"], out["depth"] = eng.kernel_variant, eng.kernel_fold_tier, eng.pipeline_depth
        out["bus"] = buf.to_host().reshape(NB, stride)[:, :FR * ch].copy()
    finally:
        buf.free()
    out["state"] = bytes(eng.save_state())
    out["next"] = eng.process_block(FR).copy()  # (a NULL destination keeps the buses in the engine: what follows them is readable)
    eng.close()
    return out


_REF = {}


def reference(**kw):
    """the batching-1 run of a configuration: computed once, shared, left unchanged"""
    key = repr(sorted(kw.items()))
    if key not in _REF:
        _REF[key] = run(1, **kw)
        assert _REF[key]["launches"] == NB and _REF[key]["blocks_timed"] == NB
        _REF[key]["bus"].setflags(write=False)
    return _REF[key]


def same(a, b):
    assert np.array_equal(a["bus"], b["bus"]), float(np.abs(a["bus"] - b["bus"]).max())
    assert a["state"] == b["state"]
    assert np.array_equal(a["next"], b["next"])


@pytest.mark.parametrize("grouped", [False, True])
def test_a_launch_of_45_blocks_equals_45_launches(grouped):
    a = reference(grouped=grouped)
    assert np.abs(a["bus"]).max() > 0.05 and np.isfinite(a["bus"]).all()
    assert np.abs(a["bus"][-1]).max() > 0.0  # (the retriggered notes sound to the end)
    b = run(0, grouped=grouped)
    c = run(40, grouped=grouped, split=40)
    print("\nlaunches/blocks: batching 1 %d/%d, automatic %d/%d, 40 %d/%d (%d after 40 blocks); %s tier %d"
          % (a["launches"], a["blocks_timed"], b["launches"], b["blocks_timed"], c["launches"], c["blocks_timed"], c["timed_after_split"],
             b["variant"], b["tier"]))
    same(b, a)
    same(c, a)
    assert (b["launches"], b["blocks_timed"]) == (1, NB)
    assert c["timed_after_split"] == 40 and (c["launches"], c["blocks_timed"]) == (2, NB)  # launches of 40 and 5 blocks
    for r in (a, b, c):  # the headline's kernel: the wide four-wave form, the zero variant of fold tier 2 (og_k4w_<hash>_00z2)
        assert r["depth"] == 4 and r["variant"].startswith("og_k4w_") and r["variant"].endswith("_z") and r["tier"] == 2, (r["variant"], r["tier"])


def test_a_ramp_inside_a_long_queue_still_splits_it_where_the_ramp_ends():
    sets = (("filter_env_amount", 2000.0),)  # the general kernels
    a = reference(sets=sets, ramp_block=3)
    b = run(0, sets=sets, ramp_block=3)
    print("\nramp: %d launches over %d blocks, %s tier %d" % (b["launches"], b["blocks_timed"], b["variant"], b["tier"]))
    same(b, a)
    assert not np.array_equal(a["bus"], reference(sets=sets)["bus"])  # (the ramp is audible)
    # blocks 0..2 (the setter launches them), 3..25 (2 205 = 22 x 96 + 93 frames: the ramp ends inside block 25), 26..44
    assert (b["launches"], b["blocks_timed"]) == (3, NB)
    assert b["tier"] == 0 and b["variant"].startswith("og_k4w_")


@pytest.mark.parametrize("dest", ["strided", "null"])
def test_strided_and_null_destinations(dest):
    """a stride larger than a block (the launch sums into the staging bus, one copy per block); a NULL destination (the
    buses stay in the engine's own buffer, which no entry reads back: the state after them and the block that follows are
    compared)"""
    a = reference()
    b = run(0, dest=dest)
    assert (b["launches"], b["blocks_timed"]) == (1, NB)
    assert b["state"] == a["state"] and np.array_equal(b["next"], a["next"])
    if dest == "strided":
        assert np.array_equal(b["bus"], a["bus"])


def test_events_scheduled_while_20_blocks_are_queued():
    a = reference(late="upfront")
    b = run(0, late="queued")
    same(b, a)
    assert not np.array_equal(a["bus"], reference()["bus"])  # (the late events are audible)
    assert (b["launches"], b["blocks_timed"]) == (1, NB)


def test_render_over_50_blocks_equals_50_blocking_blocks():
    a = engine()
    want = np.concatenate([a.process_block(FR).copy() for _ in range(50)], axis=0)
    b = engine()
    b.enable_kernel_timing(True)
    got = b.render(50 * FR, block=FR)
    assert np.array_equal(got, want)
    assert bytes(a.save_state()) == bytes(b.save_state())
    assert b.kernel_blocks_timed == 50 and b.kernel_time_ms()[1] <= 3  # (the score's upload cuts the first launch short)
    a.close()
    b.close()


def test_a_handler_that_reads_frame_offset_keeps_launches_of_32_blocks():
    """the launch carries 32 block starts for `frame_offset` (tests/test_dsl_r3_gpu.py: R3OffCap)"""
    f32 = np.float32
    oscen_amd.register_node("LLOffCap::new", inputs=[("gate", "event", 0.0, -1)], outputs=["captured_offset"],
                            state=[("cap", "f32", -1.0, -1), ("hits", "f32", 0.0, -1)],
                            handlers={"gate": "    cap = (float)frame_offset;\n    hits += 1.0f;\n"}, process="    captured_offset = cap;\n")
    try:
        n, fr, nb = 5, 64, 40
        at = {0: (1, 5), 1: (20, 63), 2: (33, 17), 3: (39, 63), 4: (35, 0)}  # voice -> (block index, offset)
        runs = []
        for batching in (1, 0):
            g = oscen_amd.Graph(dsl="""name: LLOff; input gate: event; output out: stream;
                nodes { caps = [LLOffCap::new(); 3]; }
                connections { gate -> caps.gate; caps.captured_offset -> out; }""")
            eng = oscen_amd.Engine(g, n, sample_rate=SR)
            eng.process_block(fr)
            for v, (b, off) in at.items():
                eng.schedule_voice_event("gate", v, fr + b * fr + off, 1.0)
            if batching != 1:
                eng.set_bus_batching(batching)
            eng.enable_kernel_timing(True)
            ch = eng.channels
            buf = DeviceBuffer(nb * fr * ch * 4)
            try:
                eng.process_blocks_async(fr, nb, buf.ptr.value, fr * ch * 4)
                eng.flush()
                eng.synchronize()
                bus = buf.to_host().reshape(nb, fr * ch).copy()
            finally:
                buf.free()
            cap = eng.read_state_field("caps[2].cap")
            assert np.array_equal(cap, np.array([5, 63, 17, 63, 0], dtype=f32)), cap
            assert np.array_equal(eng.read_state_field("caps[0].hits"), np.ones(n, dtype=f32))
            runs.append((bus, eng.kernel_time_ms()[1], eng.kernel_blocks_timed))
            if batching == 0:
                with pytest.raises(oscen_amd.OscenError) as err:
                    eng.set_bus_batching(33)
                assert err.value.code == oscen_amd.OG_E_INVALID and "32" in str(err.value)
                eng.set_bus_batching(32)
            eng.close()
        (bus1, l1, t1), (bus0, l0, t0) = runs
        assert (l1, t1) == (nb, nb) and (l0, t0) == (2, nb)  # 32 + 8
        for b in range(nb):
            assert np.array_equal(bus0[b], bus1[b]), b
        assert bus1[39].max() > 0.0
    finally:
        oscen_amd.unregister_node("LLOffCap::new")


def test_the_limits_of_set_bus_batching():
    eng = oscen_amd.Engine("fm_voice", N, sample_rate=SR)
    eng.set_bus_batching(LIMIT)
    with pytest.raises(oscen_amd.OscenError) as err:
        eng.set_bus_batching(LIMIT + 1)
    assert err.value.code == oscen_amd.OG_E_INVALID and str(LIMIT) in str(err.value)
    eng.set_bus_batching(1)
    eng.close()
