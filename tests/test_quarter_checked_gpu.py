"""The quiet quarters of a checked chunk (og_graph.cpp, PipelineWave::checked; og_stage_uniform.hip.h has the argument): in the
wide four-wave kernels of the deeper zero variant a chunk with an event or an envelope stage end runs as four quarters of four
frames, and a quarter in which no lane has an event and no countdown can end runs without the event and stage-end tests.
Nothing observable may change: every case is compared BIT FOR BIT, bus and saved state, with the general kernels
(OSCEN_GPU_ZERO_SPEC=0).  On the host simulator (tests/test_quarter_checked_cpu.py runs this file there) the library counts the
quarters of both kinds per stage, and the single-hit cases assert one checked and three quiet quarters per wave.

200 voices = four workgroups (every rotation of the stages over the waves, the last workgroup partly empty), blocks of 96 frames
= six chunks of 16; the events sit in the third chunk (frames 32..47) unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import oscen_amd

pytestmark = pytest.mark.gpu

N = 200
WAVES = (N + 63) // 64
SR = 48000.0
OPS = ("op3", "op2", "op1", "filter")
LONG = {"attack": 300, "decay": 300, "release": 300}  # frames: no stage ends inside the short runs


def _counts():
    """quarters per stage run (without, with) their tests so far -- host simulator only, None on a device"""
    try:
        a = (C.c_ulonglong * 16).in_dll(oscen_amd.load_library(), "og_checked_quarters")
    except ValueError:
        return None
    return np.array(a[:], dtype=np.uint64).reshape(2, 8).astype(np.int64)


def _all(frame):
    return np.full(N, frame, dtype=np.int64)


def _run(monkeypatch, general, events, times=None, blocks=(96, 96, 96), cap=None, offline=False, taps=None):
    """times: frames per stage, one value for every operator or {operator: frames}"""
    monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
    monkeypatch.setenv("OSCEN_GPU_ZERO_SPEC", "0" if general else "1")
    monkeypatch.setenv("OSCEN_GPU_ZERO2_SPEC", "0" if general else "1")
    monkeypatch.setenv("OSCEN_GPU_STAGE_SPEC", "1")
    monkeypatch.setenv("OSCEN_GPU_SPLIT", "4")
    monkeypatch.setenv("OSCEN_GPU_WIDE", "1")
    if cap is None:
        monkeypatch.delenv("OSCEN_GPU_RCP_CAP", raising=False)
    else:
        monkeypatch.setenv("OSCEN_GPU_RCP_CAP", str(cap))
    total = sum(blocks)
    eng = oscen_amd.Engine("fm_voice", N, sample_rate=SR)
    try:
        assert eng.kernel_variant.startswith("og_k4w_"), eng.kernel_variant
        rng = np.random.default_rng(14)
        eng.set_voice_values("frequency", (110.0 * 2.0 ** (rng.integers(0, 36, N) / 12.0)).astype(np.float32))
        for stage, frames in dict(LONG, **(times or {})).items():
            for op in OPS:
                n = frames[op] if isinstance(frames, dict) else frames
                eng.set_value(op + "_" + stage, (n + 0.5) / SR)
        for frames, value in events:
            for v in range(N):
                if frames[v] < total:
                    eng.schedule_voice_event("gate", v, int(frames[v]), float(value))
        if taps is not None:
            eng.set_voice_taps(taps)
        out, tapped, tiers = [], [], []
        if offline:  # the queued path: the blocks in one launch
            out.append(np.array(eng.render(total, blocks[0])))
            tiers.append(eng.kernel_fold_tier)
        else:
            for frames in blocks:
                out.append(np.array(eng.process_block(frames)))
                tiers.append(eng.kernel_fold_tier)
                if taps is not None:
                    tapped.append(np.array(eng.read_voice_taps(frames)))
        assert tiers == [0 if general else 2] * len(tiers), (general, tiers)
        return {"bus": np.concatenate(out), "state": bytes(eng.save_state()), "taps": np.concatenate(tapped, axis=1) if tapped else None}
    finally:
        eng.close()


_REF = {}


def _general(monkeypatch, key, **kw):
    """the general kernels' run of a case: computed once, shared by the tests that compare with it"""
    if key not in _REF:
        ref = _run(monkeypatch, True, **kw)
        assert np.max(np.abs(ref["bus"])) > 1e-3  # (the notes sound)
        ref["bus"].setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _same(monkeypatch, key, general_kw=None, **kw):
    ref = _general(monkeypatch, key, **(kw if general_kw is None else general_kw))
    before = _counts()
    got = _run(monkeypatch, False, **kw)
    after = _counts()
    diff = int(np.sum(got["bus"].view(np.uint32) != ref["bus"].view(np.uint32)))
    print(key, "bus words that differ:", diff, "quarters (quiet, checked) per stage:", None if after is None else (after - before)[:, :4].tolist())
    assert diff == 0, (key, diff)
    assert got["state"] == ref["state"], key
    if ref["taps"] is not None:
        assert np.array_equal(got["taps"].view(np.uint32), ref["taps"].view(np.uint32)), key
    return None if after is None else after - before


@pytest.mark.parametrize("quarter", [0, 1, 2, 3])
def test_one_event_in_each_quarter_of_a_chunk(monkeypatch, quarter):
    # every voice: gate on at the second frame of quarter `quarter` of the third chunk, nothing else in the run
    ran = _same(monkeypatch, "one%d" % quarter, events=[(_all(32 + 4 * quarter + 1), 0.9)])
    if ran is not None:  # (host simulator) one slow chunk per wave: one checked, three quiet quarters in each operator stage
        assert ran[1, :3].tolist() == [WAVES] * 3 and ran[0, :3].tolist() == [3 * WAVES] * 3, ran
        assert (ran[:, 3:] == 0).all(), ran  # the filter stage has no envelope and no quarters


def test_an_event_on_the_last_frame_of_a_quarter_and_on_the_first_of_the_next(monkeypatch):
    lane = np.arange(N) % 64
    ran = _same(monkeypatch, "edge", events=[(np.where(lane % 2 == 0, 35, 36), 0.9)])
    if ran is not None:  # two checked quarters, two quiet ones
        assert ran[1, :3].tolist() == [2 * WAVES] * 3 and ran[0, :3].tolist() == [2 * WAVES] * 3, ran


def test_two_events_of_one_lane_in_one_chunk(monkeypatch):
    # on and off ten frames apart (two quarters), in lane 5 two frames apart (one quarter), in lane 9 on neighbouring frames
    lane = np.arange(N) % 64
    off = np.where(lane == 5, 35, np.where(lane == 9, 34, 43))
    _same(monkeypatch, "two", events=[(_all(33), 0.9), (off, 0.0)])


def test_an_event_in_every_quarter(monkeypatch):
    # even lanes: on, off, on, off in the four quarters of one chunk; odd lanes: one note-on, in the quarter the lane number picks
    lane = np.arange(N) % 64
    even = lane % 2 == 0
    never = _all(1 << 30)
    ev = [(np.where(even, 33, 32 + 4 * (lane // 2 % 4) + 2), 0.9), (np.where(even, 38, never), 0.0), (np.where(even, 41, never), 0.8),
          (np.where(even, 47, never), 0.0)]
    ran = _same(monkeypatch, "every", events=ev)
    if ran is not None:
        assert (ran[1, :3] >= 4 * WAVES).all(), ran  # every quarter of that chunk is checked


SHORT = {"attack": {"op3": 5, "op2": 11, "op1": 22, "filter": 37}, "decay": {"op3": 40, "op2": 23, "op1": 9, "filter": 6},
         "release": {"op3": 7, "op2": 18, "op1": 29, "filter": 40}}


def _short_events():
    # note-ons spread over a chunk's sixteen frames by lane, note-offs likewise: with stages of 5..40 frames the stage ends of the
    # four envelopes fall into every quarter, alone and together with other lanes' events
    lane = np.arange(N) % 64
    return [(32 + lane % 16, 0.9), (200 + (lane * 5) % 16, 0.0), (420 + lane % 3, 0.7), (560 + lane % 16, 0.0)]


MIXED = dict(events=_short_events(), times=SHORT, blocks=(96,) * 8)


def test_stage_ends_in_every_quarter(monkeypatch):
    ran = _same(monkeypatch, "short", **MIXED)
    if ran is not None:
        assert (ran[:, :3] > 0).all(), ran  # both kinds ran in each operator stage


def test_a_stage_entered_and_ended_inside_one_chunk(monkeypatch):
    # attack of 3 frames: entered at 33 (quarter 0), over at 36 (quarter 1); the decay of 6 ends in quarter 2
    _same(monkeypatch, "inside", events=[(_all(33), 0.9), (_all(150), 0.0)], times={"attack": 3, "decay": 6, "release": 12})


def test_a_note_off_one_frame_before_a_release_end(monkeypatch):
    # release of 20 frames from 100: it would end on frame 119 / 120; a second note-off one frame earlier starts it again
    lane = np.arange(N) % 64
    again = np.where(lane % 2 == 0, 118, 119)
    _same(monkeypatch, "offagain", events=[(_all(10), 0.9), (_all(100), 0.0), (again, 0.0)], times={"attack": 8, "decay": 12, "release": 20})


def test_a_reciprocal_table_too_short(monkeypatch):
    # a table capped at 100 entries does not cover releases of 300 frames: rcp_len = 0 sends the wide form's release chunks to
    # the checked body, whose quarters then all run quiet, with the v_rcp_f32 form of the release
    kw = dict(events=[(_all(37), 0.9), (_all(120), 0.0)], blocks=(96,) * 4)
    ran = _same(monkeypatch, "cap", general_kw=kw, cap=100, **kw)
    if ran is not None:
        assert (ran[0, :3] > 8 * 4 * WAVES).all(), ran  # (more than eight whole chunks of quiet quarters per wave)


def test_eight_blocks_in_one_launch(monkeypatch):
    _same(monkeypatch, "short", general_kw=MIXED, offline=True, **MIXED)


def test_the_tapped_kernel(monkeypatch):
    # og_k4w_*_01z2: per-voice taps next to the bus
    _same(monkeypatch, "taps", taps=list(range(0, N, 7)), **MIXED)
