"""Stage-uniform envelope bodies of the deeper zero variant's four-wave pipeline (og_stage_uniform.hip.h; og_graph.cpp,
PipelineWave::fast_variants): a wave whose envelopes all hold (Sustain / Idle) or all release, in every lane, runs a quiet body
without the arithmetic that is known in advance.  Nothing observable may change: every case is compared BIT FOR BIT, bus and
saved state, with the general kernels (OSCEN_GPU_ZERO_SPEC=0); the first case also with the deeper variant whose bodies are
switched off (OSCEN_GPU_STAGE_SPEC=0).  On the host simulator (tests/test_stage_uniform_env_cpu.py runs this file there) the
library counts the chunks each stage ran in the two bodies, and the first case asserts that they ran.

300 voices = five workgroups (every rotation of the stages over the waves, the last workgroup partly empty), 8 blocks of 256
frames, envelope times of a few hundred frames so that every stage is crossed in every case."""
import ctypes as C

import numpy as np
import pytest

import oscen_amd

pytestmark = pytest.mark.gpu

N = 300
SR = 48000.0
BLOCKS = [256] * 8
TOTAL = sum(BLOCKS)
OPS = ("op3", "op2", "op1", "filter")
# attack 96, decay 192 frames; releases of 480 (op3, op2, filter) and 960 frames (op1): stage 2 -- env1 and env_filter -- is in
# pure release only while both release
TIMES = {"attack": 0.002, "decay": 0.004}
RELEASE = {"op3": 0.01, "op2": 0.01, "op1": 0.02, "filter": 0.01}

GENERAL, BODIES_OFF, BODIES_ON = "general", "off", "on"


def _counts():
    """chunks per stage in the (hold, pure-release) bodies so far -- host simulator only, None on a device"""
    try:
        a = (C.c_ulonglong * 16).in_dll(oscen_amd.load_library(), "og_stage_uniform_chunks")
    except ValueError:
        return None
    return np.array(a[:], dtype=np.uint64).reshape(2, 8).copy()


def _one_schedule(n):
    """every voice: on at 10, off at 700 -- Sustain from 298, Release until 1180 / 1660, Idle behind it"""
    return [(np.full(n, 10), 0.9), (np.full(n, 700), 0.0)]


def _run(monkeypatch, mode, events=None, split=4, wide=True, sets=None, cap=None, offline=False, taps=None, blocks=BLOCKS):
    monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
    monkeypatch.setenv("OSCEN_GPU_ZERO_SPEC", "0" if mode == GENERAL else "1")
    monkeypatch.setenv("OSCEN_GPU_ZERO2_SPEC", "0" if mode == GENERAL else "1")
    monkeypatch.setenv("OSCEN_GPU_STAGE_SPEC", "1" if mode == BODIES_ON else "0")
    monkeypatch.setenv("OSCEN_GPU_SPLIT", str(split))
    monkeypatch.setenv("OSCEN_GPU_WIDE", "1" if split == 4 and wide else "0")
    if cap is None:
        monkeypatch.delenv("OSCEN_GPU_RCP_CAP", raising=False)
    else:
        monkeypatch.setenv("OSCEN_GPU_RCP_CAP", str(cap))
    eng = oscen_amd.Engine("fm_voice", N, sample_rate=SR)
    try:
        shape = "og_k4w_" if split == 4 and wide else "og_k4_"
        assert eng.kernel_variant.startswith(shape), eng.kernel_variant
        rng = np.random.default_rng(11)
        eng.set_voice_values("frequency", (110.0 * 2.0 ** (rng.integers(0, 36, N) / 12.0)).astype(np.float32))
        for op in OPS:
            for k, v in TIMES.items():
                eng.set_value(op + "_" + k, v)
            eng.set_value(op + "_release", RELEASE[op])
        for name, value in (sets or {}).items():
            eng.set_value_immediate(name, value)
            assert np.float32(eng.get_value(name)).view(np.uint32) == np.float32(value).view(np.uint32)
        for frames, value in (events if events is not None else _one_schedule(N)):
            for v in range(N):
                if frames[v] < TOTAL:
                    eng.schedule_voice_event("gate", v, int(frames[v]), float(value))
        if taps is not None:
            eng.set_voice_taps(taps)
        out, tapped, tiers = [], [], []
        if offline:  # the queued path: the eight blocks in one launch
            out.append(np.array(eng.render(TOTAL, 256)))
            tiers.append(eng.kernel_fold_tier)
        else:
            for frames in blocks:
                out.append(np.array(eng.process_block(frames)))
                tiers.append(eng.kernel_fold_tier)
                if taps is not None:
                    tapped.append(np.array(eng.read_voice_taps(frames)))
        assert tiers == [0 if mode == GENERAL else 2] * len(tiers), (mode, tiers)
        return {"bus": np.concatenate(out), "state": bytes(eng.save_state()), "taps": np.concatenate(tapped, axis=1) if tapped else None}
    finally:
        eng.close()


_REF = {}


def _general(monkeypatch, key, **kw):
    """the general kernels' run of a case: computed once, shared by the tests that compare with it"""
    if key not in _REF:
        ref = _run(monkeypatch, GENERAL, **kw)
        assert np.max(np.abs(ref["bus"])) > 1e-3  # (the notes sound)
        ref["bus"].setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _equal(got, ref, what):
    assert np.array_equal(got["bus"].view(np.uint32), ref["bus"].view(np.uint32)), (what, int(np.sum(got["bus"].view(np.uint32) != ref["bus"].view(np.uint32))))
    assert got["state"] == ref["state"], what
    if ref["taps"] is not None:
        assert np.array_equal(got["taps"].view(np.uint32), ref["taps"].view(np.uint32)), what


def _same(monkeypatch, key, general_kw=None, **kw):
    ref = _general(monkeypatch, key, **(kw if general_kw is None else general_kw))
    _equal(_run(monkeypatch, BODIES_ON, **kw), ref, key)


def test_every_voice_on_one_schedule(monkeypatch):
    # (a) the hold and the release bodies dominate: every wave is uniform but for the chunks with the gate and the stage ends
    ref = _general(monkeypatch, "one")
    _equal(_run(monkeypatch, BODIES_OFF), ref, "bodies off")
    before = _counts()
    _equal(_run(monkeypatch, BODIES_ON), ref, "bodies on")
    after = _counts()
    if after is not None:  # (host simulator)
        ran = after - before
        assert (ran[:, :3] > 0).all(), ran  # both bodies in each of the three operator stages
        assert (ran[:, 3:] == 0).all(), ran  # the filter stage has no envelope
        idle = _counts()
        _run(monkeypatch, BODIES_OFF)
        assert np.array_equal(_counts(), idle)  # switched off, they do not run


def test_one_lane_per_wave_a_chunk_late_and_one_a_frame_late(monkeypatch):
    # (b) mixed <-> uniform at both edges of Sustain, Release and Idle: in every wave lane 5 runs 16 frames behind the others
    # and lane 9 one frame behind
    lane = np.arange(N) % 64
    shift = np.where(lane == 5, 16, np.where(lane == 9, 1, 0))
    _same(monkeypatch, "late", events=[(10 + shift, 0.9), (704 + shift, 0.0)])


@pytest.mark.parametrize("sustain", [0.0, -0.0], ids=["plus0", "minus0"])
def test_a_sustain_of_zero(monkeypatch, sustain):
    # (c) Decay ends on the sustain level: +0 is held by the hold body, -0 must keep the general one (fma(.., +0, -0) is +0)
    sets = {op + "_sustain": sustain for op in OPS}
    _same(monkeypatch, "sustain%s" % np.float32(sustain).view(np.uint32), sets=sets)


def test_a_retrigger_in_the_middle_of_release(monkeypatch):
    # (d) pure release, left by a gate-on at a level between 0 and 1, then the whole cycle again
    n = np.ones(N, dtype=np.int64)
    _same(monkeypatch, "retrigger", events=[(10 * n, 0.9), (500 * n, 0.0), (700 * n, 0.7), (1300 * n, 0.0)])


def test_a_release_longer_than_the_reciprocal_table(monkeypatch):
    # (e) a table capped at 100 entries does not cover the 480-frame releases: rcp_len = 0 sends the release chunks of the wide
    # form to the checked body; the hold body still runs
    _same(monkeypatch, "one", general_kw={}, cap=100)


def test_eight_blocks_in_one_launch(monkeypatch):
    # (f) the queued path (og_render: the eight blocks in one launch) against eight blocking launches of the general kernel
    _same(monkeypatch, "one", general_kw={}, offline=True)


def test_the_tapped_variant(monkeypatch):
    # (g) og_k4w_*_01z2: per-voice taps next to the bus
    _same(monkeypatch, "taps", taps=list(range(0, N, 7)))


def test_the_eight_frame_form(monkeypatch):
    # (h) og_k4_*_00z2: 8-frame hand-offs behind a barrier, release reciprocals from v_rcp_f32
    lane = np.arange(N) % 64
    shift = np.where(lane == 5, 8, np.where(lane == 9, 1, 0))
    _same(monkeypatch, "narrow", events=[(10 + shift, 0.9), (704 + shift, 0.0)], wide=False)
