"""Live messages on top of a long RESIDENT score.

The reference merges the events staged for a block into it by `frame_offset`, block after block
(oscen-graph-compiler/src/codegen/mod.rs:782-871) -- a MIDI note-off costs the same whatever is going to be played later.
Here a whole score can be resident on the device (`og_schedule_*`); until round 6 a live push re-wrote the voice's remaining
score.  Now the push becomes a short segment {what is due up to the end of the launch being prepared, the push}; the
rest of the score stays where it lies as the voice's continuation, and the engine points the voice at it -- a cursor
update -- before the launch in which its first event is due (og_timeline.h, merge_voice).  Checked: the samples against the oracle fed the merged event list, the same engine with the whole list
scheduled up front bit for bit, and `og_events_copied` -- the cost of the live messages does not grow with the score."""
import numpy as np
import pytest

import oscen_amd
from tests import observed
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
SR = 48000.0


def resident_score(n, total, rng, every):
    """per voice: gate on / off pairs all the way through `total` frames, `every` frames apart on average"""
    ev = []
    for v in range(n):
        t = int(rng.integers(0, every))
        on = True
        while t < total:
            ev.append((t, v, float(np.float32(0.4 + 0.5 * rng.random())) if on else 0.0))
            on = not on
            t += int(rng.integers(every // 2, every * 3 // 2))
    return ev


def live_messages(n, blocks, block, rng, per_block):
    """(block, frame offset, voice, value): note-offs that cut a resident note short, and retriggers"""
    out = []
    for b in range(2, blocks - 1):
        for _ in range(per_block):
            out.append((b, int(rng.integers(0, block)), int(rng.integers(0, n)), 0.0 if rng.random() < 0.6 else 0.8))
    return out


def run(n, blocks, block, score, live, *, live_as_pushes, split=None, monkeypatch=None, queued=False):
    if split is not None:
        monkeypatch.setenv("OSCEN_GPU_SPLIT", str(split))
    e = oscen_amd.Engine("fm_voice", n, sample_rate=SR)
    if split is not None:
        monkeypatch.delenv("OSCEN_GPU_SPLIT")
    freqs = oscen_amd.midi_note_to_freq(np.random.default_rng(5).integers(40, 90, n)).astype(np.float32)
    e.set_voice_values("frequency", freqs)
    allev = list(score)
    if not live_as_pushes:
        allev += [(b * block + off, v, x) for b, off, v, x in live]
    # (equal frames: the resident event was there first -- it fires first; a stable sort by frame keeps that)
    allev.sort(key=lambda t: t[0])
    e.schedule_voice_events("gate", [v for _, v, _ in allev], [f for f, _, _ in allev], [x for _, _, x in allev])
    e.set_voice_taps(np.arange(n, dtype=np.uint32))
    if queued:
        e.set_bus_batching(4)
    by_block = [[] for _ in range(blocks)]
    for b, off, v, x in live:
        by_block[b].append((off, v, x))
    taps = []
    for b in range(blocks):
        if live_as_pushes:
            for off, v, x in by_block[b]:
                assert e.push_voice_event("gate", v, off, x) == 0
        if queued:
            e.process_block_async(block)
            if b % 4 == 3:
                e.flush()
                e.synchronize()
        else:
            e.process_block(block)
            taps.append(e.read_voice_taps(block))
    if queued:
        e.flush()
        e.synchronize()
    state = e.save_state()
    return e, (np.concatenate(taps, axis=1) if taps else None), state, freqs


@pytest.mark.parametrize("split", [None, 0])
def test_live_messages_cut_into_a_resident_score_without_rewriting_it(split, monkeypatch):
    n, blocks, block = 96, 24, 128
    total = blocks * block
    rng = np.random.default_rng(2026)
    score = resident_score(n, total + 200 * block, rng, every=48)  # ~64 events per voice within the run, ~530 beyond it
    live = live_messages(n, blocks, block, rng, per_block=6)
    per_voice = len(score) / n
    assert per_voice > 400

    e_live, taps_live, state_live, freqs = run(n, blocks, block, score, live, live_as_pushes=True, split=split, monkeypatch=monkeypatch)
    st = e_live.event_stats
    assert st["full_rebuilds"] == 1 and st["incremental_updates"] >= blocks - 4, st
    # the cost of the live path: every message carries over at most what was due in its own block --
    # not the ~500 events its voice still has to play (a rest below 64 events would be carried over: og_timeline.h, CONT_MIN)
    assert st["events_copied"] <= len(live) * 12, (st, len(live), per_voice)

    # the same timeline scheduled up front, one segment per voice, no continuation anywhere: bit for bit
    e_all, taps_all, state_all, _ = run(n, blocks, block, score, live, live_as_pushes=False, split=split, monkeypatch=monkeypatch)
    assert e_all.event_stats["incremental_updates"] == 0
    assert np.array_equal(taps_live, taps_all)
    dsp = e_all.state_words_per_voice * n * 4
    assert np.array_equal(state_live[:dsp], state_all[:dsp])

    # a snapshot of the live engine holds segment + continuation: a fresh engine that loads it plays on identically
    e2 = oscen_amd.Engine("fm_voice", n, sample_rate=SR)
    e2.load_state(state_live)
    e2.set_voice_taps(np.arange(n, dtype=np.uint32))
    e_live.process_block(block)
    e2.process_block(block)
    assert np.array_equal(e_live.read_voice_taps(block), e2.read_voice_taps(block))

    # against the oracle
    probe = list(range(0, n, 7))
    bank = ol.Bank(ol.BANK_FM, len(probe), SR)
    idx = {v: i for i, v in enumerate(probe)}
    for v, i in idx.items():
        bank.set_voice_frequency(i, float(freqs[v]))
    merged = list(score) + [(b * block + off, v, x) for b, off, v, x in live]
    merged.sort(key=lambda t: t[0])
    ref = []
    for b in range(blocks):
        for f, v, x in merged:
            if v in idx and b * block <= f < (b + 1) * block:
                bank.push_event(idx[v], f - b * block, ol.EV_GATE, x)
        _, t = bank.process_block(block, taps=list(range(len(probe))))
        ref.append(t)
    ref = np.concatenate(ref, axis=1)
    err = float(np.max(np.abs(taps_live[probe] - ref) / np.maximum(1.0, np.abs(ref))))
    observed.note(err)
    assert err <= 1e-5 and np.abs(ref).max() > 1e-2, err


def test_live_messages_over_a_score_on_the_queued_entry_and_through_ring_wraps(monkeypatch):
    """the asynchronous entry with the block queue on, and a ring so small that the live segments wrap around the resident
    score's continuation segments several times: same state as the all-up-front engine"""
    n, blocks, block = 200, 32, 96
    total = blocks * block
    rng = np.random.default_rng(77)
    score = resident_score(n, total + 120 * block, rng, every=40)
    live = live_messages(n, blocks, block, rng, per_block=10)
    monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
    monkeypatch.setenv("OSCEN_GPU_EV_HEADROOM", "1024")
    e_live, _, state_live, _ = run(n, blocks, block, score, live, live_as_pushes=True, queued=True)
    monkeypatch.delenv("OSCEN_GPU_EV_HEADROOM")
    e_all, _, state_all, _ = run(n, blocks, block, score, live, live_as_pushes=False, queued=True)
    dsp = e_all.state_words_per_voice * n * 4
    assert np.array_equal(state_live[:dsp], state_all[:dsp])
    assert e_live.event_stats["incremental_updates"] > 0


import os  # noqa: E402

# (soak runs: OSCEN_SOAK_SEEDS="4 5 6 ..." adds seeds; hostsim_asan.sh and a GPU session of round 6 ran 40 of them)
SEEDS = [1, 2, 3] + [int(x) for x in os.environ.get("OSCEN_SOAK_SEEDS", "").split()]


@pytest.mark.parametrize("seed", SEEDS)
def test_random_mix_of_resident_scheduled_ahead_and_live_events_equals_the_timeline_scheduled_up_front(seed, monkeypatch):
    """Differential: one engine is given the whole timeline up front; the other gets the long-range part as a resident score
    and the rest the way a player would -- block-local pushes, events scheduled a few blocks ahead (they land between
    resident ones and split continuations), a snapshot taken and loaded back half way, blocking and queued blocks mixed, a
    small ring.  No two events of a voice share a frame, so the order is the frame order in both.  Same DSP state at the end."""
    rng = np.random.default_rng(1000 + seed)
    n, blocks, block = 64, 40, 64
    if os.environ.get("OSCEN_SOAK_SCALE"):  # (soak runs: more voices, twice the blocks)
        n, blocks = 64 * int(os.environ["OSCEN_SOAK_SCALE"]), 80
    total = blocks * block
    used = [set() for _ in range(n)]

    def fresh_frame(v, lo, hi):
        for _ in range(100):
            f = int(rng.integers(lo, hi))
            if f not in used[v]:
                used[v].add(f)
                return f
        return None

    resident = []
    for v in range(n):
        for _ in range(int(rng.integers(120, 200))):  # long scores: most of it lies beyond the run
            f = fresh_frame(v, 0, total * 4)
            if f is not None:
                resident.append((f, v, float(np.float32(rng.random())) if rng.random() < 0.5 else 0.0))
    local, ahead = [], []  # (push block, frame, voice, value)
    for b in range(1, blocks):
        for _ in range(int(rng.integers(0, 8))):
            v = int(rng.integers(0, n))
            f = fresh_frame(v, b * block, (b + 1) * block)
            if f is not None:
                local.append((b, f, v, 0.0 if rng.random() < 0.5 else 0.7))
        for _ in range(int(rng.integers(0, 4))):
            v = int(rng.integers(0, n))
            f = fresh_frame(v, (b + 1) * block, min(total * 2, (b + 1 + int(rng.integers(1, 12))) * block))
            if f is not None:
                ahead.append((b, f, v, 0.0 if rng.random() < 0.5 else 0.9))
    freqs = oscen_amd.midi_note_to_freq(rng.integers(40, 90, n)).astype(np.float32)

    def schedule(e, evs):
        evs = sorted(evs, key=lambda t: t[0])
        e.schedule_voice_events("gate", [v for _, v, _ in evs], [f for f, _, _ in evs], [x for _, _, x in evs])

    a = oscen_amd.Engine("fm_voice", n, sample_rate=SR)
    a.set_voice_values("frequency", freqs)
    schedule(a, resident + [(f, v, x) for _, f, v, x in local] + [(f, v, x) for _, f, v, x in ahead])
    for _ in range(blocks):
        a.process_block(block)
    state_a = a.save_state()

    monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
    monkeypatch.setenv("OSCEN_GPU_EV_HEADROOM", "2048")
    b_eng = oscen_amd.Engine("fm_voice", n, sample_rate=SR)
    monkeypatch.delenv("OSCEN_GPU_EV_HEADROOM")
    b_eng.set_voice_values("frequency", freqs)
    schedule(b_eng, resident)
    queued = False
    for blk in range(blocks):
        if blk == blocks // 2:  # a snapshot holds segment + continuation of every voice; a fresh engine plays on from it
            if queued:
                b_eng.flush()
                b_eng.synchronize()
            blob = b_eng.save_state()
            b_eng = oscen_amd.Engine("fm_voice", n, sample_rate=SR)
            b_eng.load_state(blob)
            queued = False
        for pb, f, v, x in ahead:
            if pb == blk:
                b_eng.schedule_voice_event("gate", v, f, x)
        for pb, f, v, x in local:
            if pb == blk:
                assert b_eng.push_voice_event("gate", v, f - blk * block, x) == 0
        if blk % 7 == 3:
            b_eng.set_bus_batching(4)
            queued = True
        if blk % 7 == 6 and queued:
            b_eng.flush()
            b_eng.synchronize()
            b_eng.set_bus_batching(1)
            queued = False
        if queued:
            b_eng.process_block_async(block)
        else:
            b_eng.process_block(block)
    if queued:
        b_eng.flush()
        b_eng.synchronize()
    state_b = b_eng.save_state()
    dsp = a.state_words_per_voice * n * 4
    assert np.array_equal(state_a[:dsp], state_b[:dsp])
    assert b_eng.event_stats["incremental_updates"] > 0
