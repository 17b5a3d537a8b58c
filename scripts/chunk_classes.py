"""Chunk classes of the headline's timed region (a MODEL from the note plan, not a measurement): which body each envelope
stage of the wide four-wave fm kernel runs in every 16-frame chunk of `python bench.py` -- event chunk, stage-end chunk, hold,
pure release, quiet without / with release -- and how many of a slow chunk's four quarters hold its hits.

As bench.py schedules it: the 1 s plan of every voice, played again every 48 000 frames; 889 warm-up blocks of 256 frames, then
the region of 188 blocks; og_group_voices policy 1 (voice slots ordered by first note-off, then first event); 64 slots a wave;
chunks aligned to the launch.  Stage lengths in frames (attack, decay, release): 480 / 4 800 / 14 400 for env3, env2 and the
filter envelope, 480 / 9 600 / 24 000 for env1.  An envelope entered at frame f with n frames to go ends its stage in the tick
of frame f + n - 1.  scripts/group_model.py is the older model of 8-frame chunks and of the grouping policies.

    python scripts/chunk_classes.py [voices]        (default 65536; a few seconds)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oscen_amd  # noqa: E402

V = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
BLOCK, WARM, STEPS, XCH = 256, 889, 188, 16
F0, T = WARM * BLOCK, (WARM + STEPS) * BLOCK
NCH = (T - F0) // XCH
E_OP, E_1 = (480, 4800, 14400), (480, 9600, 24000)
STAGES = {"0, 1 (one envelope)": [E_OP], "2 (env1 + filter envelope)": [E_1, E_OP]}
WG = V // 64

plans = oscen_amd.note_plans(V, span=48000, fold="slice")
ev_v, ev_f, ev_x = plans["events"]
reps = -(-T // 48000)
ev_v, ev_f, ev_x = np.tile(ev_v, reps), np.concatenate([ev_f + 48000 * k for k in range(reps)]), np.tile(ev_x, reps)
order = np.lexsort((ev_f, ev_v))
ev_v, ev_f, ev_x = ev_v[order], ev_f[order].astype(np.int64), ev_x[order]
nxt = np.where(np.append(ev_v[1:] == ev_v[:-1], False), np.append(ev_f[1:], 0), 1 << 40)  # the voice's next event
# policy 1: slot of every voice
first_off = np.full(V, 1 << 40, dtype=np.int64)
np.minimum.at(first_off, ev_v[ev_x <= 0], ev_f[ev_x <= 0])
first_any = np.full(V, 1 << 40, dtype=np.int64)
np.minimum.at(first_any, ev_v, ev_f)
slot = np.empty(V, dtype=np.int64)
slot[np.lexsort((first_any, first_off))] = np.arange(V)
wave = slot[ev_v] // 64


def chunk_of(f):  # the chunk whose frames hold f, -1 outside the region
    c = (f - F0) // XCH
    return np.where((f >= F0) & (f < T), c, -1)


def first_chunk_from(f):  # the first chunk that STARTS at or after frame f, clipped to the region
    return np.clip(-(-(f - F0) // XCH), 0, NCH)


def mark(grid, w, c, quarter=None, f=None):
    ok = c >= 0
    np.add.at(grid, (w[ok], c[ok]), 1)
    if quarter is not None:
        np.add.at(quarter, (w[ok], c[ok], ((f[ok] - F0) % XCH) // 4), 1)


def paint(grid, w, a, b):  # +1 over the chunks that start inside [a, b)
    lo, hi = first_chunk_from(a), first_chunk_from(b)
    np.add.at(grid, (w, lo), 1)
    np.add.at(grid, (w, hi), -1)


def classes(envs):
    events = np.zeros((WG, NCH), dtype=np.int32)
    ends = np.zeros((WG, NCH), dtype=np.int32)
    hitq = np.zeros((WG, NCH, 4), dtype=np.int32)
    mark(events, wave, chunk_of(ev_f), hitq, ev_f)
    rel = np.zeros((WG, NCH + 1), dtype=np.int32)   # envelopes of the wave in Release at the chunk's first frame
    mov = np.zeros((WG, NCH + 1), dtype=np.int32)   # ... in Attack or Decay
    on = ev_x > 0
    for (A, D, R) in envs:
        a_end, d_end, r_end = ev_f + A - 1, ev_f + A + D - 1, ev_f + R - 1
        for sel, end in ((on & (a_end < nxt), a_end), (on & (d_end < nxt), d_end), (~on & (r_end < nxt), r_end)):
            mark(ends, wave[sel], chunk_of(end[sel]), hitq, end[sel])
        paint(mov, wave[on], ev_f[on] + 1, np.minimum(d_end[on] + 1, nxt[on] + 1))
        paint(rel, wave[~on], ev_f[~on] + 1, np.minimum(r_end[~on] + 1, nxt[~on] + 1))
    rel, mov = np.cumsum(rel, axis=1)[:, :NCH], np.cumsum(mov, axis=1)[:, :NCH]
    lanes = 64 * len(envs)
    ev = events > 0
    end = ~ev & (ends > 0)
    quiet = ~ev & ~end
    out = {"event chunk": ev, "stage-end chunk": end, "hold": quiet & (rel == 0) & (mov == 0), "pure release": quiet & (rel == lanes),
           "quiet, no release": quiet & (rel == 0) & (mov > 0), "quiet release": quiet & (rel > 0) & (rel < lanes)}
    return out, hitq


for name, envs in STAGES.items():
    cls, hitq = classes(envs)
    print("stage %s: shares of the %d chunks x %d waves" % (name, NCH, WG))
    print("   " + "   ".join("%s %.1f %%" % (k, 100.0 * v.mean()) for k, v in cls.items()))
    slow = cls["event chunk"] | cls["stage-end chunk"]
    per_block = BLOCK // XCH
    for b0, b1 in ((0, 32), (32, 64), (64, STEPS)):
        s = slow[:, b0 * per_block:b1 * per_block].mean(axis=1)
        print("   blocks %3d-%3d: slow chunks per wave, mean %.1f %%, busiest wave %.1f %%" % (b0, b1 - 1, 100 * s.mean(), 100 * s.max()))
    nq = (hitq > 0).sum(axis=2)[slow]
    print("   quarters with a hit in a slow chunk: " + "  ".join("%d: %.1f %%" % (k, 100.0 * np.mean(nq == k)) for k in range(1, 5))
          + "   -> %.1f %% of the quarters of slow chunks can run quiet" % (100.0 * (1 - nq.mean() / 4)))
    outside = slow.copy()
    outside[:, ((np.arange(NCH) * XCH + F0) % 48000) < 256] = False  # (the on-window: the first 256 frames of every second)
    nqo = (hitq > 0).sum(axis=2)[outside]
    print("   ... outside the on-window: %d slow chunks, %.2f quarters hit on average" % (nqo.size, nqo.mean()))
    tab = cls["pure release"] | cls["quiet release"]
    entries = (tab[:, 1:] & ~tab[:, :-1]).sum(axis=1) + tab[:, 0]
    print("   entries into a release (table) loop per wave: mean %.1f, most %d" % (entries.mean(), entries.max()))
