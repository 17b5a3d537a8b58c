"""The deeper zero variant (og_graph.cpp, ZeroFolds): for a launch in which fm_voice's op3_feedback, op2_feedback, route and
filter_env_amount are +-0, the operator levels are finite and no ramp ticks, the engine runs og_k*_<hash>_{00,01}z2, which
leaves out the feedback fma of op3 and op2, the crossfade and the mixer as well.  Nothing observable may change: every case
is compared BIT FOR BIT, bus and saved state, with the same run under OSCEN_GPU_ZERO2_SPEC=0 (general and `_z` kernels) and
under OSCEN_GPU_ZERO_SPEC=0 (the general kernels only) -- and og_kernel_fold_tier shows which launches ran which kernel."""
import numpy as np
import pytest

import oscen_amd

pytestmark = pytest.mark.gpu

SR = 48000.0
OPS = ("op3", "op2", "op1", "filter")
FIELDS_F = ("op3_osc.phase", "op3_osc.prev_output", "op2_osc.phase", "op2_osc.prev_output", "op1_osc.phase", "op1_osc.prev_output",
            "env3.level", "env2.level", "env1.level", "env_filter.level", "filter.current_cutoff", "filter.z0", "filter.z1")
FIELDS_U = ("env3.stage", "env3.samples_remaining", "env2.stage", "env2.samples_remaining", "env1.stage", "env1.samples_remaining")


def _engine(monkeypatch, n, mode, split=None, wide=True):
    """mode 2: every tier; 1: OSCEN_GPU_ZERO2_SPEC=0; 0: OSCEN_GPU_ZERO_SPEC=0 (no zero variant at all)"""
    monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
    monkeypatch.setenv("OSCEN_GPU_ZERO_SPEC", "1" if mode >= 1 else "0")
    monkeypatch.setenv("OSCEN_GPU_ZERO2_SPEC", "1" if mode >= 2 else "0")
    if split is None:
        monkeypatch.delenv("OSCEN_GPU_SPLIT", raising=False)
        monkeypatch.delenv("OSCEN_GPU_WIDE", raising=False)
    else:
        monkeypatch.setenv("OSCEN_GPU_SPLIT", str(split))
        monkeypatch.setenv("OSCEN_GPU_WIDE", "1" if split == 4 and wide else "0")
    return oscen_amd.Engine("fm_voice", n, sample_rate=SR)


def _notes(eng, n, frames, seed=3, short=False):
    rng = np.random.default_rng(seed)
    eng.set_voice_values("frequency", (110.0 * 2.0 ** (rng.integers(0, 36, n) / 12.0)).astype(np.float32))
    if short:  # envelope stages end every few hundred frames: gate events fall into chunks with stage ends
        for op in OPS:
            eng.set_value(op + "_attack", 0.002)
            eng.set_value(op + "_decay", 0.004)
            eng.set_value(op + "_release", 0.006)
    t = 0
    while t < frames:
        on = t + rng.integers(0, 400, n)
        off = on + rng.integers(50, 900, n)
        for v in range(n):
            if on[v] < frames:
                eng.schedule_voice_event("gate", v, int(on[v]), float(rng.uniform(0.3, 1.0)))
            if off[v] < frames:
                eng.schedule_voice_event("gate", v, int(off[v]), 0.0)
        t += 1000


def _run(monkeypatch, n, mode, blocks, sets=None, split=None, wide=True, short=False, ramp=None, fields=False, snapshot=None):
    """blocks: frames per process_block call (one launch each); sets: {block index: {input: value}}, set at once; ramp:
    (block, input, value, frames).  Also returns the tier each block's launch ran and its kernel name."""
    eng = _engine(monkeypatch, n, mode, split, wide)
    try:
        total = int(sum(blocks))
        _notes(eng, n, total, short=short)
        out, state_mid, tiers, names = [], None, [], []
        for bi, frames in enumerate(blocks):
            for name, value in (sets or {}).get(bi, {}).items():
                eng.set_value_immediate(name, value)
                assert np.float32(eng.get_value(name)).view(np.uint32) == np.float32(value).view(np.uint32)
            if ramp and ramp[0] == bi:
                eng.set_value_with_ramp(ramp[1], ramp[2], ramp[3])
            if snapshot is not None and bi == snapshot:
                blob = eng.save_state()
                state_mid = bytes(blob)
                eng.load_state(blob)
            out.append(np.array(eng.process_block(frames)))
            tiers.append(eng.kernel_fold_tier)
            names.append(eng.kernel_variant)
        res = {"bus": np.concatenate(out), "state": bytes(eng.save_state()), "mid": state_mid}
        if fields:
            for f in FIELDS_F:
                res[f] = eng.read_state_field(f).view(np.uint32)
            for f in FIELDS_U:
                res[f] = eng.read_state_field(f, dtype=np.uint32)
        return res, tiers, names
    finally:
        eng.close()


def _same(monkeypatch, n, blocks, sound=True, **kw):
    """bit-equal runs in the three modes; returns the tier of every block in the run with every tier on"""
    ref, ref_t, ref_n = _run(monkeypatch, n, 0, blocks, **kw)
    assert ref_t == [0] * len(blocks) and not any(k.endswith("_z") for k in ref_n), (ref_t, ref_n)
    if sound:
        assert np.max(np.abs(ref["bus"])) > 1e-3  # (the notes sound)
    tiers = None
    for mode in (1, 2):
        got, got_t, got_n = _run(monkeypatch, n, mode, blocks, **kw)
        assert np.array_equal(got["bus"].view(np.uint32), ref["bus"].view(np.uint32)), (mode, int(np.sum(got["bus"].view(np.uint32) != ref["bus"].view(np.uint32))))
        for k in ref:
            if k != "bus":
                assert (got[k] == ref[k]) if isinstance(ref[k], (bytes, type(None))) else np.array_equal(got[k], ref[k]), (mode, k)
        # og_kernel_name: the general name + "_z" after a launch of either variant, the same shape
        assert [k[:-2] if t else k for k, t in zip(got_n, got_t)] == ref_n and all(k.endswith("_z") == (t > 0) for k, t in zip(got_n, got_t))
        if mode == 1:
            assert max(got_t) <= 1, got_t
            tier1 = got_t
        else:
            assert [min(t, 1) for t in got_t] == tier1, (got_t, tier1)  # (where tier 2 runs, `_z` ran without it)
            tiers = got_t
    return tiers


def test_the_timed_configuration_shape(monkeypatch):
    # 65 536 voices (the wide four-wave kernel) at the default patch, 256-frame blocks: every launch runs the deeper variant
    assert _same(monkeypatch, 65536, [256] * 6) == [2] * 6


def test_the_ordinary_kernel_at_262144_voices(monkeypatch):
    assert _same(monkeypatch, 262144, [256] * 3) == [2] * 3


@pytest.mark.parametrize("split,wide", [(0, False), (2, False), (4, False), (4, True)])
def test_every_shape_with_gate_events_next_to_stage_ends(monkeypatch, split, wide):
    t = _same(monkeypatch, 200, [256, 500, 17, 333, 511, 1, 480, 512], split=split, wide=wide, short=True, fields=True)
    assert t == [2] * 8, t


@pytest.mark.parametrize("name,value,between", [("op3_feedback", 0.3, 1), ("op2_feedback", 0.2, 1), ("route", 0.4, 1), ("filter_env_amount", 0.5, 0)])
def test_one_slot_switched_between_blocks(monkeypatch, name, value, between):
    # 0 -> non-zero -> 0: a feedback or the route leaves the deeper variant for `_z`, the amount leaves both; then back
    t = _same(monkeypatch, 200, [256] * 8, sets={3: {name: value}, 5: {name: 0.0}}, split=4, short=True, fields=True)
    assert t == [2, 2, 2, between, between, 2, 2, 2], t


@pytest.mark.parametrize("name", ["op3_feedback", "op2_feedback", "route", "filter_env_amount"])
def test_a_negative_zero_in_each_slot(monkeypatch, name):
    assert _same(monkeypatch, 200, [256] * 4, sets={0: {name: -0.0}}, split=4, short=True, fields=True) == [2] * 4
    assert _same(monkeypatch, 200, [256] * 2, sets={0: {name: -0.0}}, split=0, short=True, fields=True) == [2] * 2


def test_a_route_ramp_that_ends_at_zero_inside_a_launch(monkeypatch):
    # from 0.5 down to 0 over 300 frames (blocks 1 and 2): those launches tick the ramp and run the general (table) kernel,
    # block 0 has route 0.5 (`_z`), the ones after the ramp the deeper variant
    t = _same(monkeypatch, 200, [256] * 6, sets={0: {"route": 0.5}}, ramp=(1, "route", 0.0, 300), split=4, short=True, fields=True)
    assert t == [1, 0, 0, 2, 2, 2], t


def test_a_snapshot_saved_and_loaded_across_launches_of_the_deeper_variant(monkeypatch):
    assert _same(monkeypatch, 200, [256] * 6, split=4, short=True, fields=True, snapshot=3) == [2] * 6


def test_an_infinite_level_leaves_the_deeper_variant_by_its_guard(monkeypatch):
    # op2_level = inf: op2's output is inf or NaN, the general kernel's feedback fma turns prev_output * 0 into NaN; the guard
    # keeps such a launch -- and, because the NaN stays in prev_output, every later one -- off the deeper variant
    t = _same(monkeypatch, 200, [256] * 6, sound=False, sets={2: {"op2_level": float("inf")}, 4: {"op2_level": 1.0}}, split=4, short=True,
              fields=True)
    assert t == [2, 2, 1, 1, 1, 1], t
