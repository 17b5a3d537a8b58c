"""The zero variant (og_graph.cpp, ZeroChain): for a launch in which fm_voice's filter_env_amount is +-0 and no ramp ticks,
the engine runs og_k*_<hash>_{00,01}z, which leaves out `env_filter * filter_env_amount + filter_cutoff` and updates the
filter's coefficients once at the top of the launch.  Nothing observable may change: every case is compared BIT FOR BIT,
bus and saved state, with the same run under OSCEN_GPU_ZERO_SPEC=0 (the general kernels only) -- and the kernel name
(og_kernel_name: `_z` after a launch of the zero variant) shows which launches ran it."""
import numpy as np
import pytest

import oscen_amd

pytestmark = pytest.mark.gpu

SR = 48000.0
OPS = ("op3", "op2", "op1", "filter")


def _engine(monkeypatch, n, zero, split=None, wide=True):
    monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
    monkeypatch.setenv("OSCEN_GPU_ZERO_SPEC", "1" if zero else "0")
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


def _run(monkeypatch, n, zero, blocks, amounts=None, split=None, wide=True, short=False, ramp=None, fields=False, snapshot=None):
    """blocks: frames per process_block call (one launch each); amounts: {block index: filter_env_amount}, set at once (a
    ramp from +0.0 to -0.0 would be no change); ramp: (block, value, frames).  Also returns the kernel each block ran."""
    eng = _engine(monkeypatch, n, zero, split, wide)
    try:
        total = int(sum(blocks))
        _notes(eng, n, total, short=short)
        out, state_mid, kernels = [], None, []
        for bi, frames in enumerate(blocks):
            if amounts and bi in amounts:
                eng.set_value_immediate("filter_env_amount", amounts[bi])
                assert np.float32(eng.get_value("filter_env_amount")).view(np.uint32) == np.float32(amounts[bi]).view(np.uint32)
            if ramp and ramp[0] == bi:
                eng.set_value_with_ramp("filter_env_amount", ramp[1], ramp[2])
            if snapshot is not None and bi == snapshot:
                blob = eng.save_state()
                state_mid = bytes(blob)
                eng.load_state(blob)
            out.append(np.array(eng.process_block(frames)))
            kernels.append(eng.kernel_variant)
        res = {"bus": np.concatenate(out), "state": bytes(eng.save_state()), "mid": state_mid}
        if fields:
            for f in ("env_filter.level", "env_filter.velocity", "filter.current_cutoff", "filter.current_q", "filter.h", "filter.g",
                      "filter.k", "filter.z0", "filter.z1"):
                res[f] = eng.read_state_field(f).view(np.uint32)
            for f in ("env_filter.stage", "env_filter.samples_remaining"):
                res[f] = eng.read_state_field(f, dtype=np.uint32)
        return res, kernels
    finally:
        eng.close()


def _same(monkeypatch, n, blocks, **kw):
    """bit-equal runs; returns which blocks ran the zero kernel"""
    ref, ref_k = _run(monkeypatch, n, False, blocks, **kw)
    got, got_k = _run(monkeypatch, n, True, blocks, **kw)
    assert np.max(np.abs(ref["bus"])) > 1e-3  # (the notes sound)
    assert np.array_equal(got["bus"].view(np.uint32), ref["bus"].view(np.uint32)), int(np.sum(got["bus"] != ref["bus"]))
    for k in ref:
        if k != "bus":
            assert (got[k] == ref[k]) if isinstance(ref[k], (bytes, type(None))) else np.array_equal(got[k], ref[k]), k
    assert not any(k.endswith("_z") for k in ref_k), ref_k  # (OSCEN_GPU_ZERO_SPEC=0: never)
    assert [k[:-2] if k.endswith("_z") else k for k in got_k] == ref_k  # (the same shape)
    return [k.endswith("_z") for k in got_k]


def test_the_timed_configuration_shape(monkeypatch):
    # 65 536 voices (the wide four-wave kernel) at the default patch (amount 0), 256-frame blocks: every launch is a zero one
    assert _same(monkeypatch, 65536, [256] * 6) == [True] * 6


def test_the_ordinary_kernel_at_262144_voices(monkeypatch):
    assert _same(monkeypatch, 262144, [256] * 3) == [True] * 3


@pytest.mark.parametrize("split", [0, 2, 4])
def test_every_shape_with_gate_events_next_to_stage_ends(monkeypatch, split):
    assert all(_same(monkeypatch, 200, [256, 500, 17, 333, 511, 1, 480, 512], split=split, short=True, fields=True))


def test_the_narrow_four_wave_shape(monkeypatch):
    # the 8-frame four-wave kernel (og_k4_*), whose zero kernel is held to the general one's occupancy
    z = _same(monkeypatch, 200, [256, 500, 17, 333, 511, 1, 480, 512], split=4, wide=False, short=True, fields=True)
    assert all(z)


def test_the_amount_switched_between_blocks(monkeypatch):
    # 0 -> 0.5 -> 0: the launches with 0.5 run the general kernel, the cutoff moves with the envelope and comes back
    z = _same(monkeypatch, 200, [256] * 8, amounts={0: 0.0, 3: 0.5, 5: 0.0}, split=4, short=True, fields=True)
    assert z == [True, True, True, False, False, True, True, True], z


def test_a_negative_zero_amount(monkeypatch):
    # -0.0 reaches the slot (set_value_immediate keeps its bits) and runs the zero kernel
    assert _same(monkeypatch, 200, [256] * 4, amounts={0: 0.5, 1: -0.0}, split=4, fields=True) == [False, True, True, True]
    assert all(_same(monkeypatch, 200, [256] * 4, amounts={0: -0.0}, split=0, fields=True))


def test_a_ramp_that_ends_at_zero_inside_a_launch(monkeypatch):
    # from 0.5 down to 0 over 300 frames (blocks 1 and 2): those launches tick the ramp and run the general (table) kernel,
    # the ones after it the zero variant
    z = _same(monkeypatch, 200, [256] * 6, amounts={0: 0.5}, ramp=(1, 0.0, 300), split=4, short=True, fields=True)
    assert z == [False, False, False, True, True, True], z


def test_a_snapshot_saved_and_loaded_across_zero_launches(monkeypatch):
    assert all(_same(monkeypatch, 200, [256] * 6, split=4, short=True, fields=True, snapshot=3))
