"""The ADSR release reciprocals of the wide four-wave kernel (og_k4w_*) come from a device table in quiet release chunks
(og_kernel_rt.hip.h, rcp_fetch; og_engine.cpp, rcp_cover).  The table holds v_rcp_f32((float)n) as the instruction computes
it, so nothing observable may change: every case below is compared BIT FOR BIT with the ordinary kernel
(OSCEN_GPU_SPLIT=0, which keeps v_rcp_f32), the offline render (several blocks per launch) with the block-by-block path,
and the saved state with the ordinary kernel's."""
import numpy as np
import pytest

import oscen_amd

pytestmark = pytest.mark.gpu

N = 200  # ragged: four wide workgroups, the last one partly empty
SR = 48000.0
OPS = ("op3", "op2", "op1", "filter")


def _run(monkeypatch, split, releases, blocks, offline=False, cap=None):
    monkeypatch.setenv("OSCEN_GPU_SPLIT", str(split))
    monkeypatch.setenv("OSCEN_GPU_WIDE", "1" if split == 4 else "0")
    if cap is not None:
        monkeypatch.setenv("OSCEN_GPU_EXPERIMENTAL", "1")
        monkeypatch.setenv("OSCEN_GPU_RCP_CAP", str(cap))
    else:
        monkeypatch.delenv("OSCEN_GPU_RCP_CAP", raising=False)
    eng = oscen_amd.Engine("fm_voice", N, sample_rate=SR)
    try:
        assert eng.kernel_variant.startswith("og_k4w_" if split == 4 else "og_k_")
        rng = np.random.default_rng(7)
        eng.set_voice_values("frequency", (110.0 * 2.0 ** (rng.integers(0, 36, N) / 12.0)).astype(np.float32))
        for op in OPS:
            eng.set_value(op + "_attack", 0.003)
            eng.set_value(op + "_decay", 0.01)
        on = rng.integers(0, 600, N)
        off = on + rng.integers(900, 3000, N)
        for v in range(N):
            eng.schedule_voice_event("gate", v, int(on[v]), 0.9)
            eng.schedule_voice_event("gate", v, int(off[v]), 0.0)
        out = []
        f0 = 0
        for bi, frames in enumerate(blocks):
            for op in OPS:
                if bi in releases:
                    eng.set_value(op + "_release", releases[bi])
            if offline:
                out.append(eng.render(frames, 256))
            else:
                out.append(np.concatenate([eng.process_block(min(256, frames - k)) for k in range(0, frames, 256)]))
            f0 += frames
        return np.concatenate(out), bytes(eng.save_state())
    finally:
        eng.close()


def _same(monkeypatch, releases, blocks, cap=None):
    ref_bus, ref_state = _run(monkeypatch, 0, releases, blocks)
    assert np.max(np.abs(ref_bus)) > 1e-3  # (the notes sound)
    for offline in (False, True):
        bus, state = _run(monkeypatch, 4, releases, blocks, offline=offline, cap=cap)
        assert np.array_equal(bus.view(np.uint32), ref_bus.view(np.uint32)), (offline, int(np.sum(bus != ref_bus)))
        assert state == ref_state, offline


def test_a_two_second_release(monkeypatch):
    # 96 000-sample releases: the table grows past the default patch's 24 000 entries before the first block
    _same(monkeypatch, {0: 2.0}, [4096, 4096])


def test_a_release_time_raised_between_blocks_grows_the_table(monkeypatch):
    # releases running at 0.3 s when the release time goes to 1.5 s (and then back down): the launches after the change
    # read a grown table, while envelopes already releasing keep their countdowns
    _same(monkeypatch, {0: 0.3, 1: 1.5, 3: 0.2}, [1536, 2048, 1024, 2048])


def test_releases_straddle_launch_boundaries(monkeypatch):
    # block lengths that are not multiples of the 16-frame chunk: a release's chunks fall across launches at every offset
    _same(monkeypatch, {0: 0.05}, [1000, 17, 333, 511, 1, 2100, 4000])


def test_a_release_longer_than_the_table_cap_runs_the_rcp_body(monkeypatch):
    # cap 1 000 entries, releases of 0.5 s (24 000 samples): the launches run their release chunks through the checked body
    # (v_rcp_f32) -- and those with releases of 0.01 s (480 samples) in between take the table again
    _same(monkeypatch, {0: 0.5, 2: 0.01, 3: 0.5}, [1024, 2048, 1024, 2048], cap=1000)
