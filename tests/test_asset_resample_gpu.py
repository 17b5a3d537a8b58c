"""Conforming samples to the graph rate on load (csrc/og_asset_resample.hip.h): the reference's offline windowed sinc
(oscen-lib/src/asset/resample.rs) as a device kernel, behind og_resample and behind og_load_sample of a sample registered at
its own rate.  `-m gpu`.

Witness: here -- `resample_channel` and the per-channel loop of `AudioAsset::from_samples` restated with numpy f32 / Python f64
scalars operation for operation, sinf / cosf from the platform libm through ctypes (what Rust's f32::sin / cos bind to), the
sums taken in ascending tap order (np.add.accumulate is sequential).  The kernel keeps the reference's operation order and
takes its sine and cosine from og_sinf_exact / og_cosf_exact (glibc's bits), so the comparison is EXACT: np.array_equal on
the bit patterns.  Every case stays under about 3e5 taps."""
import ctypes as C
import ctypes.util
import functools
import math
import struct

import numpy as np
import pytest

import oscen_amd
from tests.test_sample_player_gpu import N, SR, bank, loop, mapped, noise, player_graph, render

pytestmark = pytest.mark.gpu
f32 = np.float32
PI = f32(3.14159274101257324)
ZERO_CROSSINGS = 32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]


def _map(fn, a):
    return np.array([fn(float(x)) for x in a], f32)


# ---- the witness ------------------------------------------------------------------------------------------------------
def sinc(x):
    """resample.rs:18-25 on an f32 array"""
    pix = PI * x
    with np.errstate(divide="ignore", invalid="ignore"):
        y = _map(_libm.sinf, pix) / pix
    return np.where(x == f32(0.0), f32(1.0), y).astype(f32)


def blackman(t):
    """resample.rs:29-39 on an f32 array"""
    phase = PI * (t + f32(1.0))
    c = _map(_libm.cosf, phase)
    y = f32(0.42) - f32(0.5) * c + f32(0.08) * (f32(2.0) * c * c - f32(1.0))
    return np.where(np.abs(t) > f32(1.0), f32(0.0), y).astype(f32)


def round_half_away(v):
    """f64::round of a non-negative value"""
    r = math.floor(v)
    return r + 1 if v - r >= 0.5 else r


def out_frames(frames, src, dst):
    return frames if frames == 0 or src == dst else int(round_half_away(float(frames) * (float(dst) / float(src))))


def resample_channel(x, src, dst):
    """resample.rs:47-103"""
    x = np.asarray(x, f32)
    if len(x) == 0 or src == dst:
        return x.copy()
    ratio = float(dst) / float(src)
    n_out = int(round_half_away(float(len(x)) * ratio))
    cutoff = f32(min(ratio, 1.0))
    radius = f32(ZERO_CROSSINGS) / cutoff
    inv_ratio = 1.0 / ratio
    inv_radius = f32(1.0) / radius
    out = np.zeros(n_out, f32)
    zero = np.zeros(1, f32)
    for n in range(n_out):
        pos = float(n) * inv_ratio
        first = max(int(math.ceil(pos - float(radius))), 0)
        last = min(int(math.floor(pos + float(radius))), len(x) - 1)
        if last < first:
            continue
        i = np.arange(first, last + 1)
        dist = (pos - i.astype(np.float64)).astype(f32)
        w = (sinc(cutoff * dist) * blackman(dist * inv_radius)).astype(f32)
        # acc += w * sample; weight_sum += w -- from +0.0, one rounding per product and per sum, in tap order
        acc = np.add.accumulate(np.concatenate([zero, (w * x[first:last + 1]).astype(f32)]), dtype=f32)[-1]
        weight_sum = np.add.accumulate(np.concatenate([zero, w]), dtype=f32)[-1]
        out[n] = acc / weight_sum if weight_sum != 0.0 else f32(0.0)
    return out


def conform(a, src, dst):
    """from_samples (asset/mod.rs:199-221): deinterleave, resample channel by channel; returned as [frames, channels]"""
    a = np.asarray(a, f32)
    a = a.reshape(len(a), -1)
    return np.stack([resample_channel(np.ascontiguousarray(a[:, c]), src, dst) for c in range(a.shape[1])], axis=1)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_witness_itself():
    """what the witness restates by hand: the rounding of the length, the guards of sinc and blackman, the sequential sum"""
    assert [round_half_away(v) for v in (0.0, 0.49, 0.5, 1.5, 2.5, 459.375)] == [0, 0, 1, 2, 3, 459]
    assert out_frames(1000, 48000, 24000) == 500 and out_frames(1, 48000, 16000) == 0
    assert sinc(np.array([0.0], f32))[0] == 1.0 and blackman(np.array([1.5, -1.0000001], f32)).tolist() == [0.0, 0.0]
    assert abs(float(blackman(np.array([0.0], f32))[0]) - 1.0) < 1e-6
    a = np.array([1.0, 2.0 ** -24, 2.0 ** -24], f32)  # ((1 + e) + e) = 1 in f32, 1 + (e + e) is not
    assert np.add.accumulate(a, dtype=f32)[-1] == f32(1.0)


# ---- 1: bit equality with the witness ------------------------------------------------------------------------------------
def zeros_in_it(seed, frames):
    a = noise(seed, frames)
    a[10:14] = 0.0
    a[120:260] = 0.0  # longer than the kernel: whole outputs are exactly 0 / weight_sum
    a[300] = -0.0
    return a


CASES = [("48000->44100 %dch" % c, 48000, 44100, 500, c) for c in (1, 2, 3, 8)] + \
        [("44100->48000 %dch" % c, 44100, 48000, 500, c) for c in (1, 2, 3, 8)] + \
        [("22050->44100", 22050, 44100, 300, 1), ("96000->44100", 96000, 44100, 700, 2), ("48000->8000 radius 192", 48000, 8000, 300, 1),
         ("one frame", 44100, 48000, 1, 1), ("two frames", 44100, 48000, 2, 2), ("several workgroups", 44100, 48000, 2100, 1),
         ("zeros", 48000, 44100, 500, 1)]


@functools.lru_cache(maxsize=None)
def case_data(label):
    k = [c[0] for c in CASES].index(label)
    _, src, dst, frames, ch = CASES[k]
    a = zeros_in_it(900 + k, frames) if label == "zeros" else noise(900 + k, frames, ch)
    want = conform(a, src, dst)
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


@pytest.mark.parametrize("label", [c[0] for c in CASES])
def test_og_resample_is_the_witness_bit_for_bit(label):
    _, src, dst, frames, ch = CASES[[c[0] for c in CASES].index(label)]
    a, want = case_data(label)
    got = oscen_amd.resample(a, src, dst)
    got = got.reshape(len(got), -1)
    assert got.shape == want.shape == (out_frames(frames, src, dst), ch)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    n_bits = int(np.count_nonzero(bits(got) != bits(want)))
    print("%s: %d frames -> %d, %d of %d values differ in their bits, max |diff| %.3g" % (label, frames, len(got), n_bits, got.size, diff.max() if diff.size else 0.0))
    assert np.array_equal(bits(got), bits(want))
    if label == "zeros":
        assert not got[150:200].any() and got[:100].any()
    if label == "several workgroups":
        assert len(got) > 8 * 256 and len(got) % 256 != 0


# ---- 2: the reference's known answers (resample.rs:110-270), with its own bounds ---------------------------------------------
def sine(freq, rate, n):
    i = np.arange(n).astype(f32)
    return np.sin(f32(2.0) * PI * f32(freq) * i / f32(rate)).astype(f32)


def test_constant_is_preserved():
    x = np.full(500, 0.7, f32)
    guard = ZERO_CROSSINGS + 4
    for src, dst in [(48000, 44100), (44100, 48000), (96000, 44100)]:
        out = oscen_amd.resample(x, src, dst)
        err = float(np.max(np.abs(out[guard:len(out) - guard] - f32(0.7))))
        print("constant %d->%d: max error %.3g" % (src, dst, err))
        assert len(out) > 2 * guard and err <= 1e-3


@pytest.mark.parametrize("src,dst,frames", [(48000, 44100, 24000), (24000, 48000, 12000)])
def test_sine_frequency_and_amplitude_preserved(src, dst, frames):
    out = oscen_amd.resample(sine(1000.0, src, frames), src, dst)
    assert len(out) == frames * dst // src
    guard = ZERO_CROSSINGS + 8
    err = float(np.max(np.abs(out - sine(1000.0, dst, len(out)))[guard:len(out) - guard]))
    print("1 kHz sine %d->%d: max error %.3g" % (src, dst, err))
    assert err < 1e-2


def test_downsample_rejects_above_nyquist():
    out = oscen_amd.resample(sine(12000.0, 48000, 24000), 48000, 16000)
    guard = ZERO_CROSSINGS + 8
    peak = float(np.max(np.abs(out[guard:len(out) - guard])))
    print("12 kHz tone 48000->16000: peak %.3g" % peak)
    assert len(out) == 8000 and peak < 0.1


def test_integer_downsample_matches_reference():
    x = sine(200.0, 48000, 12000)
    out = oscen_amd.resample(x, 48000, 24000)
    guard = ZERO_CROSSINGS + 8
    i = np.arange(guard, len(out) - guard)
    err = float(np.max(np.abs(out[i] - x[2 * i])))
    print("2:1 decimation of a 200 Hz sine: max error %.3g" % err)
    assert len(out) == 6000 and err < 5e-3


def test_output_length_tracks_ratio():
    x = np.zeros(1000, f32)
    assert len(oscen_amd.resample(x, 48000, 24000)) == 500
    assert len(oscen_amd.resample(x, 24000, 48000)) == 2000
    assert len(oscen_amd.resample(x, 48000, 48000)) == 1000


def test_output_is_finite_across_rate_sweep():
    state, x = 0x2545F4914F6CDD1D, np.zeros(4000, f32)
    for k in range(4000):
        state = (state * 6364136223846793005 + 1) & 0xFFFFFFFFFFFFFFFF
        x[k] = f32(f32(state >> 33) / f32(1 << 31)) - f32(1.0)
    for src, dst in [(48000, 44100), (44100, 48000), (96000, 44100), (44100, 96000), (48000, 8000), (22050, 44100), (48000, 48000)]:
        out = oscen_amd.resample(x, src, dst)
        assert len(out) == out_frames(4000, src, dst) and np.all(np.isfinite(out)), (src, dst)
    assert np.array_equal(bits(oscen_amd.resample(x, 48000, 48000)), bits(x))  # equal rates copy


# ---- 3: a player plays the witness's samples ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def player_sources():
    stereo, mono = noise(950, 60, 2), noise(951, 40)
    return stereo, mono, conform(stereo, 44100, 48000), conform(mono, 22050, 48000)


@pytest.mark.parametrize("width", [1, 2])
def test_a_player_plays_the_conformed_and_mapped_samples(width):
    stereo, mono, c_stereo, c_mono = player_sources()
    assert len(c_stereo) == 65 and len(c_mono) == 87
    oscen_amd.register_sample("ar_stereo_441", stereo, sample_rate=44100)
    oscen_amd.register_sample("ar_mono_2205", mono, sample_rate=22050)
    eng = bank(player_graph(width, "Ar"))
    i_s, i_m = eng.load_sample("ar_stereo_441"), eng.load_sample("ar_mono_2205")
    assert (i_s, i_m) == (0, 1) and eng.load_sample("ar_stereo_441") == 0
    eng.set_voice_samples("player", [i_s if v % 2 == 0 else i_m for v in range(N)])
    blocks = [100, 77]  # both samples loop inside the first block, the longer one a second time in the second
    taps, _ = render(eng, blocks)
    total = sum(blocks)
    for v in range(N):
        want = loop(mapped(c_stereo if v % 2 == 0 else c_mono, width), 0, 0, total)
        got = taps[v].reshape(total, width)
        assert np.array_equal(bits(got), bits(want)), v
    ph = eng.read_state_field("player.playhead", dtype=np.uint32)
    assert np.array_equal(ph, np.array([total % (65 if v % 2 == 0 else 87) for v in range(N)], np.uint32))


# ---- 4: an equal rate is today's path -------------------------------------------------------------------------------------------
def test_an_equal_rate_is_the_untagged_path():
    a = noise(960, 33, 2)
    oscen_amd.register_sample("ar_eq_plain", a)
    oscen_amd.register_sample("ar_eq_tagged", a, sample_rate=int(SR))
    eng = bank(player_graph(2, "Ar"))
    i_p, i_t = eng.load_sample("ar_eq_plain"), eng.load_sample("ar_eq_tagged")
    eng.set_voice_samples("player", [i_p if v < 35 else i_t for v in range(N)])
    taps, _ = render(eng, [50, 31])
    assert np.array_equal(bits(taps[:35]), bits(taps[35:])) and np.array_equal(bits(taps[0]), bits(loop(a, 0, 0, 81)))


# ---- 5: errors -----------------------------------------------------------------------------------------------------------------
def test_errors_of_the_load_path():
    lib = oscen_amd.load_library()
    a = noise(970, 20)
    oscen_amd.register_sample("ar_err_tagged", a, sample_rate=44100)
    oscen_amd.register_sample("ar_err_one", a[:1], sample_rate=48000)
    oscen_amd.register_sample("ar_err_plain", a)
    cold = oscen_amd.Engine(player_graph(1, "Ar"), N)  # no og_init yet: GraphRateUnset
    with pytest.raises(oscen_amd.OscenError) as ei:
        cold.load_sample("ar_err_tagged")
    assert ei.value.code == -1 and "og_init" in str(ei.value)
    assert cold.load_sample("ar_err_plain") == 0  # (untagged samples load as before)
    odd = oscen_amd.Engine(player_graph(1, "Ar"), N, sample_rate=44100.5)
    with pytest.raises(oscen_amd.OscenError) as ei:
        odd.load_sample("ar_err_tagged")
    assert ei.value.code == -1 and "integer" in str(ei.value)
    eng = bank(player_graph(1, "Ar"), taps=False)
    eng.init(16000.0)
    first = eng.load_sample("ar_err_plain")
    with pytest.raises(oscen_amd.OscenError) as ei:
        eng.load_sample("ar_err_one")  # 1 frame, 48000 -> 16000: round(1/3) = 0 frames
    assert ei.value.code == -1 and "empty" in str(ei.value)
    assert eng.load_sample("ar_err_tagged") == first + 1  # the refused load took no index
    # re-init at another rate: the conformed sample is refused, with both rates named; the untagged one still publishes
    eng.init(22050.0)
    tagged = first + 1
    assert lib.og_set_sample(eng.h, b"player", tagged) == -1
    msg = lib.og_last_error()
    assert b"16000" in msg and b"22050" in msg and b"ar_err_tagged" in msg
    one = (C.c_uint32 * 1)(tagged)
    assert lib.og_set_voice_samples(eng.h, b"player", 3, 1, C.cast(one, C.POINTER(C.c_uint32))) == -1
    assert np.array_equal(eng.read_state_field("player.sample", dtype=np.uint32), np.full(N, 0xFFFFFFFF, np.uint32))
    eng.set_sample("player", first)
    eng.init(16000.0)
    eng.set_sample("player", tagged)  # back at its rate it publishes again


# ---- 6: snapshots ----------------------------------------------------------------------------------------------------------------
def test_a_snapshot_with_a_conformed_sample_resumes_bit_for_bit_and_checks_the_rate():
    a, b = noise(980, 50, 2), noise(981, 23)
    oscen_amd.register_sample("ar_snap_tagged", a, sample_rate=44100)
    oscen_amd.register_sample("ar_snap_plain", b)
    g = player_graph(1, "Ar")
    eng = bank(g)
    i_p, i_t = eng.load_sample("ar_snap_plain"), eng.load_sample("ar_snap_tagged")
    eng.set_voice_samples("player", [i_t if v % 3 else i_p for v in range(N)])
    render(eng, [70])
    blob = eng.save_state()
    assert len(blob) == eng.state_bytes
    fresh = bank(g)
    fresh.load_state(blob)
    assert (fresh.load_sample("ar_snap_plain"), fresh.load_sample("ar_snap_tagged")) == (i_p, i_t)
    x, bus_x = render(eng, [100, 33])
    y, bus_y = render(fresh, [100, 33])
    assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(bus_x), bits(bus_y))
    want = loop(conform(a, 44100, 48000)[:, 0], 0, 70, 203)
    assert np.array_equal(bits(x[1]), bits(want))
    try:
        for other in (dict(sample_rate=32000), dict()):  # another source rate; no rate at all
            oscen_amd.register_sample("ar_snap_tagged", a, **other)
            cold = bank(g)
            with pytest.raises(oscen_amd.OscenError) as ei:
                cold.load_state(blob)
            assert ei.value.code == -1 and "ar_snap_tagged" in str(ei.value)
            assert not cold.read_state_field("player.playhead", dtype=np.uint32).any()  # nothing was changed ...
            assert cold.load_sample("ar_snap_tagged") == 0  # ... and nothing loaded
    finally:
        oscen_amd.register_sample("ar_snap_tagged", a, sample_rate=44100)
    other_rate = bank(g)
    other_rate.init(44100.0)  # the engine's rate is not the one the blob's sample was conformed to
    with pytest.raises(oscen_amd.OscenError) as ei:
        other_rate.load_state(blob)
    assert ei.value.code == -1


def test_a_blob_of_untagged_samples_is_what_it_was():
    """the sample section as it was before samples carried rates, built here by hand: magic "OSMP", count, then per sample
    {name length, frames, channels, 0} and the name padded to 4 bytes -- and nothing else behind it"""
    names = [("ar_old_a", noise(990, 7)), ("ar_old_bcd", noise(991, 12, 2))]
    eng = bank()
    for n, a in names:
        oscen_amd.register_sample(n, a)
        eng.load_sample(n)
    eng.set_sample("player", 1)
    render(eng, [20])
    blob = bytes(eng.save_state())
    tail = struct.pack("<II", 0x504D534F, len(names))
    for n, a in names:
        raw = n.encode()
        tail += struct.pack("<IIII", len(raw), len(a), a.reshape(len(a), -1).shape[1], 0) + raw + b"\0" * (-len(raw) % 4)
    assert blob.endswith(tail)
    none_loaded = bank()
    assert bytes(none_loaded.save_state()).endswith(struct.pack("<II", 0x504D534F, 0))
    assert len(blob) - len(tail) == len(bytes(none_loaded.save_state())) - 8  # everything in front of the section has the old size


# ---- 7: clusters ---------------------------------------------------------------------------------------------------------------
def test_a_two_shard_cluster_conforms_on_every_device():
    n_dev = C.c_int(0)
    if oscen_amd.load_library().hipGetDeviceCount(C.byref(n_dev)) != 0 or n_dev.value < 2:
        pytest.skip("needs two visible devices")
    stereo, mono, c_stereo, c_mono = player_sources()
    oscen_amd.register_sample("ar_clu_stereo", stereo, sample_rate=44100)
    oscen_amd.register_sample("ar_clu_mono", mono, sample_rate=22050)
    g = player_graph(1, "Ar")
    single = bank(g)
    idx = [single.load_sample("ar_clu_stereo"), single.load_sample("ar_clu_mono")]
    cl = oscen_amd.Cluster(g, N, [0, 1], sample_rate=SR)
    assert [cl.load_sample("ar_clu_stereo"), cl.load_sample("ar_clu_mono")] == idx
    shards = [cl.shard(s) for s in range(2)]
    for e in shards:
        e.set_voice_taps(list(range(e.n_voices)))
    choice = [idx[v % 2] for v in range(N)]
    single.set_voice_samples("player", choice)
    cl.set_voice_samples("player", choice)
    for frames in (100, 77):
        single.process_block(frames)
        cl.process_block(frames)
        taps_c = np.concatenate([e.read_voice_taps(frames) for e in shards], axis=0)
        assert np.array_equal(bits(taps_c), bits(single.read_voice_taps(frames)))
    assert np.array_equal(bits(taps_c[0]), bits(loop(c_stereo[:, 0], 0, 100, 177)))
    assert np.array_equal(bits(taps_c[N - 1]), bits(loop(c_mono[:, 0], 0, 100, 177)))
