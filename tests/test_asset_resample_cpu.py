"""The sample load path without a GPU: the argument checks of every new entry point, the WAV reader against og_write_wav and
against hand-built files, a gfx950 compile of the resample kernels with no private segment, and the fact that no built-in
graph's kernel was renamed by it.  (What needs a device -- the resample itself, the conforming load, the rate check on
publishing, snapshots -- is tests/test_asset_resample_gpu.py, which tests/test_asset_resample_hostsim_cpu.py runs on the host
simulator.)"""
import ctypes as C
import glob
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bench
import oscen_amd
from oscen_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p = C.POINTER(C.c_float)
INVALID, UNSUPPORTED = oscen_amd.OG_E_INVALID, oscen_amd.OG_E_UNSUPPORTED


def test_argument_validation_of_the_new_entry_points():
    lib = oscen_amd.load_library()
    a = np.arange(16, dtype=np.float32)
    out = np.zeros(64, np.float32)
    p, q = a.ctypes.data_as(f32p), out.ctypes.data_as(f32p)
    n = C.c_uint64(7)
    # og_register_sample_at_rate
    assert lib.og_register_sample_at_rate(None, p, 4, 1, 44100) == INVALID
    assert lib.og_register_sample_at_rate(b"", p, 4, 1, 44100) == INVALID
    assert lib.og_register_sample_at_rate(b"arc_x", None, 4, 1, 44100) == INVALID
    assert lib.og_register_sample_at_rate(b"arc_x", p, 4, 1, 0) == INVALID and b"rate" in lib.og_last_error()   # ZeroSampleRate
    assert lib.og_register_sample_at_rate(b"arc_x", p, 0, 1, 44100) == INVALID and b"empty" in lib.og_last_error()  # Empty
    assert lib.og_register_sample_at_rate(b"arc_x", p, 1, 9, 44100) == INVALID and b"channels" in lib.og_last_error()
    assert lib.og_register_sample_at_rate(b"arc_x", p, 1, 0, 44100) == INVALID
    assert lib.og_register_sample_at_rate(b"arc_x", p, (1 << 28) + 1, 1, 44100) == INVALID
    assert lib.og_sample_info(b"arc_x", None, None, None) == INVALID  # none of the above registered anything
    assert lib.og_register_sample_at_rate(b"arc_x", p, 2, 8, 44100) == 0
    frames, ch, rate = C.c_uint64(), C.c_uint32(), C.c_uint32()
    assert lib.og_sample_info(b"arc_x", C.byref(frames), C.byref(ch), C.byref(rate)) == 0
    assert (frames.value, ch.value, rate.value) == (2, 8, 44100)
    assert lib.og_sample_info(None, None, None, None) == INVALID
    assert lib.og_read_sample(b"arc_x", None, 2) == INVALID and lib.og_read_sample(None, q, 2) == INVALID
    assert lib.og_read_sample(b"arc_x", q, 1) == INVALID  # capacity too small
    assert lib.og_read_sample(b"arc_x", q, 2) == 0 and np.array_equal(out[:16], a) and not out[16:].any()
    assert lib.og_register_sample(b"arc_x", p, 4, 1) == 0  # the untagged call is what it was: no rate, an empty one legal
    assert lib.og_sample_info(b"arc_x", None, None, C.byref(rate)) == 0 and rate.value == 0
    assert lib.og_register_sample(b"arc_x", None, 0, 1) == 0
    assert lib.og_unregister_sample(b"arc_x") == 0
    # og_register_sample_wav
    assert lib.og_register_sample_wav(None, b"/nonexistent.wav") == INVALID
    assert lib.og_register_sample_wav(b"arc_w", None) == INVALID
    assert lib.og_register_sample_wav(b"arc_w", b"/nonexistent/nowhere.wav") == INVALID and b"cannot open" in lib.og_last_error()
    # og_resample_frames
    assert lib.og_resample_frames(500, 48000, 44100, None) == INVALID
    assert lib.og_resample_frames(500, 0, 44100, C.byref(n)) == INVALID and lib.og_resample_frames(500, 48000, 0, C.byref(n)) == INVALID
    assert n.value == 7
    for frames_in, src, dst, want in [(500, 48000, 44100, 459), (500, 44100, 48000, 544), (1000, 48000, 24000, 500), (1000, 24000, 48000, 2000),
                                      (1000, 48000, 48000, 1000), (1, 48000, 16000, 0), (3, 48000, 24000, 2), (0, 48000, 44100, 0)]:
        assert lib.og_resample_frames(frames_in, src, dst, C.byref(n)) == 0 and n.value == want, (frames_in, src, dst, n.value)
    # og_resample (every check comes before the device is touched)
    assert lib.og_resample(None, 4, 1, 48000, 44100, q, 64) == INVALID and lib.og_resample(p, 4, 1, 48000, 44100, None, 64) == INVALID
    assert lib.og_resample(p, 4, 1, 0, 44100, q, 64) == INVALID and lib.og_resample(p, 4, 1, 48000, 0, q, 64) == INVALID
    assert lib.og_resample(p, 0, 1, 48000, 44100, q, 64) == INVALID
    assert lib.og_resample(p, 1, 9, 48000, 44100, q, 64) == INVALID and b"channels" in lib.og_last_error()
    assert lib.og_resample(p, 1, 0, 48000, 44100, q, 64) == INVALID
    assert lib.og_resample(p, 16, 1, 44100, 48000, q, 16) == INVALID and b"17" in lib.og_last_error()  # capacity too small
    assert lib.og_resample(p, 16, 1, 48000, 48000, q, 15) == INVALID
    assert not out[16:].any()
    assert lib.og_resample(p, 16, 1, 48000, 48000, q, 16) == 0 and np.array_equal(out[:16], a)  # equal rates copy, no device
    with pytest.raises(ValueError):
        oscen_amd.resample(np.zeros((2, 2, 2)), 48000, 44100)
    with pytest.raises(oscen_amd.OscenError):
        oscen_amd.register_sample("arc_y", np.zeros(0, np.float32), sample_rate=44100)


# ---- the WAV reader -------------------------------------------------------------------------------------------------------
def riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def chunk(tag, data, declared=None):
    return tag + struct.pack("<I", len(data) if declared is None else declared) + data + (b"\0" if len(data) & 1 else b"")


def fmt(tag, channels, rate, bits, extensible=False):
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if extensible:  # cbSize, valid bits, channel mask, SubFormat GUID: the format tag + the fixed rest
        head += struct.pack("<HHIH", 22, bits, 3, tag) + bytes.fromhex("000000001000800000aa00389b71")
    return chunk(b"fmt ", head)


def read_back(path, name="arc_wav"):
    oscen_amd.register_sample_wav(name, path)
    try:
        return oscen_amd.registered_sample(name)
    finally:
        oscen_amd.unregister_sample(name)


def test_wav_files_written_by_og_write_wav_read_back(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.uniform(-1.0, 1.0, (37, 2)).astype(np.float32)
    a[0] = [1.0, -1.0]
    p = str(tmp_path / "f32.wav")
    oscen_amd.write_wav(p, a, sample_rate=44100, bits=32)
    got, rate = read_back(p)
    assert rate == 44100 and got.shape == a.shape and np.array_equal(got.view(np.uint32), a.view(np.uint32))  # float: exact
    p = str(tmp_path / "i16.wav")
    oscen_amd.write_wav(p, a[:, 0], sample_rate=22050, bits=16)
    got, rate = read_back(p)
    want = np.rint(a[:, 0] * np.float32(32767.0)).astype(np.int16).astype(np.float32) * np.float32(1.0 / 32768.0)
    assert rate == 22050 and got.shape == (37, 1) and np.array_equal(got[:, 0], want)  # exact after the 1/32768 scaling
    assert got[0, 0] == np.float32(32767.0 / 32768.0)


def test_hand_built_24_bit_and_extensible_files(tmp_path):
    ints = [0, 1, -1, 0x7FFFFF, -0x800000, 0x123456, -0x123456]
    data = b"".join(struct.pack("<i", v)[:3] for v in ints) + b"\x00\x00\x00"  # 8 samples: 4 stereo frames
    p = tmp_path / "i24.wav"
    p.write_bytes(riff(fmt(1, 2, 96000, 24), chunk(b"data", data)))
    got, rate = read_back(str(p))
    assert rate == 96000 and got.shape == (4, 2)
    assert np.array_equal(got.reshape(-1), (np.array(ints + [0], np.float32) * np.float32(1.0 / 8388608.0)))
    # WAVE_FORMAT_EXTENSIBLE around PCM 16 and around float 32, an unknown odd-sized chunk in front of and behind fmt
    p = tmp_path / "ext16.wav"
    p.write_bytes(riff(chunk(b"LIST", b"abc"), fmt(1, 1, 48000, 16, extensible=True), chunk(b"fact", b"\4\0\0\0"), chunk(b"data", struct.pack("<4h", 0, 16384, -32768, 32767))))
    got, rate = read_back(str(p))
    assert rate == 48000 and np.array_equal(got[:, 0], np.array([0.0, 0.5, -1.0, 32767.0 / 32768.0], np.float32))
    p = tmp_path / "extf.wav"
    p.write_bytes(riff(fmt(3, 2, 44100, 32, extensible=True), chunk(b"data", struct.pack("<4f", 0.25, -0.5, 1.5, -0.0))))
    got, rate = read_back(str(p))
    assert rate == 44100 and np.array_equal(got.view(np.uint32), np.array([[0.25, -0.5], [1.5, -0.0]], np.float32).view(np.uint32))
    p = tmp_path / "i32.wav"
    p.write_bytes(riff(fmt(1, 1, 8000, 32), chunk(b"data", struct.pack("<3i", 1 << 30, -(1 << 31), 3))))
    got, rate = read_back(str(p))
    assert rate == 8000 and np.array_equal(got[:, 0], np.array([0.5, -1.0, 3.0 / 2147483648.0], np.float32))


def test_malformed_and_unsupported_files(tmp_path):
    lib = oscen_amd.load_library()

    def rc(name, image):
        p = tmp_path / name
        p.write_bytes(image)
        code = lib.og_register_sample_wav(b"arc_bad", str(p).encode())
        msg = lib.og_last_error()
        assert lib.og_sample_info(b"arc_bad", None, None, None) == INVALID  # nothing was registered
        return code, msg

    good = riff(fmt(1, 2, 44100, 16), chunk(b"data", bytes(range(16))))
    for cut in (0, 3, 11, 12, 19, 20, 35, 36, 43, 44, 45, len(good) - 1):  # truncated anywhere
        code, msg = rc("cut%d.wav" % cut, good[:cut])
        assert code == INVALID and msg, cut
    code, msg = rc("past_end.wav", riff(chunk(b"LIST", b"abcdef", declared=4000), fmt(1, 2, 44100, 16), chunk(b"data", bytes(16))))
    assert code == INVALID and b"LIST" in msg and b"4000" in msg  # a chunk whose declared size runs past the end
    code, msg = rc("huge.wav", riff(fmt(1, 2, 44100, 16), chunk(b"data", bytes(16), declared=0xFFFFFFF0)))
    assert code == INVALID and b"data chunk declares" in msg
    code, msg = rc("nodata.wav", riff(fmt(1, 2, 44100, 16)))
    assert code == INVALID and b"no data chunk" in msg
    code, msg = rc("empty.wav", riff(fmt(1, 2, 44100, 16), chunk(b"data", b"")))
    assert code == INVALID and b"empty" in msg  # from_samples refuses an empty asset
    code, msg = rc("zero_rate.wav", riff(fmt(1, 1, 0, 16), chunk(b"data", bytes(4))))
    assert code == INVALID and b"rate" in msg
    code, msg = rc("nine.wav", riff(fmt(1, 9, 44100, 16), chunk(b"data", bytes(18))))
    assert code == INVALID and b"channels" in msg
    code, msg = rc("u8.wav", riff(fmt(1, 1, 8000, 8), chunk(b"data", bytes(8))))
    assert code == UNSUPPORTED and b"8 bits" in msg
    code, msg = rc("adpcm.wav", riff(fmt(2, 1, 8000, 4), chunk(b"data", bytes(8))))
    assert code == UNSUPPORTED
    code, msg = rc("f64.wav", riff(fmt(3, 1, 8000, 64), chunk(b"data", bytes(8))))
    assert code == UNSUPPORTED


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_the_resample_kernels_compile_for_gfx950_without_a_private_segment(tmp_path):
    hip = tmp_path / "resample.hip"
    hip.write_text('#include "og_asset_resample.hip.h"\n' + "".join(
        "template __global__ void og_asset_resample<%d>(const float*, uint64_t, uint32_t, uint64_t, double, float, float, float, float*);\n" % c for c in (1, 2, 8)))
    r = subprocess.run([b.hipcc(), "--offload-arch=" + b.ARCH, "-x", "hip", "-c", "--cuda-device-only", str(hip), "-o", str(tmp_path / "resample.o"),
                        "-Rpass-analysis=kernel-resource-usage"] + b.COMMON, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    usage = {}
    for part in r.stdout.split("Function Name: ")[1:]:
        usage[part.split()[0]] = {k.strip(): v for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", part)}
    kernels = {n: u for n, u in usage.items() if "og_asset_" in n}
    print({n: (u["VGPRs"], u["ScratchSize [bytes/lane]"]) for n, u in kernels.items()})
    assert len(kernels) == 4, sorted(usage)  # three widths of the resampler and the channel mapping
    for n, u in kernels.items():
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["LDS Size [bytes/block]"]) == 0, (n, u)
        assert int(u["VGPRs"]) <= 64, (n, u)  # eight waves per SIMD


def test_no_built_in_kernel_was_renamed():
    """the resampler's header is outside the digests that name the voice kernels: the generated sources are the committed ones,
    and the kernels bench.py times still carry the names the committed profiles were taken under"""
    digest = open(os.path.join(b.CSRC, "og_rt_digest.h")).read()
    assert "og_asset_resample" not in digest
    for h in b.RT_HEADERS + [b.ADSRP_HEADER, b.SMP_HEADER, "og_graph.cpp"]:
        assert "og_asset_resample" not in open(os.path.join(b.CSRC, h)).read(), h
    profiles = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "profiles", "*_summary.json")))
    timed = {"fm_voice"} | {c[1] for c in bench.OTHER_CONFIGS}  # (tests/test_profiles_match_cpu.py holds the whole contract)
    gens = sorted(glob.glob(os.path.join(b.GEN, "*.hip")))
    assert len(gens) >= 8
    for path in gens:
        stem = os.path.basename(path)[:-4]
        if stem.endswith("_z") or stem.endswith("_z2"):
            continue
        g = oscen_amd.Graph(builtin=stem)
        assert g.kernel_source() == open(path).read(), stem
        assert g.kernel_name() in g.kernel_source()
        if stem in timed:
            assert g.kernel_name()[:-3] in profiles, (stem, g.kernel_name())
