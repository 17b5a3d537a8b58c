"""Asset impulse responses without a GPU: the registry's semantics (both forms under one name space), the WAV reader in front
of it, the Python surface's dispatch, the refusal of `Convolver::with_ir` on an asset, the parity of header, -sys crate and
library, the built-in kernels' names (the voice kernels are untouched), the bus kernels' resource use, and the stand-alone
program of tests/standalone/ir_asset_main.cpp under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oscen_amd
from oscen_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = oscen_amd.OG_E_INVALID, oscen_amd.OG_E_UNSUPPORTED
NEW_SYMBOLS = ["og_register_ir_asset", "og_register_ir_wav", "og_ir_info", "og_bus_ir_info", "og_read_bus_ir"]


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def info(lib, name):
    frames, ch, rate = C.c_uint64(77), C.c_uint32(77), C.c_uint32(77)
    rc = lib.og_ir_info(name, C.byref(frames), C.byref(ch), C.byref(rate))
    return (frames.value, ch.value, rate.value) if rc == 0 else rc


# ---- the registry ---------------------------------------------------------------------------------------------------------
def test_registry_info_and_replacement_across_forms():
    lib = oscen_amd.load_library()
    a = np.arange(12, dtype=np.float32)
    assert info(lib, b"irc::x") == INVALID and b"irc::x" in lib.og_last_error()
    assert lib.og_register_ir_asset(b"irc::x", fptr(a), 6, 2, 44100) == 0
    assert info(lib, b"irc::x") == (6, 2, 44100)
    assert info(lib, b"x()") == (6, 2, 44100)  # by the last path segment, parentheses ignored, as with_ir resolves names
    assert lib.og_ir_info(b"irc::x", None, None, None) == 0  # out-pointers may be NULL
    assert lib.og_ir_info(None, None, None, None) == INVALID
    # the mono form under the same name replaces the asset, and the other way round
    assert lib.og_register_ir(b"irc::x", fptr(a), 5) == 0
    assert info(lib, b"irc::x") == (5, 1, 0)  # rate 0: registered through og_register_ir
    assert lib.og_register_ir_asset(b"irc::x", fptr(a), 4, 3, 96000) == 0
    assert info(lib, b"irc::x") == (4, 3, 96000)
    assert lib.og_register_ir_asset(b"irc::x", fptr(a), 12, 1, 8000) == 0  # one channel at a rate is an asset too
    assert info(lib, b"irc::x") == (12, 1, 8000)
    # og_unregister_ir removes either form
    assert lib.og_unregister_ir(b"irc::x") == 0 and info(lib, b"irc::x") == INVALID
    assert lib.og_unregister_ir(b"irc::x") == INVALID
    assert lib.og_register_ir(b"irc::x", fptr(a), 3) == 0 and lib.og_unregister_ir(b"irc::x") == 0


def test_registry_limits_and_name_rules():
    lib = oscen_amd.load_library()
    a = np.arange(16, dtype=np.float32)
    assert lib.og_register_ir_asset(b"irc::y", fptr(a), 2, 8, 48000) == 0 and info(lib, b"irc::y") == (2, 8, 48000)  # 8 channels at most
    assert lib.og_unregister_ir(b"irc::y") == 0
    for frames, ch, rate, word in ((2, 0, 48000, b"channels"), (1, 9, 48000, b"channels"), (2, 2, 0, b"rate is 0"), (0, 2, 48000, b"empty"),
                                   ((1 << 28) // 2 + 1, 2, 48000, b"2^28")):
        assert lib.og_register_ir_asset(b"irc::y", fptr(a), frames, ch, rate) == INVALID, (frames, ch, rate)
        assert word in lib.og_last_error(), (word, lib.og_last_error())
    assert lib.og_register_ir_asset(b"irc::y", None, 2, 2, 48000) == INVALID
    assert lib.og_register_ir_asset(None, fptr(a), 2, 2, 48000) == INVALID
    for name in (b"no good", b"", b"a::", b"::a", b"9lives", b"a.b"):  # og_register_ir's rule: a path of identifiers
        assert lib.og_register_ir_asset(name, fptr(a), 2, 2, 48000) == INVALID, name
        assert lib.og_register_ir(name, fptr(a), 2) == INVALID, name
    assert info(lib, b"irc::y") == INVALID  # none of the above registered anything


# ---- WAV files --------------------------------------------------------------------------------------------------------------
def riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def chunk(tag, data, declared=None):
    return tag + struct.pack("<I", len(data) if declared is None else declared) + data + (b"\0" if len(data) & 1 else b"")


def fmt(tag, channels, rate, bits, extensible=False):
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if extensible:
        head += struct.pack("<HHIH", 22, bits, 3, tag) + bytes.fromhex("000000001000800000aa00389b71")
    return chunk(b"fmt ", head)


def test_wav_formats(tmp_path):
    cases = [("i16.wav", riff(fmt(1, 2, 44100, 16), chunk(b"data", bytes(24))), (6, 2, 44100)),
             ("i24.wav", riff(fmt(1, 3, 96000, 24), chunk(b"data", bytes(27))), (3, 3, 96000)),
             ("i32.wav", riff(fmt(1, 1, 8000, 32), chunk(b"data", bytes(12))), (3, 1, 8000)),
             ("f32.wav", riff(fmt(3, 2, 48000, 32), chunk(b"data", bytes(32))), (4, 2, 48000)),
             ("ext16.wav", riff(chunk(b"LIST", b"abc"), fmt(1, 1, 22050, 16, extensible=True), chunk(b"data", bytes(8))), (4, 1, 22050)),
             ("extf.wav", riff(fmt(3, 2, 44100, 32, extensible=True), chunk(b"data", bytes(16))), (2, 2, 44100))]
    for name, image, want in cases:
        p = tmp_path / name
        p.write_bytes(image)
        oscen_amd.register_ir_wav("irc::wav", str(p))
        try:
            assert oscen_amd.registered_ir("irc::wav") == want, name
        finally:
            oscen_amd.unregister_ir("irc::wav")
    lib = oscen_amd.load_library()
    good = cases[0][1]
    bad = [("u8.wav", riff(fmt(1, 1, 8000, 8), chunk(b"data", bytes(8))), UNSUPPORTED, b"8 bits"),
           ("adpcm.wav", riff(fmt(2, 1, 8000, 4), chunk(b"data", bytes(8))), UNSUPPORTED, b""),
           ("f64.wav", riff(fmt(3, 1, 8000, 64), chunk(b"data", bytes(8))), UNSUPPORTED, b""),
           ("cut.wav", good[:-1], INVALID, b"data chunk declares"),
           ("head.wav", good[:20], INVALID, b""),
           ("empty.wav", riff(fmt(1, 2, 44100, 16), chunk(b"data", b"")), INVALID, b"empty"),
           ("zero_rate.wav", riff(fmt(1, 1, 0, 16), chunk(b"data", bytes(4))), INVALID, b"rate"),
           ("nine.wav", riff(fmt(1, 9, 44100, 16), chunk(b"data", bytes(18))), INVALID, b"channels")]
    for name, image, code, word in bad:
        p = tmp_path / name
        p.write_bytes(image)
        assert lib.og_register_ir_wav(b"irc::bad", str(p).encode()) == code, name
        assert word in lib.og_last_error(), (name, lib.og_last_error())
        assert info(lib, b"irc::bad") == INVALID  # nothing was registered
    assert lib.og_register_ir_wav(b"irc::bad", str(tmp_path / "nowhere.wav").encode()) == INVALID and b"cannot open" in lib.og_last_error()
    assert lib.og_register_ir_wav(None, b"x.wav") == INVALID and lib.og_register_ir_wav(b"irc::bad", None) == INVALID


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_python_surface_dispatch():
    try:
        oscen_amd.register_ir("irc::p", [1.0, 0.5, 0.25])  # 1-D without a rate: the old call, unchanged
        assert oscen_amd.registered_ir("irc::p") == (3, 1, None)
        oscen_amd.register_ir("irc::p", [])  # ... an empty response included
        assert oscen_amd.registered_ir("irc::p") == (0, 1, None)
        oscen_amd.register_ir("irc::p", [1.0, 0.5, 0.25], sample_rate=44100)  # a rate: the asset call
        assert oscen_amd.registered_ir("irc::p") == (3, 1, 44100)
        oscen_amd.register_ir("irc::p", np.zeros((5, 2), np.float32), sample_rate=96000)  # frames x channels
        assert oscen_amd.registered_ir("irc::p") == (5, 2, 96000)
        with pytest.raises(ValueError, match="sample_rate"):
            oscen_amd.register_ir("irc::p", np.zeros((5, 2), np.float32))  # an asset carries its rate
        with pytest.raises(ValueError):
            oscen_amd.register_ir("irc::p", np.zeros((5, 2, 2), np.float32), sample_rate=48000)
        with pytest.raises(oscen_amd.OscenError) as ei:
            oscen_amd.register_ir("irc::p", [], sample_rate=48000)  # AudioAsset::from_samples refuses an empty asset
        assert ei.value.code == INVALID
        assert oscen_amd.registered_ir("irc::p") == (5, 2, 96000)
    finally:
        oscen_amd.unregister_ir("irc::p")
    with pytest.raises(oscen_amd.OscenError):
        oscen_amd.registered_ir("irc::p")
    assert callable(oscen_amd.register_ir_wav) and callable(oscen_amd.Engine.bus_ir)


def wet_graph(ir_name):
    g = oscen_amd.Graph(builtin="sub_voice")
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.output_stream("wet")
    g.bus_convolver("reverb", ir_name)
    g.connect(out, "reverb.input")
    g.connect("reverb.output", "wet")
    return g


def test_with_ir_refuses_an_asset_at_lowering():
    oscen_amd.register_ir("irc::hall", np.ones((4, 2), np.float32), sample_rate=44100)
    try:
        with pytest.raises(oscen_amd.OscenError, match="og_set_bus_ir") as ei:
            wet_graph("irc::hall").kernel_source()
        assert ei.value.code == INVALID
        with pytest.raises(oscen_amd.OscenError, match="asset response") as ei:  # as a call with arguments, by its last segment
            wet_graph("hall(48000.0)").kernel_source()
        assert ei.value.code == INVALID
        oscen_amd.register_ir("irc::hall", [1.0, 0.5])  # the mono form under the same name lowers as it always did
        assert "og_k_" in wet_graph("irc::hall").kernel_source()
        assert "og_k_" in wet_graph(None).kernel_source()  # Convolver::new(): what an asset is published on
    finally:
        oscen_amd.unregister_ir("irc::hall")


# ---- symbols ----------------------------------------------------------------------------------------------------------------
def test_header_sys_crate_and_library_list_the_same_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oscen_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(og_[a-z_0-9]+)\s*\(", hdr))
    rs = open(os.path.join(ROOT, "bindings", "rust", "oscen-gpu-sys", "src", "lib.rs")).read()
    bound = set(re.findall(r"pub fn (og_\w+)\s*\(", rs))
    nm = subprocess.run(["nm", "-D", "--defined-only", b.LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()[-1].startswith("og_") and ln.split()[-2] in "TW"}
    assert declared == bound, sorted(declared ^ bound)
    assert declared == exported, sorted(declared ^ exported)
    for s in NEW_SYMBOLS:
        assert s in declared, s
    safe = open(os.path.join(ROOT, "bindings", "rust", "oscen-gpu", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS + ["og_set_bus_ir"]:
        assert "sys::%s(" % s in safe, s  # the safe crate reaches every one of them


# ---- kernels ----------------------------------------------------------------------------------------------------------------
# kernel_name() of the built-in graphs at the parent commit (the names in its committed csrc/gen/<graph>.hip)
PARENT_KERNELS = {
    "echo_voice": "og_k_ab2c9e6a58130339_00",
    "epiano_voice": "og_k_4a2495b0f6fccc78_00",
    "fm_voice": "og_k_6a8c619266f7cab3_00",
    "sat1x_voice": "og_k_2b74a838654fbfac_00",
    "sat4x_voice": "og_k_e4a361e8c12d6b85_00",
    "sub_voice": "og_k_7223270b2f3dc12a_00",
}


def test_no_built_in_kernel_was_renamed():
    for name, want in PARENT_KERNELS.items():
        g = oscen_amd.Graph(builtin=name)
        assert g.kernel_name() == want, name
        assert g.kernel_source() == open(os.path.join(b.GEN, name + ".hip")).read(), name
    digest = open(os.path.join(b.CSRC, "og_rt_digest.h")).read()
    for h in b.RT_HEADERS + [b.ADSRP_HEADER, b.SMP_HEADER, b.STAGEU_HEADER]:  # the bus kernels stay outside everything the digests cover
        assert "og_bus_conv" not in open(os.path.join(b.CSRC, h)).read(), h
    assert "og_bus_conv" not in digest


@pytest.mark.timeout(600)
def test_the_bus_kernels_compile_for_gfx950_within_their_budget(tmp_path):
    """the tap stride is a kernel argument added in front of the staging loop: og_bus_conv keeps its 3 KiB of LDS, no private
    segment and a register count that leaves occupancy bounded by the number of workgroups (header: ~40 VGPRs)"""
    hip = tmp_path / "bus.hip"
    hip.write_text('#include "og_bus_conv.hip.h"\n')
    r = subprocess.run([b.hipcc(), "--offload-arch=" + b.ARCH, "-x", "hip", "-c", "--cuda-device-only", str(hip), "-o", str(tmp_path / "bus.out"),
                        "-Rpass-analysis=kernel-resource-usage"] + b.COMMON, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    usage = {}
    for part in r.stdout.split("Function Name: ")[1:]:
        usage[part.split()[0]] = {k.strip(): int(v) for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", part)}
    kernels = {n: u for n, u in usage.items() if "og_bus_" in n}
    print({n: (u["VGPRs"], u["LDS Size [bytes/block]"]) for n, u in kernels.items()})
    assert len(kernels) == 4, sorted(usage)  # og_bus_conv, og_bus_conv_finish, og_bus_conv_move, og_bus_ir_planes
    for n, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)
        assert u["VGPRs"] <= 64, (n, u)
    conv = [u for n, u in kernels.items() if "og_bus_conv" in n and "finish" not in n and "move" not in n]
    assert len(conv) == 1 and conv[0]["LDS Size [bytes/block]"] == (256 + 256 + 256) * 4


# ---- sanitizers -------------------------------------------------------------------------------------------------------------
def clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if os.path.exists(c) or "/" not in c:
            return c


@pytest.mark.timeout(900)
def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """registry -> WAV parse -> channel mapping on host code, in a program with its own main (nothing is preloaded, nothing
    loaded into Python is instrumented)"""
    exe = str(tmp_path / "ir_asset_main")
    srcs = [os.path.join(ROOT, "tests", "standalone", "ir_asset_main.cpp")] + [os.path.join(b.CSRC, f) for f in ("og_wav.cpp", "og_graph.cpp", "og_builtin.cpp")]
    r = subprocess.run([clangxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "tests", "hostsim"), "-I" + b.CSRC] + srcs + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe, str(scratch)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "all asset response cases as expected" in r.stdout and "FAILED" not in r.stdout and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout
