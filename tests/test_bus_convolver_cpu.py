"""The post-mix Convolver without a GPU: tests/test_bus_convolver_gpu.py executed on the host simulator (tests/hostsim/:
the engine's host code and the kernels of csrc/og_bus_conv.hip.h compiled for x86, every lane a fibre), the impulse-response
registry on its own, and the node's way through og_graph_to_dsl."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oscen_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")


@pytest.mark.timeout(900)
def test_gpu_tests_of_the_bus_convolver_on_the_host_simulator():
    sys.path.insert(0, HOSTSIM)
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    lib = build_hostsim.build()
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = lib
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(lib), "fake_rccl") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    env.pop("OG_HOSTSIM_DEVICES", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "300", "-p", "no:cacheprovider",
                        "tests/test_bus_convolver_gpu.py"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = r.stdout[-4000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", tail)
    assert m and int(m.group(1)) >= 26 and "failed" not in tail and "skipped" not in tail and "error" not in tail.lower(), tail


def lower(graph):
    return graph.kernel_source()


def wet_graph(ir_name):
    g = oscen_amd.Graph(builtin="sub_voice")
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.output_stream("wet")
    g.bus_convolver("reverb", ir_name)
    g.connect(out, "reverb.input")
    g.connect("reverb.output", "wet")
    return g


def test_registry():
    lib = oscen_amd.load_library()
    with pytest.raises(oscen_amd.OscenError, match="unknown impulse response 'hall'"):
        lower(wet_graph("hall"))
    oscen_amd.register_ir("rooms::hall", [1.0, 0.5, 0.25])
    try:
        lower(wet_graph("hall"))             # by the last segment of a longer registered path
        lower(wet_graph("rooms::hall"))      # as written
        lower(wet_graph("hall(48000.0)"))    # parentheses and arguments are ignored
        oscen_amd.register_ir("rooms::hall", np.ones(7, np.float32))  # a duplicate name replaces the earlier response
        oscen_amd.register_ir("silence", [])                          # an empty response is legal
        lower(wet_graph("silence"))
        one = np.ones(1, np.float32)
        assert lib.og_register_ir(b"bad", None, 3) == oscen_amd.OG_E_INVALID       # NULL taps with n > 0
        assert lib.og_register_ir(None, one.ctypes.data_as(C.POINTER(C.c_float)), 1) == oscen_amd.OG_E_INVALID
        with pytest.raises(oscen_amd.OscenError, match="not a path of identifiers"):
            oscen_amd.register_ir("no good", [1.0])
        oscen_amd.unregister_ir("silence")
        with pytest.raises(oscen_amd.OscenError, match="no impulse response 'silence'"):
            oscen_amd.unregister_ir("silence")
    finally:
        oscen_amd.unregister_ir("rooms::hall")
    with pytest.raises(oscen_amd.OscenError, match="unknown impulse response"):
        lower(wet_graph("hall"))
    lower(wet_graph(None))  # Convolver::new() needs no response


def test_a_duplicate_name_replaces_the_response_for_graphs_lowered_afterwards():
    """observable without a device: the 2^20-tap limit is checked at registration, so a replaced name takes the new taps"""
    oscen_amd.register_ir("r", [1.0])
    try:
        with pytest.raises(oscen_amd.OscenError) as ei:
            oscen_amd.register_ir("r", np.zeros((1 << 20) + 1, np.float32))
        assert ei.value.code == oscen_amd.OG_E_UNSUPPORTED
        lower(wet_graph("r"))  # the earlier registration is untouched by the refused one
    finally:
        oscen_amd.unregister_ir("r")


def test_refusals_at_lowering():
    oscen_amd.register_ir("room", [1.0, 0.5])
    try:
        body = """name: %s; input frequency: value = 220.0; input gate: event; output out: stream;
            nodes { osc = PolyBlepOscillator::saw(220.0, 0.2); reverb = Convolver::with_ir(room())%s; }
            connections { frequency -> osc.frequency; osc.output -> reverb.input; reverb.output -> out; }"""
        for name, rate in (("InVoice", ""), ("Oversampled", " * 2")):
            with pytest.raises(oscen_amd.OscenError, match="only available as the post-mix") as ei:
                lower(oscen_amd.Graph(dsl=body % (name, rate)))
            assert ei.value.code == oscen_amd.OG_E_UNSUPPORTED and "unknown node type" not in str(ei.value)
        g = wet_graph("room")
        g.bus_node("tremolo", "Tremolo::new")
        with pytest.raises(oscen_amd.OscenError, match="only one post-mix"):
            lower(g)
        g = wet_graph("room")
        g.connect("frequency", "reverb.rate")
        with pytest.raises(oscen_amd.OscenError, match="no input 'rate'"):
            lower(g)
    finally:
        oscen_amd.unregister_ir("room")


def test_to_dsl_round_trip():
    """the explicit description prints the node back with its response; the wrapper text -- where the node is an ordinary
    declaration -- parses back to the same text, and the e-piano's Tremolo line is what it was"""
    oscen_amd.register_ir("room", [1.0, 0.5])
    try:
        text = wet_graph("room").to_dsl()
        assert "post-mix (bus) node: reverb = Convolver::with_ir(room())" in text
        assert "post-mix: reverb.output -> wet;" in text
        assert "post-mix (bus) node: reverb = Convolver::new()" in wet_graph(None).to_dsl()
        assert "post-mix (bus) node: tremolo = Tremolo::new()" in oscen_amd.Graph(builtin="epiano_voice").to_dsl()
        wrapper = """name: Poly; input midi_in: event; output out: stream;
            nodes { midi_parser = MidiParser::new(); voice_allocator = VoiceAllocator::<4>::new();
                    voice_handlers = [MidiVoiceHandler::new(); 4]; voices = [FMVoice::new(); 4];
                    reverb = Convolver::<Frame<2>>::with_ir(rooms::room(48000.0)); }
            connections { midi_in -> midi_parser.midi_in; midi_parser.note_on -> voice_allocator.note_on;
                    midi_parser.note_off -> voice_allocator.note_off; voice_allocator.voices -> voice_handlers.note_on;
                    voice_allocator.voices -> voice_handlers.note_off; voice_handlers.frequency -> voices.frequency;
                    voice_handlers.gate -> voices.gate; voices.audio_out -> reverb.input; reverb.output -> out; }"""
        once = oscen_amd.Graph(dsl=wrapper).to_dsl()
        assert "reverb = Convolver::<Frame<2>>::with_ir(rooms::room(48000.0));" in once
        again = oscen_amd.Graph(dsl=once)
        assert again.to_dsl() == once
        with pytest.raises(oscen_amd.OscenError, match="Frame<2>"):  # FMVoice is mono
            lower(again)
        lower(oscen_amd.Graph(dsl=once.replace("::<Frame<2>>", "")))
    finally:
        oscen_amd.unregister_ir("room")
