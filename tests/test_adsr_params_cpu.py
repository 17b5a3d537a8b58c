"""AdsrEnvelope with attack / decay / sustain / release that move (a `[ramp: N]` input, a per-voice input, an expression
of one): the graph lowers onto og::AdsrP (csrc/og_adsr_params.hip.h) and compiles for gfx950 -- and a graph whose four
parameters are block-uniform generates the kernel it generated before, under the name it had.  CPU only (hiprtc
cross-compiles)."""
import re

import pytest

import oscen_amd

ENV = """
name: EnvParams%(tag)s;
input gate: event;
%(inputs)s
output out: stream;
nodes { env = AdsrEnvelope::new(0.002, 0.03, 0.5, 0.05)%(rate)s; }
connections { gate -> env.gate; %(wires)s %(out)s }
"""
PORTS = ("attack", "decay", "sustain", "release")


def env_graph(port, how, rate=1):
    tag = "%s_%s_%d" % (port, how, rate)
    out = "env.output -> out;" if rate == 1 else "[latch] env.output -> out;"
    if how == "ramp":
        return oscen_amd.Graph(dsl=ENV % dict(tag=tag, inputs="input p: value = 0.25 [ramp: 64];", wires="p -> env.%s;" % port,
                                              rate="" if rate == 1 else " * %d" % rate, out=out))
    if how == "voice":
        return oscen_amd.Graph(dsl=ENV % dict(tag=tag, inputs="input p: value = 0.25;", wires="p -> env.%s;" % port,
                                              rate="" if rate == 1 else " * %d" % rate, out=out), per_voice=["p"])
    assert how == "expr"
    return oscen_amd.Graph(dsl=ENV % dict(tag=tag, inputs="input base: value = 0.25;\ninput scale: value = 1.0;",
                                          wires="base * scale -> env.%s;" % port, rate="" if rate == 1 else " * %d" % rate, out=out),
                           per_voice=["base"])


@pytest.mark.parametrize("how", ["ramp", "voice", "expr"])
@pytest.mark.parametrize("port", PORTS)
def test_moving_parameter_lowers_and_compiles_for_gfx950(port, how):
    g = env_graph(port, how)
    src = g.kernel_source()
    assert '#include "og_adsr_params.hip.h"' in src and "og::adsrp_tick<false>(" in src
    assert "og::adsr_tick" not in src and "rcp_fetch" not in src  # no uniform body, no release table
    assert g.jit_check() > 0


def test_oversampled_envelope_and_builder_api():
    src = env_graph("release", "voice", rate=2).kernel_source()
    assert "og::adsrp_tick<true>(" in src
    assert env_graph("release", "voice", rate=2).jit_check() > 0
    g = oscen_amd.Graph("env_builder")
    g.input_event("gate")
    g.input_value("rel", 0.05, per_voice=True)
    g.input_value("sus", 0.5, ramp=32)
    g.output_stream("out")
    g.node("env", "AdsrEnvelope::new", 0.002, 0.03, 0.5, 0.05)
    g.connect("gate", "env.gate").connect("rel", "env.release").connect("sus", "env.sustain").connect("env.output", "out")
    assert "og::adsrp_tick<false>(" in g.kernel_source()
    assert g.jit_check() > 0


def test_state_planes_keep_the_four_words():
    a = oscen_amd.Graph(dsl=ENV % dict(tag="const", inputs="", wires="", rate="", out="env.output -> out;")).kernel_source()
    b = env_graph("release", "ramp").kernel_source()
    words = lambda s: int(re.search(r"(\d+) state words/voice", s).group(1))
    assert words(a) == words(b) == 4


CONST_DSL = """
name: AdsrConstParams;
input frequency: value = 220.0;
input gate: event;
output out: stream;
nodes {
    osc = PolyBlepOscillator::saw(220.0, 0.5);
    env = AdsrEnvelope::new(0.002, 0.03, 0.5, 0.05);
}
connections {
    frequency -> osc.frequency;
    gate -> env.gate;
    osc.output * env.output -> out;
}
"""
# og_k_<hash>_00 of these graphs as the PARENT commit (c9b84ba, before og::AdsrP existed) names them: generated there
# with this very code and pasted.  The hash covers the kernel body and the digest of the device headers it includes.
PARENT_HASHES = {"fm_voice": "6a8c619266f7cab3", "sub_voice": "7223270b2f3dc12a", "epiano_voice": "4a2495b0f6fccc78",
                 "dsl": "d9e3b8c3eb62ecdb"}


def test_uniform_parameter_kernels_are_the_parents():
    srcs = {b: oscen_amd.Graph(builtin=b).kernel_source() for b in ("fm_voice", "sub_voice", "epiano_voice")}
    srcs["dsl"] = oscen_amd.Graph(dsl=CONST_DSL, per_voice=["frequency"]).kernel_source()
    for name, src in srcs.items():
        assert "adsrp" not in src.lower() and "og_adsr_params" not in src, name
        assert re.search(r"\bog_k_([0-9a-f]{16})_00\b", src).group(1) == PARENT_HASHES[name], name
    assert "og::adsr_tick" in srcs["dsl"]


def test_array_valued_voice_keeps_the_refusal():
    # the electric piano's nodes keep [f32; 32] fields: one voice spans several lanes
    def ep(per_voice_release):
        g = oscen_amd.Graph("ep_env")
        g.input_value("frequency", 220.0, per_voice=True)
        g.input_value("rel", 0.05, per_voice=per_voice_release)
        g.input_event("gate")
        g.output_stream("out")
        g.node("amp", "AmplitudeSource::new")
        g.node("bank", "OscillatorBank::new")
        g.node("env", "AdsrEnvelope::new", 0.002, 0.03, 0.5, 0.05)
        for src, dst in (("frequency", "amp.frequency"), ("frequency", "bank.frequency"), ("gate", "amp.gate"), ("gate", "bank.gate"),
                         ("gate", "env.gate"), ("rel", "env.release"), ("amp.amplitudes", "bank.amplitudes"), ("bank.output * env.output", "out")):
            g.connect(src, dst)
        return g

    assert "og::adsr_tick" in ep(False).kernel_source()  # block-uniform parameters: as before
    with pytest.raises(oscen_amd.OscenError, match="array-valued"):
        ep(True).kernel_source()
