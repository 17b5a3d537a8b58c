"""Post-mix graphs without a GPU: how a wrapper with nodes behind its voice sum is lowered (the partition into the voices and
a second compiled graph, csrc/og_graph.cpp split_post_mix / compile_post), what is refused, the new entry points in the
header, the library and the Rust crates, the post-mix unit through hipcc for gfx950, and the host-only bookkeeping
(tests/standalone/post_mix_main.cpp) as a program of its own, also under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

import oscen_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oscen_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "standalone", "post_mix_main.cpp")
HOST_SRCS = [os.path.join(CSRC, f) for f in ("og_graph.cpp", "og_builtin.cpp", "og_dsl.cpp")]

WRAPPER = """name: Poly; input midi_in: event; input cut: value = 1200.0 [ramp: 300]; input vol: value = 0.5; output out: stream; %(outputs)s
    nodes { midi_parser = MidiParser::new(); voice_allocator = VoiceAllocator::<4>::new();
            voice_handlers = [MidiVoiceHandler::new(); 4]; voices = [FMVoice::new(); 4];
            %(nodes)s }
    connections { midi_in -> midi_parser.midi_in; midi_parser.note_on -> voice_allocator.note_on;
            midi_parser.note_off -> voice_allocator.note_off; voice_allocator.voices -> voice_handlers.note_on;
            voice_allocator.voices -> voice_handlers.note_off; voice_handlers.frequency -> voices.frequency;
            voice_handlers.gate -> voices.gate;
            %(edges)s }"""
MASTER_NODES = "lfo = Oscillator::sine(0.3, 1.0); master = TptFilter::new(1200.0, 0.707); echo = Delay::new(4800.0, 0.4); trim = Gain::new(0.5);"
MASTER_EDGES = ("voices.audio_out -> master.input; lfo.output * 800.0 + cut -> master.cutoff; master.output -> [echo] -> trim.input; "
                "vol -> trim.gain; trim.output -> out;")


def wrapper(nodes="", edges="voices.audio_out -> out;", outputs=""):
    return oscen_amd.Graph(dsl=WRAPPER % dict(nodes=nodes, edges=edges, outputs=outputs))


def bus_chain(nodes, edges, inputs=()):
    """the builder form: sub_voice plus post-mix nodes (og_graph_add_bus_node)"""
    g = oscen_amd.Graph(builtin="sub_voice")
    for name, default, ramp in inputs:
        g.input_value(name, default, ramp=ramp)
    g.output_stream("wet")
    for name, ctor, *args in nodes:
        g.bus_node(name, ctor, *args)
    for e in edges:
        (g.connect_via if len(e) == 3 else g.connect)(*e)
    return g


def test_lowering_partitions_the_wrapper():
    g = wrapper(MASTER_NODES, MASTER_EDGES + " voices.audio_out -> dry;", "output dry: stream;")
    post = g.post_mix_source()
    head = post[:post.index("#include")]
    assert "The post-mix kernel" in head and "1 ramped inputs" in head and "1 channel(s) in, 2 out" in head
    order = re.search(r"// Node order: (.*)", head).group(1).split()
    assert sorted(order) == ["echo", "lfo", "master", "trim"] and order.index("lfo") < order.index("master")
    for name in ("lfo", "master", "echo", "trim"):
        assert "// %s = " % name in post and "// %s = " % name not in g.kernel_source()
    assert "og::post_fetch_ahead(" in post and "og::post_store(" in post and "og::bus_put" not in post and "og::bus_chunk_reduce" not in post
    assert "og::post_fetch" not in g.kernel_source()
    # the wrapper's broadcast inputs keep their ramp rows: the ramped cutoff is read per frame, the plain gain from its slot
    assert re.search(r"RV\(0, \d+\)", post) and "og::delay_tick(" in post


def test_the_voice_kernel_is_the_one_of_the_wrapper_without_post_mix_nodes():
    plain = wrapper()
    with_post = wrapper(MASTER_NODES, MASTER_EDGES)
    assert with_post.kernel_name() == plain.kernel_name()
    assert with_post.kernel_source() == plain.kernel_source()
    assert plain.post_mix_source() == ""
    for tier in (1, 2):
        assert with_post.variant_source(tier) == plain.variant_source(tier)
    # ... and the builder form over a built-in voice keeps the committed kernel
    g = bus_chain([("trim", "Gain::new", 0.5)], [("audio", "trim.input"), ("trim.output", "wet")])
    assert g.kernel_name() == oscen_amd.Graph(builtin="sub_voice").kernel_name()
    assert g.kernel_name()[:-3] in open(os.path.join(CSRC, "gen", "sub_voice.hip")).read()


def test_the_post_mix_unit_has_its_own_entries():
    post = wrapper(MASTER_NODES, MASTER_EDGES).post_mix_source()
    names = re.findall(r'extern "C" __global__ __launch_bounds__\(64\) void (og_kp_[0-9a-f]{16}_(?:00|10))\(OgBlockArgs A\)', post)
    assert len(names) == 2 and names[0][:-2] == names[1][:-2] and names[0].endswith("_00") and names[1].endswith("_10")
    assert '#include "og_post_mix.hip.h"' in post
    digest = re.search(r'#define OG_PM_DIGEST "([0-9a-f]{16})"', open(os.path.join(CSRC, "og_rt_digest.h")).read()).group(1)
    import hashlib
    assert digest == hashlib.sha256(open(os.path.join(CSRC, "og_post_mix.hip.h"), "rb").read()).hexdigest()[:16]
    # another post-mix graph, another kernel; the same one, the same
    other = wrapper("trim = Gain::new(0.5);", "voices.audio_out -> trim.input; trim.output -> out;").post_mix_source()
    assert re.search(r"og_kp_[0-9a-f]{16}", other).group(0) != names[0][:-3]
    assert wrapper(MASTER_NODES, MASTER_EDGES).post_mix_source() == post


def test_to_dsl_round_trips():
    once = wrapper(MASTER_NODES, MASTER_EDGES).to_dsl()
    for line in ("lfo = Oscillator::sine(", "echo = Delay::new(", "master.output -> [echo] -> trim.input;"):
        assert line in once, once
    again = oscen_amd.Graph(dsl=once)
    assert again.to_dsl() == once
    assert again.post_mix_source() == wrapper(MASTER_NODES, MASTER_EDGES).post_mix_source()
    text = bus_chain([("trim", "Gain::new", 0.5)], [("audio", "trim.input"), ("trim.output", "wet")]).to_dsl()
    assert "post-mix (bus) node: trim = Gain::new(0.5)" in text and "post-mix: trim.output -> wet;" in text


def refused(graph, match, code=oscen_amd.OG_E_UNSUPPORTED):
    with pytest.raises(oscen_amd.OscenError, match=match) as ei:
        graph.kernel_source()
    assert ei.value.code == code, str(ei.value)


def test_refusals():
    t = "trim = Gain::new(0.5); "
    tin = "voices.audio_out -> trim.input; trim.output -> out; "
    refused(wrapper("tremolo = Tremolo::new(); " + t, "voices.audio_out -> tremolo.input; tremolo.output -> trim.input; trim.output -> out;"),
            r"node 'tremolo'.*only one post-mix")
    oscen_amd.register_ir("pm_room", [1.0, 0.5])
    try:
        refused(wrapper("reverb = Convolver::with_ir(pm_room()); " + t, "voices.audio_out -> reverb.input; reverb.output -> trim.input; trim.output -> out;"),
                r"node 'reverb'.*only one post-mix")
    finally:
        oscen_amd.unregister_ir("pm_room")
    refused(wrapper("master = TptFilter::new(1200.0, 0.707) * 2;", "voices.audio_out -> master.input; master.output -> out;"), r"node 'master'.*oversampled")
    refused(wrapper(t + "sp = SamplePlayer::new();", tin + "sp.output -> trim.gain;"), r"node 'sp'.*SamplePlayer")
    oscen_amd.register_node("PmHistory::new", inputs=[("input", "stream", 0.0, -1)], outputs=["output"], process="    output = line.get(0u); line.set(0u, input);\n",
                            arrays=[("line", 8, "f32", 0.0)])
    try:
        refused(wrapper("h = PmHistory::new();", "voices.audio_out -> h.input; h.output -> out;"), r"node 'h'.*array fields")
    finally:
        oscen_amd.unregister_node("PmHistory::new")
    refused(wrapper("lfo = Oscillator::sine(0.3, 1.0); master = TptFilter::new(1200.0, 0.707);",
                    "voices.audio_out -> master.input; lfo.output -> master.cutoff; lfo.output -> voices.filter_cutoff; master.output -> out;"),
            r"node 'lfo' feeds both the voices and the post-mix node 'master'")
    refused(wrapper("master = TptFilter::new(1200.0, 0.707);", "voices.audio_out -> master.input; master.output -> voices.filter_cutoff; master.output -> out;"),
            r"post-mix node output feeds back into the voices \(.*master\.output")
    # the builder form: an event edge and a per-voice input into a post-mix node
    env = [("env", "AdsrEnvelope::new", 0.01, 0.1, 0.7, 0.2), ("trim", "Gain::new", 0.5)]
    refused(bus_chain(env, [("audio", "trim.input"), ("gate", "env.gate"), ("env.output", "trim.gain"), ("trim.output", "wet")]),
            r"post-mix node 'env': an event edge")
    refused(bus_chain([("trim", "Gain::new", 0.5)], [("audio", "trim.input"), ("frequency", "trim.gain"), ("trim.output", "wet")]),
            r"post-mix node 'trim': a per-voice input")


TWO_OUT_VOICE = """name: PmTwoOut; input frequency: value = 220.0; input gate: event; output a: stream; output b: stream;
    nodes { osc = PolyBlepOscillator::saw(220.0, 0.2); env = AdsrEnvelope::new(0.01, 0.1, 0.7, 0.2); }
    connections { frequency -> osc.frequency; gate -> env.gate; osc.output * env.output -> a; osc.output -> b; }"""


def test_more_than_one_voice_output_into_the_post_mix_graph_is_refused():
    oscen_amd.register_graph_type("PmTwoOut", oscen_amd.Graph(dsl=TWO_OUT_VOICE, per_voice=("frequency",)))
    try:
        text = (WRAPPER.replace("FMVoice", "PmTwoOut")) % dict(outputs="", nodes="ma = Gain::new(0.5); mb = Gain::new(0.5);",
                                                                edges="voices.a -> ma.input; voices.b -> mb.input; ma.output + mb.output -> out;")
        refused(oscen_amd.Graph(dsl=text), r"more than one voice output feeds the post-mix graph")
        text = (WRAPPER.replace("FMVoice", "PmTwoOut")) % dict(outputs="output dry: stream;", nodes="ma = Gain::new(0.5);",
                                                                edges="voices.a -> ma.input; ma.output -> out; voices.b -> dry;")
        refused(oscen_amd.Graph(dsl=text), r"more than one voice output feeds the post-mix graph")
    finally:
        oscen_amd.unregister_graph_type("PmTwoOut")


def test_in_voice_convolver_and_lone_stages_keep_their_messages():
    body = """name: InVoice; input frequency: value = 220.0; input gate: event; output out: stream;
        nodes { osc = PolyBlepOscillator::saw(220.0, 0.2); reverb = Convolver::new(); }
        connections { frequency -> osc.frequency; osc.output -> reverb.input; reverb.output -> out; }"""
    refused(oscen_amd.Graph(dsl=body), "only available as the post-mix")
    epiano = oscen_amd.Graph(builtin="epiano_voice")
    assert epiano.post_mix_source() == "" and "og_bus_tremolo" not in epiano.kernel_source()
    assert "post-mix (bus) node: tremolo = Tremolo::new()" in epiano.to_dsl()


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "oscen_gpu.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "oscen-gpu-sys", "src", "lib.rs")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "oscen-gpu", "src", "lib.rs")).read()
    lib = oscen_amd.load_library()
    for name in ("og_post_mix_info", "og_read_post_mix_input"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
        assert "pub fn %s(" % name in sys_rs and "sys::%s(" % name in shim, name
    assert header.count("uint32_t* n_nodes, uint32_t* in_channels, uint32_t* out_channels, uint32_t* state_words") == 1
    assert sys_rs.count("n_nodes: *mut u32, in_channels: *mut u32, out_channels: *mut u32, state_words: *mut u32") == 1
    assert lib.og_post_mix_info(None, None, None, None, None) == oscen_amd.OG_E_INVALID
    assert lib.og_read_post_mix_input(None, None, 0) == oscen_amd.OG_E_INVALID
    assert lib.og_post_mix_kind(None) == 0
    # the header's account of og_graph_add_bus_node is the new one
    doc = header[header.rindex("/*", 0, header.index("int og_graph_add_bus_node(")):header.index("int og_graph_add_bus_node(")]
    assert "POST-MIX GRAPH" in doc and "OG_E_UNSUPPORTED" in doc


def hipcc():
    for c in ("/opt/rocm/bin/hipcc", "hipcc"):
        if os.path.exists(c) or "/" not in c:
            return c


@pytest.mark.timeout(600)
def test_the_test_chains_post_mix_unit_compiles_for_gfx950(tmp_path):
    g = bus_chain([("master", "TptFilter::new", 1200.0, 0.707), ("echo", "Delay::new", 37.0, 0.4), ("trim", "Gain::new", 0.5)],
                  [("audio", "master.input"), ("cut", "master.cutoff"), ("master.output", "echo", "trim.input"), ("trim.output", "wet")],
                  inputs=[("cut", 1200.0, 300)])
    src = tmp_path / "post_mix_unit.hip"
    src.write_text(g.post_mix_source())
    r = subprocess.run([hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-x", "hip", "-c", str(src), "-o", str(tmp_path / "unit.o"), "-O3", "-std=c++17",
                        "-ffp-contract=off", "-fno-slp-vectorize", "-DOG_JIT=1", "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    kernels = re.findall(r"Function Name: (og_kp_[0-9a-f]{16}_(?:00|10))", r.stdout)
    assert len(kernels) == 2, r.stdout[-3000:]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    print(re.findall(r"(?:VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): \d+", r.stdout))
    assert scratch == [0, 0]  # the chunk's staged frames and collected outputs are registers: nothing is indexed at run time
    assert g.jit_check() > 0  # ... and both units through hiprtc, as og_create compiles them


def run_and_check(exe):
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.rstrip().endswith("ok")
    counts = {name: int(n) for name, n in re.findall(r"^path (\w+) (\d+)$", r.stdout, flags=re.M)}
    assert len(counts) >= 20 and all(n > 0 for n in counts.values()), counts
    for must in ("partition_master_section", "compiled_beside_the_plain_wrapper", "legacy_not_split", "section_round_trip", "refuse_magic", "refuse_cut_short_body"):
        assert must in counts, must


def test_post_mix_host_header_compiles_without_hip():
    h = os.path.join(CSRC, "og_post_mix_host.h")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", h], check=True)
    assert "hip" not in re.sub(r"//.*", "", open(h).read()).lower()


@pytest.mark.timeout(600)
def test_partition_and_snapshot_section_in_a_program_of_their_own(tmp_path):
    exe = tmp_path / "post_mix_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, MAIN] + HOST_SRCS + ["-o", str(exe)], check=True)
    run_and_check(exe)


def clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if os.path.exists(c) or "/" not in c:
            return c


@pytest.mark.timeout(900)
def test_the_same_program_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "post_mix_main_san"
    r = subprocess.run([clangxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + CSRC, MAIN] + HOST_SRCS + ["-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    run_and_check(exe)
