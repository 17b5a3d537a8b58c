"""Oscilloscope without a GPU: what the graph compiler makes of every constructor spelling (builder and text), the defaults, the
planes and state words a scope gets, every refusal with its code and a message that names the node, the argument errors of the
entry points, the gfx950 compile of the generated unit, the parity of header, Python mirror and -sys crate, and the stand-alone
program of tests/standalone/scope_main.cpp under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import pytest

import oscen_amd
from oscen_amd import build as b
from tests import scope_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = oscen_amd.OG_E_INVALID, oscen_amd.OG_E_UNSUPPORTED
NEW_SYMBOLS = ["og_scope_info", "og_read_scope", "og_clear_scope_triggered"]

DSL = """
name: %(name)s;
input frequency: value = 220.0;
input period: value = 64.0;
input en: value = 1.0 [ramp: 64];
output out: stream;
nodes {
    osc = PolyBlepOscillator::saw(220.0, 0.3);
    %(nodes)s
}
connections {
    frequency -> osc.frequency;
    %(edges)s
}
"""
WIRES = "osc.output -> scope.input; scope.output -> out;"


def text(ctor, edges=WIRES, name="scope_cpu", nodes=None):
    return oscen_amd.Graph(dsl=DSL % dict(name=name, nodes=nodes if nodes is not None else "scope = %s;" % ctor, edges=edges), per_voice=("frequency", "period"))


def built(ctor, *args, rate=1):
    g = oscen_amd.Graph("scope_built")
    g.input_value("frequency", 220.0, per_voice=True)
    g.output_stream("out")
    g.node("osc", "PolyBlepOscillator::saw", 220.0, 0.3)
    g.node("scope", ctor, *args, rate=rate)
    g.connect("frequency", "osc.frequency").connect("osc.output", "scope.input").connect("scope.output", "out")
    return g


def begin(src):
    """(capacity, ring base, window base) of every scope of a kernel source"""
    return [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in
            re.finditer(r"= og::scope_begin<(\d+)u>\(narr_pool, (\d+)u, (\d+)u, A\.n_voices, c\.v, c\.valid, ", src)]


def tick(src):
    m = re.search(r"og::scope_tick<(true|false), (\d+)u>\(\w+, (\w+), ([^,]+), ([^,]+), ", src)
    return m.group(1) == "true", int(m.group(2)), m.group(4), m.group(5)


def body(src):
    """a kernel source without what names the constructor: the `// scope = Type::ctor` comments and the hash in the entry names"""
    return re.sub(r"[0-9a-f]{16}", "#", "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("//")))


def refused(code, words, make):
    with pytest.raises(oscen_amd.OscenError) as ei:
        make().kernel_source()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_the_model_gives_the_references_known_answers():
    assert sm.known_answers()


def test_every_constructor_spelling_lowers_to_the_same_node():
    want = text("Oscilloscope::new(64)").kernel_source()
    assert tick(want) == (False, 64, "0x1p+6f", "0x1p+0f")  # trigger_period = capacity, trigger_enabled = 1.0
    assert begin(want) == [(64, 0, 144)]                      # the ring: 2 x 64 + 16 planes, the window behind it
    for g in (text("Oscilloscope::with_handle(OscilloscopeHandle::new(64))"), text("Oscilloscope::with_handle(64)"),
              text("Oscilloscope::with_handle( OscilloscopeHandle::new( 64usize ) )")):
        assert body(g.kernel_source()) == body(want)
    auto = text("Oscilloscope::with_auto_detect(OscilloscopeHandle::new(64))").kernel_source()
    assert tick(auto) == (True, 64, "0x1p+6f", "0x1p+0f") and body(auto) != body(want)
    assert body(text("Oscilloscope::with_auto_detect(64)").kernel_source()) == body(auto)
    # the builder API: the capacity is the one numeric argument of all three
    new = built("Oscilloscope::new", 64).kernel_source()
    assert tick(new)[:2] == (False, 64) and body(built("Oscilloscope::with_handle", 64).kernel_source()) == body(new)
    assert tick(built("Oscilloscope::with_auto_detect", 64).kernel_source())[:2] == (True, 64)
    # capacity.max(1); the largest capacity
    assert begin(text("Oscilloscope::new(0)").kernel_source()) == [(1, 0, 32)]
    assert begin(text("Oscilloscope::with_handle(OscilloscopeHandle::new(0))").kernel_source()) == [(1, 0, 32)]
    assert begin(built("Oscilloscope::new", 65536).kernel_source()) == [(65536, 0, 2 * 65536 + 16)]


def test_kernel_source_of_a_graph_with_a_scope():
    src = text("Oscilloscope::new(256)").kernel_source()
    assert src.count('#include "og_scope.hip.h"') == 1 and src.index('#include "og_node_array.hip.h"') < src.index('#include "og_scope.hip.h"')
    assert "og::narr_word* const narr_pool = og::node_array_pool(A, " in src
    assert src.count("og::scope_chunk_begin<256u>(") >= 1 and src.count("og::scope_tick<false, 256u>(") == 1
    assert "voice_block_p2" not in src and "voice_block_p4" not in src  # the ordinary kernel only
    digest = open(os.path.join(b.CSRC, "og_rt_digest.h")).read()
    assert "OG_SCOPE_DIGEST" in digest and "og_scope.hip.h" in digest
    # the value inputs take what a value port takes: per voice, ramped, a node output, an expression
    src = text("Oscilloscope::new(64)", WIRES + " period -> scope.trigger_period; en -> scope.trigger_enabled;").kernel_source()
    assert re.search(r"og::scope_tick<false, 64u>\(\w+, \w+, vin_\d+, RV\(0, \d+\), ", src)
    src = text("Oscilloscope::new(64)", WIRES + " period * 0.5 + 1.0 -> scope.trigger_period; osc.output -> scope.trigger_enabled;").kernel_source()
    assert "og::scope_tick<false, 64u>(" in src
    # a node array and two named scopes: disjoint runs of planes
    g = text(None, "osc.output -> a.input; osc.output -> s.input; osc.output -> z.input; a.output -> out; s[0].output -> m.input_a; s[1].output -> m.input_b; m.output -> out; z.output -> out;",
             nodes="a = Oscilloscope::new(16); s = [Oscilloscope::new(16); 2]; z = Oscilloscope::with_auto_detect(OscilloscopeHandle::new(7)); m = Mixer::new();")
    got = sorted(begin(g.kernel_source()), key=lambda t: t[1])
    assert [t[0] for t in got].count(16) == 3 and [t[0] for t in got].count(7) == 1
    spans = sorted([(r, r + (48 if c == 16 else 32)) for c, r, f in got] + [(f, f + c) for c, r, f in got])
    assert spans[0][0] == 0 and all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1))


def test_graphs_without_a_scope_know_nothing_of_it():
    for name in ("fm_voice", "sub_voice", "echo_voice", "epiano_voice", "sat1x_voice", "sat4x_voice"):
        src = oscen_amd.Graph(builtin=name).kernel_source()
        assert "scope" not in src and src == open(os.path.join(b.GEN, name + ".hip")).read(), name


def test_refusals_name_the_node():
    refused(UNSUPPORTED, ["'scope'", "shared_handle.clone()", "OscilloscopeHandle::new"], lambda: text("Oscilloscope::with_handle(shared_handle.clone())"))
    refused(UNSUPPORTED, ["'scope'", "OscilloscopeHandle::new"], lambda: text("Oscilloscope::with_auto_detect(OscilloscopeHandle::new(n))"))
    refused(INVALID, ["'scope'", "not a number"], lambda: text("Oscilloscope::new(OscilloscopeHandle::new(64))"))
    refused(INVALID, ["'scope'", "non-negative integer"], lambda: built("Oscilloscope::new", 6.5))
    refused(INVALID, ["'scope'", "non-negative integer"], lambda: built("Oscilloscope::new", -1.0))
    refused(INVALID, ["'scope'", "takes 1 arguments"], lambda: built("Oscilloscope::new"))
    refused(UNSUPPORTED, ["'scope'", "65537", "65536"], lambda: built("Oscilloscope::new", 65537))
    refused(UNSUPPORTED, ["'scope'", "65537"], lambda: text("Oscilloscope::with_handle(OscilloscopeHandle::new(65537))"))
    refused(UNSUPPORTED, ["'scope'", "oversampled"], lambda: text("Oscilloscope::new(64) * 2"))
    refused(UNSUPPORTED, ["'scope'", "oversampled"], lambda: built("Oscilloscope::new", 64, rate=4))
    refused(UNSUPPORTED, ["'scope'", "handle", "og_read_scope"], lambda: text(None, WIRES + " scope.handle -> g.gain; osc.output -> g.input; g.output -> out;",
                                                                               nodes="scope = Oscilloscope::new(64); g = Gain::new(1.0);"))
    refused(UNSUPPORTED, ["1048576"], lambda: text(None, "osc.output -> s.input; s.output -> out;", nodes="s = [Oscilloscope::new(65536); 6];"))
    # an array-valued voice ([f32; 32] nodes)
    dsl = oscen_amd.Graph(builtin="epiano_voice").to_dsl()
    out_name = re.search(r"output (\w+): stream", dsl).group(1)
    src_name = re.search(r"(\w+\.\w+) -> %s;" % out_name, dsl).group(1)
    dsl = dsl.replace("nodes {", "nodes {\n    scope = Oscilloscope::new(64);", 1).replace(
        "connections {", "connections {\n    %s -> scope.input;\n    scope.output -> %s;" % (src_name, out_name), 1)
    refused(UNSUPPORTED, ["'scope'", "array-valued voice"], lambda: oscen_amd.Graph(dsl=dsl, per_voice=("frequency",)))
    # a post-mix graph: the host receives the bus itself
    def post():
        g = oscen_amd.Graph(builtin="sub_voice")
        g.output_stream("wet")
        g.bus_node("trim", "Gain::new", 0.5)
        g.bus_node("scope", "Oscilloscope::new", 64)
        g.connect("audio", "trim.input").connect("trim.output", "scope.input").connect("scope.output", "wet")
        return g
    refused(UNSUPPORTED, ["'scope'", "post-mix"], post)


def test_the_generated_unit_compiles_for_gfx950():
    assert text("Oscilloscope::new(256)").jit_check("gfx950") > 0
    assert text("Oscilloscope::with_auto_detect(OscilloscopeHandle::new(7))", WIRES + " period -> scope.trigger_period; en -> scope.trigger_enabled;").jit_check("gfx950") > 0


def test_header_python_mirror_sys_crate_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "oscen_gpu.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "oscen-gpu-sys", "src", "lib.rs")).read()
    lib = oscen_amd.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and re.search(r"pub fn %s\(" % s, rs) and hasattr(lib, s), s
        c_args = re.search(r"\bint %s\(([^;]*)\);" % s, hdr).group(1).count(",")
        assert re.search(r"pub fn %s\(([^;]*)\) -> c_int;" % s, rs).group(1).count(",") == c_args == len(getattr(lib, s).argtypes) - 1


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = oscen_amd.load_library()
    assert lib.og_scope_info(None, b"scope", None, None) == INVALID
    assert lib.og_read_scope(None, b"scope", 0, 0, 4, None, None, None, None) == INVALID
    assert lib.og_clear_scope_triggered(None, b"scope", None, 0) == INVALID


# ---- sanitizers -------------------------------------------------------------------------------------------------------------
def clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if os.path.exists(c) or "/" not in c:
            return c


@pytest.mark.timeout(600)
def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """og_scope_host.h over hand-built planes, in a program with its own main (nothing is preloaded, nothing loaded into Python is
    instrumented)"""
    exe = str(tmp_path / "scope_main")
    r = subprocess.run([clangxx(), "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + b.CSRC, os.path.join(ROOT, "tests", "standalone", "scope_main.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "all scope host cases as expected" in r.stdout and "FAILED" not in r.stdout and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout
