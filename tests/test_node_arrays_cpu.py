"""Per-voice ARRAY fields of custom nodes (og_node_array) without a GPU: registration and its refusals, what the graph compiler
generates for them (the header, one view per instance and field, distinct planes), that graphs without such a field know
nothing of it, the gfx950 compile of the test graphs, the parity of header, Python mirror and -sys crate, and the stand-alone
program of tests/standalone/node_array_main.cpp under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import pytest

import oscen_amd
from oscen_amd import build as b
from tests import node_array_nodes as nn
from tests import plugin_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = oscen_amd.OG_E_INVALID, oscen_amd.OG_E_UNSUPPORTED
NEW_SYMBOLS = ["og_node_array_info", "og_read_node_array", "og_write_node_array"]


@pytest.fixture(scope="module", autouse=True)
def _nodes():
    nn.register_all()
    yield
    for name in nn.ALL:
        oscen_amd.unregister_node(name)


def refused(code, word, **kw):
    d = dict(nn.COMB)
    d.update(kw)
    with pytest.raises(oscen_amd.OscenError) as ei:
        nn.register("URefused::new", d)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def views(src):
    """(variable, element type, length, base) of every view a kernel source constructs"""
    return [(m.group(1), m.group(2), int(m.group(3)), int(m.group(4))) for m in
            re.finditer(r"og::NodeArray<\w+, \d+u> (\w+) = og::node_array<(\w+), (\d+)u>\(narr_pool, (\d+)u, A\.n_voices, c\.v, c\.valid\);", src)]


def test_registration_accepts_arrays_and_refuses_malformed_ones():
    nn.register("UAccepted::new", nn.COMB, arrays=[("buf", 1, "f32", 0.0), ("tab", 65536, "u32", 9), ("c", 5, "f32", -1.5)])
    oscen_amd.unregister_node("UAccepted::new")
    nn.register("UAccepted::new", nn.COMB, arrays=[("a%d" % k, 2, "f32", 0.0) for k in range(8)])  # eight is the most
    oscen_amd.unregister_node("UAccepted::new")
    refused(INVALID, "duplicate", arrays=[("buf", 4, "f32", 0.0), ("buf", 4, "f32", 0.0)])
    refused(INVALID, "duplicate", arrays=[("wp", 4, "f32", 0.0)])      # a state field's name
    refused(INVALID, "duplicate", arrays=[("output", 4, "f32", 0.0)])  # an output's
    refused(INVALID, "identifier", arrays=[("2nd", 4, "f32", 0.0)])
    refused(INVALID, "reserved", arrays=[("sample_rate", 4, "f32", 0.0)])
    refused(INVALID, "length 0", arrays=[("buf", 0, "f32", 0.0)])
    refused(INVALID, "at most 8", arrays=[("a%d" % k, 2, "f32", 0.0) for k in range(9)])
    refused(UNSUPPORTED, "65536", arrays=[("buf", 65537, "f32", 0.0)])
    lib = oscen_amd.load_library()
    t = oscen_amd._NodeType(b"URefused::new", 0, None, 0, None, 0, None, 0, b"", None, 0, None, 0, None, 0, None, 1)  # n_arrays without arrays
    assert lib.og_register_node(C.byref(t)) == INVALID
    with pytest.raises(oscen_amd.OscenError):
        oscen_amd.unregister_node("URefused::new")  # nothing of the refused registrations stayed


def test_a_type_without_arrays_registers_and_lowers_as_before():
    src = plugin_nodes.user_fm_voice().kernel_source()
    assert "og_node_array" not in src and "narr" not in src and "NodeArray" not in src
    for name in ("fm_voice", "sub_voice", "echo_voice", "epiano_voice", "sat4x_voice"):
        s = oscen_amd.Graph(builtin=name).kernel_source()
        assert "og_node_array" not in s and "NodeArray" not in s, name
    s = nn.comb0_scalar_graph(2).kernel_source()  # a custom node with scalar state only
    assert "og_node_array" not in s and "NodeArray" not in s


def test_the_builtin_kernels_keep_their_names():
    """the committed ahead-of-time units are what the generator writes now: no built-in kernel changed its text or hash"""
    for name in ("fm_voice", "sub_voice", "echo_voice", "epiano_voice", "sat1x_voice", "sat4x_voice"):
        committed = open(os.path.join(b.GEN, name + ".hip")).read()
        assert oscen_amd.Graph(builtin=name).kernel_source() == committed, name
    digest = open(os.path.join(b.CSRC, "og_rt_digest.h")).read()
    assert "OG_NARR_DIGEST" in digest and "og_node_array.hip.h" in digest


def test_kernel_source_of_a_graph_with_array_fields():
    src = nn.comb_graph().kernel_source()
    assert src.count('#include "og_node_array.hip.h"') == 1 and src.index('#include "og_nodes.hip.h"') < src.index('#include "og_node_array.hip.h"')
    assert "og::narr_word* const narr_pool = og::node_array_pool(A, " in src
    assert "og::NodeArray<float, 1024u>& buf" in src  # the parameter of process()
    assert [v[1:] for v in views(src)] == [("float", 1024, 0)]
    assert "voice_block_p2" not in src and "voice_block_p4" not in src  # the ordinary kernel only: one wave owns a voice's planes
    # a node array of three and two named instances: five views, five disjoint runs of planes
    v = views(nn.instances_graph().kernel_source())
    assert len(v) == 5 and len({x[0] for x in v}) == 5
    assert sorted(x[3] for x in v) == [0, 1024, 2048, 3072, 4096]
    # two instances of one type, each with an f32 and a u32 field
    g = nn.graph("narr_two", "    a = UClamp::new();\n    b = UClamp::new();\n",
                 "    osc.output -> a.input;\n    osc.output -> b.input;\n    a.output -> out;\n    b.output -> out;\n")
    v = views(g.kernel_source())
    assert [(x[1], x[2]) for x in v] == [("float", 2), ("float", 4), ("float", 4), ("uint32_t", 3)] * 2
    spans = sorted((x[3], x[3] + x[2]) for x in v)
    assert spans[0][0] == 0 and all(spans[k][1] == spans[k + 1][0] for k in range(len(spans) - 1))  # back to back, none shared
    # the handler receives the views as well
    src = nn.one_node_graph("narr_burst", "UBurst::new()", feeds_input=False, gate=True).kernel_source()
    assert re.search(r"og_user_UBurst__new_on_gate\(const float value, uint32_t& wp, og::NodeArray<float, 64u>& line, const float sample_rate\)", src)
    # an oversampled node and a nested graph type
    assert len(views(nn.comb_graph(delay_arg=0, factor=2).kernel_source())) == 1
    oscen_amd.register_graph_type("NarrInner", nn.comb_graph(delay_arg=5))
    try:
        outer = oscen_amd.Graph(dsl="""
name: narr_outer;
input frequency: value = 220.0;
output out: stream;
nodes { x = NarrInner::new(); y = NarrInner::new(); }
connections { frequency -> x.frequency; frequency -> y.frequency; x.out + y.out -> out; }
""", per_voice=("frequency",))
        assert sorted(t[3] for t in views(outer.kernel_source())) == [0, 1024]
    finally:
        oscen_amd.unregister_graph_type("NarrInner")


def test_graphs_with_array_fields_compile_for_gfx950():
    assert nn.comb_graph().jit_check("gfx950") > 0
    assert nn.one_node_graph("narr_multi", "UMulti::new()").jit_check("gfx950") > 0  # f32 and u32 arrays in one node
    assert nn.one_node_graph("narr_burst", "UBurst::new()", feeds_input=False, gate=True).jit_check("gfx950") > 0


def test_array_valued_voices_and_oversized_graphs_are_refused():
    # the electric-piano voice spans several lanes per voice ([f32; 32] nodes): a node with array fields there is refused by name
    dsl = oscen_amd.Graph(builtin="epiano_voice").to_dsl()
    assert "nodes {" in dsl and "connections {" in dsl
    dsl = dsl.replace("nodes {", "nodes {\n    extra = UTable::new();", 1).replace("connections {", "connections {\n    extra.output -> out;", 1)
    out_name = re.search(r"output (\w+): stream", dsl).group(1)
    dsl = dsl.replace("extra.output -> out;", "extra.output -> %s;" % out_name)
    with pytest.raises(oscen_amd.OscenError) as ei:
        oscen_amd.Graph(dsl=dsl, per_voice=("frequency",)).kernel_source()
    assert ei.value.code == UNSUPPORTED and "array-valued voice" in str(ei.value) and "extra" in str(ei.value)
    # 2^20 array words per voice over a graph
    nn.register("UBig::new", nn.PASS, arrays=[("big", 65536, "f32", 0.0)])
    try:
        def big(k):
            return nn.graph("narr_big", "    t = [UBig::new(); %d];\n" % k, "    osc.output -> t.input;\n    t.output -> out;\n")
        assert len(views(big(16).kernel_source())) == 16  # exactly 2^20
        with pytest.raises(oscen_amd.OscenError) as ei:
            big(17).kernel_source()
        assert ei.value.code == UNSUPPORTED and "1048576" in str(ei.value)
    finally:
        oscen_amd.unregister_node("UBig::new")


def test_header_python_mirror_sys_crate_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "oscen_gpu.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "oscen-gpu-sys", "src", "lib.rs")).read()
    lib = oscen_amd.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr) and re.search(r"pub fn %s\(" % s, rs) and hasattr(lib, s), s
    # og_node_array, field by field; og_node_type ends with `arrays`, `n_arrays` in all three
    body = re.search(r"typedef struct \{([^}]*)\} og_node_array;", hdr).group(1)
    c_fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert c_fields == ["name", "length", "is_uint", "init", "init_uint"] == [f[0] for f in oscen_amd._NodeArray._fields_]
    rs_body = re.search(r"pub struct og_node_array \{([^}]*)\}", rs).group(1)
    assert re.findall(r"pub (\w+):", rs_body) == c_fields
    node_type = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{((?:(?!typedef).)*)\} og_node_type;", hdr, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+);", node_type)[-3:] == ["event_queue_capacity", "arrays", "n_arrays"]
    assert [f[0] for f in oscen_amd._NodeType._fields_][-3:] == ["event_queue_capacity", "arrays", "n_arrays"]
    assert re.findall(r"pub (\w+):", re.search(r"pub struct og_node_type \{([^}]*)\}", rs).group(1))[-3:] == ["event_queue_capacity", "arrays", "n_arrays"]
    assert "OG_NODE_ARRAY_MAX_LEN 65536u" in hdr and "OG_NODE_ARRAYS_MAX 8u" in hdr
    assert re.search(r"OG_NODE_ARRAY_MAX_LEN: u32 = 65536", rs) and re.search(r"OG_NODE_ARRAYS_MAX: u32 = 8", rs)


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = oscen_amd.load_library()
    assert lib.og_node_array_info(None, b"a.b", None, None) == INVALID
    assert lib.og_read_node_array(None, b"a.b", 0, 0, None) == INVALID
    assert lib.og_write_node_array(None, b"a.b", 0, 0, None) == INVALID


# ---- sanitizers -------------------------------------------------------------------------------------------------------------
def clangxx():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if os.path.exists(c) or "/" not in c:
            return c


@pytest.mark.timeout(900)
def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """registration copy -> validation -> planes -> rows <-> planes -> snapshot section head on host code, in a program with its
    own main (nothing is preloaded, nothing loaded into Python is instrumented)"""
    exe = str(tmp_path / "node_array_main")
    srcs = [os.path.join(ROOT, "tests", "standalone", "node_array_main.cpp")] + [os.path.join(b.CSRC, f) for f in ("og_graph.cpp", "og_builtin.cpp")]
    r = subprocess.run([clangxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I" + b.CSRC] + srcs + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "all node-array host cases as expected" in r.stdout and "FAILED" not in r.stdout and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout
