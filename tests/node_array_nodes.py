"""Custom nodes with per-voice ARRAY fields (og_node_array) and the graphs around them, shared by tests/test_node_arrays_cpu.py
and tests/test_node_arrays_gpu.py.  Their arithmetic is chosen so that IEEE pins every sample down whether or not a compiler
contracts a multiply-add: adds of two f32 and multiplies by a power of two (exact products).  Test helper."""
import oscen_amd

N_LINE = 1024

# a feedback comb: read `delay + 1` behind the write position, write input + d / 2, advance
COMB = dict(
    inputs=[("input", "stream", 0.0, -1), ("delay", "value", 0.0, 0)], outputs=["output"], n_ctor_args=1,
    state=[("wp", "u32", 0, -1)], arrays=[("buf", N_LINE, "f32", 0.0)],
    process="""
    const uint32_t dl = (uint32_t)delay;
    const float d = buf.get((wp + 1024u - dl - 1u) & 1023u);
    buf.set(wp, input + d * 0.5f);
    wp = (wp + 1u) & (buf.length() - 1u);
    output = d;
""")
# the same recurrence for delay = 0 with scalar state only
COMB0_SCALAR = dict(
    inputs=[("input", "stream", 0.0, -1)], outputs=["output"], state=[("y", "f32", 0.0, -1)],
    process="""
    const float d = y;
    y = input + d * 0.5f;
    output = d;
""")
# three fields of different lengths and element types; set(k, x) then get(k) inside one tick
MULTI = dict(
    inputs=[("input", "stream", 0.0, -1)], outputs=["output"], state=[("k", "u32", 0, -1)],
    arrays=[("one", 1, "f32", 0.25), ("five", 5, "f32", 1.5), ("cnt", 3, "u32", 7)],
    process="""
    const float t0 = five.get(0u);
    for (uint32_t i = 0u; i + 1u < five.length(); ++i) five.set(i, five.get(i + 1u));
    five.set(4u, t0 + input);
    cnt.set(k % 3u, cnt.get(k % 3u) + 1u);
    const float x = input * 2.0f;
    one.set(0u, x);
    output = one.get(0u) + five.get(0u);
    k += 1u;
""")
# indices past the end: clamped to the last element, for writes and reads
CLAMP = dict(
    inputs=[("input", "stream", 0.0, -1)], outputs=["output"],
    arrays=[("below", 2, "f32", 3.0), ("mid", 4, "f32", 1.0), ("above", 4, "f32", 2.0), ("ids", 3, "u32", 5)],
    process="""
    mid.set(mid.length() + 3u, input);
    ids.set(0xFFFFFFFFu, ids.get(77u) + 1u);
    output = mid.get(0xFFFFFFFFu);
""")
# a line the gate handler clears and loads with a burst
BURST = dict(
    inputs=[("gate", "event", 0.0, -1)], outputs=["output"], state=[("wp", "u32", 0, -1)], arrays=[("line", 64, "f32", 0.0)],
    process="""
    output = line.get(wp);
    line.set(wp, output * 0.5f);
    wp = (wp + 1u) & 63u;
""",
    handlers={"gate": """
    for (uint32_t i = 0u; i < line.length(); ++i) line.set(i, 0.0f);
    line.set(0u, value);
    line.set(1u, value * 0.5f);
    line.set(2u, value * 0.25f);
    wp = 0u;
"""})
# a per-voice table played in a loop
TABLE = dict(
    inputs=[], outputs=["output"], state=[("ph", "u32", 0, -1), ("acc", "f32", 0.0, -1)], arrays=[("table", 64, "f32", 0.0)],
    process="""
    output = table.get(ph & 63u);
    acc += output;
    ph += 1u;
""")
PASS = dict(inputs=[("input", "stream", 0.0, -1)], outputs=["output"], process="    output = input;\n")

ALL = {"UComb::new": COMB, "UComb0::new": COMB0_SCALAR, "UMulti::new": MULTI, "UClamp::new": CLAMP, "UBurst::new": BURST,
       "UTable::new": TABLE, "UPass::new": PASS}


def register(name, d=None, **over):
    d = dict(ALL[name] if d is None else d)
    d.update(over)
    oscen_amd.register_node(name, d["inputs"], d["outputs"], d["process"], state=d.get("state", ()), handlers=d.get("handlers"),
                            n_ctor_args=d.get("n_ctor_args", 0), arrays=d.get("arrays", ()))


def register_all():
    for name in ALL:
        register(name)


HEAD = """
name: %s;
input frequency: value = 220.0;
input delay: value = 0.0;
input gate: event;
output out: stream;
"""


def graph(name, nodes, connections):
    dsl = HEAD % name + "nodes {\n    osc = PolyBlepOscillator::saw(220.0, 0.3);\n" + nodes + "}\nconnections {\n    frequency -> osc.frequency;\n" + \
        connections + "}\n"
    return oscen_amd.Graph(dsl=dsl, per_voice=("frequency", "delay"))


def source_graph():
    """the oscillator alone: the bit-equal input of every model"""
    return graph("narr_source", "", "    osc.output -> out;\n")


def comb_graph(delay_arg=None, factor=1):
    """osc -> comb -> out; the delay per voice (delay_arg None) or the constructor's"""
    ctor = "UComb::new(%s)" % ("0.0" if delay_arg is None else repr(float(delay_arg))) + (" * %d" % factor if factor > 1 else "")
    conn = "    osc.output -> comb.input;\n" + ("    delay -> comb.delay;\n" if delay_arg is None else "") + "    comb.output -> out;\n"
    return graph("narr_comb", "    comb = %s;\n" % ctor, conn)


def delay_twin_graph(delay):
    return graph("narr_delay_twin", "    comb = Delay::new(%r, 0.5);\n" % float(delay), "    osc.output -> comb.input;\n    comb.output -> out;\n")


def comb0_scalar_graph(factor):
    return graph("narr_comb0", "    comb = UComb0::new() * %d;\n" % factor, "    osc.output -> comb.input;\n    comb.output -> out;\n")


def one_node_graph(name, ctor, feeds_input=True, gate=False):
    conn = ("    osc.output -> n.input;\n" if feeds_input else "") + ("    gate -> n.gate;\n" if gate else "") + "    n.output -> out;\n"
    return graph(name, "    n = %s;\n" % ctor, conn)


INSTANCE_DELAYS = {"combs[0]": 3, "combs[1]": 17, "combs[2]": 64, "first": 0, "second": 100}


def instances_graph():
    """a node array of three combs and two named ones, each with its own delay; their outputs summed in edge order"""
    nodes = "    combs = [UComb::new(0.0); 3];\n    first = UComb::new(0.0);\n    second = UComb::new(100.0);\n    sum = UPass::new();\n    mix = UPass::new();\n"
    conn = "    osc.output -> combs.input;\n    osc.output -> first.input;\n    osc.output -> second.input;\n" + \
        "".join("    %d.0 -> combs[%d].delay;\n" % (INSTANCE_DELAYS["combs[%d]" % k], k) for k in range(3)) + \
        "    combs.output -> sum.input;\n    sum.output -> mix.input;\n    first.output -> mix.input;\n    second.output -> mix.input;\n    mix.output -> out;\n"
    return graph("narr_instances", nodes, conn)
