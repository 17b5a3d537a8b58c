"""SamplePlayer without a GPU: the sample registry's argument checks, the entry points' null checks, the four contexts the
lowering refuses, which kernels include csrc/og_sample_player.hip.h, a gfx950 compile of the mono and the Frame<2> graph,
and `external`, which the text front end still refuses.  (What needs an ENGINE -- an unknown node, an unknown index, a voice
range out of bounds -- is checked by tests/test_sample_player_gpu.py::test_engine_entry_points_refuse_bad_arguments, which
tests/test_sample_player_hostsim_cpu.py runs on the host simulator.)"""
import ctypes as C

import numpy as np
import pytest

import oscen_amd

f32p = C.POINTER(C.c_float)
INVALID, UNSUPPORTED = oscen_amd.OG_E_INVALID, oscen_amd.OG_E_UNSUPPORTED


def player(ctor="SamplePlayer::new()", name="Player", extra_nodes="", out="player.output -> out;", rate=""):
    return oscen_amd.Graph(dsl="name: %s; output out: stream; nodes { player = %s%s; %s } connections { %s }" % (name, ctor, rate, extra_nodes, out))


def test_registry_argument_validation():
    lib = oscen_amd.load_library()
    a = np.arange(16, dtype=np.float32)
    p = a.ctypes.data_as(f32p)
    assert lib.og_register_sample(None, p, 4, 1) == INVALID                      # null name
    assert lib.og_register_sample(b"", p, 4, 1) == INVALID
    assert lib.og_register_sample(b"spc_x", p, 4, 0) == INVALID                  # zero channels
    assert lib.og_register_sample(b"spc_x", p, 1, 9) == INVALID and b"channels" in lib.og_last_error()  # more than 8
    assert lib.og_register_sample(b"spc_x", None, 4, 1) == INVALID               # frames without data
    # over the size bound (checked before a byte is read): frames * channels > 2^28
    assert lib.og_register_sample(b"spc_x", p, (1 << 28) + 1, 1) == INVALID and b"2^28" in lib.og_last_error()
    assert lib.og_register_sample(b"spc_x", p, (1 << 25) + 1, 8) == INVALID
    assert lib.og_register_sample(b"spc_x", p, 1 << 62, 8) == INVALID            # (no overflow in the product)
    assert lib.og_unregister_sample(b"spc_x") == INVALID                         # none of the above registered anything
    assert lib.og_unregister_sample(None) == INVALID
    assert lib.og_register_sample(b"spc_x", p, 2, 8) == 0                        # 8 channels is the most
    assert lib.og_register_sample(b"spc_x", None, 0, 1) == 0                     # replaced by an empty one: legal
    assert lib.og_unregister_sample(b"spc_x") == 0
    oscen_amd.register_sample("spc_y", np.zeros((5, 2)))
    oscen_amd.unregister_sample("spc_y")
    with pytest.raises(oscen_amd.OscenError, match="no sample 'spc_y'"):
        oscen_amd.unregister_sample("spc_y")
    with pytest.raises(ValueError):
        oscen_amd.register_sample("spc_y", np.zeros((2, 2, 2)))


def test_engine_and_cluster_entry_points_refuse_null_arguments():
    lib = oscen_amd.load_library()
    out = C.c_uint32(0)
    idx = (C.c_uint32 * 1)(0)
    u32p = C.POINTER(C.c_uint32)
    assert lib.og_load_sample(None, b"x", C.byref(out)) == INVALID
    assert lib.og_set_sample(None, b"player", 0) == INVALID
    assert lib.og_set_voice_samples(None, b"player", 0, 1, C.cast(idx, u32p)) == INVALID
    assert lib.og_cluster_load_sample(None, b"x", C.byref(out)) == INVALID
    assert lib.og_cluster_set_sample(None, b"player", 0) == INVALID
    assert lib.og_cluster_set_voice_samples(None, b"player", 0, 1, C.cast(idx, u32p)) == INVALID
    assert oscen_amd.SAMPLE_NONE == 0xFFFFFFFF


def refused(build, *words):
    with pytest.raises(oscen_amd.OscenError) as ei:
        build().kernel_source()
    assert ei.value.code == UNSUPPORTED, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)


def test_the_four_refused_contexts_name_themselves():
    # inside an array-valued voice (the electric piano's [f32; 32] nodes)
    def array_valued():
        g = oscen_amd.Graph(builtin="epiano_voice")
        g.node("player", "SamplePlayer::new")
        out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
        g.connect("player.output", out)
        return g

    refused(array_valued, "player", "array-valued voice")

    # in a node array
    def node_array():
        g = oscen_amd.Graph("PlayerArray")
        g.output_stream("out")
        g.node_array("players", "SamplePlayer::new", length=3)
        g.connect("players.output", "out")
        return g

    refused(node_array, "players", "node array")

    # in a nested graph type
    inner = oscen_amd.Graph(dsl="name: InnerPlayer; output out: stream; nodes { p = SamplePlayer::new(); } connections { p.output -> out; }")
    oscen_amd.register_graph_type("InnerPlayer", inner)
    try:
        refused(lambda: oscen_amd.Graph(dsl="name: Outer; output out: stream; nodes { inner = InnerPlayer::new(); } connections { inner.out -> out; }"),
                "inner", "nested graph type")
    finally:
        oscen_amd.unregister_graph_type("InnerPlayer")
    # in an oversampled domain
    refused(lambda: player(rate=" * 2", name="Over"), "player", "oversampled")
    # ... and more than four players is a malformed graph, not a missing feature
    with pytest.raises(oscen_amd.OscenError) as ei:
        oscen_amd.Graph(dsl="name: Five; output out: stream; nodes { a = SamplePlayer::new(); b = SamplePlayer::new(); c = SamplePlayer::new(); "
                            "d = SamplePlayer::new(); e = SamplePlayer::new(); } connections { a.output + b.output + c.output + d.output + e.output -> out; }").kernel_source()
    assert ei.value.code == INVALID and "at most 4 SamplePlayer" in str(ei.value)


def test_only_player_graphs_include_the_header():
    src = player().kernel_source()
    assert '#include "og_sample_player.hip.h"' in src and "og::player_chunk_begin<1>" in src and "og::player_tick<1>" in src
    assert "og_k2_" not in src and "og_k4_" not in src  # the ordinary kernel only, as with a Delay
    st = player("SamplePlayer::<Frame<2>>::new()", name="Player2").kernel_source()
    assert "og::Player<2>" in st
    for builtin in ("fm_voice", "sub_voice", "echo_voice"):
        assert "og_sample_player" not in oscen_amd.Graph(builtin=builtin).kernel_source(), builtin


@pytest.mark.parametrize("ctor", ["SamplePlayer::new()", "SamplePlayer::<Frame<2>>::new()"])
def test_player_graphs_compile_for_gfx950(ctor):
    assert player(ctor, name="Jit" + str(len(ctor))).jit_check("gfx950") > 0


def test_external_is_still_refused_by_the_text_front_end():
    with pytest.raises(oscen_amd.OscenError) as ei:
        oscen_amd.Graph(dsl="name: PlayerGraph; output stream out; external sample: AudioAsset; nodes { player = SamplePlayer::new(); } "
                            "connections { sample -> player.buf; player.output -> out; }")
    assert "external" in str(ei.value)
