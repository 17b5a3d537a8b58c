"""Generated text of the Delay's event rule ("Delay parameters and set-value events"): the handler of a per-voice
value input that a Delay's delay_samples or feedback depends on ends that Delay's fast path; no other graph changes.
(What the kernels compute: tests/test_delay_edges_gpu.py, which the host simulator runs in the CPU suite too.)"""
import oscen_amd


def _graph(name, dly, fb, other=False):
    g = oscen_amd.Graph(name)
    g.input_value("frequency", 440.0, per_voice=True)
    g.input_value("dly", 40.0, per_voice=dly)
    g.input_value("fb", 0.5, per_voice=fb)
    g.output_stream("out")
    g.node("osc", "PolyBlepOscillator::saw", 440.0, 0.5)
    g.node("d", "Delay::new", 40.0, 0.5)
    g.node("e", "Delay::new", 64.0, 0.25)
    g.connect("frequency", "osc.frequency").connect("osc.output", "d.input").connect("osc.output", "e.input")
    g.connect("dly * 2.0 + 1.0" if other else "dly", "d.delay_samples").connect("fb", "d.feedback")
    g.connect("d.output + e.output", "out")
    return g


def _handlers(src):
    return [l.strip() for l in src.splitlines() if "OG_EV_SETVALUE |" in l]


def test_a_set_value_event_on_a_delay_parameter_ends_the_fast_path_of_that_delay_only():
    h = _handlers(_graph("dev_vv", True, True).kernel_source())
    assert len(h) == 3  # frequency, dly, fb
    assert ".fast" not in h[0]  # the oscillator's frequency feeds no Delay parameter
    assert h[1].endswith("{ vin_1 = ev.value; derive(); n1_pre.fast = false; }")
    assert h[2].endswith("{ vin_2 = ev.value; derive(); n1_pre.fast = false; }")
    assert "n2_pre.fast = false" not in "".join(h)  # the second Delay's parameters are its fields

    # through an expression: Val::voice_inputs carries the dependence
    h = _handlers(_graph("dev_expr", True, False, other=True).kernel_source())
    assert len(h) == 2 and h[1].endswith("derive(); n1_pre.fast = false; }")


def test_graphs_without_a_per_voice_delay_parameter_keep_their_text():
    src = _graph("dev_uu", False, False).kernel_source()
    assert "og::ring_chunk_begin(" in src and ".fast = false" not in src
    for name in ("echo_voice", "fm_voice"):
        assert ".fast = false" not in oscen_amd.Graph(builtin=name).kernel_source()
