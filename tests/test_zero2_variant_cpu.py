"""Static and host-simulator checks of the deeper zero variant (og_graph.cpp, ZeroFolds): fm_voice has a third generated unit
(csrc/gen/fm_voice_z2.hip) whose kernels also leave out the operator feedbacks, the crossfade and the mixer that a patch
with op3_feedback = op2_feedback = route = 0 does not need -- next to a general unit and a zero unit that are unchanged
(same text as a generator with the variant turned off); a graph in which a candidate has another consumer gets no such
unit; the kernels need no more registers, scratch or LDS than their `_z` twins and do not flush f32 denormals (the
crossfade fold rests on x * 1.0f == x); and tests/test_zero2_variant_gpu.py passes, bit for bit, on the host simulator."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oscen_amd  # noqa: E402
from oscen_amd import build as b  # noqa: E402

OFF = dict(os.environ, OSCEN_GPU_EXPERIMENTAL="1", OGC_ZERO2_SPEC="0")


def _ogc(*args, env=None):
    b.generate()
    return subprocess.run([os.path.join(b.BUILD, "ogc")] + list(args), env=env, stdout=subprocess.PIPE, text=True, check=True).stdout


def _sources():
    """(hash, general unit, zero unit, deeper zero unit, the deeper unit's kernel namespace)"""
    src, zsrc, z2src = _ogc("fm_voice"), _ogc("--zero", "fm_voice"), _ogc("--zero2", "fm_voice")
    h = re.search(r"\bog_k_([0-9a-f]{16})_00\b", src).group(1)
    m = re.search(r"namespace og_gen_" + h + r"_z2 \{\n(.*?)\n\} // namespace\n", z2src, flags=re.S)
    assert m, "no deeper zero variant"
    return h, src, zsrc, z2src, m.group(1)


def test_the_general_and_the_zero_unit_are_unchanged():
    assert _ogc("fm_voice") == _ogc("fm_voice", env=OFF)
    assert _ogc("--zero", "fm_voice") == _ogc("--zero", "fm_voice", env=OFF) != ""
    assert _ogc("--zero2", "fm_voice", env=OFF) == ""
    for g in ("sub_voice", "sat4x_voice", "sat1x_voice", "epiano_voice", "echo_voice"):  # (no such folds: no unit)
        assert _ogc("--zero2", g) == ""
    # the committed units are what the generator writes
    for stem, args in (("fm_voice", ["fm_voice"]), ("fm_voice_z", ["--zero", "fm_voice"]), ("fm_voice_z2", ["--zero2", "fm_voice"])):
        assert open(os.path.join(b.GEN, stem + ".hip")).read() == _ogc(*args), stem


def test_the_deeper_unit_folds_feedback_crossfade_and_mixer():
    h, general, zsrc, src, z = _sources()
    assert "og::fm_operator_tick(" in general and "og::clamp01(" in general
    assert "og::fm_operator_tick(" not in z and z.count("og::fm_operator_tick_nofb(") == general.count("og::fm_operator_tick")
    assert "clamp01(" not in z and "output_b" not in z
    # the Mixer's add: the general kernels add the crossfade's output_b to op2; here op2 passes through
    assert re.search(r"const float n10_output = x\d+_n7_output \+ x\d+_n9_output_b;", general)
    assert not re.search(r"const float n\d+_output = \w+ \+ \w+;", z) and z.count("const float n10_output = x4_n7_output;") == 3
    # it has the zero variant's folds too
    assert "n4_output" not in z and "n5_output" not in z and z.count("og::tpt_params_nomod_lazy<RAMPS, true>(SF(20), SF(21)") == 3
    # every envelope still ticks, ends its stages and takes its gate events: three sites each (ordinary, two-wave, four-wave)
    for e in range(4):
        assert z.count("og::adsr_gate(n%d_e, ev.value" % e) == 3, e
        assert z.count("og::adsr_complete(n%d_e" % e) == general.count("og::adsr_complete(n%d_e" % e) >= 3, e
    # prev_output is still stored
    assert z.count("n6_prev_output);") == general.count("n6_prev_output);") and z.count("n7_prev_output);") == general.count("n7_prev_output);")
    for k in ("og_k_", "og_k2_", "og_k4_", "og_k4w_"):
        for v in ("00z2", "01z2"):
            assert re.search(r"void %s%s_%s\(OgBlockArgs A\) \{ og_gen_%s_z2::" % (k, h, v, h), src), (k, v)
        assert k + h + "_10z2" not in src and k + h + "_11z2" not in src  # (a launch that ticks a ramp keeps the table kernels)
    # the slots the engine tests: filter_env_amount's (26, the zero unit's) + op3_feedback 2, op2_feedback 9, route 19 must be
    # +-0; op3_level 1 and op2_level 8 must be finite
    assert re.search(r"slot\(s\) 26 hold", zsrc)
    assert re.search(r"slot\(s\) 2 9 19 26 hold \+-0,\n// slot\(s\) 1 8 are finite", src)
    assert ", 2);\n#endif" in src  # (registered as tier 2)


def _fm_graph(tap=None, fb=True):
    """two operators, the first through a Crossfade and a Mixer into the second's phase_mod -- FMVoice's routing in small.
    tap: an extra consumer of `node.port` (a Gain into the output)"""
    g = oscen_amd.Graph("zfold")
    g.input_value("frequency", 220.0)
    g.input_event("gate")
    g.input_value("fb", 0.0, ramp=64)
    g.input_value("route", 0.0, ramp=64)
    g.input_value("lvl", 1.0, ramp=64)
    g.output_stream("out")
    g.node("env", "AdsrEnvelope::new", 0.01, 0.1, 0.7, 0.2)
    for op in ("a", "b", "c"):
        g.node(op, "FmOperator::new")
    g.node("xf", "Crossfade::new")
    g.node("mx", "Mixer::new")
    g.connect("gate", "env.gate")
    for op in ("a", "b", "c"):
        g.connect("frequency", op + ".base_freq").connect("env.output", op + ".envelope").connect("lvl", op + ".level")
    if fb:
        g.connect("fb", "a.feedback")
    g.connect("a.output", "xf.input").connect("route", "xf.mix").connect("xf.output_a", "b.phase_mod")
    g.connect("b.output", "mx.input_a").connect("xf.output_b", "mx.input_b").connect("mx.output", "c.phase_mod")
    if tap:
        g.node("tapg", "Gain::new", 0.5)
        g.node("sum", "Mixer::new")
        g.connect(tap, "tapg.input").connect("c.output", "sum.input_a").connect("tapg.output", "sum.input_b").connect("sum.output", "out")
    else:
        g.connect("c.output", "out")
    return g


def test_a_qualifying_user_graph_has_the_unit():
    z2 = _fm_graph().variant_source(2)
    assert "_z2 {" in z2 and "clamp01(" not in z2 and "og::fm_operator_tick(" not in z2 and "output_b" not in z2
    assert _fm_graph().variant_source(1) == "" and _fm_graph().variant_source(0) == _fm_graph().kernel_source()


@pytest.mark.parametrize("tap", ["xf.output_a", "xf.output_b", "mx.output"])
def test_a_graph_whose_crossfade_or_mixer_has_another_consumer_keeps_them(tap):
    """a tap into a Gain: the Crossfade and the Mixer stay as they are.  (The operator's feedback, rule 1, has nothing to do
    with them and is still folded -- the unit exists, with the general crossfade and mixer in it.)"""
    g = _fm_graph(tap=tap)
    assert re.search(r"\bog_k_[0-9a-f]{16}_00\b", g.kernel_source())
    z2 = g.variant_source(2)
    assert "clamp01(" in z2 and re.search(r"const float n\d+_output = \w+ \+ \w+;", z2), z2[:400]
    # ... and without a feedback slot there is nothing left to fold: no unit
    assert _fm_graph(tap=tap, fb=False).variant_source(2) == ""


@pytest.mark.timeout(900)
def test_a_qualifying_user_graph_compiles_with_its_deeper_zero_variant():
    assert _fm_graph().jit_check() > 0  # (the run-time compiler builds all the units of a graph as one)


@pytest.mark.timeout(900)
def test_the_deeper_zero_kernels_fit(tmp_path):
    h, general, zsrc, z2src, _ = _sources()
    hip, asm = tmp_path / "fm.hip", tmp_path / "fm.s"
    hip.write_text(general + zsrc + z2src)  # (one unit, as the run-time compiler builds it)
    r = subprocess.run([b.hipcc(), "--offload-arch=" + b.ARCH, "-x", "hip", "-S", "--cuda-device-only", str(hip), "-o", str(asm)] + b.COMMON,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    text = asm.read_text()

    def meta(kern):
        block = re.search(r"\.group_segment_fixed_size:\s+\d+\n(?:(?!\n  - ).)*?\.name:\s+" + kern + r"\n(?:(?!\n  - ).)*", text, flags=re.S)
        return dict(re.findall(r"\.(\w+):\s+(\S+)", block.group(0)))

    def denorm_mode(kern):
        # FLOAT_DENORM_MODE_32 of the kernel descriptor: 3 = denormals kept on input and output
        d = re.search(r"\.amdhsa_kernel " + kern + r"\n(.*?)\.end_amdhsa_kernel", text, flags=re.S).group(1)
        return int(re.search(r"\.amdhsa_float_denorm_mode_32 (\d+)", d).group(1))

    for v in ("00", "01"):
        m, z = meta("og_k4w_%s_%sz2" % (h, v)), meta("og_k4w_%s_%sz" % (h, v))
        assert m["private_segment_fixed_size"] == "0" and m["vgpr_spill_count"] == "0", m
        assert int(m["vgpr_count"]) <= 128, m["vgpr_count"]  # (four waves per SIMD)
        assert int(m["group_segment_fixed_size"]) <= int(z["group_segment_fixed_size"]), (m, z)
    for k in ("og_k_", "og_k2_", "og_k4_", "og_k4w_"):
        for v in ("00", "01"):
            m, z = meta("%s%s_%sz2" % (k, h, v)), meta("%s%s_%sz" % (k, h, v))
            assert int(m["private_segment_fixed_size"]) <= int(z["private_segment_fixed_size"]), (k, v, m, z)
            assert (int(m["vgpr_count"]) + 7) // 8 <= (int(z["vgpr_count"]) + 7) // 8, (k, v, m["vgpr_count"], z["vgpr_count"])
            assert int(m["group_segment_fixed_size"]) <= int(z["group_segment_fixed_size"]), (k, v, m, z)
            # x * 1.0f == x for a denormal x only while f32 denormals are not flushed
            assert denorm_mode("%s%s_%sz2" % (k, h, v)) == 3, (k, v)


@pytest.mark.timeout(3000)
def test_the_deeper_zero_variant_on_the_host_simulator():
    """tests/test_zero2_variant_gpu.py on the host simulator (tests/hostsim)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = build_hostsim.build()
    env.pop("OG_HOSTSIM_DEVICES", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "2800", "-p", "no:cacheprovider", "tests/test_zero2_variant_gpu.py"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " passed" in r.stdout[-3000:] and "failed" not in r.stdout[-3000:] and "skipped" not in r.stdout[-3000:], r.stdout[-3000:]
