"""Static and host-simulator checks of the zero variant (og_graph.cpp, ZeroChain): fm_voice has a second generated unit
(csrc/gen/fm_voice_z.hip) with the kernel without `env_filter * filter_env_amount + filter_cutoff` -- no Gain, no AddValue, no pipeline channel for the cutoff,
the filter's lazy update at the top of the launch -- next to general kernels that are unchanged (same text, same hash as
a generator with the variant turned off); its wide four-wave form does not spill, keeps four waves per SIMD and needs less LDS than the general one;
and tests/test_zero_variant_gpu.py passes, bit for bit, on the host simulator."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oscen_amd  # noqa: E402
from oscen_amd import build as b  # noqa: E402


def _ogc(*args, env=None):
    b.generate()
    return subprocess.run([os.path.join(b.BUILD, "ogc")] + list(args), env=env, stdout=subprocess.PIPE, text=True, check=True).stdout


def _sources():
    """(hash, general unit, zero unit, the zero unit's kernel namespace)"""
    src, zsrc = _ogc("fm_voice"), _ogc("--zero", "fm_voice")
    h = re.search(r"\bog_k_([0-9a-f]{16})_00\b", src).group(1)
    m = re.search(r"namespace og_gen_" + h + r"_z \{\n(.*?)\n\} // namespace\n", zsrc, flags=re.S)
    assert m, "no zero variant"
    return h, src, zsrc, m.group(1)


def test_the_zero_variant_leaves_out_the_chain():
    h, general, src, z = _sources()
    assert general == oscen_amd.Graph(builtin="fm_voice").kernel_source()
    # the general kernels carry the cutoff through a channel and test it every frame; the zero variant does neither
    assert "x8_n3_output * " in general and "chan11" in general
    assert " * RVP(7, 26)" not in z and " * RV(7, 26)" not in z and " + RVP(5, 20)" not in z and " + RV(5, 20)" not in z
    assert "n4_output" not in z and "n5_output" not in z and "chan11" not in z
    # the filter's update runs in derive(), off the slot, once per shape (ordinary, two-wave, four-wave)
    assert z.count("og::tpt_params_nomod_lazy<RAMPS, true>(SF(20), SF(21)") == 3
    assert "og::tpt_params_nomod_lazy<RAMPS, true>(x" not in z
    # the envelope still ticks, ends its stages and takes its gate events
    assert z.count("og::adsr_gate(n3_e, ev.value") == 3 and "og::adsr_complete(n3_e" in z
    for k in ("og_k_", "og_k2_", "og_k4_", "og_k4w_"):
        for v in ("00z", "01z"):
            assert re.search(r"void %s%s_%s\(OgBlockArgs A\) \{ og_gen_%s_z::" % (k, h, v, h), src), (k, v)
        assert k + h + "_10z" not in src and k + h + "_11z" not in src  # (a launch that ticks a ramp keeps the table kernels)


def test_the_general_kernels_are_unchanged():
    """the generator with the zero variant turned off (OGC_ZERO_SPEC=0) writes the same general unit, under the same hash"""
    off = _ogc("fm_voice", env=dict(os.environ, OSCEN_GPU_EXPERIMENTAL="1", OGC_ZERO_SPEC="0"))
    assert off == _ogc("fm_voice")
    assert _ogc("--zero", "fm_voice", env=dict(os.environ, OSCEN_GPU_EXPERIMENTAL="1", OGC_ZERO_SPEC="0")) == ""
    # graphs without such a chain have no zero unit
    for g in ("sub_voice", "sat4x_voice", "sat1x_voice", "epiano_voice", "echo_voice"):
        assert _ogc("--zero", g) == ""


def _chain_graph(consumer, port, ramp):
    """env -> Gain(amt) -> AddValue(base) -> <consumer>.<port>, the consumer filtering the envelope"""
    g = oscen_amd.Graph("zchain")
    g.input_event("gate")
    g.input_value("amt", 0.0, ramp=ramp)
    g.input_value("base", 800.0, ramp=ramp)
    g.output_stream("out")
    g.node("env", "AdsrEnvelope::new", 0.01, 0.1, 0.7, 0.2)
    g.node("eg", "Gain::new", 1.0)
    g.node("add", "AddValue::new", 0.0)
    g.node("f2", consumer, 1000.0, 0.7)
    g.connect("gate", "env.gate").connect("env.output", "eg.input").connect("amt", "eg.gain").connect("eg.output", "add.input")
    g.connect("base", "add.value").connect("add.output", "f2." + port).connect("env.output", "f2.input").connect("f2.output", "out")
    return g


@pytest.mark.parametrize("ramp", [0, 64])
@pytest.mark.parametrize("consumer,port", [("IirLowpass::new", "cutoff"), ("IirLowpass::new", "q"), ("TptFilter::new", "q"),
                                           ("TptFilter::new", "cutoff")])
def test_graphs_with_other_consumers_still_compile(consumer, port, ramp):
    """only a TPT cutoff is folded; any other consumer of the AddValue keeps the general kernel alone, and no chain ever
    costs a graph its compile"""
    src = _chain_graph(consumer, port, ramp).kernel_source()
    assert re.search(r"\bog_k_[0-9a-f]{16}_00\b", src) and "_z {" not in src


@pytest.mark.timeout(900)
def test_a_user_graph_with_a_tpt_cutoff_chain_compiles_with_its_zero_variant():
    # (the run-time compiler builds the general and the zero unit as one)
    assert _chain_graph("TptFilter::new", "cutoff", 64).jit_check() > 0


@pytest.mark.timeout(900)
def test_the_wide_zero_kernel_fits(tmp_path):
    h, general, zsrc, _ = _sources()
    hip, asm = tmp_path / "fm.hip", tmp_path / "fm.s"
    hip.write_text(general + zsrc)  # (one unit, as the run-time compiler builds it)
    r = subprocess.run([b.hipcc(), "--offload-arch=" + b.ARCH, "-x", "hip", "-S", "--cuda-device-only", str(hip), "-o", str(asm)] + b.COMMON,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    text = asm.read_text()

    def meta(kern):
        block = re.search(r"\.group_segment_fixed_size:\s+\d+\n(?:(?!\n  - ).)*?\.name:\s+" + kern + r"\n(?:(?!\n  - ).)*", text, flags=re.S)
        return dict(re.findall(r"\.(\w+):\s+(\S+)", block.group(0)))

    for v in ("00z", "01z"):
        m = meta("og_k4w_%s_%s" % (h, v))
        assert m["private_segment_fixed_size"] == "0" and m["vgpr_spill_count"] == "0", m
        assert int(m["vgpr_count"]) <= 128, m["vgpr_count"]  # (four waves per SIMD, as the general kernel)
        assert int(m["group_segment_fixed_size"]) < int(meta("og_k4w_%s_%s" % (h, v[:2]))["group_segment_fixed_size"]), m
    for k in ("og_k_", "og_k2_", "og_k4_"):
        for v in ("00", "01"):
            m, g = meta("%s%s_%sz" % (k, h, v)), meta("%s%s_%s" % (k, h, v))
            assert int(m["private_segment_fixed_size"]) <= int(g["private_segment_fixed_size"]), (k, v, m, g)
            # no fewer waves per SIMD than the general kernel: no more granules of 8 VGPRs, no more LDS
            assert (int(m["vgpr_count"]) + 7) // 8 <= (int(g["vgpr_count"]) + 7) // 8, (k, v, m["vgpr_count"], g["vgpr_count"])
            assert int(m["group_segment_fixed_size"]) <= int(g["group_segment_fixed_size"]), (k, v, m, g)


@pytest.mark.timeout(2400)
def test_the_zero_variant_on_the_host_simulator():
    """tests/test_zero_variant_gpu.py on the host simulator (tests/hostsim)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = build_hostsim.build()
    env.pop("OG_HOSTSIM_DEVICES", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "2000", "-p", "no:cacheprovider", "tests/test_zero_variant_gpu.py"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "10 passed" in r.stdout[-3000:], r.stdout[-3000:]
