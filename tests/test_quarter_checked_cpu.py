"""Static and host-simulator checks of the quiet quarters of a checked chunk (og_graph.cpp, PipelineWave::checked;
og_stage_uniform.hip.h has the argument): only the deeper zero variant's unit changes, and in it only the checked branch of the
three envelope stages of the four-wave template; the four-wave kernels of the unit still fit; and
tests/test_quarter_checked_gpu.py passes, bit for bit, on the host simulator, where the library counts the quarters."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oscen_amd import build as b  # noqa: E402

ARGS = {"fm_voice": ["fm_voice"], "fm_voice_z": ["--zero", "fm_voice"], "fm_voice_z2": ["--zero2", "fm_voice"]}
OFF = dict(os.environ, OSCEN_GPU_EXPERIMENTAL="1", OGC_STAGE_SPEC="0")
MC = ("n0_e.cnt", "n1_e.cnt", "min(n2_e.cnt, n3_e.cnt)")  # the stages' minimum countdowns, as their quiet tests have them


def _ogc(*args, env=None):
    b.generate()
    return subprocess.run([os.path.join(b.BUILD, "ogc")] + list(args), env=env, stdout=subprocess.PIPE, text=True, check=True).stdout


def _checked_branches(p4):
    """the text of the checked branch of each stage of voice_block_p4 that has one"""
    head = "// an event or a stage end in this chunk: the checked, unrolled body\n"
    return [part[:part.index("og::set_prio<BASE_PRIO>();")] for part in p4.split(head)[1:]]


def test_the_generated_text():
    for stem in ("fm_voice", "fm_voice_z"):  # the general and the `_z` unit: the committed files, switch or no switch
        text = _ogc(*ARGS[stem])
        assert open(os.path.join(b.GEN, stem + ".hip")).read() == text == _ogc(*ARGS[stem], env=OFF), stem
        assert "quarter" not in text, stem
    z2, off = _ogc(*ARGS["fm_voice_z2"]), _ogc(*ARGS["fm_voice_z2"], env=OFF)
    assert open(os.path.join(b.GEN, "fm_voice_z2.hip")).read() == z2
    assert "quarter" not in off and "for (uint32_t q = 0;" not in off
    p4 = z2[z2.index("void voice_block_p4("):]
    assert z2.count("og::quarter_count<") == p4.count("og::quarter_count<") == 6  # nowhere but in the four-wave template
    branches = _checked_branches(p4)
    assert len(branches) == 3  # stages 0-2; the filter stage has no countdown and no checked body
    for stage, (text, mc) in enumerate(zip(branches, MC)):
        # XCH / 4 quarters, unrolled; before each one the quarter test: the event horizon and the stage's minimum countdown
        assert text.count("#pragma unroll\n            for (uint32_t q = 0; q < XCH / 4u; ++q) {\n") == 1, stage
        test = "if (FD_T != 0 && __all((int)(c.next_ev >= base + 4u * q + 4u)) && __all((int)(%s > 4u))) {" % mc
        assert text.count(test) == 1 and text.count("__all(") == 2, stage
        body = text[text.index(test):]
        quiet, chk = body[:body.index("} else {")], body[body.index("} else {"):]
        for part in (quiet, chk):  # four frames each, `j` a constant of the unrolled loops
            assert part.count("#pragma unroll\n                    for (uint32_t i = 0; i < 4u; ++i) {\n                        const uint32_t j = 4u * q + i, f = base + j;\n") == 1, stage
        # the quiet quarter: the same tick site without stage-end checks, release arithmetic on, no table; no event test
        assert quiet.count("tick(f, ch, j, og::BoolC<false, true, true, false>{})") == 1 and "events(" not in quiet and "__any" not in quiet, stage
        assert "og::quarter_count<false>(%du);" % stage in quiet and "og::quarter_count<true>(%du);" % stage in chk, stage
        # the checked quarter: the frames as they were
        assert chk.count("if (__any((int)(f == c.next_ev))) events(f);") == 1 and chk.count("tick(f, ch, j, og::BoolC<true, true, true, false>{})") == 1, stage
        assert text.count("tick(") == 2 and "StageC" not in text, stage
        # (the two-envelope stage fences its checked frames: registers, see the next test)
        assert text.count("frame_sched_fence") == chk.count("if constexpr (FD_T != 0) og::frame_sched_fence();") == (1 if stage == 2 else 0), stage
    # s_setprio(3) stays around the whole chunk
    assert p4.count("__builtin_amdgcn_s_setprio(3); // the wave on the slow path is the straggler\n") == 3
    # what tests/test_stage_uniform_env_cpu.py pins: tick, gate and StageC sites
    assert z2.count("og::StageC<og::ENV_HOLD") == p4.count("og::StageC<og::ENV_HOLD") == 3
    assert z2.count("og::StageC<og::ENV_RELEASE") == p4.count("og::StageC<og::ENV_RELEASE") == 3
    for e in range(4):
        assert p4.count("og::adsr_tick_stage<og::env_mode(decltype(chk){}), decltype(chk)::release, decltype(chk)::table>(n%d_e, " % e) == 1, e
        assert z2.count("og::adsr_gate(n%d_e, ev.value" % e) == 3, e
        assert z2.count("og::adsr_complete(n%d_e" % e) == off.count("og::adsr_complete(n%d_e" % e), e


@pytest.mark.timeout(900)
def test_the_four_wave_kernels_still_fit(tmp_path):
    general, zsrc, z2src = (_ogc(*ARGS[s]) for s in ("fm_voice", "fm_voice_z", "fm_voice_z2"))
    h = re.search(r"\bog_k_([0-9a-f]{16})_00\b", general).group(1)
    hip, asm = tmp_path / "fm.hip", tmp_path / "fm.s"
    hip.write_text(zsrc + z2src)  # (the `_z` twins next to them; OG_JIT leaves the host side of the units out)
    r = subprocess.run([b.hipcc(), "--offload-arch=" + b.ARCH, "-x", "hip", "-S", "--cuda-device-only", "-DOG_JIT=1", str(hip), "-o", str(asm)] + b.COMMON,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    text = asm.read_text()

    def meta(kern):
        block = re.search(r"\.group_segment_fixed_size:\s+\d+\n(?:(?!\n  - ).)*?\.name:\s+" + kern + r"\n(?:(?!\n  - ).)*", text, flags=re.S)
        return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block.group(0))}

    for v in ("00", "01"):
        m, z = meta("og_k4w_%s_%sz2" % (h, v)), meta("og_k4w_%s_%sz" % (h, v))
        print("og_k4w_*_%sz2" % v, m, "twin", z)
        assert m["vgpr_count"] <= 128, m  # four waves per SIMD
        assert (m["vgpr_count"] + 7) // 8 <= (z["vgpr_count"] + 7) // 8, (m, z)  # ... and the `_z` twin's granule (tests/test_zero2_variant_cpu.py)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m  # no scratch, nothing spilled
        assert m["sgpr_spill_count"] <= z["sgpr_spill_count"], (m, z)
        assert m["group_segment_fixed_size"] <= 28768, (m, z)
        m, z = meta("og_k4_%s_%sz2" % (h, v)), meta("og_k4_%s_%sz" % (h, v))
        print("og_k4_*_%sz2" % v, m, "twin", z)
        assert (m["vgpr_count"] + 7) // 8 <= (z["vgpr_count"] + 7) // 8, (m, z)  # six workgroups per CU
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
        assert m["group_segment_fixed_size"] <= z["group_segment_fixed_size"], (m, z)


@pytest.mark.timeout(1500)
def test_the_quarters_on_the_host_simulator():
    """tests/test_quarter_checked_gpu.py on the host simulator (tests/hostsim): the general kernels and the deeper variant give
    the same bus and state bytes in every case, and there the single-hit case asserts from the library's counters that a chunk
    with one hit ran one checked and three quiet quarters in each operator stage (on a device the counters do not exist)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = build_hostsim.build()
    env.pop("OG_HOSTSIM_DEVICES", None)
    probe = ("import ctypes, oscen_amd; ctypes.c_ulonglong.in_dll(oscen_amd.load_library(), 'og_checked_quarters')")
    assert subprocess.run([sys.executable, "-c", probe], cwd=ROOT, env=env).returncode == 0  # (the counters are there to be read)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "1200", "-p", "no:cacheprovider", "tests/test_quarter_checked_gpu.py"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " passed" in r.stdout[-3000:] and "skipped" not in r.stdout[-3000:] and "failed" not in r.stdout[-3000:], r.stdout[-3000:]
