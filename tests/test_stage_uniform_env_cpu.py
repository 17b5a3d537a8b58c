"""Static and host-simulator checks of the stage-uniform envelope bodies (og_stage_uniform.hip.h; og_graph.cpp,
PipelineWave::fast_variants): only the deeper zero variant's unit changes -- the general and the zero unit keep their text
and the kernels their hash, and the generator's switch gives the unit's earlier text back; the four-wave kernels of the
unit still fit (registers, scratch, LDS, workgroups per CU); and tests/test_stage_uniform_env_gpu.py passes, bit for bit,
on the host simulator, where the library counts the chunks run in the two new bodies."""
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oscen_amd import build as b  # noqa: E402

# sha256 of the three fm_voice units as the commit before this one had them
BEFORE = {"fm_voice": "1e51d2eebb8dbc27863a78a2abcce8e6f8e510fc443513052a9ccc5e92f9977e",
          "fm_voice_z": "613d17de4df373589f9ea0de36a9aae4624169b33ccf512911e5acc0d969c404",
          "fm_voice_z2": "1c76f5dc1f697333f95764fb7ddd70b933e686649408127ec04f5585b8b1d8a8"}
ARGS = {"fm_voice": ["fm_voice"], "fm_voice_z": ["--zero", "fm_voice"], "fm_voice_z2": ["--zero2", "fm_voice"]}
OFF = dict(os.environ, OSCEN_GPU_EXPERIMENTAL="1", OGC_STAGE_SPEC="0")


def _ogc(*args, env=None):
    b.generate()
    return subprocess.run([os.path.join(b.BUILD, "ogc")] + list(args), env=env, stdout=subprocess.PIPE, text=True, check=True).stdout


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def test_only_the_deeper_unit_changes_and_the_switch_gives_its_earlier_text():
    for stem in ("fm_voice", "fm_voice_z"):
        text = _ogc(*ARGS[stem])
        assert _sha(text) == BEFORE[stem], stem
        assert open(os.path.join(b.GEN, stem + ".hip")).read() == text == _ogc(*ARGS[stem], env=OFF), stem
    z2 = _ogc(*ARGS["fm_voice_z2"])
    assert open(os.path.join(b.GEN, "fm_voice_z2.hip")).read() == z2
    assert _sha(z2) != BEFORE["fm_voice_z2"] and _sha(_ogc(*ARGS["fm_voice_z2"], env=OFF)) == BEFORE["fm_voice_z2"]
    # the general hash (the kernels' names) is the one of the general unit
    h = re.search(r"\bog_k_([0-9a-f]{16})_00\b", _ogc("fm_voice")).group(1)
    assert ("og_k4w_%s_00z2(" % h) in z2 and ("og_k4_%s_01z2(" % h) in z2
    # two more chunk flags per envelope stage in the four-wave template and nowhere else; no new tick, gate or stage-end site
    assert '#include "og_stage_uniform.hip.h"' in z2 and "og_stage_uniform" not in _ogc("fm_voice") + _ogc("--zero", "fm_voice")
    p4 = z2[z2.index("void voice_block_p4("):]
    assert z2.count("og::StageC<og::ENV_HOLD") == p4.count("og::StageC<og::ENV_HOLD") == 3
    assert z2.count("og::StageC<og::ENV_RELEASE") == p4.count("og::StageC<og::ENV_RELEASE") == 3
    for e in range(4):
        assert p4.count("og::adsr_tick_stage<og::env_mode(decltype(chk){}), decltype(chk)::release, decltype(chk)::table>(n%d_e, " % e) == 1, e
        assert z2.count("og::adsr_gate(n%d_e, ev.value" % e) == 3, e
    # stage 2 holds two envelopes: its bodies are entered only when both qualify
    assert "og::adsr_holds(n2_e) && og::adsr_holds(n3_e)" in p4 and "og::adsr_releases(n2_e) && og::adsr_releases(n3_e)" in p4
    for g in ("sub_voice", "sat4x_voice", "sat1x_voice", "epiano_voice", "echo_voice"):  # (no deeper variant: nothing to change)
        assert _ogc(g) == _ogc(g, env=OFF) and _ogc("--zero2", g) == ""


@pytest.mark.timeout(900)
def test_the_four_wave_kernels_of_the_unit_still_fit(tmp_path):
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
        assert m["vgpr_count"] <= 128, m  # (four waves per SIMD)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m  # nothing goes to memory
        # (scalar registers parked in VGPR lanes, v_writelane / v_readlane outside the chunk loops: the `_z` twin has two, and so
        #  has this kernel since the bodies were added)
        assert m["sgpr_spill_count"] <= z["sgpr_spill_count"], (m, z)
        assert m["group_segment_fixed_size"] <= 28768 and z["group_segment_fixed_size"] == 28768, (m, z)
        m, z = meta("og_k4_%s_%sz2" % (h, v)), meta("og_k4_%s_%sz" % (h, v))
        # six workgroups per CU: the VGPR granule of the `_z` twin, no scratch, no more LDS
        assert (m["vgpr_count"] + 7) // 8 <= (z["vgpr_count"] + 7) // 8, (m, z)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
        assert m["group_segment_fixed_size"] <= z["group_segment_fixed_size"], (m, z)


@pytest.mark.timeout(1500)
def test_the_bodies_on_the_host_simulator():
    """tests/test_stage_uniform_env_gpu.py on the host simulator (tests/hostsim): general kernels, the deeper variant with the
    bodies off and with them on give the same bus and state bytes at the pinned wide four-wave shape, 300 voices, 8 blocks,
    short envelopes -- and there the first case asserts, from the library's counters, that each operator stage ran both
    bodies (on a device the counters do not exist)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = build_hostsim.build()
    env.pop("OG_HOSTSIM_DEVICES", None)
    probe = ("import ctypes, oscen_amd; ctypes.c_ulonglong.in_dll(oscen_amd.load_library(), 'og_stage_uniform_chunks')")
    assert subprocess.run([sys.executable, "-c", probe], cwd=ROOT, env=env).returncode == 0  # (the counters are there to be read)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "1200", "-p", "no:cacheprovider", "tests/test_stage_uniform_env_gpu.py"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "9 passed" in r.stdout[-3000:] and "skipped" not in r.stdout[-3000:], r.stdout[-3000:]
