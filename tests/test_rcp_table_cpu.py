"""Static and host-simulator checks of the ADSR release reciprocal table (og_kernel_rt.hip.h, rcp_fetch): the wide four-wave
kernel's quiet release loops read the reciprocals from the table instead of computing them (no v_rcp_f32 left in them),
without spilling, register moves across the back edge or a change of the LDS footprint that keeps four workgroups per CU;
and the table path runs, bit for bit against the ordinary kernel, on the host simulator."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oscen_amd  # noqa: E402
from oscen_amd import build as b  # noqa: E402


def _loop_spans(asm, kern):
    """every loop of `kern` as laid out: (first, last, opcodes) from a label to a backward branch to it"""
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kern + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    ins, label_at = [], {}
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            label_at[m.group(1)] = len(ins)
        elif t and t[0] not in ";.":
            ins.append(t.split(";")[0].strip())
    spans = []
    for i, t in enumerate(ins):
        w = t.split()
        if (w[0].startswith("s_cbranch") or w[0] == "s_branch") and len(w) > 1 and w[1] in label_at and label_at[w[1]] <= i:
            spans.append((label_at[w[1]], i, [x.split()[0] for x in ins[label_at[w[1]]:i + 1]]))
    return spans


@pytest.mark.timeout(600)
def test_the_wide_kernels_quiet_release_loops_read_the_table(tmp_path):
    src = oscen_amd.Graph(builtin="fm_voice").kernel_source()
    kern = re.search(r"\b(og_k4w_[0-9a-f]{16}_00)\b", src).group(1)
    hip, asm = tmp_path / "fm.hip", tmp_path / "fm.s"
    hip.write_text(src)
    r = subprocess.run([b.hipcc(), "--offload-arch=" + b.ARCH, "-x", "hip", "-S", "--cuda-device-only", str(hip), "-o", str(asm)] + b.COMMON,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    text = asm.read_text()
    meta = dict(re.findall(r"\.(\w+):\s+(\S+)", re.search(r"\.group_segment_fixed_size:\s+\d+\n(?:(?!\n  - ).)*?\.name:\s+" + kern + r"\n(?:(?!\n  - ).)*", text, flags=re.S).group(0)))
    assert int(meta["vgpr_count"]) <= 128, meta["vgpr_count"]
    assert meta["private_segment_fixed_size"] == "0" and meta["vgpr_spill_count"] == "0", meta
    assert meta["group_segment_fixed_size"] == "36960", meta["group_segment_fixed_size"]  # four workgroups per CU
    # the table loops: the sticky release loops that load the next chunk's reciprocals (the innermost loops holding
    # 16-byte loads) -- one per wave that holds envelopes (fm_voice: three; the second holds two envelopes)
    spans = [s for s in _loop_spans(text, kern) if s[2].count("global_load_dwordx4") >= 4]
    tab = [l for a, e, l in spans if not any((o[0], o[1]) != (a, e) and a <= o[0] and o[1] <= e for o in spans)]
    assert sorted(l.count("global_load_dwordx4") for l in tab) == [4, 4, 8], [len(l) for l in tab]
    for l in tab:
        assert l.count("v_sin_f32_e32") == 16  # (a whole 16-frame chunk of the wave's operator in the loop)
        assert l.count("v_rcp_f32_e32") == 0
        assert not any(op.startswith("scratch_") for op in l)
        assert sum(1 for op in l if op in ("v_mov_b32_e32", "v_mov_b64_e32")) <= 2


@pytest.mark.timeout(1500)
def test_the_table_path_on_the_host_simulator():
    """tests/test_rcp_table_gpu.py on the host simulator (tests/hostsim: v_rcp_f32 is 1/x there, for the table as for the
    ordinary kernel, so the comparisons stay bit for bit)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hostsim"))
    try:
        import build_hostsim
    finally:
        sys.path.pop(0)
    env = dict(os.environ)
    env["OSCEN_GPU_LIB"] = build_hostsim.build()
    env.pop("OG_HOSTSIM_DEVICES", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "--timeout", "1200", "-p", "no:cacheprovider", "tests/test_rcp_table_gpu.py"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "4 passed" in r.stdout[-3000:], r.stdout[-3000:]
