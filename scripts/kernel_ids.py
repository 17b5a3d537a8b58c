"""Kernel identity of the run-time compiled graphs of the CPU suite, for comparing two builds of the graph compiler:

    OSCEN_GPU_LIB=<library A> python scripts/kernel_ids.py a.txt
    OSCEN_GPU_LIB=<library B> python scripts/kernel_ids.py b.txt && cmp a.txt b.txt

Runs tests/test_codegen_fuzz_cpu.py, tests/test_dsl_corpus_cpu.py and tests/test_plugin_cpu.py in this process and writes,
for every graph whose kernel_source() they ask for, one line: the kernel name, then the SHA-256 of the general unit and of
its two zero variants.  Nothing is compiled for the device (jit_check is skipped): the generator's TEXT is what is compared.
profiles/r12_knob_retirement.md has the one use so far."""
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytest  # noqa: E402

import oscen_amd  # noqa: E402

lines = []
FEATURES = {"two-wave pipeline": "voice_block_p2(", "four-wave pipeline": "voice_block_p4(", "wide four-wave form": "og_k4w_",
            "delay rings": "ring_lds[", "oversampled region": "// oversampled inner loop", "node-to-node events": "OG_EV_LOOP_PRAGMA\n",
            "several lanes per voice": "#define OG_HPL", "no pipeline (too light or not splittable)": None}
reached = {k: set() for k in FEATURES}
plain_source = oscen_amd.Graph.kernel_source


def recorded_source(self):
    src = plain_source(self)
    digests = [hashlib.sha256(t.encode()).hexdigest() for t in (src, self.variant_source(1), self.variant_source(2))]
    lines.append(" ".join([re.search(r"\bog_k_[0-9a-f]{16}_00\b", src).group(0)] + digests))
    for k, mark in FEATURES.items():
        if (mark in src) if mark else ("voice_block_p2(" not in src):
            reached[k].add(digests[0])
    return src


if __name__ == "__main__":
    oscen_amd.Graph.kernel_source = recorded_source
    oscen_amd.Graph.jit_check = lambda self, arch="gfx950": 1 << 20  # (a code size no test takes for a failure)
    rc = pytest.main(["-q", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", f) for f in
                                                         ("test_codegen_fuzz_cpu.py", "test_dsl_corpus_cpu.py", "test_plugin_cpu.py")])
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d kernel_source() calls, %d distinct graphs, library %s" % (len(lines), len(set(lines)), oscen_amd.LIB_PATH))
    print("distinct units with: " + ", ".join("%s %d" % (k, len(v)) for k, v in reached.items()))
    sys.exit(int(rc))
