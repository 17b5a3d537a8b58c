"""EventTimeline (csrc/og_timeline.h) against a naive model, on the CPU: tests/standalone/timeline_model_main.cpp drives the
class beside a per-voice list of every event pushed and a fake device ring, and checks after every launch that each voice was
delivered, and still holds, exactly the model's events in (frame, push order).  The header is host C++ without HIP: it is
compiled alone first.  The program also counts the paths of the incremental update it took; a run that missed one fails."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oscen_amd", "csrc")
PATHS = ["fast_path", "short_segment_merge", "merge_left_continuation", "pointed_at_continuation_in_place", "stale_cont_due_skipped",
         "ring_wrap", "refused_staging_full", "refused_ring_full", "late_local_dropped"]
SEEDS = [1, 2, 3, 4]


def test_timeline_header_compiles_without_hip():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "og_timeline.h")], check=True)


def test_timeline_matches_the_model_and_takes_every_path(tmp_path):
    exe = tmp_path / "timeline_model_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, os.path.join(ROOT, "tests", "standalone", "timeline_model_main.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)] + [str(s) for s in SEEDS], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    counts = {(int(s), name): int(n) for s, name, n in re.findall(r"^path seed (\d+) (\w+) (\d+)$", r.stdout, flags=re.M)}
    assert sorted(counts) == sorted((s, p) for s in SEEDS for p in PATHS)
    assert all(n > 0 for n in counts.values()), {k: n for k, n in counts.items() if n == 0}
    # blocks were queued and not launched at once: the consumed horizon lay behind the launch end
    assert all(int(n) > 0 for n in re.findall(r"horizon_behind (\d+)", r.stdout)) and r.stdout.count("horizon_behind") == len(SEEDS)
