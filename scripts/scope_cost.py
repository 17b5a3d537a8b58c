"""What an Oscilloscope in a voice costs: the voice kernel's time per 256-frame block with and without the node, from rocprofv3.

    python scripts/scope_cost.py [--voices 65536] [--rounds 3] [--out build/scope_cost]

Graphs: `osc = PolyBlepOscillator::saw` at a per-voice frequency (55 .. 1760 Hz over the bank) -> `scope = Oscilloscope::new(256)`
-> out, and its twin without the scope.  Three patterns: `short` (a steady tone, 200 .. 1760 Hz: every period is below the
capacity, windows are superseded before their deadline, nothing is copied), `steady` (a steady tone, 55 .. 1760 Hz: the 8 % of
the voices below 187.5 Hz have a period above the capacity and copy one window per period) and `gaps` (55 .. 1760 Hz, two
blocks of tone, two of amplitude 0, and so on: every voice copies its window once per gap).  One launch per block, 40 warm-up launches, 200 timed.  Every case is a run of its own under
`rocprofv3 --kernel-trace --stats` (this script starts itself as the worker behind `--`); the six cases are taken in turn,
`--rounds` times over, so that the spread between runs shows.  Writes <out>/scope_cost.json and prints a markdown table
(profiles/oscilloscope.md keeps it)."""
import argparse
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR, BLOCK, WARMUP, TIMED, CAPACITY = 48000.0, 256, 40, 200, 256
CASES = ("scope_short", "twin_short", "scope_steady", "twin_steady", "scope_gaps", "twin_gaps")


def graph(with_scope):
    import oscen_amd

    nodes = "osc = PolyBlepOscillator::saw(220.0, 0.3);" + (" scope = Oscilloscope::new(%d);" % CAPACITY if with_scope else "")
    wires = "osc.output -> scope.input; scope.output -> out;" if with_scope else "osc.output -> out;"
    return oscen_amd.Graph(dsl="name: scope_cost_%s;\ninput frequency: value = 220.0;\ninput amp: value = 0.3;\noutput out: stream;\nnodes { %s }\n"
                               "connections { frequency -> osc.frequency; amp -> osc.amplitude; %s }\n" % ("scope" if with_scope else "twin", nodes, wires),
                           per_voice=("frequency",))


def worker(case, voices):
    import numpy as np

    import oscen_amd

    with_scope, pattern = case.split("_")[0] == "scope", case.split("_")[1]
    eng = oscen_amd.Engine(graph(with_scope), voices, sample_rate=SR)
    eng.set_voice_values("frequency", np.linspace(200.0 if pattern == "short" else 55.0, 1760.0, voices).astype(np.float32))
    eng.set_bus_batching(1)
    for k in range(WARMUP + TIMED):
        if pattern == "gaps" and k % 2 == 0:
            eng.set_value("amp", 0.3 if k % 4 == 0 else 0.0)
        eng.process_block_async(BLOCK)
    eng.flush()
    eng.synchronize()
    copies = int(eng.read_state_field("scope.copies", dtype=np.uint32).astype(np.int64).sum()) if with_scope else 0
    print("worker %s: %d voices, %d launches, kernel %s, copies %d" % (case, voices, WARMUP + TIMED, eng.kernel_variant, copies))


def voice_kernel_ns(outdir):
    """durations of the voice kernel's launches in ns, in launch order, from the rocpd database(s) under outdir"""
    out = []
    for db in sorted(glob.glob(os.path.join(outdir, "**", "*results.db"), recursive=True)):
        con = sqlite3.connect(db)
        out += [(int(start), name, int(dur)) for name, start, dur in con.execute("select name, start, (end - start) from kernels")
                if re.search(r"^og_k\d?w?_[0-9a-f]{16}_", name)]
    out.sort()
    return [(n, d) for _, n, d in out]


def measure(case, voices, out, round_):
    d = os.path.join(out, "%s_%d" % (case, round_))
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "stats", "--", sys.executable, os.path.abspath(__file__), "--worker", case, "--voices", str(voices)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=170)
    open(os.path.join(d, "run.log"), "w").write(r.stdout)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 run '%s' failed (%d):\n%s" % (case, r.returncode, r.stdout[-2000:]))
    launches = voice_kernel_ns(d)
    if len(launches) != WARMUP + TIMED:
        raise SystemExit("run '%s': %d voice-kernel launches in the trace, expected %d" % (case, len(launches), WARMUP + TIMED))
    timed = sorted(t for _, t in launches[WARMUP:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("worker ")]
    return {"case": case, "round": round_, "kernel": launches[-1][0], "launches": len(timed), "mean_us": sum(timed) / len(timed) / 1e3, "min_us": timed[0] / 1e3,
            "median_us": timed[len(timed) // 2] / 1e3, "max_us": timed[-1] / 1e3, "worker": line[-1] if line else ""}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--voices", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "scope_cost"))
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.voices)
    rows = []
    for r in range(a.rounds):
        for case in CASES:
            rows.append(measure(case, a.voices, a.out, r))
            json.dump(rows, open(os.path.join(a.out, "scope_cost.json"), "w"), indent=1)
            print(json.dumps(rows[-1]), flush=True)
    print("\n| case | kernel | runs | mean us per block, per run | median us, per run | min .. max us over all launches |")
    print("|---|---|---|---|---|---|")
    mean = {}
    for case in CASES:
        rs = [x for x in rows if x["case"] == case]
        mean[case] = sum(x["mean_us"] for x in rs) / len(rs)
        print("| %s | `%s` | %d | %s | %s | %.1f .. %.1f |" % (case, rs[0]["kernel"], len(rs), ", ".join("%.1f" % x["mean_us"] for x in rs),
                                                            ", ".join("%.1f" % x["median_us"] for x in rs), min(x["min_us"] for x in rs), max(x["max_us"] for x in rs)))
    for p in ("short", "steady", "gaps"):
        print("%s: scope / twin = %.3f (+%.1f us per block of %d frames)" % (p, mean["scope_" + p] / mean["twin_" + p], mean["scope_" + p] - mean["twin_" + p], BLOCK))
    for x in rows:
        if x["round"] == 0:
            print(x["worker"])


if __name__ == "__main__":
    main()
