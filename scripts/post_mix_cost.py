"""What a post-mix graph costs: the time of its kernel (og_kp_*) beside the voice kernel's, from rocprofv3.

    python scripts/post_mix_cost.py [--voices 65536] [--blocks 192] [--out build/post_mix_cost]

The chain is the tests' one -- TptFilter -> [Delay, feedback 0.4] -> Gain behind the sum of `fm_voice` voices -- rendered in
256-frame blocks twice: one block per launch (og_set_bus_batching(1): the live setting) and under the automatic queue
(og_render).  Each case is a run of its own under `rocprofv3 --kernel-trace --stats` (this script starts itself as the
worker behind `--`), and the kernel times are read from the trace: per launch, per 256-frame block, against the 5.33 ms a
block lasts at 48 kHz.  Writes <out>/post_mix_cost.json and prints a markdown table (profiles/post_mix_graph.md keeps it).
"""
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
SR, BLOCK = 48000.0, 256


def chain_graph():
    import oscen_amd

    g = oscen_amd.Graph(builtin="fm_voice")
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.output_stream("wet")
    g.bus_node("master", "TptFilter::new", 1200.0, 0.707)
    g.bus_node("echo", "Delay::new", 37.0, 0.4)
    g.bus_node("trim", "Gain::new", 0.5)
    g.connect(out, "master.input")
    g.connect_via("master.output", "echo", "trim.input")
    g.connect("trim.output", "wet")
    return g


def worker(mode, voices, blocks):
    import oscen_amd

    eng = oscen_amd.Engine(chain_graph(), voices, sample_rate=SR)
    oscen_amd.schedule_note_plans(eng, oscen_amd.note_plans(voices, span=blocks * BLOCK), total_frames=blocks * BLOCK)
    if mode == "per_block":
        eng.set_bus_batching(1)
        for _ in range(blocks):
            eng.process_block_async(BLOCK)
        eng.flush()
        eng.synchronize()
    else:
        eng.render(blocks * BLOCK, block=BLOCK)
    print("worker %s: %d voices, %d blocks, post-mix %s" % (mode, voices, blocks, eng.post_mix_info()))


def kernel_times(outdir):
    """{kernel name: [durations in ns, in launch order]} from the rocpd database(s) rocprofv3 wrote under outdir"""
    times = {}
    for db in sorted(glob.glob(os.path.join(outdir, "**", "*results.db"), recursive=True)):
        con = sqlite3.connect(db)
        for name, dur in con.execute("select name, (end - start) from kernels order by start"):
            times.setdefault(name, []).append(int(dur))
    return times


def measure(mode, voices, blocks, out):
    d = os.path.join(out, mode)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "stats", "--", sys.executable, os.path.abspath(__file__), "--worker", mode,
           "--voices", str(voices), "--blocks", str(blocks)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=280)
    open(os.path.join(d, "run.log"), "w").write(r.stdout)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 run '%s' failed (%d):\n%s" % (mode, r.returncode, r.stdout[-2000:]))
    times = kernel_times(d)
    row = {"mode": mode, "voices": voices, "blocks": blocks}
    for key, pat in (("post_mix", r"^og_kp_[0-9a-f]{16}_"), ("voice", r"^og_k\d?w?_[0-9a-f]{16}_"), ("reduce", r"og_bus_reduce")):
        durs = [t for n, ts in times.items() if re.search(pat, n) for t in ts]
        names = sorted(n for n in times if re.search(pat, n))
        row[key] = {"kernels": names, "launches": len(durs), "total_us": sum(durs) / 1e3,
                    "per_launch_us": (sum(durs) / 1e3 / len(durs)) if durs else None, "per_block_us": sum(durs) / 1e3 / blocks}
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--voices", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=192)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "post_mix_cost"))
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.voices, a.blocks)
    rows = [measure(m, a.voices, a.blocks, a.out) for m in ("per_block", "auto_queue")]
    json.dump(rows, open(os.path.join(a.out, "post_mix_cost.json"), "w"), indent=1)
    deadline_us = BLOCK / SR * 1e6
    print("| launches | kernel | launches | us per launch | us per 256-frame block | of the %.0f us block |" % deadline_us)
    print("|---|---|---|---|---|---|")
    for row in rows:
        for key in ("post_mix", "voice", "reduce"):
            k = row[key]
            print("| %s | %s | %d | %s | %.2f | %.2f %% |" % (row["mode"], key, k["launches"], "%.2f" % k["per_launch_us"] if k["per_launch_us"] else "-",
                                                         k["per_block_us"], 100.0 * k["per_block_us"] / deadline_us))


if __name__ == "__main__":
    main()
