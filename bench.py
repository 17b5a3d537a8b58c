#!/usr/bin/env python
"""Benchmark of the hot path: voices*samples/sec of the fm-synth voice bank.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A step = one 256-frame block of the fm_voice graph over this rank's voice shard (BASELINE.json
configs[1]: 65 536 voices per GPU, 48 kHz, f32, synthetic note streams already resident in HBM;
`--voices-per-gpu 262144 --gpus 8` is configs[3], the 2 097 152-voice node).  With --gpus N > 1 and
no torch.distributed environment the script launches itself under torch.distributed.run (one rank
per GPU, RCCL); the driver's own `python -m torch.distributed.run ... bench.py --gpus N` works too.
Rank 0 prints ONE JSON line.

A plain run times ONE region of exactly K steps (barrier + synchronize on both sides) after the warm-up, which is at
least W blocks and ~40 ms of work, so that the GPU's clock governor has settled when the clock starts; `ms_per_step` =
the region / K.  --dump-outputs DIR writes the mix bus of the last timed step as DIR/bus.npy (float32, [frames, channels]);
the inputs are seeded, so the same arguments give the same bus on every run.

--full adds everything that is not the headline figure: the K-step region run --repeats times (default: ~40 ms of
timed work, 5..48 regions; `value` is then the MEDIAN region, every region's time is in the detail record), the other
BASELINE configurations (`configs`; N > 1: `config4` and the `og_cluster` leg), the REAL-TIME entry (`realtime`:
blocking og_midi_process_block, one launch per 256-frame block, live MIDI, p50 / p99 / max wall latency against the
5.333 ms deadline) and the CPU baseline (`cpu_baseline`).

`--gpus N --cluster` runs the same workload through the C-ABI cluster (og_cluster_*: ONE process, one engine per GPU,
one batched ncclReduce per launch batch) instead of one torch.distributed rank per GPU.

Other modes (not the headline): --midi-live (events arrive through og_midi_send + the blocking
og_process_block every block instead of a resident timeline), --graph <built-in> for the other
BASELINE configurations.
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import time

T_START = time.time()  # (wall-clock budget of the run: line["wall_s"])

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)


def pmc_profile(voices, block, graph, kernel_hash, blocks_per_launch=None, variant=None):
    """The committed rocprofv3 PMC summary (profiles/*_summary.json, scripts/prof_summary.py) of THIS kernel:
    same graph, bank size, block and kernel hash.  FETCH_SIZE / WRITE_SIZE / SQ_* come from separate --pmc
    runs, so they cannot be measured in-process; a summary of another kernel build is never mixed in --
    it is reported as stale instead."""
    match, stale = None, None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_summary.json"))):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        if d.get("voices") != voices or d.get("frames") != block or d.get("graph", "fm_voice") != graph or d.get("variant") != variant:
            continue
        if d.get("kernel_hash") == kernel_hash and "hbm_traffic" in d:
            # several summaries of this kernel: the one whose command queued the same number of blocks per launch
            def off(x):
                return abs(x.get("blocks_per_launch", 1.0) - (blocks_per_launch or x.get("blocks_per_launch", 1.0)))
            if match is None or off(d) <= off(match[1]):
                match = (path, d)
        else:
            stale = path
    if match:
        d = match[1]
        valu = d.get("pmc_voice_kernel", {}).get("SQ_INSTS_VALU", {}).get("avg_per_dispatch")
        # the shader clock the kernel actually ran at under the profiler: GRBM_GUI_ACTIVE counts busy cycles of all 8
        # XCDs per launch; / 8 / the launch duration of the same run
        grbm = d.get("pmc_voice_kernel", {}).get("GRBM_GUI_ACTIVE", {}).get("avg_per_dispatch")
        sclk = grbm / 8.0 / (d["timed_avg_us"] * 1e-6) / 1e9 if (grbm and d.get("timed_avg_us")) else None
        return {"bytes": d["hbm_traffic"]["total_bytes_corrected"], "valu": valu, "blocks_per_launch": d.get("blocks_per_launch", 1.0),
                "source": os.path.relpath(match[0], ROOT), "stale": None, "sclk_ghz": sclk}
    return {"bytes": None, "valu": None, "blocks_per_launch": None, "source": None, "sclk_ghz": None,
            "stale": os.path.relpath(stale, ROOT) if stale else None}


def cpu_baseline(block, seed, frames, span):
    """Time the CPU oracle (scalar C port of the reference path) on the host cores, bounded sample of the
    same note streams.  Two shapes of the same arithmetic: banks of 8 voices per graph, each rendered block
    by block (the reference's own `voices = [FMVoice; 8]`, examples/fm-synth/src/lib.rs:68-73, whose state
    stays in cache) -- the headline CPU figure -- and one big bank per thread walked voice-minor every sample
    (cache-hostile; what round 1 reported)."""
    import ctypes as C

    from tests import oracle_lib as ol

    lib = ol.load()
    lib.oo_bench_set_fold(ol.FOLD["slice"])
    cores = os.cpu_count() or 1
    cs = C.c_double()
    frames = int(max(block, min(frames, 48000)))

    def timed(voices, nframes, threads, group):
        t = lib.oo_bank_bench_grouped(ol.BANK_FM, voices, nframes, block, threads, group, seed, span, C.byref(cs))
        return voices * nframes / max(t, 1e-9)

    # How many threads does this box really run?  os.cpu_count() reports the host's CPUs, a container may be
    # throttled far below that (the round-1 figure of 1.6e5 voices*samples/s per thread against 2.6e6 on one
    # unconstrained core was this, not cache misses).  A short scaling probe picks the thread count with the best
    # aggregate rate; the single-thread rate is reported next to it.
    pf = min(frames, 1024)
    single = max(timed(64, pf, 1, 8), timed(64, pf, 1, 8))
    best_t, best_rate = 1, single
    t = 2
    cand = []
    while t < cores:
        cand.append(t)
        t *= 2
    cand.append(cores)
    probe = {"1": single}
    for t in cand:
        r = max(timed(64 * t, pf, t, 8), timed(64 * t, pf, t, 8))
        probe[str(t)] = r
        if r > best_rate:
            best_t, best_rate = t, r
    threads = best_t
    # A cgroup CPU quota below the CPU count (the MI355X boxes: 256 CPUs reported, cpu.max = 16 cores) makes the probe's
    # short bursts misleading: 64 threads burst to 3x what the quota sustains.  The sustained measurement runs with as
    # many threads as the quota grants -- the figure a reader should compare with -- and `cores` says so.
    quota = host_facts().get("cgroup_cpu_quota_cores")
    quota_threads = None
    if quota and quota < cores:
        quota_threads = max(1, int(round(quota)))
        threads = quota_threads
        if str(threads) not in probe:
            probe[str(threads)] = max(timed(64 * threads, pf, threads, 8), timed(64 * threads, pf, threads, 8))
        best_rate = probe[str(threads)]

    def run(group, budget_s, rate_guess):
        for _ in range(3):  # size the sample for ~budget_s seconds of wall time, re-sizing once or twice if the guess was off
            voices = int(max(8 * threads, min(1 << 21, rate_guess * budget_s / frames)))
            voices = max(8 * threads, (voices // (8 * threads)) * 8 * threads)
            rate = timed(voices, frames, threads, group)
            secs = voices * frames / rate
            if secs >= 0.4 * budget_s or voices >= (1 << 21):
                break
            rate_guess = rate
        return voices, secs, 0.0

    v8, t8, _ = run(8, 4.0, best_rate)  # (a throttled container sustains less than the probe burst: lands at 10-20 s)
    vw, tw, _ = run(0, 1.5, best_rate * 0.5)
    # the reference's own criterion shapes (oscen-lib/benches/static_vs_runtime.rs:68-116) + BASELINE config 1, one thread
    shapes = (C.c_double * 4)()
    lib.oo_criterion_shapes.argtypes = [C.c_double, C.POINTER(C.c_double)]
    lib.oo_criterion_shapes.restype = None
    lib.oo_criterion_shapes(0.3, shapes)
    return {
        "criterion_shapes": {
            "simple_graph/static_ns_per_process": shapes[0],
            "complex_graph/static_ns_per_process": shapes[1],
            "batch_processing/static_graph_512_ns": shapes[2],
            "config1_fm_voice_1voice_1s_block256_seconds": shapes[3],
            "config1_voices_samples_per_s": 48000.0 / shapes[3] if shapes[3] > 0 else None,
            "source": "C oracle (port) of StaticSimpleGraph / StaticComplexGraph process() at 44.1 kHz and of the FMVoice "
                      "graph (1 voice, 48 000 frames, note-on frame 0, note-off frame 24 000), single thread, ~0.3 s each",
        },
        "host": host_facts(),
        "scaling_probe": probe,
        "value": v8 * frames / t8,
        "unit": "voices*samples/s",
        "cores": threads,
        "cores_is": ("the cgroup CPU quota (%d of %d CPUs): the probe's best burst was at %d threads" % (threads, cores, best_t))
                    if quota_threads else "best of the scaling probe (no CPU quota below the CPU count)",
        "cpu_count": cores,
        "kind": "port",
        "per_thread": v8 * frames / t8 / threads,
        "single_thread": single,
        "sample": "%d voices x %d frames (block %d) of the same synthetic fm-synth note streams as banks of 8 voices "
                  "(the reference's [FMVoice; 8] graph) rendered block by block, C oracle, %d threads (%s; one thread alone: %.3g), "
                  "%.1f s" % (v8, frames, block, threads, "the cgroup CPU quota" if quota_threads else "best of a scaling probe over 1..%d" % cores, single, t8),
        "whole_bank_per_thread": {
            "value": vw * frames / tw,
            "per_thread": vw * frames / tw / threads,
            "sample": "%d voices x %d frames, one bank per thread walked voice-minor per sample (cache-hostile), "
                      "%d threads, %.1f s" % (vw, frames, threads, tw),
        },
    }


def host_facts():
    """What the box really gives this process: CPUs reported, CPUs in the affinity mask, the cgroup CPU quota and the
    CPU model -- so that `cores` and the per-thread rate of the CPU baseline can be read against evidence."""
    facts = {"os_cpu_count": os.cpu_count()}
    try:
        facts["sched_affinity_cpus"] = len(os.sched_getaffinity(0))
    except Exception:
        facts["sched_affinity_cpus"] = None
    quota = None
    try:  # cgroup v2: "max 100000" or "<quota> <period>"
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
        facts["cgroup_cpu_max"] = "%s %s" % (q, per)
    except Exception:
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = None if q <= 0 else q / float(per)
            facts["cgroup_cpu_max"] = "%d %d" % (q, per)
        except Exception:
            facts["cgroup_cpu_max"] = None
    facts["cgroup_cpu_quota_cores"] = quota
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                facts["cpu_model"] = ln.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    try:
        out = subprocess.run(["lscpu"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=5).stdout
        keep = {}
        for ln in out.splitlines():
            k, _, v = ln.partition(":")
            if k.strip() in ("Model name", "Socket(s)", "Core(s) per socket", "Thread(s) per core", "CPU(s)", "CPU max MHz"):
                keep[k.strip()] = v.strip()
        facts["lscpu"] = keep
    except Exception:
        facts["lscpu"] = None
    try:
        facts["loadavg"] = open("/proc/loadavg").read().split()[:3]
    except Exception:
        pass
    return facts


def realtime_record(graph, block, voices_list, n_blocks, midi_per_block, device, paced_blocks=0, loaded_voices=(), loaded_blocks=0,
                    loaded_paced=0):
    """The real-time entry, measured as a host would call it: one blocking og_midi_process_block per 256-frame block
    (the reference's audio callback: drain the MIDI queue, process_block, copy the bus out --
    examples/fm-synth/src/main.rs:148-215, 512-frame callback :273-277), one kernel launch per block, nothing
    queued ahead, `midi_per_block` live MIDI messages per block.  Wall latency per block against the deadline
    block / 48 kHz."""
    import numpy as np

    import oscen_amd

    deadline_ms = block / 48000.0 * 1e3
    out = []
    # The loops below time Python calls.  A generation-2 collection of this process's heap (torch is imported: ~10^6
    # tracked objects) takes 20-35 ms and lands on whichever block allocates the 700th object since the last one: seen
    # as one 24-34 ms "block" in every few thousand, at any bank size.  That is the harness, not the entry (a C or Rust
    # host has no collector; scripts/dbg_rt_hiccup.py, which does not import torch, shows none in 40 000 blocks), so the
    # collector is parked while the latencies are taken.
    import gc

    gc.collect()
    t0 = time.perf_counter()
    gc.collect()  # (a second full collection of the now clean heap: what one generation-2 pass costs this process)
    gc_ms = (time.perf_counter() - t0) * 1e3
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        rec = _realtime_record(graph, block, voices_list, n_blocks, midi_per_block, device, paced_blocks, deadline_ms, out,
                               loaded_voices, loaded_blocks, loaded_paced)
        rec["harness"] = {"python_gc": "disabled while latencies are taken", "full_collection_ms": gc_ms,
                          "tracked_objects": len(gc.get_objects())}
        return rec
    finally:
        if gc_was_on:
            gc.enable()


def _mem_budget_bytes():
    """Host memory this process may use for a resident score: a quarter of what the box / cgroup leaves."""
    avail = None
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                avail = int(ln.split()[1]) * 1024
                break
    except Exception:
        pass
    try:
        m = open("/sys/fs/cgroup/memory.max").read().strip()
        if m != "max":
            lim = int(m)
            try:
                lim -= int(open("/sys/fs/cgroup/memory.current").read().strip())
            except Exception:
                pass
            avail = lim if avail is None else min(avail, lim)
    except Exception:
        pass
    return (avail if avail is not None else 64 << 30) // 4


def _rt_bank(graph, V, block, n_blocks, paced_blocks, midi_per_block, device, deadline_ms, loaded, max_events):
    """One bank of the real-time record.  loaded = the synthetic score of SURVEY 8(d) (every voice plays its cyclic 1 s
    note plan: 3 gate events per voice per second) is resident in HBM for the whole run, ON TOP of the live MIDI."""
    import numpy as np

    import oscen_amd

    warm = 50
    note = None
    if loaded:
        # events the run needs: 3 per voice per 48 000 frames; a host-memory bound (~100 B per event while the timeline
        # is built) shortens the run instead of risking the box
        per_block = 3.0 * V * block / 48000.0
        fit = int(max_events / per_block) - warm
        if fit < n_blocks + paced_blocks:
            scale = fit / float(n_blocks + paced_blocks)
            n_blocks, paced_blocks = max(200, int(n_blocks * scale)), (max(100, int(paced_blocks * scale)) if paced_blocks else 0)
            note = "run shortened to %d + %d blocks: the resident score is bounded to %.0f M events by host memory" % (n_blocks, paced_blocks, max_events / 1e6)
    eng = oscen_amd.Engine(graph, V, device=device, sample_rate=48000.0)
    plans = oscen_amd.note_plans(V)
    n_resident = 0
    t_score = time.perf_counter()
    if loaded:
        total_frames = (warm + n_blocks + paced_blocks + 2) * block
        ev_v, ev_f0, ev_x = plans["events"]
        reps = -(-total_frames // 48000)
        plans["events"] = (np.tile(ev_v, reps), np.concatenate([ev_f0 + 48000 * k for k in range(reps)]), np.tile(ev_x, reps))
        # a live message re-writes its voice's remaining score as a fresh segment behind the score (og_reserve_events):
        # midi_per_block voices per block, half the run's events per voice on average, twice over for margin
        per_voice = 3.0 * total_frames / 48000.0
        eng.reserve_events(int(midi_per_block * (warm + n_blocks + paced_blocks) * per_voice) + (1 << 20))
        n_resident = oscen_amd.schedule_note_plans(eng, plans, total_frames=total_frames)
        if os.environ.get("OSCEN_BENCH_GROUP_VOICES"):  # (--group-voices reaches the real-time child through the environment)
            eng.group_voices(int(os.environ["OSCEN_BENCH_GROUP_VOICES"]))
        plans["events"] = None
    else:
        eng.set_voice_values("frequency", plans["frequency"])
    midi = oscen_amd.Midi(eng)
    midi.set_queue_capacity(max(32, midi_per_block))
    rng = np.random.default_rng(0x05CE2026)
    n_pat = 64  # message patterns built once: the loop pays for the engine's live path, not for numpy
    notes = rng.integers(36, 97, size=(n_pat, midi_per_block)).astype(np.uint8)
    frames = np.sort(rng.integers(0, block, size=(n_pat, midi_per_block)), axis=1).astype(np.uint32)
    packed = [midi.pack_messages(notes[i - (i % 2)], frames[i], on=(i % 2 == 0)) for i in range(n_pat)]
    lat = np.empty(n_blocks, dtype=np.float64)
    peak = 0.0
    first_ms = None
    for i in range(warm + n_blocks):
        t0 = time.perf_counter()
        if midi_per_block:
            midi.send_packed(packed[i % n_pat])
        bus = midi.process_block(block)
        t1 = time.perf_counter()
        if i == 0:
            first_ms = (t1 - t0) * 1e3  # (a resident score goes to the device with the first block: warm-up, not timed)
            t_score = t1 - t_score
        if i >= warm:
            lat[i - warm] = t1 - t0
            peak = max(peak, float(np.abs(bus).max()))
    calls, timeouts = eng.blocking_stats
    lat_ms = lat * 1e3
    worst = np.argsort(lat_ms)[-5:][::-1]
    rec = {
        "voices": V,
        "blocks": n_blocks,
        "midi_messages_per_block": midi_per_block,
        "resident_score_events": n_resident,
        "latency_ms": {"p50": float(np.percentile(lat_ms, 50)), "p99": float(np.percentile(lat_ms, 99)),
                       "p999": float(np.percentile(lat_ms, 99.9)), "max": float(lat_ms.max()), "mean": float(lat_ms.mean())},
        "deadline_ms": deadline_ms,
        "deadline_misses": int(np.count_nonzero(lat_ms > deadline_ms)),
        "value_blocking": V * block / float(lat.mean()),
        "marker_timeouts": timeouts,
        "worst_blocks": [[int(i), float(lat_ms[i])] for i in worst],
        "event_stats": eng.event_stats,
        "bus_peak": peak,
        "kernel_variant": eng.kernel_variant,
        "first_block_ms": first_ms,
        "setup_s": t_score,
    }
    if note:
        rec["note"] = note
    if paced_blocks:
        # the same entry called when a sound card would call it: once per block PERIOD (the loop above calls back
        # to back, i.e. holds the GPU at full load; here it idles between blocks and the clocks follow)
        plat = np.empty(paced_blocks, dtype=np.float64)
        t_next = time.perf_counter()
        for i in range(paced_blocks):
            t_next += deadline_ms * 1e-3
            while time.perf_counter() < t_next:
                pass
            t0 = time.perf_counter()
            if midi_per_block:
                midi.send_packed(packed[i % n_pat])
            midi.process_block(block)
            plat[i] = time.perf_counter() - t0
        plat *= 1e3
        rec["paced"] = {"blocks": paced_blocks, "period_ms": deadline_ms,
                        "latency_ms": {"p50": float(np.percentile(plat, 50)), "p99": float(np.percentile(plat, 99)),
                                       "p999": float(np.percentile(plat, 99.9)), "max": float(plat.max()), "mean": float(plat.mean())},
                        "deadline_misses": int(np.count_nonzero(plat > deadline_ms))}
    del midi
    eng.close()
    return rec


def _rt_ok(r):
    return r["deadline_misses"] == 0 and r.get("paced", {}).get("deadline_misses", 0) == 0 and r["bus_peak"] > 0.0


def _realtime_record(graph, block, voices_list, n_blocks, midi_per_block, device, paced_blocks, deadline_ms, out,
                     loaded_voices=(), loaded_blocks=0, loaded_paced=0):
    import numpy as np

    import oscen_amd

    for V in voices_list:  # the idle bank: live MIDI only (at most a few 10^4 of the voices sound)
        out.append(_rt_bank(graph, V, block, n_blocks, paced_blocks if V == max(voices_list) else 0, midi_per_block, device,
                            deadline_ms, False, 0))
    # the LOADED bank: every voice plays the synthetic score the throughput lines use, plus the live messages
    loaded = []
    # (64 M events = 1 GB on the device, ~6 GB of host memory while the timeline is built, ~5 s of set-up per bank: the
    #  default `python bench.py --full` has to finish within minutes)
    max_events = min(64e6, _mem_budget_bytes() / 100.0)
    for V in loaded_voices:
        loaded.append(_rt_bank(graph, V, block, loaded_blocks, 0, midi_per_block, device, deadline_ms, True, max_events))
    paced_rec = None
    ok_loaded = [r for r in loaded if _rt_ok(r)]
    if ok_loaded and loaded_paced:  # the largest bank that met every deadline back to back, now called once per block period
        Vp = max(r["voices"] for r in ok_loaded)
        pr = _rt_bank(graph, Vp, block, 200, loaded_paced, midi_per_block, device, deadline_ms, True, max_events)
        paced_rec = {"voices": Vp, "note": pr.get("note"), "resident_score_events": pr["resident_score_events"], **pr["paced"]}
        for r in loaded:
            if r["voices"] == Vp:
                r["paced"] = pr["paced"]
    # the multi-GPU real-time entry (og_midi_process_block over og_cluster_process_block): what can be measured on one
    # GPU is its HOST side -- one thread per shard, cross-stream events, the per-device accumulation, the pinned
    # hand-over -- with both shards on this device (no RCCL leg: a communicator needs distinct devices)
    cluster_rec = None
    try:
        V = 131072
        cl = oscen_amd.Cluster(graph, V, [device, device], sample_rate=48000.0)
        cl.set_voice_values("frequency", oscen_amd.note_plans(V)["frequency"])
        midi = oscen_amd.Midi(cl)
        midi.set_queue_capacity(max(32, midi_per_block))
        rng = np.random.default_rng(0x05CE2026)
        notes = rng.integers(36, 97, size=(64, midi_per_block)).astype(np.uint8)
        frames = np.sort(rng.integers(0, block, size=(64, midi_per_block)), axis=1).astype(np.uint32)
        packed = [midi.pack_messages(notes[i - (i % 2)], frames[i], on=(i % 2 == 0)) for i in range(64)]
        nb = max(200, n_blocks // 4)
        lat = np.empty(nb, dtype=np.float64)
        for i in range(50 + nb):
            t0 = time.perf_counter()
            if midi_per_block:
                midi.send_packed(packed[i % 64])
            bus = midi.process_block(block)
            if i >= 50:
                lat[i - 50] = time.perf_counter() - t0
        lat_ms = lat * 1e3
        cluster_rec = {
            "entry": "og_midi_create_cluster + og_midi_process_block (og_cluster_process_block), 2 shards on ONE device: host-side "
                     "cost of the cluster entry only, no RCCL leg",
            "voices": V, "shards": 2, "blocks": nb, "midi_messages_per_block": midi_per_block,
            "latency_ms": {"p50": float(np.percentile(lat_ms, 50)), "p99": float(np.percentile(lat_ms, 99)), "max": float(lat_ms.max()),
                           "mean": float(lat_ms.mean())},
            "deadline_ms": deadline_ms, "deadline_misses": int(np.count_nonzero(lat_ms > deadline_ms)),
            "bus_peak": float(np.abs(bus).max()),
        }
        del midi
        cl.close()
    except Exception as e:  # (never fail the bench line over the side record)
        cluster_rec = {"error": str(e)[:200]}
    ok = [r for r in out if _rt_ok(r)]
    ok_loaded = [r for r in loaded if _rt_ok(r)]
    best = max(ok_loaded, key=lambda r: r["voices"]) if ok_loaded else None
    return {
        "cluster_entry_host_side": cluster_rec,
        "entry": "og_midi_send_batch + og_midi_process_block (blocking: bus in host memory when the call returns), "
                 "one launch per block, default batching",
        "block": block,
        # every voice playing the resident synthetic score (3 gate events per voice per second) + the live messages
        "loaded": {"runs": loaded, "paced": paced_rec,
                   "score": "oscen_amd.note_plans: the 1 s plan of every voice, cyclic, resident in HBM (schedule_note_plans)"},
        # live MIDI only: at most a few 10^4 voices sound, the rest take the cheapest chunk variant
        "idle_bank": {"runs": out,
                      "realtime_voices_at_48k": max([r["voices"] for r in ok]) if ok else 0},
        # the largest LOADED bank measured here whose EVERY block met the deadline (not an extrapolation)
        "realtime_voices_at_48k": best["voices"] if best else 0,
        "realtime_voices_at_48k_is": "loaded bank (resident score on every voice + live MIDI), back to back and paced",
        # p99-latency-scaled estimate from that bank (how many voices would still fit the deadline if the block time
        # scaled linearly): an upper bound, not a measurement
        "realtime_voices_at_48k_extrapolated": (best["voices"] * deadline_ms / best["latency_ms"]["p99"]) if best else 0,
    }


def self_launch(args):
    """`python bench.py --gpus N` without a torch.distributed environment: one rank per GPU over RCCL."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def roofline_record(eng, V, block, graph, kern_ms, n_launch, n_blocks_timed, variant=None):
    """The HBM roofline object of the contract for the voice kernel of `eng` (one shard of V voices)."""
    words = eng.state_words_per_voice
    lanes = eng.voices_per_wave * eng.lanes_per_voice
    n_wg = eng.partial_rows
    # SURVEY 8(d)'s per-unit figure (state read + written once per 256-frame block, event cursors, one partial row per
    # workgroup) x the units one launch processes: a launch that renders several queued blocks is charged that many
    # blocks' worth, although it touches the state planes only once -- so `achieved` is an ACCOUNTING rate, not a DRAM
    # bandwidth; `dram_gbs` (PMC bytes / kernel time) is the bandwidth
    bytes_per_block = V * (4 * (words + eng.state_words_written_per_voice) + 8) + n_wg * block * 4
    # graphs with a Delay: every voice-sample reads one and writes one 4-byte slot of its HBM ring
    bytes_per_block += V * block * 8 * {"echo_voice": 1}.get(graph, 0)
    blocks_per_launch = n_blocks_timed / float(max(1, n_launch))
    bytes_per_launch = bytes_per_block * blocks_per_launch
    achieved = bytes_per_launch / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0
    prof = pmc_profile(V, block, graph, eng.kernel_hash, blocks_per_launch, variant)
    pmc_bytes, pmc_valu, pmc_src = prof["bytes"], prof["valu"], prof["source"]
    pmc_note = None
    if pmc_src and abs(prof["blocks_per_launch"] - blocks_per_launch) > 0.02 * blocks_per_launch:
        # the profiled command queued a different number of blocks per launch: instruction counts scale with the frames
        # rendered; HBM traffic does not (the state planes are touched once per launch) and is not extrapolated
        pmc_note = ("profile has %.2f blocks per launch, this run %.2f: VALU count scaled by the ratio, traffic omitted"
                    % (prof["blocks_per_launch"], blocks_per_launch))
        pmc_valu = pmc_valu * blocks_per_launch / prof["blocks_per_launch"] if pmc_valu else None
        pmc_bytes = None
    traffic = pmc_bytes / (kern_ms * 1e-3) / 1e9 if (pmc_bytes and kern_ms > 0) else None
    return {
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "achieved_is": "charged bytes (SURVEY 8d per-block accounting x blocks per launch) / kernel time -- an accounting "
                       "rate; the DRAM bandwidth is dram_gbs",
        "charged_gbs": achieved,
        "traffic": traffic,
        "dram_gbs": traffic,
        "dram_frac": traffic / HBM_PEAK_GBS if traffic else None,
        "traffic_bytes_per_launch": pmc_bytes,
        "traffic_source": pmc_src,
        "stale_profile": prof["stale"],  # newest summary of this configuration taken on ANOTHER kernel build
        "profile_note": pmc_note,
        "kernel_hash": eng.kernel_hash,
        "kernel_variant": eng.kernel_variant,
        "kernel_ms_avg": kern_ms,
        "kernel_launches": n_launch,
        "blocks_per_launch": blocks_per_launch,
        "kernel_ms_per_block": kern_ms / blocks_per_launch if blocks_per_launch else None,
        "algorithmic_bytes_per_launch": bytes_per_launch,
        "voices_per_wave": lanes,
        "pipeline_waves_per_64_voices": eng.pipeline_depth,
        "bytes_per_voice_sample": bytes_per_block / float(V * block),
        "note": "path is VALU/transcendental-bound (SURVEY F8): HBM is touched once per launch; "
                "see valu_issue for the bound that applies",
        # The limiter: instruction issue / dependent-instruction latency.  peak = the nominal rate
        # MI355X_MICROARCH.md gives (a wave64 VALU instruction every 2 cycles per SIMD: 1024 SIMDs x 2.4 GHz / 2 = the
        # 157 TF vector peak); measured_ceiling = the plain-FMA stream ceiling cdna_hip_programming.md quotes (103 TF
        # of v_fma_f32 = 3.05 cycles per instruction; scripts/pk_probe reaches 3.2 with eight waves per SIMD).
        # achieved = SQ_INSTS_VALU per launch (committed PMC pass of the SAME kernel hash) / the kernel duration
        # measured in this run.
        "valu_issue": None if not (pmc_valu and kern_ms > 0) else {
            "achieved": pmc_valu / (kern_ms * 1e-3) / 1e9,
            "peak": 1024 * 2.4 / 2.0,
            "measured_ceiling": 1024 * 2.4 / 3.05,
            "unit": "G wave-instructions/s",
            "frac": pmc_valu / (kern_ms * 1e-3) / 1e9 / (1024 * 2.4 / 2.0),
            "frac_of_measured_ceiling": pmc_valu / (kern_ms * 1e-3) / 1e9 / (1024 * 2.4 / 3.05),
            "valu_wave_inst_per_64_voices_per_frame": pmc_valu / (V / 64.0 * block * blocks_per_launch),
            # cycles one SIMD spends per VALU wave-instruction of this launch, at the clock the profile saw (the part
            # runs at ~2.1 GHz under this load, not at the 2.4 GHz the peaks above are quoted for): 2.0 would be the
            # nominal issue rate, 3.05 the FMA-stream ceiling
            "sclk_ghz_profiled": prof.get("sclk_ghz"),
            "cycles_per_valu_inst_per_simd": (kern_ms * 1e-3 * prof["sclk_ghz"] * 1e9) / (pmc_valu / 1024.0) if prof.get("sclk_ghz") else None,
            "source": pmc_src,
        },
    }


# The other BASELINE.json configurations on one GPU (graph, bank size, frames rendered), measured by the
# same timed_bank() as the headline after it, so that the driver's one command records every configuration.
OTHER_CONFIGS = [
    # (name, graph, voices, blocks per timed region, variant)
    ("2-variant: fm-synth 65 536 voices, feedback .3/.2, route .5, env amount 2000, cutoff ramp", "fm_voice", 65536, 188, "survey2"),
    ("4-shard: fm-synth 262 144 voices (config 4's per-GPU shard)", "fm_voice", 262144, 188, None),
    ("3a: electric-piano 262 144 voices -> Tremolo, stereo", "epiano_voice", 262144, 94, None),
    ("3b: osc+env+TptFilter 262 144 voices", "sub_voice", 262144, 94, None),
    ("5: SatGraph_4x 131 072 voices (multirate)", "sat4x_voice", 131072, 94, None),
]


def config_records(args, local_rank):
    """One compact record per entry of OTHER_CONFIGS (N = 1 only): value, ms per step, the kernel and its roofline figures."""
    import copy

    import numpy as np
    import torch

    out = []
    a = copy.copy(args)
    a.midi_live, a.midi_blocking, a.sparse_events, a.bus_batch = 0, False, False, 0
    W, R = 8, 3
    for name, graph, V, K, variant in OTHER_CONFIGS:
        if args.test_scale > 1:
            V, K, W, R = max(64, V // args.test_scale), (24 if variant else 4), 2, 2
        try:
            m = timed_bank(a, graph, V, K, W, R, 0, local_rank, 1, None, variant)
            mix = m.bus[torch.from_numpy(m.timed_blocks).to(m.bus.device)].float().cpu().numpy()
            assert np.isfinite(mix).all() and np.abs(mix).max() > 0.0, "bus is silent or non-finite"
            elapsed, _ = region_stats(m.times, V, K, m.block)
            rf = roofline_record(m.eng, V, m.block, graph, m.kern_ms, m.n_launch, m.n_blocks_timed, variant)
            vi = rf.get("valu_issue") or {}
            out.append({
                "config": name, "graph": graph, "voices": V, "steps": K, "repeats": R, "variant": variant,
                "value": V * K * m.block / elapsed, "ms_per_step": elapsed / K * 1e3,
                "kernel": rf["kernel_variant"], "kernel_hash": rf["kernel_hash"], "kernel_ms_per_block": rf["kernel_ms_per_block"],
                "blocks_per_launch": rf["blocks_per_launch"], "bytes_per_voice_sample": rf["bytes_per_voice_sample"],
                "roofline_frac": rf["frac"], "valu_issue_frac": vi.get("frac"),
                "valu_per_64_voices_per_frame": vi.get("valu_wave_inst_per_64_voices_per_frame"),
                "dram_gbs": rf["dram_gbs"], "profile": rf["traffic_source"], "stale_profile": rf["stale_profile"],
                "events_in_timed_region": m.n_events_timed // R,
            })
            m.eng.close()
            del m
            torch.cuda.empty_cache()
        except Exception as e:  # (a side record never costs the headline line)
            out.append({"config": name, "graph": graph, "voices": V, "error": str(e)[:200]})
    return out


SURVEY2 = {"op3_feedback": 0.3, "op2_feedback": 0.2, "route": 0.5, "filter_env_amount": 2000.0}


def timed_bank(args, graph, V, K, W, R, rank, local_rank, world_size, dist, variant=None):
    """The measurement proper: this rank's shard of a bank of V voices per GPU, W warm-up blocks, then R timed regions of K
    blocks each (barrier + synchronize on both sides).  Used for the headline line and, at N = 1, once more for every other
    BASELINE configuration (`configs`)."""
    import types

    import numpy as np
    import torch

    import oscen_amd
    from oscen_amd import distributed as ogd

    rccl_ranks = None
    total_voices = V * world_size
    lo, hi = ogd.shard_range(rank, world_size, total_voices)
    block = args.block
    # block sequence: W warm-up blocks (the last one runs after the barrier, see below), then R regions of K timed
    # blocks, regions 1.. each preceded by ONE untimed block that plays the same role as that last warm-up block
    n_blocks = W + R * K + (R - 1)
    total_frames = n_blocks * block
    # the score: regions of a second or more play the 1 s plan of SURVEY 8(d) as it is (note-ons in block 0 of every second);
    # shorter regions see every voice's CYCLIC plan from a per-voice offset (fold="slice"), i.e. the plan's real event
    # density -- 3 events per voice per 48 000 frames, all three kinds -- in every region, however many regions there are
    short_regions = K * block < 48000
    span = 0 if args.sparse_events else (total_frames if short_regions else min(total_frames, 48000))

    eng = oscen_amd.Engine(graph, hi - lo, device=local_rank, sample_rate=48000.0)
    # global voice ids keep their note streams; a run shorter than the 1 s score sees a slice of it at its real density
    plans = oscen_amd.note_plans(hi - lo, first_voice=lo, span=span, fold="cyclic" if short_regions else "slice")
    midi = None
    ramp_blocks = {}
    if variant == "survey2":
        # SURVEY 8(d), config 2's VARIANT: operator feedback, the modulation routed both ways, an envelope-modulated cutoff
        # (a per-sample tan: filters/tpt/mod.rs:85-101 is the branch the defaults never take) and the ramped filter_cutoff
        # 2 000 -> 6 000 over 2 205 frames at frame 4 800 of each timed second (block 19 of a region; the next region
        # ramps back, the same work)
        for name, val in SURVEY2.items():
            eng.set_value_immediate(name, val)
        for r in range(R):
            if K > 19:
                ramp_blocks[W + r * (K + 1) + 19] = 6000.0 if r % 2 == 0 else 2000.0
    timed_blocks = np.zeros(n_blocks, dtype=bool)
    for r in range(R):
        b0 = W + r * (K + 1)
        timed_blocks[b0:b0 + K] = True
    if args.midi_live:
        eng.set_voice_values("frequency", plans["frequency"])
        midi = oscen_amd.Midi(eng)
        midi.set_queue_capacity(max(32, args.midi_live))
        n_events_timed = args.midi_live * K * R
    else:
        if total_frames > 48000 and not (short_regions and span):  # a run longer than the 1 s score plays it again and again
            ev_v, ev_f0, ev_x = plans["events"]
            reps = -(-total_frames // 48000)
            plans["events"] = (np.tile(ev_v, reps), np.concatenate([ev_f0 + 48000 * k for k in range(reps)]), np.tile(ev_x, reps))
        oscen_amd.schedule_note_plans(eng, plans, total_frames=total_frames)
        if args.group_voices:  # (og_group_voices: voices whose notes end together share waves)
            eng.group_voices(args.group_voices)
        ev_f = plans["events"][1]
        if "gate" in eng.input_names:
            inside = ev_f < total_frames
            n_events_timed = int(np.count_nonzero(timed_blocks[(ev_f[inside] // block).astype(np.int64)]))
        else:
            n_events_timed = 0
    stream = torch.cuda.current_stream()
    eng.set_stream(stream.cuda_stream)
    if args.bus_batch != 1:  # queued blocks share a launch; every bus is complete before the timed region closes (flush below)
        eng.set_bus_batching(args.bus_batch)
    ch = eng.channels
    bus = torch.zeros((n_blocks, block * ch), dtype=torch.float32, device="cuda")
    base = bus.data_ptr()
    host_bus = np.zeros((n_blocks, block * ch), dtype=np.float32)
    rng = np.random.default_rng(0x05CE2026 + rank)
    live = []
    if midi is not None:  # messages built once: the timed loop pays for the engine's live path, not for numpy
        live_notes = rng.integers(36, 97, size=(n_blocks, args.midi_live)).astype(np.uint8)
        live_frames = np.sort(rng.integers(0, block, size=(n_blocks, args.midi_live)), axis=1).astype(np.uint32)
        for i in range(n_blocks):  # even blocks play notes, odd blocks release the notes of the block before
            live.append(midi.pack_messages(live_notes[i - (i % 2)], live_frames[i], on=(i % 2 == 0)))

    def step(i):
        if i in ramp_blocks:
            eng.set_value("filter_cutoff", ramp_blocks[i])  # `[ramp: 2205]` (fm_voice.rs); launches what is queued first
        if midi is None:
            eng.process_block_async(block, base + i * block * ch * 4)
        else:
            midi.send_packed(live[i])
            if args.midi_blocking:
                host_bus[i] = midi.process_block(block).reshape(-1)
            else:
                midi.process_block_async(block, base + i * block * ch * 4)

    def steps(a, b):
        """blocks a .. b-1.  Where nothing happens between blocks (no MIDI, no value change) they cross the boundary in ONE
        call, og_process_blocks_async: same queue, same launches, same buses bit for bit -- what is left out is Python's
        ~2 us per ctypes call, 40 us of a 600 us region at the driver's 20 steps, which a compiled host does not pay
        (--per-block-calls keeps one call per block)."""
        if midi is not None or args.per_block_calls:
            for i in range(a, b):
                step(i)
            return
        i = a
        while i < b:
            if i in ramp_blocks:
                eng.set_value("filter_cutoff", ramp_blocks[i])
            j = i + 1
            while j < b and j not in ramp_blocks:
                j += 1
            eng.process_blocks_async(block, j - i, base + i * block * ch * 4, block * ch * 4)
            i = j

    def reduce_bus(t):
        if args.backend == "gloo":  # CPU collective (plumbing check only)
            h = t.cpu()
            ogd.reduce_bus(h, engine=eng)
            t.copy_(h)
        else:
            ogd.reduce_bus(t, engine=eng)

    def barrier():
        if args.backend == "gloo":
            dist.barrier()
        else:
            dist.barrier(device_ids=[local_rank])

    # Warm-up: W - 1 blocks, the communicator set-up, the barrier -- and then the LAST warm-up block, so that the voice
    # kernel is the most recent thing every CU ran when the clock starts.  Measured on MI355X: the first launch of the
    # voice kernel after OTHER kernels (RCCL's, or any torch kernel) is ~35 % slower than in a steady stream of blocks
    # (same instruction count, +57 % instruction-fetch wait: its code has to come back from HBM), and with one launch per
    # 20-32 blocks that launch is the whole timed region -- a measurement artefact of the barrier, not of the path.
    steps(0, max(0, W - 1))
    eng.flush()
    if dist is not None:  # communicator set-up (lazy in RCCL) must not land in the timed region
        reduce_bus(bus[:max(1, W - 1)] if W > 1 else torch.zeros((1, block * ch), dtype=torch.float32, device="cuda"))
        ones = torch.ones(1, dtype=torch.float32, device="cpu" if args.backend == "gloo" else "cuda")
        dist.all_reduce(ones)  # every rank of the communicator took part
        rccl_ranks = int(round(float(ones.item())))
    times, sclk, kclk = [], [], []
    reduce_events, reduce_host_ms = [], []
    kern_total_ms, n_launch, n_blocks_timed = 0.0, 0, 0
    for r in range(R):
        first = W + r * (K + 1)        # first timed block of this region
        torch.cuda.synchronize()
        if dist is not None:
            barrier()
        torch.cuda.synchronize()
        if first > 0 and (r > 0 or W > 0):  # the untimed block right in front of the region
            step(first - 1)
            eng.flush()
            torch.cuda.synchronize()
        eng.enable_kernel_timing(True)  # (per region: the untimed block in front of it is not part of the launch average)
        t0 = time.perf_counter()
        steps(first, first + K)
        eng.flush()  # the reduces of the last (partial) batch of blocks: inside the timed region
        if dist is not None:
            # ONE RCCL reduce of the [K, block] mix bus over xGMI, bracketed by events on the stream it runs on (the
            # engine renders on torch's current stream), so that a scaling record explains its own efficiency
            t_r0 = time.perf_counter()
            ev_r0, ev_r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev_r0.record(stream)
            reduce_bus(bus[first:first + K])
            ev_r1.record(stream)
            reduce_host_ms.append((time.perf_counter() - t_r0) * 1e3)
            reduce_events.append((ev_r0, ev_r1))
        torch.cuda.synchronize()
        if dist is not None:
            barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        elapsed = t1 - t0
        if dist is not None:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if args.backend == "gloo" else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        times.append(elapsed)
        sclk.append(eng.shader_clock_ghz())        # (after the clock has stopped: a 20 us probe of the shader clock as the region left it)
        ms, n = eng.kernel_time_ms()               # average duration of a voice-kernel LAUNCH (HIP events on the engine's stream)
        kclk.append(eng.kernel_clock_ghz or None)  # ... and the shader clock those launches ran at, read by the kernel itself
        kern_total_ms += ms * n
        n_launch += n
        n_blocks_timed += eng.kernel_blocks_timed  # blocks those launches rendered (up to --bus-batch per launch)
        eng.enable_kernel_timing(False)
    kern_ms = kern_total_ms / max(1, n_launch)
    multi_gpu = None
    if dist is not None:
        # per rank: the voice kernel's average launch and per-block time, and what the reduce cost on this rank's stream
        # (device time between the two events: includes waiting for the slowest rank -- a reduce cannot finish before
        # every contribution exists) and on its host thread
        red_dev = [a.elapsed_time(b) for a, b in reduce_events] if args.backend != "gloo" else list(reduce_host_ms)
        mine = torch.tensor([kern_ms, kern_ms * n_launch / max(1, n_blocks_timed), float(np.median(red_dev)) if red_dev else 0.0,
                             float(np.median(reduce_host_ms)) if reduce_host_ms else 0.0], dtype=torch.float64,
                            device="cpu" if args.backend == "gloo" else "cuda")
        allr = [torch.zeros_like(mine) for _ in range(world_size)]
        dist.all_gather(allr, mine)
        rows = [[float(x) for x in t.cpu().tolist()] for t in allr]
        multi_gpu = {
            "rccl_ranks": rccl_ranks,
            "backend": "RCCL" if args.backend == "nccl" else "gloo",
            "per_rank_kernel_ms_avg": [r[0] for r in rows],
            "per_rank_kernel_ms_per_block": [r[1] for r in rows],
            "per_rank_reduce_ms": [r[2] for r in rows],
            "per_rank_reduce_host_ms": [r[3] for r in rows],
            "reduce_ms_max": max(r[2] for r in rows),
            "reduce_bytes": int(K * block * ch * 4),
            "reduce_share_of_region": max(r[2] for r in rows) / (float(np.median(times)) * 1e3) if times else None,
            "note": "reduce = one [K x block x channels] f32 sum onto rank 0 per timed region; device time between events "
                    "recorded around it on the rendering stream (median over the regions)",
        }

    return types.SimpleNamespace(eng=eng, times=times, sclk=sclk, kclk=kclk, kern_ms=kern_ms, n_launch=n_launch, n_blocks_timed=n_blocks_timed, multi_gpu=multi_gpu,
                                 rccl_ranks=rccl_ranks, timed_blocks=timed_blocks, bus=bus, host_bus=host_bus, midi=midi,
                                 n_events_timed=n_events_timed, span=span, total_voices=total_voices, block=block, ch=ch)


def region_stats(times, total_voices, K, block):
    import numpy as np

    t = np.asarray(times, dtype=np.float64)
    med = float(np.median(t))
    return med, {
        "repeats": len(times),
        "regions_ms": [x * 1e3 for x in times],
        "value_median": total_voices * K * block / med,
        "value_min": total_voices * K * block / float(t.max()),
        "value_max": total_voices * K * block / float(t.min()),
        "value_first_region": total_voices * K * block / float(t[0]),
        # what five regions alone would have reported (rounds 1-4): the governor's cold figure
        "value_median_first5": total_voices * K * block / float(np.median(t[:5])),
    }


def cluster_record(args, N, V, K, W, R, graph=None, dump_dir=None):
    """The workload through the C-ABI cluster (og_cluster_create over devices 0..N-1, og_cluster_render of the K blocks inside
    the timed region: per-shard host threads, one batched ncclReduce over xGMI): what a Rust / C caller of liboscen_gpu.so
    gets on a multi-GPU node.  Returns the record; `--cluster` prints it as the line, a `--gpus N` run without the flag
    carries it as the `og_cluster` sub-record."""
    import numpy as np
    import torch

    import oscen_amd

    graph = graph or args.graph
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (the engine has no CPU fallback)")
    n_dev = torch.cuda.device_count()
    devices = [0] * N if args.single_device else list(range(N))
    if not args.single_device and n_dev < N:
        sys.exit("bench.py --cluster --gpus %d: only %d device(s) visible" % (N, n_dev))
    block = args.block
    total_voices = V * N
    total_frames = (W + R * K) * block
    span = 0 if args.sparse_events else min(total_frames, 48000)
    cl = oscen_amd.Cluster(graph, total_voices, devices, sample_rate=48000.0)
    plans = oscen_amd.note_plans(total_voices, span=span, fold="slice")
    cl.set_voice_values("frequency", plans["frequency"])
    ev_v, ev_f, ev_x = plans["events"]
    if total_frames > 48000:  # a run longer than the 1 s score plays it again and again
        reps = -(-total_frames // 48000)
        ev_v, ev_f, ev_x = np.tile(ev_v, reps), np.concatenate([ev_f + 48000 * k for k in range(reps)]), np.tile(ev_x, reps)
    keep = ev_f < total_frames
    has_gate = True
    try:
        cl.schedule_voice_events("gate", ev_v[keep], ev_f[keep], ev_x[keep])
    except oscen_amd.OscenError:
        has_gate = False
    n_events_timed = int(np.count_nonzero((ev_f >= W * block) & (ev_f < total_frames))) if has_gate else 0
    if has_gate and args.group_voices:
        cl.group_voices(args.group_voices)
    shard0 = cl.shard(0)
    shards = [cl.shard(s) for s in range(cl.num_shards)]
    if W > 0:
        cl.render(W * block, block)
    torch.cuda.synchronize()
    for sh in shards:
        sh.enable_kernel_timing(True)
    cl.enable_reduce_timing(True)
    times = []
    mix = None
    for r in range(R):
        for d in set(devices):
            torch.cuda.synchronize(d)
        t0 = time.perf_counter()
        mix = cl.render(K * block, block)  # blocks until the reduced bus of all K blocks is in host memory
        for d in set(devices):
            torch.cuda.synchronize(d)
        times.append(time.perf_counter() - t0)
    per_shard = []
    for sh in shards:  # every shard's own voice-kernel time (HIP events on its stream)
        ms, n = sh.kernel_time_ms()
        per_shard.append((ms, n, sh.kernel_blocks_timed))
        sh.enable_kernel_timing(False)
    kern_ms, n_launch, n_blocks_timed = per_shard[0]
    red_total_ms, red_n = cl.reduce_time_ms()
    cl.enable_reduce_timing(False)
    assert np.isfinite(mix).all() and np.abs(mix).max() > 0.0, "bus is silent or non-finite"
    if dump_dir:
        dump_outputs(dump_dir, np.asarray(mix, dtype=np.float32).reshape(K, block, -1)[-1])
    elapsed, stats = region_stats(times, total_voices, K, block)
    line = {
        "metric": "voices*samples/sec (fm-synth graph, 48 kHz)",
        "value": total_voices * K * block / elapsed,
        "unit": "voices*samples/s",
        "n_gpus": N,
        "steps": K,
        "warmup": W,
        "ms_per_step": elapsed / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": "fm-synth voice bank (FMVoice graph) through the C-ABI cluster (og_cluster_render), %d voices/GPU on %d "
                        "device(s), block=%d frames, 48 kHz, f32; synthetic note streams splitmix64(0x05CE2026 ^ voice) "
                        "resident in HBM; %d note events inside the timed regions; %s"
                        % (V, len(set(devices)), block, n_events_timed,
                           "mix bus of each launch batch summed with one ncclReduce over xGMI" if cl.rccl_reduces
                           else "one device: no collective on the data path"),
            "graph": graph,
            "voices_per_gpu": V,
            "total_voices": total_voices,
            "block": block,
            "sample_rate": 48000,
            "parallelism": "cluster voice-shard x%d (one process, one host thread per shard)" % N,
            "events_in_timed_region": n_events_timed,
            "note_plan_span_frames": span if span else 48000,
            "event_path": "resident timeline (og_cluster_schedule_voice_events)",
        },
        "timing": stats,
        "rccl_ranks": cl.num_devices if cl.rccl_reduces else None,
        "cluster": {"shards": cl.num_shards, "devices": cl.num_devices, "rccl_reduces": cl.rccl_reduces},
        "multi_gpu": {
            "rccl_ranks": cl.num_devices if cl.rccl_reduces else None,
            "backend": "RCCL (ncclReduce issued by the library, one communicator per device)" if cl.rccl_reduces else "none (one device)",
            "per_rank_kernel_ms_avg": [p[0] for p in per_shard],
            "per_rank_kernel_ms_per_block": [p[0] * p[1] / max(1, p[2]) for p in per_shard],
            "reduce_ms_total": red_total_ms,
            "reduces_timed": red_n,
            "reduce_ms_avg": red_total_ms / red_n if red_n else None,
            "reduce_share_of_run": (red_total_ms / R) / (elapsed * 1e3) if red_n else None,
            "note": "reduce = device time between HIP events recorded around each batched ncclReduce on the root's stream "
                    "(og_cluster_reduce_time_ms); it overlaps the next batch's voice kernels",
        },
        "offline_voices_at_48k": total_voices * K * block / elapsed / 48000.0,
        "roofline": roofline_record(shard0, V, block, graph, kern_ms, n_launch, n_blocks_timed),
        "cpu_baseline": None,
    }
    if not args.single_device and N > 1:
        assert cl.rccl_reduces and cl.num_devices == N, "the cluster's RCCL leg did not span %d devices" % N
    cl.close()
    return line


class Watchdog:
    """Calls `on_timeout` from another thread unless cancel() comes within `seconds` (C calls release the GIL, so a leg that
    hangs inside the library or inside RCCL does not block it)."""

    def __init__(self, seconds, on_timeout):
        import threading

        self._done = threading.Event()
        self._thread = threading.Thread(target=lambda: None if self._done.wait(seconds) else on_timeout(), daemon=True)
        self._thread.start()

    def cancel(self):
        self._done.set()


def _sig(x, n=6):
    """Floats to n significant digits (the line is read by people and by a tail-limited log), everything else as is."""
    if isinstance(x, float):
        return float("%.*g" % (n, x)) if x == x and x not in (float("inf"), float("-inf")) else None
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, n) for v in x]
    return x


def _pick(d, keys):
    return None if d is None else {k: d[k] for k in keys if k in d}


LINE_LIMIT = 8000  # bytes: a log that keeps only its last 8 KB still holds the whole line (tests/test_bench_line_cpu.py)


def compact_line(full):
    """The ONE line of the contract, <= LINE_LIMIT bytes: the contract's keys, a trimmed `roofline` and `cpu_baseline`, the
    compact `configs` array and one-number summaries of the other legs.  Everything else (every region's time, the real-time
    runs, the CPU scaling probe, per-configuration roofline records) is in the detail record emit() writes beside it."""
    out = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                    "vs_baseline", "dtype", "data")}
    cfg = dict(full.get("config") or {})
    if len(str(cfg.get("workload", ""))) > 420:
        cfg["workload"] = cfg["workload"][:417] + "..."
    out["config"] = cfg
    rf = full.get("roofline")
    if rf is not None:
        r = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "traffic", "dram_gbs", "traffic_bytes_per_launch", "traffic_source",
                       "stale_profile", "kernel_variant", "kernel_hash", "kernel_ms_avg", "kernel_launches", "blocks_per_launch",
                       "kernel_ms_per_block", "algorithmic_bytes_per_launch", "bytes_per_voice_sample", "pipeline_waves_per_64_voices"))
        r["achieved_is"] = "charged bytes (SURVEY 8d) / kernel time; DRAM bandwidth by counters = dram_gbs; the bound that applies = valu_issue"
        r["valu_issue"] = _pick(rf.get("valu_issue"), ("achieved", "peak", "measured_ceiling", "unit", "frac", "frac_of_measured_ceiling",
                                                       "valu_wave_inst_per_64_voices_per_frame", "cycles_per_valu_inst_per_simd"))
        out["roofline"] = r
    else:
        out["roofline"] = None
    cb = full.get("cpu_baseline")
    if cb is not None:
        c = _pick(cb, ("value", "unit", "cores", "kind", "single_thread", "per_thread", "cpu_count"))
        c["sample"] = str(cb.get("sample", ""))[:360]
        cs = cb.get("criterion_shapes") or {}
        c["criterion_shapes"] = {k: v for k, v in cs.items() if k != "source"}
        out["cpu_baseline"] = c
    else:
        out["cpu_baseline"] = None
    tm = full.get("timing") or {}
    out["timing"] = _pick(tm, ("repeats", "value_median", "value_min", "value_max", "value_first_region", "value_median_first5", "repeats_rule"))
    if out["timing"] is not None:
        k = [x for x in (tm.get("kernel_sclk_ghz") or []) if x]
        out["timing"]["kernel_sclk_ghz_first_last"] = [k[0], k[-1]] if k else None
        if len(str(out["timing"].get("repeats_rule", ""))) > 80:
            out["timing"]["repeats_rule"] = out["timing"]["repeats_rule"][:77] + "..."
    out["value_median_first5"] = tm.get("value_median_first5")
    out["wall_s"] = full.get("wall_s")
    out["rccl_ranks"] = full.get("rccl_ranks")
    mg = full.get("multi_gpu")
    out["multi_gpu"] = None if mg is None else {k: v for k, v in mg.items() if not isinstance(v, (list, dict)) or len(json.dumps(v)) < 400}
    for k in ("config4", "og_cluster"):
        if full.get(k) is not None:
            rec = full[k]
            out[k] = {kk: vv for kk, vv in rec.items() if not isinstance(vv, (list, dict)) or len(json.dumps(vv)) < 300}
    if full.get("event_stats") is not None:
        out["event_stats"] = full["event_stats"]
    rt = full.get("realtime")
    if rt is not None:
        def one(r):
            lat = r.get("latency_ms") or {}
            rec = {"voices": r.get("voices"), "loaded": bool(r.get("resident_score_events")), "p50_ms": lat.get("p50"), "p99_ms": lat.get("p99"),
                   "max_ms": lat.get("max"), "misses": r.get("deadline_misses"), "blocks": r.get("blocks")}
            if r.get("paced"):
                rec["paced_p99_ms"], rec["paced_misses"] = (r["paced"].get("latency_ms") or {}).get("p99"), r["paced"].get("deadline_misses")
            return rec
        runs = list((rt.get("idle_bank") or {}).get("runs") or []) + list((rt.get("loaded") or {}).get("runs") or [])
        runs = [r for r in runs if isinstance(r, dict) and "voices" in r][:8]
        out["realtime"] = {"deadline_ms": runs[0].get("deadline_ms") if runs else None,
                           "midi_messages_per_block": runs[0].get("midi_messages_per_block") if runs else None,
                           "entry": "og_midi_send_batch + og_midi_process_block (blocking), one launch per block", "runs": [one(r) for r in runs]}
        out["realtime_voices_at_48k"] = full.get("realtime_voices_at_48k")
    else:
        out["realtime"] = None
    out["offline_voices_at_48k"] = full.get("offline_voices_at_48k")
    if full.get("configs") is not None:
        out["configs"], out["configs_keys"] = full["configs"], full["configs_keys"]
    out["detail"] = full.get("detail")
    # (the contract's own numbers -- value, ms_per_step -- stay at full precision: a reader may cross-check one against the other)
    out = {k: (_sig(v, 17) if not isinstance(v, (dict, list)) else _sig(v)) for k, v in out.items()}
    s = json.dumps(out, allow_nan=False)
    for k in ("realtime", "og_cluster", "config4", "multi_gpu", "timing"):  # (never print a line a tail would cut)
        if len(s) <= LINE_LIMIT:
            break
        out[k] = "dropped: the line would exceed %d bytes; see the detail record" % LINE_LIMIT
        s = json.dumps(out, allow_nan=False)
    return s


def emit(full):
    """Write the FULL record to a side file and to stdout as a `BENCH_DETAIL ` line, then the compact line of the contract as
    the LAST line of stdout."""
    import ctypes

    path = os.environ.get("OSCEN_BENCH_DETAIL")
    if not path:
        d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpurun_out")
        try:
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, "bench_detail_n%s.json" % full.get("n_gpus", 1))
        except OSError:
            path = None
    detail = json.dumps(_sig(full, 9))
    if path:
        try:
            with open(path, "w") as f:
                f.write(detail + "\n")
            full["detail"] = os.path.relpath(path, os.path.dirname(os.path.abspath(__file__)))
        except OSError:
            full["detail"] = "stdout: the BENCH_DETAIL line above"
    # RCCL writes a version banner through C stdio: push it out first, so that the JSON is the LAST line of stdout
    ctypes.CDLL(None).fflush(None)
    sys.stdout.write("BENCH_DETAIL " + detail + "\n")
    sys.stdout.write(compact_line(full) + "\n")
    sys.stdout.flush()


def emit_line_and_exit(line, extra):
    """The watchdog's exit: print the line as it stands (plus `extra`) as the LAST line of stdout and leave the process."""
    line.update(extra)
    emit(line)
    os._exit(0)


def dump_outputs(d, bus):
    """--dump-outputs: what a caller of the timed path received from its last step, the mix bus of the last timed block
    ([frames, channels] float32), as <d>/bus.npy."""
    import numpy as np

    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "bus.npy"), np.ascontiguousarray(bus, dtype=np.float32))


def run_cluster(args):
    """--cluster: ONE process drives every GPU through the C-ABI cluster."""
    R = args.repeats if args.repeats > 0 else (5 if args.full else 1)
    line = cluster_record(args, args.gpus, args.voices_per_gpu, args.steps, args.warmup, R, dump_dir=args.dump_outputs)
    emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=188)   # 188 x 256 frames = 1 s of audio
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline figure: repeated timed regions, the other BASELINE configurations "
                         "(N > 1: config4 and the og_cluster leg), the real-time record and the CPU baseline")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the mix bus of the last timed step to DIR/bus.npy (float32, [frames, channels])")
    ap.add_argument("--repeats", type=int, default=0,
                    help="how many times the K-step timed region is run (value = the median region; every region is in the line).  "
                         "0 = one region after a warm-up of ~40 ms of work; with --full, as many as make ~40 ms of timed work, at least 5 "
                         "and at most 48: the GPU's clock governor needs tens of "
                         "milliseconds of load to settle (measured round 5: forty-eight 0.75 ms regions in a row go 0.76 -> 0.68 ms, "
                         "the cycle count per frame of the kernel is the same throughout -- GRBM_GUI_ACTIVE), so five regions of 20 "
                         "blocks measure the governor, not the kernel")
    ap.add_argument("--voices-per-gpu", type=int, default=65536,
                    help="65536 = BASELINE configs[1]; 262144 with --gpus 8 = configs[3] (2 097 152 voices)")
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--graph", default="fm_voice")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--variant", default=None, choices=["survey2"],
                    help="survey2 = SURVEY 8(d) config 2's variant of the fm-synth bank: op3_feedback .3, op2_feedback .2, route .5, "
                         "filter_env_amount 2000 (per-sample tan) and the 2 205-frame filter_cutoff ramp at frame 4 800 of every timed second")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the `configs` array (the other BASELINE configurations, measured after the headline at N = 1)")
    ap.add_argument("--no-realtime", action="store_true", help="skip the blocking-path real-time latency record")
    ap.add_argument("--per-block-calls", action="store_true",
                    help="hand the blocks of a region to the engine one og_process_block_async call at a time (default: one "
                         "og_process_blocks_async call per run of blocks with nothing in between)")
    ap.add_argument("--cluster-timeout", type=int, default=300,
                    help="N > 1: seconds the og_cluster sub-record may take before the line is printed without it")
    ap.add_argument("--rt-blocks", type=int, default=1000, help="blocks per bank size of the real-time record")
    ap.add_argument("--rt-paced-blocks", type=int, default=750,
                    help="blocks of the paced run (one call per 5.33 ms block period) on the largest bank of the real-time record")
    ap.add_argument("--rt-voices", default="65536,1048576,8388608",
                    help="bank sizes of the real-time record (comma separated)")
    ap.add_argument("--rt-midi", type=int, default=1000, help="live MIDI messages per block in the real-time record")
    ap.add_argument("--rt-loaded-voices", default="4194304,6291456,8388608",
                    help="bank sizes of the LOADED real-time record: the synthetic score resident on every voice + the live "
                         "messages (empty: skip)")
    ap.add_argument("--rt-loaded-blocks", type=int, default=1000, help="back-to-back blocks per loaded bank")
    ap.add_argument("--rt-loaded-paced-blocks", type=int, default=750, help="paced blocks on the largest loaded bank that met every deadline")
    ap.add_argument("--cluster", action="store_true",
                    help="multi-GPU through the C-ABI cluster (og_cluster_*, one process) instead of one rank per GPU; "
                         "with --gpus 1 the plain engine path runs (identical to the default)")
    ap.add_argument("--bus-batch", type=int, default=0,
                    help="blocks the engine may render per kernel launch (og_set_bus_batching: 0 = the engine's choice, 8..32 "
                         "by bank size; 1 = a launch and a bus reduce per block)")
    ap.add_argument("--sparse-events", action="store_true",
                    help="keep the 1 s note plan as is even when the run is shorter (default: every voice plays a slice "
                         "of its cyclic plan, so that note-on, note-off and retrigger all fall inside the timed region at "
                         "the plan's real density)")
    ap.add_argument("--midi-live", type=int, default=0, metavar="N",
                    help="live path: N MIDI messages per block through og_midi_send_batch; the block is enqueued with "
                         "og_midi_process_block_async (the host parses block k+1 while block k renders)")
    ap.add_argument("--group-voices", type=int, nargs="?", const=1, default=1, metavar="POLICY",
                    help="og_group_voices(POLICY) after the score is scheduled (default 1; 0 = off): voice slots ordered by first "
                         "note-off, so that the voices of a wave release together and the wave takes the cheaper chunk bodies more "
                         "often -- same voices, same per-voice samples bit for bit; the bus differs by the association of the sum.  "
                         "Measured round 5: +2.5 % at the driver's command, +5 % at 131 072 voices, +10 % at 1 048 576")
    ap.add_argument("--midi-blocking", action="store_true",
                    help="with --midi-live: the blocking drop-in entry og_midi_process_block (= process_block + bus to host)")
    # plumbing checks of the multi-rank path on a 1-GPU box (not a benchmark configuration):
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--single-device", action="store_true", help="map every rank / shard onto GPU 0")
    ap.add_argument("--dist-single", action="store_true",
                    help="run the RCCL leg (process group, reduce, barrier) with a one-rank communicator: RCCL refuses two "
                         "ranks on one GPU ('Duplicate GPU detected'), so this is how a one-GPU box exercises it")
    ap.add_argument("--realtime-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--test-scale", type=int, default=1, help=argparse.SUPPRESS)  # tests/test_bench_line_cpu.py: banks and runs of `configs` divided by this
    args = ap.parse_args()
    if args.group_voices:
        os.environ["OSCEN_BENCH_GROUP_VOICES"] = str(args.group_voices)

    if args.realtime_child:
        # the real-time record in a process of its own: numpy + the engine, nothing else -- like a host application.  (In
        # the bench process torch is loaded: its heap makes a collector pass cost 20-40 ms, and the pageable transfers
        # torch made for the timed regions leave pinned host mappings behind whose later release stalls the GPU queues.)
        rt_voices = [int(x) for x in args.rt_voices.split(",") if x.strip()]
        ld_voices = [int(x) for x in args.rt_loaded_voices.split(",") if x.strip()]
        rec = realtime_record(args.graph, args.block, rt_voices, args.rt_blocks, args.rt_midi, 0, args.rt_paced_blocks,
                              ld_voices, args.rt_loaded_blocks, args.rt_loaded_paced_blocks)
        sys.stdout.flush()
        print("REALTIME_RECORD " + json.dumps(rec))
        return 0

    if args.cluster and args.gpus > 1:
        if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
            sys.exit("bench.py --cluster is a single-process mode: start it as `python bench.py --gpus N --cluster`")
        return run_cluster(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import numpy as np
    import torch

    import oscen_amd
    from oscen_amd import distributed as ogd

    rank, local_rank, world_size = ogd.world()
    if world_size != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d ranks" % (args.gpus, world_size))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (the engine has no CPU fallback)")
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    rccl_ranks = None
    if world_size > 1 or args.dist_single:
        import torch.distributed as dist

        if world_size == 1:
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
            s.close()
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group(args.backend, rank=rank, world_size=world_size)

    V, K, W = args.voices_per_gpu, args.steps, args.warmup
    W_run = W  # warm-up blocks rendered
    if args.repeats > 0:
        R, repeats_rule = args.repeats, "--repeats %d" % args.repeats
    elif args.full:
        est_region_ms = max(1e-3, K * 0.045 * V / 65536.0)  # ~0.045 ms per 256-frame block of 65 536 fm voices
        R = int(max(5, min(48, -(-40.0 // est_region_ms))))
        repeats_rule = "auto: ~40 ms of timed work (5..48 regions) so that the clock governor has settled by the median region"
    else:
        # ONE region of exactly K timed blocks.  The clock governor needs ~40 ms of load to settle (see --repeats): the
        # warm-up is stretched to that much estimated work, a block count fixed by the arguments, so that the same
        # arguments render the same blocks on every run.  (The load has to be this bank's own: measured on MI355X, ~40 ms
        # on a second bank closed right before the warm-up leaves the region at the cold clock.)
        R = 1
        W_run = max(W, min(1024, int(-(-40.0 // max(0.01, 0.045 * V / 65536.0)))))
        repeats_rule = "one region of --steps blocks after %d warm-up blocks (~40 ms of work: the clock governor settles first)" % W_run
    # wall-clock budget of the run, leg by leg (N > 1: the driver's 8-GPU command = headline + config4 + og_cluster; the line
    # carries it so that the run can be seen to fit a timeout before one is hit -- VERDICT r5, item 8)
    t_legs, t_leg0 = {}, time.time()
    m = timed_bank(args, args.graph, V, K, W_run, R, rank, local_rank, world_size, dist, args.variant)
    t_legs["headline"] = time.time() - t_leg0
    eng, times, kern_ms, n_launch, n_blocks_timed, multi_gpu = m.eng, m.times, m.kern_ms, m.n_launch, m.n_blocks_timed, m.multi_gpu
    rccl_ranks, timed_blocks, bus, host_bus, midi = m.rccl_ranks, m.timed_blocks, m.bus, m.host_bus, m.midi
    n_events_timed, span, total_voices, block = m.n_events_timed, m.span, m.total_voices, m.block

    # N > 1: BASELINE config 4's per-GPU shard (262 144 voices per GPU, 1 s of audio per region) through the same ranks and
    # the same RCCL reduce, as a sub-record of the line (the driver's command does not pass --voices-per-gpu)
    config4 = None
    V4 = max(64, 262144 // args.test_scale)
    if args.full and world_size > 1 and not args.no_configs and args.graph == "fm_voice" and not args.midi_live and not args.variant and V4 != V:
        K4, W4, R4 = (188, 8, 3) if args.test_scale == 1 else (4, 2, 2)
        t_leg0 = time.time()
        m4 = timed_bank(args, "fm_voice", V4, K4, W4, R4, rank, local_rank, world_size, dist, None)
        t_legs["config4"] = time.time() - t_leg0
        if rank == 0:
            e4, _ = region_stats(m4.times, m4.total_voices, K4, block)
            rf4 = roofline_record(m4.eng, V4, block, "fm_voice", m4.kern_ms, m4.n_launch, m4.n_blocks_timed)
            config4 = {"config": "4: fm-synth %d voices sharded over %d GPUs (%d per GPU), one reduce of the [K x block] mix bus per region"
                                 % (m4.total_voices, world_size, V4),
                       "total_voices": m4.total_voices, "voices_per_gpu": V4, "steps": K4, "repeats": R4,
                       "value": m4.total_voices * K4 * block / e4, "ms_per_step": e4 / K4 * 1e3, "rccl_ranks": m4.rccl_ranks,
                       "multi_gpu": m4.multi_gpu, "kernel": rf4["kernel_variant"], "kernel_ms_per_block": rf4["kernel_ms_per_block"],
                       "roofline_frac": rf4["frac"], "valu_issue_frac": (rf4.get("valu_issue") or {}).get("frac"),
                       "dram_gbs": rf4["dram_gbs"], "stale_profile": rf4["stale_profile"]}
        m4.eng.close()
        del m4
    if world_size > 1 and args.backend == "nccl" and not args.single_device:
        assert rccl_ranks == world_size, "RCCL communicator spans %s ranks, expected %d" % (rccl_ranks, world_size)

    if rank == 0:
        sel = torch.from_numpy(timed_blocks)
        mix = host_bus[timed_blocks] if (midi is not None and args.midi_blocking) else bus[sel.to(bus.device)].float().cpu().numpy()
        assert np.isfinite(mix).all() and np.abs(mix).max() > 0.0, "bus is silent or non-finite"
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, mix[-1].reshape(block, -1))
        elapsed, stats = region_stats(times, total_voices, K, block)
        value = total_voices * K * block / elapsed
        line = {
            "metric": "voices*samples/sec (fm-synth graph, 48 kHz)",
            "value": value,
            "unit": "voices*samples/s",
            "n_gpus": world_size,
            "steps": K,
            "warmup": W,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": "fm-synth voice bank (FMVoice graph), %d voices/GPU, block=%d frames, 48 kHz, f32; "
                            "synthetic note streams splitmix64(0x05CE2026 ^ voice) resident in HBM%s; "
                            "%d note events (on / off / retrigger) fall inside the %d timed regions; %s"
                            % (V, block, "" if not span or span == 48000 else
                               ", the %d-frame run plays every voice's cyclic 1 s note plan from a per-voice offset: the plan's real event density in every region" % span,
                               n_events_timed, R,
                               "one GPU: no collective on the data path" if dist is None else
                               "the [K x block] mix bus of a region reduced once over %s (%d rank%s)"
                               % ("RCCL" if args.backend == "nccl" else "gloo", world_size, "" if world_size == 1 else "s")),
                "graph": args.graph,
                "voices_per_gpu": V,
                "total_voices": total_voices,
                "block": block,
                "sample_rate": 48000,
                "parallelism": "voice-shard x%d" % world_size,
                "events_in_timed_region": n_events_timed // R,
                "note_plan_span_frames": span if span else 48000,
                "blocks_per_launch_limit": args.bus_batch if args.bus_batch else "engine's choice (8..32 by bank size)",
                "host_calls": "one og_process_block_async per block" if (midi is not None or args.per_block_calls)
                              else "one og_process_blocks_async per run of blocks between value changes (K blocks per region)",
                "voice_slots": ("grouped by first note-off (og_group_voices policy %d)" % args.group_voices) if (args.group_voices and midi is None) else "in voice order",
                "event_path": ("midi-live (og_midi_send_batch + %s per block)" %
                               ("og_midi_process_block, blocking" if args.midi_blocking else "og_midi_process_block_async"))
                              if midi is not None
                              else "resident timeline (og_schedule_voice_events)",
            },
            # kernel_sclk_ghz: the shader clock the voice kernel ran at in each region, measured by the kernel itself (workgroup
            # 0: shader cycles / 100 MHz ticks between its first and last instruction, og_kernel_clock_ghz) -- region times
            # follow it; sclk_ghz_after_region: what an idle-GPU probe reads right after the region (og_shader_clock_ghz)
            "timing": dict(stats, repeats_rule=repeats_rule, kernel_sclk_ghz=[None if not x else round(x, 3) for x in m.kclk],
                           sclk_ghz_after_region=[None if x is None else round(x, 3) for x in m.sclk]),
            "rccl_ranks": rccl_ranks,
            "multi_gpu": multi_gpu,  # None at N = 1 (no collective on the data path)
            # throughput of the QUEUED path (blocks known ahead, up to 32 per launch) expressed in 48 kHz voices: an
            # offline-render rate.  The real-time figure comes from the blocking entry: realtime.realtime_voices_at_48k
            "offline_voices_at_48k": value / 48000.0,
            "roofline": roofline_record(eng, V, block, args.graph, kern_ms, n_launch, n_blocks_timed, args.variant),
        }
        # the bound that applies (VALU issue) next to the contract's HBM object, so that nobody reads
        # the charged-bytes fraction as a bandwidth
        line["valu_issue"] = line["roofline"].get("valu_issue")
        if args.variant:
            line["config"]["variant"] = args.variant
        if midi is not None:
            line["config"]["midi_messages_per_block"] = args.midi_live
            line["event_stats"] = eng.event_stats
    else:
        line = None
    if dist is not None:
        if args.backend == "gloo":
            dist.barrier()
        else:
            dist.barrier(device_ids=[local_rank])
        dist.destroy_process_group()
    # N > 1: rank 0 goes on to drive ALL N devices from one process (the og_cluster leg).  The other ranks give their device
    # back first -- engine closed, allocator emptied -- and say so through a file; rank 0 waits for every such file before it
    # touches their devices (torchrun gives no "the others are done" signal once the process group is gone).
    release_dir = None
    cluster_leg = args.full and world_size > 1 and not args.no_configs and not args.midi_live and not args.variant
    if cluster_leg:
        import tempfile
        release_dir = os.path.join(tempfile.gettempdir(), "oscen_bench_release_%d_%s" % (os.getppid(), os.environ.get("MASTER_PORT", "0")))
        os.makedirs(release_dir, exist_ok=True)
        if rank != 0:
            eng.close()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            with open(os.path.join(release_dir, "rank%d.released" % rank), "w") as f:
                f.write("%f\n" % time.time())
    if line is not None:
        has_gate = "gate" in eng.input_names
        if config4 is not None:
            line["config4"] = config4
        if cluster_leg:
            # the SAME workload through the product's own multi-GPU leg: one process, og_cluster_* over all N devices, the
            # library's ncclReduce (the ranks above used torch.distributed's communicator).  Rank 0 runs it after the
            # process group is gone; the other ranks have finished.
            eng.close()
            t_leg0 = time.time()
            want = [os.path.join(release_dir, "rank%d.released" % r) for r in range(1, world_size)]
            while not all(os.path.exists(w) for w in want) and time.time() - t_leg0 < 60.0:
                time.sleep(0.02)
            released = all(os.path.exists(w) for w in want)
            t_legs["wait_for_ranks_to_release_devices"] = time.time() - t_leg0
            for w in want:
                try:
                    os.remove(w)
                except OSError:
                    pass
            try:
                os.rmdir(release_dir)
            except OSError:
                pass
            t_leg0 = time.time()
            # (the one leg of an N > 1 run that no rank-per-GPU phase above has exercised: if it does not come back, the
            #  line -- headline and config4 complete -- is printed without it instead of being lost with the process)
            guard = Watchdog(args.cluster_timeout, lambda: emit_line_and_exit(
                line, {"og_cluster": {"error": "the og_cluster leg did not finish within %d s" % args.cluster_timeout},
                       "realtime": None, "cpu_baseline": None}))
            try:
                c = cluster_record(args, world_size, V, K, W, R)
                line["og_cluster"] = {k: c[k] for k in ("value", "ms_per_step", "rccl_ranks", "cluster", "multi_gpu", "timing")}
                line["og_cluster"]["entry"] = "og_cluster_create + og_cluster_render (C ABI, one process, the library's own RCCL communicator)"
                rf = c["roofline"]
                line["og_cluster"]["kernel"], line["og_cluster"]["kernel_ms_per_block"] = rf["kernel_variant"], rf["kernel_ms_per_block"]
            except (Exception, SystemExit) as e:
                line["og_cluster"] = {"error": str(e)[:300]}
            finally:
                guard.cancel()
            if isinstance(line.get("og_cluster"), dict):
                line["og_cluster"]["ranks_released_devices_first"] = released
            t_legs["og_cluster"] = time.time() - t_leg0
        configs = None
        if args.full and world_size == 1 and not args.no_configs and args.graph == "fm_voice" and not args.midi_live and not args.variant:
            eng.close()
            torch.cuda.synchronize()
            configs = config_records(args, local_rank)
            line["configs_detail"] = configs
        if args.full and world_size == 1 and not args.no_realtime and has_gate and args.graph == "fm_voice":
            torch.cuda.synchronize()
            env = dict(os.environ)
            env["HIP_VISIBLE_DEVICES"] = env.get("HIP_VISIBLE_DEVICES", "").split(",")[local_rank] if env.get("HIP_VISIBLE_DEVICES") else str(local_rank)
            cmd = [sys.executable, os.path.abspath(__file__), "--realtime-child", "--graph", args.graph, "--block", str(block),
                   "--rt-voices", args.rt_voices, "--rt-blocks", str(args.rt_blocks), "--rt-midi", str(args.rt_midi),
                   "--rt-paced-blocks", str(args.rt_paced_blocks), "--rt-loaded-voices", args.rt_loaded_voices,
                   "--rt-loaded-blocks", str(args.rt_loaded_blocks), "--rt-loaded-paced-blocks", str(args.rt_loaded_paced_blocks)]
            try:
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500)
                rec = [ln for ln in out.stdout.splitlines() if ln.startswith("REALTIME_RECORD ")]
                if out.returncode != 0 or not rec:
                    raise RuntimeError("child exited with %d: %s" % (out.returncode, out.stderr[-400:]))
                line["realtime"] = json.loads(rec[-1][len("REALTIME_RECORD "):])
                line["realtime"]["process"] = "a child process of bench.py (numpy + the engine; torch is not loaded there)"
            except Exception as e:  # (fall back to measuring in this process rather than losing the record)
                rt_voices = [int(x) for x in args.rt_voices.split(",") if x.strip()]
                ld_voices = [int(x) for x in args.rt_loaded_voices.split(",") if x.strip()]
                line["realtime"] = realtime_record(args.graph, block, rt_voices, args.rt_blocks, args.rt_midi, local_rank, args.rt_paced_blocks,
                                                   ld_voices, args.rt_loaded_blocks, args.rt_loaded_paced_blocks)
                line["realtime"]["process"] = "bench.py itself (the child process failed: %s)" % str(e)[:200]
            line["realtime_voices_at_48k"] = line["realtime"]["realtime_voices_at_48k"]
        else:
            line["realtime"] = None
        if args.full and world_size == 1 and not args.no_cpu_baseline:
            # (the oracle folds the plan the same way; a rotated plan of more than a second reads the same in any window)
            line["cpu_baseline"] = cpu_baseline(block, oscen_amd.SYNTH_SEED, K * block, span if span <= 48000 else 47999)
        else:
            line["cpu_baseline"] = None
        if configs is not None:
            # LAST key of the line, compact, so that the tail a log keeps still shows every configuration:
            # [name, voices, value, ms_per_step, kernel, roofline.frac, valu_issue.frac, dram GB/s, stale profile]
            def sig(x):
                return None if x is None else float("%.4g" % x)

            line["configs"] = [[c["config"].split(":")[0], c["voices"], sig(c.get("value")), sig(c.get("ms_per_step")), c.get("kernel"),
                                sig(c.get("roofline_frac")), sig(c.get("valu_issue_frac")), sig(c.get("dram_gbs")), c.get("stale_profile"),
                                c.get("error")] for c in configs]
            line["configs_keys"] = "name, voices, voices*samples/s, ms_per_step, kernel, roofline.frac (charged), valu_issue.frac, dram GB/s, stale_profile, error"
        t_legs["total_since_start"] = time.time() - T_START
        line["wall_s"] = {k: round(v, 2) for k, v in t_legs.items()}
        emit(line)


if __name__ == "__main__":
    main()
