"""Chords through a master section behind the voice sum -- a post-mix graph -- into a WAV.

    python examples/render_master_bus.py [out.wav]

raw MIDI bytes -> og_midi -> 64 FM voices -> sum -> master low-pass with an LFO on its cutoff -> feedback echo -> gain ->
16-bit PCM.  The four nodes behind the sum are ordinary nodes of the library that tick once per frame on the summed voices:
they are compiled into a kernel of their own (og_kp_*); the voice kernel is the one fm_voice has without them.  The reference's
counterpart is the same four declarations in the wrapper graph with `voices.audio_out -> master.input`.
Needs an MI355X (there is no CPU fallback).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oscen_amd  # noqa: E402

SR, BLOCK = 48000, 256
CHORDS = [(57, 60, 64, 69), (53, 57, 60, 65), (48, 52, 55, 60), (55, 59, 62, 67)]  # Am F C G


def master_graph():
    """fm_voice with `lfo -> master.cutoff; voices -> master -> trim -> wet; master -> [echo] -> trim` behind the voice sum"""
    g = oscen_amd.Graph(builtin="fm_voice")
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.input_value("master_cutoff", 1800.0, ramp=2400)
    g.input_value("master_volume", 0.8)
    g.output_stream("wet")
    g.bus_node("lfo", "Oscillator::sine", 0.3, 1.0)
    g.bus_node("master", "TptFilter::new", 1800.0, 0.9)
    g.bus_node("echo", "Delay::new", 0.375 * SR, 0.45)  # a dotted eighth at 120 bpm, fed back
    g.bus_node("trim", "Gain::new", 0.8)
    g.connect(out, "master.input")
    g.connect("lfo.output * 900.0 + master_cutoff", "master.cutoff")
    g.connect("master.output", "trim.input")  # the filtered sum itself ...
    g.connect_via("master.output", "echo", "trim.input")  # ... plus its echoes: a fan-in sum
    g.connect("master_volume", "trim.gain")
    g.connect("trim.output", "wet")
    return g


def main(path):
    eng = oscen_amd.Engine(master_graph(), 64, sample_rate=float(SR))
    print("post-mix graph:", eng.post_mix_info(), "kind", eng.post_mix_kind)
    eng.set_value_immediate("filter_cutoff", 2400.0)
    eng.set_value_immediate("filter_env_amount", 3000.0)
    midi = oscen_amd.Midi(eng, 64)
    out = []
    bar = SR  # one chord per second
    total_blocks = (len(CHORDS) * bar + 3 * SR) // BLOCK  # ... and three seconds of echoes
    for b in range(total_blocks):
        f0 = b * BLOCK
        if f0 == 2 * bar:
            eng.set_value("master_cutoff", 4200.0)  # [ramp: 2400]: the master filter opens over 50 ms, frame by frame
        for ci, chord in enumerate(CHORDS):
            on, off = ci * bar, ci * bar + int(0.8 * bar)
            for k, note in enumerate(chord):
                t_on = on + k * 1200  # strum
                if f0 <= t_on < f0 + BLOCK:
                    midi.note_on(note, 70 + 10 * k, frame_offset=t_on - f0)
                if f0 <= off < f0 + BLOCK:
                    midi.note_off(note, frame_offset=off - f0)
        out.append(midi.process_block(BLOCK).copy())
    audio = np.concatenate(out, axis=0)
    peak = float(np.max(np.abs(audio)))
    audio = audio * np.float32(0.8 / max(peak, 1e-6))
    oscen_amd.write_wav(path, audio, sample_rate=SR, bits=16)
    print("wrote %s: %d frames, peak before normalisation %.3f" % (path, audio.shape[0], peak))
    return peak


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out", nargs="?", default="master_bus.wav")
    main(ap.parse_args().out)
