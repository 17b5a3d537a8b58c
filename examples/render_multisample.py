"""Render a small multisample bank -- every voice loops its own synthesised sample through an envelope -- and write a WAV.

    python examples/render_multisample.py [out.wav]
    python examples/render_multisample.py --out out.wav kick.wav snare.wav ...

register_sample -> Engine.load_sample -> Engine.set_voice_samples: each voice's SamplePlayer reads its buffer from the engine's
device sample pool; a gate event per voice opens its AdsrEnvelope.  Without input files the samples are synthesised here; with
WAV files on the command line (any rate: register_sample_wav keeps the file's rate and load_sample conforms it to the
engine's on the device) the pattern plays those instead.  Needs an MI355X (there is no CPU fallback).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oscen_amd  # noqa: E402

SR, BLOCK, VOICES = 48000, 256, 16
VOICE = """
name: SamplerVoice;
input gate: event;
output out: stream;
nodes { player = SamplePlayer::new(); env = AdsrEnvelope::new(0.005, 0.08, 0.5, 0.25); }
connections { gate -> env.gate; player.output * env.output -> out; }
"""


def tone(midi_note, cycles=64):
    """a few whole cycles of a bright tone: loops without a click"""
    freq = 440.0 * 2.0 ** ((midi_note - 69) / 12.0)
    n = int(round(cycles * SR / freq))
    t = np.arange(n) * (cycles / n)
    return (0.6 * np.sin(2 * np.pi * t) + 0.25 * np.sin(4 * np.pi * t) + 0.15 * np.sin(6 * np.pi * t)).astype(np.float32)


def main(path, wavs=()):
    eng = oscen_amd.Engine(oscen_amd.Graph(dsl=VOICE), VOICES, sample_rate=float(SR))
    notes = [48, 52, 55, 60, 64, 67, 72, 76]
    index = []
    for k, n in enumerate(notes):
        if wavs:  # the files in turn, at their own rates
            name = "wav_%d" % (k % len(wavs))
            oscen_amd.register_sample_wav(name, wavs[k % len(wavs)])
        else:
            name = "tone_%d" % n
            oscen_amd.register_sample(name, tone(n))
        index.append(eng.load_sample(name))
    step = SR // 4  # a note every quarter of a second, two voices per note an octave of the pattern apart
    out = []
    for b in range((len(notes) * step + SR) // BLOCK):
        f0 = b * BLOCK
        for k in range(len(notes)):
            for v in (k, k + len(notes)):
                on = k * step + (v // len(notes)) * 2 * step
                off = on + step
                if f0 <= on < f0 + BLOCK:
                    eng.set_voice_samples("player", [index[(k + v // len(notes) * 2) % len(notes)]], first=v)  # block-granular (re)trigger
                    eng.push_voice_event("gate", v, on - f0, 0.9)
                if f0 <= off < f0 + BLOCK:
                    eng.push_voice_event("gate", v, off - f0, 0.0)
        out.append(eng.process_block(BLOCK).copy())
    audio = np.concatenate(out, axis=0)
    peak = float(np.max(np.abs(audio)))
    audio = audio * np.float32(0.8 / max(peak, 1e-6))
    oscen_amd.write_wav(path, audio, sample_rate=SR, bits=16)
    print("wrote %s: %d frames, peak before normalisation %.3f" % (path, audio.shape[0], peak))
    return peak


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        k = args.index("--out")
        main(args[k + 1], args[:k] + args[k + 2:])
    else:
        main(args[0] if args else "multisample.wav")
