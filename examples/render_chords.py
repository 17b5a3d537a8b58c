"""Play a short chord progression into a bank of FM voices through the MIDI front end and write a WAV.

    python examples/render_chords.py [out.wav] [--ir hall.wav]

raw MIDI bytes -> og_midi (parser, LRU voice allocator, note->Hz) -> per-voice frequency/gate events ->
fused voice kernel on the GPU -> mix bus -> 16-bit PCM.  Needs an MI355X (there is no CPU fallback).

--ir FILE puts a convolution reverb behind the voice sum: the WAV (any rate, 1..8 channels) is registered as an asset
response and published on an empty post-mix Convolver, which conforms it to 48 000 Hz on the device; the bus of FM voices
is mono, so a stereo response is averaged, as the reference's from_asset does.  The reference's counterpart is
`external ir: AudioAsset; ir -> reverb.ir;` with `graph.ir.load_wav(path)`.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oscen_amd  # noqa: E402

SR, BLOCK = 48000, 256
CHORDS = [(57, 60, 64, 69), (53, 57, 60, 65), (48, 52, 55, 60), (55, 59, 62, 67)]  # Am F C G


def reverb_graph():
    """fm_voice with `reverb = Convolver::new()` behind the voice sum: silent until a response is published"""
    g = oscen_amd.Graph(builtin="fm_voice")
    out = [ln.split()[1].rstrip(":;") for ln in g.to_dsl().splitlines() if ln.startswith("output ")][0]
    g.output_stream("wet")
    g.bus_convolver("reverb")
    g.connect(out, "reverb.input")
    g.connect("reverb.output", "wet")
    return g


def main(path, ir=None):
    eng = oscen_amd.Engine(reverb_graph() if ir else "fm_voice", 64, sample_rate=float(SR))
    tail = 0
    if ir:
        oscen_amd.register_ir_wav("chords::hall", ir)
        eng.set_bus_ir("chords::hall")  # conformed to SR, mapped onto the mono bus; fades in over the first 20 ms
        frames, channels, rate = oscen_amd.registered_ir("chords::hall")
        tail = eng.bus_ir().shape[0]
        print("reverb: %s, %d frames x %d channels at %d Hz -> %d taps at %d Hz" % (ir, frames, channels, rate, tail, SR))
    eng.set_value_immediate("filter_cutoff", 2400.0)
    eng.set_value_immediate("filter_env_amount", 3000.0)
    midi = oscen_amd.Midi(eng, 64)
    out = []
    bar = SR  # one chord per second
    total_blocks = (len(CHORDS) * bar + SR + tail) // BLOCK
    for b in range(total_blocks):
        f0 = b * BLOCK
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
    ap.add_argument("out", nargs="?", default="chords.wav")
    ap.add_argument("--ir", help="WAV file of an impulse response (PCM 16 / 24 / 32 or float 32, any rate)")
    a = ap.parse_args()
    main(a.out, a.ir)
