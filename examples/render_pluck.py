"""A Karplus-Strong string written as a CUSTOM node with a per-voice delay line, played through the MIDI front end into a WAV.

    python examples/render_pluck.py [out.wav]

The node is what a user of the reference writes as a `#[derive(Node)]` struct with a `line: [f32; 2048]` field: here the field
is an array field of a registered node type (og_node_array) -- per-voice device memory the process() body and the gate handler
reach through `line.get(i)` / `line.set(i, x)`.  on_gate fills the first `period` elements with noise from a per-voice LCG (a
u32 field); every tick averages two neighbours and writes the result back, so the line rings at sample_rate / period.

raw MIDI bytes -> og_midi (parser, LRU voice allocator, note->Hz) -> per-voice frequency / gate events -> fused voice kernel
on the GPU -> mix bus -> 16-bit PCM.  Needs an MI355X (there is no CPU fallback); with OSCEN_GPU_LIB pointing at the host
simulator of tests/hostsim it renders on the CPU.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oscen_amd  # noqa: E402

SR, BLOCK, VOICES, LINE = 48000, 256, 16, 2048
MELODY = [(0.00, 52), (0.25, 55), (0.50, 59), (0.75, 64), (1.00, 59), (1.25, 55), (1.50, 52), (1.75, 47),
          (2.00, 45), (2.25, 52), (2.50, 57), (2.75, 60), (3.00, 64), (3.00, 57), (3.00, 52), (3.00, 45)]  # (seconds, note)

PLUCK = dict(
    inputs=[("period", "value", 109.0, -1), ("gate", "event", 0.0, -1)], outputs=["output"],
    state=[("wp", "u32", 0, -1), ("seed", "u32", 22222, -1), ("loss", "f32", 0.996, -1)],
    arrays=[("line", LINE, "f32", 0.0)],
    process="""
    const uint32_t n = min(max((uint32_t)period, 2u), line.length());
    const uint32_t nx = wp + 1u >= n ? 0u : wp + 1u;
    const float a = line.get(wp);
    line.set(wp, (a + line.get(nx)) * 0.5f * loss);
    wp = nx;
    output = a;
""",
    handlers={"gate": """
    if (value > 0.0f) { // pluck: a burst of noise one period long
        const uint32_t n = min(max((uint32_t)period, 2u), line.length());
        for (uint32_t i = 0u; i < n; ++i) {
            seed = seed * 1664525u + 1013904223u;
            line.set(i, value * ((float)(seed >> 8) * (1.0f / 8388608.0f) - 1.0f));
        }
        wp = 0u;
        loss = 0.996f;
    } else {
        loss = 0.9f; // note off: damp the string
    }
"""})

DSL = """
name: pluck_voice;
input frequency: value = 220.0;
input gate: event;
output out: stream;
nodes {
    string = KarplusString::new();
}
connections {
    %d.0 / frequency -> string.period;
    gate -> string.gate;
    string.output -> out;
}
""" % SR


def main(path):
    oscen_amd.register_node("KarplusString::new", PLUCK["inputs"], PLUCK["outputs"], PLUCK["process"], state=PLUCK["state"],
                            handlers=PLUCK["handlers"], arrays=PLUCK["arrays"])
    eng = oscen_amd.Engine(oscen_amd.Graph(dsl=DSL, per_voice=("frequency",)), VOICES, sample_rate=float(SR))
    midi = oscen_amd.Midi(eng, VOICES)
    out = []
    for b in range(int(5.0 * SR) // BLOCK):
        f0 = b * BLOCK
        for t, note in MELODY:
            on, off = int(t * SR), int((t + 1.2) * SR)
            if f0 <= on < f0 + BLOCK:
                midi.note_on(note, 100, frame_offset=on - f0)
            if f0 <= off < f0 + BLOCK:
                midi.note_off(note, frame_offset=off - f0)
        out.append(midi.process_block(BLOCK).copy())
    audio = np.concatenate(out, axis=0)
    peak = float(np.max(np.abs(audio)))
    audio = audio * np.float32(0.8 / max(peak, 1e-6))
    oscen_amd.write_wav(path, audio, sample_rate=SR, bits=16)
    length, kind = eng.node_array_info("string.line")
    print("wrote %s: %d frames, peak before normalisation %.3f (%d voices, a %d-element %s line each)" % (path, audio.shape[0], peak, VOICES, length, kind))
    return peak


if __name__ == "__main__":
    try:
        main(sys.argv[1] if len(sys.argv) > 1 else "pluck.wav")
    except oscen_amd.OscenError as e:  # (no device: the engine has no CPU fallback)
        sys.exit(str(e))
