// og_scope.hip.h -- Oscilloscope (oscen-lib/src/oscilloscope/mod.rs): the signal passes through, the last `capacity` samples
// stay readable, and a rising zero crossing freezes the last period.  Included only by the kernels of graphs that hold a
// scope, behind og_node_array.hip.h (whose pool and word type it uses); its digest (OG_SCOPE_DIGEST, og_rt_digest.h) goes
// into THEIR hashes alone.
//
// The reference's process() (mod.rs:241-286): output = input; push(input) (51-65: ring[counter % capacity] = input,
// counter += 1, written = min(written + 1, capacity)); then, only while trigger_enabled > 0.5, with
// crossing = last_sample <= 0.0 && input > 0.0:
//   manual (273-282):       crossing -> store_triggered(round(max(trigger_period, 1.0)) as usize)
//   auto-detect (253-272):  period_sample_count += 1; crossing -> { if period_sample_count > 1 { detected_period =
//                           max(min(period_sample_count, capacity), 10) }; store_triggered(detected_period);
//                           period_sample_count = 0 }
// and last_sample = input always (285).  store_triggered(length) (111-123): length = max(min(length, capacity), 1);
// triggered[0..length) = the last `length` pushed samples in time order; triggered_length = length.
//
// What is NOT done here is the copy inside the tick.  Two runs of planes per scope in the node-array pool
// ([element][n_voices], voices contiguous):
//   ring    P elements, the PHYSICAL ring: P = 2 x capacity rounded up to a multiple of OG_BUS_CHUNK, + OG_BUS_CHUNK
//           (scope_ring_len; what the deadline below needs is P >= capacity + OG_BUS_CHUNK)
//   frozen  capacity elements, the frozen window
// A tick stores `input` at the lane's write position (voices started together share it: one 256-byte run per wave) and
// does register work.  A crossing records where its window ENDS in the physical ring (window_end, one past its last sample)
// and how long it is (triggered_length), and sets `pending`; a newer crossing simply replaces these.  At the top of every
// chunk (scope_chunk_begin) a lane whose pending window would be reached by the pushes of the chunk that starts now copies
// it into `frozen` and clears the mark.
//   Deadline.  d = pushes since the crossing = (write_pos - window_end) mod P; the pushes of a chunk overwrite the window's
//   first sample once d + OG_BUS_CHUNK > P - triggered_length.  At the crossing d = 0 and P - triggered_length >=
//   OG_BUS_CHUNK, so the rest of that chunk (< OG_BUS_CHUNK pushes) cannot reach it, and every later chunk is checked
//   before its first push: one test per chunk is enough and loses nothing.
// With P >= 2 x capacity + OG_BUS_CHUNK a window stays pending for at least `capacity` pushes, so a signal whose period is at
// most the capacity never copies: its next crossing comes first.  A copy happens only when crossings stop.
//
// The samples in front of the first push read 0.0, the planes' og_init fill (the reference forms their index with
// usize::wrapping_sub, which for a capacity that is no power of two lands on a slot that depends on the width of usize).
//
// Addresses are in the GLOBAL address space (og::narr_word); a lane beyond the bank's last voice neither loads nor stores.
#pragma once

namespace og {

// elements of the physical ring of a scope of `cap` samples (the host computes the same: og_scope_host.h)
constexpr uint32_t scope_ring_len(uint32_t cap)
{
    return (cap * 2u + OG_BUS_CHUNK - 1u) / OG_BUS_CHUNK * OG_BUS_CHUNK + OG_BUS_CHUNK;
}

constexpr uint32_t SCOPE_COPY_BATCH = 16u; // loads in flight per lane while a window is copied (scope_chunk_begin)

template <uint32_t CAP>
struct Scope {
    static_assert(CAP >= 1u, "a scope holds at least one sample");
    static constexpr uint32_t P = scope_ring_len(CAP);
    narr_word* ring;   // element 0 of this lane's voice in the physical ring
    narr_word* frozen; // ... in the frozen window
    uint32_t stride;   // words between elements: n_voices
    bool valid;        // the lane holds a voice
};

// once per launch.  `ring_base`, `frozen_base`: first planes, in words per voice.  A loaded state image cannot point past
// the planes: the positions are brought into range here and nothing else ever moves them out of it.
template <uint32_t CAP>
OG_DEV Scope<CAP> scope_begin(narr_word* pool, uint32_t ring_base, uint32_t frozen_base, uint32_t n_voices, uint32_t v, bool valid, uint32_t& write_pos,
                              uint32_t& window_end, uint32_t& triggered_length)
{
    Scope<CAP> S;
    const uint32_t col = valid ? v : 0u;
    S.ring = pool + ((size_t)ring_base * n_voices + col);
    S.frozen = pool + ((size_t)frozen_base * n_voices + col);
    S.stride = n_voices;
    S.valid = valid;
    write_pos = write_pos < Scope<CAP>::P ? write_pos : 0u;
    window_end = window_end < Scope<CAP>::P ? window_end : 0u;
    triggered_length = triggered_length < CAP ? triggered_length : CAP;
    return S;
}

// top of a chunk: resolve the pending window if this chunk's pushes would reach it
template <uint32_t CAP>
OG_DEV void scope_chunk_begin(const Scope<CAP>& S, uint32_t write_pos, uint32_t window_end, uint32_t triggered_length, uint32_t& pending, uint32_t& copies)
{
    constexpr uint32_t P = Scope<CAP>::P;
    if (!S.valid || pending == 0u) return;
    const uint32_t d = write_pos >= window_end ? write_pos - window_end : write_pos + P - window_end;
    if (d + OG_BUS_CHUNK <= P - triggered_length) return; // (triggered_length <= CAP <= P - OG_BUS_CHUNK)
    uint32_t src = window_end >= triggered_length ? window_end - triggered_length : window_end + P - triggered_length;
    // A lane's elements lie n_voices words apart: every load is a cache line of its own and a load-then-store loop would
    // wait out one memory latency per element.  So SCOPE_COPY_BATCH independent loads are issued before their stores (the
    // two runs of planes never overlap).
    uint32_t j = 0;
    for (; j + SCOPE_COPY_BATCH <= triggered_length; j += SCOPE_COPY_BATCH) {
        uint32_t t[SCOPE_COPY_BATCH];
#pragma unroll
        for (uint32_t k = 0; k < SCOPE_COPY_BATCH; ++k) {
            const uint32_t q = src + k;
            t[k] = S.ring[(size_t)(q >= P ? q - P : q) * S.stride];
        }
#pragma unroll
        for (uint32_t k = 0; k < SCOPE_COPY_BATCH; ++k) S.frozen[(size_t)(j + k) * S.stride] = t[k];
        src = src + SCOPE_COPY_BATCH >= P ? src + SCOPE_COPY_BATCH - P : src + SCOPE_COPY_BATCH;
    }
    for (; j < triggered_length; ++j) {
        S.frozen[(size_t)j * S.stride] = S.ring[(size_t)src * S.stride];
        src = src + 1u == P ? 0u : src + 1u;
    }
    pending = 0u;
    copies += 1u;
}

template <bool AUTO, uint32_t CAP>
OG_DEV float scope_tick(const Scope<CAP>& S, float input, float trigger_period, float trigger_enabled, uint32_t& write_pos, uint32_t& written,
                        float& last_sample, uint32_t& period_sample_count, uint32_t& detected_period, uint32_t& triggered_length,
                        uint32_t& window_end, uint32_t& pending)
{
    constexpr uint32_t P = Scope<CAP>::P;
    if (S.valid) S.ring[(size_t)write_pos * S.stride] = __float_as_uint(input); // push(), :51-65
    write_pos = write_pos + 1u == P ? 0u : write_pos + 1u;
    written = written < CAP ? written + 1u : CAP;
    if (trigger_enabled > 0.5f) { // :249
        const bool crossing = last_sample <= 0.0f && input > 0.0f; // :251
        uint32_t length = 0u;
        if (AUTO) {
            period_sample_count = period_sample_count == 0xFFFFFFFFu ? period_sample_count : period_sample_count + 1u; // :255 (saturating)
            if (crossing) {
                if (period_sample_count > 1u) { // :259-263
                    const uint32_t m = period_sample_count < CAP ? period_sample_count : CAP;
                    detected_period = m > 10u ? m : 10u;
                }
                length = detected_period; // :266-268 (never 0: it starts at the capacity)
                period_sample_count = 0u; // :271
            }
        } else if (crossing) { // :275-281
            const float period = trigger_period > 1.0f ? trigger_period : 1.0f; // f32::max: a NaN gives 1.0
            const float r = roundf(period);                                      // half away from zero
            length = r >= (float)CAP ? CAP : (uint32_t)r;                        // `as usize` saturates; min(capacity) follows
        }
        if (crossing) { // store_triggered(length), :111-123 -- recorded, not copied
            length = length < CAP ? length : CAP;
            triggered_length = length > 1u ? length : 1u;
            window_end = write_pos;
            pending = 1u;
        }
    }
    last_sample = input; // :285
    return input;        // :246
}

} // namespace og
