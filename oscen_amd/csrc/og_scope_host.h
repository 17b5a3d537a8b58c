// og_scope_host.h -- host side of the Oscilloscope (device side: og_scope.hip.h): what a read has to reconstruct.  The device
// keeps a PHYSICAL ring of ring_len(capacity) samples per voice and defers the copy of a triggered window, so the two results
// of the reference's snapshot(sample_count) (oscen-lib/src/oscilloscope/mod.rs:67-109) are put together here, from the planes
// and the state words of one voice -- whether the window is still pending in the ring or already lies in the frozen planes.
// Host-only and free of the HIP runtime, so that tests/standalone/scope_main.cpp runs it under the sanitizers.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace ogscope {

constexpr uint32_t CHUNK = 16u;          // OG_BUS_CHUNK (og_kernel_rt.hip.h)
constexpr uint32_t MAX_CAPACITY = 65536u; // the node-array field limit (OG_NODE_ARRAY_MAX_LEN)

// elements of the physical ring: 2 x capacity rounded up to a multiple of CHUNK, and one CHUNK more -- a pending window then
// survives at least `capacity` pushes (the deadline rule of og_scope.hip.h needs capacity + CHUNK); og::scope_ring_len
constexpr uint32_t ring_len(uint32_t cap)
{
    return (cap * 2u + CHUNK - 1u) / CHUNK * CHUNK + CHUNK;
}

// the state words a read needs, of one voice
struct Words {
    uint32_t write_pos = 0;        // where the next push lands in the physical ring
    uint32_t written = 0;          // pushes so far, saturating at the capacity
    uint32_t triggered_length = 0; // 0: no window
    uint32_t window_end = 0;       // one past the window's last sample in the physical ring (while pending)
    uint32_t pending = 0;          // the window still lies in the ring
};

// element i of a voice's column: planes are [element][n_voices]
struct Column {
    const float* p = nullptr;
    size_t stride = 1;
    float operator[](uint32_t i) const { return p[(size_t)i * stride]; }
};

// the `count` samples that end in front of physical position `end`, in time order
inline void last_samples(const Column& ring, uint32_t P, uint32_t end, uint32_t count, float* out)
{
    uint32_t src = (end % P + P - count % P) % P;
    for (uint32_t j = 0; j < count; ++j) {
        out[j] = ring[src];
        src = src + 1u == P ? 0u : src + 1u;
    }
}

// snapshot(sample_count): samples[0..*n_samples) = the last clamp(sample_count, 1, available) samples, triggered[0..*n_triggered)
// = the frozen window; both empty while nothing was pushed (mod.rs:73-78).  `samples` holds max(sample_count, 1) floats or is
// null, `triggered` holds `capacity` floats or is null; the counts may be null as well.
inline void snapshot(uint32_t capacity, const Column& ring, const Column& frozen, const Words& w, uint32_t sample_count, float* samples, uint32_t* n_samples,
                     float* triggered, uint32_t* n_triggered)
{
    const uint32_t P = ring_len(capacity);
    const uint32_t available = w.written < capacity ? w.written : capacity;
    uint32_t ns = 0, nt = 0;
    if (available) {
        ns = sample_count < 1u ? 1u : sample_count;
        ns = ns < available ? ns : available;
        if (samples) last_samples(ring, P, w.write_pos, ns, samples);
        nt = w.triggered_length < capacity ? w.triggered_length : capacity;
        if (triggered && nt) {
            if (w.pending) last_samples(ring, P, w.window_end, nt, triggered);
            else
                for (uint32_t j = 0; j < nt; ++j) triggered[j] = frozen[j];
        }
    }
    if (n_samples) *n_samples = ns;
    if (n_triggered) *n_triggered = nt;
}

// the reference's spelling of a node -> its name in the flattened graph, as og_read_state_field: `scopes[1]` -> `scopes__1`,
// `inner.scope` -> `inner_scope`
inline std::string flat_node(const char* path)
{
    std::string p;
    for (const char* c = path; *c; ++c) {
        if (*c == '[') p += "__";
        else if (*c == '.') p.push_back('_');
        else if (*c != ']' && !isspace((unsigned char)*c)) p.push_back(*c);
    }
    return p;
}

// `OscilloscopeHandle::new(<integer literal>)`, the reference's spelling of a handle in the text front end: the capacity, or
// -1 for any other expression
inline long long handle_capacity(const std::string& raw)
{
    std::string t;
    for (char ch : raw)
        if (!isspace((unsigned char)ch)) t.push_back(ch);
    const std::string head = "OscilloscopeHandle::new(";
    if (t.size() < head.size() + 2 || t.compare(0, head.size(), head) != 0 || t.back() != ')') return -1;
    std::string num = t.substr(head.size(), t.size() - head.size() - 1);
    std::string digits;
    for (char ch : num)
        if (ch != '_') digits.push_back(ch);
    if (digits.size() > 5 && digits.compare(digits.size() - 5, 5, "usize") == 0) digits.resize(digits.size() - 5);
    if (digits.empty() || digits.size() > 12) return -1;
    for (char ch : digits)
        if (!isdigit((unsigned char)ch)) return -1;
    return atoll(digits.c_str());
}

} // namespace ogscope
