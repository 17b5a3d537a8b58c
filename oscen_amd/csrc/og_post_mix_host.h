// og_post_mix_host.h -- host-only bookkeeping of a post-mix graph's snapshot section (no HIP: tests/standalone builds it
// with a plain C++ compiler under sanitizers).  The partition itself is og_graph.h's split_post_mix().
//
// Section (the LAST of a blob, and only in blobs of graphs that have a post-mix graph -- every other blob is what it was):
//   head    magic "OGPM", version, state words, rings, the rings' capacities, a digest of the state words' names
//   words   the post-mix state image: one 32-bit word per state word (one voice)
//   rings   the Delay lines back to back, [capacity][1] floats each
// og_load_state checks the head against the engine's own post-mix graph before it changes anything.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ogpm {

constexpr uint32_t SECTION_MAGIC = 0x4D50474Fu; // "OGPM"
constexpr uint32_t SECTION_VERSION = 1u;
constexpr uint32_t MAX_RINGS = 4u; // (OG_MAX_RINGS)

struct SectionHead {
    uint32_t magic, version;
    uint32_t state_words, n_rings;
    uint32_t ring_cap[MAX_RINGS];
    uint64_t names_digest; // FNV-1a of the state words' names, '\n'-separated: the same node fields in the same order
};

// what an engine expects of (and writes into) the section
struct Layout {
    std::vector<std::string> state_names;
    std::vector<uint32_t> ring_caps;
};

inline uint64_t names_digest(const std::vector<std::string>& names)
{
    uint64_t h = 1469598103934665603ull;
    for (const std::string& n : names) {
        for (unsigned char ch : n) h = (h ^ ch) * 1099511628211ull;
        h = (h ^ (unsigned char)'\n') * 1099511628211ull;
    }
    return h;
}
inline uint64_t ring_words(const Layout& l)
{
    uint64_t n = 0;
    for (uint32_t c : l.ring_caps) n += c;
    return n;
}
inline size_t section_bytes(const Layout& l) { return sizeof(SectionHead) + (size_t)(l.state_names.size() + ring_words(l)) * 4; }

inline SectionHead make_head(const Layout& l)
{
    SectionHead h;
    memset(&h, 0, sizeof h);
    h.magic = SECTION_MAGIC;
    h.version = SECTION_VERSION;
    h.state_words = (uint32_t)l.state_names.size();
    h.n_rings = (uint32_t)l.ring_caps.size();
    for (size_t k = 0; k < l.ring_caps.size() && k < MAX_RINGS; ++k) h.ring_cap[k] = l.ring_caps[k];
    h.names_digest = names_digest(l.state_names);
    return h;
}

// the section from its parts; `rings` holds the lines back to back
inline std::vector<char> encode(const Layout& l, const uint32_t* words, const float* rings)
{
    std::vector<char> out(section_bytes(l));
    const SectionHead h = make_head(l);
    memcpy(out.data(), &h, sizeof h);
    const size_t nw = l.state_names.size() * 4, nr = (size_t)ring_words(l) * 4;
    if (nw) memcpy(out.data() + sizeof h, words, nw);
    if (nr) memcpy(out.data() + sizeof h + nw, rings, nr);
    return out;
}

// "" when the `len` bytes at `src` are this layout's section, else why not.  Reads nothing beyond `len`.
inline std::string check(const Layout& l, const void* src, size_t len)
{
    if (l.ring_caps.size() > MAX_RINGS) return "state blob: the post-mix graph has more delay lines than a section holds";
    SectionHead h;
    if (!src || len < sizeof h) return "state blob: the post-mix graph's section is missing (the blob is from a graph without one, or cut short)";
    memcpy(&h, src, sizeof h);
    if (h.magic != SECTION_MAGIC) return "state blob: the post-mix graph's section is missing or malformed (bad magic)";
    if (h.version != SECTION_VERSION) return "state blob: the post-mix graph's section has version " + std::to_string(h.version) + ", this build reads " + std::to_string(SECTION_VERSION);
    if (h.state_words != l.state_names.size() || h.names_digest != names_digest(l.state_names))
        return "state blob: the post-mix graph's section was saved by another post-mix graph (" + std::to_string(h.state_words) + " state words, this one has " +
               std::to_string(l.state_names.size()) + ", or other node fields)";
    if (h.n_rings != l.ring_caps.size()) return "state blob: the post-mix graph's section holds " + std::to_string(h.n_rings) + " delay lines, this graph has " + std::to_string(l.ring_caps.size());
    for (size_t k = 0; k < l.ring_caps.size(); ++k)
        if (h.ring_cap[k] != l.ring_caps[k])
            return "state blob: delay line " + std::to_string(k) + " of the post-mix graph was saved with " + std::to_string(h.ring_cap[k]) + " samples, this engine's has " +
                   std::to_string(l.ring_caps[k]) + " (another sample rate)";
    if (len != section_bytes(l)) return "state blob: the post-mix graph's section has " + std::to_string(len) + " bytes, " + std::to_string(section_bytes(l)) + " expected";
    return std::string();
}

// where the parts of a checked section start, in bytes (a blob's section need not be aligned: copy, do not cast)
inline size_t words_offset() { return sizeof(SectionHead); }
inline size_t rings_offset(const Layout& l) { return sizeof(SectionHead) + l.state_names.size() * 4; }
inline void decode(const Layout& l, const void* src, std::vector<uint32_t>& words, std::vector<float>& rings)
{
    words.resize(l.state_names.size());
    rings.resize((size_t)ring_words(l));
    if (!words.empty()) memcpy(words.data(), (const char*)src + words_offset(), words.size() * 4);
    if (!rings.empty()) memcpy(rings.data(), (const char*)src + rings_offset(l), rings.size() * 4);
}

} // namespace ogpm
