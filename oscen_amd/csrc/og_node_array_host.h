// og_node_array_host.h -- host side of the array fields of registered node types (device side: og_node_array.hip.h): the copy
// og_register_node takes of a description, the look-up of a field by its path, the transposition between a caller's
// [voice][element] rows and the pool's [element][voice slot] planes, and the snapshot section.  Host-only and free of the
// HIP runtime, so that tests/standalone/node_array_main.cpp runs it under the sanitizers.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/oscen_gpu.h"
#include "og_graph.h"

namespace ognarr {

using Field = ogc::CompiledGraph::ArraySpec;

// og_register_node: the array descriptions of a type, copied (the caller's strings need not outlive the call).  What
// depends on one entry alone is checked by ogc::register_user_node; here only what cannot be copied.
inline void copy_arrays(const og_node_array* arrays, uint32_t n, std::vector<ogc::UserArray>& out)
{
    if (n && !arrays) throw std::runtime_error("n_arrays > 0 with arrays == NULL");
    if (n > OG_NODE_ARRAYS_MAX) throw std::runtime_error("at most " + std::to_string(OG_NODE_ARRAYS_MAX) + " array fields per node type");
    for (uint32_t i = 0; i < n; ++i) {
        const og_node_array& a = arrays[i];
        if (!a.name) throw std::runtime_error("bad array field description");
        ogc::UserArray u;
        u.name = a.name;
        u.length = a.length;
        u.is_uint = a.is_uint != 0;
        u.init_f = a.init;
        u.init_u = a.init_uint;
        out.push_back(u);
    }
}

// the reference's spelling -> the names of the flattened graph, as og_read_state_field: `combs[1].buf` -> `combs__1.buf`,
// `inner.comb.buf` -> `inner_comb.buf` (the last dot separates node and field)
inline std::string flat_path(const char* path)
{
    std::string p;
    for (const char* c = path; *c; ++c) {
        if (*c == '[') p += "__";
        else if (*c != ']' && !isspace((unsigned char)*c)) p.push_back(*c);
    }
    const size_t last = p.rfind('.');
    for (size_t k = 0; k < p.size(); ++k)
        if (p[k] == '.' && k != last) p[k] = '_';
    return p;
}
inline int find_field(const std::vector<Field>& fields, const char* path)
{
    const std::string p = flat_path(path);
    for (size_t k = 0; k < fields.size(); ++k)
        if (fields[k].path == p) return (int)k;
    return -1;
}

inline uint64_t words_per_voice(const std::vector<Field>& fields)
{
    return fields.empty() ? 0u : (uint64_t)fields.back().base + fields.back().length;
}
inline uint64_t pool_bytes(const std::vector<Field>& fields, uint32_t n_voices) { return words_per_voice(fields) * n_voices * 4u; }

// rows[count][length] of voices first .. <-> planes[length][n_voices] of one field; slot_of: logical voice -> slot (null: identity)
inline void scatter_rows(const Field& f, uint32_t n_voices, const uint32_t* slot_of, uint32_t first, uint32_t count, const uint32_t* rows, uint32_t* planes)
{
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t s = slot_of ? slot_of[first + k] : first + k;
        for (uint32_t i = 0; i < f.length; ++i) planes[(size_t)i * n_voices + s] = rows[(size_t)k * f.length + i];
    }
}
inline void gather_rows(const Field& f, uint32_t n_voices, const uint32_t* slot_of, uint32_t first, uint32_t count, const uint32_t* planes, uint32_t* rows)
{
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t s = slot_of ? slot_of[first + k] : first + k;
        for (uint32_t i = 0; i < f.length; ++i) rows[(size_t)k * f.length + i] = planes[(size_t)i * n_voices + s];
    }
}

// ---- snapshot section: {magic, n_fields}, n_fields lengths (bit 31: u32 elements), then the pool as it lies on the device --
constexpr uint32_t SNAP_NARR_MAGIC = 0x52414E4Fu; // "ONAR"
inline size_t section_head_bytes(const std::vector<Field>& fields) { return fields.empty() ? 0 : (2 + fields.size()) * sizeof(uint32_t); }
inline uint32_t length_word(const Field& f) { return f.length | (f.is_uint ? 0x80000000u : 0u); }
inline void write_section_head(const std::vector<Field>& fields, void* dst)
{
    if (fields.empty()) return;
    std::vector<uint32_t> w;
    w.push_back(SNAP_NARR_MAGIC);
    w.push_back((uint32_t)fields.size());
    for (const Field& f : fields) w.push_back(length_word(f));
    memcpy(dst, w.data(), w.size() * sizeof(uint32_t));
}
// "" when the `avail` bytes at p start with the head of exactly these fields; otherwise what is wrong (nothing is read past avail)
inline std::string check_section_head(const std::vector<Field>& fields, const void* p, size_t avail)
{
    if (fields.empty()) return std::string();
    uint32_t h[2];
    if (avail < sizeof h) return "state blob: the node-array section is missing";
    memcpy(h, p, sizeof h);
    if (h[0] != SNAP_NARR_MAGIC) return "state blob: the node-array section is missing or malformed";
    if (h[1] != fields.size())
        return "state blob: it holds " + std::to_string(h[1]) + " node-array fields, this graph has " + std::to_string(fields.size());
    if ((avail - sizeof h) / sizeof(uint32_t) < fields.size()) return "state blob: the node-array section is truncated";
    for (size_t k = 0; k < fields.size(); ++k) {
        uint32_t w;
        memcpy(&w, (const char*)p + sizeof h + k * sizeof w, sizeof w);
        if (w != length_word(fields[k]))
            return "state blob: node-array field '" + fields[k].path + "' has " + std::to_string(fields[k].length) + " elements here, " +
                   std::to_string(w & 0x7FFFFFFFu) + " in the blob (or another element type)";
    }
    return std::string();
}

} // namespace ognarr
