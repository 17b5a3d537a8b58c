// og_wav.cpp -- the output step immediately downstream of the path: interleaved bus -> RIFF/WAVE
// file (the reference examples use the `hound` crate for this: 16-bit PCM or 32-bit IEEE float) -- and the input step in
// front of the sample registry: a RIFF/WAVE file -> interleaved f32 at the file's own rate (AudioAsset::from_wav,
// oscen-lib/src/asset/mod.rs:138-155).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/oscen_gpu.h"
#include "og_abi.h"
#include "og_wav.h"

namespace {
void put_u32(std::vector<uint8_t>& b, uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); }
void put_u16(std::vector<uint8_t>& b, uint16_t v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
uint32_t get_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t get_u16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
} // namespace

// The file image `b` (n bytes) -> interleaved f32.  Chunks are walked by their declared sizes, none of which is trusted past
// the end of the image: a chunk header that does not fit, a `fmt ` body that does, or a `data` chunk that claims more bytes
// than are there is a malformed file.  Integers are scaled by 1 / 2^(bits - 1) as from_wav does.
int ogwav::decode(const uint8_t* b, size_t n, Decoded& out, std::string& why)
{
    if (n < 12 || memcmp(b, "RIFF", 4) != 0 || memcmp(b + 8, "WAVE", 4) != 0) {
        why = "not a RIFF/WAVE file";
        return OG_E_INVALID;
    }
    bool have_fmt = false;
    uint16_t tag = 0, channels = 0, bits = 0, align = 0;
    uint32_t rate = 0;
    size_t at = 12;
    while (true) {
        if (n - at < 8) {
            why = have_fmt ? "no data chunk before the end of the file" : "no fmt chunk before the end of the file";
            return OG_E_INVALID;
        }
        const uint8_t* id = b + at;
        const size_t size = get_u32(b + at + 4);
        at += 8;
        if (memcmp(id, "fmt ", 4) == 0) {
            if (size < 16 || size > n - at) {
                why = "the fmt chunk is truncated";
                return OG_E_INVALID;
            }
            tag = get_u16(b + at);
            channels = get_u16(b + at + 2);
            rate = get_u32(b + at + 4);
            align = get_u16(b + at + 12);
            bits = get_u16(b + at + 14);
            if (tag == 0xFFFE) { // WAVE_FORMAT_EXTENSIBLE: the format is the first two bytes of the SubFormat GUID
                if (size < 40) {
                    why = "the extensible fmt chunk is truncated";
                    return OG_E_INVALID;
                }
                tag = get_u16(b + at + 24);
            }
            have_fmt = true;
        } else if (memcmp(id, "data", 4) == 0) {
            if (!have_fmt) {
                why = "the data chunk comes before the fmt chunk";
                return OG_E_INVALID;
            }
            if (size > n - at) {
                why = "the data chunk declares " + std::to_string(size) + " bytes, the file has " + std::to_string(n - at) + " left";
                return OG_E_INVALID;
            }
            const bool is_float = tag == 3 && bits == 32;
            const bool is_int = tag == 1 && (bits == 16 || bits == 24 || bits == 32);
            if (!is_float && !is_int) {
                why = "format tag " + std::to_string(tag) + " with " + std::to_string(bits) + " bits per sample is not supported (PCM 16 / 24 / 32, IEEE float 32)";
                return OG_E_UNSUPPORTED;
            }
            const size_t bytes = bits / 8u;
            if (channels == 0 || align != channels * bytes) {
                why = "the fmt chunk's block alignment does not match its channels and bits per sample";
                return OG_E_INVALID;
            }
            if (size % align != 0) {
                why = "the data chunk does not hold whole frames";
                return OG_E_INVALID;
            }
            out.channels = channels;
            out.sample_rate = rate;
            out.frames = size / align;
            out.interleaved.resize(size / bytes);
            const uint8_t* p = b + at;
            const float scale = 1.0f / (float)((int64_t)1 << (bits - 1));
            for (size_t i = 0; i < out.interleaved.size(); ++i, p += bytes) {
                if (is_float) {
                    const uint32_t u = get_u32(p);
                    memcpy(&out.interleaved[i], &u, 4);
                } else {
                    int32_t v;
                    if (bits == 16) v = (int16_t)get_u16(p);
                    else if (bits == 24) v = (int32_t)(((uint32_t)p[0] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 24)) >> 8;
                    else v = (int32_t)get_u32(p);
                    out.interleaved[i] = (float)v * scale;
                }
            }
            return OG_OK;
        } else if (size > n - at) {
            why = "chunk '" + std::string((const char*)id, 4) + "' declares " + std::to_string(size) + " bytes, the file has " + std::to_string(n - at) + " left";
            return OG_E_INVALID;
        }
        at += size;
        if ((size & 1) && at < n) at += 1; // chunks are word-aligned
    }
}

int ogwav::read(const char* path, Decoded& out, std::string& why)
{
    FILE* f = fopen(path, "rb");
    if (!f) {
        why = std::string("cannot open '") + path + "'";
        return OG_E_INVALID;
    }
    std::vector<uint8_t> b;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) {
        why = std::string("error reading '") + path + "'";
        return OG_E_INVALID;
    }
    return decode(b.data(), b.size(), out, why);
}

extern "C" {
int og_register_sample_wav(const char* name, const char* path)
{
    return ogabi::guard([&]() -> int {
    if (!name || !*name || !path) return ogabi::set_error(OG_E_INVALID, "og_register_sample_wav: a sample needs a name and a path");
    ogwav::Decoded d;
    std::string why;
    const int rc = ogwav::read(path, d, why);
    if (rc != OG_OK) return ogabi::set_error(rc, "og_register_sample_wav: '" + std::string(path) + "': " + why);
    return og_register_sample_at_rate(name, d.interleaved.data(), d.frames, d.channels, d.sample_rate);
    });
}

int og_register_ir_wav(const char* name, const char* path)
{
    return ogabi::guard([&]() -> int {
    if (!name || !*name || !path) return ogabi::set_error(OG_E_INVALID, "og_register_ir_wav: a response needs a name and a path");
    ogwav::Decoded d;
    std::string why;
    const int rc = ogwav::read(path, d, why);
    if (rc != OG_OK) return ogabi::set_error(rc, "og_register_ir_wav: '" + std::string(path) + "': " + why);
    return og_register_ir_asset(name, d.interleaved.data(), d.frames, d.channels, d.sample_rate);
    });
}

int og_write_wav(const char* path, const float* interleaved, uint64_t frames, uint32_t channels,
                 uint32_t sample_rate, uint32_t bits_per_sample)
{
    return ogabi::guard([&]() -> int { // (the file image is assembled in a vector: bad_alloc -> OG_E_NOMEM)
    if (!path || (!interleaved && frames) || channels == 0 || (bits_per_sample != 16 && bits_per_sample != 32))
        return OG_E_INVALID;
    const bool f32 = bits_per_sample == 32;
    const uint64_t n = frames * channels;
    const uint64_t data_bytes = n * (bits_per_sample / 8);
    if (data_bytes > 0xFFFFFFFFull - 44) return OG_E_INVALID;
    std::vector<uint8_t> b;
    b.reserve(44 + (size_t)data_bytes);
    b.insert(b.end(), {'R', 'I', 'F', 'F'});
    put_u32(b, (uint32_t)(36 + data_bytes));
    b.insert(b.end(), {'W', 'A', 'V', 'E', 'f', 'm', 't', ' '});
    put_u32(b, 16);
    put_u16(b, f32 ? 3 : 1); // WAVE_FORMAT_IEEE_FLOAT / WAVE_FORMAT_PCM
    put_u16(b, (uint16_t)channels);
    put_u32(b, sample_rate);
    put_u32(b, sample_rate * channels * (bits_per_sample / 8));
    put_u16(b, (uint16_t)(channels * (bits_per_sample / 8)));
    put_u16(b, (uint16_t)bits_per_sample);
    b.insert(b.end(), {'d', 'a', 't', 'a'});
    put_u32(b, (uint32_t)data_bytes);
    for (uint64_t i = 0; i < n; ++i) {
        const float x = interleaved[i];
        if (f32) {
            uint32_t u;
            memcpy(&u, &x, 4);
            put_u32(b, u);
        } else {
            float c = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
            if (c != c) c = 0.0f;
            put_u16(b, (uint16_t)(int16_t)lrintf(c * 32767.0f));
        }
    }
    FILE* f = fopen(path, "wb");
    if (!f) return OG_E_INVALID;
    const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
    fclose(f);
    return ok ? OG_OK : OG_E_INVALID;
    });
}
} // extern "C"
