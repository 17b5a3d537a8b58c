// og_wav.h -- the RIFF/WAVE reader of og_wav.cpp (og_register_sample_wav), on its own so that a stand-alone program can feed
// it malformed files.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ogwav {
struct Decoded {
    std::vector<float> interleaved;
    uint64_t frames = 0;
    uint32_t channels = 0, sample_rate = 0;
};
// OG_OK, OG_E_UNSUPPORTED (a format other than PCM 16 / 24 / 32 and IEEE float 32, plain or WAVE_FORMAT_EXTENSIBLE) or
// OG_E_INVALID (malformed, truncated, unreadable), with the reason in `why`
int decode(const uint8_t* image, size_t n, Decoded& out, std::string& why);
int read(const char* path, Decoded& out, std::string& why);
} // namespace ogwav
