// tests/standalone/asset_load_main.cpp -- TEST INFRASTRUCTURE, never part of the product and never linked into the library.
//
// A stand-alone program around the two host-side pieces of the sample load path, for runs under sanitizers (it has its own
// main, so it needs nothing preloaded) and for one orientation number:
//
//   asset_load_main wav            feeds ogwav::decode (csrc/og_wav.cpp) well-formed and malformed file images -- truncated at
//                                  every length, chunk sizes past the end, odd formats -- and prints what each one gave
//   asset_load_main time [seconds] the resample of csrc/og_asset_resample.hip.h, lane by lane on ONE host thread (the header
//                                  compiled against the host simulator's stand-in for the HIP runtime): seconds of stereo
//                                  44 100 -> 48 000, wall time.  For orientation only: the library has no CPU path.
//
//   clang++ -std=c++17 -O2 -ffp-contract=off -mfma -fsanitize=address,undefined -Itests/hostsim -Ioscen_amd/csrc \
//       tests/standalone/asset_load_main.cpp oscen_amd/csrc/og_wav.cpp -o asset_load_main
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "og_asset_resample.hip.h"
#include "og_wav.h"
#include "../../include/oscen_gpu.h"
#include "og_abi.h"

// what og_wav.cpp takes from og_engine.cpp
static std::string g_last;
int ogabi::set_error(int code, const std::string& m)
{
    g_last = m;
    return code;
}
int ogabi::set_error(int code, const char* m) noexcept
{
    g_last = m;
    return code;
}
extern "C" int og_register_sample_at_rate(const char*, const float*, uint64_t, uint32_t, uint32_t) { return OG_OK; }

namespace {
void u16(std::vector<uint8_t>& b, unsigned v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
void u32(std::vector<uint8_t>& b, unsigned v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); }
void tag(std::vector<uint8_t>& b, const char* t) { b.insert(b.end(), t, t + 4); }

std::vector<uint8_t> wav(unsigned fmt, unsigned channels, unsigned rate, unsigned bits, unsigned data_bytes, bool extensible = false,
                         long junk_size = -1)
{
    std::vector<uint8_t> b;
    tag(b, "RIFF");
    u32(b, 0);
    tag(b, "WAVE");
    if (junk_size >= 0) { // an unknown chunk in front of fmt: 6 bytes present, `junk_size` declared
        tag(b, "LIST");
        u32(b, (unsigned)junk_size);
        for (int i = 0; i < 6; ++i) b.push_back(0x55);
    }
    tag(b, "fmt ");
    u32(b, extensible ? 40 : 16);
    u16(b, extensible ? 0xFFFE : fmt);
    u16(b, channels);
    u32(b, rate);
    u32(b, rate * channels * bits / 8);
    u16(b, channels * bits / 8);
    u16(b, bits);
    if (extensible) {
        u16(b, 22);
        u16(b, bits);
        u32(b, 3);
        u16(b, fmt);
        for (int i = 0; i < 14; ++i) b.push_back((uint8_t)i);
    }
    tag(b, "data");
    u32(b, data_bytes);
    for (unsigned i = 0; i < data_bytes; ++i) b.push_back((uint8_t)(i * 37 + 11));
    return b;
}

int feed(const char* what, const std::vector<uint8_t>& image, size_t n)
{
    // an exact-size heap copy: a read past the image's end is a heap overflow the sanitizer sees
    uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
    memcpy(copy, image.data(), n);
    ogwav::Decoded d;
    std::string why;
    const int rc = ogwav::decode(copy, n, d, why);
    free(copy);
    if (what) printf("%-44s rc %2d  frames %4llu  channels %u  rate %u  %s\n", what, rc, (unsigned long long)d.frames, d.channels, d.sample_rate, why.c_str());
    return rc;
}

int wav_cases()
{
    int bad = 0;
    const auto pcm16 = wav(1, 2, 44100, 16, 16), pcm24 = wav(1, 1, 48000, 24, 9), pcm32 = wav(1, 1, 8000, 32, 8), flt = wav(3, 2, 96000, 32, 16);
    const auto ext16 = wav(1, 2, 44100, 16, 8, true), extf = wav(3, 1, 22050, 32, 8, true);
    bad += feed("PCM 16 stereo", pcm16, pcm16.size()) != OG_OK;
    bad += feed("PCM 24 mono", pcm24, pcm24.size()) != OG_OK;
    bad += feed("PCM 32 mono", pcm32, pcm32.size()) != OG_OK;
    bad += feed("float 32 stereo", flt, flt.size()) != OG_OK;
    bad += feed("extensible PCM 16", ext16, ext16.size()) != OG_OK;
    bad += feed("extensible float 32", extf, extf.size()) != OG_OK;
    bad += feed("unknown chunk, odd size, in front of fmt", wav(1, 1, 44100, 16, 4, false, 5), 12 + 8 + 6 + 24 + 8 + 4) != OG_OK;
    bad += feed("8-bit PCM", wav(1, 1, 8000, 8, 4), 48) != OG_E_UNSUPPORTED;
    bad += feed("ADPCM tag", wav(2, 1, 8000, 4, 4), 48) != OG_E_UNSUPPORTED;
    bad += feed("unknown chunk declaring 4 GiB", wav(1, 1, 44100, 16, 4, false, 0xFFFFFFFFl), 12 + 8 + 6 + 24 + 8 + 4) != OG_E_INVALID;
    bad += feed("unknown chunk declaring 1 byte too many", wav(1, 1, 44100, 16, 0, false, 6 + 24 + 8 + 1), 12 + 8 + 6 + 24 + 8) != OG_E_INVALID;
    auto big = pcm16;
    big[40] = 0xFF; // the data chunk declares more than is there
    bad += feed("data chunk declaring 255 bytes of 16", big, big.size()) != OG_E_INVALID;
    bad += feed("block alignment that does not match", [] { auto b = wav(1, 2, 44100, 16, 8); b[32] = 3; return b; }(), 52) != OG_E_INVALID;
    bad += feed("half a frame of data", wav(1, 2, 44100, 16, 6), 50) != OG_E_INVALID;
    bad += feed("not RIFF", std::vector<uint8_t>(64, 0x41), 64) != OG_E_INVALID;
    // every truncation of every well-formed image: never OK with more frames than the bytes can hold, never a read past the end
    size_t n_trunc = 0;
    for (const auto* img : {&pcm16, &pcm24, &pcm32, &flt, &ext16, &extf})
        for (size_t n = 0; n < img->size(); ++n, ++n_trunc) bad += feed(nullptr, *img, n) != OG_E_INVALID;
    printf("%zu truncated images: every one refused with OG_E_INVALID\n", n_trunc);
    // every single-byte corruption of a header: any answer is fine, no read past the end is the point
    size_t n_flip = 0;
    for (size_t at = 0; at < 44; ++at)
        for (unsigned v : {0u, 1u, 0x7Fu, 0x80u, 0xFFu}) {
            auto b = ext16;
            b[at] = (uint8_t)v;
            (void)feed(nullptr, b, b.size());
            ++n_flip;
        }
    printf("%zu corrupted headers decoded without a fault\n", n_flip);
    printf("%s\n", bad ? "FAILED" : "all WAV cases as expected");
    return bad ? 1 : 0;
}

int time_host(double seconds)
{
    const uint32_t src_rate = 44100, dst_rate = 48000, ch = 2;
    const uint64_t frames = (uint64_t)(seconds * src_rate);
    std::vector<float> in(frames * ch);
    uint64_t s = 0x2545F4914F6CDD1Dull;
    for (float& x : in) {
        s = s * 6364136223846793005ull + 1;
        x = (float)(s >> 33) / 2147483648.0f - 1.0f;
    }
    const OgResamplePlan p = og_resample_plan(frames, src_rate, dst_rate);
    std::vector<float> out(p.out_len * ch);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t n = 0; n < p.out_len; ++n) og_resample_frame<2>(in.data(), frames, ch, n, p.inv_ratio, p.cutoff, p.radius, p.inv_radius, out.data());
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double sum = 0.0;
    for (float x : out) sum += x;
    printf("host restatement, one thread: %.1f s stereo %u -> %u, %llu -> %llu frames: %.3f s (checksum %.6f)\n", seconds, src_rate, dst_rate,
           (unsigned long long)frames, (unsigned long long)p.out_len, dt, sum);
    return 0;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "wav")) return wav_cases();
    if (argc >= 2 && !strcmp(argv[1], "time")) return time_host(argc >= 3 ? atof(argv[2]) : 60.0);
    fprintf(stderr, "usage: %s wav | time [seconds]\n", argv[0]);
    return 2;
}
