// tests/standalone/ir_asset_main.cpp -- TEST INFRASTRUCTURE, never part of the product and never linked into the library.
//
// A stand-alone program around the host-side pieces of the asset impulse-response path, for runs under sanitizers (it has its
// own main, so it needs nothing preloaded): the registry of csrc/og_graph.cpp (both forms under one name space), the RIFF
// reader in front of it (og_register_ir_wav, csrc/og_wav.cpp) and the channel mapping of csrc/og_bus_conv.hip.h
// (og_bus_ir_tap, compiled against the host simulator's stand-in for the HIP runtime), every buffer an exact-size heap
// allocation so that an access past an end is one the sanitizer sees.  tests/test_ir_assets_cpu.py builds and runs it:
//
//   clang++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Itests/hostsim -Ioscen_amd/csrc tests/standalone/ir_asset_main.cpp oscen_amd/csrc/og_wav.cpp \
//       oscen_amd/csrc/og_graph.cpp oscen_amd/csrc/og_builtin.cpp -o ir_asset_main && ./ir_asset_main <scratch directory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "og_bus_conv.hip.h"
#include "og_graph.h"
#include "../../include/oscen_gpu.h"
#include "og_abi.h"

// what og_wav.cpp takes from og_engine.cpp: the error slot, and the two registrations it forwards to (the asset one is, as
// there, the guard around ogc::register_ir_asset, which holds every check on the data)
static std::string g_last;
int ogabi::set_error(int code, const std::string& m)
{
    g_last = m;
    return code;
}
int ogabi::set_error(int code, const char* m) noexcept
{
    g_last = m ? m : "";
    return code;
}
extern "C" int og_register_sample_at_rate(const char*, const float*, uint64_t, uint32_t, uint32_t) { return OG_OK; }
extern "C" int og_register_ir_asset(const char* name, const float* interleaved, uint64_t frames, uint32_t channels, uint32_t sample_rate)
{
    return ogabi::guard([&]() -> int {
        if (!name) return ogabi::set_error(OG_E_INVALID, "null argument");
        ogc::register_ir_asset(name, interleaved, frames, channels, sample_rate);
        return OG_OK;
    });
}

namespace {
int bad = 0;
void expect(bool ok, const char* what)
{
    printf("%-84s %s\n", what, ok ? "ok" : "FAILED");
    bad += ok ? 0 : 1;
}
template <class F>
bool throws(F&& f)
{
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

// an exact-size heap copy of n floats
float* heap(const std::vector<float>& v)
{
    float* p = (float*)malloc(v.size() ? v.size() * 4 : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * 4);
    return p;
}

std::vector<float> ramp(size_t n, float step)
{
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = 0.25f + step * (float)i;
    return v;
}

void registry_cases()
{
    const auto mono = ramp(5, 0.5f), st = ramp(12, 0.125f);
    float* pm = heap(mono);
    float* ps = heap(st);
    ogc::register_ir("rooms::hall", pm, mono.size());
    std::string resolved;
    ogc::IrEntry e = ogc::lookup_ir_entry("rooms::hall(48000.0)", &resolved);
    expect(e.taps && !e.asset && e.taps->size() == 5 && resolved == "rooms::hall", "a mono response is found by its call text");
    ogc::register_ir_asset("rooms::hall", ps, 6, 2, 44100); // the other form under the same name replaces it
    e = ogc::lookup_ir_entry("hall()");
    expect(!e.taps && e.asset && e.asset->frames == 6 && e.asset->channels == 2 && e.asset->rate == 44100 && e.asset->interleaved == st,
           "an asset registration replaces the mono one and is found by the last path segment");
    expect(!ogc::lookup_ir("rooms::hall"), "lookup_ir (Convolver::with_ir) does not see an asset");
    ogc::register_ir("rooms::hall", pm, 2);
    e = ogc::lookup_ir_entry("rooms::hall");
    expect(e.taps && !e.asset && e.taps->size() == 2, "... and the mono form replaces the asset");
    expect(throws([&] { ogc::register_ir_asset("no good", ps, 6, 2, 44100); }), "a name that is no path of identifiers is refused");
    expect(throws([&] { ogc::register_ir_asset("x", ps, 1, 0, 44100); }) && throws([&] { ogc::register_ir_asset("x", ps, 1, 9, 44100); }), "0 and 9 channels are refused");
    expect(throws([&] { ogc::register_ir_asset("x", ps, ((uint64_t)1 << 28) / 2 + 1, 2, 44100); }), "more than 2^28 samples are refused before they are read");
    expect(throws([&] { ogc::register_ir_asset("x", ps, 6, 2, 0); }) && throws([&] { ogc::register_ir_asset("x", ps, 0, 2, 44100); }) &&
               throws([&] { ogc::register_ir_asset("x", nullptr, 6, 2, 44100); }),
           "a zero rate, an empty response and null data are refused");
    expect(!ogc::lookup_ir_entry("x"), "... and none of these registered anything");
    for (uint32_t ch = 1; ch <= 8; ++ch) { // every width, the buffer exactly frames x channels
        const auto v = ramp(3 * ch, 1.0f);
        float* p = heap(v);
        ogc::register_ir_asset("wide", p, 3, ch, 8000);
        free(p);
        e = ogc::lookup_ir_entry("wide");
        if (!(e.asset && e.asset->channels == ch && e.asset->interleaved == v)) expect(false, "every width from 1 to 8 is copied whole");
    }
    expect(ogc::unregister_ir("wide") && ogc::unregister_ir("rooms::hall") && !ogc::unregister_ir("rooms::hall"), "unregister_ir removes either form, once");
    free(pm);
    free(ps);
}

void u16(std::vector<uint8_t>& b, unsigned v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
void u32(std::vector<uint8_t>& b, unsigned v) { for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i))); }
void tag(std::vector<uint8_t>& b, const char* t) { b.insert(b.end(), t, t + 4); }
std::vector<uint8_t> wav(unsigned fmt, unsigned channels, unsigned rate, unsigned bits, unsigned data_bytes)
{
    std::vector<uint8_t> b;
    tag(b, "RIFF");
    u32(b, 36 + data_bytes);
    tag(b, "WAVE");
    tag(b, "fmt ");
    u32(b, 16);
    u16(b, fmt);
    u16(b, channels);
    u32(b, rate);
    u32(b, rate * channels * bits / 8);
    u16(b, channels * bits / 8);
    u16(b, bits);
    tag(b, "data");
    u32(b, data_bytes);
    for (unsigned i = 0; i < data_bytes; ++i) b.push_back((uint8_t)(i * 37 + 11));
    return b;
}
int register_file(const std::string& dir, const char* name, const std::vector<uint8_t>& image, size_t n)
{
    const std::string path = dir + "/ir_asset_main.wav";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(image.data(), 1, n, f) != n) {
        fprintf(stderr, "cannot write %s\n", path.c_str());
        exit(2);
    }
    fclose(f);
    const int rc = og_register_ir_wav(name, path.c_str());
    remove(path.c_str());
    return rc;
}

void wav_cases(const std::string& dir)
{
    const auto pcm16 = wav(1, 2, 44100, 16, 24), pcm24 = wav(1, 3, 96000, 24, 27), flt = wav(3, 1, 22050, 32, 16);
    expect(register_file(dir, "w16", pcm16, pcm16.size()) == OG_OK && ogc::lookup_ir_entry("w16").asset &&
               ogc::lookup_ir_entry("w16").asset->frames == 6 && ogc::lookup_ir_entry("w16").asset->channels == 2 && ogc::lookup_ir_entry("w16").asset->rate == 44100,
           "PCM 16 stereo registers at the header's rate");
    expect(register_file(dir, "w24", pcm24, pcm24.size()) == OG_OK && ogc::lookup_ir_entry("w24").asset->frames == 3 && ogc::lookup_ir_entry("w24").asset->channels == 3,
           "PCM 24, three channels");
    expect(register_file(dir, "wf", flt, flt.size()) == OG_OK && ogc::lookup_ir_entry("wf").asset->frames == 4 && ogc::lookup_ir_entry("wf").asset->rate == 22050, "float 32 mono");
    expect(register_file(dir, "bad", wav(1, 1, 8000, 8, 4), 48) == OG_E_UNSUPPORTED, "8-bit PCM is OG_E_UNSUPPORTED");
    expect(register_file(dir, "bad", wav(2, 1, 8000, 4, 4), 48) == OG_E_UNSUPPORTED, "ADPCM is OG_E_UNSUPPORTED");
    expect(register_file(dir, "bad", wav(1, 9, 8000, 16, 18), 62) == OG_E_INVALID, "nine channels are OG_E_INVALID");
    expect(register_file(dir, "bad", wav(1, 1, 0, 16, 4), 48) == OG_E_INVALID, "a zero rate is OG_E_INVALID");
    expect(register_file(dir, "bad", wav(1, 1, 8000, 16, 0), 44) == OG_E_INVALID, "an empty data chunk is OG_E_INVALID");
    size_t refused = 0;
    for (size_t n = 0; n < pcm16.size(); ++n) refused += register_file(dir, "bad", pcm16, n) == OG_E_INVALID;
    expect(refused == pcm16.size(), "every truncation of a well-formed file is OG_E_INVALID");
    expect(!ogc::lookup_ir_entry("bad"), "... and none of these registered anything");
    expect(og_register_ir_wav("bad", (dir + "/nowhere.wav").c_str()) == OG_E_INVALID && og_register_ir_wav(nullptr, "x") == OG_E_INVALID, "a missing file and a null name");
    for (const char* n : {"w16", "w24", "wf"}) ogc::unregister_ir(n);
}

// from_asset, restated naively: [planes][taps]
std::vector<float> map_naive(const std::vector<float>& conformed, uint32_t taps, uint32_t src_ch, uint32_t bus_ch, uint32_t* planes)
{
    std::vector<float> out;
    if (bus_ch == 1 && src_ch > 1) {
        *planes = 1;
        std::vector<float> mono(taps, 0.0f);
        for (uint32_t c = 0; c < src_ch; ++c)
            for (uint32_t k = 0; k < taps; ++k) mono[k] += conformed[(size_t)k * src_ch + c];
        const float inv = 1.0f / (float)src_ch;
        for (float& m : mono) m *= inv;
        return mono;
    }
    *planes = src_ch == 1 ? 1 : bus_ch;
    for (uint32_t p = 0; p < *planes; ++p) {
        const uint32_t sc = src_ch == 1 ? 0 : (p < src_ch - 1 ? p : src_ch - 1);
        for (uint32_t k = 0; k < taps; ++k) out.push_back(conformed[(size_t)k * src_ch + sc]);
    }
    return out;
}

void mapping_cases()
{
    size_t cases = 0, wrong = 0;
    for (uint32_t src_ch = 1; src_ch <= 8; ++src_ch)
        for (uint32_t bus_ch = 1; bus_ch <= 4; ++bus_ch)
            for (uint32_t taps : {1u, 2u, 255u, 257u}) {
                std::vector<float> conformed((size_t)taps * src_ch);
                uint64_t s = 0x9E3779B97F4A7C15ull + src_ch * 131 + bus_ch * 17 + taps;
                for (float& x : conformed) {
                    s = s * 6364136223846793005ull + 1442695040888963407ull;
                    x = (float)(int32_t)(s >> 33) / 1073741824.0f;
                }
                uint32_t planes = 0;
                const std::vector<float> want = map_naive(conformed, taps, src_ch, bus_ch, &planes);
                // what conv_build_asset does, lane by lane, on exact-size heap buffers
                const uint32_t eng_planes = (src_ch == 1 || bus_ch == 1) ? 1u : bus_ch;
                const uint32_t downmix = bus_ch == 1 && src_ch > 1 ? 1u : 0u;
                float* src = heap(conformed);
                float* dst = (float*)malloc((size_t)eng_planes * taps * 4);
                for (uint32_t p = 0; p < eng_planes; ++p)
                    for (uint32_t k = 0; k < taps; ++k) dst[(size_t)p * taps + k] = og_bus_ir_tap(src + (size_t)k * src_ch, src_ch, p, downmix, 1.0f / (float)src_ch);
                wrong += eng_planes != planes || memcmp(dst, want.data(), want.size() * 4) != 0;
                free(src);
                free(dst);
                ++cases;
            }
    printf("%zu mappings (1..8 source channels onto 1..4 bus channels)\n", cases);
    expect(wrong == 0, "every mapping is from_asset's, bit for bit");
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]);
        return 2;
    }
    registry_cases();
    wav_cases(argv[1]);
    mapping_cases();
    printf("%s\n", bad ? "FAILED" : "all asset response cases as expected");
    return bad ? 1 : 0;
}
