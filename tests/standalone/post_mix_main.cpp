// tests/standalone/post_mix_main.cpp -- the host-only bookkeeping of post-mix graphs, as a program of its own (built with a
// plain C++ compiler, also under -fsanitize=address,undefined; nothing is loaded into Python):
//   * ogc::split_post_mix (og_graph.cpp): the partition of a lowered wrapper into the voices and the post-mix graph, and
//     every shape it refuses;
//   * ogpm::* (og_post_mix_host.h): the snapshot section's encode, decode and refusal paths, on buffers of exactly the
//     section's size (a read past the end is the sanitizer's to find), at odd alignments.
// Prints one "path <name> <count>" line per branch it is meant to take and "ok" at the end; exit status 1 on a failed check.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <set>
#include <stdexcept>
#include <string>

#include "og_graph.h"
#include "og_post_mix_host.h"

static std::map<std::string, int> paths;
static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static const char* WRAPPER_HEAD =
    "name: Poly; input midi_in: event; input cut: value = 1200.0 [ramp: 300]; output out: stream; %s\n"
    "nodes { midi_parser = MidiParser::new(); voice_allocator = VoiceAllocator::<4>::new();\n"
    "        voice_handlers = [MidiVoiceHandler::new(); 4]; voices = [FMVoice::new(); 4];\n"
    "        %s }\n"
    "connections { midi_in -> midi_parser.midi_in; midi_parser.note_on -> voice_allocator.note_on;\n"
    "        midi_parser.note_off -> voice_allocator.note_off; voice_allocator.voices -> voice_handlers.note_on;\n"
    "        voice_allocator.voices -> voice_handlers.note_off; voice_handlers.frequency -> voices.frequency;\n"
    "        voice_handlers.gate -> voices.gate;\n"
    "        %s }\n";

static ogc::GraphDesc wrapper(const std::string& outputs, const std::string& nodes, const std::string& edges)
{
    char buf[8192];
    snprintf(buf, sizeof buf, WRAPPER_HEAD, outputs.c_str(), nodes.c_str(), edges.c_str());
    return ogc::parse_dsl(buf, {});
}

static std::set<std::string> names(const std::vector<ogc::GNode>& v)
{
    std::set<std::string> s;
    for (const auto& n : v) s.insert(n.name);
    return s;
}

// the message of the refusal (empty: none)
static std::string refusal(const ogc::GraphDesc& g)
{
    try {
        ogc::PostSplit ps;
        (void)ogc::split_post_mix(ogc::expand(g), ps);
    } catch (const std::exception& e) {
        return e.what();
    }
    return std::string();
}

static void partition()
{
    { // a master section: filter with an LFO on its cutoff, echo, gain; a dry output beside it
        const ogc::GraphDesc g = wrapper("output dry: stream;",
                                         "lfo = Oscillator::sine(0.3, 1.0); master = TptFilter::new(1200.0, 0.707); echo = Delay::new(4800.0, 0.4); trim = Gain::new(0.5);",
                                         "voices.audio_out -> master.input; lfo.output * 800.0 + cut -> master.cutoff; master.output -> [echo] -> trim.input; "
                                         "trim.output -> out; voices.audio_out -> dry;");
        ogc::PostSplit ps;
        CHECK(ogc::split_post_mix(ogc::expand(g), ps));
        CHECK((names(ps.post.nodes) == std::set<std::string>{"lfo", "master", "echo", "trim"}));
        for (const auto& n : ps.voice.nodes) CHECK(!n.bus && !names(ps.post.nodes).count(n.name));
        CHECK(ps.voice.outputs.size() == 1 && ps.voice.outputs[0].name == ps.sum_input);
        CHECK(ps.post.outputs.size() == 2 && ps.post.outputs[0].name == "out" && ps.post.outputs[1].name == "dry");
        CHECK(!ps.post.inputs.empty() && ps.post.inputs.back().name == ps.sum_input && ps.post.inputs.back().kind == ogc::Kind::Stream);
        bool has_cut = false, dry_edge = false;
        for (const auto& in : ps.post.inputs) {
            CHECK(in.kind != ogc::Kind::Event && !in.per_voice);
            has_cut = has_cut || (in.name == "cut" && in.ramp_frames == 300);
        }
        CHECK(has_cut);
        for (const auto& e : ps.post.edges) dry_edge = dry_edge || (e.dst == "dry" && e.src == ps.sum_input);
        CHECK(dry_edge);
        paths["partition_master_section"] += 1;
        // compiled: the voice kernel is the wrapper's without the post-mix nodes, the post-mix unit has its own entries
        const auto with = ogc::compile(g);
        const auto without = ogc::compile(wrapper("", "", "voices.audio_out -> out;"));
        CHECK(with->post && with->post->is_post && with->post->source.find("og_kp_") != std::string::npos);
        CHECK(with->post->post_nodes.size() == 4 && with->channels == 2 && with->voice_channels == 1);
        CHECK(!without->post && with->hash == without->hash);
        paths["compiled_beside_the_plain_wrapper"] += 1;
    }
    { // the legacy stages are not split
        const ogc::GraphDesc g = wrapper("", "tremolo = Tremolo::new();", "voices.audio_out -> tremolo.input; tremolo.output -> out;");
        ogc::PostSplit ps;
        CHECK(!ogc::split_post_mix(ogc::expand(g), ps));
        CHECK(!ogc::split_post_mix(ogc::expand(wrapper("", "", "voices.audio_out -> out;")), ps));
        paths["legacy_not_split"] += 1;
    }
    struct Case {
        const char* path;
        std::string outputs, nodes, edges, expect;
    };
    const Case refusals[] = {
        {"refuse_tremolo_with_others", "", "tremolo = Tremolo::new(); trim = Gain::new(0.5);",
         "voices.audio_out -> tremolo.input; tremolo.output -> trim.input; trim.output -> out;", "only one post-mix"},
        {"refuse_oversampled", "", "master = TptFilter::new(1200.0, 0.707) * 2;", "voices.audio_out -> master.input; master.output -> out;", "oversampled"},
        {"refuse_sample_player", "", "trim = Gain::new(0.5); sp = SamplePlayer::new();", "voices.audio_out -> trim.input; sp.output -> trim.gain; trim.output -> out;",
         "a SamplePlayer is not supported"},
        {"refuse_feeds_both", "", "lfo = Oscillator::sine(0.3, 1.0); master = TptFilter::new(1200.0, 0.707);",
         "voices.audio_out -> master.input; lfo.output -> master.cutoff; lfo.output -> voices.filter_cutoff; master.output -> out;", "feeds both"},
        {"refuse_feedback_into_voices", "", "master = TptFilter::new(1200.0, 0.707);",
         "voices.audio_out -> master.input; master.output -> voices.filter_cutoff; master.output -> out;", "feeds back into the voices"},
    };
    for (const Case& c : refusals) {
        const std::string msg = refusal(wrapper(c.outputs, c.nodes, c.edges));
        if (msg.empty() || msg.find(c.expect) == std::string::npos) fprintf(stderr, "%s: got '%s'\n", c.path, msg.c_str());
        CHECK(!msg.empty() && msg.find(c.expect) != std::string::npos);
        paths[c.path] += 1;
    }
}

static void section()
{
    ogpm::Layout l;
    l.state_names = {"master.z0", "master.z1", "echo.write_pos"};
    l.ring_caps = {8, 16};
    std::vector<uint32_t> words = {0x3f800000u, 0xbf000000u, 7u};
    std::vector<float> rings(24);
    for (size_t i = 0; i < rings.size(); ++i) rings[i] = 0.25f * (float)i;
    const std::vector<char> sec = ogpm::encode(l, words.data(), rings.data());
    CHECK(sec.size() == ogpm::section_bytes(l) && sec.size() == sizeof(ogpm::SectionHead) + (3 + 24) * 4);
    // at every alignment, in a buffer of exactly the section's size
    for (size_t shift = 0; shift < 4; ++shift) {
        std::vector<char> outer(shift + sec.size());
        std::copy(sec.begin(), sec.end(), outer.begin() + (long)shift);
        CHECK(ogpm::check(l, outer.data() + shift, sec.size()).empty());
        std::vector<uint32_t> w2;
        std::vector<float> r2;
        ogpm::decode(l, outer.data() + shift, w2, r2);
        CHECK(w2 == words && r2 == rings);
        paths["section_round_trip"] += 1;
    }
    { // a graph without state words or delay lines: the head alone
        ogpm::Layout e;
        const std::vector<char> s = ogpm::encode(e, nullptr, nullptr);
        CHECK(s.size() == sizeof(ogpm::SectionHead) && ogpm::check(e, s.data(), s.size()).empty());
        std::vector<uint32_t> w2;
        std::vector<float> r2;
        ogpm::decode(e, s.data(), w2, r2);
        CHECK(w2.empty() && r2.empty());
        paths["section_empty"] += 1;
    }
    auto refused = [&](const char* path, const ogpm::Layout& want, const std::vector<char>& bytes, const char* expect) {
        std::vector<char> exact(bytes); // (its own allocation: the check may not read past bytes.size())
        const std::string msg = ogpm::check(want, exact.empty() ? nullptr : exact.data(), exact.size());
        if (msg.find(expect) == std::string::npos) fprintf(stderr, "%s: got '%s'\n", path, msg.c_str());
        CHECK(!msg.empty() && msg.find(expect) != std::string::npos);
        paths[path] += 1;
    };
    refused("refuse_missing", l, {}, "missing");
    refused("refuse_cut_short_head", l, std::vector<char>(sec.begin(), sec.begin() + 12), "missing");
    refused("refuse_cut_short_body", l, std::vector<char>(sec.begin(), sec.end() - 4), "bytes");
    refused("refuse_trailing_bytes", l, [&] { auto b = sec; b.push_back(0); return b; }(), "bytes");
    {
        auto b = sec;
        b[0] ^= 1;
        refused("refuse_magic", l, b, "bad magic");
        b = sec;
        b[4] = 9;
        refused("refuse_version", l, b, "version");
    }
    {
        ogpm::Layout other = l;
        other.state_names[1] = "master.z9";
        refused("refuse_other_fields", other, sec, "another post-mix graph");
        other = l;
        other.state_names.push_back("trim.x");
        refused("refuse_other_word_count", other, sec, "another post-mix graph");
        other = l;
        other.ring_caps.pop_back();
        refused("refuse_ring_count", other, sec, "delay lines");
        other = l;
        other.ring_caps[1] = 32;
        refused("refuse_ring_capacity", other, sec, "another sample rate");
        other = l;
        other.ring_caps = {1, 2, 3, 4, 5};
        refused("refuse_too_many_rings", other, sec, "more delay lines");
    }
}

int main()
{
    try {
        partition();
        section();
    } catch (const std::exception& e) {
        fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    for (const auto& kv : paths) printf("path %s %d\n", kv.first.c_str(), kv.second);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
