// og_graph.h -- host-side graph description, lowering and HIP code generation.
//
// This is the MI355X engine's counterpart of the reference's compile-time
// layer (oscen-macros `graph!` -> oscen-graph-compiler: parse -> IR -> passes
// -> codegen).  The reference decides the schedule when rustc expands the
// macro; here the same decisions are taken when a graph description is
// flattened on the host:
//   * Kahn topological order over non-feedback edges   (ir/lower.rs:1015-1085)
//   * dead-node removal by reverse BFS from the outputs (ir/passes/dead_nodes.rs:11-62)
//   * >= 2 stream sources into one input = sum in edge order
//                                                       (codegen/emit_node.rs:35-111,153-174)
//   * compound sources (`a.x * b.y -> dst`) evaluated as f32 expressions
//                                                       (codegen/emit_node.rs:241-286)
//   * event inputs dispatched to the node handlers on their exact frame
//                                                       (codegen/mod.rs:755-873)
// and the result is one fused voice kernel (HIP source) whose per-voice state
// is laid out as [word][voice] planes.
#pragma once
#include "og_abi.h"
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace ogc {

enum class Kind { Value = 0, Event = 1, Stream = 2 };

// How fast a value changes, which decides where it is computed.
enum class Rate {
    Const = 0,   // literal
    UBlock = 1,  // voice-uniform, constant over the block (plain broadcast value input)
    UFrame = 2,  // voice-uniform, per-frame (ramped broadcast value input)
    VBlock = 3,  // per-voice, changes only through set-value events
    Vary = 4,    // per-voice per-sample
};

struct UEnv { // host-side evaluation environment for block-uniform expressions
    float sample_rate;
    const float* input_values; // by graph-input index (ramped inputs: `.current`)
    // the blocks one launch renders: first frame of block k inside the launch (block 0 starts at 0), for handlers that
    // read EventInstance::frame_offset (the offset inside the process_block call)
    const uint32_t* block_starts = nullptr;
    uint32_t n_blocks = 0;
};
using HostFn = std::function<float(const UEnv&)>;

struct GInput {
    std::string name;
    Kind kind = Kind::Value;
    float def = 0.0f;
    uint32_t ramp_frames = 0; // [ramp: N] (value inputs only)
    bool per_voice = false;   // value input fed per voice (MidiVoiceHandler.frequency)
    int channels = 1;         // stream inputs: `input stream dry: Frame<2>;` (oscen-lib/tests/stereo_render.rs:46-47) = N rows
};
struct GOutput {
    std::string name;
    Kind kind = Kind::Stream;
    int channels = 0; // `output out: stream: Frame<2>;`: the declared frame width (0 = not declared: taken from what feeds it)
};
struct GNode {
    std::string name;
    std::string type; // "AdsrEnvelope::new", "PolyBlepOscillator::saw", ...
    std::vector<float> args;
    uint32_t rate_factor = 1; // `* N`
    bool bus = false;         // post-mix node of the wrapper graph (runs once on the summed bus, e.g. Tremolo)
    uint32_t array_len = 0;   // `name = [Type::ctor(..); N]` (parse.rs:447-520): a node array of N elements; 0 = a single node
    // constructor arguments that are not numbers (`Voice::new(sample_rate)`, `Convolver::with_ir(reverb_ir())`): raw text,
    // parallel to `args` ("" where the argument is a number; empty vector = all numeric).  A node type that needs the
    // value of such an argument is diagnosed at lowering; nested graph types ignore their constructor arguments.
    std::vector<std::string> raw_args;
    bool inline_bare = false; // nested graph inlined WITHOUT the `<name>_` prefix (the voice graph of a lowered poly wrapper)
};
struct GEdge {
    std::string src; // endpoint or compound expression: "env.output", "a.x * b.y", "gate"
    std::string dst; // "node.port" or graph output name
    std::string policy; // "", "sinc", "sinc_iir", "linear", "latch"
    // outgoing leg of `src -> [via] -> dst` (ir/lower.rs:342-347): imposes no ordering; a consumer
    // scheduled before `via` reads the output `via` produced on the previous frame
    bool feedback = false;
};

struct GraphDesc {
    std::string name;
    std::vector<GInput> inputs;
    std::vector<GOutput> outputs;
    std::vector<GNode> nodes;
    std::vector<GEdge> edges;
};

// What lowering a poly WRAPPER graph (MidiParser -> VoiceAllocator<N> -> [MidiVoiceHandler; N] -> [Voice; N] -> sum
// [-> post-mix node], examples/fm-synth/src/lib.rs:22-131) found: the control-rate MIDI nodes run on the host
// (og_midi_*), the voice array is the bank.  `declared_voices` is the reference's N (the bank size is og_create's).
struct PolyInfo {
    bool is_wrapper = false;
    uint32_t declared_voices = 0;
    std::string voice_type;      // "FMVoice"
    std::string frequency_input; // per-voice value input of the lowered graph fed by MidiVoiceHandler.frequency
    std::string gate_input;      // event input fed by MidiVoiceHandler.gate
    std::string midi_input;      // the wrapper's raw-MIDI event input (`midi_in`), served by og_midi_send
    std::vector<std::string> dropped_event_outputs; // `midi_parser.note_on -> note_on_out`: host-side events, not lowered
};
// The voice-bank graph a poly wrapper lowers to (identity for any other description).
GraphDesc lower_poly_wrapper(const GraphDesc& g, PolyInfo* info = nullptr);
// the reference's example voice graphs as graph TYPES (usable as nested nodes and as the voice of a poly wrapper):
// "FMVoice" (examples/fm-synth/src/fm_voice.rs:6-156), "ElectricPianoVoiceNode" (electric_piano_voice.rs:362-402)
std::map<std::string, GraphDesc> builtin_voice_graph_types();

// ---- compiled form ---------------------------------------------------------
struct InputInfo {
    GInput decl;
    int slot = -1;       // broadcast value inputs: block-uniform slot with the current value
    int ramp_row = -1;   // ramped inputs: row in the per-frame ramp table
    int state_word = -1; // per-voice value inputs: state plane
    int event_index = -1;
    int stream_row = -1; // stream inputs: row of the per-frame table (after the ramp rows)
};
struct StateWord {
    std::string name;
    bool is_float = true;
    std::function<uint32_t(const UEnv&)> init; // initial bits
    bool read_mostly = false; // written back only in blocks that changed it (tables derived from events)
};
struct UniformProg {
    int dst;
    std::function<uint32_t(const UEnv&)> fn;
};
struct RingSpec { // a per-voice delay line in HBM (Delay's RingBuffer, delay/mod.rs:59-69)
    std::string name;
    float rate_factor = 1.0f;
    // next_power_of_two(min((2.0 * sr) as usize, 88200))
    uint32_t capacity(float graph_sr) const;
};
enum class BusStage { None = 0, Tremolo = 1, Convolver = 2 };
struct CompiledGraph {
    std::string name;
    std::string source; // complete HIP translation unit for this graph
    std::string zero_source; // ... and that of its zero variant (og_graph.cpp, ZeroChain; empty: none): csrc/gen/<graph>_z.hip
    std::string zero2_source; // ... and that of its deeper zero variant (og_graph.cpp, ZeroFolds; empty: none): csrc/gen/<graph>_z2.hip
    uint64_t hash = 0;  // FNV-1a of the kernel body: AOT registry / JIT cache key
    std::vector<InputInfo> inputs;
    std::vector<StateWord> state;      // per-voice words
    std::vector<StateWord> lane_state; // per-(voice, lane) words of LPV > 1 graphs
    std::vector<RingSpec> rings;       // delay lines (at most OG_MAX_RINGS)
    // SamplePlayer nodes (og_sample_player.hip.h; at most MAX_PLAYERS): the engine publishes a sample by writing the two state
    // words; player_slot0 is the first of five slots the ENGINE fills per launch (pool address, descriptor table address,
    // entries per player) -- they have no UniformProg
    struct PlayerSpec {
        std::string name;
        int channels = 1;                          // 1 = f32, N = Frame<N>
        int sample_word = -1, playhead_word = -1;  // state planes
    };
    std::vector<PlayerSpec> players;
    int player_slot0 = -1;
    // array fields of registered node types (og_node_array.hip.h): one entry per (node instance, field).  Element i of voice
    // slot v lives at pool[(base + i) * n_voices + v] of the engine's node-array pool; narr_slot0 is the first of the two
    // slots the ENGINE fills per launch with the pool's address (no UniformProg)
    struct ArraySpec {
        std::string path;  // "node.field" of the flattened graph, as the state words are named
        uint32_t base = 0; // first plane, in words per voice
        uint32_t length = 0;
        bool is_uint = false;
        uint32_t init = 0; // bits
    };
    std::vector<ArraySpec> arrays;
    int narr_slot0 = -1;
    uint32_t array_words() const { return arrays.empty() ? 0u : arrays.back().base + arrays.back().length; } // per voice
    // Oscilloscope nodes (og_scope.hip.h): the physical ring and the frozen window are two entries of `arrays`
    // ("<node>.ring", "<node>.triggered"), everything else is ordinary state words
    struct ScopeSpec {
        std::string name; // node name of the flattened graph
        uint32_t capacity = 1;
        bool auto_detect = false;
        int ring_array = -1, frozen_array = -1; // indices into `arrays`
        int w_write_pos = -1, w_written = -1, w_triggered_length = -1, w_window_end = -1, w_pending = -1; // state planes
    };
    std::vector<ScopeSpec> scopes;
    bool reads_block_starts = false;   // an event handler reads frame_offset: a launch carries the starts of its (at most 32) blocks
    int lpv = 1;                       // lanes per voice (8 for the electric-piano voice)
    int lane_width = 1;                // words a lane owns of every lane_state array (OG_HPL = 4 when lpv > 1)
    bool can_split = false;            // a two-wave pipeline variant of the kernel exists (og_k2_*)
    int max_pipeline = 1;              // deepest pipeline variant generated: 1, 2 (og_k2_*) or 4 (og_k4_*)
    bool wide4 = false;                // the four-wave pipeline also exists with 16-frame hand-offs (og_k4w_*): fewer barriers, twice
                                       // the LDS rings -- for banks whose workgroups all fit a CU at once
    // the zero variant (og_graph.cpp, ZeroChain): slots whose values must all be +-0 for a launch to run og_k*_<hash>_{00,01}z
    // (empty: the graph has no such kernel)
    std::vector<int> zero_slots;
    // the deeper zero variant (og_graph.cpp, ZeroFolds): a launch runs og_k*_<hash>_{00,01}z2 when every slot of zero2_slots
    // (zero_slots included) holds +-0 and every slot of finite_slots holds a finite value (empty zero2_slots: no such kernel)
    std::vector<int> zero2_slots, finite_slots;
    bool stage_spec = false; // ... and its four-wave pipeline has the stage-uniform envelope bodies (og_stage_uniform.hip.h)
    int valu_estimate = 0;             // estimated VALU instructions per frame of one wave of the ordinary kernel (node weights)
    // post-mix stage: one node on the summed bus.  Tremolo (electric-piano/src/main.rs:88-96) -> Frame<2>; Convolver
    // (oscen-lib/src/convolution/mod.rs) -> as many channels as the voices
    BusStage bus_stage = BusStage::None;
    HostFn tremolo_rate, tremolo_depth;
    std::string bus_ir_name;                            // Convolver::with_ir(<name>()): the registered response ("": Convolver::new())
    std::shared_ptr<const std::vector<float>> bus_ir;   // ... its taps as registered when the graph was lowered (null: the empty convolver)
    // post-mix GRAPH (any other set of wrapper-level nodes behind the voice sum): those nodes compiled as a second graph of one
    // voice whose last stream input carries the voice sum, run by its own one-wave kernel (og_kp_<hash>_{00,10},
    // og_post_mix.hip.h) between the bus reduce and the copies.  The voice graph is compiled as if they were not there.
    std::unique_ptr<CompiledGraph> post;
    // ... and, in `post` itself:
    bool is_post = false;
    int pm_slot0 = -1;                    // first of the five slots the ENGINE fills per launch: input rows (2), destination (2), row stride
    std::vector<int> post_input_of;       // per input of `post`: the wrapper's input it mirrors (-1: the voice sum)
    std::vector<std::string> post_nodes;  // the partition: names of the post-mix nodes, in declaration order
    std::vector<UniformProg> uprogs;
    std::vector<int> release_slots; // release length in samples (ADSR_R_N) of every outer-rate envelope: sizes the reciprocal table
    int n_slots = 0;
    int n_ramps = 0;
    int n_streams = 0; // rows n_ramps.. of the per-frame table taken by graph-level stream inputs (`<stream_in>_block`;
                       // a Frame<N> input takes N consecutive rows, one per channel)
    int n_stream_inputs = 0; // the stream inputs themselves (BlockRender::NUM_STREAM_INPUTS)
    int n_event_inputs = 0;
    std::vector<std::string> event_outputs; // the graph's event outputs that a node feeds, in declaration order (og_read_output_events)
    bool has_node_event_outputs = false;    // some live node has an #[output(event)] field (drops are counted on the device)
    uint32_t channels = 1;
    uint32_t voice_channels = 1; // channels of the voice sum: one per stream output of the voice graph, a Frame<2> output two
    struct OutChan {
        std::string name;
        int offset, width;
    };
    std::vector<OutChan> output_channels; // where every stream output sits in a frame of the bus / of a tap
    uint32_t latency_samples = 0;
    std::vector<std::string> node_order;     // the reference's topological order (Kahn, ir/lower.rs:1015-1085)
    std::vector<std::string> schedule_order; // the order the nodes are emitted in (== node_order unless the graph is a pure
                                             // per-frame dataflow, which is scheduled depth first from its sinks)
    int find_input(const std::string& n) const;
};

// The partition of an EXPANDED description whose bus nodes form a post-mix graph: `voice` is the description without them (its
// one stream output is the voice sum), `post` holds them -- the wrapper's broadcast value inputs in order, then the stream
// input `sum_input` (the voice sum; compile() sets its width), the graph's outputs but the sum.  False (nothing written): no
// bus node, or a lone Tremolo / Convolver (their own stages).  Throws what compile() throws for the shapes it refuses.
struct PostSplit {
    GraphDesc voice, post;
    std::string sum_input;
};
bool split_post_mix(const GraphDesc& expanded, PostSplit& out);

// Throws std::runtime_error with a diagnostic on malformed/unsupported graphs.
std::unique_ptr<CompiledGraph> compile(const GraphDesc& g);
// The connections the reference's macro refuses (kind mismatch between typed ends, ir/lower.rs:459-490; a summed fan-in with a
// compound / cross-rate / array source, codegen/emit_node.rs:35-125), checked on the description as written.  compile() and
// register_graph_type() call it; throws with the reference's wording.
void check_reference_rules(const GraphDesc& g);

// ---- user node types: the `#[derive(Node)]` plug-in surface (oscen-macros/src/lib.rs:7-327) -----------------
// A node type = its endpoints (`#[input(stream|value|event)]`, `#[output(stream)]` fields), its private fields
// (per-voice state words), the body of `SignalProcessor::process()` and of the `on_<event>()` handlers, given as
// device source.  Inside the bodies every input is a `const float <name>`, every state field a `float& <name>` /
// `uint32_t& <name>`, every output a `float& <name>`, plus `const float sample_rate`; an event handler also sees
// `const float value` (the scalar payload).  The bodies are compiled into the fused voice kernel (hiprtc).
struct UserPort {
    std::string name;
    Kind kind = Kind::Stream;
    float def = 0.0f;
    int arg = -1; // constructor argument that initialises the field, or -1
    int channels = 1; // stream inputs: 1 = f32, N = Frame<N>
};
struct UserState {
    std::string name;
    bool is_uint = false;
    float init_f = 0.0f;
    uint32_t init_u = 0;
    int arg = -1; // constructor argument that initialises it (f32 fields), or -1
};
struct UserArray { // a per-voice array field (og_node_array)
    std::string name;
    uint32_t length = 0;
    bool is_uint = false;
    float init_f = 0.0f;
    uint32_t init_u = 0;
};
constexpr uint32_t NODE_ARRAY_MAX_LEN = 65536u;       // (OG_NODE_ARRAY_MAX_LEN)
constexpr uint32_t NODE_ARRAYS_MAX = 8u;              // per type
constexpr uint32_t NODE_ARRAY_WORDS_MAX = 1u << 20;   // per voice, summed over a graph
struct UserNodeType {
    std::string type; // "FmOperator::new"
    size_t nargs = 0;
    std::vector<UserPort> inputs;
    std::vector<std::string> outputs;
    std::vector<int> out_channels;       // per output: 1 = f32, N = Frame<N> (empty: all f32)
    std::vector<std::string> ev_outputs; // `#[output(event)]` fields
    std::vector<UserState> state;
    std::vector<UserArray> arrays; // `og::NodeArray<T, N>& <name>` in the bodies, after the state fields
    std::string process_src;
    std::map<std::string, std::string> handlers; // event input -> body of on_<input>()
    int weight = 0; // estimated VALU cost per tick (0 = estimate from the source)
    int event_capacity = 0; // pushes per frame an event output of this type holds (0 = 2; the reference: 32)
};
void register_user_node(const UserNodeType& t); // throws on malformed descriptions or a clash with a built-in type
bool unregister_user_node(const std::string& type);

// named pure functions applied on a connection (`half(a.output) -> out`, `dsp::decode_ms(s.output) -> out`;
// ast.rs:126-128, oscen-lib/tests/connection_expr_functions.rs): device source, like a user node's process()
struct UserFunction {
    std::string name;                   // "half", or a path "dsp::decode_ms"
    std::vector<std::string> arg_names; // parameter names inside `source`
    std::vector<int> arg_channels;      // 1 = f32, N = Frame<N> (og::Frame<N>)
    int result_channels = 1;
    std::string source;                 // the function body: `return x * 0.5f;`
};
void register_user_function(const UserFunction& f); // throws on a malformed description
bool unregister_user_function(const std::string& name);

// impulse responses by name (`Convolver::with_ir(reverb_ir())`): mono, at the session rate; a registration under a name
// that exists replaces it.  lookup: the call's path as written or its last segment, parentheses and arguments ignored.
void register_ir(const std::string& name, const float* taps, size_t n_taps);
bool unregister_ir(const std::string& name);
std::shared_ptr<const std::vector<float>> lookup_ir(const std::string& call_text, std::string* resolved = nullptr);
// ... and the ASSET form beside it, in the same name space (a name holds one form; registering either replaces what the name
// held): 1..8 channels of interleaved frames at their own rate -- the reference's `#[input(asset)] ir` slot, an AudioAsset
// handed to ConvolverConsumer::build.  It is published with og_set_bus_ir, which conforms it to the engine's rate and maps
// its channels onto the bus's; `Convolver::with_ir` (the reference's mono, session-rate constructor) refuses it.
struct IrAsset {
    std::vector<float> interleaved; // [frames][channels]
    uint32_t frames = 0, channels = 0, rate = 0;
};
constexpr uint32_t MAX_IR_ASSET_CHANNELS = 8;             // (MAX_CONV_CHANNELS, convolution/mod.rs:310)
constexpr uint64_t MAX_IR_ASSET_FLOATS = (uint64_t)1 << 28; // frames x channels, as for samples
// (throws on a bad name, a zero rate, no frames, null data, a channel count outside 1..8, more than 2^28 samples)
void register_ir_asset(const std::string& name, const float* interleaved, uint64_t frames, uint32_t channels, uint32_t rate);
// what a name holds: `taps` (the mono form), `asset`, or neither
struct IrEntry {
    std::shared_ptr<const std::vector<float>> taps;
    std::shared_ptr<const IrAsset> asset;
    explicit operator bool() const { return taps || asset; }
};
IrEntry lookup_ir_entry(const std::string& call_text, std::string* resolved = nullptr);
constexpr size_t MAX_IR_TAPS = (size_t)1 << 20; // (og_bus_conv.hip.h: OG_CONV_MAX_TAPS)
constexpr size_t MAX_PLAYERS = 4;                   // SamplePlayer nodes per graph

// graph types usable as nodes of other graphs (nested graphs: `sub = SubGraph::new()`), expanded inline
void register_graph_type(const std::string& name, const GraphDesc& g);
bool unregister_graph_type(const std::string& name);
// node arrays and nested graphs are desugared before lowering; exposed for tests / to_dsl of the expansion
GraphDesc expand(const GraphDesc& g);
// `TptFilter::<Frame<2>>::new` / `::<Stereo>` -> "TptFilter<2>::new"; `::<f32>` -> "TptFilter::new"
std::string normalize_type(const std::string& type);

uint64_t fnv1a(const std::string& s);

// `graph! { ... }` body text -> description (og_dsl.cpp).  `per_voice` names the value inputs the
// poly wrapper feeds per voice (e.g. "frequency").  to_dsl() prints a description back as DSL text.
GraphDesc parse_dsl(const std::string& text, const std::vector<std::string>& per_voice);
std::string to_dsl(const GraphDesc& g);

// Built-in graph descriptions (builder form of the reference graphs in scope).
GraphDesc builtin_graph(const std::string& name);
std::vector<std::string> builtin_graph_names();

} // namespace ogc
