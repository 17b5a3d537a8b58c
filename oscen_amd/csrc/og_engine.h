// og_engine.h -- internal: `struct og_engine` and its helper structs, for the translation units that implement the C ABI of
// include/oscen_gpu.h on an engine's internals: og_engine.cpp (the host runtime and its kernels), og_snapshot.cpp (state
// blobs) and og_cluster.cpp (multi-GPU banks).  The methods declared but not defined here launch kernels or use the device
// headers of og_engine.cpp: they are defined there.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/oscen_gpu.h"
#include "og_abi.h"
#include "og_bus_conv_host.h"
#include "og_graph.h"
#include "og_jit.h"
#include "og_node_array_host.h"
#include "og_scope_host.h"
#include "og_registry.h"
#include "og_timeline.h"

static_assert(sizeof(TlEvent) == sizeof(OgEvent) && offsetof(TlEvent, frame) == offsetof(OgEvent, frame) &&
                  offsetof(TlEvent, target) == offsetof(OgEvent, target) && offsetof(TlEvent, value) == offsetof(OgEvent, value),
              "the timeline's records are the kernels' OgEvent");

inline int set_err(int code, const std::string& m) { return ogabi::set_error(code, m); }
using ogabi::guard; // Error (carries its OG_E_* code) / bad_alloc / std::exception -> code + og_last_error(); og_abi.h

using HipError = ogabi::DeviceError;
#define HIPCK(expr)                                                                                    \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            throw HipError(std::string(#expr) + ": " + hipGetErrorString(_e));                         \
    } while (0)

// Host memory this library does not own (a caller's array, a std::vector) never goes to hipMemcpyAsync directly.  For
// a transfer above a size threshold the runtime pins the pages where they lie (a userptr mapping) and keeps the
// pinning cached; whenever the kernel later migrates, compacts or unmaps those pages the driver evicts and restores
// EVERY queue of the process.  Measured through the blocking entry at 4 M / 8 M voices (bench.py's real-time record:
// the 32 MB frequency array of og_set_voice_values and the event-timeline vectors of the first rebuild were such
// mappings): one ~23 ms stall of the stream -- several missed audio deadlines -- every few thousand blocks.  So every
// transfer larger than a staging copy goes through two pinned bounce buffers of this engine's own.
struct Bounce {
    static constexpr size_t CHUNK = (size_t)4 << 20, DIRECT = 16384; // (below DIRECT the runtime stages the bytes itself)
    void* h[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int k = 0;
    void ensure()
    {
        if (h[0]) return;
        for (int i = 0; i < 2; ++i) {
            HIPCK(hipHostMalloc(&h[i], CHUNK, hipHostMallocDefault));
            HIPCK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
    }
    // host -> device, asynchronous like hipMemcpyAsync from pinned memory: `src` may be reused when the call returns
    void h2d(void* dst, const void* src, size_t n, hipStream_t s)
    {
        if (n <= DIRECT) {
            if (n) HIPCK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s));
            return;
        }
        ensure();
        for (size_t off = 0; off < n; off += CHUNK) {
            const size_t len = std::min(CHUNK, n - off);
            if (busy[k]) HIPCK(hipEventSynchronize(ev[k]));
            memcpy(h[k], (const char*)src + off, len);
            HIPCK(hipMemcpyAsync((char*)dst + off, h[k], len, hipMemcpyHostToDevice, s));
            HIPCK(hipEventRecord(ev[k], s));
            busy[k] = true;
            k ^= 1;
        }
    }
    // device -> host; the bytes are in `dst` when the call returns (the stream is drained up to the copy)
    void d2h(void* dst, const void* src, size_t n, hipStream_t s)
    {
        if (n <= DIRECT) {
            if (n) HIPCK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            return;
        }
        ensure();
        size_t pend_off[2] = {0, 0}, pend_len[2] = {0, 0};
        auto land = [&](int i) {
            if (!pend_len[i]) return;
            HIPCK(hipEventSynchronize(ev[i]));
            memcpy((char*)dst + pend_off[i], h[i], pend_len[i]);
            pend_len[i] = 0;
            busy[i] = false;
        };
        for (int i = 0; i < 2; ++i)
            if (busy[i]) { // (an upload still reading the buffer)
                HIPCK(hipEventSynchronize(ev[i]));
                busy[i] = false;
            }
        for (size_t off = 0; off < n; off += CHUNK) {
            const size_t len = std::min(CHUNK, n - off);
            land(k);
            HIPCK(hipMemcpyAsync(h[k], (const char*)src + off, len, hipMemcpyDeviceToHost, s));
            HIPCK(hipEventRecord(ev[k], s));
            pend_off[k] = off;
            pend_len[k] = len;
            k ^= 1;
        }
        land(k);
        land(k ^ 1);
    }
    void release()
    {
        for (int i = 0; i < 2; ++i) {
            if (h[i]) (void)hipHostFree(h[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            h[i] = nullptr;
            ev[i] = nullptr;
        }
    }
};

struct Ramp { // ValueRampState  oscen-lib/src/graph/types.rs:300-373
    float current = 0, target = 0, increment = 0;
    uint32_t frames_remaining = 0;
    uint32_t default_frames = 0;
    bool ramping() const { return frames_remaining > 0; }
    void set_immediate(float v)
    {
        current = target = v;
        increment = 0.0f;
        frames_remaining = 0;
    }
    void set_with_ramp(float t, uint32_t frames)
    {
        if (frames == 0) {
            set_immediate(t);
        } else {
            target = t;
            increment = (t - current) / (float)frames;
            frames_remaining = frames;
        }
    }
    bool tick()
    {
        if (frames_remaining > 0) {
            frames_remaining -= 1;
            if (frames_remaining == 0) {
                current = target;
                increment = 0.0f;
                return true;
            }
            current += increment;
        }
        return false;
    }
};

constexpr int RAMP_RING = 8;
// Host-side bounds of one launch of queued blocks (og_set_bus_batching).  OG_MAX_LAUNCH_BLOCKS (32, og_kernel_rt.hip.h) stays
// the bound for graphs that read block starts on the device.
constexpr uint32_t OG_MAX_QUEUE_BLOCKS = 256;               // blocks one launch may cover
constexpr size_t OG_WIDE_ROW_BUDGET = (size_t)256 << 20;    // partial rows of one automatic launch of the wide four-wave form
constexpr int EV_RING = 8;              // pinned staging buffers of the incremental event path

struct og_graph_desc {
    ogc::GraphDesc g;
};

// ---- samples by name (og_register_sample): process-wide, beside the impulse responses --------------------------------
// interleaved frames as registered -- at the graph's rate (og_register_sample: rate 0, untagged) or at their own
// (og_register_sample_at_rate / og_register_sample_wav: og_load_sample conforms them on the device); a name that exists is
// replaced (engines that loaded the old one keep their device copy)
struct SampleData {
    std::vector<float> interleaved;
    uint32_t frames = 0, channels = 1;
    uint32_t rate = 0; // 0: untagged
};
std::shared_ptr<const SampleData> lookup_sample(const std::string& name);

// OSCEN_GPU_HOST_PROF=1: wall time of the host-side phases of the live path, printed when the engine is destroyed
struct HostProf {
    enum { SYNC_EVENTS, INCREMENTAL, REBUILD, LAUNCH, RAMPS, EV_WAIT, EV_COMMIT, N };
    double t[N] = {};
    uint64_t n[N] = {};
    bool on = ogabi::experiment_knob("OSCEN_GPU_HOST_PROF") != nullptr;
    struct Scope {
        HostProf& p;
        int k;
        std::chrono::steady_clock::time_point t0;
        Scope(HostProf& p_, int k_) : p(p_), k(k_) { if (p.on) t0 = std::chrono::steady_clock::now(); }
        ~Scope()
        {
            if (!p.on) return;
            p.t[k] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            p.n[k] += 1;
        }
    };
    void report() const
    {
        if (!on) return;
        static const char* names[N] = {"sync_events", "incremental_update", "full_rebuild", "flush_bus (launches)", "ramp table",
                                        "  staging-slot wait", "  commit + launch"};
        for (int k = 0; k < N; ++k)
            if (n[k]) fprintf(stderr, "[oscen_gpu host prof] %-22s %9llu calls %10.1f us total %8.2f us/call\n", names[k],
                              (unsigned long long)n[k], t[k] * 1e6, t[k] * 1e6 / (double)n[k]);
    }
};

struct og_engine {
    HostProf prof;
    std::unique_ptr<ogc::CompiledGraph> cg;
    OgLaunchFn launch = nullptr;
    OgZeroLaunchFn launch_zero = nullptr; // the zero variant of `launch` (og_graph.cpp, ZeroChain), where the graph has one
    bool zero_spec = true; // launches may run the graph's zero variant (OSCEN_GPU_ZERO_SPEC=0: never)
    bool last_zero = false; // the last launch ran a zero variant (og_kernel_name)
    // the deeper zero variant (og_graph.cpp, ZeroFolds): tier 2 of the registry
    OgZeroLaunchFn launch_zero2 = nullptr;
    bool zero2_spec = true; // launches may run it (OSCEN_GPU_ZERO2_SPEC=0, or OSCEN_GPU_ZERO_SPEC=0: never)
    bool stage_spec = true; // ... with its stage-uniform envelope bodies (OSCEN_GPU_STAGE_SPEC=0: the general quiet bodies only)
    bool guards_held = true; // every launch so far had finite values in cg->finite_slots: no operator state can hold inf / NaN
    int last_tier = 0;       // what the last launch ran: 0 general, 1 zero variant, 2 deeper zero variant (og_kernel_fold_tier)
    std::unique_ptr<OgJitKernel> jit;
    uint32_t V = 0;
    int device = 0;
    float sr = 44100.0f;
    bool inited = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    std::vector<float> values; // per input: plain value, or mirror of ramp.current
    std::vector<std::vector<float>> stream_blocks; // per input: `<stream_in>_block` (stream inputs only), OG_MAX_BLOCK samples
    std::vector<Ramp> ramps;   // per input (only meaningful when ramp_row >= 0)
    uint32_t active_ramps = 0;

    uint32_t n_wg = 0;
    uint32_t lanes = OG_WAVE;
    uint32_t split = 0; // pipeline depth of the launched kernel variant: 0 (ordinary), 2 or 4 waves per 64 voices
    bool wide = false;  // split == 4: the 16-frame hand-off form (og_k4w_*)
    uint32_t* d_state = nullptr;
    Bounce bounce; // pinned staging for transfers from / to memory that is not ours
    uint32_t* d_lane_state = nullptr;
    float* d_ring[OG_MAX_RINGS] = {nullptr, nullptr, nullptr, nullptr}; // delay lines [capacity][V]
    uint32_t ring_cap[OG_MAX_RINGS] = {0, 0, 0, 0};
    float* d_mono = nullptr;      // summed voices before the post-mix stage
    float* d_bus_phase = nullptr; // Tremolo.phase
    // ---- post-mix graph (cg->post; og_post_mix.hip.h) -------------------------------------------------
    // A second state image of ONE voice -- state words, Delay rings [capacity][1] -- and the rows og_bus_reduce writes the
    // voice sum into ([voice_channels][cap_frames], planar).  flush_bus: voice kernel -> reduce (into d_pm_in) -> post-mix
    // kernel (into the destination) -> copies.
    std::unique_ptr<OgJitKernel> pm_jit;
    uint32_t* d_pm_state = nullptr;
    float* d_pm_ring[OG_MAX_RINGS] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t pm_ring_cap[OG_MAX_RINGS] = {0, 0, 0, 0};
    float* d_pm_in = nullptr;
    uint32_t pm_last_frames = 0; // frames of the last launch: what d_pm_in holds (og_read_post_mix_input)
    uint32_t* d_pm_ev = nullptr; // {cursor, end} of the post-mix voice: both 0, no event ever reaches it
    std::vector<float> pm_values; // the post-mix graph's inputs: mirrors of `values` (filled per launch)
    bool post_on() const { return cg->post != nullptr; }
    void pm_reset(); // og_init: initial state words (the sample-rate-dependent ones recomputed), fresh zeroed rings
    size_t pm_ring_words() const
    {
        size_t n = 0;
        for (size_t k = 0; post_on() && k < cg->post->rings.size(); ++k) n += pm_ring_cap[k];
        return n;
    }
    ogc::UEnv pm_env()
    {
        const ogc::CompiledGraph& p = *cg->post;
        pm_values.assign(p.inputs.size(), 0.0f);
        for (size_t i = 0; i < p.inputs.size(); ++i)
            if (p.post_input_of[i] >= 0) pm_values[i] = values[(size_t)p.post_input_of[i]];
        return ogc::UEnv{sr, pm_values.data()};
    }
    // ---- post-mix Convolver (og_bus_conv.hip.h) ---------------------------------------------------
    // The host bookkeeping is og_bus_conv_host.h's: which response runs over which frames, where in the history, how large
    // the buffers are.  The engine owns the device memory and does the device work the class's plans describe.
    BusConvolver bus_conv;
    float* d_hist = nullptr;       // history: [bus_conv.hist_len()][voice_channels]
    float* d_conv_rows = nullptr;  // partial rows: 2 x bus_conv.rows_half() floats
    std::vector<float*> conv_bufs; // every device tap buffer this engine holds (conv_gc frees the unused ones)
    bool conv_on() const { return cg->bus_stage == ogc::BusStage::Convolver && bus_stage; }
    uint32_t conv_fade_len() const { return (uint32_t)std::max(1.0f, roundf(0.02f * sr)); } // prepare(): CROSSFADE_SECONDS * sr, rounded, >= 1
    std::shared_ptr<ConvIR> conv_upload(const float* taps, size_t n, uint32_t planes = 1) // n taps per plane
    {
        auto ir = std::make_shared<ConvIR>();
        ir->planes = n ? planes : 1u;
        ir->taps.assign(taps, taps + n * ir->planes);
        if (n) {
            HIPCK(hipMalloc(&ir->d, ir->taps.size() * 4));
            conv_bufs.push_back(ir->d);
            bounce.h2d(ir->d, ir->taps.data(), ir->taps.size() * 4, stream);
        }
        return ir;
    }
    // og_set_bus_ir on an asset response: conformed to the engine's rate and mapped onto the bus's channels on the device
    std::shared_ptr<ConvIR> conv_build_asset(const std::string& name, const ogc::IrAsset& a);
    void conv_gc() // free the taps no response in use points at; only with nothing queued and the stream idle
    {
        if (!queue.empty() || hipStreamQuery(stream) != hipSuccess) return;
        std::vector<float*> keep;
        for (float* p : conv_bufs) {
            if (bus_conv.holds(p)) keep.push_back(p);
            else (void)hipFree(p);
        }
        conv_bufs.swap(keep);
    }
    // (re)size the history and the partial rows for responses of up to k taps and the current launch capacity, keeping
    // the history; the stream is idle (callers launch the queue and wait first)
    void conv_alloc(size_t k);
    void conv_clear_history() { HIPCK(hipMemsetAsync(d_hist, 0, bus_conv.hist_len() * cg->voice_channels * 4, stream)); }
    void conv_reset() // prepare(): cleared history, no fade; the current response stays
    {
        if (!d_hist) return;
        conv_clear_history();
        bus_conv.reset();
    }
    float* conv_place_dry(BusConvolver::Launch& l); // plan the launch; where its dry sum goes (flush_bus)
    void conv_stage(BusConvolver::Launch& l, float* wet); // the post-mix stage of flush_bus
    // ---- SamplePlayer: the device sample pool ------------------------------------------------------------------------
    // og_load_sample appends a sample to the pool once per width the graph's players have (the reference's Vec<F>,
    // frame-major) and gives it the next index; the descriptor table [player][sample_cap]{offset in floats, frames} is what
    // the kernels read once per launch.  Growing either waits for the stream (not an audio-thread call).  Publishing
    // (og_set_sample / og_set_voice_samples) writes the players' two state words behind the queued blocks.
    struct LoadedSample {
        std::string name;
        uint32_t frames = 0, channels = 0; // the source's shape (snapshots check it)
        uint32_t src_rate = 0;             // the source's rate tag (0: untagged, never checked)
        uint32_t rate = 0;                 // tagged: the graph rate it was conformed to ...
        uint32_t pool_frames = 0;          // ... and its length in the pool (untagged: `frames`)
        uint32_t off[5] = {0, 0, 0, 0, 0}; // [width]: offset of the width's copy in the pool, in floats
    };
    // the graph rate a tagged sample is conformed to: og_init's, a positive integer (AudioAsset's rates are u32)
    uint32_t graph_rate(const char* who) const
    {
        if (!inited) throw ogabi::Error(OG_E_INVALID, std::string(who) + ": the graph rate is not set yet (og_init comes first for a sample registered at a rate)");
        if (!(sr >= 1.0f && sr < 4294967296.0f && sr == floorf(sr)))
            throw ogabi::Error(OG_E_INVALID, std::string(who) + ": a sample registered at a rate needs an engine rate that is a positive integer, this engine runs at " + std::to_string(sr));
        return (uint32_t)sr;
    }
    // the length a tagged sample has once conformed to `dst` (the checks of from_samples behind the resample)
    static uint32_t conformed_frames(const std::string& name, const SampleData& sd, uint32_t dst);
    std::vector<LoadedSample> samples;
    float* d_pool = nullptr;
    size_t pool_used = 0, pool_cap = 0; // floats
    uint32_t* d_desc = nullptr;
    uint32_t sample_cap = 0; // entries per player in d_desc
    void pool_reserve(size_t need)
    {
        if (need <= pool_cap) return;
        const size_t cap = std::max(need, std::max<size_t>(2 * pool_cap, (size_t)1 << 16));
        float* n = nullptr;
        HIPCK(hipMalloc(&n, cap * 4));
        if (pool_used) HIPCK(hipMemcpyAsync(n, d_pool, pool_used * 4, hipMemcpyDeviceToDevice, stream));
        HIPCK(hipStreamSynchronize(stream));
        if (d_pool) HIPCK(hipFree(d_pool));
        d_pool = n;
        pool_cap = cap;
    }
    void upload_desc() // the whole table: a few words per sample
    {
        const size_t np = cg->players.size();
        if (samples.size() > sample_cap) {
            const uint32_t cap = std::max<uint32_t>(16u, 2u * (uint32_t)samples.size());
            if (d_desc) HIPCK(hipFree(d_desc));
            d_desc = nullptr;
            sample_cap = 0;
            HIPCK(hipMalloc(&d_desc, np * cap * 2 * 4));
            sample_cap = cap;
        }
        std::vector<uint32_t> tab(np * sample_cap * 2, 0u);
        for (size_t k = 0; k < np; ++k)
            for (size_t i = 0; i < samples.size(); ++i) {
                tab[2 * (k * sample_cap + i)] = samples[i].off[cg->players[k].channels];
                tab[2 * (k * sample_cap + i) + 1] = samples[i].pool_frames;
            }
        bounce.h2d(d_desc, tab.data(), tab.size() * 4, stream);
        HIPCK(hipStreamSynchronize(stream));
    }
    // brings a registered sample onto the device (every width the players have); returns its index
    uint32_t load_sample(const std::string& name, const SampleData& sd);
    int find_player(const char* node) const
    {
        std::string p; // the spelling of og_read_state_field paths: `inner.player` -> `inner_player`
        for (const char* c = node; *c; ++c) {
            if (*c == '[') p += "__";
            else if (*c == '.') p.push_back('_');
            else if (*c != ']' && !isspace((unsigned char)*c)) p.push_back(*c);
        }
        for (size_t k = 0; k < cg->players.size(); ++k)
            if (cg->players[k].name == p) return (int)k;
        return -1;
    }
    // ---- array fields of registered node types: the node-array pool (og_node_array.hip.h) ----------------------------------
    // [cg->array_words()][V] words, allocated by og_create, filled with the fields' `init` by every og_init, handed to the
    // kernels through two uniform slots per launch
    uint32_t* d_narr = nullptr;
    bool narr_dirty = false; // written since the last fill (og_write_node_array, og_load_state): og_group_voices moves the columns
    size_t narr_bytes() const { return (size_t)ognarr::pool_bytes(cg->arrays, V); }
    void narr_fill(); // stream-ordered
    OgEvent* d_events = nullptr;
    uint32_t* d_ev_end = nullptr;
    uint32_t* d_ev_cursor = nullptr;
    float* d_partials = nullptr;
    float* d_partials2 = nullptr; // group sums of the multi-pass bus reduce
    // ADSR release reciprocals (OgBlockArgs::rcp_tab): entries 1 .. rcp_n, grown (never per block: at least doubled) when a
    // launch's longest release needs more; a replaced table stays allocated until og_destroy -- launches already queued may
    // still read it -- so that growing never waits for the device.  Launches whose release exceeds rcp_cap (OG_RCP_MAX;
    // experiment knob OSCEN_GPU_RCP_CAP) run the v_rcp_f32 bodies.
    float* d_rcp = nullptr;
    uint32_t rcp_n = 0;
    uint32_t rcp_cap = OG_RCP_MAX;
    std::vector<float*> rcp_old;
    // Block queue (og_set_bus_batching): up to `bus_batch` consecutive async blocks that nothing separates (no value
    // change, no event push, no taps) are rendered by ONE launch of the voice kernel over their frames back to back --
    // state loaded and stored once, one inter-kernel gap, one bus reduce per tree level -- instead of one launch each.
    // A queued block has had its ramps ticked and its stream samples captured; anything that touches engine state
    // launches the queue first.  Results are those of block-by-block processing, bit for bit.
    std::vector<uint32_t> tap_voices; // og_set_voice_taps: the tapped voices by the caller's numbers (slots are resolved from them)
    // The queue is also bounded in FRAMES (`cap_frames`): the partial rows, the staging bus, the convolver rows and the ramp
    // tables are sized by it, and a block that would not fit launches the queue first.  Up to OG_MAX_LAUNCH_BLOCKS blocks the
    // capacity is that of full 512-frame blocks, so a frame bound never cuts such a queue; longer queues are sized for
    // 256-frame blocks (launch_frames_cap).
    uint32_t bus_batch = 1; // queue limit (blocks per launch)
    size_t cap_frames = OG_MAX_BLOCK; // frames one launch may cover: what the buffers are sized for
    struct QueuedBlock {
        float* dst; // where the block's bus goes
        uint32_t frames;
        float trem_rate, trem_depth;
        uint32_t conv; // BusConvolver::queue_block (post-mix Convolver)
    };
    std::vector<QueuedBlock> queue;
    uint64_t q_frame0 = 0;   // absolute frame of the first queued block
    uint32_t q_frames = 0;   // frames queued
    bool q_ramps = false;    // some queued block ticked a ramp (or the graph has stream inputs): table-reading variant
    int q_ramp_slot = -1;    // staging buffer of the per-frame table being filled
    float* d_stage_bus = nullptr; // bus of a launch whose blocks' destinations are not contiguous
    float* d_bus = nullptr;
    float* d_ramp[RAMP_RING] = {};
    float* h_ramp[RAMP_RING] = {};
    uint64_t ramp_seq[RAMP_RING] = {}; // batch whose launch copied ramp table i to the device (0 = never)
    int ramp_head = 0;
    // events leaving the voices (graph event outputs) and pushes the in-voice queues dropped: device log / counter
    OgOutEvent* d_out_ev = nullptr;
    uint32_t* d_out_ev_count = nullptr; // [0] = events appended, [1] = in-voice pushes lost
    uint32_t out_ev_cap = 0;
    uint64_t out_ev_overflow = 0;       // events that did not fit the log (reported by og_read_output_events)
    uint64_t ev_lost_total = 0;         // in-voice pushes lost, read back so far
    std::vector<OgOutEvent> out_ev_carry; // og_read_output_events: drained from the device log, not yet handed out
    float* d_taps = nullptr;
    int32_t* d_tap_slot = nullptr;
    uint32_t n_taps = 0;
    uint32_t last_frames = 0;

    // ---- event timeline ---------------------------------------------------------------------------
    // The host bookkeeping is og_timeline.h's; the engine owns what the device sees of it -- d_events, d_ev_cursor, d_ev_end,
    // the pinned staging ring -- and does the device work between the halves of its two update paths (og_engine.cpp).
    EventTimeline tl;
    // og_group_voices: logical voice (what every entry point takes and hands out) -> physical slot (what the device arrays
    // and everything below the entry points index).  Empty = identity.
    std::vector<uint32_t> phys_of, logical_of;
    uint32_t phys(uint32_t v) const { return phys_of.empty() ? v : phys_of[v]; }
    uint32_t logical(uint32_t p) const { return logical_of.empty() ? p : logical_of[p]; }
    // end of the launch that is being prepared: everything before it must be in the voices' segments
    uint64_t launch_end() const { return queue.empty() ? frame_now : q_frame0 + q_frames; }
    void sync_lost_counter(); // device "lost pushes" counter -> ev_lost_total (synchronises the stream)
    TlEvent* h_stage_ev[EV_RING] = {};   // pinned
    uint32_t* h_stage_upd[EV_RING] = {}; // pinned, n x {voice, cursor, end}
    uint32_t* d_stage_upd[EV_RING] = {};
    uint64_t stage_seq[EV_RING] = {};         // batch (flush_seq) whose launch read staging slot i (0 = never used)
    uint64_t flush_seq = 0;                    // batches launched so far
    bool batch_staged = false;                 // the batch being assembled reads a host staging buffer
    volatile uint64_t* h_progress = nullptr;  // pinned: number of the last batch the stream has finished (og_stream_mark)
    float* h_bus_pinned = nullptr; // pinned + device-visible: destination of a blocking block's bus (og_process_block)
    bool blocking_memcpy = false; // OSCEN_GPU_BLOCKING_MEMCPY (A/B knob), read once at og_create
    uint64_t blocking_waits = 0, blocking_timeouts = 0; // og_process_block calls / calls whose marker wait timed out
    bool wait_progress(uint64_t seq) // false: the stream was found finished before the marker was seen
    {
        // the batch is tens of microseconds long: spin on the marker word (a runtime wait costs more than the block).
        // A marker that does not show is rare (twice in 44 000 blocks of 4 M voices, both a 20-30 ms block under the
        // earlier "give it 20 ms, then hipStreamSynchronize" rule): from 256 us on the stream itself is asked every
        // 128 us (hipStreamQuery does not block), so a late marker costs a fraction of a block, not several deadlines.
        using clk = std::chrono::steady_clock;
        const auto t0 = clk::now();
        auto next_query = t0 + std::chrono::microseconds(256);
        for (uint32_t spins = 0; !h_progress || *h_progress < seq; ++spins) {
            if ((spins & 255u) == 255u) {
                const auto now = clk::now();
                if (now >= next_query) {
                    const hipError_t q = hipStreamQuery(stream);
                    if (q == hipSuccess) return h_progress && *h_progress >= seq;
                    if (q != hipErrorNotReady) HIPCK(q);
                    next_query = now + std::chrono::microseconds(128);
                }
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
        return true;
    }
    bool batch_done(uint64_t seq)
    {
        if (seq == 0 || (h_progress && *h_progress >= seq)) return true;
        if (seq > flush_seq) return true; // (staged for a batch that was never launched: nothing read it)
        HIPCK(hipStreamSynchronize(stream)); // (a ring slot that is still in flight: never seen in practice)
        return true;
    }
    int stage_head = 0;
    uint32_t bus_passes = 0; // og_bus_reduce launches of the last block (1 + levels of the multi-pass tree)
    uint64_t frame_now = 0;

    bool bus_stage = true; // run the post-mix node (Tremolo) here; a cluster shard hands over the mono sum instead

    bool timing = false;
    std::vector<hipEvent_t> t_start, t_stop;
    unsigned long long* h_clock = nullptr; // pinned, [T_CLOCK][4]: {cycles, ticks} at the start and at the end of timed launch i
    static constexpr size_t T_CLOCK = 8192;
    size_t t_used = 0;
    size_t t_blocks = 0; // blocks the timed launches covered
    double last_clock_ghz = 0.0;

    ~og_engine();

    ogc::UEnv env() const { return ogc::UEnv{sr, values.data()}; }

    void upload_initial_state();
    size_t ring_bytes() const
    {
        size_t n = 0;
        for (size_t k = 0; k < cg->rings.size(); ++k) n += (size_t)ring_cap[k] * V * 4;
        return n;
    }

    void reset_timeline()
    {
        tl.reset();
        HIPCK(hipMemsetAsync(d_ev_cursor, 0, (size_t)V * 4, stream));
        HIPCK(hipMemsetAsync(d_ev_end, 0, (size_t)V * 4, stream));
    }

    // Blocks per launch for throughput callers (og_render*, cluster shards, og_set_bus_batching(e, 0)): as many as the
    // launch overhead still pays for while the launch's partial-sum rows stay modest.  Measured: fm_voice at 65 536 voices
    // gains 30 % from 1 -> 8 blocks and 3.5 % more from 8 -> 32 (32 MB of rows); sat4x_voice at 131 072 voices and sub_voice
    // at 262 144 LOSE 10-25 % once the rows of one launch pass ~64 MB, with either row layout (not understood further; those
    // banks run in several rounds of workgroups, where a longer launch makes the last round's tail longer).  The wide
    // four-wave form (`wide`: every workgroup resident in one round) is the other way round: a launch there takes everything
    // the caller queued, up to OG_MAX_QUEUE_BLOCKS blocks within OG_WIDE_ROW_BUDGET of rows -- fm_voice at 65 536 voices, six
    // launches of 32 blocks against one of 188: +2 % with the folded kernels (inside a run's spread), +11 % with the general
    // ones; part launch boundaries, part the end of every launch, where its dearest workgroups run on alone
    // (profiles/r13_launch_length.md).  Kept at 8..32 also there: graphs whose handlers read frame_offset (32 block-start
    // slots) and graphs with a post-mix Convolver (its rows grow with response x launch length).
    uint32_t auto_batch() const
    {
        const size_t per_block = (size_t)std::max<uint32_t>(n_wg, 1u) * 256u * 4u; // rows of one 256-frame block
        if (wide && !cg->reads_block_starts && cg->bus_stage != ogc::BusStage::Convolver) {
            const size_t b = OG_WIDE_ROW_BUDGET / (per_block * std::max<size_t>(cg->voice_channels, 1));
            return (uint32_t)std::min<size_t>(OG_MAX_QUEUE_BLOCKS, std::max<size_t>(8, b));
        }
        const size_t b = ((size_t)32 << 20) / per_block;
        return (uint32_t)std::min<size_t>(OG_MAX_LAUNCH_BLOCKS, std::max<size_t>(8, b));
    }
    // Frames one launch may cover under a queue limit of `blocks`.  1..32 blocks: full blocks, as ever.  Above: 256-frame
    // blocks (at 512 the rows of a 256-block queue on 1 024 workgroups would be 0.5 GB), never less than 32 full blocks.
    // The kernels themselves count frames, chunks and hand-off words in 32 bits and event offsets in 64; the one 32-bit
    // product on the way is OgBlockArgs::partial_plane (frames rounded to 16 x workgroups), which a Frame<2> bank reads.
    size_t launch_frames_cap(uint32_t blocks) const
    {
        if (blocks <= OG_MAX_LAUNCH_BLOCKS) return (size_t)OG_MAX_BLOCK * blocks;
        size_t f = std::max<size_t>(OG_MAX_LAUNCH_FRAMES, (size_t)256 * blocks);
        const size_t plane = (size_t)0xFFFFFFFFu / std::max<uint32_t>(n_wg, 1u) / OG_BUS_CHUNK * OG_BUS_CHUNK;
        if (cg->voice_channels > 1) f = std::max<size_t>(OG_MAX_LAUNCH_FRAMES, std::min(f, plane));
        return f;
    }
    // Everything before this frame has been consumed on the device by the time an update issued now takes effect:
    // launched blocks run before it in stream order; blocks still in the queue have not seen their events yet.
    uint64_t consumed_horizon() const { return queue.empty() ? frame_now : q_frame0; }
    void full_rebuild();
    // live pushes: O(#pushes) host work, asynchronous upload.  Returns false when the batch does not fit
    // (staging buffer, tail of d_events): the caller falls back to full_rebuild().
    bool incremental_update();
    // bring the device timeline up to date: right before the queued blocks are launched (their events may have arrived
    // over several blocks: one staging copy and one cursor update for all of them)
    void upload_events();

    // the longest release, in samples, of the outer-rate envelopes under these block-uniform slots
    uint32_t release_need(const uint32_t* slots) const
    {
        uint32_t need = 0;
        for (int k : cg->release_slots) need = std::max(need, slots[k]);
        return need;
    }
    // make the reciprocal table cover `need` entries (stream-ordered: the fill runs ahead of the launches that read it);
    // false when `need` is over the cap
    bool rcp_cover(uint32_t need);
    void alloc_bus_buffers(uint32_t batch);
    // process_block(frames), asynchronous: the block joins the queue; the queue is launched when it is full or when
    // something needs its results or is about to change what it would see
    void process_async(uint32_t frames, float* d_out);
    // launch the queued blocks: voice kernel over their frames, bus reduce (fixed-association tree: groups of 1024
    // rows, then, for > 1024 waves, the group sums), post-mix stage block by block
    void flush_bus();
    // og_cluster.cpp's post-mix Tremolo on the root device: the kernel is og_engine.cpp's
    static void launch_bus_tremolo(const float* mono, uint32_t frames, float rate, float depth, float sr, float* phase_state, float* out,
                                   hipStream_t stream);
};
