// og_engine.cpp -- host runtime of the voice-bank engine + the C ABI of
// include/oscen_gpu.h.  Compiled by hipcc (host side only; the kernels live in
// csrc/gen/*.hip and in og_kernel_rt.hip.h).
//
// An engine is the MI355X form of the reference's poly wrapper graph
// (examples/fm-synth/src/lib.rs:22-131): `voices = [Voice; N]`, every broadcast
// value input fanned out to all voices (ramped where declared `[ramp: N]`),
// per-voice `frequency`/`gate`, and `voices.out -> out` summed onto the bus.
#include "og_engine.h"
#include "og_math.h"
#include "og_bus_conv.hip.h"
#include "og_asset_resample.hip.h"
#define OG_NODE_ARRAY_FILL_KERNEL 1
#include "og_node_array.hip.h"

// Sum the per-workgroup partial rows (fixed association, no atomics).
// One workgroup per 16 frames, 64 row-slices x 16 frames = 1024 threads: thread (slice s, frame f) adds
// rows s, s+64, s+128, ... of its group of <= 1024 rows with eight independent accumulators -- its
// <= 16 loads are all in flight together, so the pass costs about two memory latencies (the rows
// were written by other XCDs, they come from HBM/MALL) -- then the 64 slice sums are folded 4 -> 1
// and 16 -> 1 through LDS.  History: 4 waves walking all rows 40 us; 16 slices x 64 frames 6.5 us.
#define OG_RED_SLICES 64
#define OG_RED_FRAMES 16
static_assert(OG_RED_FRAMES == OG_BUS_CHUNK, "og_bus_reduce reads the chunks og::bus_chunk_reduce writes");
#define OG_RED_GROUP 1024 // rows per workgroup; larger banks take a second pass over the group sums
// out_stride / out_off: the last pass of a stereo bus writes channel out_off of interleaved Frame<2> samples
__device__ __forceinline__ void og_bus_reduce_body(const float* __restrict__ partials, uint32_t n_rows, uint32_t frames,
                                                   float* __restrict__ out, uint32_t out_stride, uint32_t out_off)
{
    __shared__ float part[OG_RED_SLICES][OG_RED_FRAMES];
    __shared__ float quad[OG_RED_SLICES / 4][OG_RED_FRAMES];
    const uint32_t fx = threadIdx.x % OG_RED_FRAMES;
    const uint32_t slice = threadIdx.x / OG_RED_FRAMES;
    const uint32_t f = blockIdx.x * OG_RED_FRAMES + fx;
    const uint32_t row0 = blockIdx.y * OG_RED_GROUP;
    const uint32_t row1 = min(n_rows, row0 + OG_RED_GROUP);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // rows are chunk-major, [chunk][row][OG_RED_FRAMES] (og::bus_chunk_reduce): this workgroup's chunk is contiguous
    const float* __restrict__ chunk = partials + (size_t)blockIdx.x * n_rows * OG_RED_FRAMES;
    if (f < frames) {
        uint32_t r = row0 + slice;
        for (; r + 7 * OG_RED_SLICES < row1; r += 8 * OG_RED_SLICES) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += chunk[(size_t)(r + i * OG_RED_SLICES) * OG_RED_FRAMES + fx];
        }
        for (int i = 0; r < row1; r += OG_RED_SLICES, ++i) acc[i] += chunk[(size_t)r * OG_RED_FRAMES + fx];
    }
    part[slice][fx] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    __syncthreads();
    if (slice < OG_RED_SLICES / 4)
        quad[slice][fx] = (part[4 * slice][fx] + part[4 * slice + 1][fx]) + (part[4 * slice + 2][fx] + part[4 * slice + 3][fx]);
    __syncthreads();
    if (slice == 0 && f < frames) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < OG_RED_SLICES / 4; ++i) s[i & 3] += quad[i][fx];
        // group sums in the same layout, [chunk][group][OG_RED_FRAMES]; with one group that is the bus itself
        out[(((size_t)blockIdx.x * gridDim.y + blockIdx.y) * OG_RED_FRAMES + fx) * out_stride + out_off] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}

// og_shader_clock_ghz: one wave spins for `ticks` of the constant 100 MHz counter (s_memrealtime) and counts shader cycles
// (s_memtime: one tick per shader clock, MI355X_MICROARCH.md) over the same span
__global__ __launch_bounds__(64) void og_clock_probe(unsigned long long* out, unsigned ticks)
{
#ifndef OG_HOSTSIM
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c0 = __builtin_readcyclecounter();
    unsigned long long r1;
    do {
        r1 = __builtin_amdgcn_s_memrealtime();
    } while (r1 - r0 < ticks);
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) {
        out[0] = c1 - c0;
        out[1] = r1 - r0;
    }
#else
    if (threadIdx.x == 0) out[0] = out[1] = 0ull; // (the host simulator has no shader clock)
    (void)ticks;
#endif
}

__global__ __launch_bounds__(1024) void og_bus_reduce(const float* __restrict__ partials, uint32_t n_rows,
                                                      uint32_t frames, float* __restrict__ out, uint32_t out_stride, uint32_t out_off)
{
    og_bus_reduce_body(partials, n_rows, frames, out, out_stride, out_off);
}

// Post-mix Tremolo (examples/electric-piano/src/tremolo.rs:40-62) on the summed bus -> Frame<2>.
// The LFO phase recurrence `phase = fract(phase + rate/sr)` is serial but two ops per frame: lane 0
// runs it into LDS, then every frame computes its sine (bit-exact libm restatement) in parallel.
__global__ __launch_bounds__(512) void og_bus_tremolo(const float* __restrict__ mono, uint32_t frames, float rate,
                                                      float depth, float sr, float* __restrict__ phase_state,
                                                      float* __restrict__ out)
{
    __shared__ float ph[OG_MAX_BLOCK];
    if (threadIdx.x == 0) {
        float p = *phase_state;
        const float phase_increment = rate / sr;
        for (uint32_t f = 0; f < frames; ++f) {
            ph[f] = p;
            const float q = p + phase_increment;
            p = q - truncf(q);
        }
        *phase_state = p;
    }
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < frames; f += blockDim.x) {
        const float input = mono[f];
        const float lfo = og_sinf_exact(ph[f] * 2.0f * 3.14159274101257324f);
        const float scaled_depth = depth / 3.0f;
        const float pan = 0.5f + lfo * scaled_depth;
        out[2 * f] = input * pan;
        out[2 * f + 1] = input * (1.0f - pan);
    }
}

// Incremental event path: append the staged segments to the timeline and point the listed voices at them.
// `staged` and `upd` are PINNED HOST buffers read by the kernel itself: a kernel launch never waits for the stream,
// whereas hipMemcpyAsync of a small pinned buffer was measured to block until the stream had drained (~290 us with a
// batch of blocks in flight), which serialised the host's event preparation with the GPU.
// upd = n x {voice, cursor, end}
__global__ void og_apply_event_updates(const uint4* __restrict__ staged, uint32_t n_ev, uint4* __restrict__ timeline_tail,
                                       const uint32_t* __restrict__ upd, uint32_t n, uint32_t* __restrict__ cursor,
                                       uint32_t* __restrict__ end)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ev) timeline_tail[i] = staged[i]; // (OgEvent = 16 bytes)
    if (i < n) {
        const uint32_t v = upd[EV_UPD_WORDS * i];
        cursor[v] = upd[EV_UPD_WORDS * i + 1];
        end[v] = upd[EV_UPD_WORDS * i + 2];
    }
}

// Stream progress marker: launched after every batch of blocks, writes the batch number into a word of pinned host
// memory.  The host checks it before it reuses a staging buffer (event segments, ramp tables): hipEventSynchronize on an
// event recorded many launches earlier was measured to block until the whole stream had drained (~350 us per call with
// a batch in flight), which serialised the host's preparation of the next batch with the GPU.
__global__ void og_stream_mark(volatile uint64_t* host_word, uint64_t seq)
{
    __threadfence_system();
    __hip_atomic_store(const_cast<uint64_t*>(host_word), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- registry ---------------------------------------------------------------
OgKernelEntry*& og_kernel_registry_head()
{
    static OgKernelEntry* head = nullptr;
    return head;
}
OgLaunchFn og_find_kernel(uint64_t hash)
{
    for (OgKernelEntry* e = og_kernel_registry_head(); e; e = e->next)
        if (e->hash == hash) return e->launch;
    return nullptr;
}
OgOccupancyFn og_find_occupancy(uint64_t hash)
{
    for (OgKernelEntry* e = og_kernel_registry_head(); e; e = e->next)
        if (e->hash == hash) return e->occupancy;
    return nullptr;
}
OgZeroKernelEntry*& og_zero_kernel_registry_head()
{
    static OgZeroKernelEntry* head = nullptr;
    return head;
}
OgZeroLaunchFn og_find_zero_kernel(uint64_t hash, int tier)
{
    for (OgZeroKernelEntry* e = og_zero_kernel_registry_head(); e; e = e->next)
        if (e->hash == hash && e->tier == tier) return e->launch;
    return nullptr;
}

namespace {
thread_local std::string g_err;
}
namespace ogabi {
int set_error(int code, const std::string& m)
{
    try {
        g_err = m;
    } catch (...) { // (out of memory while recording the message: keep the code)
        g_err.clear();
    }
    return code;
}
// the form guard()'s catch handlers use: the std::string is built INSIDE the try (guard is noexcept: a bad_alloc while
// copying e.what() must not become std::terminate)
int set_error(int code, const char* m) noexcept
{
    try {
        g_err.assign(m ? m : "");
    } catch (...) {
        g_err.clear();
    }
    return code;
}
} // namespace ogabi

// ---- samples by name (og_register_sample): the process-wide registry (SampleData: og_engine.h) ------------------------
namespace {
// device memory that lives for one call
struct DeviceScratch {
    float* p = nullptr;
    explicit DeviceScratch(size_t floats) { HIPCK(hipMalloc(&p, std::max<size_t>(floats, 1) * 4)); }
    ~DeviceScratch() { if (p) (void)hipFree(p); }
    DeviceScratch(const DeviceScratch&) = delete;
    DeviceScratch& operator=(const DeviceScratch&) = delete;
};
std::map<std::string, std::shared_ptr<const SampleData>>& sample_registry()
{
    static std::map<std::string, std::shared_ptr<const SampleData>> R;
    return R;
}
std::mutex& sample_registry_lock()
{
    static std::mutex m;
    return m;
}
} // namespace
std::shared_ptr<const SampleData> lookup_sample(const std::string& name)
{
    std::lock_guard<std::mutex> lk(sample_registry_lock());
    auto it = sample_registry().find(name);
    return it == sample_registry().end() ? nullptr : it->second;
}
namespace {
// SamplePlayerConsumer::build (sample_player/mod.rs:38-50): the source's channels onto a player of `width` channels,
// frame-major -- one source channel broadcasts, otherwise target channel c takes source channel min(c, src_ch - 1)
void map_sample_channels(const SampleData& s, uint32_t width, float* dst)
{
    for (size_t t = 0; t < s.frames; ++t)
        for (uint32_t c = 0; c < width; ++c) {
            const uint32_t sc = s.channels == 1 ? 0u : std::min(c, s.channels - 1u);
            dst[t * width + c] = s.interleaved[t * s.channels + sc];
        }
}
} // namespace

// ---- og_engine: the methods that launch kernels or use the device headers above ---------------------------------------
// (re)size the history and the partial rows for responses of up to k taps and the current launch capacity, keeping the
// history; the stream is idle (callers launch the queue and wait first)
void og_engine::conv_alloc(size_t k)
{
    const size_t vc = cg->voice_channels;
    const BusConvolver::Sizing sz = bus_conv.size_for(k, cap_frames, vc);
    if (sz.new_hist) {
        float* n = nullptr;
        HIPCK(hipMalloc(&n, sz.len * vc * 4));
        HIPCK(hipMemsetAsync(n, 0, sz.len * vc * 4, stream));
        if (d_hist) {
            HIPCK(hipMemcpyAsync(n + sz.copy_to * vc, d_hist + sz.copy_from * vc, sz.copy_frames * vc * 4, hipMemcpyDeviceToDevice, stream));
            HIPCK(hipStreamSynchronize(stream));
            HIPCK(hipFree(d_hist));
        }
        d_hist = n;
    }
    if (sz.new_rows) {
        if (d_conv_rows) HIPCK(hipFree(d_conv_rows));
        d_conv_rows = nullptr;
        HIPCK(hipMalloc(&d_conv_rows, 2 * sz.rows_half * 4));
    }
    bus_conv.resized(sz);
    HIPCK(hipStreamSynchronize(stream));
}

// flush_bus, in front of the bus sum: the dry sum goes behind the history; when the buffer is full the newest frames move
// to its front first
float* og_engine::conv_place_dry(BusConvolver::Launch& l)
{
    const uint32_t ch = cg->voice_channels;
    l = bus_conv.plan_launch(q_frame0, q_frames, conv_fade_len());
    if (l.move) {
        const uint32_t n = (uint32_t)(l.move_frames * ch);
        hipLaunchKernelGGL(og_bus_conv_move, dim3((n + 255) / 256), dim3(256), 0, stream, d_hist + l.move_from * ch, d_hist + l.move_to * ch, n);
    }
    return d_hist + l.dry_at * ch;
}

// flush_bus, behind the bus sum: one pass per run of blocks queued under the same responses -- as a rule the whole launch
void og_engine::conv_stage(BusConvolver::Launch& l, float* wet)
{
    const uint32_t ch = cg->voice_channels, row_stride = bus_conv.row_stride();
    BusConvolver::Run run;
    while (bus_conv.next_run(l, queue, run)) {
        run.cur.rows = d_conv_rows;
        run.old.rows = d_conv_rows + bus_conv.rows_half();
        const float* x = d_hist + run.x_at * ch;
        for (const OgConvResponse* r : {&run.cur, &run.old})
            if (r->n_frames && r->n_taps)
                hipLaunchKernelGGL(og_bus_conv, dim3((r->n_frames + OG_CONV_F - 1) / OG_CONV_F, (r->n_taps + OG_CONV_S - 1) / OG_CONV_S, ch),
                                   dim3(OG_CONV_LANES), 0, stream, x, ch, *r, row_stride);
        hipLaunchKernelGGL(og_bus_conv_finish, dim3((run.nf + 255) / 256, ch), dim3(256), 0, stream, run.cur, run.old, ch, row_stride,
                           run.fade_pos, run.fade_len, wet + run.f0 * ch);
    }
    bus_conv.launched(l);
    HIPCK(hipGetLastError());
}

// og_set_bus_ir on an asset response (ConvolverConsumer::build -> MultiConvolverEngine::from_asset, convolution/mod.rs:335-351):
// every source channel conformed to the engine's rate by the load path's resampler (equal rates: as registered), then mapped
// onto the bus's channels -- a multi-channel response on a mono bus is averaged (to_mono), one source channel is ONE plane
// shared by every bus channel, otherwise bus channel c takes source channel min(c, channels - 1).  Every check comes before
// the device is touched; the engine's state is not changed here.  Waits for the stream (the host copy comes back).
std::shared_ptr<ConvIR> og_engine::conv_build_asset(const std::string& name, const ogc::IrAsset& a)
{
    const uint32_t rate = graph_rate("og_set_bus_ir");
    const bool conform = a.rate != rate;
    const OgResamplePlan plan = conform ? og_resample_plan(a.frames, a.rate, rate) : OgResamplePlan{};
    const uint64_t K = conform ? plan.out_len : a.frames;
    if (K > OG_CONV_MAX_TAPS)
        throw ogabi::Unsupported("impulse response '" + name + "' (" + std::to_string(a.frames) + " frames at " + std::to_string(a.rate) + " Hz) has " +
                                 std::to_string(K) + " taps per channel once conformed to " + std::to_string(rate) + " Hz (at most " + std::to_string(OG_CONV_MAX_TAPS) + ")");
    if (K == 0)
        throw ogabi::Error(OG_E_INVALID, "impulse response '" + name + "' (" + std::to_string(a.frames) + " frames at " + std::to_string(a.rate) + " Hz) is empty once conformed to " + std::to_string(rate) + " Hz");
    const uint32_t vc = cg->voice_channels;
    const bool downmix = vc == 1 && a.channels > 1;
    auto ir = std::make_shared<ConvIR>();
    ir->planes = (a.channels == 1 || vc == 1) ? 1u : vc;
    ir->taps.resize((size_t)ir->planes * K);
    DeviceScratch d_src(a.interleaved.size()), d_conf(conform ? (size_t)K * a.channels : 1);
    bounce.h2d(d_src.p, a.interleaved.data(), a.interleaved.size() * 4, stream);
    if (conform) og_resample_launch(d_src.p, a.frames, a.channels, plan, d_conf.p, stream);
    HIPCK(hipMalloc(&ir->d, ir->taps.size() * 4));
    conv_bufs.push_back(ir->d);
    hipLaunchKernelGGL(og_bus_ir_planes, dim3((unsigned)((K + 255) / 256), ir->planes), dim3(256), 0, stream, conform ? d_conf.p : d_src.p, (uint32_t)K,
                       a.channels, downmix ? 1u : 0u, 1.0f / (float)a.channels, ir->d);
    HIPCK(hipGetLastError());
    bounce.d2h(ir->taps.data(), ir->d, ir->taps.size() * 4, stream);
    return ir;
}

// the length a tagged sample has once conformed to `dst` (the checks of from_samples behind the resample)
uint32_t og_engine::conformed_frames(const std::string& name, const SampleData& sd, uint32_t dst)
{
    if (sd.rate == dst) return sd.frames;
    const OgResamplePlan p = og_resample_plan(sd.frames, sd.rate, dst);
    if (p.out_len == 0)
        throw ogabi::Error(OG_E_INVALID, "sample '" + name + "' (" + std::to_string(sd.frames) + " frames at " + std::to_string(sd.rate) + ") is empty once conformed to " + std::to_string(dst));
    if (p.out_len >= ((uint64_t)1 << 32)) throw ogabi::Error(OG_E_NOMEM, "og_load_sample: the engine's sample pool is limited to 2^32 floats");
    return (uint32_t)p.out_len;
}

// brings a registered sample onto the device (every width the players have); returns its index
uint32_t og_engine::load_sample(const std::string& name, const SampleData& sd)
{
    flush_bus();
    HIPCK(hipStreamSynchronize(stream)); // (launches in flight read the pool and the table)
    LoadedSample ls;
    ls.name = name;
    ls.frames = sd.frames;
    ls.channels = sd.channels;
    ls.src_rate = sd.rate;
    ls.rate = sd.rate ? graph_rate("og_load_sample") : 0u;
    ls.pool_frames = sd.rate ? conformed_frames(name, sd, ls.rate) : sd.frames;
    const bool conform = sd.rate && sd.rate != ls.rate; // (an equal rate takes the untagged path)
    bool widths[5] = {false, false, false, false, false};
    size_t need = pool_used;
    for (const auto& pl : cg->players)
        if (!widths[pl.channels]) {
            widths[pl.channels] = true;
            need += (size_t)ls.pool_frames * pl.channels;
        }
    if (need >= ((size_t)1 << 32)) throw ogabi::Error(OG_E_NOMEM, "og_load_sample: the engine's sample pool is limited to 2^32 floats");
    pool_reserve(need);
    if (conform) { // the source goes up once; conformed and mapped on the device, straight into the pool
        const OgResamplePlan plan = og_resample_plan(sd.frames, sd.rate, ls.rate);
        DeviceScratch d_src(sd.interleaved.size()), d_conf((size_t)ls.pool_frames * sd.channels);
        bounce.h2d(d_src.p, sd.interleaved.data(), sd.interleaved.size() * 4, stream);
        og_resample_launch(d_src.p, sd.frames, sd.channels, plan, d_conf.p, stream);
        for (uint32_t w = 1; w <= 4; ++w) {
            if (!widths[w]) continue;
            ls.off[w] = (uint32_t)pool_used;
            og_map_channels_launch(d_conf.p, ls.pool_frames, sd.channels, w, d_pool + pool_used, stream);
            pool_used += (size_t)ls.pool_frames * w;
        }
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(stream));
    }
    std::vector<float> mapped;
    for (uint32_t w = 1; w <= 4 && !conform; ++w) {
        if (!widths[w]) continue;
        ls.off[w] = (uint32_t)pool_used;
        mapped.resize((size_t)sd.frames * w);
        map_sample_channels(sd, w, mapped.data());
        if (!mapped.empty()) bounce.h2d(d_pool + pool_used, mapped.data(), mapped.size() * 4, stream);
        HIPCK(hipStreamSynchronize(stream));
        pool_used += mapped.size();
    }
    samples.push_back(ls);
    upload_desc();
    return (uint32_t)samples.size() - 1;
}

og_engine::~og_engine()
{
    prof.report();
    (void)hipSetDevice(device);
    // a borrowed stream (og_set_stream) may already be gone: wait for the device instead of touching it
    if (own_stream && stream) (void)hipStreamSynchronize(stream);
    else (void)hipDeviceSynchronize();
    bounce.release();
    (void)hipFree(d_state);
    (void)hipFree(d_lane_state);
    for (int k = 0; k < OG_MAX_RINGS; ++k) (void)hipFree(d_ring[k]);
    (void)hipFree(d_mono);
    (void)hipFree(d_bus_phase);
    (void)hipFree(d_pm_state);
    for (int k = 0; k < OG_MAX_RINGS; ++k) (void)hipFree(d_pm_ring[k]);
    (void)hipFree(d_pm_in);
    (void)hipFree(d_pm_ev);
    (void)hipFree(d_hist);
    (void)hipFree(d_conv_rows);
    for (float* p : conv_bufs) (void)hipFree(p);
    (void)hipFree(d_events);
    (void)hipFree(d_ev_end);
    (void)hipFree(d_ev_cursor);
    (void)hipFree(d_partials);
    (void)hipFree(d_partials2);
    (void)hipFree(d_rcp);
    (void)hipFree(d_pool);
    (void)hipFree(d_desc);
    for (float* p : rcp_old) (void)hipFree(p);
    (void)hipFree(d_stage_bus);
    (void)hipFree(d_bus);
    (void)hipFree(d_taps);
    (void)hipFree(d_tap_slot);
    (void)hipFree(d_narr);
    (void)hipFree(d_out_ev);
    (void)hipFree(d_out_ev_count);
    for (int i = 0; i < RAMP_RING; ++i) {
        (void)hipFree(d_ramp[i]);
        if (h_ramp[i]) (void)hipHostFree(h_ramp[i]);
    }
    for (int i = 0; i < EV_RING; ++i) {
        if (h_stage_ev[i]) (void)hipHostFree(h_stage_ev[i]);
        if (h_stage_upd[i]) (void)hipHostFree(h_stage_upd[i]);
        (void)hipFree(d_stage_upd[i]);
    }
    if (h_progress) (void)hipHostFree((void*)h_progress);
    if (h_bus_pinned) (void)hipHostFree(h_bus_pinned);
    if (h_clock) (void)hipHostFree(h_clock);
    for (auto ev : t_start) (void)hipEventDestroy(ev);
    for (auto ev : t_stop) (void)hipEventDestroy(ev);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

void og_engine::narr_fill()
{
    for (const auto& f : cg->arrays) {
        const size_t n = (size_t)f.length * V;
        const size_t threads = std::max<size_t>(3, (n + 3) / 4); // (og_node_array_fill: the 16-byte body and up to 3 words at either end)
        hipLaunchKernelGGL(og_node_array_fill, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, d_narr + (size_t)f.base * V, n, f.init);
        HIPCK(hipGetLastError());
    }
    narr_dirty = false;
}

void og_engine::upload_initial_state()
{
    const size_t nw = cg->state.size();
    std::vector<uint32_t> img(nw * (size_t)V);
    ogc::UEnv e = env();
    for (size_t w = 0; w < nw; ++w) {
        const uint32_t bits = cg->state[w].init(e);
        std::fill(img.begin() + w * V, img.begin() + (w + 1) * V, bits);
    }
    bounce.h2d(d_state, img.data(), img.size() * 4, stream);
    std::vector<uint32_t> limg;
    if (!cg->lane_state.empty()) {
        const size_t per = (size_t)V * cg->lpv * cg->lane_width;
        limg.resize(cg->lane_state.size() * per);
        for (size_t k = 0; k < cg->lane_state.size(); ++k)
            std::fill(limg.begin() + k * per, limg.begin() + (k + 1) * per, cg->lane_state[k].init(e));
        bounce.h2d(d_lane_state, limg.data(), limg.size() * 4, stream);
    }
    if (d_bus_phase) HIPCK(hipMemsetAsync(d_bus_phase, 0, 4, stream));
    conv_reset();
    // prepare(): every Delay gets a fresh zeroed ring sized from the sample rate (delay/mod.rs:59-69)
    for (size_t k = 0; k < cg->rings.size(); ++k) {
        const uint32_t cap = cg->rings[k].capacity(sr);
        if (cap != ring_cap[k]) {
            if (d_ring[k]) HIPCK(hipFree(d_ring[k]));
            d_ring[k] = nullptr;
            ring_cap[k] = 0;
            HIPCK(hipMalloc(&d_ring[k], (size_t)cap * V * 4));
            ring_cap[k] = cap;
        }
        HIPCK(hipMemsetAsync(d_ring[k], 0, (size_t)cap * V * 4, stream));
    }
    narr_fill(); // every array field of a registered node type holds its `init`
    pm_reset();
    HIPCK(hipStreamSynchronize(stream));
}

// the post-mix graph's state image: one voice
void og_engine::pm_reset()
{
    if (!post_on()) return;
    const ogc::CompiledGraph& p = *cg->post;
    const ogc::UEnv e = pm_env();
    std::vector<uint32_t> img(p.state.size());
    for (size_t w = 0; w < img.size(); ++w) img[w] = p.state[w].init(e);
    if (!img.empty()) HIPCK(hipMemcpyAsync(d_pm_state, img.data(), img.size() * 4, hipMemcpyHostToDevice, stream));
    for (size_t k = 0; k < p.rings.size(); ++k) {
        const uint32_t cap = p.rings[k].capacity(sr);
        if (cap != pm_ring_cap[k]) {
            if (d_pm_ring[k]) HIPCK(hipFree(d_pm_ring[k]));
            d_pm_ring[k] = nullptr;
            pm_ring_cap[k] = 0;
            HIPCK(hipMalloc(&d_pm_ring[k], (size_t)cap * 4));
            pm_ring_cap[k] = cap;
        }
        HIPCK(hipMemsetAsync(d_pm_ring[k], 0, (size_t)cap * 4, stream));
    }
    HIPCK(hipStreamSynchronize(stream)); // (the image dies here)
}

// ---- event timeline: the device halves of og_timeline.h's two update paths ---------------------------------------------
void og_engine::full_rebuild()
{
    HostProf::Scope ps(prof, HostProf::REBUILD);
    EventTimeline::Rebuild r = tl.plan_rebuild(consumed_horizon(), d_events != nullptr);
    const size_t n = r.events.size();
    if (r.realloc) {
        if (d_events) HIPCK(hipFree(d_events));
        d_events = nullptr;
        if (!r.capacity) throw ogabi::Error(OG_E_NOMEM, "event timeline + og_reserve_events exceed the 32-bit event ring");
        HIPCK(hipMalloc(&d_events, r.capacity * sizeof(OgEvent)));
    }
    if (n) bounce.h2d(d_events, r.events.data(), n * sizeof(OgEvent), stream);
    bounce.h2d(d_ev_cursor, r.cursor.data(), (size_t)V * 4, stream);
    bounce.h2d(d_ev_end, r.end.data(), (size_t)V * 4, stream);
    HIPCK(hipStreamSynchronize(stream)); // the staging vectors die here
    tl.adopt(r);
}

bool og_engine::incremental_update()
{
    HostProf::Scope ps(prof, HostProf::INCREMENTAL);
    if (!h_stage_ev[0]) {
        for (int i = 0; i < EV_RING; ++i) {
            HIPCK(hipHostMalloc((void**)&h_stage_ev[i], tl.stage_events() * sizeof(OgEvent), hipHostMallocDefault));
            HIPCK(hipHostMalloc((void**)&h_stage_upd[i], tl.stage_events() * EV_UPD_WORDS * 4, hipHostMallocDefault));
        }
    }
    const int r = stage_head;
    {
        HostProf::Scope pw(prof, HostProf::EV_WAIT);
        batch_done(stage_seq[r]); // (EV_RING batches ago: long done)
    }
    TlEvent* sev = h_stage_ev[r];
    uint32_t* upd = h_stage_upd[r];
    const EventTimeline::Batch b = tl.plan_incremental(sev, upd, consumed_horizon(), launch_end());
    if (!b) return false;
    if (b.n_upd == 0) return true; // (every due entry was stale, nothing was pushed: no kernel to launch)
    // commit: host mirror, then the device
    HostProf::Scope pc(prof, HostProf::EV_COMMIT);
    tl.commit_incremental(b, sev, upd);
    static_assert(sizeof(OgEvent) == sizeof(uint4), "og_apply_event_updates copies events as 16-byte words");
    const uint32_t n_wg_upd = (uint32_t)((std::max(b.n_upd, b.n_ev) + 255) / 256);
    hipLaunchKernelGGL(og_apply_event_updates, dim3(n_wg_upd), dim3(256), 0, stream, (const uint4*)sev, (uint32_t)b.n_ev,
                       (uint4*)(d_events + b.base), (const uint32_t*)upd, (uint32_t)b.n_upd, d_ev_cursor, d_ev_end);
    HIPCK(hipGetLastError());
    stage_seq[r] = flush_seq + 1; // read in stream order before the batch that is about to be launched
    batch_staged = true;
    stage_head = (stage_head + 1) % EV_RING;
    return true;
}

void og_engine::upload_events()
{
    if (!tl.needs_upload(launch_end())) return;
    EventTimeline::HoldLocal hold(tl); // (block-local pushes of the block being assembled stay on the host)
    if (!tl.needs_upload(launch_end())) return;
    HostProf::Scope ps(prof, HostProf::SYNC_EVENTS);
    // many voices touched at once (bulk scheduling): one compact CSR rebuild beats per-voice segments
    const bool bulk = tl.wants_rebuild() || tl.n_pending() > tl.stage_events() || tl.n_pending() > (size_t)V / 2 + 64 || !d_events;
    if (bulk || !incremental_update()) full_rebuild();
}

bool og_engine::rcp_cover(uint32_t need)
{
    if (need > rcp_cap) return false;
    if (need <= rcp_n) return true;
    const uint32_t n = std::min(rcp_cap, std::max(need, 2 * rcp_n));
    float* t = nullptr;
    HIPCK(hipMalloc(&t, ((size_t)OG_RCP_PAD + n + 1) * sizeof(float)));
    const uint32_t words = OG_RCP_PAD + n + 1;
    hipLaunchKernelGGL(og::rcp_table_fill<0>, dim3((words + 255) / 256), dim3(256), 0, stream, t, n);
    HIPCK(hipGetLastError());
    if (d_rcp) rcp_old.push_back(d_rcp);
    d_rcp = t;
    rcp_n = n;
    return true;
}

void og_engine::alloc_bus_buffers(uint32_t batch)
{
    HIPCK(hipStreamSynchronize(stream));
    for (float** p : {&d_partials, &d_partials2, &d_mono, &d_stage_bus, &d_pm_in})
        if (*p) {
            HIPCK(hipFree(*p));
            *p = nullptr;
        }
    cap_frames = launch_frames_cap(batch);
    const size_t max_frames = cap_frames;
    const size_t vc = cg->voice_channels; // a Frame<2> voice output: two planes of partial rows
    HIPCK(hipMalloc(&d_partials, (size_t)n_wg * max_frames * 4 * vc));
    HIPCK(hipMemset(d_partials, 0, (size_t)n_wg * max_frames * 4 * vc));
    HIPCK(hipMalloc(&d_partials2, ((size_t)n_wg / OG_RED_GROUP + 2 + 64) * max_frames * 4));
    HIPCK(hipMalloc(&d_stage_bus, max_frames * OG_MAX_BUS_CHANNELS * 4));
    if (cg->bus_stage == ogc::BusStage::Tremolo) HIPCK(hipMalloc(&d_mono, max_frames * 4));
    if (cg->bus_stage == ogc::BusStage::Convolver) conv_alloc(bus_conv.longest_taps());
    if (post_on()) { // the rows the last reduce pass writes and the post-mix kernel reads in whole 16-frame chunks (cap_frames is a multiple)
        HIPCK(hipMalloc(&d_pm_in, max_frames * vc * 4));
        HIPCK(hipMemset(d_pm_in, 0, max_frames * vc * 4));
        pm_last_frames = 0;
    }
    const size_t rows = (size_t)(cg->n_ramps + cg->n_streams);
    for (int i = 0; i < RAMP_RING && rows; ++i) {
        if (d_ramp[i]) HIPCK(hipFree(d_ramp[i]));
        if (h_ramp[i]) HIPCK(hipHostFree(h_ramp[i]));
        d_ramp[i] = h_ramp[i] = nullptr;
        HIPCK(hipMalloc(&d_ramp[i], rows * max_frames * 4));
        HIPCK(hipHostMalloc((void**)&h_ramp[i], rows * max_frames * 4, hipHostMallocDefault));
        ramp_seq[i] = 0;
    }
}

void og_engine::process_async(uint32_t frames, float* d_out)
{
    HIPCK(hipSetDevice(device));
    tl.drop_late_local(frame_now + frames);
    // events wait on the host until the queue is launched: launch it before they outgrow the staging buffers (or the
    // size up to which per-voice segments beat a rebuild of the whole timeline)
    if (!queue.empty() && tl.n_pending() > std::min<size_t>(tl.stage_events() / 2, (size_t)V / 4 + 32)) flush_bus();
    // the buffers hold cap_frames frames per launch (a queue of up to 32 blocks never reaches this: its capacity is 32 full blocks)
    if (!queue.empty() && (size_t)q_frames + frames > cap_frames) flush_bus();
    if (queue.empty()) {
        q_frame0 = frame_now;
        q_frames = 0;
        q_ramps = cg->n_streams > 0;
        q_ramp_slot = -1;
    }
    // tick_ramps (codegen/mod.rs:878-914): the value seen by frame f is the one after f+1 ticks.  The same
    // per-frame table carries the graph's stream inputs (`<stream_in>_block`, one row each, broadcast to every
    // voice); a graph with stream inputs always runs the table-reading kernel variant.
    const size_t stride = cap_frames;
    const bool ramping = active_ramps > 0 && cg->n_ramps > 0;
    if ((ramping || cg->n_streams > 0 || q_ramps) && cg->n_ramps + cg->n_streams > 0) {
        if (q_ramp_slot < 0) { // first block of the queue that needs the table: earlier blocks get constant rows
            q_ramp_slot = ramp_head;
            ramp_head = (ramp_head + 1) % RAMP_RING;
            batch_done(ramp_seq[q_ramp_slot]);
            float* tab0 = h_ramp[q_ramp_slot];
            for (size_t i = 0; i < cg->inputs.size(); ++i) {
                const int row = cg->inputs[i].ramp_row;
                if (row >= 0) std::fill(tab0 + (size_t)row * stride, tab0 + (size_t)row * stride + q_frames, ramps[i].current);
            }
        }
        q_ramps = true;
        float* tab = h_ramp[q_ramp_slot];
        for (uint32_t f = 0; f < frames; ++f) {
            for (size_t i = 0; i < cg->inputs.size(); ++i) {
                const int row = cg->inputs[i].ramp_row;
                if (row < 0) continue;
                if (active_ramps > 0 && ramps[i].tick()) active_ramps -= 1;
                tab[(size_t)row * stride + q_frames + f] = ramps[i].current;
            }
        }
        for (size_t i = 0; i < cg->inputs.size(); ++i) {
            if (cg->inputs[i].ramp_row >= 0) values[i] = ramps[i].current;
            const int srow = cg->inputs[i].stream_row;
            for (int k = 0; srow >= 0 && k < std::max(1, cg->inputs[i].decl.channels); ++k) // (planar: one row per channel)
                memcpy(tab + (size_t)(srow + k) * stride + q_frames, stream_blocks[i].data() + (size_t)k * OG_MAX_BLOCK, (size_t)frames * 4);
        }
    }
    QueuedBlock qb;
    qb.dst = d_out ? d_out : d_bus;
    qb.frames = frames;
    qb.trem_rate = qb.trem_depth = 0.0f;
    qb.conv = 0;
    if (conv_on()) qb.conv = bus_conv.queue_block(frame_now, conv_fade_len()); // voices.output -> reverb.input; reverb.output -> out
    if (cg->bus_stage == ogc::BusStage::Tremolo && bus_stage) { // voices.output -> tremolo.input; tremolo.output -> out (Frame<2>)
        ogc::UEnv ev = env();
        qb.trem_rate = cg->tremolo_rate(ev);
        qb.trem_depth = cg->tremolo_depth(ev);
    }
    queue.push_back(qb);
    q_frames += frames;
    frame_now += frames;
    last_frames = frames;
    // The last ramp ended inside this block: launch what is queued, so that the blocks that follow -- nothing moves in
    // them -- start a queue of their own on the kernel variant that does not read the table.  (Round 6, the moving-cutoff
    // variant of the bench: the launch that held the 2 205-frame cutoff ramp also held the ~20 quiet blocks queued behind
    // it and ran them 35 % slower -- per-frame parameter tests, table reads -- than the `_00` variant; a launch costs 25 us.)
    const bool ramps_done = ramping && active_ramps == 0 && cg->n_streams == 0;
    if (queue.size() >= bus_batch || n_taps > 0 || ramps_done) flush_bus();
}

void og_engine::flush_bus()
{
    if (queue.empty()) return;
    upload_events(); // (before the launch arguments are formed: a rebuild may move the timeline)
    HostProf::Scope ps(prof, HostProf::LAUNCH);
    OgBlockArgs A;
    memset(&A, 0, sizeof A);
    A.n_voices = V;
    A.frames = q_frames;
    A.ramp_stride = (uint32_t)cap_frames;
    A.lanes = lanes;
    A.split = split;
    A.wide = wide ? 1u : 0u;
    A.frame0 = q_frame0;
    A.state = d_state;
    A.lane_state = d_lane_state;
    A.lane_dump = d_lane_state ? d_lane_state + cg->lane_state.size() * (size_t)V * cg->lpv * cg->lane_width : nullptr;
    A.events = d_events;
    A.ev_end = d_ev_end;
    A.ev_cursor = d_ev_cursor;
    A.partials = d_partials;
    const uint32_t n_chunks16 = (q_frames + OG_RED_FRAMES - 1) / OG_RED_FRAMES;
    A.partial_plane = (uint32_t)((size_t)n_chunks16 * n_wg * OG_RED_FRAMES);
    A.taps = d_taps;
    A.tap_slot = d_tap_slot;
    A.out_ev = d_out_ev;
    A.out_ev_cap = out_ev_cap;
    A.out_ev_count = d_out_ev ? d_out_ev_count : nullptr;
    A.ev_lost = d_out_ev_count ? d_out_ev_count + 1 : nullptr;
    for (size_t k = 0; k < cg->rings.size(); ++k) {
        A.rings[k] = d_ring[k];
        A.ring_cap[k] = ring_cap[k];
    }
    // block-uniform slots: the values the queued blocks were queued under (a setter launches the queue before it
    // changes one; ramped inputs are read from the table whenever a ramp moved inside the queue)
    {
        ogc::UEnv e = env();
        uint32_t starts[OG_MAX_LAUNCH_BLOCKS + 1];
        uint32_t acc = 0, nb = 0;
        for (const QueuedBlock& qb : queue) {
            if (nb < OG_MAX_LAUNCH_BLOCKS) starts[nb++] = acc;
            acc += qb.frames;
        }
        e.block_starts = starts;
        e.n_blocks = nb;
        for (const auto& up : cg->uprogs) A.slots[up.dst] = up.fn(e);
    }
    if (cg->player_slot0 >= 0) { // SamplePlayer: the pool and the descriptor table (og_sample_player.hip.h)
        uint32_t* ps = A.slots + cg->player_slot0;
        ps[0] = (uint32_t)((uintptr_t)d_pool & 0xFFFFFFFFu);
        ps[1] = (uint32_t)((uint64_t)(uintptr_t)d_pool >> 32);
        ps[2] = (uint32_t)((uintptr_t)d_desc & 0xFFFFFFFFu);
        ps[3] = (uint32_t)((uint64_t)(uintptr_t)d_desc >> 32);
        ps[4] = sample_cap;
    }
    if (cg->narr_slot0 >= 0) { // array fields of registered node types: the pool (og_node_array.hip.h)
        A.slots[cg->narr_slot0] = (uint32_t)((uintptr_t)d_narr & 0xFFFFFFFFu);
        A.slots[cg->narr_slot0 + 1] = (uint32_t)((uint64_t)(uintptr_t)d_narr >> 32);
    }
    if (rcp_cover(release_need(A.slots))) {
        A.rcp_tab = d_rcp;
        A.rcp_len = rcp_n;
    }
    const bool ramps_on = q_ramps && q_ramp_slot >= 0;
    if (ramps_on) {
        const int r = q_ramp_slot;
        const size_t rows = (size_t)(cg->n_ramps + cg->n_streams);
        HIPCK(hipMemcpyAsync(d_ramp[r], h_ramp[r], rows * A.ramp_stride * 4, hipMemcpyHostToDevice, stream));
        ramp_seq[r] = flush_seq + 1;
        batch_staged = true;
        A.ramp_table = d_ramp[r];
    }
    const bool taps_on = n_taps > 0;
    const bool timed = timing && t_used < 8192; // (a host that never collects the timings stops adding events)
    if (timed) {
        if (t_used == t_start.size()) {
            hipEvent_t a, b;
            HIPCK(hipEventCreate(&a));
            HIPCK(hipEventCreate(&b));
            t_start.push_back(a);
            t_stop.push_back(b);
        }
        HIPCK(hipEventRecord(t_start[t_used], stream));
        if (!h_clock) {
            HIPCK(hipHostMalloc((void**)&h_clock, T_CLOCK * 4 * sizeof(unsigned long long), hipHostMallocDefault));
            memset(h_clock, 0, T_CLOCK * 4 * sizeof(unsigned long long));
        }
        A.clock_out = h_clock + 4 * t_used; // (pinned host memory is device-visible: four 8-byte stores per launch)
    }
    // The zero variant (og_graph.cpp, ZeroChain): every block of this launch was queued under these slot values (a setter
    // launches the queue before it changes one) and no ramp ticks in it, so a zero slot here is +-0 on every frame.
    bool zero = zero_spec && !ramps_on && !cg->zero_slots.empty();
    for (int zs : cg->zero_slots) zero = zero && (A.slots[zs] & 0x7fffffffu) == 0u;
    // The deeper zero variant (ZeroFolds) also needs finite operator levels -- in this launch and in every one before it:
    // an inf or NaN an earlier launch left in an operator's prev_output stays there under the general kernel (NaN * 0).
    for (int fs : cg->finite_slots) guards_held = guards_held && (A.slots[fs] & 0x7f800000u) != 0x7f800000u;
    bool zero2 = zero_spec && zero2_spec && guards_held && !ramps_on && !cg->zero2_slots.empty();
    for (int zs : cg->zero2_slots) zero2 = zero2 && (A.slots[zs] & 0x7fffffffu) == 0u;
    last_zero = false;
    last_tier = 0;
    // (OSCEN_GPU_STAGE_SPEC=0: the deeper variant without its stage-uniform envelope bodies -- the switch is the last uniform
    //  slot, which a graph that has the bodies does not use, og_stage_uniform.hip.h; the other kernels never read it)
    if (zero2 && !stage_spec && cg->stage_spec) A.slots[OG_MAX_SLOTS - 1] = 1u;
    if (zero2 && (launch ? launch_zero2 != nullptr : jit->launch_zero2(A, taps_on, stream))) {
        if (launch) launch_zero2(A, taps_on, stream);
        last_zero = true;
        last_tier = 2;
    } else if (launch && zero && launch_zero) {
        launch_zero(A, taps_on, stream);
        last_zero = true;
    } else if (launch) {
        launch(A, ramps_on, taps_on, stream);
    } else if (zero) {
        last_zero = jit->launch_zero(A, taps_on, stream);
    } else {
        jit->launch(A, ramps_on, taps_on, stream);
    }
    if (last_zero && last_tier == 0) last_tier = 1;
    if (timed) {
        HIPCK(hipEventRecord(t_stop[t_used], stream));
        ++t_used;
        t_blocks += queue.size();
    }
    HIPCK(hipGetLastError());
    // ---- bus: sum the partial rows ----------------------------------------------------------------
    const bool post_mix = cg->bus_stage == ogc::BusStage::Tremolo && bus_stage;
    const bool post_conv = conv_on();
    const uint32_t ch = cg->voice_channels; // summed voices: mono, or Frame<2> voices (a post-mix node writes its Frame<2> bus itself)
    const bool post_graph = post_on(); // the post-mix kernel writes the bus (cg->channels wide) where the last reduce pass would have
    const uint32_t och = post_graph ? cg->channels : ch;
    bool contiguous = !post_mix;
    for (size_t k = 1; k < queue.size() && contiguous; ++k)
        contiguous = queue[k].dst == queue[k - 1].dst + (size_t)queue[k - 1].frames * och;
    float* sum_dst = post_mix ? d_mono : (contiguous ? queue[0].dst : d_stage_bus);
    float* const wet_dst = sum_dst;
    BusConvolver::Launch conv_launch{};
    if (post_conv) sum_dst = conv_place_dry(conv_launch);
    for (uint32_t c = 0; c < ch; ++c) { // one tree per channel plane; the last pass interleaves Frame<2> samples
        const float* src = d_partials + (size_t)c * A.partial_plane;
        uint32_t rows = n_wg;
        float* tmp = d_partials2;
        bus_passes = 1;
        while (rows > OG_RED_GROUP) {
            bus_passes += 1;
            const uint32_t groups = (rows + OG_RED_GROUP - 1) / OG_RED_GROUP;
            hipLaunchKernelGGL(og_bus_reduce, dim3(n_chunks16, groups), dim3(1024), 0, stream, src, rows, q_frames, tmp, 1u, 0u);
            src = tmp;
            rows = groups;
            tmp = tmp + (size_t)groups * n_chunks16 * OG_RED_FRAMES; // next level writes behind this one
        }
        if (post_graph) // planar, straight into the rows the post-mix kernel reads
            hipLaunchKernelGGL(og_bus_reduce, dim3(n_chunks16, 1), dim3(1024), 0, stream, src, rows, q_frames, d_pm_in + (size_t)c * cap_frames, 1u, 0u);
        else
            hipLaunchKernelGGL(og_bus_reduce, dim3(n_chunks16, 1), dim3(1024), 0, stream, src, rows, q_frames, sum_dst, ch, c);
    }
    HIPCK(hipGetLastError());
    if (post_graph) { // the nodes behind the sum: one wave over all q_frames of the launch, into the destination
        const ogc::CompiledGraph& p = *cg->post;
        OgBlockArgs P;
        memset(&P, 0, sizeof P);
        P.n_voices = 1;
        P.frames = q_frames;
        P.ramp_stride = (uint32_t)cap_frames;
        P.lanes = OG_WAVE;
        P.frame0 = q_frame0;
        P.state = d_pm_state;
        P.ev_cursor = d_pm_ev;
        P.ev_end = d_pm_ev + 1;
        P.ramp_table = A.ramp_table; // (the post-mix graph declares the wrapper's broadcast inputs in order: the same ramp rows)
        for (size_t k = 0; k < p.rings.size(); ++k) {
            P.rings[k] = d_pm_ring[k];
            P.ring_cap[k] = pm_ring_cap[k];
        }
        const ogc::UEnv pe = pm_env();
        for (const auto& up : p.uprogs) P.slots[up.dst] = up.fn(pe);
        uint32_t* io = P.slots + p.pm_slot0;
        io[0] = (uint32_t)((uintptr_t)d_pm_in & 0xFFFFFFFFu);
        io[1] = (uint32_t)((uint64_t)(uintptr_t)d_pm_in >> 32);
        io[2] = (uint32_t)((uintptr_t)wet_dst & 0xFFFFFFFFu);
        io[3] = (uint32_t)((uint64_t)(uintptr_t)wet_dst >> 32);
        io[4] = (uint32_t)cap_frames;
        pm_jit->launch(P, ramps_on && p.n_ramps > 0, false, stream);
        pm_last_frames = q_frames;
        HIPCK(hipGetLastError());
    }
    if (post_conv) conv_stage(conv_launch, wet_dst);
    size_t off = 0;
    for (const QueuedBlock& qb : queue) {
        if (post_mix) {
            hipLaunchKernelGGL(og_bus_tremolo, dim3(1), dim3(512), 0, stream, d_mono + off, qb.frames, qb.trem_rate, qb.trem_depth, sr,
                               d_bus_phase, qb.dst);
        } else if (!contiguous) {
            HIPCK(hipMemcpyAsync(qb.dst, d_stage_bus + off * och, (size_t)qb.frames * och * 4, hipMemcpyDeviceToDevice, stream));
        }
        off += qb.frames;
    }
    HIPCK(hipGetLastError());
    flush_seq += 1;
    if (batch_staged) { // this batch read a host staging buffer: tell the host when the stream is past it
        if (!h_progress) {
            HIPCK(hipHostMalloc((void**)&h_progress, 64, hipHostMallocCoherent)); // (fine-grained: a device store is visible to the host while the stream runs)
            *h_progress = 0;
        }
        hipLaunchKernelGGL(og_stream_mark, dim3(1), dim3(1), 0, stream, h_progress, flush_seq);
        HIPCK(hipGetLastError());
        batch_staged = false;
    }
    queue.clear();
    q_frames = 0;
}

void og_engine::launch_bus_tremolo(const float* mono, uint32_t frames, float rate, float depth, float sr, float* phase_state, float* out,
                                   hipStream_t stream)
{
    hipLaunchKernelGGL(og_bus_tremolo, dim3(1), dim3(512), 0, stream, mono, frames, rate, depth, sr, phase_state, out);
}

namespace {

int check_value_input(const og_engine* e, uint32_t input, bool per_voice)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (input >= e->cg->inputs.size()) return set_err(OG_E_INVALID, "input index out of range");
    const auto& in = e->cg->inputs[input];
    if (in.decl.kind != ogc::Kind::Value) return set_err(OG_E_INVALID, "'" + in.decl.name + "' is not a value input");
    if (in.decl.per_voice != per_voice)
        return set_err(OG_E_INVALID, "'" + in.decl.name + (per_voice ? "' is a broadcast input" : "' is a per-voice input"));
    return OG_OK;
}

int push_event(og_engine* e, uint32_t input, uint32_t voice, uint64_t frame, float value, bool local, bool setvalue)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (input >= e->cg->inputs.size()) return set_err(OG_E_INVALID, "input index out of range");
    if (voice >= e->V) return set_err(OG_E_INVALID, "voice index out of range");
    voice = e->phys(voice);
    const auto& in = e->cg->inputs[input];
    uint32_t target;
    if (setvalue) {
        if (in.decl.kind != ogc::Kind::Value || !in.decl.per_voice)
            return set_err(OG_E_INVALID, "'" + in.decl.name + "' is not a per-voice value input");
        target = OG_EV_SETVALUE | input;
    } else {
        if (in.decl.kind != ogc::Kind::Event) return set_err(OG_E_INVALID, "'" + in.decl.name + "' is not an event input");
        target = (uint32_t)in.event_index;
    }
    if (local && !setvalue) { // ArrayVec<EventInstance, 32> capacity per endpoint per block
        if (!e->tl.count_local(voice, target, (size_t)std::max(1, e->cg->n_event_inputs), OG_MAX_EVENTS_PER_BLOCK))
            return set_err(OG_E_OVERFLOW, "event queue full (32 per voice per input per block): event dropped");
    }
    // (an event scheduled in the past fires on the first frame of the next block, like a late event on the device)
    e->tl.push(voice, std::max(frame, e->frame_now), target, value, local);
    return OG_OK;
}

} // namespace

extern "C" {

const char* og_last_error(void) { return g_err.c_str(); }
const char* og_version(void)
{
    return "oscen_amd 0.1 (gfx950); settings: " OG_SETTINGS "; experiment knobs (read only when OSCEN_GPU_EXPERIMENTAL=1): " OG_EXPERIMENT_KNOBS;
}

int og_graph_new(const char* name, og_graph_desc** out)
{
    return ogabi::guard([&]() -> int {
    if (!name || !out) return set_err(OG_E_INVALID, "null argument");
    auto* g = new og_graph_desc;
    g->g.name = name;
    *out = g;
    return OG_OK;
    });
}

int og_graph_builtin(const char* name, og_graph_desc** out)
{
    if (!name || !out) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        auto* g = new og_graph_desc;
        try {
            g->g = ogc::builtin_graph(name);
        } catch (...) {
            delete g;
            throw;
        }
        *out = g;
        return OG_OK;
    });
}

int og_graph_add_input(og_graph_desc* g, const char* name, int kind, float def, uint32_t ramp_frames, uint32_t flags)
{
    return ogabi::guard([&]() -> int {
    if (!g || !name) return set_err(OG_E_INVALID, "null argument");
    if (kind < 0 || kind > 2) return set_err(OG_E_INVALID, "bad endpoint kind");
    ogc::GInput in;
    in.name = name;
    in.kind = (ogc::Kind)kind;
    in.def = def;
    in.ramp_frames = ramp_frames;
    in.per_voice = (flags & OG_IN_PER_VOICE) != 0;
    const uint32_t ch = (flags >> 8) & 0xFu; // OG_IN_CHANNELS(n): a Frame<n> stream input
    if (ch > 4 || (ch > 1 && kind != OG_KIND_STREAM)) return set_err(OG_E_INVALID, "OG_IN_CHANNELS: a stream input is an f32 or a Frame<2..4>");
    in.channels = ch > 1 ? (int)ch : 1;
    g->g.inputs.push_back(in);
    return (int)g->g.inputs.size() - 1;
    });
}

int og_graph_add_output(og_graph_desc* g, const char* name, int kind)
{
    return ogabi::guard([&]() -> int {
    if (!g || !name) return set_err(OG_E_INVALID, "null argument");
    if (kind < 0 || kind > 2) return set_err(OG_E_INVALID, "bad endpoint kind");
    g->g.outputs.push_back({name, (ogc::Kind)kind});
    return (int)g->g.outputs.size() - 1;
    });
}

int og_graph_add_node(og_graph_desc* g, const char* name, const char* type_ctor, const float* args, uint32_t n_args,
                      uint32_t rate_factor)
{
    return ogabi::guard([&]() -> int {
    if (!g || !name || !type_ctor || (n_args && !args)) return set_err(OG_E_INVALID, "null argument");
    ogc::GNode n;
    n.name = name;
    n.type = type_ctor;
    n.args.assign(args, args + n_args);
    n.rate_factor = rate_factor ? rate_factor : 1;
    g->g.nodes.push_back(n);
    return (int)g->g.nodes.size() - 1;
    });
}

int og_graph_add_node_array(og_graph_desc* g, const char* name, const char* type_ctor, const float* args, uint32_t n_args,
                            uint32_t rate_factor, uint32_t length)
{
    if (length == 0) return set_err(OG_E_INVALID, "node array length must be > 0");
    int rc = og_graph_add_node(g, name, type_ctor, args, n_args, rate_factor);
    if (rc >= 0) g->g.nodes.back().array_len = length;
    return rc;
}

int og_register_node(const og_node_type* t)
{
    if (!t || !t->type_ctor || !t->process_src || (t->n_inputs && !t->inputs) || (t->n_outputs && !t->outputs) ||
        (t->n_state && !t->state))
        return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        ogc::UserNodeType u;
        u.type = t->type_ctor;
        u.nargs = t->n_ctor_args;
        for (uint32_t i = 0; i < t->n_inputs; ++i) {
            const og_node_port& p = t->inputs[i];
            if (!p.name || p.kind < 0 || p.kind > 2) throw std::runtime_error("bad input port description");
            u.inputs.push_back({p.name, (ogc::Kind)p.kind, p.default_value, p.ctor_arg, p.channels > 1 ? (int)p.channels : 1});
            if (p.kind == OG_KIND_EVENT && t->event_handler_src && t->event_handler_src[i]) u.handlers[p.name] = t->event_handler_src[i];
        }
        for (uint32_t i = 0; i < t->n_outputs; ++i) {
            if (!t->outputs[i]) throw std::runtime_error("bad output name");
            u.outputs.push_back(t->outputs[i]);
        }
        for (uint32_t i = 0; i < t->n_state; ++i) {
            const og_node_field& f = t->state[i];
            if (!f.name) throw std::runtime_error("bad state field description");
            ogc::UserState st;
            st.name = f.name;
            st.is_uint = f.is_uint != 0;
            st.init_f = f.init;
            st.init_u = f.init_uint;
            st.arg = f.ctor_arg;
            u.state.push_back(st);
        }
        for (uint32_t i = 0; t->output_channels && i < t->n_outputs; ++i) u.out_channels.push_back((int)t->output_channels[i]);
        for (uint32_t i = 0; i < t->n_event_outputs; ++i) {
            if (!t->event_outputs || !t->event_outputs[i]) throw std::runtime_error("bad event output name");
            u.ev_outputs.push_back(t->event_outputs[i]);
        }
        u.process_src = t->process_src;
        u.weight = (int)t->cost_hint;
        if (t->event_queue_capacity > 32) throw std::runtime_error("event_queue_capacity: at most 32 (the reference's ArrayVec<EventInstance, 32>)");
        u.event_capacity = (int)t->event_queue_capacity;
        ognarr::copy_arrays(t->arrays, t->n_arrays, u.arrays);
        ogc::register_user_node(u);
        return OG_OK;
    });
}

int og_unregister_node(const char* type_ctor)
{
    return ogabi::guard([&]() -> int {
    if (!type_ctor) return set_err(OG_E_INVALID, "null argument");
    return ogc::unregister_user_node(type_ctor) ? OG_OK : set_err(OG_E_INVALID, std::string("no user node type '") + type_ctor + "'");
    });
}

int og_register_function(const og_function_type* f)
{
    if (!f || !f->name || !f->source || !f->n_args || !f->arg_names) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        ogc::UserFunction u;
        u.name = f->name;
        for (uint32_t k = 0; k < f->n_args; ++k) {
            if (!f->arg_names[k]) throw std::runtime_error("null argument name");
            u.arg_names.push_back(f->arg_names[k]);
            u.arg_channels.push_back(f->arg_channels && f->arg_channels[k] > 1 ? (int)f->arg_channels[k] : 1);
        }
        u.result_channels = f->result_channels > 1 ? (int)f->result_channels : 1;
        u.source = f->source;
        ogc::register_user_function(u);
        return OG_OK;
    });
}

int og_unregister_function(const char* name)
{
    return ogabi::guard([&]() -> int {
    if (!name) return set_err(OG_E_INVALID, "null argument");
    return ogc::unregister_user_function(name) ? OG_OK : set_err(OG_E_INVALID, std::string("no function '") + name + "'");
    });
}

int og_register_graph_type(const char* type_name, const og_graph_desc* g)
{
    if (!type_name || !g) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        ogc::register_graph_type(type_name, g->g);
        return OG_OK;
    });
}

int og_unregister_graph_type(const char* type_name)
{
    return ogabi::guard([&]() -> int {
    if (!type_name) return set_err(OG_E_INVALID, "null argument");
    return ogc::unregister_graph_type(type_name) ? OG_OK : set_err(OG_E_INVALID, std::string("no graph type '") + type_name + "'");
    });
}

int og_graph_add_bus_node(og_graph_desc* g, const char* name, const char* type_ctor, const float* args, uint32_t n_args)
{
    int rc = og_graph_add_node(g, name, type_ctor, args, n_args, 1);
    if (rc >= 0) g->g.nodes.back().bus = true;
    return rc;
}

int og_graph_add_bus_convolver(og_graph_desc* g, const char* name, const char* ir_name)
{
    return ogabi::guard([&]() -> int {
    if (!g || !name) return set_err(OG_E_INVALID, "null argument");
    ogc::GNode n;
    n.name = name;
    n.type = ir_name ? "Convolver::with_ir" : "Convolver::new";
    if (ir_name) { // the response's name travels as the raw text of the constructor argument, as the DSL front end leaves it
        n.args.push_back(0.0f);
        n.raw_args.push_back(std::string(ir_name).find('(') == std::string::npos ? std::string(ir_name) + "()" : std::string(ir_name));
    }
    n.bus = true;
    g->g.nodes.push_back(n);
    return (int)g->g.nodes.size() - 1;
    });
}

int og_register_ir(const char* name, const float* taps, uint32_t n_taps)
{
    return ogabi::guard([&]() -> int {
    if (!name || (n_taps && !taps)) return set_err(OG_E_INVALID, "null argument");
    ogc::register_ir(name, taps, n_taps);
    return OG_OK;
    });
}

// the asset form: every check on the data is ogc::register_ir_asset's (one copy, the one the stand-alone program runs)
int og_register_ir_asset(const char* name, const float* interleaved, uint64_t frames, uint32_t channels, uint32_t sample_rate)
{
    return ogabi::guard([&]() -> int {
    if (!name) return set_err(OG_E_INVALID, "null argument");
    ogc::register_ir_asset(name, interleaved, frames, channels, sample_rate);
    return OG_OK;
    });
}

int og_ir_info(const char* name, uint64_t* frames, uint32_t* channels, uint32_t* sample_rate)
{
    return ogabi::guard([&]() -> int {
    if (!name) return set_err(OG_E_INVALID, "null argument");
    std::string resolved;
    const ogc::IrEntry ir = ogc::lookup_ir_entry(name, &resolved);
    if (!ir) return set_err(OG_E_INVALID, "no impulse response '" + resolved + "'");
    if (frames) *frames = ir.asset ? ir.asset->frames : ir.taps->size();
    if (channels) *channels = ir.asset ? ir.asset->channels : 1u;
    if (sample_rate) *sample_rate = ir.asset ? ir.asset->rate : 0u;
    return OG_OK;
    });
}

int og_unregister_ir(const char* name)
{
    return ogabi::guard([&]() -> int {
    if (!name) return set_err(OG_E_INVALID, "null argument");
    return ogc::unregister_ir(name) ? OG_OK : set_err(OG_E_INVALID, std::string("no impulse response '") + name + "'");
    });
}

int og_graph_connect(og_graph_desc* g, const char* src, const char* dst, const char* policy)
{
    return ogabi::guard([&]() -> int {
    if (!g || !src || !dst) return set_err(OG_E_INVALID, "null argument");
    g->g.edges.push_back({src, dst, policy ? policy : ""});
    return OG_OK;
    });
}

int og_graph_connect_via(og_graph_desc* g, const char* src, const char* via, const char* dst)
{
    return ogabi::guard([&]() -> int {
    if (!g || !src || !via || !dst) return set_err(OG_E_INVALID, "null argument");
    std::string v = via;
    bool numeric = !v.empty();
    for (char ch : v) numeric = numeric && isdigit((unsigned char)ch);
    if (numeric) { // `-> [N] ->`: an anonymous Delay::new(N, 0.0)  (ir/lower.rs:575-650)
        int k = 0;
        for (const auto& nd : g->g.nodes)
            if (nd.name.rfind("__inline_delay_", 0) == 0) ++k;
        ogc::GNode d;
        d.name = "__inline_delay_" + std::to_string(k);
        d.type = "Delay::new";
        d.args = {(float)atof(via), 0.0f};
        g->g.nodes.push_back(d);
        v = d.name;
    }
    ogc::GEdge in_leg{src, v + ".input", ""}, out_leg{v + ".output", dst, ""};
    out_leg.feedback = true;
    g->g.edges.push_back(in_leg);
    g->g.edges.push_back(out_leg);
    return OG_OK;
    });
}

int og_graph_parse(const char* dsl_text, const char* per_voice_inputs, og_graph_desc** out)
{
    if (!dsl_text || !out) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        std::vector<std::string> pv;
        if (per_voice_inputs) {
            std::string cur;
            for (const char* p = per_voice_inputs;; ++p) {
                if (*p == ',' || *p == 0) {
                    while (!cur.empty() && isspace((unsigned char)cur.back())) cur.pop_back();
                    while (!cur.empty() && isspace((unsigned char)cur.front())) cur.erase(cur.begin());
                    if (!cur.empty()) pv.push_back(cur);
                    cur.clear();
                    if (*p == 0) break;
                } else {
                    cur.push_back(*p);
                }
            }
        }
        std::unique_ptr<og_graph_desc> g(new og_graph_desc);
        g->g = ogc::parse_dsl(dsl_text, pv);
        *out = g.release();
        return OG_OK;
    });
}

int og_graph_poly_info(const og_graph_desc* g, uint32_t* declared_voices, char* frequency_input, char* gate_input, size_t cap)
{
    if (!g) return set_err(OG_E_INVALID, "null graph");
    int is_wrapper = 0;
    int rc = guard([&] {
        ogc::PolyInfo pi;
        (void)ogc::lower_poly_wrapper(g->g, &pi);
        is_wrapper = pi.is_wrapper ? 1 : 0;
        if (declared_voices) *declared_voices = pi.declared_voices;
        auto put = [&](char* dst, const std::string& s) {
            if (!dst || !cap) return;
            const size_t n = std::min(cap - 1, s.size());
            memcpy(dst, s.data(), n);
            dst[n] = 0;
        };
        put(frequency_input, pi.frequency_input);
        put(gate_input, pi.gate_input);
        return OG_OK;
    });
    return rc == OG_OK ? is_wrapper : rc;
}

int64_t og_graph_to_dsl(const og_graph_desc* g, char* buf, size_t cap)
{
    return ogabi::guard_value<int64_t>((int64_t)OG_E_NOMEM, [&]() -> int64_t {
    if (!g) return set_err(OG_E_INVALID, "null graph");
    const std::string t = ogc::to_dsl(g->g);
    if (buf && cap) {
        size_t n = std::min(cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int64_t)t.size();
    });
}

void og_graph_free(og_graph_desc* g) { delete g; }

int64_t og_graph_kernel_source(const og_graph_desc* g, char* buf, size_t cap)
{
    if (!g) return set_err(OG_E_INVALID, "null graph");
    int64_t len = -1;
    int rc = guard([&] {
        auto cg = ogc::compile(g->g);
        len = (int64_t)cg->source.size();
        if (buf && cap) {
            size_t n = std::min(cap - 1, cg->source.size());
            memcpy(buf, cg->source.data(), n);
            buf[n] = 0;
        }
        return OG_OK;
    });
    return rc == OG_OK ? len : rc;
}

int64_t og_graph_variant_source(const og_graph_desc* g, int tier, char* buf, size_t cap)
{
    if (!g || tier < 0 || tier > 3) return set_err(OG_E_INVALID, "null graph or no such tier");
    int64_t len = -1;
    int rc = guard([&] {
        auto cg = ogc::compile(g->g);
        static const std::string none;
        const std::string& src = tier == 3 ? (cg->post ? cg->post->source : none) : (tier == 2 ? cg->zero2_source : (tier == 1 ? cg->zero_source : cg->source));
        len = (int64_t)src.size();
        if (buf && cap) {
            size_t n = std::min(cap - 1, src.size());
            memcpy(buf, src.data(), n);
            buf[n] = 0;
        }
        return OG_OK;
    });
    return rc == OG_OK ? len : rc;
}

int64_t og_graph_jit_check(const og_graph_desc* g, const char* arch)
{
    if (!g || !arch) return set_err(OG_E_INVALID, "null argument");
    int64_t len = -1;
    int rc = guard([&] {
        auto cg = ogc::compile(g->g);
        len = (int64_t)og_jit_compile_only(*cg, arch);
        if (cg->post) len += (int64_t)og_jit_compile_only(*cg->post, arch);
        return OG_OK;
    });
    return rc == OG_OK ? len : rc;
}

int og_create(const og_graph_desc* g, uint32_t n_voices, int device_id, og_engine** out)
{
    if (!g || !out) return set_err(OG_E_INVALID, "null argument");
    if (n_voices == 0) return set_err(OG_E_INVALID, "n_voices must be > 0");
    return guard([&] {
        std::unique_ptr<og_engine> e(new og_engine);
        e->cg = ogc::compile(g->g);
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
            throw HipError("no HIP device available (this engine has no CPU fallback)");
        if (device_id < 0 || device_id >= n_dev) throw HipError("device id out of range");
        e->device = device_id;
        HIPCK(hipSetDevice(device_id));
        e->launch = og_find_kernel(e->cg->hash);
        if (e->launch && !e->cg->zero_slots.empty()) e->launch_zero = og_find_zero_kernel(e->cg->hash);
        if (e->launch && !e->cg->zero2_slots.empty()) e->launch_zero2 = og_find_zero_kernel(e->cg->hash, 2);
        if (!e->launch) e->jit = og_jit_compile(*e->cg); // throws if hiprtc is unavailable or fails
        if (e->cg->post) e->pm_jit = og_jit_compile(*e->cg->post); // (no built-in graph has a post-mix graph: always compiled here)
        e->V = n_voices;
        // voices per wave: narrow the wave until every SIMD holds two (og_kernel_rt.hip.h)
        {
            hipDeviceProp_t prop;
            HIPCK(hipGetDeviceProperties(&prop, device_id));
            const uint32_t simds = 4u * (uint32_t)prop.multiProcessorCount;
            // Measured on MI355X (65 536 fm voices): 64 lanes 0.129 ms, 32 lanes 0.185 ms, 16 lanes
            // 0.325 ms per block -- a wave-instruction costs the same issue time however many of its
            // lanes are active, so narrowing only multiplies instructions.  Kept as an experiment knob.
            e->blocking_memcpy = ogabi::experiment_knob("OSCEN_GPU_BLOCKING_MEMCPY") != nullptr; // (environment knobs are read HERE, once)
            if (const char* zs = ogabi::experiment_knob("OSCEN_GPU_ZERO_SPEC")) e->zero_spec = atoi(zs) != 0;
            if (const char* zs = ogabi::experiment_knob("OSCEN_GPU_ZERO2_SPEC")) e->zero2_spec = atoi(zs) != 0;
            if (const char* ss = ogabi::experiment_knob("OSCEN_GPU_STAGE_SPEC")) e->stage_spec = atoi(ss) != 0;
            if (const char* rc = ogabi::experiment_knob("OSCEN_GPU_RCP_CAP")) e->rcp_cap = std::min<uint32_t>(OG_RCP_MAX, (uint32_t)atoll(rc));
            size_t headroom = EventTimeline::HEADROOM;
            if (const char* hv = ogabi::experiment_knob("OSCEN_GPU_EV_HEADROOM")) headroom = std::max<size_t>(64, (size_t)atoll(hv));
            e->tl = EventTimeline(n_voices, EventTimeline::STAGE_EVENTS, headroom);
            uint32_t lanes = OG_WAVE;
            if (const char* ev = ogabi::experiment_knob("OSCEN_GPU_LANES")) {
                const int l = atoi(ev);
                if (l == 16 || l == 32 || l == 64) lanes = (uint32_t)l;
            }
            e->lanes = lanes;
            // Pipelined variants for banks too small to put enough ordinary waves on every SIMD.  Which depth (waves per 64
            // voices: 1, 2 or 4) runs is decided by a small model of time against waves per SIMD.  (Rounds 1-3 derived it
            // from two constants -- 4.8 cycles per instruction for a lone wave, 3.05 per SIMD otherwise -- which put the
            // four-wave pipeline behind the two-wave one at 65 536 voices; with the round-4 kernels it is 12 % ahead.)
            // Round 4: calibrated on the round-4 kernels instead of derived (profiles/r04_depth_sweep.md: fm_voice, 40
            // blocks of 256 frames per region, ms per block by bank size and depth).  With r = waves per SIMD
            // (ceil(workgroups x depth / SIMDs)) every depth is a straight line in r above a latency floor:
            //   one wave per 64 voices   max(0.074, 0.0365 r + 0.030)   r = 1..4   (16 384 .. 262 144 voices)
            //   two waves                max(0.058, 0.0255 r + 0.006)   r = 1..8
            //   four waves               max(0.034, 0.0113 r + 0.0085)  r = 1..16
            // i.e. a lone wave is bound by its own dependent-issue latency (the floors), and at saturation the pipelines
            // cost MORE SIMD time per voice than the ordinary kernel (2 x 0.0255 and 4 x 0.0113 against 0.0365: hand-offs,
            // barriers, per-wave loop and event bookkeeping) -- they win where they raise occupancy: four waves up to
            // ~131 072 voices (measured 65 536: 0.0535 against 0.0605 / 0.0753; 98 304: 0.076 against 0.097 / 0.101), the
            // ordinary kernel from ~196 608 on.  Other graphs scale the lines by their estimated cost.
            // Round 5: re-calibrated on the round-5 kernels (profiles/r05e_depth_sweep.md) and made aware of RESIDENCY.  A CU
            // holds only so many workgroups of a shape at once (registers, LDS: 16 / 8 / 6 for fm_voice's three shapes --
            // asked of the runtime per kernel, hipOccupancyMaxActiveBlocksPerMultiprocessor); a bank of more workgroups per CU
            // runs in rounds, and a short last round costs almost a full one: at 131 072 voices the four-wave shape (8
            // workgroups per CU, 6 resident) took 0.070 ms per block against 0.057 for two waves, at 196 608 (12 = two full
            // rounds) 0.086 against 0.096 and 0.094 -- the straight lines of round 4 could not see that.  Per round, time
            // against w = workgroups per CU (ms per 256-frame block, fm_voice; other graphs scale by their estimated cost,
            // which does not change the choice):
            //   one wave per 64 voices   w <= 4: 0.058; 8: 0.072; 12: 0.094; 16: 0.116
            //   two waves                w <= 4: 0.043; 6..8: 0.057
            //   four waves               1: 0.0318; 2: 0.0329; 3: 0.0345; 4: 0.0370; 6: 0.0438
            const uint32_t waves1 = (n_voices + OG_WAVE - 1) / OG_WAVE;
            const double cus = std::max(1, prop.multiProcessorCount);
            const double scale = (double)std::max(8, e->cg->valu_estimate) / 76.0; // fm_voice
            auto interp = [](const double* xs, const double* ys, int n, double x) {
                if (x <= xs[0]) return ys[0];
                for (int k = 1; k < n; ++k)
                    if (x <= xs[k]) return ys[k - 1] + (ys[k] - ys[k - 1]) * (x - xs[k - 1]) / (xs[k] - xs[k - 1]);
                return ys[n - 1] * x / xs[n - 1];
            };
            auto round_ms = [&](int d, double w) {
                static const double x1[] = {4, 8, 12, 16}, y1[] = {0.058, 0.072, 0.094, 0.116};
                static const double x2[] = {4, 6, 8}, y2[] = {0.043, 0.057, 0.057};
                static const double x4[] = {1, 2, 3, 4, 6}, y4[] = {0.0318, 0.0329, 0.0345, 0.0370, 0.0438};
                return d == 1 ? interp(x1, y1, 4, w) : (d == 2 ? interp(x2, y2, 3, w) : interp(x4, y4, 5, w));
            };
            auto resident = [&](int d) { // workgroups of this shape a CU holds at once
                int n = 0;
                if (OgOccupancyFn occ = og_find_occupancy(e->cg->hash)) n = occ(d);
                else if (e->jit) n = e->jit->occupancy(d);
                if (n <= 0) n = d == 4 ? 6 : (d == 2 ? 8 : 16);
                return (double)n;
            };
            auto cycles = [&](int d) {
                const double w = std::ceil((double)waves1 / cus); // workgroups per CU (every shape: one workgroup per 64 voices)
                const double cap = resident(d);
                const double full = std::floor(w / cap), rest = w - full * cap;
                return scale * (full * round_ms(d, cap) + (rest > 0.0 ? round_ms(d, rest) : 0.0));
            };
            uint32_t depth = 0;
            double best = cycles(1);
            if (e->cg->max_pipeline >= 2 && cycles(2) < 0.97 * best) { // (a deeper pipeline has to pay for itself)
                best = cycles(2);
                depth = 2;
            }
            if (e->cg->max_pipeline >= 4 && cycles(4) < 0.97 * best) depth = 4;
            if (const char* ev = getenv("OSCEN_GPU_SPLIT")) {
                const int want = atoi(ev);
                depth = (want >= 4 && e->cg->max_pipeline >= 4) ? 4 : ((want >= 2 && e->cg->max_pipeline >= 2) ? 2 : 0);
                if (want == 1 && e->cg->max_pipeline >= 2) depth = 2; // (old boolean meaning)
            }
            if (e->lanes != OG_WAVE) depth = 0; // the pipelined variants always run 64 voices per workgroup
            e->split = depth;
            // the wide four-wave form (16-frame hand-offs: half the barriers, twice the LDS rings) where one round holds the
            // whole bank: +2.4 .. +3.3 % at 65 536 voices (profiles/r05l_session11.log).  OSCEN_GPU_WIDE=0|1 pins it.
            e->wide = false;
            if (depth == 4 && e->cg->wide4) {
                int cap = 0;
                if (OgOccupancyFn occ = og_find_occupancy(e->cg->hash)) cap = occ(5);
                else if (e->jit) cap = e->jit->occupancy(5);
                e->wide = cap > 0 && std::ceil((double)waves1 / cus) <= (double)cap;
                if (const char* ev = getenv("OSCEN_GPU_WIDE")) e->wide = atoi(ev) != 0 && cap > 0;
            }
        }
        e->n_wg = (uint32_t)(((size_t)n_voices * e->cg->lpv + e->lanes - 1) / e->lanes);
        HIPCK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->own_stream = true;
        const auto& cg = *e->cg;
        e->values.resize(cg.inputs.size());
        e->ramps.resize(cg.inputs.size());
        for (size_t i = 0; i < cg.inputs.size(); ++i) {
            e->values[i] = cg.inputs[i].decl.def;
            e->ramps[i].set_immediate(cg.inputs[i].decl.def); // ValueRampState::new(default)
            e->ramps[i].default_frames = cg.inputs[i].decl.ramp_frames;
        }
        HIPCK(hipMalloc(&e->d_state, std::max<size_t>(1, cg.state.size()) * (size_t)n_voices * 4));
        if (!cg.lane_state.empty())
            // (+ one wave's worth of lane words behind the last plane: OgBlockArgs::lane_dump, where a lane beyond the last
            //  voice writes what an event handler of an array-valued node writes through its state planes)
            HIPCK(hipMalloc(&e->d_lane_state, cg.lane_state.size() * (size_t)n_voices * cg.lpv * cg.lane_width * 4 + (size_t)OG_WAVE * OG_LANE_DUMP_WORDS * 4));
        if (!cg.arrays.empty()) { // the node-array pool: every array field of every voice
            const size_t bytes = e->narr_bytes();
            if (hipMalloc(&e->d_narr, bytes) != hipSuccess) {
                (void)hipGetLastError();
                e->d_narr = nullptr;
                throw ogabi::Error(OG_E_NOMEM, "og_create: the array fields of this graph need a pool of " + std::to_string(bytes) + " bytes for " +
                                                   std::to_string(n_voices) + " voices (" + std::to_string(cg.array_words()) + " words per voice), which the device cannot provide");
            }
        }
        if (cg.bus_stage == ogc::BusStage::Tremolo) HIPCK(hipMalloc(&e->d_bus_phase, 4));
        if (cg.post) {
            HIPCK(hipMalloc(&e->d_pm_state, std::max<size_t>(1, cg.post->state.size()) * 4));
            HIPCK(hipMalloc(&e->d_pm_ev, 2 * 4));
            HIPCK(hipMemset(e->d_pm_ev, 0, 2 * 4));
        }
        if (cg.bus_stage == ogc::BusStage::Convolver) // Convolver::with_ir(..) / ::new(): the empty response
            e->bus_conv.set_current(e->conv_upload(cg.bus_ir ? cg.bus_ir->data() : nullptr, cg.bus_ir ? cg.bus_ir->size() : 0));
        HIPCK(hipMalloc(&e->d_ev_end, (size_t)n_voices * 4));
        HIPCK(hipMalloc(&e->d_ev_cursor, (size_t)n_voices * 4));
        HIPCK(hipMemset(e->d_ev_end, 0, (size_t)n_voices * 4));
        HIPCK(hipMemset(e->d_ev_cursor, 0, (size_t)n_voices * 4));
        e->alloc_bus_buffers(1);
        HIPCK(hipMalloc(&e->d_bus, (size_t)OG_MAX_BLOCK * OG_MAX_BUS_CHANNELS * 4));
        HIPCK(hipMalloc(&e->d_tap_slot, (size_t)n_voices * 4));
        HIPCK(hipMemset(e->d_tap_slot, 0xFF, (size_t)n_voices * 4));
        if (!cg.event_outputs.empty() || cg.has_node_event_outputs) {
            HIPCK(hipMalloc(&e->d_out_ev_count, 2 * sizeof(uint32_t)));
            HIPCK(hipMemset(e->d_out_ev_count, 0, 2 * sizeof(uint32_t)));
        }
        if (!cg.event_outputs.empty()) { // room for four events per voice between two reads (OSCEN_GPU_OUT_EVENTS overrides)
            size_t cap = std::max<size_t>(65536, (size_t)n_voices * 4);
            if (const char* ev = ogabi::experiment_knob("OSCEN_GPU_OUT_EVENTS")) cap = std::max<size_t>(16, (size_t)atoll(ev));
            e->out_ev_cap = (uint32_t)std::min<size_t>(cap, 0x7FFFFFFFu);
            HIPCK(hipMalloc(&e->d_out_ev, (size_t)e->out_ev_cap * sizeof(OgOutEvent)));
        }
        e->stream_blocks.resize(cg.inputs.size());
        for (size_t i = 0; i < cg.inputs.size(); ++i)
            if (cg.inputs[i].stream_row >= 0) e->stream_blocks[i].assign((size_t)OG_MAX_BLOCK * std::max(1, cg.inputs[i].decl.channels), 0.0f);
        e->upload_initial_state(); // Graph::new(): 44.1 kHz until init()
        *out = e.release();
        return OG_OK;
    });
}

void og_destroy(og_engine* e) { delete e; }

int og_init(og_engine* e, float sample_rate)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (!(sample_rate > 0.0f)) return set_err(OG_E_INVALID, "sample rate must be positive");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->sr = sample_rate;
        e->queue.clear();
        e->q_frames = 0;
        e->upload_initial_state();
        e->reset_timeline();
        if (e->d_out_ev_count) HIPCK(hipMemsetAsync(e->d_out_ev_count, 0, 2 * sizeof(uint32_t), e->stream));
        e->out_ev_overflow = 0;
        e->out_ev_carry.clear();
        e->ev_lost_total = 0;
        e->phys_of.clear(); // (og_group_voices: a fresh state has no voice order to keep)
        e->logical_of.clear();
        e->frame_now = 0;
        { // the reciprocal table for the releases of the initial parameters, before the first block
            std::vector<uint32_t> slots((size_t)std::max(e->cg->n_slots, 1), 0u);
            const ogc::UEnv ev = e->env();
            for (const auto& up : e->cg->uprogs) slots[up.dst] = up.fn(ev);
            e->rcp_cover(e->release_need(slots.data()));
        }
        e->inited = true;
        return OG_OK;
    });
}

int og_set_bus_ir(og_engine* e, const char* ir_name)
{
    if (!e || !ir_name) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        if (!e->conv_on()) return set_err(OG_E_INVALID, "og_set_bus_ir: this engine has no post-mix Convolver");
        std::string resolved;
        const ogc::IrEntry ir = ogc::lookup_ir_entry(ir_name, &resolved);
        if (!ir) return set_err(OG_E_INVALID, "unknown impulse response '" + resolved + "'; responses are registered with og_register_ir, og_register_ir_asset or og_register_ir_wav");
        HIPCK(hipSetDevice(e->device));
        // an asset response: the playable form is built first -- nothing of the engine has changed if that is refused
        std::shared_ptr<ConvIR> built;
        if (ir.asset) built = e->conv_build_asset(resolved, *ir.asset);
        const size_t k = built ? built->K() : ir.taps->size();
        if (e->bus_conv.outgrows(k)) { // a longer response than the buffers were sized for (not a real-time path)
            e->flush_bus();
            HIPCK(hipStreamSynchronize(e->stream));
            e->conv_alloc(k);
        }
        // the new response replaces a swap no block has picked up yet: that one goes before conv_gc (no launch ever read
        // it), an asset's planes are already held by `built` when the gc runs
        e->bus_conv.publish(built);
        e->conv_gc();
        if (!built) e->bus_conv.publish(e->conv_upload(ir.taps->data(), ir.taps->size()));
        return OG_OK;
    });
}

int og_bus_ir_info(const og_engine* e, uint32_t* taps, uint32_t* channels)
{
    return ogabi::guard([&]() -> int {
    if (!e) return set_err(OG_E_INVALID, "null argument");
    if (!e->conv_on()) return set_err(OG_E_INVALID, "og_bus_ir_info: this engine has no post-mix Convolver");
    const ConvIR* ir = e->bus_conv.published();
    if (taps) *taps = ir ? ir->K() : 0u;
    if (channels) *channels = ir ? ir->planes : 1u;
    return OG_OK;
    });
}

int og_read_bus_ir(const og_engine* e, uint32_t channel, float* out, uint32_t capacity)
{
    return ogabi::guard([&]() -> int {
    if (!e || !out) return set_err(OG_E_INVALID, "null argument");
    if (!e->conv_on()) return set_err(OG_E_INVALID, "og_read_bus_ir: this engine has no post-mix Convolver");
    if (channel >= e->cg->voice_channels) return set_err(OG_E_INVALID, "og_read_bus_ir: the bus has " + std::to_string(e->cg->voice_channels) + " channels");
    const ConvIR* ir = e->bus_conv.published();
    const uint32_t k = ir ? ir->K() : 0u;
    if (capacity < k) return set_err(OG_E_INVALID, "og_read_bus_ir: the output holds " + std::to_string(capacity) + " taps, the response has " + std::to_string(k));
    if (k) memcpy(out, ir->taps.data() + (size_t)(ir->planes > 1 ? channel : 0u) * k, (size_t)k * 4);
    return OG_OK;
    });
}

int og_input_index(const og_engine* e, const char* name)
{
    return ogabi::guard([&]() -> int {
    if (!e || !name) return set_err(OG_E_INVALID, "null argument");
    int i = e->cg->find_input(name);
    return i >= 0 ? i : set_err(OG_E_INVALID, std::string("no input named '") + name + "'");
    });
}
uint32_t og_num_inputs(const og_engine* e) { return e ? (uint32_t)e->cg->inputs.size() : 0; }

int og_set_value(og_engine* e, uint32_t input, float v)
{
    int rc = check_value_input(e, input, false);
    if (rc) return rc;
    if (!e->queue.empty() && (rc = og_flush(e)) != OG_OK) return rc; // queued blocks keep the old value
    if (e->cg->inputs[input].ramp_row < 0) {
        e->values[input] = v;
        return OG_OK;
    }
    Ramp& r = e->ramps[input]; // set_<name>  codegen/mod.rs:931-940
    if (v != r.target) {
        if (!r.ramping()) e->active_ramps += 1;
        r.set_with_ramp(v, r.default_frames);
        e->values[input] = r.current;
    }
    return OG_OK;
}

int og_set_value_ramp(og_engine* e, uint32_t input, float v, uint32_t frames)
{
    int rc = check_value_input(e, input, false);
    if (rc) return rc;
    if (!e->queue.empty() && (rc = og_flush(e)) != OG_OK) return rc; // queued blocks keep the old value
    if (e->cg->inputs[input].ramp_row < 0) {
        e->values[input] = v;
        return OG_OK;
    }
    Ramp& r = e->ramps[input]; // set_<name>_with_ramp  codegen/mod.rs:944-953
    if (v != r.target) {
        if (frames > 0 && !r.ramping()) e->active_ramps += 1;
        // (the reference leaves active_ramps untouched when a running ramp is cut by
        //  frames == 0; the counter only gates ticking, so results are unaffected)
        if (frames == 0 && r.ramping()) e->active_ramps -= 1;
        r.set_with_ramp(v, frames);
        e->values[input] = r.current;
    }
    return OG_OK;
}

int og_set_value_immediate(og_engine* e, uint32_t input, float v)
{
    int rc = check_value_input(e, input, false);
    if (rc) return rc;
    if (!e->queue.empty() && (rc = og_flush(e)) != OG_OK) return rc; // queued blocks keep the old value
    if (e->cg->inputs[input].ramp_row >= 0) { // set_<name>_immediate  codegen/mod.rs:957-963
        Ramp& r = e->ramps[input];
        if (r.ramping()) e->active_ramps -= 1;
        r.set_immediate(v);
    }
    e->values[input] = v;
    return OG_OK;
}

int og_get_value(const og_engine* e, uint32_t input, float* out)
{
    int rc = check_value_input(e, input, false);
    if (rc) return rc;
    if (!out) return set_err(OG_E_INVALID, "null argument");
    *out = e->values[input];
    return OG_OK;
}

int og_ramp_state(const og_engine* e, uint32_t input, float* current, float* target, uint32_t* frames_remaining)
{
    int rc = check_value_input(e, input, false);
    if (rc) return rc;
    const Ramp& r = e->ramps[input];
    const bool ramped = e->cg->inputs[input].decl.ramp_frames > 0 || r.ramping();
    if (current) *current = ramped ? r.current : e->values[input];
    if (target) *target = ramped ? r.target : e->values[input];
    if (frames_remaining) *frames_remaining = r.frames_remaining;
    return OG_OK;
}
uint32_t og_active_ramps(const og_engine* e) { return e ? e->active_ramps : 0; }

int og_set_voice_values(og_engine* e, uint32_t input, uint32_t first, uint32_t count, const float* v)
{
    int rc = check_value_input(e, input, true);
    if (rc) return rc;
    if (!v || (uint64_t)first + count > e->V) return set_err(OG_E_INVALID, "voice range out of bounds");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        const size_t w = (size_t)e->cg->inputs[input].state_word;
        if (e->phys_of.empty()) {
            e->bounce.h2d(e->d_state + w * e->V + first, v, (size_t)count * 4, e->stream);
        } else if (count <= 64u) { // grouped voices, a few values: one word each
            for (uint32_t i = 0; i < count; ++i) e->bounce.h2d(e->d_state + w * e->V + e->phys_of[first + i], v + i, 4, e->stream);
        } else { // grouped voices: the range is scattered over the plane
            std::vector<float> plane(e->V);
            if (count < e->V) {
                e->bounce.d2h(plane.data(), e->d_state + w * e->V, (size_t)e->V * 4, e->stream);
                HIPCK(hipStreamSynchronize(e->stream));
            }
            for (uint32_t i = 0; i < count; ++i) plane[e->phys_of[first + i]] = v[i];
            e->bounce.h2d(e->d_state + w * e->V, plane.data(), (size_t)e->V * 4, e->stream);
        }
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}

int og_set_voice_value(og_engine* e, uint32_t input, uint32_t voice, float v)
{
    return og_set_voice_values(e, input, voice, 1, &v);
}

// ---- SamplePlayer: registry, device pool, publishing ------------------------------------------------------------------
namespace {
// rate 0: untagged (og_register_sample)
int register_sample(const char* who, const char* name, const float* interleaved, uint64_t frames, uint32_t channels, uint32_t rate)
{
    if (!name || !*name) return set_err(OG_E_INVALID, std::string(who) + ": a sample needs a name");
    if (channels < 1 || channels > OG_MAX_SAMPLE_CHANNELS)
        return set_err(OG_E_INVALID, std::string(who) + ": 1 to " + std::to_string(OG_MAX_SAMPLE_CHANNELS) + " channels");
    if (frames > OG_MAX_SAMPLE_FLOATS / channels)
        return set_err(OG_E_INVALID, std::string(who) + ": '" + std::string(name) + "' has more than 2^28 samples (frames x channels)");
    if (frames && !interleaved) return set_err(OG_E_INVALID, "null argument");
    auto sd = std::make_shared<SampleData>();
    sd->frames = (uint32_t)frames;
    sd->channels = channels;
    sd->rate = rate;
    if (frames) sd->interleaved.assign(interleaved, interleaved + (size_t)frames * channels);
    std::lock_guard<std::mutex> lk(sample_registry_lock());
    sample_registry()[name] = sd;
    return OG_OK;
}
// host buffers through the resample kernel on the current device (og_resample)
void resample_on_device(const float* in, uint64_t frames, uint32_t channels, const OgResamplePlan& plan, float* out)
{
    DeviceScratch d_src((size_t)frames * channels), d_dst((size_t)plan.out_len * channels);
    HIPCK(hipMemcpy(d_src.p, in, (size_t)frames * channels * 4, hipMemcpyHostToDevice));
    og_resample_launch(d_src.p, frames, channels, plan, d_dst.p, nullptr);
    HIPCK(hipGetLastError());
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpy(out, d_dst.p, (size_t)plan.out_len * channels * 4, hipMemcpyDeviceToHost));
}
} // namespace

int og_register_sample(const char* name, const float* interleaved, uint64_t frames, uint32_t channels)
{
    return ogabi::guard([&]() -> int { return register_sample("og_register_sample", name, interleaved, frames, channels, 0u); });
}

// AudioAsset::from_samples' own checks (asset/mod.rs:175-192): an empty asset and a zero rate are refused
int og_register_sample_at_rate(const char* name, const float* interleaved, uint64_t frames, uint32_t channels, uint32_t sample_rate)
{
    return ogabi::guard([&]() -> int {
    if (sample_rate == 0) return set_err(OG_E_INVALID, "og_register_sample_at_rate: the sample rate is 0");
    if (frames == 0) return set_err(OG_E_INVALID, "og_register_sample_at_rate: the sample is empty");
    return register_sample("og_register_sample_at_rate", name, interleaved, frames, channels, sample_rate);
    });
}

int og_sample_info(const char* name, uint64_t* frames, uint32_t* channels, uint32_t* sample_rate)
{
    return ogabi::guard([&]() -> int {
    if (!name) return set_err(OG_E_INVALID, "null argument");
    const auto sd = lookup_sample(name);
    if (!sd) return set_err(OG_E_INVALID, std::string("no sample '") + name + "'");
    if (frames) *frames = sd->frames;
    if (channels) *channels = sd->channels;
    if (sample_rate) *sample_rate = sd->rate;
    return OG_OK;
    });
}

int og_read_sample(const char* name, float* out, uint64_t capacity_frames)
{
    return ogabi::guard([&]() -> int {
    if (!name || !out) return set_err(OG_E_INVALID, "null argument");
    const auto sd = lookup_sample(name);
    if (!sd) return set_err(OG_E_INVALID, std::string("no sample '") + name + "'");
    if (capacity_frames < sd->frames) return set_err(OG_E_INVALID, "og_read_sample: the output holds " + std::to_string(capacity_frames) + " frames, the sample has " + std::to_string(sd->frames));
    if (!sd->interleaved.empty()) memcpy(out, sd->interleaved.data(), sd->interleaved.size() * 4);
    return OG_OK;
    });
}

int og_resample_frames(uint64_t frames, uint32_t src_rate, uint32_t dst_rate, uint64_t* out_frames)
{
    return ogabi::guard([&]() -> int {
    if (!out_frames) return set_err(OG_E_INVALID, "null argument");
    if (src_rate == 0 || dst_rate == 0) return set_err(OG_E_INVALID, "og_resample_frames: the sample rate is 0");
    if (frames > OG_MAX_SAMPLE_FLOATS) return set_err(OG_E_INVALID, "og_resample_frames: more than 2^28 frames");
    *out_frames = frames == 0 || src_rate == dst_rate ? frames : og_resample_plan(frames, src_rate, dst_rate).out_len;
    return OG_OK;
    });
}

int og_resample(const float* interleaved, uint64_t frames, uint32_t channels, uint32_t src_rate, uint32_t dst_rate, float* out,
                uint64_t out_capacity_frames)
{
    return ogabi::guard([&]() -> int {
    if (!interleaved || !out) return set_err(OG_E_INVALID, "null argument");
    if (src_rate == 0 || dst_rate == 0) return set_err(OG_E_INVALID, "og_resample: the sample rate is 0");
    if (frames == 0) return set_err(OG_E_INVALID, "og_resample: the input is empty");
    if (channels < 1 || channels > OG_MAX_SAMPLE_CHANNELS)
        return set_err(OG_E_INVALID, "og_resample: 1 to " + std::to_string(OG_MAX_SAMPLE_CHANNELS) + " channels");
    if (frames > OG_MAX_SAMPLE_FLOATS / channels) return set_err(OG_E_INVALID, "og_resample: more than 2^28 samples (frames x channels)");
    const OgResamplePlan plan = og_resample_plan(frames, src_rate, dst_rate);
    const uint64_t n = src_rate == dst_rate ? frames : plan.out_len;
    if (n > out_capacity_frames)
        return set_err(OG_E_INVALID, "og_resample: the output holds " + std::to_string(out_capacity_frames) + " frames, " + std::to_string(n) + " are needed (og_resample_frames)");
    if (n > OG_MAX_SAMPLE_FLOATS / channels) return set_err(OG_E_INVALID, "og_resample: the output has more than 2^28 samples (frames x channels)");
    if (src_rate == dst_rate) {
        memmove(out, interleaved, (size_t)frames * channels * 4);
        return OG_OK;
    }
    if (n) resample_on_device(interleaved, frames, channels, plan, out);
    return OG_OK;
    });
}

int og_unregister_sample(const char* name)
{
    return ogabi::guard([&]() -> int {
    if (!name) return set_err(OG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(sample_registry_lock());
    return sample_registry().erase(name) ? OG_OK : set_err(OG_E_INVALID, std::string("no sample '") + name + "'");
    });
}

int og_load_sample(og_engine* e, const char* name, uint32_t* index)
{
    if (!e || !name || !index) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        if (e->cg->players.empty()) return set_err(OG_E_INVALID, "og_load_sample: this graph has no SamplePlayer");
        for (size_t i = 0; i < e->samples.size(); ++i)
            if (e->samples[i].name == name) { // idempotent per name
                *index = (uint32_t)i;
                return OG_OK;
            }
        const auto sd = lookup_sample(name);
        if (!sd) return set_err(OG_E_INVALID, std::string("unknown sample '") + name + "'; samples are registered with og_register_sample");
        HIPCK(hipSetDevice(e->device));
        *index = e->load_sample(name, *sd);
        return OG_OK;
    });
}

int og_set_voice_samples(og_engine* e, const char* node, uint32_t first, uint32_t count, const uint32_t* indices)
{
    if (!e || !node || (count && !indices)) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        const int k = e->find_player(node);
        if (k < 0) return set_err(OG_E_INVALID, std::string("no SamplePlayer named '") + node + "'");
        if ((uint64_t)first + count > e->V) return set_err(OG_E_INVALID, "voice range out of bounds");
        for (uint32_t i = 0; i < count; ++i)
            if (indices[i] != OG_SAMPLE_NONE && indices[i] >= e->samples.size())
                return set_err(OG_E_INVALID, "sample index " + std::to_string(indices[i]) + " was not handed out by og_load_sample");
        for (uint32_t i = 0; i < count; ++i) { // SampleRateMismatch: a conformed sample plays at the rate it was conformed to only
            if (indices[i] == OG_SAMPLE_NONE) continue;
            const auto& ls = e->samples[indices[i]];
            if (ls.src_rate && (float)ls.rate != e->sr)
                return set_err(OG_E_INVALID, "sample '" + ls.name + "' was conformed to " + std::to_string(ls.rate) + " Hz, the engine now runs at " + std::to_string(e->sr) + " Hz");
        }
        if (!count) return OG_OK;
        HIPCK(hipSetDevice(e->device));
        e->flush_bus(); // queued blocks keep what they were queued under: the words are written behind them, in stream order
        uint32_t* smp = e->d_state + (size_t)e->cg->players[k].sample_word * e->V;
        uint32_t* ph = e->d_state + (size_t)e->cg->players[k].playhead_word * e->V;
        if (e->phys_of.empty()) {
            e->bounce.h2d(smp + first, indices, (size_t)count * 4, e->stream);
            HIPCK(hipMemsetAsync(ph + first, 0, (size_t)count * 4, e->stream));
        } else { // grouped voices: the range is scattered over the planes
            std::vector<uint32_t> a(e->V), b(e->V);
            if (count < e->V) {
                e->bounce.d2h(a.data(), smp, (size_t)e->V * 4, e->stream);
                e->bounce.d2h(b.data(), ph, (size_t)e->V * 4, e->stream);
            }
            for (uint32_t i = 0; i < count; ++i) {
                a[e->phys_of[first + i]] = indices[i];
                b[e->phys_of[first + i]] = 0u;
            }
            e->bounce.h2d(smp, a.data(), (size_t)e->V * 4, e->stream);
            e->bounce.h2d(ph, b.data(), (size_t)e->V * 4, e->stream);
        }
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}

int og_set_sample(og_engine* e, const char* node, uint32_t index)
{
    if (!e || !node) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        const std::vector<uint32_t> all(e->V, index);
        return og_set_voice_samples(e, node, 0, e->V, all.data());
    });
}

int og_push_voice_event(og_engine* e, uint32_t input, uint32_t voice, uint32_t frame_offset, float scalar)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return push_event(e, input, voice, e->frame_now + frame_offset, scalar, true, false);
}
int og_push_voice_value(og_engine* e, uint32_t input, uint32_t voice, uint32_t frame_offset, float v)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return push_event(e, input, voice, e->frame_now + frame_offset, v, true, true);
}
int og_schedule_voice_event(og_engine* e, uint32_t input, uint32_t voice, uint64_t abs_frame, float scalar)
{
    return push_event(e, input, voice, abs_frame, scalar, false, false);
}
int og_schedule_voice_value(og_engine* e, uint32_t input, uint32_t voice, uint64_t abs_frame, float v)
{
    return push_event(e, input, voice, abs_frame, v, false, true);
}

int og_schedule_voice_events(og_engine* e, uint32_t input, uint32_t n, const uint32_t* voices, const uint64_t* abs_frames,
                             const float* values)
{
    return ogabi::guard([&]() -> int {
    if (!e || (n && (!voices || !abs_frames || !values))) return set_err(OG_E_INVALID, "null argument");
    if (input >= e->cg->inputs.size()) return set_err(OG_E_INVALID, "input index out of range");
    const auto& in = e->cg->inputs[input];
    uint32_t target;
    if (in.decl.kind == ogc::Kind::Event) target = (uint32_t)in.event_index;
    else if (in.decl.kind == ogc::Kind::Value && in.decl.per_voice) target = OG_EV_SETVALUE | input;
    else return set_err(OG_E_INVALID, "'" + in.decl.name + "' is neither an event input nor a per-voice value input");
    for (uint32_t i = 0; i < n; ++i)
        if (voices[i] >= e->V) return set_err(OG_E_INVALID, "voice index out of range");
    e->tl.reserve_pending(n);
    for (uint32_t i = 0; i < n; ++i)
        e->tl.push(e->phys(voices[i]), std::max(abs_frames[i], e->frame_now), target, values[i], false);
    return OG_OK;
    });
}

int og_process_block_async(og_engine* e, uint32_t frames, float* d_out_bus)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (!e->inited) return set_err(OG_E_STATE, "og_init must be called before processing");
    if (frames > OG_MAX_BLOCK_SIZE) return set_err(OG_E_INVALID, "frames must be in 0..512");
    return guard([&] {
        if (frames == 0) { // process_block(0): no frame runs; events queued for the block are discarded with it
            HIPCK(hipSetDevice(e->device));
            e->flush_bus();
            e->tl.drop_late_local(e->frame_now);
            e->last_frames = 0;
            return OG_OK;
        }
        e->process_async(frames, d_out_bus);
        return OG_OK;
    });
}

// n consecutive og_process_block_async calls in one: a render loop that has nothing to say between its blocks (offline
// rendering, a streaming caller that queues a buffer's worth) crosses the boundary once.  Same queue, same results.
int og_process_blocks_async(og_engine* e, uint32_t frames, uint32_t n_blocks, float* d_out_bus, size_t out_stride_bytes)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (!e->inited) return set_err(OG_E_STATE, "og_init must be called before processing");
    if (frames == 0 || frames > OG_MAX_BLOCK_SIZE) return set_err(OG_E_INVALID, "frames must be in 1..512");
    if (d_out_bus && out_stride_bytes % sizeof(float)) return set_err(OG_E_INVALID, "out_stride_bytes must be a multiple of 4");
    return guard([&] {
        for (uint32_t b = 0; b < n_blocks; ++b)
            e->process_async(frames, d_out_bus ? d_out_bus + (size_t)b * (out_stride_bytes / sizeof(float)) : nullptr);
        return OG_OK;
    });
}

int og_synchronize(og_engine* e)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        HIPCK(hipStreamSynchronize(e->stream));
        e->sync_lost_counter(); // (graphs with in-voice event queues only)
        return OG_OK;
    });
}

int og_set_bus_batching(og_engine* e, uint32_t blocks)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (blocks > OG_MAX_QUEUE_BLOCKS)
        return set_err(OG_E_INVALID, "bus batching: 0 (automatic) or 1.." + std::to_string(OG_MAX_QUEUE_BLOCKS) + " blocks");
    if (blocks > OG_MAX_LAUNCH_BLOCKS && e->cg->reads_block_starts) // (the launch carries OG_MAX_LAUNCH_BLOCKS block starts)
        return set_err(OG_E_INVALID, "bus batching: a graph whose event handlers read frame_offset takes 0 (automatic) or 1.." +
                                         std::to_string(OG_MAX_LAUNCH_BLOCKS) + " blocks");
    if (blocks == 0) blocks = e->auto_batch();
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        if (e->launch_frames_cap(blocks) > e->cap_frames) e->alloc_bus_buffers(blocks);
        e->bus_batch = blocks;
        return OG_OK;
    });
}

int og_flush(og_engine* e)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        return OG_OK;
    });
}

// The blocking drop-in entry (the reference's process_block + reading the output field): the bus of this one block is
// written by the device straight into pinned host memory, and completion is a word of pinned memory the stream marker
// writes -- no hipMemcpy, no hipStreamSynchronize (both cost tens of microseconds of runtime latency per block).
int og_process_block(og_engine* e, uint32_t frames, float* out_bus)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (!e->inited) return set_err(OG_E_STATE, "og_init must be called before processing");
    if (frames > OG_MAX_BLOCK_SIZE) return set_err(OG_E_INVALID, "frames must be in 0..512");
    if (frames == 0 || !out_bus || e->n_taps > 0 || e->blocking_memcpy) { // (taps are read with a stream sync anyway)
        int rc = og_process_block_async(e, frames, nullptr);
        if (rc) return rc;
        return guard([&] {
            e->flush_bus();
            if (out_bus && frames)
                e->bounce.d2h(out_bus, e->d_bus, (size_t)frames * e->cg->channels * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
            return OG_OK;
        });
    }
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus(); // earlier async blocks keep their own destinations
        if (!e->h_bus_pinned) HIPCK(hipHostMalloc((void**)&e->h_bus_pinned, (size_t)OG_MAX_BLOCK * OG_MAX_BUS_CHANNELS * 4, hipHostMallocDefault));
        // ask for the stream marker behind this block's launch BEFORE the block is queued: with one block per launch
        // (the default) process_async launches it itself, and a marker requested afterwards would never be written
        // (the wait then ran into its 20 ms timeout on every call -- ADVICE r2)
        e->batch_staged = true;
        const uint64_t seq = e->flush_seq + 1;
        e->process_async(frames, e->h_bus_pinned);
        e->flush_bus();
        e->blocking_waits += 1;
        if (!e->wait_progress(seq)) e->blocking_timeouts += 1;
        memcpy(out_bus, e->h_bus_pinned, (size_t)frames * e->cg->channels * 4);
        return OG_OK;
    });
}

int og_set_stream(og_engine* e, void* s)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        HIPCK(hipStreamSynchronize(e->stream));
        if (e->own_stream) HIPCK(hipStreamDestroy(e->stream));
        e->own_stream = false;
        e->stream = (hipStream_t)s;
        return OG_OK;
    });
}

int og_render(og_engine* e, uint64_t total_frames, uint32_t block, float* out_bus)
{
    if (!e || !out_bus) return set_err(OG_E_INVALID, "null argument");
    if (block == 0 || block > OG_MAX_BLOCK_SIZE) return set_err(OG_E_INVALID, "block must be in 1..512");
    if (!e->inited) return set_err(OG_E_STATE, "og_init must be called before processing");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        const uint32_t ch = e->cg->channels;
        float* d_all = nullptr;
        HIPCK(hipMalloc(&d_all, (size_t)total_frames * ch * 4));
        // an offline render has nothing between its blocks: several per launch (the caller's setting is restored)
        e->flush_bus();
        const uint32_t user_batch = e->bus_batch;
        if (e->cap_frames < e->launch_frames_cap(e->auto_batch())) e->alloc_bus_buffers(e->auto_batch());
        e->bus_batch = e->auto_batch();
        struct Restore {
            og_engine* e;
            uint32_t b;
            ~Restore() { e->bus_batch = b; }
        } restore{e, user_batch};
        try {
            for (uint64_t f0 = 0; f0 < total_frames; f0 += block) {
                const uint32_t frames = (uint32_t)std::min<uint64_t>(block, total_frames - f0);
                e->process_async(frames, d_all + f0 * ch);
            }
            e->flush_bus();
            e->bounce.d2h(out_bus, d_all, (size_t)total_frames * ch * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
        } catch (...) {
            (void)hipFree(d_all);
            throw;
        }
        HIPCK(hipFree(d_all));
        return OG_OK;
    });
}

int og_set_stream_block(og_engine* e, uint32_t input, const float* samples, uint32_t n)
{
    return ogabi::guard([&]() -> int {
    if (!e || (n && !samples)) return set_err(OG_E_INVALID, "null argument");
    if (input >= e->cg->inputs.size() || e->cg->inputs[input].stream_row < 0) return set_err(OG_E_INVALID, "not a stream input");
    if (n > OG_MAX_BLOCK_SIZE) return set_err(OG_E_INVALID, "a stream block holds at most 512 samples");
    const uint32_t w = (uint32_t)std::max(1, e->cg->inputs[input].decl.channels); // Frame<N>: `samples` holds n frames of N, interleaved
    float* blk = e->stream_blocks[input].data();
    for (uint32_t k = 0; k < w; ++k)
        for (uint32_t j = 0; j < n; ++j) blk[(size_t)k * OG_MAX_BLOCK + j] = samples[(size_t)j * w + k];
    return OG_OK;
    });
}

uint32_t og_num_stream_inputs(const og_engine* e) { return e ? (uint32_t)e->cg->n_stream_inputs : 0; }

uint32_t og_stream_input_channels(const og_engine* e, uint32_t input)
{
    return ogabi::guard_value<uint32_t>((uint32_t)0, [&]() -> uint32_t {
    if (!e || input >= e->cg->inputs.size() || e->cg->inputs[input].stream_row < 0) return 0;
    return (uint32_t)std::max(1, e->cg->inputs[input].decl.channels);
    });
}

int og_render_inputs(og_engine* e, const float* const* inputs, const uint64_t* input_lens, uint32_t n_inputs, uint64_t tail,
                     float* out_bus, uint64_t* frames_rendered)
{
    if (!e || (n_inputs && (!inputs || !input_lens))) return set_err(OG_E_INVALID, "null argument");
    if (!e->inited) return set_err(OG_E_STATE, "og_init must be called before processing");
    if (n_inputs != (uint32_t)e->cg->n_stream_inputs) // render(): assert_eq!(inputs.len(), NUM_STREAM_INPUTS)
        return set_err(OG_E_INVALID, "render: expected " + std::to_string(e->cg->n_stream_inputs) + " input streams, got " + std::to_string(n_inputs));
    uint64_t in_len = 0;
    for (uint32_t i = 0; i < n_inputs; ++i) in_len = std::max(in_len, input_lens[i]);
    const uint64_t total = in_len + tail;
    if (frames_rendered) *frames_rendered = total;
    if (total == 0) return OG_OK;
    if (!out_bus) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        std::vector<int> sidx; // stream inputs in declaration order
        for (size_t i = 0; i < e->cg->inputs.size(); ++i)
            if (e->cg->inputs[i].stream_row >= 0) sidx.push_back((int)i);
        const uint32_t ch = e->cg->channels;
        float* d_all = nullptr;
        HIPCK(hipMalloc(&d_all, (size_t)total * ch * 4));
        e->flush_bus();
        const uint32_t user_batch = e->bus_batch;
        if (e->cap_frames < e->launch_frames_cap(e->auto_batch())) e->alloc_bus_buffers(e->auto_batch());
        e->bus_batch = e->auto_batch();
        struct Restore {
            og_engine* e;
            uint32_t b;
            ~Restore() { e->bus_batch = b; }
        } restore{e, user_batch};
        try {
            for (uint64_t pos = 0; pos < total; pos += OG_MAX_BLOCK) { // chunks of DEFAULT_MAX_BLOCK_SIZE, offline.rs:71-90
                const uint32_t n = (uint32_t)std::min<uint64_t>(OG_MAX_BLOCK, total - pos);
                for (uint32_t k = 0; k < n_inputs; ++k) {
                    float* blk = e->stream_blocks[sidx[k]].data();
                    const uint32_t w = (uint32_t)std::max(1, e->cg->inputs[sidx[k]].decl.channels); // (lengths count FRAMES)
                    for (uint32_t c = 0; c < w; ++c)
                        for (uint32_t j = 0; j < n; ++j) // silence past the end
                            blk[(size_t)c * OG_MAX_BLOCK + j] = (pos + j < input_lens[k]) ? inputs[k][(pos + j) * w + c] : 0.0f;
                }
                e->process_async(n, d_all + pos * ch);
            }
            e->flush_bus();
            e->bounce.d2h(out_bus, d_all, (size_t)total * ch * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
        } catch (...) {
            (void)hipFree(d_all);
            throw;
        }
        HIPCK(hipFree(d_all));
        return OG_OK;
    });
}

// `graph.<node>.<field>`: the generated struct's node fields are public in the reference and its tests read them
// (`graph.sinks[i].last`, `graph.inner.dummy.val`).  Here a node's persistent fields are planes of the state image.
static int find_state_word(const og_engine* e, const char* path)
{
    // the reference's spelling -> the names of the flattened graph: `sinks[1].last` -> `sinks__1.last`,
    // `inner.dummy.val` -> `inner_dummy.val` (the last dot separates node and field)
    std::string p;
    for (const char* c = path; *c; ++c) {
        if (*c == '[') p += "__";
        else if (*c != ']' && !isspace((unsigned char)*c)) p.push_back(*c);
    }
    const size_t last = p.rfind('.');
    for (size_t k = 0; k < p.size(); ++k)
        if (p[k] == '.' && k != last) p[k] = '_';
    for (size_t w = 0; w < e->cg->state.size(); ++w)
        if (e->cg->state[w].name == p) return (int)w;
    // the fields of the post-mix nodes: the words of the second state image, numbered behind the voices'
    for (size_t w = 0; e->cg->post && w < e->cg->post->state.size(); ++w)
        if (e->cg->post->state[w].name == p) return (int)(e->cg->state.size() + w);
    return -1;
}

int og_state_field_index(const og_engine* e, const char* path)
{
    if (!e || !path) return -1;
    return find_state_word(e, path);
}

int og_read_state_field(og_engine* e, const char* path, uint32_t first_voice, uint32_t n, void* out)
{
    if (!e || !path || (n && !out)) return set_err(OG_E_INVALID, "null argument");
    const int w = find_state_word(e, path);
    if (w < 0) return set_err(OG_E_INVALID, std::string("no state field '") + path + "'");
    const bool post_field = (size_t)w >= e->cg->state.size();
    if (post_field && (first_voice != 0 || n != 1))
        return set_err(OG_E_INVALID, std::string("state field '") + path + "' belongs to a post-mix node: there is one of it (first_voice 0, n 1)");
    if ((uint64_t)first_voice + n > e->V) return set_err(OG_E_INVALID, "voice range out of bounds");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        if (post_field) {
            e->bounce.d2h(out, e->d_pm_state + ((size_t)w - e->cg->state.size()), 4, e->stream);
        } else if (n && e->phys_of.empty()) {
            e->bounce.d2h(out, e->d_state + (size_t)w * e->V + first_voice, (size_t)n * 4, e->stream);
        } else if (n) { // grouped voices: gather
            std::vector<uint32_t> plane(e->V);
            e->bounce.d2h(plane.data(), e->d_state + (size_t)w * e->V, (size_t)e->V * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
            for (uint32_t i = 0; i < n; ++i) ((uint32_t*)out)[i] = plane[e->phys_of[first_voice + i]];
        }
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}

// ---- array fields of registered node types (og_node_array.hip.h; host bookkeeping: og_node_array_host.h) ---------------------
int og_node_array_info(const og_engine* e, const char* path, uint32_t* length, int* is_uint)
{
    if (!e || !path) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        const int k = ognarr::find_field(e->cg->arrays, path);
        if (k < 0) return set_err(OG_E_INVALID, std::string("no array field '") + path + "'");
        if (length) *length = e->cg->arrays[k].length;
        if (is_uint) *is_uint = e->cg->arrays[k].is_uint ? 1 : 0;
        return OG_OK;
    });
}

// the planes of field k <-> the caller's rows; a whole-field transfer (the planes of a field are contiguous, the columns of a
// voice range are not), then the transposition on the host
static int node_array_transfer(og_engine* e, const char* path, uint32_t first_voice, uint32_t count, void* out, const void* data)
{
    return guard([&]() -> int {
        const int k = ognarr::find_field(e->cg->arrays, path);
        if (k < 0) return set_err(OG_E_INVALID, std::string("no array field '") + path + "'");
        if ((uint64_t)first_voice + count > e->V) return set_err(OG_E_INVALID, "voice range out of bounds");
        HIPCK(hipSetDevice(e->device));
        e->flush_bus(); // queued blocks keep what they were queued under: a write lands behind them, in stream order
        const auto& f = e->cg->arrays[k];
        if (count) {
            uint32_t* d = e->d_narr + (size_t)f.base * e->V;
            const size_t bytes = (size_t)f.length * e->V * 4;
            std::vector<uint32_t> planes((size_t)f.length * e->V);
            const uint32_t* slot_of = e->phys_of.empty() ? nullptr : e->phys_of.data();
            if (out || count < e->V) e->bounce.d2h(planes.data(), d, bytes, e->stream);
            if (out) ognarr::gather_rows(f, e->V, slot_of, first_voice, count, planes.data(), (uint32_t*)out);
            if (data) {
                ognarr::scatter_rows(f, e->V, slot_of, first_voice, count, (const uint32_t*)data, planes.data());
                e->narr_dirty = true;
                e->bounce.h2d(d, planes.data(), bytes, e->stream);
            }
        }
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}
int og_read_node_array(og_engine* e, const char* path, uint32_t first_voice, uint32_t count, void* out)
{
    if (!e || !path || (count && !out)) return set_err(OG_E_INVALID, "null argument");
    return node_array_transfer(e, path, first_voice, count, out, nullptr);
}
int og_write_node_array(og_engine* e, const char* path, uint32_t first_voice, uint32_t count, const void* data)
{
    if (!e || !path || (count && !data)) return set_err(OG_E_INVALID, "null argument");
    return node_array_transfer(e, path, first_voice, count, nullptr, data);
}

// ---- Oscilloscope nodes (og_scope.hip.h; what a read reconstructs: og_scope_host.h) -----------------------------------------
static int find_scope(const og_engine* e, const char* path)
{
    const std::string p = ogscope::flat_node(path);
    for (size_t k = 0; k < e->cg->scopes.size(); ++k)
        if (e->cg->scopes[k].name == p) return (int)k;
    return -1;
}
int og_scope_info(const og_engine* e, const char* node_path, uint32_t* capacity, int* auto_detect)
{
    if (!e || !node_path) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        const int k = find_scope(e, node_path);
        if (k < 0) return set_err(OG_E_INVALID, std::string("no Oscilloscope named '") + node_path + "'");
        if (capacity) *capacity = e->cg->scopes[k].capacity;
        if (auto_detect) *auto_detect = e->cg->scopes[k].auto_detect ? 1 : 0;
        return OG_OK;
    });
}
int og_read_scope(og_engine* e, const char* node_path, uint32_t first_voice, uint32_t n_voices, uint32_t sample_count, float* samples, uint32_t* n_samples,
                  float* triggered, uint32_t* n_triggered)
{
    if (!e || !node_path) return set_err(OG_E_INVALID, "null argument");
    if ((samples && !n_samples) || (triggered && !n_triggered)) return set_err(OG_E_INVALID, "og_read_scope: rows without their lengths");
    return guard([&]() -> int {
        const int k = find_scope(e, node_path);
        if (k < 0) return set_err(OG_E_INVALID, std::string("no Oscilloscope named '") + node_path + "'");
        if ((uint64_t)first_voice + n_voices > e->V) return set_err(OG_E_INVALID, "voice range out of bounds");
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        if (!n_voices) return OG_OK;
        const auto& sp = e->cg->scopes[k];
        const auto& fr = e->cg->arrays[sp.ring_array];
        const auto& ff = e->cg->arrays[sp.frozen_array];
        const uint32_t V = e->V;
        // whole planes, as og_read_node_array: the planes of a field are contiguous, the columns of a voice range are not
        std::vector<float> ring((size_t)fr.length * V), frozen((size_t)ff.length * V);
        const int words[5] = {sp.w_write_pos, sp.w_written, sp.w_triggered_length, sp.w_window_end, sp.w_pending};
        std::vector<uint32_t> planes((size_t)5 * V);
        e->bounce.d2h(ring.data(), e->d_narr + (size_t)fr.base * V, ring.size() * 4, e->stream);
        e->bounce.d2h(frozen.data(), e->d_narr + (size_t)ff.base * V, frozen.size() * 4, e->stream);
        for (int w = 0; w < 5; ++w) e->bounce.d2h(planes.data() + (size_t)w * V, e->d_state + (size_t)words[w] * V, (size_t)V * 4, e->stream);
        HIPCK(hipStreamSynchronize(e->stream));
        const uint32_t row = sample_count < 1u ? 1u : sample_count; // (snapshot() hands out at least one sample)
        for (uint32_t i = 0; i < n_voices; ++i) {
            const uint32_t s = e->phys(first_voice + i);
            ogscope::Words w;
            w.write_pos = planes[s];
            w.written = planes[(size_t)V + s];
            w.triggered_length = planes[(size_t)2 * V + s];
            w.window_end = planes[(size_t)3 * V + s];
            w.pending = planes[(size_t)4 * V + s];
            ogscope::snapshot(sp.capacity, ogscope::Column{ring.data() + s, V}, ogscope::Column{frozen.data() + s, V}, w, sample_count,
                              samples ? samples + (size_t)i * row : nullptr, n_samples ? n_samples + i : nullptr,
                              triggered ? triggered + (size_t)i * sp.capacity : nullptr, n_triggered ? n_triggered + i : nullptr);
        }
        return OG_OK;
    });
}
int og_clear_scope_triggered(og_engine* e, const char* node_path, const uint32_t* voices, uint32_t n)
{
    if (!e || !node_path) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        const int k = find_scope(e, node_path);
        if (k < 0) return set_err(OG_E_INVALID, std::string("no Oscilloscope named '") + node_path + "'");
        for (uint32_t i = 0; voices && i < n; ++i)
            if (voices[i] >= e->V) return set_err(OG_E_INVALID, "voice " + std::to_string(voices[i]) + " out of bounds");
        HIPCK(hipSetDevice(e->device));
        e->flush_bus(); // queued blocks keep what they were queued under: the clear lands behind them, on a launch boundary
        const auto& sp = e->cg->scopes[k];
        // clear_triggered() (mod.rs:125-127): triggered_length = 0 -- and a window still pending in the ring is dropped with it
        for (const int w : {sp.w_triggered_length, sp.w_pending}) {
            uint32_t* d = e->d_state + (size_t)w * e->V;
            if (!voices) {
                HIPCK(hipMemsetAsync(d, 0, (size_t)e->V * 4, e->stream));
            } else if (n) {
                std::vector<uint32_t> plane(e->V);
                e->bounce.d2h(plane.data(), d, (size_t)e->V * 4, e->stream);
                HIPCK(hipStreamSynchronize(e->stream));
                for (uint32_t i = 0; i < n; ++i) plane[e->phys(voices[i])] = 0u;
                e->bounce.h2d(d, plane.data(), (size_t)e->V * 4, e->stream);
            }
        }
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}

int og_set_voice_taps(og_engine* e, const uint32_t* voices, uint32_t n)
{
    if (!e || (n && !voices)) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        HIPCK(hipStreamSynchronize(e->stream));
        std::vector<int32_t> slot(e->V, -1);
        for (uint32_t i = 0; i < n; ++i) {
            if (voices[i] >= e->V) throw std::runtime_error("tap voice out of range");
            slot[e->phys(voices[i])] = (int32_t)i;
        }
        e->bounce.h2d(e->d_tap_slot, slot.data(), (size_t)e->V * 4, e->stream);
        HIPCK(hipStreamSynchronize(e->stream));
        if (e->d_taps) HIPCK(hipFree(e->d_taps));
        e->d_taps = nullptr;
        if (n) {
            // (a Frame<2> voice output: [tap][frame][2])
            HIPCK(hipMalloc(&e->d_taps, (size_t)n * OG_MAX_BLOCK * 4 * e->cg->voice_channels));
            HIPCK(hipMemset(e->d_taps, 0, (size_t)n * OG_MAX_BLOCK * 4 * e->cg->voice_channels));
        }
        e->n_taps = n;
        e->tap_voices.assign(voices, voices + n); // the caller's voice numbers: og_load_state re-resolves them when it adopts another slot order
        return OG_OK;
    });
}

int og_read_voice_taps(og_engine* e, float* out, uint32_t n, uint32_t frames)
{
    if (!e || !out) return set_err(OG_E_INVALID, "null argument");
    if (n > e->n_taps || frames != e->last_frames) return set_err(OG_E_INVALID, "taps: n/frames do not match the last block");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        e->bounce.d2h(out, e->d_taps, (size_t)n * frames * 4 * e->cg->voice_channels, e->stream);
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}

uint32_t og_channels(const og_engine* e) { return e ? e->cg->channels : 0; }
uint32_t og_voice_channels(const og_engine* e) { return e ? e->cg->voice_channels : 0; }
int og_output_channel(const og_engine* e, const char* name, uint32_t* offset, uint32_t* width)
{
    return ogabi::guard([&]() -> int {
    if (!e || !name) return set_err(OG_E_INVALID, "null argument");
    for (const auto& oc : e->cg->output_channels)
        if (oc.name == name) {
            if (offset) *offset = (uint32_t)oc.offset;
            if (width) *width = (uint32_t)oc.width;
            return OG_OK;
        }
    return set_err(OG_E_INVALID, std::string("no stream output named '") + name + "' on the bus");
    });
}
uint32_t og_num_voices(const og_engine* e) { return e ? e->V : 0; }
uint32_t og_latency_samples(const og_engine* e) { return e ? e->cg->latency_samples : 0; }
// (Tremolo and Convolver are the post-mix node types the compiler takes -- og_graph.cpp, bus nodes -- and both are linear in
// their input)
int og_post_mix_kind(const og_engine* e) { return !e ? 0 : (e->cg->post ? 2 : (e->cg->bus_stage != ogc::BusStage::None ? 1 : 0)); }

int og_post_mix_info(const og_engine* e, uint32_t* n_nodes, uint32_t* in_channels, uint32_t* out_channels, uint32_t* state_words)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return guard([&] {
        if (!e->cg->post) throw ogabi::Error(OG_E_INVALID, "og_post_mix_info: this engine has no post-mix graph");
        const ogc::CompiledGraph& p = *e->cg->post;
        if (n_nodes) *n_nodes = (uint32_t)p.post_nodes.size();
        if (in_channels) *in_channels = e->cg->voice_channels;
        if (out_channels) *out_channels = e->cg->channels;
        if (state_words) *state_words = (uint32_t)p.state.size();
        return OG_OK;
    });
}

int og_read_post_mix_input(og_engine* e, float* out, uint32_t frames)
{
    if (!e || (frames && !out)) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        if (!e->cg->post) throw ogabi::Error(OG_E_INVALID, "og_read_post_mix_input: this engine has no post-mix graph");
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        if (frames > e->pm_last_frames)
            throw ogabi::Error(OG_E_INVALID, "og_read_post_mix_input: " + std::to_string(frames) + " frames asked for, the last launch rendered " +
                                                 std::to_string(e->pm_last_frames));
        const uint32_t vc = e->cg->voice_channels, first = e->pm_last_frames - frames;
        std::vector<float> row(frames);
        for (uint32_t c = 0; c < vc && frames; ++c) { // planar rows -> interleaved frames
            e->bounce.d2h(row.data(), e->d_pm_in + (size_t)c * e->cap_frames + first, (size_t)frames * 4, e->stream);
            for (uint32_t f = 0; f < frames; ++f) out[(size_t)f * vc + c] = row[f];
        }
        HIPCK(hipStreamSynchronize(e->stream));
        return OG_OK;
    });
}
uint64_t og_frames_processed(const og_engine* e) { return e ? e->frame_now : 0; }
uint32_t og_state_words_per_voice(const og_engine* e)
{
    return e ? (uint32_t)(e->cg->state.size() + e->cg->lane_state.size() * e->cg->lpv * e->cg->lane_width) : 0;
}
uint32_t og_state_words_written_per_voice(const og_engine* e)
{
    if (!e) return 0;
    uint32_t n = 0;
    for (const auto& w : e->cg->state) n += w.read_mostly ? 0u : 1u;
    for (const auto& w : e->cg->lane_state) n += w.read_mostly ? 0u : (uint32_t)(e->cg->lpv * e->cg->lane_width);
    return n;
}
uint32_t og_lanes_per_voice(const og_engine* e) { return e ? (uint32_t)e->cg->lpv : 0; }
int og_uses_split_kernel(const og_engine* e) { return e ? (int)e->split : 0; }
uint32_t og_voices_per_wave(const og_engine* e) { return e ? e->lanes / (uint32_t)e->cg->lpv : 0; }
// Side-effect free (a monitoring thread may poll it while the audio thread renders): host-side drops plus what
// og_sync_event_counters() last folded in from the device.
uint64_t og_events_dropped(const og_engine* e) { return e ? e->tl.dropped + e->ev_lost_total : 0; }

// in-voice event queues (#[output(event)] fields of user nodes) hold OG_NODE_EVENTS_PER_FRAME events per frame and
// output; what they could not hold is counted on the device.  This launches the queued blocks, reads that counter back
// (one small copy + a stream synchronise; graphs with such nodes only) and folds it into og_events_dropped().  Called
// by the thread that renders; og_synchronize() and og_read_output_events() do it as part of their own synchronise.
int og_sync_event_counters(og_engine* e)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    return guard([&] {
        e->sync_lost_counter();
        return OG_OK;
    });
}

uint32_t og_num_event_outputs(const og_engine* e) { return e ? (uint32_t)e->cg->event_outputs.size() : 0; }
int og_event_output_index(const og_engine* e, const char* name)
{
    return ogabi::guard([&]() -> int {
    if (!e || !name) return set_err(OG_E_INVALID, "null argument");
    for (size_t i = 0; i < e->cg->event_outputs.size(); ++i)
        if (e->cg->event_outputs[i] == name) return (int)i;
    return set_err(OG_E_INVALID, std::string("no event output named '") + name + "'");
    });
}

void og_engine::sync_lost_counter()
{
    if (!(d_out_ev_count && cg->has_node_event_outputs && inited)) return;
    HIPCK(hipSetDevice(device));
    flush_bus();
    uint32_t lost = 0;
    HIPCK(hipMemcpyAsync(&lost, d_out_ev_count + 1, sizeof lost, hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemsetAsync(d_out_ev_count + 1, 0, sizeof(uint32_t), stream));
    HIPCK(hipStreamSynchronize(stream));
    ev_lost_total += lost;
}

// Drains the device log into a host-side queue and hands out the oldest `cap` events; what does not fit the caller's
// buffer STAYS queued for the next call (round 3 threw it away).  `n_overflowed` counts only what the device log itself
// could not hold.
int og_read_output_events(og_engine* e, og_out_event* buf, uint32_t cap, uint32_t* n_out, uint64_t* n_overflowed)
{
    if (!e || (cap && !buf) || !n_out) return set_err(OG_E_INVALID, "null argument");
    *n_out = 0;
    if (n_overflowed) *n_overflowed = 0;
    if (!e->d_out_ev) return OG_OK; // (a graph without event outputs: nothing ever arrives)
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        uint32_t counters[2] = {0u, 0u}; // {events logged, in-voice pushes lost}
        HIPCK(hipMemcpyAsync(counters, e->d_out_ev_count, sizeof counters, hipMemcpyDeviceToHost, e->stream));
        HIPCK(hipStreamSynchronize(e->stream));
        const uint32_t count = counters[0];
        const uint32_t have = std::min(count, e->out_ev_cap);
        const size_t old = e->out_ev_carry.size();
        e->out_ev_carry.resize(old + have);
        try {
            if (have) e->bounce.d2h(e->out_ev_carry.data() + old, e->d_out_ev, (size_t)have * sizeof(OgOutEvent), e->stream);
            HIPCK(hipMemsetAsync(e->d_out_ev_count, 0, 2 * sizeof(uint32_t), e->stream));
            HIPCK(hipStreamSynchronize(e->stream));
        } catch (...) {
            e->out_ev_carry.resize(old); // (a failed copy leaves no half-filled records in the queue)
            throw;
        }
        e->out_ev_overflow += count - have;
        e->ev_lost_total += counters[1];
        if (!e->logical_of.empty()) // grouped voices: the log holds physical slots
            for (size_t i = old; i < e->out_ev_carry.size(); ++i) e->out_ev_carry[i].voice = e->logical_of[e->out_ev_carry[i].voice];
        // frame order; within a frame voice order; a voice's events of one frame in push order (the append index of
        // one lane grows in program order).  Events carried over from an earlier call lie on earlier frames.
        std::sort(e->out_ev_carry.begin() + (ptrdiff_t)old, e->out_ev_carry.end(), [](const OgOutEvent& a, const OgOutEvent& b) {
            if (a.frame != b.frame) return a.frame < b.frame;
            if (a.voice != b.voice) return a.voice < b.voice;
            return a.seq < b.seq;
        });
        const uint32_t give = (uint32_t)std::min<size_t>(e->out_ev_carry.size(), cap);
        for (uint32_t i = 0; i < give; ++i) {
            const OgOutEvent& x = e->out_ev_carry[i];
            buf[i] = og_out_event{x.voice, x.output, x.frame, x.value, 0u};
        }
        e->out_ev_carry.erase(e->out_ev_carry.begin(), e->out_ev_carry.begin() + give);
        *n_out = give;
        if (n_overflowed) {
            *n_overflowed = e->out_ev_overflow;
            e->out_ev_overflow = 0;
        }
        return OG_OK;
    });
}
uint64_t og_kernel_hash(const og_engine* e) { return e ? e->cg->hash : 0; }
int og_kernel_is_jit(const og_engine* e) { return e ? (e->launch ? 0 : 1) : 0; }
uint32_t og_bus_reduce_passes(const og_engine* e) { return e ? e->bus_passes : 0; }
uint32_t og_partial_rows(const og_engine* e) { return e ? e->n_wg : 0; }
const char* og_kernel_name(const og_engine* e)
{
    static thread_local char buf[64];
    if (!e) return "";
    snprintf(buf, sizeof buf, "og_k%s_%016llx%s", e->split == 4 ? (e->wide ? "4w" : "4") : (e->split == 2 ? "2" : ""), (unsigned long long)e->cg->hash,
             e->last_zero ? "_z" : "");
    return buf;
}
int og_kernel_fold_tier(const og_engine* e) { return e ? e->last_tier : 0; }
int og_event_stats(const og_engine* e, uint64_t* full_rebuilds, uint64_t* incremental_updates, uint64_t* resident_events)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (full_rebuilds) *full_rebuilds = e->tl.n_full_rebuilds;
    if (incremental_updates) *incremental_updates = e->tl.n_incremental;
    if (resident_events) *resident_events = (uint64_t)e->tl.resident_events();
    return OG_OK;
}

uint64_t og_event_ring_wraps(const og_engine* e) { return e ? e->tl.n_ring_wraps : 0; }
uint64_t og_events_copied(const og_engine* e) { return e ? e->tl.n_events_copied : 0; }

int og_reserve_events(og_engine* e, uint64_t n_events)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (n_events > 0xF0000000ull) return set_err(OG_E_INVALID, "og_reserve_events: at most 2^32 - 2^28 events");
    e->tl.reserve((size_t)n_events, e->d_events != nullptr); // takes effect with the next rebuild
    return OG_OK;
}

// Voice grouping for resident scores.  A wave renders 64 consecutive voice slots and takes, chunk by chunk, the cheapest body
// ALL of its lanes allow: one releasing lane puts the whole wave on the release arithmetic, one event or envelope stage end
// on the checked body.  With the voices of a bank in arbitrary order nearly every wave holds a releasing lane nearly all
// the time.  og_group_voices re-orders the SLOTS so that voices whose notes end at about the same time share waves --
// policy 1: by the frame of the voice's first scheduled note-off (an event-input event with a value <= 0), then by its
// first event of any kind -- and keeps a logical -> physical table: every entry point still takes and hands out the
// caller's voice numbers, per-voice samples are bit for bit those of the ungrouped bank, the summed bus differs by the
// association of the sum only.  Policy 0 restores the identity.  To be called after og_init and after the score has been
// scheduled, before the first block (the only per-voice state then are the per-voice value inputs, which move along).
int og_group_voices(og_engine* e, uint32_t policy)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (policy > 2u) return set_err(OG_E_INVALID, "og_group_voices: policy 0 (identity), 1 (by first note-off) or 2 (1 + waves dealt out by weight)");
    if (!e->inited) return set_err(OG_E_STATE, "og_init must be called before og_group_voices");
    if (e->frame_now != 0 || !e->queue.empty() || e->tl.has_resident() || e->tl.n_local() != 0)
        return set_err(OG_E_STATE, "og_group_voices: only before the first block (and before block-local pushes)");
    if (e->n_taps != 0) return set_err(OG_E_STATE, "og_group_voices: set the voice taps after grouping");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        const uint32_t V = e->V;
        std::vector<uint32_t> new_phys(V);
        if (policy == 0u) {
            for (uint32_t v = 0; v < V; ++v) new_phys[v] = v;
        } else {
            const uint64_t NONE = ~(uint64_t)0;
            std::vector<uint64_t> first_off(V, NONE), first_any(V, NONE);
            for (const HostEvent& h : e->tl.pending_events()) {
                const uint32_t v = e->logical(h.voice);
                first_any[v] = std::min(first_any[v], h.frame);
                if (!(h.target & OG_EV_SETVALUE) && h.value <= 0.0f) first_off[v] = std::min(first_off[v], h.frame);
            }
            std::vector<uint32_t> order(V);
            for (uint32_t v = 0; v < V; ++v) order[v] = v;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                if (first_off[a] != first_off[b]) return first_off[a] < first_off[b];
                return first_any[a] < first_any[b];
            });
            if (policy == 2u && V >= 2u * 256u * OG_WAVE) {
                // Policy 2 (experiment, not measured): the same waves, DEALT OUT.  With every workgroup of a launch resident
                // at once (65 536 voices = 1 024 workgroups = 4 per CU) a launch ends with the busiest CU; policy 1 leaves
                // the waves that hold the score's events next to each other in dispatch order.  Here the groups of 64 slots
                // are ranked by the number of events they hold and placed boustrophedon over rows of 256 groups -- row 0
                // left to right, row 1 right to left, ... -- so that groups i, i + 256, i + 512, ... (which share a CU if
                // workgroups are handed to the 256 CUs round robin: an assumption) add up to about the same weight.
                const uint32_t W = (V + OG_WAVE - 1) / OG_WAVE, ROW = 256u;
                std::vector<uint32_t> weight(W, 0u), rank(W);
                std::vector<uint32_t> slot_of(V);
                for (uint32_t r = 0; r < V; ++r) slot_of[order[r]] = r;
                for (const HostEvent& h : e->tl.pending_events()) weight[slot_of[e->logical(h.voice)] / OG_WAVE] += 1u;
                for (uint32_t w = 0; w < W; ++w) rank[w] = w;
                std::stable_sort(rank.begin(), rank.end(), [&](uint32_t a, uint32_t b) { return weight[a] > weight[b]; });
                std::vector<uint32_t> place(W); // place[k] = position of the k-th heaviest group
                for (uint32_t k = 0; k < W; ++k) {
                    const uint32_t row = k / ROW, col = k % ROW;
                    const uint32_t row_len = std::min(ROW, W - row * ROW);
                    place[k] = row * ROW + ((row & 1u) ? (row_len - 1u - std::min(col, row_len - 1u)) : col);
                }
                std::vector<uint32_t> group_pos(W);
                for (uint32_t k = 0; k < W; ++k) group_pos[rank[k]] = place[k];
                // (a last, partial group stays last: it is the lightest or is forced there)
                const bool partial = (V % OG_WAVE) != 0u;
                if (partial && group_pos[W - 1] != W - 1) {
                    for (uint32_t w = 0; w < W; ++w)
                        if (group_pos[w] == W - 1) {
                            group_pos[w] = group_pos[W - 1];
                            break;
                        }
                    group_pos[W - 1] = W - 1;
                }
                std::vector<uint32_t> dealt(V);
                for (uint32_t r = 0; r < V; ++r) dealt[r] = group_pos[r / OG_WAVE] * OG_WAVE + r % OG_WAVE;
                for (uint32_t r = 0; r < V; ++r) new_phys[order[r]] = dealt[r];
            } else {
                for (uint32_t r = 0; r < V; ++r) new_phys[order[r]] = r;
            }
        }
        // the per-voice value inputs move with their voices
        std::vector<float> plane(V), moved(V);
        for (size_t i = 0; i < e->cg->inputs.size(); ++i) {
            const auto& in = e->cg->inputs[i];
            if (!(in.decl.kind == ogc::Kind::Value && in.decl.per_voice)) continue;
            float* d = reinterpret_cast<float*>(e->d_state) + (size_t)in.state_word * V;
            e->bounce.d2h(plane.data(), d, (size_t)V * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
            for (uint32_t v = 0; v < V; ++v) moved[new_phys[v]] = plane[e->phys(v)];
            e->bounce.h2d(d, moved.data(), (size_t)V * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
        }
        // ... and so do array fields that were written (og_write_node_array) since og_init; untouched ones hold `init` everywhere
        for (size_t k = 0; e->narr_dirty && k < e->cg->arrays.size(); ++k) {
            const auto& f = e->cg->arrays[k];
            uint32_t* d = e->d_narr + (size_t)f.base * V;
            std::vector<uint32_t> from((size_t)f.length * V), to((size_t)f.length * V);
            e->bounce.d2h(from.data(), d, from.size() * 4, e->stream);
            for (uint32_t i = 0; i < f.length; ++i)
                for (uint32_t v = 0; v < V; ++v) to[(size_t)i * V + new_phys[v]] = from[(size_t)i * V + e->phys(v)];
            e->bounce.h2d(d, to.data(), to.size() * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
        }
        e->tl.remap_pending([&](uint32_t slot) { return new_phys[e->logical(slot)]; });
        bool identity = true;
        for (uint32_t v = 0; v < V && identity; ++v) identity = new_phys[v] == v;
        if (identity) {
            e->phys_of.clear();
            e->logical_of.clear();
        } else {
            e->logical_of.assign(V, 0u);
            for (uint32_t v = 0; v < V; ++v) e->logical_of[new_phys[v]] = v;
            e->phys_of.swap(new_phys);
        }
        return OG_OK;
    });
}
int og_voice_slot(const og_engine* e, uint32_t voice, uint32_t* slot)
{
    if (!e || !slot) return set_err(OG_E_INVALID, "null argument");
    if (voice >= e->V) return set_err(OG_E_INVALID, "voice index out of range");
    *slot = e->phys(voice);
    return OG_OK;
}

int og_blocking_stats(const og_engine* e, uint64_t* calls, uint64_t* marker_timeouts)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    if (calls) *calls = e->blocking_waits;
    if (marker_timeouts) *marker_timeouts = e->blocking_timeouts;
    return OG_OK;
}

int og_enable_kernel_timing(og_engine* e, int on)
{
    if (!e) return set_err(OG_E_INVALID, "null engine");
    e->timing = on != 0;
    e->t_used = 0;
    e->t_blocks = 0;
    return OG_OK;
}

uint64_t og_kernel_blocks_timed(const og_engine* e) { return e ? (uint64_t)e->t_blocks : 0; }

double og_kernel_time_ms(og_engine* e, uint32_t* n_launches)
{
    if (!e || !e->timing) return -1.0;
    double total = 0.0;
    (void)hipSetDevice(e->device);
    (void)og_flush(e);
    (void)hipStreamSynchronize(e->stream);
    for (size_t i = 0; i < e->t_used; ++i) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e->t_start[i], e->t_stop[i]) == hipSuccess) total += ms;
    }
    if (n_launches) *n_launches = (uint32_t)e->t_used;
    const double avg = e->t_used ? total / (double)e->t_used : 0.0;
    // the shader clock of those launches: total cycles / total 100 MHz ticks between the marks of workgroup 0
    double cyc = 0.0, ticks = 0.0;
    for (size_t i = 0; e->h_clock && i < e->t_used; ++i) {
        const unsigned long long* q = e->h_clock + 4 * i;
        if (q[3] > q[1] && q[2] > q[0]) {
            cyc += (double)(q[2] - q[0]);
            ticks += (double)(q[3] - q[1]);
        }
    }
    e->last_clock_ghz = ticks > 0.0 ? cyc / ticks * 0.1 : 0.0;
    e->t_used = 0;
    return avg;
}

/* the shader clock the launches of the LAST og_kernel_time_ms call ran at, measured by the voice kernel itself (0 where the
 * device has no such counters) */
double og_kernel_clock_ghz(const og_engine* e) { return e ? e->last_clock_ghz : 0.0; }

int og_shader_clock_ghz(og_engine* e, double* ghz)
{
    if (!e || !ghz) return set_err(OG_E_INVALID, "null argument");
    return guard([&]() -> int {
        HIPCK(hipSetDevice(e->device));
        unsigned long long* h = nullptr;
        HIPCK(hipHostMalloc((void**)&h, 2 * sizeof(unsigned long long), hipHostMallocDefault));
        h[0] = h[1] = 0ull;
        hipLaunchKernelGGL(og_clock_probe, dim3(1), dim3(64), 0, e->stream, h, 2000u); // 20 us
        const hipError_t rc = hipStreamSynchronize(e->stream);
        const unsigned long long cyc = h[0], ref = h[1];
        (void)hipHostFree(h);
        if (rc != hipSuccess) throw HipError(std::string("og_clock_probe: ") + hipGetErrorString(rc));
        if (ref == 0ull) return set_err(OG_E_UNSUPPORTED, "no shader clock counter on this device");
        *ghz = (double)cyc / (double)ref * 0.1; // cycles per 10 ns tick
        return OG_OK;
    });
}

} // extern "C"
