// og_snapshot.cpp -- state snapshots of an engine behind the C ABI: og_state_bytes, og_save_state, og_load_state.
#include "og_engine.h"
#include "og_post_mix_host.h"

// ---- state snapshot ---------------------------------------------------------------------------------------------
// blob = DSP state (state planes, lane arrays, post-mix phase, delay lines) + control block: frame counter, the value
// and ValueRampState of every input, the ramp counter and every event that has not fired yet (resident timeline and
// queued pushes).  Loading it into an engine of the same graph / voice count / sample rate continues the render
// sample for sample.
namespace {
struct SnapHeader {
    uint32_t magic, version;
    uint64_t frame_now;
    uint32_t n_inputs, active_ramps;
    uint64_t n_events;
};
struct SnapRamp {
    float current, target, increment;
    uint32_t frames_remaining;
};
struct SnapEvent {
    uint32_t voice, target;
    uint64_t frame;
    float value;
    uint32_t block_local;
};
constexpr uint32_t SNAP_MAGIC = 0x3253474Fu; // "OGS2"
// Post-mix Convolver: a section of its own BEHIND everything else (its size depends on the live responses, which a blob
// brings along): header, taps of the current response, taps of the outgoing one, then the history -- the last
// max(K) - 1 frames of the dry bus, interleaved.  A swap that no block has picked up yet is not part of the state.
struct SnapConv {
    uint32_t magic, channels;
    uint32_t k_cur, k_old; // k_old = 0xFFFFFFFF: no fade in progress
    uint64_t cur_from, old_from, fade_start;
    uint32_t hist_frames, reserved;
};
constexpr uint32_t SNAP_CONV_MAGIC = 0x56434E4Fu; // "ONCV"
// ... and, ONLY when a live response has one tap plane per channel (an asset response, og_set_bus_ir; a blob without one
// stays what it was), the section has another magic and `reserved` holds the planes of the two responses (current | outgoing
// << 16); the taps of a response are then its planes back to back, k taps each
constexpr uint32_t SNAP_CONVP_MAGIC = 0x50434E4Fu; // "ONCP"
size_t conv_bytes(const og_engine* e)
{
    if (!e->conv_on()) return 0;
    const ConvCfg& cv = e->bus_conv.cfg();
    return sizeof(SnapConv) + ((cv.cur ? cv.cur->taps.size() : 0u) + (cv.old ? cv.old->taps.size() : 0u) +
                               e->bus_conv.tail_frames() * e->cg->voice_channels) * 4;
}

// SamplePlayer: a section of its own at the very end -- the loaded samples' names and shapes in index order (the per-voice
// words are state planes like any other); og_load_state resolves the names through the registry and loads them
struct SnapSamples {
    uint32_t magic, n;
};
struct SnapSample {
    uint32_t name_len, frames, channels, reserved;
};
constexpr uint32_t SNAP_SMP_MAGIC = 0x504D534Fu; // "OSMP"
// ... and, ONLY when a sample registered at a rate is loaded (a blob without one stays what it was), the section has another
// magic and every entry is followed by the rates: og_load_state conforms again from the registry and compares
struct SnapSampleRate {
    uint32_t src_rate, rate, pool_frames, reserved; // src_rate 0: an untagged sample among tagged ones
};
constexpr uint32_t SNAP_SMPR_MAGIC = 0x524D534Fu; // "OSMR"
bool samples_tagged(const og_engine* e)
{
    for (const auto& ls : e->samples)
        if (ls.src_rate) return true;
    return false;
}
size_t samples_bytes(const og_engine* e)
{
    if (e->cg->players.empty()) return 0;
    size_t n = sizeof(SnapSamples);
    const size_t extra = samples_tagged(e) ? sizeof(SnapSampleRate) : 0;
    for (const auto& ls : e->samples) n += sizeof(SnapSample) + (ls.name.size() + 3) / 4 * 4 + extra;
    return n;
}

// Array fields of registered node types: a section of their own behind the delay lines, ONLY in blobs of graphs that have
// such a field -- a head naming the fields' lengths (og_node_array_host.h), then the node-array pool as it lies on the device
size_t narr_section_bytes(const og_engine* e) { return e->cg->arrays.empty() ? 0 : ognarr::section_head_bytes(e->cg->arrays) + e->narr_bytes(); }
size_t dsp_bytes(const og_engine* e)
{
    return (e->cg->state.size() + e->cg->lane_state.size() * e->cg->lpv * e->cg->lane_width) * (size_t)e->V * 4 +
           (e->cg->bus_stage == ogc::BusStage::Tremolo ? 4 : 0) + e->ring_bytes() + narr_section_bytes(e);
}
// Every event that has not fired by frame_now.  Blocks that are still queued (og_set_bus_batching) consume the events
// in [q_frame0, frame_now) when they are launched, and the snapshot header stores the post-queue frame_now: those
// events must not be saved (they would fire a second time after a load -- ADVICE r2), so the horizon is frame_now,
// not consumed_horizon().  og_save_state launches the queue first; og_state_bytes only counts.
void collect_unconsumed(const og_engine* e, std::vector<SnapEvent>& out)
{
    const uint64_t hz = e->frame_now;
    std::vector<TlEvent> old;
    if (e->tl.has_resident())
        for (uint32_t v = 0; v < e->V; ++v) {
            old.clear();
            e->tl.resident_unconsumed(v, hz, old); // the voice's segment, then its continuation
            for (const TlEvent& ev : old) out.push_back(SnapEvent{v, ev.target, ev.frame, ev.value, 0u});
        }
    for (const HostEvent& h : e->tl.pending_events())
        if (h.frame >= hz) out.push_back(SnapEvent{h.voice, h.target, h.frame, h.value, h.block_local ? 1u : 0u});
}
// (a blob of an engine with grouped voices -- og_group_voices -- is version 3: the state planes and the events are in
//  PHYSICAL order, and the logical -> physical table follows the events; loading it adopts the table)
size_t control_bytes(const og_engine* e, size_t n_events, bool grouped)
{
    return sizeof(SnapHeader) + e->cg->inputs.size() * (sizeof(float) + sizeof(SnapRamp)) + n_events * sizeof(SnapEvent) +
           (grouped ? (size_t)e->V * sizeof(uint32_t) : 0);
}
size_t control_bytes(const og_engine* e, size_t n_events) { return control_bytes(e, n_events, !e->phys_of.empty()); }

// Post-mix graph: a section of its own at the very END of the blob (og_post_mix_host.h), only in blobs of graphs that have
// one -- the second state image and its delay lines
ogpm::Layout post_layout(const og_engine* e)
{
    ogpm::Layout l;
    if (!e->post_on()) return l;
    for (const auto& w : e->cg->post->state) l.state_names.push_back(w.name);
    for (size_t k = 0; k < e->cg->post->rings.size(); ++k) l.ring_caps.push_back(e->pm_ring_cap[k]);
    return l;
}
size_t post_bytes(const og_engine* e) { return e->post_on() ? ogpm::section_bytes(post_layout(e)) : 0; }
} // namespace

extern "C" {

size_t og_state_bytes(const og_engine* e)
{
    return ogabi::guard_value<size_t>((size_t)0, [&]() -> size_t {
    // (delay lines are part of the state: their size is known once og_init has sized them)
    if (!e) return 0;
    std::vector<SnapEvent> evs;
    collect_unconsumed(e, evs);
    return dsp_bytes(e) + control_bytes(e, evs.size()) + conv_bytes(e) + samples_bytes(e) + post_bytes(e);
    });
}

int og_save_state(og_engine* e, void* dst, size_t cap)
{
    if (!e || !dst) return set_err(OG_E_INVALID, "null argument");
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus(); // queued blocks consume their events first: what is collected below is what frame_now has not reached
        std::vector<SnapEvent> evs;
        collect_unconsumed(e, evs);
        if (cap < dsp_bytes(e) + control_bytes(e, evs.size()) + conv_bytes(e) + samples_bytes(e) + post_bytes(e)) throw std::runtime_error("buffer too small");
        const size_t a = e->cg->state.size() * (size_t)e->V * 4, b = e->cg->lane_state.size() * (size_t)e->V * e->cg->lpv * e->cg->lane_width * 4;
        e->bounce.d2h(dst, e->d_state, a, e->stream);
        if (b) e->bounce.d2h((char*)dst + a, e->d_lane_state, b, e->stream);
        if (e->d_bus_phase) HIPCK(hipMemcpyAsync((char*)dst + a + b, e->d_bus_phase, 4, hipMemcpyDeviceToHost, e->stream));
        size_t off = a + b + (e->d_bus_phase ? 4 : 0);
        for (size_t k = 0; k < e->cg->rings.size(); ++k) {
            const size_t n = (size_t)e->ring_cap[k] * e->V * 4;
            if (n) e->bounce.d2h((char*)dst + off, e->d_ring[k], n, e->stream);
            off += n;
        }
        if (!e->cg->arrays.empty()) {
            ognarr::write_section_head(e->cg->arrays, (char*)dst + off);
            off += ognarr::section_head_bytes(e->cg->arrays);
            e->bounce.d2h((char*)dst + off, e->d_narr, e->narr_bytes(), e->stream);
            off += e->narr_bytes();
        }
        HIPCK(hipStreamSynchronize(e->stream));
        char* p = (char*)dst + off;
        const SnapHeader h{SNAP_MAGIC, e->phys_of.empty() ? 2u : 3u, e->frame_now, (uint32_t)e->cg->inputs.size(), e->active_ramps, (uint64_t)evs.size()};
        memcpy(p, &h, sizeof h);
        p += sizeof h;
        memcpy(p, e->values.data(), e->values.size() * sizeof(float));
        p += e->values.size() * sizeof(float);
        for (const Ramp& r : e->ramps) {
            const SnapRamp sr{r.current, r.target, r.increment, r.frames_remaining};
            memcpy(p, &sr, sizeof sr);
            p += sizeof sr;
        }
        if (!evs.empty()) memcpy(p, evs.data(), evs.size() * sizeof(SnapEvent));
        p += evs.size() * sizeof(SnapEvent);
        if (!e->phys_of.empty()) memcpy(p, e->phys_of.data(), (size_t)e->V * sizeof(uint32_t));
        p += e->phys_of.empty() ? 0 : (size_t)e->V * sizeof(uint32_t);
        if (e->conv_on()) {
            const ConvCfg& cv = e->bus_conv.cfg();
            const uint32_t kc = ConvCfg::taps_of(cv.cur), ko = ConvCfg::taps_of(cv.old);
            const uint32_t pc = ConvCfg::planes_of(cv.cur), po = ConvCfg::planes_of(cv.old);
            const size_t hf = e->bus_conv.tail_frames(), vc = e->cg->voice_channels;
            const bool per_channel = cv.per_channel();
            const size_t nc = (size_t)kc * pc, no = (size_t)ko * po;
            const SnapConv sc{per_channel ? SNAP_CONVP_MAGIC : SNAP_CONV_MAGIC, (uint32_t)vc, kc, cv.old ? ko : 0xFFFFFFFFu, cv.cur_from, cv.old_from, cv.fade_start, (uint32_t)hf,
                              per_channel ? (pc | (po << 16)) : 0u};
            memcpy(p, &sc, sizeof sc);
            p += sizeof sc;
            if (nc) memcpy(p, cv.cur->taps.data(), nc * 4);
            p += nc * 4;
            if (no) memcpy(p, cv.old->taps.data(), no * 4);
            p += no * 4;
            if (hf) e->bounce.d2h(p, e->d_hist + e->bus_conv.tail_at(hf) * vc, hf * vc * 4, e->stream);
            p += hf * vc * 4;
        }
        if (!e->cg->players.empty()) {
            const bool tagged = samples_tagged(e);
            const SnapSamples sh{tagged ? SNAP_SMPR_MAGIC : SNAP_SMP_MAGIC, (uint32_t)e->samples.size()};
            memcpy(p, &sh, sizeof sh);
            p += sizeof sh;
            for (const auto& ls : e->samples) {
                const SnapSample ss{(uint32_t)ls.name.size(), ls.frames, ls.channels, 0u};
                memcpy(p, &ss, sizeof ss);
                p += sizeof ss;
                const size_t padded = (ls.name.size() + 3) / 4 * 4;
                memset(p, 0, padded);
                memcpy(p, ls.name.data(), ls.name.size());
                p += padded;
                if (tagged) {
                    const SnapSampleRate sr{ls.src_rate, ls.rate, ls.pool_frames, 0u};
                    memcpy(p, &sr, sizeof sr);
                    p += sizeof sr;
                }
            }
        }
        if (e->post_on()) {
            const ogpm::Layout l = post_layout(e);
            const ogpm::SectionHead ph = ogpm::make_head(l);
            memcpy(p, &ph, sizeof ph);
            if (!l.state_names.empty()) e->bounce.d2h(p + ogpm::words_offset(), e->d_pm_state, l.state_names.size() * 4, e->stream);
            size_t at = ogpm::rings_offset(l);
            for (size_t k = 0; k < l.ring_caps.size(); ++k) {
                if (l.ring_caps[k]) e->bounce.d2h(p + at, e->d_pm_ring[k], (size_t)l.ring_caps[k] * 4, e->stream);
                at += (size_t)l.ring_caps[k] * 4;
            }
            HIPCK(hipStreamSynchronize(e->stream));
            p += at;
        }
        return OG_OK;
    });
}

int og_load_state(og_engine* e, const void* src, size_t len)
{
    if (!e || !src) return set_err(OG_E_INVALID, "null argument");
    // the post-mix graph's section closes the blob: its head is checked before anything is believed, and everything below
    // sees the blob without it
    const size_t pm_bytes = post_bytes(e);
    ogpm::Layout pm_layout;
    if (pm_bytes) {
        const int rc = ogabi::guard([&]() -> int {
            pm_layout = post_layout(e);
            const size_t at = len > pm_bytes ? len - pm_bytes : 0;
            const std::string bad = ogpm::check(pm_layout, (const char*)src + at, len - at);
            return bad.empty() ? OG_OK : set_err(OG_E_INVALID, bad);
        });
        if (rc != OG_OK) return rc;
        len -= pm_bytes;
    }
    const char* const pm_src = (const char*)src + len;
    const size_t dsp = dsp_bytes(e);
    if (!e->cg->arrays.empty()) { // the node-array section names its fields: checked before anything else is believed
        const int rc = ogabi::guard([&]() -> int {
            const size_t at = dsp - narr_section_bytes(e);
            const std::string bad = ognarr::check_section_head(e->cg->arrays, (const char*)src + std::min(at, len), len > at ? len - at : 0);
            return bad.empty() ? OG_OK : set_err(OG_E_INVALID, bad);
        });
        if (rc != OG_OK) return rc;
    }
    if (len < dsp + sizeof(SnapHeader)) return set_err(OG_E_INVALID, "state blob size mismatch");
    SnapHeader h;
    memcpy(&h, (const char*)src + dsp, sizeof h);
    // (n_events is checked against the bytes that are there BEFORE it enters any size arithmetic: a crafted count must
    //  not wrap control_bytes() around to a matching length)
    const bool grouped = h.version == 3u;
    const size_t fixed = control_bytes(e, 0, grouped);
    if (h.magic != SNAP_MAGIC || (h.version != 2u && h.version != 3u) || h.n_inputs != e->cg->inputs.size() || len < dsp + fixed ||
        h.n_events > (uint64_t)((len - dsp - fixed) / sizeof(SnapEvent)) || len < dsp + control_bytes(e, (size_t)h.n_events, grouped))
        return set_err(OG_E_INVALID, "state blob does not belong to this graph / voice count (or is from another version)");
    size_t full_len = len;
    len = dsp + control_bytes(e, (size_t)h.n_events, grouped); // what follows is the post-mix Convolver's section
    // ... and, last, the SamplePlayer section: found from the front (behind the Convolver's, whose size its header gives)
    struct WantSample {
        std::string name;
        uint32_t frames, channels;
        uint32_t src_rate, rate, pool_frames;
    };
    std::vector<WantSample> want_samples;
    if (!e->cg->players.empty()) {
        const int rc = ogabi::guard([&]() -> int {
            size_t at = len;
            if (e->conv_on()) {
                SnapConv pc{};
                if (full_len - at < sizeof pc) return set_err(OG_E_INVALID, "state blob: the post-mix Convolver's section is missing or malformed");
                memcpy(&pc, (const char*)src + at, sizeof pc);
                const uint64_t ko = pc.k_old == 0xFFFFFFFFu ? 0u : pc.k_old;
                const uint64_t pl_cur = pc.magic == SNAP_CONVP_MAGIC ? (pc.reserved & 0xFFFFu) : 1u, pl_old = pc.magic == SNAP_CONVP_MAGIC ? (pc.reserved >> 16) : 1u;
                const uint64_t n = sizeof pc + ((uint64_t)pc.k_cur * pl_cur + ko * pl_old + (uint64_t)pc.hist_frames * pc.channels) * 4;
                if (n > full_len - at) return set_err(OG_E_INVALID, "state blob: the post-mix Convolver's section is missing or malformed");
                at += (size_t)n;
            }
            const size_t smp_at = at;
            SnapSamples sh{};
            bool ok = full_len - at >= sizeof sh;
            if (ok) memcpy(&sh, (const char*)src + at, sizeof sh);
            const bool tagged = ok && sh.magic == SNAP_SMPR_MAGIC;
            ok = ok && (sh.magic == SNAP_SMP_MAGIC || tagged);
            at += sizeof sh;
            for (uint32_t i = 0; ok && i < sh.n; ++i) {
                SnapSample ss{};
                ok = full_len - at >= sizeof ss;
                if (!ok) break;
                memcpy(&ss, (const char*)src + at, sizeof ss);
                at += sizeof ss;
                const size_t padded = ((size_t)ss.name_len + 3) / 4 * 4;
                ok = ss.name_len <= 4096u && full_len - at >= padded;
                if (!ok) break;
                want_samples.push_back({std::string((const char*)src + at, ss.name_len), ss.frames, ss.channels, 0u, 0u, ss.frames});
                at += padded;
                if (tagged) {
                    SnapSampleRate sr{};
                    ok = full_len - at >= sizeof sr;
                    if (!ok) break;
                    memcpy(&sr, (const char*)src + at, sizeof sr);
                    at += sizeof sr;
                    want_samples.back().src_rate = sr.src_rate;
                    want_samples.back().rate = sr.rate;
                    want_samples.back().pool_frames = sr.pool_frames;
                }
            }
            if (!ok || at != full_len) return set_err(OG_E_INVALID, "state blob: the SamplePlayer section is missing or malformed");
            // every sample must be there, in the shape it was saved with, before anything is changed
            for (size_t i = 0; i < want_samples.size(); ++i) {
                const WantSample& w = want_samples[i];
                if (i < e->samples.size()) {
                    const auto& ls = e->samples[i];
                    if (ls.name != w.name || ls.frames != w.frames || ls.channels != w.channels || ls.src_rate != w.src_rate ||
                        ls.pool_frames != w.pool_frames)
                        return set_err(OG_E_INVALID, "state blob: sample " + std::to_string(i) + " is '" + w.name + "', this engine has loaded '" + ls.name + "' there");
                    continue;
                }
                const auto sd = lookup_sample(w.name);
                if (!sd) return set_err(OG_E_INVALID, "state blob: sample '" + w.name + "' is not registered (og_register_sample)");
                if (sd->frames != w.frames || sd->channels != w.channels)
                    return set_err(OG_E_INVALID, "state blob: sample '" + w.name + "' is registered with another shape than the one it was saved with");
                if (sd->rate != w.src_rate)
                    return set_err(OG_E_INVALID, "state blob: sample '" + w.name + "' was saved at source rate " + std::to_string(w.src_rate) + ", it is registered at " + std::to_string(sd->rate) + " (0: no rate)");
                if (sd->rate && (e->graph_rate("og_load_state") != w.rate ||
                                 og_engine::conformed_frames(w.name, *sd, w.rate) != w.pool_frames))
                    return set_err(OG_E_INVALID, "state blob: sample '" + w.name + "' was saved with " + std::to_string(w.pool_frames) + " frames conformed to " + std::to_string(w.rate) + " Hz; this engine's rate or the registered data give another length");
            }
            full_len = smp_at;
            return OG_OK;
        });
        if (rc != OG_OK) return rc;
    }
    SnapConv sc{};
    uint32_t pl_cur = 1, pl_old = 1; // tap planes of the two responses
    if (e->conv_on()) {
        bool ok = full_len - len >= sizeof sc;
        if (ok) memcpy(&sc, (const char*)src + len, sizeof sc);
        const bool per_channel = ok && sc.magic == SNAP_CONVP_MAGIC;
        if (per_channel) {
            pl_cur = sc.reserved & 0xFFFFu;
            pl_old = sc.reserved >> 16;
            // a plane per bus channel or one shared plane, and at least one response with planes of its own
            ok = (pl_cur == 1 || pl_cur == sc.channels) && (pl_old == 1 || pl_old == sc.channels) && (pl_cur > 1 || pl_old > 1) &&
                 (pl_cur == 1 || sc.k_cur > 0) && (pl_old == 1 || (sc.k_old != 0xFFFFFFFFu && sc.k_old > 0));
        }
        ok = ok && (sc.magic == SNAP_CONV_MAGIC || per_channel) && sc.channels == e->cg->voice_channels && sc.k_cur <= ogc::MAX_IR_TAPS &&
             (sc.k_old == 0xFFFFFFFFu || sc.k_old <= ogc::MAX_IR_TAPS);
        const uint64_t ko = sc.k_old == 0xFFFFFFFFu ? 0u : sc.k_old, kmax = std::max<uint64_t>(sc.k_cur, ko);
        ok = ok && sc.hist_frames == (kmax ? kmax - 1 : 0) &&
             full_len - len == sizeof sc + ((size_t)sc.k_cur * pl_cur + ko * pl_old + (size_t)sc.hist_frames * sc.channels) * 4;
        if (!ok) return set_err(OG_E_INVALID, "state blob: the post-mix Convolver's section is missing or malformed");
    } else if (full_len != len) {
        return set_err(OG_E_INVALID, "state blob does not belong to this graph / voice count (or is from another version)");
    }
    std::vector<uint32_t> new_phys, new_logical;
    if (grouped) { // the voice order must be a permutation before anything is changed
        new_phys.resize(e->V);
        new_logical.assign(e->V, 0xFFFFFFFFu);
        memcpy(new_phys.data(), (const char*)src + len - (size_t)e->V * sizeof(uint32_t), (size_t)e->V * sizeof(uint32_t));
        for (uint32_t v = 0; v < e->V; ++v) {
            if (new_phys[v] >= e->V || new_logical[new_phys[v]] != 0xFFFFFFFFu) return set_err(OG_E_INVALID, "state blob: the voice order is not a permutation");
            new_logical[new_phys[v]] = v;
        }
    }
    { // validate the events before anything is changed: the kernel indexes handlers / per-voice inputs by `target`
        const char* q = (const char*)src + dsp + control_bytes(e, 0, false);
        for (uint64_t i = 0; i < h.n_events; ++i, q += sizeof(SnapEvent)) {
            SnapEvent ev;
            memcpy(&ev, q, sizeof ev);
            bool ok = ev.voice < e->V;
            if (ev.target & OG_EV_SETVALUE) {
                const uint32_t in = ev.target & ~OG_EV_SETVALUE;
                ok = ok && in < e->cg->inputs.size() && e->cg->inputs[in].decl.kind == ogc::Kind::Value && e->cg->inputs[in].decl.per_voice;
            } else {
                ok = ok && (int)ev.target < e->cg->n_event_inputs;
            }
            if (!ok) return set_err(OG_E_INVALID, "state blob: event " + std::to_string(i) + " addresses a voice or input this graph does not have");
        }
    }
    return guard([&] {
        HIPCK(hipSetDevice(e->device));
        e->flush_bus();
        const size_t a = e->cg->state.size() * (size_t)e->V * 4, b = e->cg->lane_state.size() * (size_t)e->V * e->cg->lpv * e->cg->lane_width * 4;
        e->bounce.h2d(e->d_state, src, a, e->stream);
        if (b) e->bounce.h2d(e->d_lane_state, (const char*)src + a, b, e->stream);
        if (e->d_bus_phase) HIPCK(hipMemcpyAsync(e->d_bus_phase, (const char*)src + a + b, 4, hipMemcpyHostToDevice, e->stream));
        size_t off = a + b + (e->d_bus_phase ? 4 : 0);
        for (size_t k = 0; k < e->cg->rings.size(); ++k) {
            const size_t n = (size_t)e->ring_cap[k] * e->V * 4;
            if (n) e->bounce.h2d(e->d_ring[k], (const char*)src + off, n, e->stream);
            off += n;
        }
        if (!e->cg->arrays.empty()) {
            off += ognarr::section_head_bytes(e->cg->arrays);
            e->bounce.h2d(e->d_narr, (const char*)src + off, e->narr_bytes(), e->stream);
            e->narr_dirty = true;
            off += e->narr_bytes();
        }
        if (pm_bytes) {
            if (!pm_layout.state_names.empty()) e->bounce.h2d(e->d_pm_state, pm_src + ogpm::words_offset(), pm_layout.state_names.size() * 4, e->stream);
            size_t at = ogpm::rings_offset(pm_layout);
            for (size_t k = 0; k < pm_layout.ring_caps.size(); ++k) {
                if (pm_layout.ring_caps[k]) e->bounce.h2d(e->d_pm_ring[k], pm_src + at, (size_t)pm_layout.ring_caps[k] * 4, e->stream);
                at += (size_t)pm_layout.ring_caps[k] * 4;
            }
        }
        e->reset_timeline();
        HIPCK(hipStreamSynchronize(e->stream));
        for (size_t i = e->samples.size(); i < want_samples.size(); ++i) { // (validated above; the registry may have changed since)
            const auto sd = lookup_sample(want_samples[i].name);
            if (!sd || sd->frames != want_samples[i].frames || sd->channels != want_samples[i].channels || sd->rate != want_samples[i].src_rate)
                throw ogabi::Error(OG_E_INVALID, "state blob: sample '" + want_samples[i].name + "' is not registered in the shape it was saved with");
            (void)e->load_sample(want_samples[i].name, *sd);
        }
        if (e->conv_on()) {
            const size_t vc = e->cg->voice_channels;
            const size_t ko = sc.k_old == 0xFFFFFFFFu ? 0u : sc.k_old;
            const float* q = (const float*)((const char*)src + len + sizeof sc);
            const size_t kmax = std::max<size_t>(sc.k_cur, ko); // (validated above: hist_frames is its reach)
            if (e->bus_conv.outgrows(kmax)) e->conv_alloc(kmax);
            const size_t nc = (size_t)sc.k_cur * pl_cur, no = ko * pl_old;
            auto cur = e->conv_upload(q, sc.k_cur, pl_cur);
            e->bus_conv.restore(cur, sc.k_old == 0xFFFFFFFFu ? nullptr : e->conv_upload(q + nc, ko, pl_old), sc.cur_from, sc.old_from, sc.fade_start);
            e->conv_clear_history();
            if (sc.hist_frames)
                e->bounce.h2d(e->d_hist + e->bus_conv.tail_at(sc.hist_frames) * vc, q + nc + no, (size_t)sc.hist_frames * vc * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
            e->conv_gc();
        }
        const bool order_changed = e->phys_of != new_phys;
        e->phys_of.swap(new_phys); // (version 2: identity)
        e->logical_of.swap(new_logical);
        if (order_changed && e->n_taps) { // taps were resolved to physical slots under the old order: resolve the SAME voices again
            std::vector<int32_t> slot(e->V, -1);
            for (uint32_t i = 0; i < e->n_taps; ++i) slot[e->phys(e->tap_voices[i])] = (int32_t)i;
            e->bounce.h2d(e->d_tap_slot, slot.data(), (size_t)e->V * 4, e->stream);
            HIPCK(hipStreamSynchronize(e->stream));
        }
        const char* p = (const char*)src + off + sizeof h;
        memcpy(e->values.data(), p, e->values.size() * sizeof(float));
        p += e->values.size() * sizeof(float);
        for (Ramp& r : e->ramps) {
            SnapRamp sr;
            memcpy(&sr, p, sizeof sr);
            p += sizeof sr;
            r.current = sr.current;
            r.target = sr.target;
            r.increment = sr.increment;
            r.frames_remaining = sr.frames_remaining;
        }
        e->active_ramps = h.active_ramps;
        e->frame_now = h.frame_now;
        for (uint64_t i = 0; i < h.n_events; ++i) {
            SnapEvent ev;
            memcpy(&ev, p, sizeof ev);
            p += sizeof ev;
            const bool local = ev.block_local != 0u;
            e->tl.push(ev.voice, std::max(ev.frame, h.frame_now), ev.target, ev.value, local);
            // the try_push capacity count of the block being assembled
            if (local && !(ev.target & OG_EV_SETVALUE)) (void)e->tl.count_local(ev.voice, ev.target, (size_t)std::max(1, e->cg->n_event_inputs), 255u);
        }
        return OG_OK;
    });
}

} // extern "C"
