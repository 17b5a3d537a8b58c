// og_timeline.h -- the event timeline's host bookkeeping: where every pushed event lands in the device ring.
// Host C++17 only (no HIP): the engine (og_engine.h) does the device work between the plan and the commit half of each of the
// two update paths; tests/standalone/timeline_model_main.cpp holds the class against a naive model on the CPU.
//
// Device: d_events holds every voice's unconsumed events as one segment [cursor, end), sorted by
// (frame, push order).  A full rebuild lays the segments out in voice order (CSR) and uploads
// O(V) words; the incremental path (live pushes: og_push_voice_event / MIDI) appends a new segment
// for each voice that received events -- its unconsumed old events merged with the new ones -- at the
// tail of d_events and repoints that voice's (cursor, end) with a tiny kernel: O(#pushes) host work,
// one async copy from a pinned staging ring, no stream synchronisation.
//
// The timeline never looks at the block queue: the consumed horizon `hz` (everything before it has been consumed on the
// device by the time an update issued now takes effect) and the end `lend` of the launch being prepared (everything before
// it must be in the voices' segments) are arguments.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <stdexcept>
#include <utility>
#include <vector>

// og_apply_event_updates (og_engine.cpp) reads upd = n x {voice, cursor, end}
constexpr size_t EV_UPD_WORDS = 3;

// One record of the ring.  The kernels read it as OgEvent (og_kernel_rt.hip.h, a device header this one cannot include):
// the engine asserts that the two layouts are one.
struct TlEvent {
    uint64_t frame;  // absolute frame since og_init
    uint32_t target; // event-input index, or OG_EV_SETVALUE | per-voice value index
    float value;
};

struct HostEvent { // a push that has not reached the device timeline yet
    uint32_t voice;
    uint64_t frame;
    uint32_t target;
    float value;
    uint64_t seq;
    bool block_local; // pushed relative to the next block (reference try_push semantics)
};

class EventTimeline {
public:
    static constexpr size_t STAGE_EVENTS = 131072;      // events (and voice updates) one staging buffer holds (8 x 2 MB + 8 x 1.5 MB pinned)
    static constexpr size_t HEADROOM = (size_t)2 << 20; // room for appended segments (2 M events, 32 MB) before the ring has to wrap
    // A rest shorter than this is carried over with the merge: copying a kilobyte costs less than the bookkeeping of a
    // continuation (a heap entry, a second cursor update, two more looks into the cold host mirror) -- measured on the loaded
    // real-time banks, whose 1 s scores leave ~14 events per voice: with continuations for those p99 rose from 2.29 to
    // 2.69 ms at 4 194 304 voices (gpurun r06q).
    static constexpr uint32_t CONT_MIN = 64;
    static constexpr size_t CAP_MAX = 0xFFFFFFF0ull; // ring positions are 32-bit

    // headroom: OSCEN_GPU_EV_HEADROOM (tests: force compactions), read at og_create
    explicit EventTimeline(uint32_t voices = 0, size_t stage_events = STAGE_EVENTS, size_t headroom = HEADROOM)
        : V(voices), stage_cap(stage_events), ev_headroom(headroom) {}

    uint64_t n_full_rebuilds = 0, n_incremental = 0;
    uint64_t n_events_copied = 0; // events written to the ring by incremental updates (old ones carried over + new ones)
    uint64_t n_ring_wraps = 0;
    uint64_t dropped = 0;
    // how often each branch of the incremental path ran.  Test instrumentation that the engine's instance carries too
    // (tests/standalone/timeline_model_main.cpp fails a run that missed a branch): one add per merged voice at most.
    struct Paths {
        uint64_t fast = 0, short_merge = 0, cont_left = 0, in_place = 0, stale_due = 0;
    } paths;

    bool wants_rebuild() const { return ev_rebuild; } // next block must rebuild the whole timeline
    size_t stage_events() const { return stage_cap; }
    size_t capacity() const { return ev_cap; }
    size_t resident_events() const { return ev_tail; } // next free slot of d_events
    size_t n_pending() const { return pending.size(); }
    size_t n_local() const { return n_block_local; }
    bool has_resident() const { return !h_events.empty(); }
    const std::vector<HostEvent>& pending_events() const { return pending; } // (PHYSICAL voice slots)

    void reset()
    {
        pending.clear();
        local_from = 0;
        h_events.clear();
        seg_begin.clear();
        seg_end.clear();
        seg_last.clear();
        cont_begin.clear();
        cont_end.clear();
        cont_last.clear();
        cont_due.clear();
        n_conts = 0;
        ev_tail = 0;
        ring_live.clear();
        ev_rebuild = false;
        n_block_local = 0;
        clear_local_counts();
    }

    // ---- pushes -------------------------------------------------------------------------------------------------------
    void reserve_pending(size_t n) { pending.reserve(pending.size() + n); }
    void push(uint32_t voice, uint64_t frame, uint32_t target, float value, bool local)
    {
        pending.push_back(HostEvent{voice, frame, target, value, seq++, local});
        if (local) n_block_local += 1;
    }
    // one more try_push'ed event on endpoint `target` of `voice` (of `ne` per voice) in the block being assembled;
    // false, and the event counted as dropped: the endpoint already holds `cap`
    bool count_local(uint32_t voice, uint32_t target, size_t ne, uint32_t cap)
    {
        if (local_cnt.empty()) local_cnt.assign((size_t)V * ne, 0);
        const size_t k = (size_t)voice * ne + target;
        uint8_t& cnt = local_cnt[k];
        if (cnt >= cap) {
            dropped += 1;
            return false;
        }
        if (cnt == 0) local_touched.push_back((uint32_t)k);
        cnt += 1;
        return true;
    }
    template <class F>
    void remap_pending(F&& slot_of) // og_group_voices: the pending events move with their voices
    {
        for (HostEvent& h : pending) h.voice = slot_of(h.voice);
    }
    // og_reserve_events: room kept behind a bulk score for live segments; takes effect with the next rebuild
    void reserve(size_t n_events, bool have_ring)
    {
        ev_reserve = n_events;
        ev_rebuild = ev_rebuild || (have_ring && ev_tail + ev_reserve > ev_cap);
    }

    // a block ending at frame `lim` is about to be queued: a try_push'ed event whose frame_offset >= its length is never
    // delivered (the reference clears the queues at the end of the block)
    void drop_late_local(uint64_t lim)
    {
        const size_t from = std::min(local_from, pending.size()); // pushes since the previous block sit behind this index
        local_from = pending.size();
        if (!n_block_local) return;
        const size_t before = pending.size();
        pending.erase(std::remove_if(pending.begin() + (long)from, pending.end(),
                                     [&](const HostEvent& h) { return h.block_local && h.frame >= lim; }),
                      pending.end());
        dropped += before - pending.size();
        for (size_t i = from; i < pending.size(); ++i) pending[i].block_local = false; // (delivered: part of the timeline from here on)
        local_from = pending.size();
        n_block_local = 0;
        clear_local_counts();
    }
    // try_push'ed events of the block that is still being assembled (pushed since the last block was queued) stay
    // on the host: drop_late_local() has not judged them against that block's length yet.  A flush in between --
    // og_process_block launches earlier async blocks, the setters launch the queue -- must not turn an event whose
    // frame_offset >= frames into one that fires in a later block.  Held back while this object lives.
    struct HoldLocal {
        EventTimeline& t;
        std::vector<HostEvent> held;
        explicit HoldLocal(EventTimeline& t_) : t(t_)
        {
            if (t.n_block_local == 0) return;
            const size_t from = std::min(t.local_from, t.pending.size());
            auto mid = std::stable_partition(t.pending.begin() + (long)from, t.pending.end(), [](const HostEvent& h) { return !h.block_local; });
            held.assign(mid, t.pending.end());
            t.pending.erase(mid, t.pending.end());
        }
        ~HoldLocal()
        {
            if (held.empty()) return;
            t.local_from = std::min(t.local_from, t.pending.size());
            t.pending.insert(t.pending.end(), held.begin(), held.end());
        }
        HoldLocal(const HoldLocal&) = delete;
        HoldLocal& operator=(const HoldLocal&) = delete;
    };
    // something to bring to the device before the launch that ends at `lend`
    bool needs_upload(uint64_t lend) const { return !pending.empty() || ev_rebuild || (!cont_due.empty() && cont_due.front().first < lend); }

    // unconsumed events of voice v on the device timeline at horizon hz (a block consumes everything before its end): the
    // voice's segment, then its continuation
    void resident_unconsumed(uint32_t v, uint64_t hz, std::vector<TlEvent>& out) const
    {
        uint32_t hb, he, cb, ce;
        unconsumed_ranges(v, hz, hb, he, cb, ce); // (binary search for the horizon: no walk over what has been played)
        out.insert(out.end(), h_events.begin() + hb, h_events.begin() + he);
        out.insert(out.end(), h_events.begin() + cb, h_events.begin() + ce);
    }

    // ---- full rebuild: plan -> the engine (re)allocates and uploads the image -> adopt ----------------------------------
    struct Rebuild {
        std::vector<TlEvent> events;       // the CSR image: every voice's unconsumed events, in voice order
        std::vector<uint32_t> cursor, end; // [V]
        std::vector<uint64_t> last;
        bool realloc = false; // the ring must be (re)allocated ...
        size_t capacity = 0;  // ... with this many events; 0: refused (the score and its reserve exceed the 32-bit ring)
    };
    // the capacity a ring that must hold n events is given, or 0: n + reserve cannot be addressed
    static size_t grown_capacity(size_t n, size_t reserve, size_t headroom)
    {
        size_t cap = std::max<size_t>(n + std::max<size_t>(n / 2, reserve), 1024) + headroom;
        // ring positions (seg_begin / seg_end, the device cursor and end words) are 32-bit: the ring never grows past
        // what they address -- the slack shrinks first, and a score that does not fit with its reserve is refused
        if (cap > CAP_MAX) cap = CAP_MAX;
        return n + reserve > cap ? 0 : cap;
    }
    Rebuild plan_rebuild(uint64_t hz, bool have_ring)
    {
        std::stable_sort(pending.begin(), pending.end(), push_order);
        Rebuild r;
        r.cursor.resize(V);
        r.end.resize(V);
        r.last.assign(V, 0);
        std::vector<TlEvent>& evs = r.events;
        std::vector<TlEvent> old;
        size_t p = 0;
        const size_t np = pending.size();
        const bool had = !seg_begin.empty();
        evs.reserve(np + (had ? ev_tail : 0));
        for (uint32_t v = 0; v < V; ++v) {
            r.cursor[v] = (uint32_t)evs.size();
            size_t q = p;
            while (q < np && pending[q].voice == v) ++q;
            if (had && (seg_begin[v] != seg_end[v] || has_cont(v))) {
                old.clear();
                if (has_old_events(v, hz)) resident_unconsumed(v, hz, old); // (else no look at h_events: cold memory)
                merge_by_frame(old, pending.data() + p, pending.data() + q, evs);
            } else {
                for (size_t i = p; i < q; ++i) evs.push_back(TlEvent{pending[i].frame, pending[i].target, pending[i].value});
            }
            p = q;
            r.end[v] = (uint32_t)evs.size();
            if (r.end[v] != r.cursor[v]) r.last[v] = evs.back().frame;
        }
        const size_t n = evs.size();
        if (n > CAP_MAX) throw std::runtime_error("event timeline too long");
        r.realloc = n + std::max<size_t>(std::min<size_t>(stage_cap, 64), ev_reserve) > ev_cap || !have_ring;
        r.capacity = r.realloc ? grown_capacity(n, ev_reserve, ev_headroom) : ev_cap;
        return r;
    }
    // the image is on the device (the stream has been synchronised: the plan's vectors die here)
    void adopt(Rebuild& r)
    {
        const size_t n = r.events.size();
        ev_cap = r.capacity;
        cont_due.clear();
        h_events.swap(r.events);
        // mirror of the whole ring, reserved up front so that the live path never reallocates while playing (grown on demand:
        // no zero-fill of the room here) -- up to 2^28 events (4 GB of host memory); a ring larger than that mirrors what is
        // resident plus the promised reserve and grows on demand beyond it
        h_events.reserve(ev_cap <= ((size_t)1 << 28) ? ev_cap : std::min(ev_cap, h_events.size() + std::max<size_t>(ev_reserve, (size_t)1 << 28)));
        // ... and the first half gigabyte of that room is touched HERE, while the score is being laid out: the live path appends
        // ~150 KB of segments per block at 8 M voices, i.e. it enters a fresh 2 MB region of this mapping every dozen blocks,
        // and a first touch that has to wait for the kernel to find (compact) a huge page is a stall of milliseconds on the
        // real-time path (one 12.5 ms block in five driver-command runs of round 6, one 6.4 ms block in round 5's -- neither
        // reproduced on demand).  Half a gigabyte covers ~3 000 blocks of live playing at that size; costs ~0.1 s here.
        {
            const size_t room = (h_events.capacity() - h_events.size()) * sizeof(TlEvent);
            if (room) memset(reinterpret_cast<char*>(h_events.data()) + h_events.size() * sizeof(TlEvent), 0, std::min<size_t>(room, (size_t)512 << 20));
        }
        seg_begin.swap(r.cursor);
        seg_end.swap(r.end);
        seg_last.swap(r.last);
        n_conts = 0;
        cont_begin.assign(V, 0); // (everything is in the segments now; the arrays are sized here, not on the live path)
        cont_end.assign(V, 0);
        cont_last.assign(V, 0);
        ev_tail = n;
        ring_live.clear();
        for (uint32_t v = 0; v < V; ++v)
            if (seg_begin[v] != seg_end[v]) ring_live.push_back(RingSeg{v, seg_begin[v], seg_end[v]});
        pending.clear();
        local_from = 0;
        ev_rebuild = false;
        n_full_rebuilds += 1;
    }

    // ---- incremental update: plan (fills the staging slot) -> commit (the mirror) -> the engine launches the update kernel --
    // live pushes: O(#pushes) host work, asynchronous upload.  A batch that does not fit (staging buffer, tail of d_events)
    // goes to the full rebuild.
    struct Batch {
        enum Fit { OK, STAGING_FULL, RING_FULL } fit = OK;
        size_t n_ev = 0, n_upd = 0; // n_upd == 0 (with OK): every due entry was stale, nothing was pushed -- no kernel to launch
        size_t base = 0;            // where the staged events go in the ring
        explicit operator bool() const { return fit == OK; }
    };
    // sev / upd: the staging slot's two buffers (stage_events() events, stage_events() x EV_UPD_WORDS words)
    Batch plan_incremental(TlEvent* sev, uint32_t* upd, uint64_t hz, uint64_t lend)
    {
        Batch b;
        if (pending.size() > stage_cap) return refuse(b, Batch::STAGING_FULL);
        if (seg_begin.empty()) {
            seg_begin.assign(V, 0);
            seg_end.assign(V, 0);
            seg_last.assign(V, 0);
            ensure_cont();
        }
        // group the pending pushes per voice without sorting the batch: chain them in arrival order (O(n)), then put
        // every (short) chain into (frame, push order)
        const size_t np = pending.size();
        constexpr uint32_t NONE = 0xFFFFFFFFu;
        if (grp_head.empty()) {
            grp_head.assign(V, NONE);
            grp_tail.assign(V, NONE);
        }
        grp_next.assign(np, NONE);
        grp_voices.clear();
        for (size_t i = 0; i < np; ++i) {
            const uint32_t v = pending[i].voice;
            if (grp_head[v] == NONE) {
                grp_head[v] = (uint32_t)i;
                grp_voices.push_back(v);
            } else {
                grp_next[grp_tail[v]] = (uint32_t)i;
            }
            grp_tail[v] = (uint32_t)i;
        }
        // voices whose continuation has its first event inside the launch being prepared (and no push in this batch: a
        // pushed voice is brought up to the end of the launch anyway)
        std::vector<uint32_t> due;
        while (!cont_due.empty() && cont_due.front().first < lend) {
            const std::pair<uint64_t, uint32_t> top = cont_due.front();
            std::pop_heap(cont_due.begin(), cont_due.end(), std::greater<std::pair<uint64_t, uint32_t>>());
            cont_due.pop_back();
            const uint32_t v = top.second;
            if (!has_cont(v) || h_events[cont_begin[v]].frame != top.first) { // (stale: the voice was merged or re-pointed since)
                paths.stale_due += 1;
                continue;
            }
            if (grp_head[v] != NONE) continue;
            due.push_back(v);
        }
        std::sort(due.begin(), due.end());
        due.erase(std::unique(due.begin(), due.end()), due.end());
        std::vector<TlEvent> old, merged;
        std::vector<HostEvent> mine;
        kept.clear();
        size_t n_ev = 0, n_upd = 0;
        bool fits = true;
        for (const uint32_t v : grp_voices) {
            // the usual live case: nothing of this voice is waiting on the device and its pushes arrived in frame order
            // (a note-on is a frequency value and a gate on one frame) -- straight into the staging buffer
            if (fits && !has_old_events(v, hz)) {
                size_t k = 0;
                uint64_t last = 0;
                bool ordered = true;
                for (uint32_t i = grp_head[v]; i != NONE; i = grp_next[i], ++k) {
                    const HostEvent& h = pending[i];
                    ordered = ordered && h.frame >= last;
                    last = h.frame;
                    if (n_ev + k < stage_cap) sev[n_ev + k] = TlEvent{h.frame, h.target, h.value};
                }
                if (ordered && n_ev + k <= stage_cap) {
                    grp_head[v] = NONE;
                    // (cursor, end) relative to the batch: its place in the ring is chosen below
                    put_update(upd, n_upd, v, (uint32_t)n_ev, (uint32_t)(n_ev + k));
                    n_ev += k;
                    paths.fast += 1;
                    continue;
                }
            }
            mine.clear();
            for (uint32_t i = grp_head[v]; i != NONE; i = grp_next[i]) mine.push_back(pending[i]);
            grp_head[v] = NONE; // (left clean for the next batch, also on the early exit below)
            if (!fits) continue;
            for (size_t i = 1; i < mine.size(); ++i) { // insertion sort by frame; arrival order breaks ties
                const HostEvent k = mine[i];
                size_t j = i;
                while (j > 0 && mine[j - 1].frame > k.frame) {
                    mine[j] = mine[j - 1];
                    --j;
                }
                mine[j] = k;
            }
            if (!merge_voice(v, mine, hz, lend, sev, upd, n_ev, n_upd, old, merged)) fits = false;
        }
        for (const uint32_t v : due) { // (after the pushed voices: `due` holds none of them)
            if (!fits) { // (the batch goes to full_rebuild, which merges every continuation)
                break;
            }
            mine.clear();
            if (!merge_voice(v, mine, hz, lend, sev, upd, n_ev, n_upd, old, merged)) fits = false;
        }
        if (!fits) return refuse(b, Batch::STAGING_FULL);
        if (n_upd == 0) {
            pending.clear();
            local_from = 0;
            return b;
        }
        // a place in the ring for the whole batch (the segments touched above count as superseded only after the commit,
        // so the batch never lands on the old events it was merged from)
        b.base = ring_alloc(n_ev, hz);
        if (b.base == SIZE_MAX) return refuse(b, Batch::RING_FULL);
        b.n_ev = n_ev;
        b.n_upd = n_upd;
        return b;
    }
    // the host mirror follows the plan; the batch-relative positions in `upd` become ring positions
    void commit_incremental(const Batch& b, const TlEvent* sev, uint32_t* upd)
    {
        const size_t base = b.base, n_ev = b.n_ev;
        if (h_events.size() < base + n_ev) h_events.resize(base + n_ev); // (capacity ev_cap is reserved: no reallocation, no fill of the unused room)
        memcpy(h_events.data() + base, sev, n_ev * sizeof(TlEvent));
        size_t kq = 0; // (next entry of `kept`: they are in update order)
        for (size_t i = 0; i < b.n_upd; ++i) {
            uint32_t* u = upd + EV_UPD_WORDS * i;
            const uint32_t v = u[0];
            Kept k{(uint32_t)i, 0u, 0u, false};
            if (kq < kept.size() && kept[kq].upd == (uint32_t)i) k = kept[kq++];
            if (k.in_place) { // pointed at records that are in the ring already (the segment they lie in stays alive: ring_alloc)
                seg_begin[v] = u[1];
                seg_end[v] = u[2];
                seg_last[v] = h_events[u[2] - 1].frame;
                if (n_conts) set_cont(v, 0u, 0u);
                continue;
            }
            seg_last[v] = sev[u[2] - 1].frame;
            u[1] += (uint32_t)base;
            u[2] += (uint32_t)base;
            seg_begin[v] = u[1];
            seg_end[v] = u[2];
            if (k.begin != k.end) {
                ensure_cont();
                set_cont(v, k.begin, k.end);
                cont_due_push(v);
            } else if (n_conts) {
                set_cont(v, 0u, 0u);
            }
            ring_live.push_back(RingSeg{v, u[1], u[2]});
        }
        n_events_copied += n_ev;
        ev_tail = base + n_ev;
        pending.clear();
        local_from = 0;
        n_incremental += 1;
    }

private:
    uint32_t V;
    size_t stage_cap, ev_headroom;
    std::vector<HostEvent> pending;      // pushes not yet on the device timeline (PHYSICAL voice slots)
    std::vector<TlEvent> h_events;       // host mirror of d_events (the whole ring)
    std::vector<uint32_t> seg_begin, seg_end; // per voice: its current segment (empty vectors = all segments empty)
    std::vector<uint64_t> seg_last;           // per voice: frame of the segment's last event (< frame_now: all consumed)
    // Continuation (round 6): on the HOST a voice's timeline is its segment [seg_begin, seg_end) followed by
    // [cont_begin, cont_end) -- the tail of an EARLIER segment left where it lies in the ring.  A live push onto a voice with
    // a long score ahead of it writes a new segment {what is due up to the end of the launch being prepared, merged with the
    // pushes} and remembers the rest as the continuation; every frame in the segment is < every frame in the continuation.
    // The device knows nothing of this (one segment per voice, as ever -- a first form that taught the kernels to hop cost
    // the four-wave kernel 4 % and the ordinary one 30 spills): before the launch in which a continuation's first event is
    // due the host points the voice at it -- a 12-byte cursor update when the segment in front has been played, which is
    // the usual case (plan_incremental / merge_voice).  Cost of a message: its own records, whatever the score's length.
    // Vectors are empty until a continuation exists; `cont_due` orders the voices by their continuation's first frame.
    std::vector<uint32_t> cont_begin, cont_end;
    std::vector<uint64_t> cont_last;
    std::vector<std::pair<uint64_t, uint32_t>> cont_due; // min-heap of {first frame of the continuation, voice}; stale entries are skipped
    size_t n_conts = 0; // voices that have a continuation right now (0: nobody looks at the cont_* arrays -- cold memory)
    std::vector<uint32_t> grp_head, grp_tail, grp_next, grp_voices; // incremental path: pending events chained per voice
    std::vector<uint8_t> local_cnt;      // [voice * n_event_inputs + event input]: try_push'ed events queued for the next block
    std::vector<uint32_t> local_touched; // entries of local_cnt to clear when the block starts
    size_t ev_cap = 0;
    bool ev_rebuild = false; // next block must rebuild the whole timeline
    size_t ev_reserve = 0;
    size_t ev_tail = 0;       // next free slot of d_events
    size_t n_block_local = 0; // events pushed with try_push semantics for the next block
    size_t local_from = 0;    // index in `pending` of the first push since the previous block was queued
    uint64_t seq = 0;
    // d_events is a RING for the live path: segments are appended at ev_tail; a segment is dead once its voice has been
    // given a newer one or its last event lies before the consumed horizon, and the space of the dead segments at the
    // front is reused when the tail reaches the end of the buffer -- a steady stream of live pushes (MIDI playing)
    // never triggers the O(V) rebuild + stream synchronise that a bump pointer needs for compaction (measured: a
    // 7 ms stall every ~1 400 blocks at 1 M voices, a missed audio deadline).  Only a segment that stays alive at the
    // front for a whole lap (an event scheduled far ahead) still forces a rebuild.
    struct RingSeg {
        uint32_t voice, begin, end;
    };
    std::deque<RingSeg> ring_live; // live segments in append order (oldest first)
    // the updates of a batch that are not plain "new segment, no continuation" (few), in update order: the continuation the
    // voice keeps; in_place: the update's positions are absolute ring positions (the voice is pointed at records in place)
    struct Kept {
        uint32_t upd, begin, end;
        bool in_place;
    };
    std::vector<Kept> kept;

    static Batch& refuse(Batch& b, Batch::Fit why)
    {
        b.fit = why;
        return b;
    }
    static void put_update(uint32_t* upd, size_t& n_upd, uint32_t v, uint32_t cursor, uint32_t end)
    {
        upd[EV_UPD_WORDS * n_upd] = v;
        upd[EV_UPD_WORDS * n_upd + 1] = cursor;
        upd[EV_UPD_WORDS * n_upd + 2] = end;
        n_upd += 1;
    }
    void clear_local_counts()
    {
        for (uint32_t k : local_touched) local_cnt[k] = 0;
        local_touched.clear();
    }
    void cont_due_push(uint32_t v)
    {
        cont_due.emplace_back(h_events[cont_begin[v]].frame, v);
        std::push_heap(cont_due.begin(), cont_due.end(), std::greater<std::pair<uint64_t, uint32_t>>());
    }
    bool has_cont(uint32_t v) const { return n_conts != 0 && cont_begin[v] != cont_end[v]; }
    void set_cont(uint32_t v, uint32_t b, uint32_t e)
    {
        const bool had = cont_begin[v] != cont_end[v];
        cont_begin[v] = b;
        cont_end[v] = e;
        if (b != e) cont_last[v] = h_events[e - 1].frame;
        n_conts += (b != e ? 1 : 0);
        n_conts -= (had ? 1 : 0);
    }
    void ensure_cont() // (sized with the segment arrays, outside the real-time path: 16 bytes per voice of zero-fill)
    {
        if (cont_begin.empty()) {
            cont_begin.assign(V, 0);
            cont_end.assign(V, 0);
            cont_last.assign(V, 0);
        }
    }
    // events of one segment are sorted by frame: first index in [b, e) whose frame is >= fr / > fr
    uint32_t lower_frame(uint32_t b, uint32_t e, uint64_t fr) const
    {
        while (b < e) {
            const uint32_t m = b + (e - b) / 2;
            if (h_events[m].frame < fr) b = m + 1;
            else e = m;
        }
        return b;
    }
    uint32_t upper_frame(uint32_t b, uint32_t e, uint64_t fr) const
    {
        while (b < e) {
            const uint32_t m = b + (e - b) / 2;
            if (h_events[m].frame <= fr) b = m + 1;
            else e = m;
        }
        return b;
    }
    // the unconsumed part of the voice's segment / of its continuation, as index ranges of h_events
    void unconsumed_ranges(uint32_t v, uint64_t hz, uint32_t& hb, uint32_t& he, uint32_t& cb, uint32_t& ce) const
    {
        hb = he = cb = ce = 0;
        if (seg_begin.empty()) return;
        if (seg_begin[v] != seg_end[v] && seg_last[v] >= hz) {
            hb = lower_frame(seg_begin[v], seg_end[v], hz);
            he = seg_end[v];
        }
        if (has_cont(v) && cont_last[v] >= hz) {
            cb = lower_frame(cont_begin[v], cont_end[v], hz);
            ce = cont_end[v];
        }
    }
    bool has_old_events(uint32_t v, uint64_t hz) const
    {
        if (seg_begin.empty()) return false;
        return (seg_begin[v] != seg_end[v] && seg_last[v] >= hz) || (has_cont(v) && cont_last[v] >= hz);
    }
    // where `n` events can be appended, or SIZE_MAX when the ring is full
    size_t ring_alloc(size_t n, uint64_t hz)
    {
        size_t at = ring_alloc_bounded(n, 4096, hz);
        if (at == SIZE_MAX) at = ring_alloc_bounded(n, SIZE_MAX, hz); // (no room behind a bounded sweep: finish it, then decide)
        return at;
    }
    // `sweep` bounds how many dead segments one call retires.  When a long resident score runs out, the segments of ALL
    // voices die within a few blocks: retiring millions of them in one call was a 10-15 ms stall on the real-time path
    // (round 4, the loaded bank: one block near the end of every run at 4-8 M voices); the room they occupy is not needed
    // at once, so the sweep is spread over the following calls.
    size_t ring_alloc_bounded(size_t n, size_t sweep, uint64_t hz)
    {
        while (!ring_live.empty() && sweep-- > 0) {
            const RingSeg& f = ring_live.front();
            // alive: the voice's current segment, or the segment its continuation lies in, with something left to play
            // (a voice that was pointed at its continuation plays a sub-range of the older segment the continuation lay in)
            // (seg_begin first: a superseded segment -- the usual one at the front -- is settled by that one cold word, as ever)
            const uint32_t sb = seg_begin[f.voice];
            const bool is_head = sb >= f.begin && sb < f.end && seg_end[f.voice] <= f.end && sb != seg_end[f.voice] && seg_last[f.voice] >= hz;
            const bool holds_cont = has_cont(f.voice) && cont_begin[f.voice] >= f.begin && cont_end[f.voice] <= f.end && cont_last[f.voice] >= hz;
            const bool dead = !is_head && !holds_cont;
            if (!dead) break;
            ring_live.pop_front();
        }
        if (ring_live.empty()) {
            ev_tail = 0;
            return n <= ev_cap ? 0 : SIZE_MAX;
        }
        const size_t head = ring_live.front().begin;
        if (ev_tail >= head) { // live data is [head, tail): room behind the tail, or -- wrapping -- in front of the head
            if (ev_tail + n <= ev_cap) return ev_tail;
            if (n < head) {
                n_ring_wraps += 1;
                return 0;
            }
            return SIZE_MAX;
        }
        return ev_tail + n < head ? ev_tail : SIZE_MAX; // wrapped: the tail runs up to the head
    }

    static bool push_order(const HostEvent& a, const HostEvent& b)
    {
        if (a.voice != b.voice) return a.voice < b.voice;
        if (a.frame != b.frame) return a.frame < b.frame;
        return a.seq < b.seq;
    }
    // old (already on the device) before new on equal frames: the old ones were pushed earlier
    static void merge_by_frame(const std::vector<TlEvent>& old, const HostEvent* nb, const HostEvent* ne, std::vector<TlEvent>& out)
    {
        size_t i = 0;
        while (i < old.size() || nb != ne) {
            if (nb == ne || (i < old.size() && old[i].frame <= nb->frame)) {
                out.push_back(old[i++]);
            } else {
                out.push_back(TlEvent{nb->frame, nb->target, nb->value});
                ++nb;
            }
        }
    }
    // `merged` goes behind the batch's events, the voice is pointed at it (relative to the batch: its place in the ring is
    // chosen at the commit); false: the staging buffer is full
    bool stage_segment(uint32_t v, const std::vector<TlEvent>& merged, TlEvent* sev, uint32_t* upd, size_t& n_ev, size_t& n_upd) const
    {
        if (n_ev + merged.size() > stage_cap || n_upd >= stage_cap) return false;
        memcpy(sev + n_ev, merged.data(), merged.size() * sizeof(TlEvent));
        put_update(upd, n_upd, v, (uint32_t)n_ev, (uint32_t)(n_ev + merged.size()));
        n_ev += merged.size();
        return true;
    }
    // the voice is pointed at [b, e), records that lie in the ring already (absolute ring positions)
    bool point_in_place(uint32_t v, uint32_t b, uint32_t e, uint32_t* upd, size_t& n_upd)
    {
        if (n_upd >= stage_cap) return false;
        kept.push_back(Kept{(uint32_t)n_upd, 0u, 0u, true});
        put_update(upd, n_upd, v, b, e);
        paths.in_place += 1;
        return true;
    }
    // One voice of an incremental batch: its pushes `mine` (sorted; may be empty: a voice whose continuation falls due) merged
    // with what it still has to play UP TO `bound` = the later of the last pushed frame and the end of the launch being
    // prepared; what lies behind stays where it is and becomes (or remains) the continuation -- the rest of a long score is
    // never copied.  A short rest is carried over instead.  A voice without pushes whose segment has been played is simply
    // pointed at its continuation: no record is written at all.  false: the batch does not fit the staging buffer.
    bool merge_voice(uint32_t v, const std::vector<HostEvent>& mine, uint64_t hz, uint64_t lend, TlEvent* sev, uint32_t* upd, size_t& n_ev,
                     size_t& n_upd, std::vector<TlEvent>& old, std::vector<TlEvent>& merged)
    {
        old.clear();
        merged.clear();
        uint32_t keep_b = 0, keep_e = 0;
        if (!mine.empty() && !has_cont(v) && seg_end[v] - seg_begin[v] < CONT_MIN) {
            // the usual loaded voice: a handful of waiting events, no continuation, nothing worth leaving behind -- one pass
            // over the segment, as before round 6 (the real-time banks: ~1000 of these per block)
            if (seg_last[v] >= hz)
                for (uint32_t i = seg_begin[v]; i < seg_end[v]; ++i)
                    if (h_events[i].frame >= hz) old.push_back(h_events[i]);
            merge_by_frame(old, mine.data(), mine.data() + mine.size(), merged);
            paths.short_merge += 1;
            return stage_segment(v, merged, sev, upd, n_ev, n_upd);
        }
        const uint64_t bound = std::max<uint64_t>(mine.empty() ? 0 : mine.back().frame, lend ? lend - 1 : 0);
        uint32_t hb, he, cb, ce;
        unconsumed_ranges(v, hz, hb, he, cb, ce);
        if (mine.empty()) {
            if (cb == ce) return true; // (nothing left behind after all)
            // the segment in front has been played: the continuation IS the voice's segment from here on
            if (hb == he) return point_in_place(v, cb, ce, upd, n_upd);
        }
        if (cb != ce) { // (every frame of the segment is <= every frame of the continuation)
            const uint32_t split = upper_frame(cb, ce, bound);
            old.insert(old.end(), h_events.begin() + hb, h_events.begin() + he);
            old.insert(old.end(), h_events.begin() + cb, h_events.begin() + split);
            if (ce - split >= CONT_MIN) {
                keep_b = split;
                keep_e = ce;
            } else {
                old.insert(old.end(), h_events.begin() + split, h_events.begin() + ce);
            }
        } else {
            const uint32_t split = upper_frame(hb, he, bound);
            if (he - split >= CONT_MIN) {
                old.insert(old.end(), h_events.begin() + hb, h_events.begin() + split);
                keep_b = split;
                keep_e = he;
            } else {
                old.insert(old.end(), h_events.begin() + hb, h_events.begin() + he);
            }
        }
        merge_by_frame(old, mine.data(), mine.data() + mine.size(), merged);
        if (merged.empty()) { // (only a rest behind the launch: point the voice at it, as above)
            if (keep_b == keep_e) return true;
            return point_in_place(v, keep_b, keep_e, upd, n_upd);
        }
        const size_t at = n_upd;
        if (!stage_segment(v, merged, sev, upd, n_ev, n_upd)) return false;
        if (keep_b != keep_e) {
            kept.push_back(Kept{(uint32_t)at, keep_b, keep_e, false});
            paths.cont_left += 1;
        }
        return true;
    }
};
