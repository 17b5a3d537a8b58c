// tests/standalone/timeline_model_main.cpp -- TEST INFRASTRUCTURE, never part of the product and never linked into the library.
//
// A stand-alone program that holds EventTimeline (csrc/og_timeline.h: where every pushed event lands in the device ring) against
// a naive model, on the CPU and without HIP.  Beside the timeline it keeps
//   - the model: per voice every event pushed and not yet delivered, ordered by (frame, push number);
//   - a fake device: an event array of the ring's capacity and cursor[V] / end[V], written exactly as the engine writes the real
//     ones -- the three uploads of a full rebuild; for an incremental batch the staged events copied to `base`, then the
//     update triples applied (og_apply_event_updates) -- and read as a launch reads them (a voice consumes what lies before the
//     launch's end);
//   - the engine's side of the bargain (og_engine.cpp: upload_events, full_rebuild, incremental_update, process_async): the block
//     queue that gives the consumed horizon and the launch end, the hold-back of block-local pushes, the bulk / incremental
//     decision with its thresholds.
// Random steps from a fixed seed: bulk scores with long per-voice runs, live pushes in and out of frame order and on equal
// frames, block-local pushes on both sides of the next block's length, blocks queued but not launched, launches, reserve, reset.
// After every launch, for every voice: what the launch delivered is the model's events before the launch end, in order; what
// the timeline calls unconsumed at the new horizon is the model's rest, in order; the device segment is the front of that;
// cursor <= end <= capacity.  A run that never took one of the paths listed in `need` below fails: tune the generator.
//
//   timeline_model_main [seed ...]      (default: four seeds)
//
//   g++ -std=c++17 -O1 -Ioscen_amd/csrc tests/standalone/timeline_model_main.cpp -o timeline_model_main
// and, under sanitizers (it has its own main, so it needs nothing preloaded), the same with
//   clang++ -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "og_timeline.h"

namespace {

constexpr uint32_t V = 37;         // voices
constexpr size_t STAGE = 96;       // events one staging buffer holds
constexpr size_t HEADROOM = 64;    // the ring wraps every few hundred steps
constexpr uint32_t NE = 2;         // event inputs per voice
constexpr uint32_t LOCAL_CAP = 32; // try_push capacity per endpoint per block
constexpr uint32_t BATCH = 3;      // blocks per launch at the most
constexpr uint32_t QUIET0 = 31;    // voices from here on are pushed rarely: an event far ahead stays at the ring's front for a lap

struct MEv {
    uint64_t frame;
    uint32_t target, id;
};

struct Sim {
    uint64_t seed;
    size_t step = 0;
    std::mt19937_64 rng;
    EventTimeline tl{V, STAGE, HEADROOM};
    std::vector<std::vector<MEv>> live{V};                // the model
    std::vector<std::pair<uint32_t, uint32_t>> unjudged; // {voice, id}: block-local pushes since the last block was queued
    uint32_t next_id = 1;
    // the engine's block queue
    uint64_t frame_now = 0, q_frame0 = 0;
    uint32_t q_frames = 0, q_blocks = 0;
    // the fake device
    bool have_ring = false;
    std::vector<TlEvent> dev;
    std::vector<uint32_t> cur = std::vector<uint32_t>(V, 0), end = std::vector<uint32_t>(V, 0);
    std::vector<TlEvent> sev = std::vector<TlEvent>(STAGE);
    std::vector<uint32_t> upd = std::vector<uint32_t>(STAGE * EV_UPD_WORDS);
    uint64_t n_staging_full = 0, n_ring_full = 0, n_launches = 0, n_delivered = 0, n_resets = 0, n_horizon_behind = 0;
    uint64_t n_late_dropped = 0, n_over_cap = 0; // pushes the MODEL removed in queue_block / never made

    explicit Sim(uint64_t s) : seed(s), rng(s) {}

    [[noreturn]] void fail(const char* what, uint32_t v)
    {
        printf("FAIL seed %" PRIu64 " step %zu voice %u: %s\n", seed, step, v, what);
        exit(1);
    }
    uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }
    uint64_t horizon() const { return q_blocks ? q_frame0 : frame_now; }
    uint64_t launch_end() const { return q_blocks ? q_frame0 + q_frames : frame_now; }

    void push(uint32_t v, uint64_t frame, bool local)
    {
        frame = std::max(frame, frame_now);
        const uint32_t target = rnd(NE);
        if (local && !tl.count_local(v, target, NE, LOCAL_CAP)) { // (over the cap: counted as dropped, never pushed)
            n_over_cap += 1;
            return;
        }
        const uint32_t id = next_id++;
        if (id >= (1u << 24)) fail("push numbers no longer fit a float", v);
        tl.push(v, frame, target, (float)id, local);
        auto& l = live[v];
        size_t at = l.size();
        while (at > 0 && l[at - 1].frame > frame) --at; // behind every earlier push on the same frame
        l.insert(l.begin() + (long)at, MEv{frame, target, id});
        if (local) unjudged.emplace_back(v, id);
    }

    // ---- og_engine.cpp's side ---------------------------------------------------------------------------------------
    void full_rebuild()
    {
        EventTimeline::Rebuild r = tl.plan_rebuild(horizon(), have_ring);
        if (r.realloc) {
            if (!r.capacity) fail("rebuild refused", 0);
            dev.assign(r.capacity, TlEvent{~0ull, ~0u, -1.0f});
            have_ring = true;
        }
        if (r.events.size() > dev.size()) fail("rebuild image larger than the ring", 0);
        std::copy(r.events.begin(), r.events.end(), dev.begin());
        cur = r.cursor;
        end = r.end;
        tl.adopt(r);
        if (tl.capacity() != dev.size()) fail("capacity differs from the ring's", 0);
    }
    bool incremental_update()
    {
        const EventTimeline::Batch b = tl.plan_incremental(sev.data(), upd.data(), horizon(), launch_end());
        if (!b) {
            (b.fit == EventTimeline::Batch::RING_FULL ? n_ring_full : n_staging_full) += 1;
            return false;
        }
        if (b.n_upd == 0) return true;
        if (b.n_ev > STAGE || b.n_upd > STAGE) fail("batch larger than the staging buffer", 0);
        tl.commit_incremental(b, sev.data(), upd.data());
        if (b.base + b.n_ev > dev.size()) fail("batch beyond the ring", 0);
        for (size_t i = 0; i < b.n_ev; ++i) dev[b.base + i] = sev[i]; // og_apply_event_updates
        for (size_t i = 0; i < b.n_upd; ++i) {
            const uint32_t v = upd[EV_UPD_WORDS * i];
            if (v >= V) fail("update of a voice that does not exist", v);
            cur[v] = upd[EV_UPD_WORDS * i + 1];
            end[v] = upd[EV_UPD_WORDS * i + 2];
        }
        return true;
    }
    void upload_events()
    {
        if (!tl.needs_upload(launch_end())) return;
        EventTimeline::HoldLocal hold(tl);
        if (!tl.needs_upload(launch_end())) return;
        const bool bulk = tl.wants_rebuild() || tl.n_pending() > tl.stage_events() || tl.n_pending() > (size_t)V / 2 + 64 || !have_ring;
        if (bulk || !incremental_update()) full_rebuild();
    }
    bool is_unjudged(uint32_t v, uint32_t id) const
    {
        for (const auto& u : unjudged)
            if (u.first == v && u.second == id) return true;
        return false;
    }
    void launch()
    {
        if (!q_blocks) return;
        upload_events();
        const uint64_t lend = launch_end();
        n_launches += 1;
        std::vector<TlEvent> rest;
        for (uint32_t v = 0; v < V; ++v) {
            if (!(cur[v] <= end[v] && end[v] <= dev.size())) fail("cursor <= end <= capacity", v);
            auto& l = live[v];
            size_t k = 0; // the launch consumes what lies before its end
            for (; cur[v] < end[v] && dev[cur[v]].frame < lend; ++cur[v], ++k) {
                const TlEvent& d = dev[cur[v]];
                if (k >= l.size() || l[k].frame != d.frame || l[k].target != d.target || (float)l[k].id != d.value) fail("delivered event is not the model's next", v);
            }
            if (k < l.size() && l[k].frame < lend) fail("an event due in this launch was not delivered", v);
            l.erase(l.begin(), l.begin() + (long)k);
            n_delivered += k;
            // the rest: the timeline's own account at the new horizon, and the device segment in front of it
            rest.clear();
            tl.resident_unconsumed(v, lend, rest);
            size_t m = 0;
            for (const MEv& e : l) {
                if (is_unjudged(v, e.id)) continue; // (held back on the host)
                if (m >= rest.size() || rest[m].frame != e.frame || rest[m].target != e.target || rest[m].value != (float)e.id) fail("unconsumed events differ from the model's", v);
                ++m;
            }
            if (m != rest.size()) fail("the timeline holds events the model does not", v);
            if (end[v] - cur[v] > rest.size()) fail("device segment longer than what is unconsumed", v);
            for (uint32_t i = cur[v]; i < end[v]; ++i) {
                const TlEvent& a = dev[i];
                const TlEvent& b = rest[i - cur[v]];
                if (a.frame != b.frame || a.target != b.target || a.value != b.value) fail("device segment is not the front of the unconsumed events", v);
            }
        }
        q_blocks = 0;
        q_frames = 0;
    }
    void queue_block(uint32_t frames)
    {
        const uint64_t lim = frame_now + frames;
        tl.drop_late_local(lim);
        for (const auto& u : unjudged) { // the model's drop_late_local
            auto& l = live[u.first];
            for (size_t i = 0; i < l.size(); ++i)
                if (l[i].id == u.second) {
                    if (l[i].frame >= lim) {
                        l.erase(l.begin() + (long)i);
                        n_late_dropped += 1;
                    }
                    break;
                }
        }
        unjudged.clear();
        if (q_blocks && tl.n_pending() > std::min<size_t>(tl.stage_events() / 2, (size_t)V / 4 + 32)) launch();
        if (!q_blocks) q_frame0 = frame_now;
        q_blocks += 1;
        q_frames += frames;
        frame_now += frames;
        if (q_blocks > 1) n_horizon_behind += 1;
        if (q_blocks >= BATCH) launch();
    }
    void reset()
    {
        launch();
        tl.reset();
        for (auto& l : live) l.clear();
        unjudged.clear();
        std::fill(cur.begin(), cur.end(), 0u);
        std::fill(end.begin(), end.end(), 0u);
        frame_now = 0;
        n_resets += 1;
    }

    // ---- the generator ----------------------------------------------------------------------------------------------
    uint32_t busy_voice() { return rnd(100) < 3 ? QUIET0 + rnd(V - QUIET0) : rnd(QUIET0); }
    void one_step()
    {
        const uint32_t op = rnd(1000);
        if (op < 2) { // a score: long runs on a few voices, scheduled in bulk
            const uint32_t nv = 1 + rnd(3);
            for (uint32_t i = 0; i < nv; ++i) {
                const uint32_t v = rnd(QUIET0), n = 70 + rnd(120);
                const uint32_t gap = rnd(2) ? 40 : 1000; // (a sparse score's continuation waits long enough to be pushed onto again)
                uint64_t f = frame_now + rnd(3000);
                for (uint32_t k = 0; k < n; ++k, f += rnd(8) ? 1 + rnd(gap) : 0) push(v, f, false);
            }
        } else if (op < 4) { // a handful of waiting events on several voices: what a later batch has to carry over
            const uint32_t nv = 2 + rnd(4);
            for (uint32_t i = 0; i < nv; ++i) {
                const uint32_t v = rnd(QUIET0), n = 8 + rnd(12);
                uint64_t f = frame_now + 4000 + rnd(20000);
                for (uint32_t k = 0; k < n; ++k, f += rnd(50)) push(v, f, false);
            }
        } else if (op < 330) { // a note-on: two pushes on one frame, in order
            const uint32_t nv = rnd(4) ? 1 : 2 + rnd(5); // (now and then a chord)
            const uint64_t f = frame_now + rnd(256);
            for (uint32_t i = 0; i < nv; ++i) {
                const uint32_t v = busy_voice();
                push(v, f, false);
                push(v, f, false);
                if (rnd(2)) push(v, f + 1 + rnd(500), false); // ... and its note-off
            }
        } else if (op < 480) { // pushes out of frame order, some far enough ahead to move a continuation's front
            const uint32_t v = busy_voice(), n = 1 + rnd(5);
            for (uint32_t k = 0; k < n; ++k) push(v, frame_now + (rnd(3) ? rnd(600) : rnd(4000)), false);
        } else if (op < 486) { // one event far ahead on a quiet voice
            push(QUIET0 + rnd(V - QUIET0), frame_now + 200000 + rnd(1000000), false);
        } else if (op < 600) { // block-local pushes, offsets on both sides of the next block's length
            const uint32_t n = 1 + rnd(4);
            for (uint32_t k = 0; k < n; ++k) push(busy_voice(), frame_now + rnd(320), true);
        } else if (op < 930) {
            queue_block(rnd(4) ? 128 : 1 + rnd(512));
        } else if (op < 996) {
            launch();
        } else if (op < 999) {
            tl.reserve(rnd(400), have_ring);
        } else if (rnd(3) == 0) {
            reset();
        }
    }
};

int run(uint64_t seed, size_t steps)
{
    Sim s(seed);
    for (s.step = 0; s.step < steps; ++s.step) s.one_step();
    s.launch();
    const EventTimeline& t = s.tl;
    const struct {
        const char* name;
        uint64_t n;
    } need[] = {
        {"fast_path", t.paths.fast},
        {"short_segment_merge", t.paths.short_merge},
        {"merge_left_continuation", t.paths.cont_left},
        {"pointed_at_continuation_in_place", t.paths.in_place},
        {"stale_cont_due_skipped", t.paths.stale_due},
        {"ring_wrap", t.n_ring_wraps},
        {"refused_staging_full", s.n_staging_full},
        {"refused_ring_full", s.n_ring_full},
        {"late_local_dropped", s.n_late_dropped},
    };
    printf("seed %" PRIu64 ": steps %zu launches %" PRIu64 " delivered %" PRIu64 " full_rebuilds %" PRIu64 " incremental %" PRIu64
           " copied %" PRIu64 " resets %" PRIu64 " horizon_behind %" PRIu64 " capacity %zu\n",
           seed, steps, s.n_launches, s.n_delivered, t.n_full_rebuilds, t.n_incremental, t.n_events_copied, s.n_resets, s.n_horizon_behind, t.capacity());
    if (t.dropped != s.n_late_dropped + s.n_over_cap) s.fail("the timeline's drop count differs from the model's", 0);
    int missed = 0;
    for (const auto& p : need) {
        printf("path seed %" PRIu64 " %s %" PRIu64 "\n", seed, p.name, p.n);
        missed += p.n == 0;
    }
    if (s.n_horizon_behind == 0) missed += 1;
    if (missed) printf("FAIL seed %" PRIu64 ": %d path(s) never taken\n", seed, missed);
    return missed;
}

} // namespace

int main(int argc, char** argv)
{
    std::vector<uint64_t> seeds;
    for (int i = 1; i < argc; ++i) seeds.push_back(strtoull(argv[i], nullptr, 10));
    if (seeds.empty()) seeds = {1, 2, 3, 4};
    int bad = 0;
    for (uint64_t s : seeds) bad += run(s, 8000);
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
