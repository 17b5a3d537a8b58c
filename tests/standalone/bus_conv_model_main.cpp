// tests/standalone/bus_conv_model_main.cpp -- TEST INFRASTRUCTURE, never part of the product and never linked into the library.
//
// A stand-alone program that holds BusConvolver (csrc/og_bus_conv_host.h: which response of the post-mix Convolver runs over
// which frames, from which "history valid from" frame, where in the history buffer) against two naive models, on the CPU and
// without HIP.  Beside the class it keeps
//   - the model: Convolver::process with its swap and fade rules (oscen-lib/src/convolution/mod.rs:535-573), frame by frame,
//     a published response picked up at the first frame of the next block.  For every queued frame it records the current
//     response and the frame its history is valid from, the outgoing response with its own while the fade lasts, and the
//     position in the fade;
//   - a shadow of the history buffer: one absolute frame number per slot (-1: a zero), updated by exactly the copies, moves
//     and appends the class's plans prescribe, as the engine (og_engine.cpp: conv_alloc, conv_place_dry, conv_reset;
//     og_snapshot.cpp) carries them out on the device;
//   - the engine's side of the bargain: the block queue with its limits in blocks and in frames, the launch in front of a
//     re-size, og_init, a snapshot saved and loaded back.
// Random steps from a fixed seed: blocks of 1 to 512 frames, queue limits from 1 to 256 blocks, launches forced early,
// responses published at random times -- twice before a block picks one up, during a fade, empty, of 1, 2, S-1, S, S+1,
// 2S+3, a few thousand taps, exactly as long as the history allows and longer than it was sized for (while an outgoing
// response fades) --, the launch capacity changed in mid-stream, resets, restores, a new engine.
// After every planned launch:
//   1. the runs partition the launch's frames in order, every block lies in one run and a run has one configuration;
//   2. per run, current and outgoing response, their frame counts and the fade position are the model's;
//   3. for every frame f of a run and every tap k, the sample f - k of a response is readable (>= lo) and found in the shadow
//      slot it is read from if it is at or after the response's "valid from" frame, and not readable otherwise.  (Checked in
//      closed form over the whole run -- the entitled samples of a run are one interval, the shadow is walked once -- and
//      literally for a random handful of (f, k).)
//   4. bounds: hist_pos >= keep, hist_pos + frames <= len, no read below slot 0, nf <= row_stride, the rows of either response
//      within its half of the row buffer, every copy and move inside its buffers.
// A run that never took one of the branches listed in `need` below fails: tune the generator.
// Not covered: frame numbers beyond 2^31 (the clamps of `lo`); og_init restarts the count at 0.
//
//   bus_conv_model_main [seed ...]      (default: four seeds)
//
//   g++ -std=c++17 -O1 -Ioscen_amd/csrc tests/standalone/bus_conv_model_main.cpp -o bus_conv_model_main
// and, under sanitizers (it has its own main, so it needs nothing preloaded),
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ioscen_amd/csrc
//       tests/standalone/bus_conv_model_main.cpp -o bus_conv_model_main
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "og_bus_conv_host.h"

namespace {

constexpr uint32_t S = OG_CONV_S;
// og_kernel_rt.hip.h / og_engine.h, device headers this program cannot include
constexpr uint32_t MAX_BLOCK = 512, MAX_LAUNCH_BLOCKS = 32, MAX_QUEUE_BLOCKS = 256;
constexpr uint32_t FADE = 960; // 20 ms at 48 kHz
constexpr uint32_t CH = 2;
constexpr size_t STEPS = 4000;
constexpr size_t KEEP_MAX = 6 * 1024; // a new engine once the history has grown to this

size_t launch_frames_cap(uint32_t blocks) // og_engine::launch_frames_cap without its bound by workgroups
{
    if (blocks <= MAX_LAUNCH_BLOCKS) return (size_t)MAX_BLOCK * blocks;
    return std::max<size_t>((size_t)MAX_BLOCK * MAX_LAUNCH_BLOCKS, (size_t)256 * blocks);
}

struct MFrame { // what the model says of one queued frame
    int cur, old; // response ids; old == -1: no fade
    uint64_t cur_from, old_from;
    uint32_t pos;
};

struct QB {
    uint32_t frames, conv;
};

struct Sim {
    uint64_t seed;
    size_t step = 0;
    std::mt19937_64 rng;
    BusConvolver bc;
    BusConvolver::Paths total; // of the engines before this one
    std::vector<std::shared_ptr<ConvIR>> irs; // by id
    // the model
    int m_cur = 0, m_old = -1, m_pending = -1;
    uint64_t m_cur_from = 0, m_old_from = 0;
    uint32_t m_pos = 0;
    std::vector<MFrame> qrec;
    // the engine's block queue
    std::vector<QB> queue;
    uint64_t frame_now = 0, q_frame0 = 0;
    uint32_t q_frames = 0, batch = 1;
    size_t cap_frames = MAX_BLOCK;
    // the shadow of d_hist
    std::vector<int64_t> hist;
    uint64_t n_launches = 0, n_runs = 0, n_frames = 0, n_tight = 0, n_grow_in_fade = 0, n_resets = 0, n_restores = 0, n_engines = 1;

    explicit Sim(uint64_t s) : seed(s), rng(s) {}

    [[noreturn]] void fail(const char* what, int64_t a = 0, int64_t b = 0)
    {
        printf("FAIL seed %" PRIu64 " step %zu: %s (%" PRId64 ", %" PRId64 ")\n", seed, step, what, a, b);
        exit(1);
    }
    void want(bool ok, const char* what, int64_t a = 0, int64_t b = 0)
    {
        if (!ok) fail(what, a, b);
    }
    uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); }

    int make_ir(uint32_t k)
    {
        auto ir = std::make_shared<ConvIR>();
        ir->planes = (k && rnd(0, 3) == 0) ? CH : 1u;
        ir->taps.assign((size_t)k * ir->planes, 0.5f);
        const int id = (int)irs.size();
        if (k) ir->d = reinterpret_cast<float*>((uintptr_t)(id + 1) << 24); // never dereferenced
        irs.push_back(ir);
        return id;
    }

    // ---- the engine's side ------------------------------------------------------------------------------------------------
    void resize(size_t k) // og_engine::conv_alloc
    {
        want(queue.empty(), "re-size with blocks queued");
        const BusConvolver::Sizing sz = bc.size_for(k, cap_frames, CH);
        if (sz.new_hist) {
            std::vector<int64_t> n(sz.len, -1);
            if (!hist.empty()) {
                want(sz.copy_from + sz.copy_frames <= hist.size() && sz.copy_to + sz.copy_frames <= n.size(), "history copy out of bounds");
                std::copy(hist.begin() + sz.copy_from, hist.begin() + sz.copy_from + sz.copy_frames, n.begin() + sz.copy_to);
            }
            hist.swap(n);
        }
        bc.resized(sz);
        want(bc.hist_len() == hist.size() && bc.hist_pos() >= bc.hist_keep() && bc.hist_pos() <= bc.hist_len() && (!sz.new_hist || bc.hist_pos() + cap_frames <= bc.hist_len()),
             "sizes after a re-size");
    }
    void create() // og_create: the graph's response, buffers for one block per launch
    {
        bc = BusConvolver();
        hist.clear();
        batch = 1;
        cap_frames = launch_frames_cap(1);
        static const uint32_t first[] = {0, 1, 300};
        m_cur = make_ir(first[rnd(0, 2)]);
        m_old = m_pending = -1;
        m_cur_from = m_old_from = 0;
        m_pos = 0;
        bc.set_current(irs[m_cur]);
        resize(bc.longest_taps());
        frame_now = 0;
    }
    void add_paths()
    {
        const BusConvolver::Paths& p = bc.paths;
        total.wrap += p.wrap, total.grow_taps += p.grow_taps, total.resize_cap += p.resize_cap, total.retire_time += p.retire_time;
        total.swap_in_fade += p.swap_in_fade, total.pending_replaced += p.pending_replaced, total.empty_response += p.empty_response;
        total.multi_run += p.multi_run;
    }

    void block(uint32_t frames) // og_engine::process_async
    {
        if (!queue.empty() && (size_t)q_frames + frames > cap_frames) launch();
        if (queue.empty()) {
            q_frame0 = frame_now;
            q_frames = 0;
        }
        const uint32_t conv = bc.queue_block(frame_now, FADE);
        if (m_pending >= 0) { // 1. pull a newly published engine: fade from the current one, whatever was fading is retired
            m_old = m_cur;
            m_old_from = m_cur_from;
            m_cur = m_pending;
            m_cur_from = frame_now;
            m_pos = 0;
            m_pending = -1;
        }
        for (uint32_t f = 0; f < frames; ++f) {
            qrec.push_back(MFrame{m_cur, m_old, m_cur_from, m_old_from, m_pos});
            if (m_old >= 0 && ++m_pos >= FADE) m_old = -1;
        }
        queue.push_back(QB{frames, conv});
        q_frames += frames;
        frame_now += frames;
        if (queue.size() >= batch) launch();
    }

    void publish(uint32_t k) // og_set_bus_ir
    {
        const int id = make_ir(k);
        if (bc.outgrows(k)) {
            launch();
            if (m_old >= 0) n_grow_in_fade += 1;
            resize(k);
        }
        if (k && k == bc.hist_keep() + 1) n_tight += 1;
        bc.publish(irs[id]);
        want(bc.published() == irs[id].get(), "published()");
        m_pending = id;
    }

    void set_batching(uint32_t blocks, bool shrink) // og_set_bus_batching (the engine itself never shrinks its buffers)
    {
        launch();
        const size_t cap = launch_frames_cap(blocks);
        if (cap > cap_frames || shrink) {
            cap_frames = cap;
            resize(bc.longest_taps());
        }
        batch = blocks;
    }

    void reset() // og_init: the queue is dropped, the history cleared, a published response stays published
    {
        queue.clear();
        qrec.clear();
        q_frames = 0;
        std::fill(hist.begin(), hist.end(), -1);
        bc.reset();
        m_old = -1;
        m_cur_from = m_old_from = 0;
        m_pos = 0;
        frame_now = 0;
        n_resets += 1;
    }

    void save_and_load() // og_save_state, then og_load_state of that blob: a swap no block has picked up is not part of it
    {
        launch();
        const ConvCfg cv = bc.cfg();
        const size_t hf = bc.tail_frames();
        want(hf <= bc.hist_pos(), "snapshot tail in front of the buffer");
        const std::vector<int64_t> tail(hist.begin() + bc.tail_at(hf), hist.begin() + bc.hist_pos());
        if (bc.outgrows(cv.longest_taps())) fail("a live response outgrows its own history");
        bc.restore(cv.cur, cv.old, cv.cur_from, cv.old_from, cv.fade_start);
        std::fill(hist.begin(), hist.end(), -1);
        want(hf <= bc.hist_pos() && bc.hist_pos() == bc.hist_keep(), "restore position");
        std::copy(tail.begin(), tail.end(), hist.begin() + bc.tail_at(hf));
        m_pending = -1;
        n_restores += 1;
    }

    // ---- a launch, checked ---------------------------------------------------------------------------------------------------
    void check_response(const OgConvResponse& r, int id, uint64_t from, uint64_t t0, size_t x_at)
    {
        const ConvIR& ir = *irs[id];
        want(r.taps == ir.d && r.n_taps == ir.K() && r.tap_stride == ir.stride(), "a run's response is not the model's", id);
        want((r.n_taps + S - 1) / S * (size_t)CH * bc.row_stride() <= bc.rows_half(), "rows outgrow their half", r.n_taps);
        want(r.lo > INT32_MIN && (int64_t)x_at + r.lo >= 0, "read below slot 0", r.lo);
        if (!r.n_taps || !r.n_frames) return;
        want(from <= t0, "valid-from frame behind the run's first frame");
        const int64_t K = r.n_taps, nf = r.n_frames, rel_from = (int64_t)from - (int64_t)t0;
        // frame f, tap k reads rel = f - k: entitled iff rel >= rel_from (frames before 0 lie before every `from`); the lowest
        // such sample of the run is frame 0's
        const int64_t lowest = std::max(rel_from, -(K - 1));
        want(r.lo <= lowest, "an entitled sample is below lo: the history is too short", r.lo, lowest);
        want(r.lo >= rel_from, "lo lets a sample through that lies before the valid-from frame", r.lo, rel_from);
        for (int64_t rel = lowest; rel < nf; ++rel)
            want(hist[(size_t)((int64_t)x_at + rel)] == (int64_t)t0 + rel, "the slot does not hold the frame read from it", rel, hist[(size_t)((int64_t)x_at + rel)]);
        for (int i = 0; i < 8; ++i) { // ... and as stated
            const int64_t f = (int64_t)rnd(0, (uint64_t)nf - 1), k = (int64_t)rnd(0, (uint64_t)K - 1), s = (int64_t)t0 + f - k;
            const bool entitled = s >= (int64_t)from && s >= 0, readable = f - k >= r.lo;
            want(entitled == readable, "entitled and readable differ", f, k);
            if (entitled) want(hist[(size_t)((int64_t)x_at + f - k)] == s, "sample (f, k) is not in its slot", f, k);
        }
    }

    void launch() // og_engine::flush_bus
    {
        if (queue.empty()) return;
        BusConvolver::Launch l = bc.plan_launch(q_frame0, q_frames, FADE);
        if (l.move) { // og_bus_conv_move: the ranges never overlap
            want(l.move_from + l.move_frames <= hist.size() && l.move_to + l.move_frames <= l.move_from, "history move out of bounds or overlapping");
            std::copy(hist.begin() + l.move_from, hist.begin() + l.move_from + l.move_frames, hist.begin() + l.move_to);
        }
        want(l.dry_at == bc.hist_pos() && l.dry_at >= bc.hist_keep() && l.dry_at + q_frames <= bc.hist_len(), "the dry sum does not fit", (int64_t)l.dry_at, q_frames);
        for (uint32_t f = 0; f < q_frames; ++f) hist[l.dry_at + f] = (int64_t)(q_frame0 + f);
        BusConvolver::Run r;
        size_t f0 = 0, b = 0, runs = 0;
        while (bc.next_run(l, queue, r)) {
            want(r.f0 == f0 && r.nf > 0 && r.nf <= bc.row_stride() && r.x_at == l.dry_at + f0, "run out of order or out of size", (int64_t)r.f0, r.nf);
            const uint32_t conv = queue[b].conv; // the blocks of the run: whole blocks of one configuration
            size_t covered = 0;
            while (b < queue.size() && covered < r.nf) {
                want(queue[b].conv == conv, "a run over two configurations", (int64_t)b);
                covered += queue[b++].frames;
            }
            want(covered == r.nf, "a run cuts a block", (int64_t)covered, r.nf);
            const uint64_t t0 = q_frame0 + f0;
            const MFrame& m0 = qrec[f0];
            uint32_t fading = 0;
            for (uint32_t f = 0; f < r.nf; ++f) {
                const MFrame& m = qrec[f0 + f];
                want(m.cur == m0.cur && m.cur_from == m0.cur_from, "the current response changes inside a run", f);
                if (m.old < 0) continue;
                want(fading == f, "the fade resumes inside a run", f);
                want(m.old == m0.old && m.old_from == m0.old_from && m.pos == r.fade_pos + f && m.pos < r.fade_len, "fade position", f, m.pos);
                fading += 1;
            }
            want(r.cur.n_frames == r.nf, "cur.n_frames", r.cur.n_frames);
            want(r.old.n_frames == fading, "old.n_frames is not the rest of the fade", r.old.n_frames, fading);
            want(r.fade_len == FADE, "fade_len");
            check_response(r.cur, m0.cur, m0.cur_from, t0, r.x_at);
            if (fading) check_response(r.old, m0.old, m0.old_from, t0, r.x_at);
            f0 += r.nf;
            runs += 1;
        }
        want(f0 == q_frames && b == queue.size(), "the runs do not cover the launch", (int64_t)f0, q_frames);
        bc.launched(l);
        want(bc.hist_pos() == l.dry_at + q_frames, "hist_pos after the launch");
        n_launches += 1;
        n_runs += runs;
        n_frames += q_frames;
        queue.clear();
        qrec.clear();
        q_frames = 0;
    }

    // ---- the generator --------------------------------------------------------------------------------------------------------
    uint32_t some_length()
    {
        static const uint32_t edges[] = {0, 1, 2, S - 1, S, S + 1, 2 * S + 3};
        const uint64_t c = rnd(0, 19);
        if (c < 8) return edges[rnd(0, 6)];
        if (c < 12) return (uint32_t)rnd(3, 700);
        if (c < 14) return (uint32_t)rnd(1000, 4000);                  // a few thousand
        if (c < 19) return (uint32_t)bc.hist_keep() + 1;               // exactly what the history allows: K - 1 == keep
        return (uint32_t)(bc.hist_keep() + 2 + rnd(0, 600));           // longer than it was sized for
    }
    uint32_t some_batch()
    {
        switch (rnd(0, 5)) {
        case 0: return 1;
        case 1: return (uint32_t)rnd(2, 8);
        case 2: case 3: return (uint32_t)rnd(2, MAX_LAUNCH_BLOCKS);
        case 4: return (uint32_t)rnd(MAX_LAUNCH_BLOCKS + 1, MAX_QUEUE_BLOCKS);
        default: return MAX_QUEUE_BLOCKS;
        }
    }
    void run()
    {
        create();
        for (step = 0; step < STEPS; ++step) {
            const uint64_t c = rnd(0, 999);
            if (c < 800) {
                const uint64_t k = rnd(0, 9);
                block(k == 0 ? (uint32_t)rnd(1, 8) : k == 1 ? MAX_BLOCK : k < 5 ? 256u : (uint32_t)rnd(1, MAX_BLOCK));
            } else if (c < 900) {
                publish(m_old >= 0 && rnd(0, 7) == 0 ? (uint32_t)(bc.hist_keep() + 2 + rnd(0, 300)) : some_length());
                if (rnd(0, 3) == 0) publish(some_length()); // before any block picked the first one up
            } else if (c < 940) {
                launch(); // forced early (a setter, a read-back)
            } else if (c < 975) {
                set_batching(some_batch(), rnd(0, 3) == 0);
            } else if (c < 985) {
                reset();
            } else if (c < 993) {
                save_and_load();
            } else if (bc.hist_keep() >= KEEP_MAX || rnd(0, 3) == 0) {
                launch();
                add_paths();
                create();
                n_engines += 1;
            }
        }
        launch();
        add_paths();
        const struct {
            const char* name;
            uint64_t n;
        } need[] = {{"history_wrap", total.wrap},
                    {"growth_by_taps", total.grow_taps},
                    {"resize_by_capacity", total.resize_cap},
                    {"retire_by_time", total.retire_time},
                    {"swap_during_fade", total.swap_in_fade},
                    {"pending_replaced", total.pending_replaced},
                    {"empty_response", total.empty_response},
                    {"multi_run_launch", total.multi_run},
                    {"tight_response", n_tight},
                    {"growth_during_fade", n_grow_in_fade}};
        bool missed = false;
        for (const auto& p : need) {
            printf("path seed %" PRIu64 " %s %" PRIu64 "\n", seed, p.name, p.n);
            missed = missed || p.n == 0;
        }
        printf("seed %" PRIu64 ": %zu steps, %" PRIu64 " launches, %" PRIu64 " runs, %" PRIu64 " frames, %zu responses, %" PRIu64 " resets, %" PRIu64
               " restores, %" PRIu64 " engines, keep %zu\n",
               seed, STEPS, n_launches, n_runs, n_frames, irs.size(), n_resets, n_restores, n_engines, bc.hist_keep());
        if (missed) {
            step = STEPS;
            fail("a branch never ran");
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    std::vector<uint64_t> seeds;
    for (int i = 1; i < argc; ++i) seeds.push_back(strtoull(argv[i], nullptr, 10));
    if (seeds.empty()) seeds = {1, 2, 3, 4};
    for (uint64_t s : seeds) Sim(s).run();
    printf("ok\n");
    return 0;
}
