// og_bus_conv_host.h -- the post-mix Convolver's host bookkeeping: which response runs over which frames of a launch, from
// which "history valid from" frame, where in the history buffer, and how large the buffers are.
// Host C++17 only (no HIP): the engine (og_engine.h) owns the device memory -- the history, the partial rows, the tap
// buffers -- and does the device work a plan describes; a `float*` device address is just a pointer here.  The kernels are
// og_bus_conv.hip.h's (it includes this header for the sizes and OgConvResponse);
// tests/standalone/bus_conv_model_main.cpp holds the class against a naive model on the CPU.
//
// The class never looks at the block queue or the clock: the frame a block starts at, the frames of a launch and the
// length of the crossfade (the engine's rate decides it) are arguments.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <memory>
#include <vector>

#define OG_CONV_S 256 // taps per segment
#define OG_CONV_F 256 // frames per tile
#define OG_CONV_LANES (OG_CONV_F / 4)
#define OG_CONV_MAX_TAPS (1u << 20) // 4 096 partial rows per frame at most

struct OgConvResponse {
    const float* taps; // device: n_taps floats, or -- tap_stride != 0 -- one plane of n_taps floats per channel, tap_stride apart
    uint32_t n_taps;   // per channel
    uint32_t n_frames; // frames of the run this response is evaluated for (the fading-out one: up to the end of the fade)
    int32_t lo;        // first readable sample, relative to the run's first frame: max(history valid from, start of the buffer)
    uint32_t tap_stride; // floats between the tap planes of two channels; 0: every channel reads the same plane
    float* rows;       // partial rows [segment][channel][row_stride]
};

// A response lives on the device from og_set_bus_ir (or og_create) until the engine is destroyed or a later
// og_set_bus_ir finds the stream idle: launches already queued may still read it.
// planes == 1: one tap plane shared by every bus channel (a mono response, a one-channel asset, any asset on a mono bus);
// otherwise one plane per bus channel, K() floats apart, plane-major on the device and in the host copy
struct ConvIR {
    float* d = nullptr;
    std::vector<float> taps; // host copy (snapshots, og_read_bus_ir): [planes][K]
    uint32_t planes = 1;
    uint32_t K() const { return (uint32_t)(taps.size() / planes); }
    uint32_t stride() const { return planes > 1 ? K() : 0u; } // OgConvResponse::tap_stride
};
// what a block is rendered under: the current response and, during the crossfade of a swap, the outgoing one; each with
// the frame its history is valid from (a new response only sees input from the swap frame on)
struct ConvCfg {
    std::shared_ptr<ConvIR> cur, old;
    uint64_t cur_from = 0, old_from = 0, fade_start = 0;
    bool same(const ConvCfg& o) const
    {
        return cur == o.cur && old == o.old && cur_from == o.cur_from && old_from == o.old_from && fade_start == o.fade_start;
    }
    static uint32_t taps_of(const std::shared_ptr<ConvIR>& ir) { return ir ? ir->K() : 0u; }
    static uint32_t planes_of(const std::shared_ptr<ConvIR>& ir) { return ir ? ir->planes : 1u; }
    uint32_t longest_taps() const { return std::max(taps_of(cur), taps_of(old)); } // the longer of current and outgoing response
    bool per_channel() const { return planes_of(cur) > 1 || planes_of(old) > 1; }
};

class BusConvolver {
public:
    // how often each branch ran.  Test instrumentation that the engine's instance carries too
    // (tests/standalone/bus_conv_model_main.cpp fails a run that missed a branch): one add per block or launch at most.
    struct Paths {
        uint64_t wrap = 0, grow_taps = 0, resize_cap = 0, retire_time = 0, swap_in_fade = 0, pending_replaced = 0, empty_response = 0,
                 multi_run = 0;
    } paths;

    // ---- sizing ---------------------------------------------------------------------------------------------------------
    // history: interleaved frames, [len][channels]; the next launch's dry bus goes to frame pos and at least keep frames in
    // front of it hold the input that came before (zeros before the first block).
    // partial rows: [current | outgoing][segment][channel][row_stride], rows_half floats each half
    size_t hist_len() const { return len_; }
    size_t hist_keep() const { return keep_; }
    size_t hist_pos() const { return pos_; }
    uint32_t row_stride() const { return row_stride_; }
    size_t rows_half() const { return rows_half_; }
    struct Sizing {
        size_t keep, len; // history
        uint32_t row_stride;
        size_t rows_half;
        bool new_hist, new_rows; // the buffer must be reallocated (a new history starts zeroed)
        size_t copy_from, copy_to, copy_frames; // new_hist: these frames of the old history go there in the new one
    };
    // buffers for responses of up to k taps and launches of up to cap_frames frames; the history never shrinks
    Sizing size_for(size_t k, size_t cap_frames, size_t channels) const
    {
        Sizing s;
        s.keep = std::max(keep_, (std::max<size_t>(k, 1) + OG_CONV_S - 1) / OG_CONV_S * OG_CONV_S);
        s.len = 2 * s.keep + 2 * cap_frames;
        s.new_hist = s.keep != keep_ || s.len != len_;
        s.copy_from = pos_ - keep_;
        s.copy_to = s.keep - keep_;
        s.copy_frames = keep_;
        s.row_stride = (uint32_t)((cap_frames + 3) / 4 * 4);
        s.rows_half = (s.keep / OG_CONV_S + 1) * channels * s.row_stride;
        s.new_rows = s.row_stride != row_stride_ || s.rows_half != rows_half_;
        return s;
    }
    void resized(const Sizing& s) // the engine has made the buffers what `s` says (nothing is queued)
    {
        if (s.new_hist && len_) (s.keep != keep_ ? paths.grow_taps : paths.resize_cap) += 1;
        keep_ = s.keep;
        len_ = s.len;
        if (s.new_hist) pos_ = s.keep;
        row_stride_ = s.row_stride;
        rows_half_ = s.rows_half;
    }
    // a response of k taps is longer than the buffers were sized for
    bool outgrows(size_t k) const { return k > keep_ + 1; }
    uint32_t longest_taps() const { return cfg_.longest_taps(); }
    // the input a snapshot carries: the longest live response's reach, the frames [hist_pos - n, hist_pos)
    size_t tail_frames() const { return longest_taps() ? longest_taps() - 1 : 0; }
    size_t tail_at(size_t n) const { return pos_ - n; } // (n <= keep <= pos)

    // ---- publishing (og_set_bus_ir) ---------------------------------------------------------------------------------------
    // takes effect at the first frame of the next block; replaces a response no block has picked up yet
    void publish(std::shared_ptr<ConvIR> ir)
    {
        if (pending_) paths.pending_replaced += 1;
        pending_ = std::move(ir);
    }
    // the response published last: the swap waiting for the next block, else the one the last block ran under
    const ConvIR* published() const { return pending_ ? pending_.get() : cfg_.cur.get(); }
    const ConvCfg& cfg() const { return cfg_; } // the state after the last queued block
    bool holds(const float* d) const // some response in use has its taps there
    {
        for (const ConvIR* ir : {cfg_.cur.get(), cfg_.old.get(), pending_.get()})
            if (ir && ir->d == d) return true;
        return false;
    }

    // ---- queuing a block ----------------------------------------------------------------------------------------------------
    // Convolver::process (convolution/mod.rs:535-573): the outgoing response is dropped once pos reaches fade_len; a swap
    // retires a response that is still fading out at once and fades from the current one, which keeps its history.
    // Returns the block's index into the queued configurations (QueuedBlock::conv).
    uint32_t queue_block(uint64_t frame_now, uint32_t fade_len)
    {
        if (cfg_.old && frame_now >= cfg_.fade_start + fade_len) {
            cfg_.old.reset();
            paths.retire_time += 1;
        }
        if (pending_) {
            if (cfg_.old) paths.swap_in_fade += 1;
            cfg_.old = std::move(cfg_.cur);
            cfg_.old_from = cfg_.cur_from;
            cfg_.cur = std::move(pending_);
            cfg_.cur_from = cfg_.fade_start = frame_now;
            pending_.reset();
        }
        if (q_.empty() || !q_.back().same(cfg_)) q_.push_back(cfg_);
        return (uint32_t)q_.size() - 1;
    }

    // ---- a launch -------------------------------------------------------------------------------------------------------------
    // The dry sum of the launch's frames goes behind the history; when the buffer is full the newest keep frames move to its
    // front first.  Then one pass per run of blocks queued under the same responses -- as a rule the whole launch.
    struct Launch {
        bool move;                                 // first: move_frames frames from history frame move_from to move_to
        size_t move_from, move_to, move_frames;
        size_t dry_at;                             // history frame of the launch's first frame
        uint64_t frame0;
        uint32_t frames, fade_len;
        size_t b, f0;                              // next_run: the next block and its first frame
    };
    struct Run {
        size_t f0;   // first frame, relative to the launch
        uint32_t nf;
        size_t x_at; // history frame of f0
        OgConvResponse cur, old; // `rows` is the engine's to fill; old.n_frames == 0: no fade over these frames
        uint32_t fade_pos, fade_len; // position in the fade at f0
    };
    Launch plan_launch(uint64_t q_frame0, uint32_t q_frames, uint32_t fade_len)
    {
        Launch l{};
        l.move = pos_ + q_frames > len_;
        if (l.move) {
            l.move_from = pos_ - keep_;
            l.move_to = 0;
            l.move_frames = keep_;
            pos_ = keep_;
            paths.wrap += 1;
        }
        l.dry_at = pos_;
        l.frame0 = q_frame0;
        l.frames = q_frames;
        l.fade_len = fade_len;
        return l;
    }
    // queue[i].frames / queue[i].conv: the queued blocks.  false: the launch has no further run
    template <class Queue>
    bool next_run(Launch& l, const Queue& queue, Run& r)
    {
        if (l.b >= queue.size()) return false;
        const size_t b0 = l.b;
        uint32_t nf = 0;
        while (l.b < queue.size() && queue[l.b].conv == queue[b0].conv) nf += queue[l.b++].frames;
        const ConvCfg& cf = q_[queue[b0].conv];
        const uint64_t t0 = l.frame0 + l.f0;
        const uint64_t fade_end = cf.fade_start + l.fade_len;
        r.f0 = l.f0;
        r.nf = nf;
        r.x_at = l.dry_at + l.f0;
        r.cur = response(cf.cur, cf.cur_from, t0, r.x_at, nf);
        r.old = response(cf.old, cf.old_from, t0, r.x_at, (cf.old && t0 < fade_end) ? (uint32_t)std::min<uint64_t>(nf, fade_end - t0) : 0u);
        r.fade_pos = (uint32_t)(t0 - cf.fade_start);
        r.fade_len = l.fade_len;
        if (b0 > 0 && l.b == queue.size()) paths.multi_run += 1;
        if (r.cur.n_taps == 0 || (r.old.n_frames && r.old.n_taps == 0)) paths.empty_response += 1;
        l.f0 += nf;
        return true;
    }
    void launched(const Launch& l)
    {
        pos_ += l.frames;
        q_.clear();
    }

    // ---- reset and restore ------------------------------------------------------------------------------------------------
    void reset() // prepare(): cleared history (the engine zeroes it), no fade; the current response stays
    {
        pos_ = keep_;
        cfg_.old.reset();
        cfg_.cur_from = cfg_.old_from = cfg_.fade_start = 0;
        q_.clear();
    }
    void set_current(std::shared_ptr<ConvIR> ir) { cfg_.cur = std::move(ir); } // og_create: the graph's response
    // og_load_state: the engine zeroes the history and writes the blob's tail to tail_at(its frames)
    void restore(std::shared_ptr<ConvIR> cur, std::shared_ptr<ConvIR> old, uint64_t cur_from, uint64_t old_from, uint64_t fade_start)
    {
        cfg_.cur = std::move(cur);
        cfg_.old = std::move(old);
        cfg_.cur_from = cur_from;
        cfg_.old_from = old_from;
        cfg_.fade_start = fade_start;
        pending_.reset();
        pos_ = keep_;
    }

private:
    static OgConvResponse response(const std::shared_ptr<ConvIR>& ir, uint64_t from, uint64_t t0, size_t x_at, uint32_t frames)
    {
        const int64_t buf_lo = -(int64_t)x_at;
        OgConvResponse r;
        r.taps = ir ? ir->d : nullptr;
        r.n_taps = ir ? ir->K() : 0u;
        r.n_frames = frames;
        r.lo = (int32_t)std::max<int64_t>(buf_lo, from >= t0 ? (int64_t)std::min<uint64_t>(from - t0, 0x7fffffffu) : -(int64_t)std::min<uint64_t>(t0 - from, 0x7fffffffu));
        r.tap_stride = ir ? ir->stride() : 0u;
        r.rows = nullptr;
        return r;
    }

    ConvCfg cfg_;
    std::shared_ptr<ConvIR> pending_;
    std::vector<ConvCfg> q_; // configurations of the queued blocks; keeps its capacity
    size_t len_ = 0, keep_ = 0, pos_ = 0;
    uint32_t row_stride_ = 0;
    size_t rows_half_ = 0;
};
