// tests/standalone/scope_main.cpp -- what a read of an Oscilloscope reconstructs on the host (csrc/og_scope_host.h), as a program
// of its own (built with a plain C++ compiler, also under -fsanitize=address,undefined; nothing is loaded into Python).
// A small simulation of the device's scheme (og_scope.hip.h: a physical ring, a window recorded by its end and length, copied
// only when asked to) fills planes of exactly the pool's size for three voices; ogscope::snapshot is compared with a plain
// history of what was pushed.  Cases: a pending window that wraps the physical ring, a copied window, capacity 1, an empty
// scope, sample_count beyond `available` and 0, null result pointers, the handle spelling and the node paths.
// Prints "all scope host cases as expected" at the end; exit status 1 on a failed check.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "og_scope_host.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: check FAILED: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

struct Sim { // one scope of a bank of NV voices, voice `v`
    uint32_t cap, P, nv, v;
    std::vector<float> ring, frozen; // [element][voice], exactly P x nv and cap x nv
    ogscope::Words w;
    std::vector<float> history, window; // the witnesses
    Sim(uint32_t cap_, uint32_t nv_, uint32_t v_) : cap(cap_), P(ogscope::ring_len(cap_)), nv(nv_), v(v_), ring((size_t)P * nv_, -7.0f), frozen((size_t)cap_ * nv_, -9.0f)
    {
        for (uint32_t i = 0; i < P; ++i) ring[(size_t)i * nv + v] = 0.0f;
    }
    void push(float x)
    {
        ring[(size_t)w.write_pos * nv + v] = x;
        w.write_pos = w.write_pos + 1 == P ? 0 : w.write_pos + 1;
        w.written = w.written < cap ? w.written + 1 : cap;
        history.push_back(x);
    }
    void trigger(uint32_t length)
    {
        length = length < cap ? length : cap;
        w.triggered_length = length > 1 ? length : 1;
        w.window_end = w.write_pos;
        w.pending = 1;
        window.clear();
        for (uint32_t j = 0; j < w.triggered_length; ++j) {
            const long t = (long)history.size() - (long)w.triggered_length + (long)j;
            window.push_back(t >= 0 ? history[(size_t)t] : 0.0f);
        }
    }
    void copy()
    {
        for (uint32_t j = 0; j < w.triggered_length; ++j)
            frozen[(size_t)j * nv + v] = ring[(size_t)((w.window_end + P - w.triggered_length + j) % P) * nv + v];
        w.pending = 0;
    }
    ogscope::Column ring_col() const { return ogscope::Column{ring.data() + v, nv}; }
    ogscope::Column frozen_col() const { return ogscope::Column{frozen.data() + v, nv}; }
    // snapshot(sample_count) against the witnesses; the result rows are exactly as long as the interface says
    void check(uint32_t sample_count) const
    {
        std::vector<float> s(sample_count < 1 ? 1 : sample_count, -1.0f), t(cap, -1.0f);
        uint32_t ns = 99, nt = 99;
        ogscope::snapshot(cap, ring_col(), frozen_col(), w, sample_count, s.data(), &ns, t.data(), &nt);
        const uint32_t available = history.size() < cap ? (uint32_t)history.size() : cap;
        uint32_t want = sample_count < 1 ? 1 : sample_count;
        want = want < available ? want : available;
        CHECK(ns == want);
        for (uint32_t j = 0; j < ns; ++j) CHECK(s[j] == history[history.size() - ns + j]);
        CHECK(nt == (available ? (uint32_t)window.size() : 0u));
        for (uint32_t j = 0; j < nt; ++j) CHECK(t[j] == window[j]);
        // lengths alone, and nothing at all
        uint32_t ns2 = 99, nt2 = 99;
        ogscope::snapshot(cap, ring_col(), frozen_col(), w, sample_count, nullptr, &ns2, nullptr, &nt2);
        CHECK(ns2 == ns && nt2 == nt);
        ogscope::snapshot(cap, ring_col(), frozen_col(), w, sample_count, nullptr, nullptr, nullptr, nullptr);
    }
    void check_all() const
    {
        for (uint32_t c : {0u, 1u, 5u, cap, cap + 1u, 10u * cap}) check(c);
    }
};

int main()
{
    CHECK(ogscope::ring_len(1) == 32 && ogscope::ring_len(7) == 32 && ogscope::ring_len(8) == 32 && ogscope::ring_len(64) == 144 && ogscope::ring_len(256) == 528);
    for (uint32_t cap = 1; cap <= 300; ++cap) CHECK(ogscope::ring_len(cap) % ogscope::CHUNK == 0 && ogscope::ring_len(cap) >= 2 * cap + ogscope::CHUNK);
    CHECK(ogscope::ring_len(ogscope::MAX_CAPACITY) == 2 * 65536 + 16);

    { // an empty scope: both results empty, whatever is asked for
        Sim s(16, 3, 1);
        s.check_all();
        s.w.triggered_length = 5; // (a loaded image may say so; nothing was pushed, nothing is handed out)
        uint32_t ns = 9, nt = 9;
        ogscope::snapshot(16, s.ring_col(), s.frozen_col(), s.w, 8, nullptr, &ns, nullptr, &nt);
        CHECK(ns == 0 && nt == 0);
    }
    { // the reference's known answers (mod.rs:293-323)
        Sim s(8, 3, 2);
        for (int i = 0; i < 10; ++i) s.push((float)i);
        float out[4];
        uint32_t n = 0, nt = 9;
        ogscope::snapshot(8, s.ring_col(), s.frozen_col(), s.w, 4, out, &n, nullptr, &nt);
        CHECK(n == 4 && out[0] == 6 && out[1] == 7 && out[2] == 8 && out[3] == 9 && nt == 0);
        Sim q(4, 3, 0);
        for (int i = 0; i < 4; ++i) q.push((float)i);
        q.check(16);
    }
    { // a pending window that wraps the physical ring, then the same window copied
        Sim s(8, 3, 1); // P = 32
        for (int i = 0; i < 35; ++i) s.push(100.0f + (float)i);
        CHECK(s.w.write_pos == 3);
        s.trigger(8); // physical 27..31, 0..2
        CHECK(s.w.window_end == 3 && s.w.pending == 1);
        s.check_all();
        for (int i = 0; i < 7; ++i) s.push(-(float)i); // later pushes do not disturb it
        s.check_all();
        s.copy();
        for (int i = 0; i < 40; ++i) s.push(0.5f * (float)i); // the ring may now run over where it lay
        CHECK(s.w.pending == 0);
        s.check_all();
    }
    { // a window longer than what was pushed so far: the samples in front of the first push are 0.0
        Sim s(8, 3, 0);
        for (int i = 0; i < 3; ++i) s.push(1.0f + (float)i);
        s.trigger(8); // physical 27..31 (never written: 0.0), 0..2
        CHECK(s.window[0] == 0.0f && s.window[4] == 0.0f && s.window[5] == 1.0f && s.window[7] == 3.0f);
        s.check_all();
        s.copy();
        s.check_all();
    }
    { // short windows, window_end at 0 and at P - 1
        Sim s(7, 3, 2); // P = 32
        for (int i = 0; i < 32; ++i) s.push((float)i);
        CHECK(s.w.write_pos == 0);
        s.trigger(3);
        s.check_all();
        for (int i = 0; i < 31; ++i) {
            s.push(40.0f + (float)i);
            if (i == 5) s.trigger(1000); // clamped to the capacity
        }
        CHECK(s.w.write_pos == 31 && s.w.triggered_length == 7);
        s.check_all();
        s.trigger(0); // at least one sample
        CHECK(s.w.triggered_length == 1 && s.w.window_end == 31);
        s.check_all();
    }
    { // capacity 1
        Sim s(1, 3, 1);
        s.check_all();
        for (int i = 0; i < 70; ++i) {
            s.push(3.0f * (float)i);
            if (i % 9 == 4) s.trigger(1);
            if (i % 18 == 13) s.copy();
            s.check_all();
        }
    }
    { // a cleared window: length 0, pending or not
        Sim s(8, 3, 1);
        for (int i = 0; i < 20; ++i) s.push((float)i);
        s.trigger(8);
        s.w.triggered_length = 0;
        s.w.pending = 0;
        s.window.clear();
        s.check_all();
    }
    // the handle of the text front end
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new(64)") == 64);
    CHECK(ogscope::handle_capacity(" OscilloscopeHandle :: new ( 4_096usize ) ") == 4096);
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new(0)") == 0);
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new()") == -1);
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new(n)") == -1);
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new(6.5)") == -1);
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new(-4)") == -1);
    CHECK(ogscope::handle_capacity("OscilloscopeHandle::new(9999999999999)") == -1);
    CHECK(ogscope::handle_capacity("shared_handle.clone()") == -1);
    CHECK(ogscope::handle_capacity("") == -1);
    CHECK(ogscope::flat_node("scope") == "scope" && ogscope::flat_node("scopes[1]") == "scopes__1" && ogscope::flat_node("inner.scopes[0]") == "inner_scopes__0");

    if (failures) {
        fprintf(stderr, "%d checks FAILED\n", failures);
        return 1;
    }
    printf("all scope host cases as expected\n");
    return 0;
}
