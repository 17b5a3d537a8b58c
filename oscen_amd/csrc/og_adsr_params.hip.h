// og_adsr_params.hip.h -- the AdsrEnvelope body for attack / decay / sustain / release that move: og::AdsrP, and the exact
// expf its per-lane coefficients need.  Included only by the generated kernels that use it (og_graph.cpp, emit_adsr), so
// it is no part of OG_RT_DIGEST: the kernels of graphs with block-uniform envelope parameters keep their names, and the
// committed profiles stay theirs.  Its own digest, OG_ADSRP_DIGEST, is folded into the hash of the kernels that do
// include it (og_rt_digest.h, written by build.py).
//
// og_expf_exact() is plain C++ (host and device), like og_math.h: tests/test_expf_exact_cpu.py builds it for the host.
#pragma once
#include "og_math.h"

// ---------------------------------------------------------------------------
// expf(x) for x in [-4.6051702, 0), correctly rounded from a double evaluation: the argument of the ADSR one-pole
// coefficient `1 - exp(-4.6051702 / n)` (oscen-lib/src/envelope/adsr.rs:132-133).  The coefficient is applied n times,
// so an expf that is one ulp off moves the curve by 2e-5 at n = 4 800 and 2e-4 at n = 48 000: the device needs the
// host libm's bits wherever a lane derives its own coefficient (og::AdsrP below).  glibc's expf is itself a
// double evaluation rounded once and equals the correctly rounded value on all but 2 of the 2^24 arguments
// -4.6051702f / (float)n (tests/test_expf_exact_cpu.py counts them), so this routine aims at correct rounding rather
// than at glibc's table: x = k ln2 + r with |r| <= ln2 / 2 (two-word ln2, exact products: |k| <= 7), the degree-13
// Taylor polynomial of exp(r) (truncation 4e-18) by Horner with fma, an exact scaling by 2^k and ONE rounding to f32.
// Error before that rounding <= ~2e-16, against f32 half-ulps of 3e-8.  IEEE double +, * and fma (the builtin) only -- no
// libm, no device math library -- so host and device give the same bits.  Outside the domain the result is still a good exp
// for |x| < 700 but the exactness claim is not made.
// ---------------------------------------------------------------------------
OG_HD float og_expf_exact(float xf)
{
    const double INV_LN2 = 0x1.71547652b82fep+0;
    const double LN2_HI = 0x1.62e42fefa38p-1;    // 42 leading bits of ln 2: k * LN2_HI is exact
    const double LN2_LO = 0x1.ef35793c7673p-45;  // ln 2 - LN2_HI
    const double MAGIC = 0x1.8p52;
    const double x = (double)xf;
    const double kd = (x * INV_LN2 + MAGIC) - MAGIC; // rint(x / ln 2)
    double r = __builtin_fma(-kd, LN2_HI, x);
    r = __builtin_fma(-kd, LN2_LO, r);
    double p = 0x1.6124613a86d09p-33;            // 1/13!
    p = __builtin_fma(p, r, 0x1.1eed8eff8d898p-29);        // 1/12!
    p = __builtin_fma(p, r, 0x1.ae64567f544e4p-26);        // 1/11!
    p = __builtin_fma(p, r, 0x1.27e4fb7789f5cp-22);        // 1/10!
    p = __builtin_fma(p, r, 0x1.71de3a556c734p-19);        // 1/9!
    p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-16);        // 1/8!
    p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-13);        // 1/7!
    p = __builtin_fma(p, r, 0x1.6c16c16c16c17p-10);        // 1/6!
    p = __builtin_fma(p, r, 0x1.1111111111111p-7);         // 1/5!
    p = __builtin_fma(p, r, 0x1.5555555555555p-5);         // 1/4!
    p = __builtin_fma(p, r, 0x1.5555555555555p-3);         // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    union { double d; unsigned long long u; } s;
    s.u = (unsigned long long)(1023 + (int32_t)kd) << 52;  // 2^k
    return (float)(p * s.d);
}

#if defined(__HIPCC__) || defined(OG_HOSTSIM)
#include "og_nodes.hip.h"

namespace og {

// ---------------------------------------------------------------------------
// AdsrEnvelope whose attack / decay / sustain / release are NOT block-uniform: a ramped input, a per-voice input, a
// node output or an expression of one.  The reference re-derives everything from its four fields on every sample
// (process() starts with apply_parameters(), adsr.rs:84-134, 282-285); og::Adsr (og_nodes.hip.h) leaves that to the host, once
// per block.  Here every lane keeps the reference's derived fields in registers next to the last raw values of the four
// inputs, compares them each frame (like the TPT filter its raw cutoff) and redoes apply_parameters() on a change and
// once at block start; repeating it on unchanged fields changes nothing (the lengths, coefficients and sustain_level
// come out the same, samples_remaining is already inside its stage's length), so the frames in between skip it.
//
// The per-sample arithmetic is that of og::adsr_tick (fused one-pole step, Release as rcp(cnt)); a stage end is
// tested on every frame, right after the step.  The coefficients need the host libm's bits (og_expf_exact above):
// the uniform body gets them from the host.
//
// (stage, cnt, lv, vel) are what the four state words hold; everything else is rebuilt by the block's first tick
// (adsrp_block_begin): snapshots keep their layout.  What that costs against the reference: it carries its cached lengths
// across a block boundary, so a gate-off on the very first frame after `release` changed starts from the old length
// there and from the new one here (the uniform body has the same rule for a value changed between two blocks).
// ---------------------------------------------------------------------------
constexpr float ADSR_MIN_TIME_SECONDS = 1.0e-5f;
constexpr float ADSR_CURVE_TIME_CONSTANT = 4.6051702f;

struct AdsrP {
    uint32_t stage = 0u, cnt = ADSR_HOLD; // cnt = samples_remaining, ADSR_HOLD in Sustain / Idle
    float lv = 0.0f, tgt = 0.0f, cf = 0.0f, vel = 1.0f, sus = 0.0f, rs = 0.0f;
    float in_a = 0.0f, in_d = 0.0f, in_s = 0.0f, in_r = 0.0f; // the raw inputs the cached fields below were derived from
    uint32_t a_n = 1u, d_n = 1u, r_n = 1u;                    // attack_samples, decay_samples, release_samples
    float a_c = 0.0f, d_c = 0.0f;                             // attack_coeff, decay_coeff
    uint32_t fresh = 1u;          // the block's first tick has not run yet: (stage, cnt, lv, vel) are the raw state words
    uint32_t qn = 0u;             // gate events waiting for this frame's tick (the node's event queue)
    float q0 = 0.0f, q1 = 0.0f;
};

// the state words as loaded; the cache is built by the block's first tick, where every kind of source has a value
OG_DEV void adsrp_load(AdsrP& e, uint32_t stage, uint32_t rem, float level, float vel)
{
    e.stage = stage;
    e.cnt = rem;
    e.lv = level;
    e.vel = vel;
    e.fresh = 1u;
}
// A gate event arrives: it is handled by the tick of its frame, after that frame's parameter values are known -- the
// reference's order at the outer rate (connection assignments, process_event_inputs(), process()).  Two per frame (a
// note-off and a note-on on one frame); of more than two the last two are kept.
OG_DEV void adsrp_push(AdsrP& e, float v)
{
    e.q0 = (e.qn == 0u) ? v : ((e.qn >= 2u) ? e.q1 : e.q0);
    e.q1 = (e.qn == 0u) ? e.q1 : v;
    e.qn = min(e.qn + 1u, 2u);
}

// `(t.max(MIN_TIME_SECONDS) * sample_rate.max(1.0)) as u32`, `.max(1)` (adsr.rs:118-127; `as u32` saturates)
OG_DEV uint32_t adsrp_samples(float t, float sr)
{
    const float x = fmaxf(fmaxf(t, 0.0f), ADSR_MIN_TIME_SECONDS) * fmaxf(sr, 1.0f);
    const uint32_t n = (x >= 4294967296.0f) ? 0xFFFFFFFFu : (uint32_t)x;
    return max(n, 1u);
}
// `1.0 - (-CURVE_TIME_CONSTANT / n as f32).exp()` (adsr.rs:132-133): IEEE f32 division, the host libm's exp
OG_DEV float adsrp_coeff(uint32_t n) { return 1.0f - og_expf_exact(-ADSR_CURVE_TIME_CONSTANT / (float)n); }

// what set_stage() leaves behind, from the cached fields
OG_DEV void adsrp_enter(AdsrP& e, uint32_t stage)
{
    // (every field is read before the selects: a select between two loads becomes a load from a selected address, and the
    //  struct then lives in scratch instead of registers)
    const uint32_t a_n = e.a_n, d_n = e.d_n, r_n = e.r_n;
    const float a_c = e.a_c, d_c = e.d_c, sus = e.sus;
    const bool att = stage == ST_ATTACK, dec = stage == ST_DECAY, rel = stage == ST_RELEASE;
    e.stage = stage;
    e.cnt = att ? a_n : (dec ? d_n : (rel ? r_n : ADSR_HOLD));
    e.tgt = att ? 1.0f : (dec ? sus : 0.0f);
    e.cf = att ? a_c : (dec ? d_c : 0.0f);
    e.rs = rel ? 1.0f : 0.0f;
}

// apply_parameters() + update_sustain_level() (adsr.rs:84-115) for the raw inputs (a, d, s, r): the clamps, sustain_level,
// the three lengths, both coefficients, the samples_remaining clamp of the stage in progress and the target refresh.
// (A coefficient is only recomputed when its length moved: it is a function of the length alone.)
OG_DEV void adsrp_apply(AdsrP& e, float a, float d, float s, float r, float sr)
{
    e.in_a = a;
    e.in_d = d;
    e.in_s = s;
    e.in_r = r;
    e.sus = clamp01(clamp01(s) * e.vel);
    const uint32_t a_n = adsrp_samples(a, sr), d_n = adsrp_samples(d, sr);
    if (a_n != e.a_n) e.a_c = adsrp_coeff(a_n);
    if (d_n != e.d_n) e.d_c = adsrp_coeff(d_n);
    e.a_n = a_n;
    e.d_n = d_n;
    e.r_n = adsrp_samples(r, sr);
    const bool att = e.stage == ST_ATTACK, dec = e.stage == ST_DECAY, rel = e.stage == ST_RELEASE;
    // (selects on values read beforehand, see adsrp_enter.  cnt >= 1 while one of the three stages is in progress -- a
    //  countdown that reaches 0 completes the stage -- so the reference's `samples_remaining > 0` guard always holds)
    const uint32_t r_n = e.r_n, cnt = e.cnt;
    const float a_c = e.a_c, d_c = e.d_c, sus = e.sus, tgt = e.tgt;
    const uint32_t lim = att ? a_n : (dec ? d_n : r_n);
    e.cnt = (att | dec | rel) ? max(min(cnt, lim), 1u) : cnt;
    e.cf = att ? a_c : (dec ? d_c : 0.0f);
    e.tgt = dec ? sus : tgt; // (Sustain: adsrp_tick pins the level itself; Release: tgt is 0 already)
}

// the block's first tick: the register form of the four state words, then the parameter cache from the values of that frame
OG_DEV void adsrp_block_begin(AdsrP& e, float a, float d, float s, float r, float sr)
{
    const uint32_t stage = e.stage;
    const bool moving = (stage == ST_ATTACK) | (stage == ST_DECAY) | (stage == ST_RELEASE);
    e.cnt = (moving && e.cnt > 0u) ? e.cnt : ADSR_HOLD;
    e.lv = (stage == ST_IDLE) ? 0.0f : clamp01(e.lv);
    e.tgt = (stage == ST_ATTACK) ? 1.0f : 0.0f;
    e.rs = (stage == ST_RELEASE) ? 1.0f : 0.0f;
    e.a_n = e.d_n = 0u; // (no length: both coefficients are derived below)
    e.a_c = e.d_c = 0.0f;
    e.fresh = 0u;
    adsrp_apply(e, a, d, s, r, sr);
}
// what the state plane holds at block end (a block of no frames: the word as loaded)
OG_DEV uint32_t adsrp_rem(const AdsrP& e) { return (e.stage == ST_SUSTAIN || e.stage == ST_IDLE) ? 0u : e.cnt; }

// handle_gate_event (adsr.rs:250-273) with the parameter values (a, d, s, r) the reference's fields hold when its
// handler runs (adsrp_tick: which frame's values those are).  Gate-on goes through
// update_sustain_level(), i.e. re-derives every cached field from them; gate-off takes release_samples as cached by the
// last process() or gate-on and reads only `release` itself.
OG_DEV void adsrp_gate(AdsrP& e, float v, float a, float d, float s, float r, float sr)
{
    if (v > 0.0f) {
        e.vel = clamp01(v);
        adsrp_apply(e, a, d, s, r, sr);
        if (a <= ADSR_MIN_TIME_SECONDS) {
            e.lv = 1.0f;
            adsrp_enter(e, ST_DECAY);
        } else {
            adsrp_enter(e, ST_ATTACK);
        }
    } else if (r <= ADSR_MIN_TIME_SECONDS) {
        e.lv = 0.0f;
        adsrp_enter(e, ST_IDLE);
    } else {
        adsrp_enter(e, ST_RELEASE);
    }
}

// One sample: the frame's gate events (process_event_inputs()), then process() = apply_parameters() when an input moved
// and process_stage() (adsr.rs:206-248) with complete_stage().
// HELD: an envelope of the oversampled region.  The reference runs its handlers in front of the inner loop (step 6a of
// the frame) and writes its value inputs inside it: a handler reads the values the previous tick was given, in_*.
template <bool HELD>
OG_DEV float adsrp_tick(AdsrP& e, float a, float d, float s, float r, float sr)
{
    if (e.fresh != 0u) adsrp_block_begin(e, a, d, s, r, sr);
    if (e.qn != 0u) {
        adsrp_gate(e, e.q0, HELD ? e.in_a : a, HELD ? e.in_d : d, HELD ? e.in_s : s, HELD ? e.in_r : r, sr);
        if (e.qn > 1u) adsrp_gate(e, e.q1, HELD ? e.in_a : a, HELD ? e.in_d : d, HELD ? e.in_s : s, HELD ? e.in_r : r, sr);
        e.qn = 0u;
    }
    if ((a != e.in_a) | (d != e.in_d) | (s != e.in_s) | (r != e.in_r)) adsrp_apply(e, a, d, s, r, sr);
#ifdef OG_STRICT
    float lv = e.lv + (e.tgt - e.lv) * e.cf;
    lv = fmaf(e.rs, div_near(-lv, (float)e.cnt), lv);
#else
    const float cf = fmaf(e.rs, __builtin_amdgcn_rcpf((float)e.cnt), e.cf); // (cnt >= 1, ADSR_HOLD while holding: finite)
    float lv = fmaf(e.tgt - e.lv, cf, e.lv);
#endif
    if (e.stage == ST_SUSTAIN) lv = e.sus; // Stage::Sustain: level = sustain_level on every sample (adsr.rs:241-243)
    e.cnt -= 1u;
    if (e.cnt == 0u) { // the stage ends on its target level, which is also this frame's output
        lv = e.tgt;
        adsrp_enter(e, (e.stage + 1u) & 7u); // Attack -> Decay -> Sustain, Release -> Idle
    }
    e.lv = lv;
    return lv;
}

} // namespace og
#endif
