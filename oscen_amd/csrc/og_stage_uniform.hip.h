// og_stage_uniform.hip.h -- stage-uniform envelope bodies of the deeper zero variant's four-wave pipeline (og_graph.cpp,
// PipelineWave::fast_variants): the entry predicates, the chunk flag and the envelope tick of the two sticky quiet bodies a
// wave takes while EVERY envelope of its stage, in EVERY lane, sits in a stage whose per-frame arithmetic is known in advance.
// Included only by the `_z2` units (csrc/gen/<graph>_z2.hip), so it is no part of OG_RT_DIGEST and of no kernel's hash: the
// general kernels keep their names and the committed profiles stay theirs.  Its own digest, OG_STAGEU_DIGEST (og_rt_digest.h,
// written by build.py), stands in the head comment of every unit that includes it.
//
// The general quiet tick of og::Adsr (og_nodes.hip.h, adsr_tick / adsr_tick_r) is, per envelope and frame,
//     cf' = fma(rs, r, cf)          (release bodies only; r = v_rcp_f32((float)cnt), computed or read from the table)
//     lv' = fma(tgt - lv, cf', lv)
// rs, cf and tgt are written by adsr_enter() alone -- at block start, on a gate event, at a stage end -- and a quiet chunk has
// none of the three: inside a sticky quiet loop they do not change.  Both predicates below are therefore tested where a wave
// ENTERS a body and hold for as long as the loop's own stay condition does.
//
// ---- the hold body (ENV_HOLD) ----------------------------------------------------
// Entry: in every lane, for every envelope of the stage, cf bits == 0 and rs bits == 0 (Sustain, Idle, or an Attack / Decay whose
// coefficient is +0), lv bits != 0x80000000, and lv and tgt are below 2^127 in magnitude (in particular no inf, no NaN).
// Claim: fma(tgt - lv, +0, lv) has the bits of lv.
//   d = tgt - lv is finite (|tgt|, |lv| < 2^127, so |d| < 2^128 does not overflow), so p = d * (+0) is +0 or -0, exactly, and the
//   fma returns p + lv rounded once.
//   lv != 0 (normal or denormal; the kernels keep denormals):  p + lv = lv exactly, no rounding.
//   lv == +0:  (+0) + (+0) = +0 and (-0) + (+0) = +0 under round-to-nearest-even.  lv's bits.
//   lv == -0:  d = tgt + 0 is >= +0 for every tgt >= 0, so p = +0 and (+0) + (-0) = +0 -- NOT lv's bits.  This is why the entry
//              tests the sign-only pattern: clamp01(-0) can be -0, and a sustain of -0 puts it into lv at a Decay's end.
//   lv inf / NaN:  excluded (inf * 0 and the quieting of a signalling NaN change bits).
// The release-free general body is that one fma (RELEASE = false: cf' = cf), so the body's output and level are `lv`, untouched;
// cnt steps as it does today (ADSR_HOLD - k in a holding stage, re-pinned by adsr_enter; the countdown of a +0-coefficient
// Attack / Decay still ends its stage through the loop's `cnt > XCH` test).
//
// ---- the pure-release body (ENV_RELEASE) --------------------------------------
// Entry: in every lane, for every envelope of the stage, rs bits == 1.0f, cf bits == 0, tgt bits == 0 (what adsr_enter sets for
// Release) and lv is no NaN.  A lane past the last voice of the bank counts as qualifying (see below).
// Claim: fma(tgt - lv, fma(rs, r, cf), lv) has the bits of fma(-lv, r, lv).
//   cf' = fma(1.0f, r, +0) = r + (+0), one rounding of an exact value: r for every r but -0.  r is the reciprocal of a countdown
//        in [1, 2^32): positive and normal.  cf' == r.
//   d = (+0) - lv:  lv != 0 or lv == -0 -> d = -lv exactly (0 - (-0) = +0 = -(-0)).  lv == +0 -> d = +0 where -lv = -0: the one
//        pattern where the operands differ -- and there fma(+0, r, +0) = (+0) + (+0) = +0 and fma(-0, r, +0) = (-0) + (+0) = +0
//        (r > 0, finite): the same bits.  lv = +-inf: d = -lv exactly, identical operands.  NaN: excluded (the sign of a NaN
//        operand may reach the result's bits).
// So one v_fma_f32 with a negated source replaces v_fma + v_sub + v_fma.  r comes from where it comes today: the chunk's table
// entries (wide form, og::rcp_fetch / rcp_refill) or v_rcp_f32(fc) with fc -= 1 (8-frame form).
// Lanes past the last voice (c.valid false) keep the constructor's envelope {lv +0, tgt 1, cf +0, rs +0, cnt ADSR_HOLD}: the
// general body gives fma(1 - 0, fma(0, r, 0), +0) = +0 and this one fma(-0, r, +0) = +0 with r finite (the table entry at
// min(cnt, rcp_len), or 1 / fc with fc = (float)cnt just below 2^32): their level stays +0 either way, and nothing of theirs
// is stored.
//
// OG_STRICT builds keep the general tick in both bodies (its release arithmetic is a different expression).
//
// ---- the quiet quarters of a checked chunk (og_graph.cpp, PipelineWave::checked; wide form) ----
// A chunk with an event or a stage end in ANY lane runs the checked body: per frame f = base + j one wave-uniform event test
// (`any lane has next_ev == f` -> events(f)) and, per envelope, the tick adsr_tick<true, true> on e.fc followed by the stage-end
// test (cnt == 0 -> adsr_complete).  The body is cut into quarters of four frames, j = 4q .. 4q + 3, and before quarter q the
// wave tests, on the state quarter q - 1 left,
//     (E) in every lane  next_ev >= base + 4q + 4        (M) in every lane, for every envelope of the stage  cnt > 4
// and where both hold it runs the four frames with the chunk flag BoolC<false, true, pre, false> instead of <true, true, pre,
// false>, and without the event test.
// Claim: under (E) and (M) the checked quarter's tests do not fire, so leaving them out leaves the same operations.
//   Events.  next_ev changes only in events() (og::ev_advance), which the quiet quarter does not call; so next_ev >= base + 4q + 4
//     > f holds at each of its frames, in every lane: `f == next_ev` is false in every lane and the checked quarter would not
//     have called events() either.
//   Stage ends.  cnt changes by the tick's `cnt -= 1` and in adsr_enter(), which only events() and adsr_complete() reach.  With
//     no events() (above), by induction over the four frames: before frame 4q + i no stage end has fired in this quarter, so cnt
//     is its value at the test minus i, > 4 - i; after the tick it is > 3 - i >= 0 for i <= 3: not 0, adsr_complete() does
//     nothing, and the induction goes on.  A holding envelope counts down from ADSR_HOLD = 2^32 - 1 and is re-pinned by
//     adsr_enter(); it passes (M) for as long as it passes the chunk test's `cnt > XCH`.
//   The tick.  The flag's `value` guards the stage-end blocks and nothing else; `release`, `pre`, `steady` and `table` are the
//     same in both flags and neither is a StageC, so both quarters run adsr_tick_chunk<true, false> = adsr_tick<true, true>: the
//     reciprocal of e.fc and `fc -= 1`.  e.fc == (float)cnt at the chunk's top (the body's first lines) and after every
//     adsr_enter(); the quiet and the checked quarters step it alike, so it does not matter which kind ran before.
//   The test is taken again before every quarter.  An event or a completed stage in quarter q - 1 went through adsr_enter(): the
//     countdown (M) reads before quarter q is the entered stage's real one (a 3-frame attack entered in quarter q - 1 fails (M)
//     and its end is met in a checked quarter), and next_ev is the lane's following event.
// Not covered, on purpose: rcp_len, rs and the stage-uniform predicates play no part -- the quarter keeps the checked body's own
// release form, so a short reciprocal table or a mixed wave changes nothing here.
#pragma once
#include "og_nodes.hip.h"

// the last uniform slot, when the graph does not use it (og_graph.cpp emits these bodies only then): non-zero = the launch keeps
// to the general quiet bodies.  The engine sets it under OSCEN_GPU_EXPERIMENTAL=1 OSCEN_GPU_STAGE_SPEC=0 (A/B of the bodies
// inside one library).
#define OG_STAGE_SPEC_SLOT (OG_MAX_SLOTS - 1)

#ifdef OG_HOSTSIM
// host simulator only: chunks run in the hold ([0][stage]) and the pure-release ([1][stage]) body since the library was
// loaded, one count per wave and chunk -- a test reads it through the library's handle, like the runtime's C symbols
extern "C" {
__attribute__((weak)) unsigned long long og_stage_uniform_chunks[2][8] = {};
// ... and the quarters of checked chunks run without ([0][stage]) and with ([1][stage]) their tests, one count per wave and quarter
__attribute__((weak)) unsigned long long og_checked_quarters[2][8] = {};
}
#endif

namespace og {

enum : int { ENV_GENERAL = 0, ENV_HOLD = 1, ENV_RELEASE = 2 };

// the chunk flag of the two bodies: og::BoolC (no stage-end checks; release arithmetic and table as in the body they stand
// next to) plus which envelope arithmetic the chunk's ticks run
template <int M, bool P, bool S, bool T = false>
struct StageC : BoolC<false, M == ENV_RELEASE, P, S, T> {
    static constexpr int env = M;
};
template <bool B, bool R, bool P, bool S, bool T>
constexpr int env_mode(BoolC<B, R, P, S, T>) { return ENV_GENERAL; }
template <int M, bool P, bool S, bool T>
constexpr int env_mode(StageC<M, P, S, T>) { return M; }

__device__ __forceinline__ bool stage_spec_on(const OgBlockArgs& a) { return a.slots[OG_STAGE_SPEC_SLOT] == 0u; }

// |x| < 2^127: the exponent field is below 0xfe
OG_DEV bool adsr_small(const float x) { return (__float_as_uint(x) & 0x7f800000u) < 0x7f000000u; }

OG_DEV bool adsr_holds(const Adsr& e)
{
    return (__float_as_uint(e.cf) | __float_as_uint(e.rs)) == 0u && __float_as_uint(e.lv) != 0x80000000u && adsr_small(e.lv) && adsr_small(e.tgt);
}

OG_DEV bool adsr_releases(const Adsr& e)
{
    return __float_as_uint(e.rs) == 0x3f800000u && (__float_as_uint(e.cf) | __float_as_uint(e.tgt)) == 0u && e.lv == e.lv;
}

// frame j of a chunk body: M = ENV_GENERAL is og::adsr_tick_chunk
template <int M, bool RELEASE, bool TABLE, uint32_t N>
OG_DEV float adsr_tick_stage(Adsr& e, const float (&rcp)[N], const uint32_t j)
{
#ifndef OG_STRICT
    if constexpr (M == ENV_HOLD) {
        e.cnt -= 1u;
        return e.lv;
    } else if constexpr (M == ENV_RELEASE) {
        float r;
        if constexpr (TABLE) {
            r = rcp[j];
        } else {
            r = __builtin_amdgcn_rcpf(e.fc);
            e.fc -= 1.0f;
        }
        const float lv = fmaf(-e.lv, r, e.lv);
        e.cnt -= 1u;
        e.lv = lv;
        return lv;
    } else
#endif
        return adsr_tick_chunk<RELEASE, TABLE>(e, rcp, j);
}

// after frame j of an unrolled chunk of N frames: the instruction scheduler does not move anything across the chunk's middle
// (og_graph.cpp, PipelineWave::quiet, says where and why); no instruction of its own
template <uint32_t N>
__device__ __forceinline__ void stage_sched_fence(const uint32_t j)
{
#ifndef OG_HOSTSIM
    if (2u * (j + 1u) == N) __builtin_amdgcn_sched_barrier(0);
#else
    (void)j;
#endif
}

// host simulator: one count per wave and chunk; nothing on the device
template <int M>
__device__ __forceinline__ void stage_body_count(const uint32_t stage)
{
#ifdef OG_HOSTSIM
    static_assert(M == ENV_HOLD || M == ENV_RELEASE, "a stage-uniform body");
    if (threadIdx.x % OG_WAVE == 0u) og_stage_uniform_chunks[M - 1][stage & 7u] += 1ull;
#else
    (void)stage;
#endif
}

// after a frame of a checked quarter: the instruction scheduler does not move anything across (og_graph.cpp,
// PipelineWave::checked, says where and why); no instruction of its own
__device__ __forceinline__ void frame_sched_fence()
{
#ifndef OG_HOSTSIM
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// host simulator: one count per wave and quarter of a checked chunk (CHECKED = the quarter kept its tests); nothing on the device
template <bool CHECKED>
__device__ __forceinline__ void quarter_count(const uint32_t stage)
{
#ifdef OG_HOSTSIM
    if (threadIdx.x % OG_WAVE == 0u) og_checked_quarters[CHECKED ? 1 : 0][stage & 7u] += 1ull;
#else
    (void)stage;
#endif
}

} // namespace og
