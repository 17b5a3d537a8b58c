// og_sample_player.hip.h -- SamplePlayer (oscen-lib/src/sample_player/mod.rs): looping playback of a buffer from the
// engine's device sample pool.  Included only by the kernels of graphs that hold a player; its digest (OG_SMP_DIGEST,
// og_rt_digest.h) goes into THEIR hashes alone.
//
// The reference's process(): output = current[playhead]; playhead += 1; playhead = 0 once it reaches len; an empty buffer
// gives F::default().  Here the buffer is a span of the pool (`Vec<F>`: frame-major, C floats per frame) and every voice
// holds its own buffer choice and playhead as two ordinary state words.
//
// Read path.  A voice reads consecutive frames in TIME; the lanes of a wave read unrelated addresses.  A load per frame
// would be 64 scattered dwords per wave instruction, each pulling its own cache line, with the latency inside the tick.
// So the frames are requested a chunk ahead, as the Delay stages its line (og::ring_chunk_begin): at the top of every
// OG_BUS_CHUNK-frame chunk a lane asks for the 16 frames its NEXT chunk will emit -- four 16-byte loads per channel when
// those frames do not wrap (every cache line it touches is used whole), a frame-by-frame walk when they do -- and takes
// over the ones it asked for a chunk ago.  The ticks read registers: the chunk's frames sit in cur[], a tick emits cur[0..C)
// and shifts the rest down (in the unrolled chunk body the shifts are register renames), so nothing in a tick indexes a
// register array by a run-time value.  Inside a launch the prediction is exact: a publish falls on a launch boundary, every
// chunk but a launch's last is full, and nothing else moves a playhead.
//
// The descriptor of a voice's buffer (offset into the pool, frames) is read once per launch (player_begin).
#pragma once

namespace og {

// 16 bytes from a dword-aligned address (a buffer starts anywhere in the pool), like og_rcp4
typedef float og_smp4 __attribute__((ext_vector_type(4), aligned(4)));
// the pool and the table are device allocations handed over as integers: the GLOBAL address space, so that the loads are
// global_load_* and not flat ones (the host simulator has one address space)
#ifndef OG_HOSTSIM
typedef __attribute__((address_space(1))) const float smp_f;
typedef __attribute__((address_space(1))) const og_smp4 smp_f4;
typedef __attribute__((address_space(1))) const uint32_t smp_u;
#else
typedef const float smp_f;
typedef const og_smp4 smp_f4;
typedef const uint32_t smp_u;
#endif

template <int C>
struct Player {
    smp_f* buf;       // the voice's buffer (null / len 0: unloaded or empty -> silence)
    uint32_t len;     // frames
    bool primed;      // wave-uniform: nxt[] holds the frames of the chunk that starts now
    float cur[OG_BUS_CHUNK * C];
    float nxt[OG_BUS_CHUNK * C];
};

// a 64-bit device address handed over in two slots (OgBlockArgs keeps its layout)
OG_DEV unsigned long long slot_addr(const OgBlockArgs& a, int i)
{
    return ((unsigned long long)scalar_u(a, i + 1) << 32) | (unsigned long long)scalar_u(a, i);
}

// slots s0 .. s0+4: pool address (2), descriptor table address (2), entries per player in the table.
// Table: [player][entry]{offset in floats, frames}; entries past the loaded samples hold {0, 0}.
template <int C>
OG_DEV void player_begin(const OgBlockArgs& a, int s0, uint32_t k, bool valid, uint32_t sample, uint32_t& playhead, Player<C>& P)
{
    smp_f* pool = (smp_f*)slot_addr(a, s0);
    smp_u* desc = (smp_u*)slot_addr(a, s0 + 2);
    const uint32_t cap = scalar_u(a, s0 + 4);
    P.buf = pool;
    P.len = 0u;
    if (valid && sample < cap) { // (OG_SAMPLE_NONE = 0xFFFFFFFF is past every table)
        smp_u* d = desc + 2u * ((size_t)k * cap + sample);
        P.buf = pool + d[0];
        P.len = d[1];
    }
    playhead = playhead < P.len ? playhead : 0u; // (a loaded state image cannot point past the buffer)
    P.primed = false;
}

// the OG_BUS_CHUNK frames from position p on, wrapping at len
template <int C>
OG_DEV void player_fetch(smp_f* buf, uint32_t len, uint32_t p, float (&dst)[OG_BUS_CHUNK * C])
{
    if (len == 0u) {
#pragma unroll
        for (uint32_t i = 0; i < OG_BUS_CHUNK * C; ++i) dst[i] = 0.0f;
    } else if (p + OG_BUS_CHUNK <= len) { // no wrap: OG_BUS_CHUNK * C consecutive floats
        smp_f* s = buf + (size_t)p * C;
#pragma unroll
        for (uint32_t g = 0; g < OG_BUS_CHUNK * C / 4; ++g) {
            const og_smp4 v = *(smp_f4*)(s + 4 * g);
            dst[4 * g] = v.x;
            dst[4 * g + 1] = v.y;
            dst[4 * g + 2] = v.z;
            dst[4 * g + 3] = v.w;
        }
    } else {
        uint32_t q = p;
#pragma unroll
        for (uint32_t j = 0; j < OG_BUS_CHUNK; ++j) {
#pragma unroll
            for (uint32_t c = 0; c < (uint32_t)C; ++c) dst[j * C + c] = buf[(size_t)q * C + c];
            q = (q + 1u >= len) ? 0u : q + 1u;
        }
    }
}

// top of a chunk: `more` (wave-uniform) = another chunk follows in this launch, and then this one is full
template <int C>
OG_DEV void player_chunk_begin(Player<C>& P, uint32_t playhead, bool more)
{
    if (P.primed) {
#pragma unroll
        for (uint32_t i = 0; i < OG_BUS_CHUNK * C; ++i) P.cur[i] = P.nxt[i];
    } else { // first chunk of a launch
        player_fetch<C>(P.buf, P.len, playhead, P.cur);
    }
    P.primed = more;
    if (more) {
        uint32_t p = playhead + OG_BUS_CHUNK; // playhead < len (or both 0)
        if (p >= P.len && P.len != 0u) {
            p -= P.len;
            if (p >= P.len) p %= P.len; // buffers shorter than a chunk
        }
        player_fetch<C>(P.buf, P.len, p, P.nxt);
    }
}

template <int C>
OG_DEV Frame<C> player_tick(Player<C>& P, uint32_t& playhead)
{
    Frame<C> out;
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)C; ++c) out.v[c] = P.cur[c];
#pragma unroll
    for (uint32_t i = 0; i + C < OG_BUS_CHUNK * C; ++i) P.cur[i] = P.cur[i + C];
    const uint32_t n = playhead + 1u;
    playhead = n < P.len ? n : 0u;
    return out;
}

} // namespace og
