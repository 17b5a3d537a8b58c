// og_post_mix.hip.h -- the run-time pieces of a post-mix kernel (og_kp_<hash>_{00,10}; og_graph.cpp, write_post_kernel): the
// wrapper-level nodes behind the voice sum, compiled as a graph of ONE voice whose stream input is that sum.  Included only by
// post-mix units; its digest (OG_PM_DIGEST, og_rt_digest.h) goes into THEIR hashes alone.
//
// The kernel is one wave and lane 0 is the voice: the recurrence is serial in time (a filter state, a delay line, a
// limiter's envelope), so its cost is the latency of one frame's dependent chain times the frames of the launch, and the
// frame around the ticks keeps memory out of that chain:
//   input    og_bus_reduce's last pass writes the voice sum planar -- one row of `stride` frames per channel -- and the
//            kernel reads a chunk's 16 frames per channel with four 16-byte loads from a uniform address, issued a whole
//            chunk before the ticks that use them (post_fetch_ahead), as og_sample_player.hip.h stages its frames.  A tick
//            reads registers; nothing in it waits for a load of its own.
//   output   a chunk's frames are collected in registers and leave as 16-byte stores of interleaved frames, straight into
//            the destination of the launch (the caller's buffer, or the staging bus when the queued blocks' destinations
//            are not contiguous).  No tile, no partial rows, no second reduce.
//   pointers two 64-bit device addresses and the row stride, handed over in five uniform slots: OgBlockArgs keeps its layout.
// A launch's last chunk may be partial: its frames are read and written one by one (post_in<false>, post_store1).
#pragma once

namespace og {

// 16 bytes from / to a dword-aligned address: a destination is any float pointer the caller gave plus whole frames
typedef float og_pm4 __attribute__((ext_vector_type(4), aligned(4)));
#ifndef OG_HOSTSIM
typedef __attribute__((address_space(1))) const float pm_cf;
typedef __attribute__((address_space(1))) const og_pm4 pm_cf4;
typedef __attribute__((address_space(1))) float pm_f;
typedef __attribute__((address_space(1))) og_pm4 pm_f4;
#else
typedef const float pm_cf;
typedef const og_pm4 pm_cf4;
typedef float pm_f;
typedef og_pm4 pm_f4;
#endif

struct PostIo {
    pm_cf* in;       // [channels of the sum][stride]: the voice sum of this launch, planar; rows padded to whole chunks
    pm_f* out;       // [frames][channels of the bus], interleaved
    uint32_t stride; // frames between the rows of `in`
};

__device__ __forceinline__ unsigned long long post_addr(const OgBlockArgs& a, int i)
{
    return ((unsigned long long)scalar_u(a, i + 1) << 32) | (unsigned long long)scalar_u(a, i);
}
// slots s0 .. s0+4: input rows (2), destination (2), row stride in frames
__device__ __forceinline__ PostIo post_io(const OgBlockArgs& a, int s0)
{
    PostIo io;
    io.in = (pm_cf*)post_addr(a, s0);
    io.out = (pm_f*)post_addr(a, s0 + 2);
    io.stride = scalar_u(a, s0 + 4);
    return io;
}

// the OG_BUS_CHUNK frames from `base` (a multiple of the chunk) of every input channel
template <int C>
__device__ __forceinline__ void post_fetch(float (&dst)[C][OG_BUS_CHUNK], const PostIo& io, const uint32_t base)
{
#pragma unroll
    for (int k = 0; k < C; ++k) {
        pm_cf* s = io.in + (size_t)k * io.stride + base;
#pragma unroll
        for (uint32_t g = 0; g < OG_BUS_CHUNK / 4; ++g) {
            const og_pm4 v = *(pm_cf4*)(s + 4 * g);
            dst[k][4 * g] = v.x;
            dst[k][4 * g + 1] = v.y;
            dst[k][4 * g + 2] = v.z;
            dst[k][4 * g + 3] = v.w;
        }
    }
}
// ... of the NEXT chunk, asked for at the top of this one (a uniform branch: the launch's last chunk asks for nothing)
template <int C>
__device__ __forceinline__ void post_fetch_ahead(float (&dst)[C][OG_BUS_CHUNK], const PostIo& io, const uint32_t next_base, const uint32_t frames)
{
    if (next_base < frames) {
        post_fetch(dst, io, next_base);
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k)
#pragma unroll
            for (uint32_t j = 0; j < OG_BUS_CHUNK; ++j) dst[k][j] = 0.0f;
    }
}
template <int C>
__device__ __forceinline__ void post_take(float (&cur)[C][OG_BUS_CHUNK], const float (&next)[C][OG_BUS_CHUNK])
{
#pragma unroll
    for (int k = 0; k < C; ++k)
#pragma unroll
        for (uint32_t j = 0; j < OG_BUS_CHUNK; ++j) cur[k][j] = next[k][j];
}

// one input sample: from the chunk's registers in the straight-line chunk body (STAGED: j is a constant once the body is
// unrolled), from memory in a partial chunk
template <bool STAGED, int C>
__device__ __forceinline__ float post_in(const float (&cur)[C][OG_BUS_CHUNK], const int k, const uint32_t j, const PostIo& io, const uint32_t f)
{
    if constexpr (STAGED) return cur[k][j];
    else return io.in[(size_t)k * io.stride + f];
}

// a chunk's output frames, interleaved: lane 0 holds the voice
__device__ __forceinline__ void post_store(const PostIo& io, const VoiceCtx& c, const uint32_t base, const float (&o)[OG_BUS_CHUNK])
{
    if (c.lane != 0u) return;
    pm_f* d = io.out + (size_t)base;
#pragma unroll
    for (uint32_t g = 0; g < OG_BUS_CHUNK / 4; ++g) *(pm_f4*)(d + 4 * g) = og_pm4{o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
}
template <int N>
__device__ __forceinline__ void post_store(const PostIo& io, const VoiceCtx& c, const uint32_t base, const OutN<N> (&o)[OG_BUS_CHUNK])
{
    if (c.lane != 0u) return;
    pm_f* d = io.out + (size_t)base * N;
    float flat[OG_BUS_CHUNK * N];
#pragma unroll
    for (uint32_t j = 0; j < OG_BUS_CHUNK; ++j)
#pragma unroll
        for (int k = 0; k < N; ++k) flat[j * N + k] = o[j].v[k];
#pragma unroll
    for (uint32_t g = 0; g < OG_BUS_CHUNK * N / 4; ++g) *(pm_f4*)(d + 4 * g) = og_pm4{flat[4 * g], flat[4 * g + 1], flat[4 * g + 2], flat[4 * g + 3]};
}
__device__ __forceinline__ void post_store1(const PostIo& io, const VoiceCtx& c, const uint32_t f, const float o)
{
    if (c.lane == 0u) io.out[f] = o;
}
template <int N>
__device__ __forceinline__ void post_store1(const PostIo& io, const VoiceCtx& c, const uint32_t f, const OutN<N> o)
{
    if (c.lane != 0u) return;
#pragma unroll
    for (int k = 0; k < N; ++k) io.out[(size_t)f * N + k] = o.v[k];
}

} // namespace og
