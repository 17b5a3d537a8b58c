// og_node_array.hip.h -- per-voice ARRAY fields of registered node types (og_node_array, include/oscen_gpu.h): what a
// `buf: [f32; N]` field of a #[derive(Node)] struct is in the reference -- a delay line, a history, a table.  Included only
// by the kernels of graphs that hold such a field; its digest (OG_NARR_DIGEST, og_rt_digest.h) goes into THEIR hashes alone.
//
// Layout.  One device allocation per engine, the node-array pool: [array words per voice][n_voices] 32-bit words.  Element i
// of a field whose first plane is `base` lives, for voice slot v, at pool[(base + i) * n_voices + v] -- the Delay ring's
// convention: the 64 lanes of a wave that use the same index touch one 256-byte run, and a wave is the only one that ever
// touches its voices' columns (the ordinary kernel: one wave per 64 voices; graphs with array fields get no pipelined
// variants).  `base` is a compile-time constant of the generated kernel, one per (node instance, field).
//
// Addressing.  The pool's address reaches the kernel in two uniform slots the engine fills per launch (OgBlockArgs keeps
// its layout), as the sample pool's does; the pointer is in the GLOBAL address space, so the accesses are global_load /
// global_store and not flat ones.
//
// Semantics (documented for the node author in include/oscen_gpu.h):
//   * an index >= N is clamped to N - 1, reads and writes alike (one v_min_u32): whatever the user's source computes, an
//     access stays inside the voice's own planes;
//   * a lane beyond the bank's last voice touches nothing (get gives 0);
//   * get(i) after set(i, x) gives x: both go through the same plain pointer -- no __restrict__, no non-temporal hint -- so
//     the compiler keeps them in program order, and the memory pipeline returns a wave's accesses to one address in order
//     (DESIGN 4f records what the compiler emits between them).
#pragma once

namespace og {

#ifndef OG_HOSTSIM
typedef __attribute__((address_space(1))) uint32_t narr_word;
#else
typedef uint32_t narr_word; // (the host simulator has one address space)
#endif

// slots s0, s0 + 1: the pool's address
__device__ __forceinline__ narr_word* node_array_pool(const OgBlockArgs& a, int s0)
{
    return (narr_word*)(((unsigned long long)scalar_u(a, s0 + 1) << 32) | (unsigned long long)scalar_u(a, s0));
}

template <typename T>
struct NodeArrayElem;
template <>
struct NodeArrayElem<float> {
    static __device__ __forceinline__ uint32_t bits(float x) { return __float_as_uint(x); }
    static __device__ __forceinline__ float value(uint32_t w) { return __uint_as_float(w); }
};
template <>
struct NodeArrayElem<uint32_t> {
    static __device__ __forceinline__ uint32_t bits(uint32_t x) { return x; }
    static __device__ __forceinline__ uint32_t value(uint32_t w) { return w; }
};

template <typename T, uint32_t N>
struct NodeArray {
    static_assert(N >= 1u, "an array field has at least one element");
    narr_word* col;  // element 0 of this lane's voice
    uint32_t stride; // words between elements: n_voices
    bool valid;      // the lane holds a voice
    static constexpr uint32_t length() { return N; }
    __device__ __forceinline__ T get(uint32_t i) const
    {
        i = i < N ? i : N - 1u;
        uint32_t w = 0u;
        if (valid) w = col[(size_t)i * stride];
        return NodeArrayElem<T>::value(w);
    }
    __device__ __forceinline__ void set(uint32_t i, T x)
    {
        i = i < N ? i : N - 1u;
        if (valid) col[(size_t)i * stride] = NodeArrayElem<T>::bits(x);
    }
};

// the view of one field for this lane's voice; `base`: the field's first plane, in words per voice
template <typename T, uint32_t N>
__device__ __forceinline__ NodeArray<T, N> node_array(narr_word* pool, uint32_t base, uint32_t n_voices, uint32_t v, bool valid)
{
    NodeArray<T, N> a;
    a.col = pool + ((size_t)base * n_voices + (valid ? v : 0u));
    a.stride = n_voices;
    a.valid = valid;
    return a;
}

} // namespace og

#ifdef OG_NODE_ARRAY_FILL_KERNEL
// og_init: `bits` over the n words at p (the planes of one field).  One lane per word at the unaligned ends, one lane per
// 16 bytes in between.  grid x block >= max(3, ceil((n - head) / 4)) threads.
__global__ __launch_bounds__(256) void og_node_array_fill(uint32_t* p, size_t n, uint32_t bits)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t head = (size_t)((4u - (uint32_t)(((uintptr_t)p >> 2) & 3u)) & 3u); // words up to the first 16-byte boundary
    if (head > n) head = n;
    const size_t n4 = (n - head) / 4, tail0 = head + 4 * n4;
    if (i < head) p[i] = bits;
    if (i < n4) *reinterpret_cast<uint4*>(p + head + 4 * i) = make_uint4(bits, bits, bits, bits);
    if (i < n - tail0) p[tail0 + i] = bits;
}
#endif
