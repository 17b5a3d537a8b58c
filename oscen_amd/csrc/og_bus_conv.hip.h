// og_bus_conv.hip.h -- the post-mix Convolver (oscen-lib/src/convolution/mod.rs): y[t] = sum_k h[k] x[t-k] on the summed
// bus, zero latency, evaluated directly.  Included by og_engine.cpp only (it is no part of the voice kernels' runtime and
// so no part of OG_RT_DIGEST).
//
// The stage runs once per launched batch over all of its frames.  The input is a linear history buffer: the dry bus of
// this batch preceded by the samples of the batches before it (the host keeps at least K-1 of them in front).
//
//   og_bus_conv        grid (frame tile, tap segment, channel): workgroup (i, j, c) computes, for the OG_CONV_F frames of
//                      tile i, the products of taps [j S, (j+1) S) of channel c -- taps and the input window
//                      (OG_CONV_F + OG_CONV_S samples) staged in LDS, four consecutive frames per lane, accumulated with
//                      fmaf in registers in ASCENDING k -- and writes one partial row per segment.
//                      A response is either ONE tap plane shared by every channel (tap_stride == 0: the mono response of
//                      og_register_ir, or a one-channel asset) or one plane per channel, tap_stride floats apart (a
//                      multi-channel asset, MultiConvolverEngine::from_asset): workgroup (i, j, c) stages taps + c * tap_stride.
//                      The offset is uniform over the workgroup and paid once, in front of the staging loop.
//   og_bus_conv_finish sums the rows of a frame in a fixed order (four interleaved accumulators over the segment number,
//                      folded (a0 + a1) + (a2 + a3)), applies the equal-power crossfade of a live response swap and writes
//                      the wet bus.
//
// No atomics.  The order in which the K products of an output sample are summed depends on k alone -- not on where the
// sample falls in a tile, a block or a batch: a frame's window holds the same samples wherever the tile starts, taps
// beyond the response are zeros in LDS (fmaf(0, x, acc) == acc), and samples in front of a response's "history valid
// from" frame are read as zeros.  So the output is bit-identical however the same frames are cut into blocks and batches.
//
// Sizes (MI355X: 256 CUs, 64-lane waves, 64 LDS banks of 4 bytes, 160 KiB LDS per CU):
//   OG_CONV_S = 256 taps per segment, OG_CONV_F = 256 frames per tile, one wave per workgroup, 4 frames per lane.
//   * a single 256-frame block at 72 000 taps is 282 workgroups -- one wave on every CU -- each with 256 x 256
//     multiply-adds: 1 024 v_fma per lane behind 64 LDS reads; S = 512 would leave 115 CUs idle for that block, S = 128
//     doubles the partial rows (K / S rows of 4 bytes per frame and channel) for no shorter critical path than the launch.
//   * a lane's four frames are consecutive, so the eight window samples it needs for four taps are two aligned float4:
//     one ds_read_b128 per four taps (16 fmaf), lanes 16 bytes apart -- conflict-free; the four taps are one broadcast
//     ds_read_b128.  (One frame per lane would need one LDS read per fmaf.)
//   * 3 KiB of LDS and ~40 VGPRs per workgroup: occupancy is bounded by the number of workgroups, never by resources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "og_bus_conv_host.h" // OG_CONV_S, OG_CONV_F, OG_CONV_LANES, OG_CONV_MAX_TAPS, OgConvResponse
#include "og_math.h"

// x: interleaved history, pointing at the run's first frame; sample (f, c) = x[f * channels + c], f may be negative down to r.lo
__global__ __launch_bounds__(OG_CONV_LANES) void og_bus_conv(const float* __restrict__ x, uint32_t channels, OgConvResponse r, uint32_t row_stride)
{
    __shared__ float4 win[(OG_CONV_F + OG_CONV_S) / 4];
    __shared__ float4 tap[OG_CONV_S / 4];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.z;
    const int32_t tile0 = (int32_t)(blockIdx.x * OG_CONV_F);
    const uint32_t k0 = blockIdx.y * OG_CONV_S;
    // window sample j = frame tile0 - k0 - OG_CONV_S + j  (frame f, tap k0 + d: j = f - tile0 - d + OG_CONV_S)
    const int32_t w0 = tile0 - (int32_t)k0 - OG_CONV_S;
    float* wf = reinterpret_cast<float*>(win);
    float* tf = reinterpret_cast<float*>(tap);
    for (uint32_t j = lane; j < OG_CONV_F + OG_CONV_S; j += OG_CONV_LANES) {
        const int32_t f = w0 + (int32_t)j;
        wf[j] = (f >= r.lo && f < (int32_t)r.n_frames) ? x[(int64_t)f * (int64_t)channels + c] : 0.0f;
    }
    const float* __restrict__ taps = r.taps + (size_t)c * r.tap_stride;
    for (uint32_t j = lane; j < OG_CONV_S; j += OG_CONV_LANES) tf[j] = (k0 + j < r.n_taps) ? taps[k0 + j] : 0.0f;
    __syncthreads();
    const uint32_t seg_taps = min((uint32_t)OG_CONV_S, r.n_taps - k0);
    float y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, y3 = 0.0f;
    // a = window samples [4 lane + S - 4 - d0, +8) for the four taps d0 .. d0 + 3: frame 4 lane + q, tap d0 + d reads a[q - d + 4]
    float4 hi = win[lane + OG_CONV_S / 4];
    for (uint32_t d0 = 0; d0 < seg_taps; d0 += 4) {
        const float4 lo = win[lane + OG_CONV_S / 4 - 1 - d0 / 4];
        const float4 h = tap[d0 / 4];
        y0 = fmaf(h.x, hi.x, y0);
        y1 = fmaf(h.x, hi.y, y1);
        y2 = fmaf(h.x, hi.z, y2);
        y3 = fmaf(h.x, hi.w, y3);
        y0 = fmaf(h.y, lo.w, y0);
        y1 = fmaf(h.y, hi.x, y1);
        y2 = fmaf(h.y, hi.y, y2);
        y3 = fmaf(h.y, hi.z, y3);
        y0 = fmaf(h.z, lo.z, y0);
        y1 = fmaf(h.z, lo.w, y1);
        y2 = fmaf(h.z, hi.x, y2);
        y3 = fmaf(h.z, hi.y, y3);
        y0 = fmaf(h.w, lo.y, y0);
        y1 = fmaf(h.w, lo.z, y1);
        y2 = fmaf(h.w, lo.w, y2);
        y3 = fmaf(h.w, hi.x, y3);
        hi = lo;
    }
    const uint32_t f = (uint32_t)tile0 + 4 * lane;
    float* row = r.rows + ((size_t)blockIdx.y * channels + c) * row_stride;
    if (f + 3 < r.n_frames) {
        *reinterpret_cast<float4*>(row + f) = make_float4(y0, y1, y2, y3); // (row_stride and the tile are multiples of 4)
    } else {
        if (f < r.n_frames) row[f] = y0;
        if (f + 1 < r.n_frames) row[f + 1] = y1;
        if (f + 2 < r.n_frames) row[f + 2] = y2;
    }
}

__device__ __forceinline__ float og_conv_row_sum(const float* __restrict__ rows, uint32_t n_rows, size_t stride)
{
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    uint32_t j = 0;
    for (; j + 3 < n_rows; j += 4) {
        a0 += rows[(size_t)j * stride];
        a1 += rows[(size_t)(j + 1) * stride];
        a2 += rows[(size_t)(j + 2) * stride];
        a3 += rows[(size_t)(j + 3) * stride];
    }
    if (j < n_rows) a0 += rows[(size_t)j * stride];
    if (j + 1 < n_rows) a1 += rows[(size_t)(j + 1) * stride];
    if (j + 2 < n_rows) a2 += rows[(size_t)(j + 2) * stride];
    return (a0 + a1) + (a2 + a3);
}

// out[f * channels + c] = current response, crossfaded with the fading-out one while f < old.n_frames:
// g = pos / fade_len, new sin(g pi/2) + old cos(g pi/2)  (convolution/mod.rs:553-571); fade_pos0 = pos at the run's frame 0
__global__ __launch_bounds__(256) void og_bus_conv_finish(OgConvResponse cur, OgConvResponse old, uint32_t channels, uint32_t row_stride,
                                                          uint32_t fade_pos0, uint32_t fade_len, float* __restrict__ out)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t c = blockIdx.y;
    if (f >= cur.n_frames) return;
    const size_t seg_stride = (size_t)channels * row_stride;
    float y = og_conv_row_sum(cur.rows + (size_t)c * row_stride + f, (cur.n_taps + OG_CONV_S - 1) / OG_CONV_S, seg_stride);
    if (f < old.n_frames) {
        const float o = og_conv_row_sum(old.rows + (size_t)c * row_stride + f, (old.n_taps + OG_CONV_S - 1) / OG_CONV_S, seg_stride);
        const float g = (float)(fade_pos0 + f) / (float)fade_len;
        const float gain_new = og_sinf_exact(g * 1.57079637050628662f);
        const float gain_old = og_cosf_exact(g * 1.57079637050628662f);
        y = y * gain_new + o * gain_old;
    }
    out[(size_t)f * channels + c] = y;
}

// og_set_bus_ir on an asset response: the conformed frames [n_taps][src_ch] (interleaved) -> tap planes [gridDim.y][n_taps],
// with the channel mapping of MultiConvolverEngine::from_asset (convolution/mod.rs:335-351).  downmix (a multi-channel
// response on a mono bus, AudioAsset::to_mono, asset/mod.rs:115-131): channels 0, 1, .. added in that order into 0.0f, then
// times inv = 1.0f / src_ch (formed on the host) -- that order in f32 is the contract.  Otherwise plane p takes source
// channel min(p, src_ch - 1).
OG_HD float og_bus_ir_tap(const float* __restrict__ frame, uint32_t src_ch, uint32_t p, uint32_t downmix, float inv)
{
    if (downmix) {
        float acc = 0.0f;
        for (uint32_t c = 0; c < src_ch; ++c) acc += frame[c];
        return acc * inv;
    }
    return frame[p < src_ch - 1u ? p : src_ch - 1u];
}

// one lane per tap of a plane
__global__ __launch_bounds__(256) void og_bus_ir_planes(const float* __restrict__ conformed, uint32_t n_taps, uint32_t src_ch, uint32_t downmix,
                                                        float inv, float* __restrict__ dst)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p = blockIdx.y;
    if (k >= n_taps) return;
    dst[(size_t)p * n_taps + k] = og_bus_ir_tap(conformed + (size_t)k * src_ch, src_ch, p, downmix, inv);
}

// history upkeep: dst[i] = src[i] (the newest samples moved to the front of the buffer; the ranges never overlap)
__global__ __launch_bounds__(256) void og_bus_conv_move(const float* __restrict__ src, float* __restrict__ dst, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
