// og_asset_resample.hip.h -- conforming a sample to the graph rate on load: the reference's offline windowed sinc
// (oscen-lib/src/asset/resample.rs:47-103, `resample_channel`) as a device kernel, and the channel mapping of
// SamplePlayerConsumer::build from the conformed frames into the engine's sample pool.
//
// Included by og_engine.cpp ONLY: no voice kernel sees it, so it is in none of the digests that name the voice kernels.
//
// One lane per OUTPUT FRAME, 256 lanes per workgroup.  Lane n walks its taps first..last in ascending order, exactly as the
// reference's loop does, and sums in f32 in that order: the result is the reference's, bit for bit.  The weight of tap i
// depends on (n, i) alone, so the lane computes it ONCE for all channels of its frame and keeps one accumulator per channel --
// the bits of the reference's channel-by-channel loop (from_samples, asset/mod.rs:207-221) at 1/channels of the sine/cosine
// work.  Weights are not tabulated per polyphase: `pos` is an f64 product and `dist` the f32 rounding of an f64 difference, so
// the weights of two outputs with the same fractional position are NOT the same bits.
//
// Sine and cosine are og_sinf_exact / og_cosf_exact (og_math.h: glibc's bits, |x| < 120): the sinc argument is at most
// 32 pi ~ 100.6 (cutoff * dist <= cutoff * radius = 32), the window's at most 2 pi.  Everything else is plain IEEE f32 / f64
// under -ffp-contract=off; f32 division is correctly rounded on host and device.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "og_math.h"

#define OG_RESAMPLE_ZERO_CROSSINGS 32
#define OG_RESAMPLE_BLOCK 256
#define OG_RESAMPLE_MAX_CHANNELS 8

// the scalars of one resample, formed on the host exactly as resample.rs:56-71 forms them
struct OgResamplePlan {
    uint64_t out_len;   // round(len * ratio), half away from zero
    double inv_ratio;   // output index -> input position
    float cutoff;       // min(ratio, 1)
    float radius;       // kernel half-width in input samples: 32 / cutoff
    float inv_radius;
};

static inline OgResamplePlan og_resample_plan(uint64_t len, uint32_t src_rate, uint32_t dst_rate)
{
    OgResamplePlan p;
    const double ratio = (double)dst_rate / (double)src_rate;
    p.out_len = (uint64_t)round((double)len * ratio);
    const double cut = ratio < 1.0 ? ratio : 1.0;
    p.cutoff = (float)cut;
    p.radius = (float)OG_RESAMPLE_ZERO_CROSSINGS / p.cutoff;
    p.inv_ratio = 1.0 / ratio;
    p.inv_radius = 1.0f / p.radius;
    return p;
}

// resample.rs:18-25
OG_HD float og_resample_sinc(float x)
{
    if (x == 0.0f) return 1.0f;
    const float pix = 3.14159274101257324f * x;
    return og_sinf_exact(pix) / pix;
}

// resample.rs:29-39
OG_HD float og_resample_blackman(float t)
{
    if (fabsf(t) > 1.0f) return 0.0f;
    const float phase = 3.14159274101257324f * (t + 1.0f);
    const float c = og_cosf_exact(phase);
    return 0.42f - 0.5f * c + 0.08f * (2.0f * c * c - 1.0f);
}

// Output frame n of all `channels` channels (CH = 1, 2: exactly that many; CH = 8: 1..8, the accumulators beyond `channels`
// stay 0 and are never stored).  src / dst are interleaved; len >= 1; n < out_len is the caller's check.
template <int CH>
OG_HD void og_resample_frame(const float* __restrict__ src, uint64_t len, uint32_t channels, uint64_t n, double inv_ratio, float cutoff,
                             float radius, float inv_radius, float* __restrict__ dst)
{
    const double pos = (double)n * inv_ratio;
    int64_t first = (int64_t)ceil(pos - (double)radius);
    if (first < 0) first = 0;
    int64_t last = (int64_t)floor(pos + (double)radius);
    if (last > (int64_t)len - 1) last = (int64_t)len - 1;
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
    float weight_sum = 0.0f;
    for (int64_t i = first; i <= last; ++i) {
        const float dist = (float)(pos - (double)i);
        const float w = og_resample_sinc(cutoff * dist) * og_resample_blackman(dist * inv_radius);
        const float* __restrict__ frame = src + (size_t)i * channels;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (CH <= 2 || (uint32_t)c < channels) acc[c] += w * frame[c];
        weight_sum += w;
    }
    float* __restrict__ out = dst + (size_t)n * channels;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (CH <= 2 || (uint32_t)c < channels) out[c] = weight_sum != 0.0f ? acc[c] / weight_sum : 0.0f;
}

template <int CH>
__global__ __launch_bounds__(OG_RESAMPLE_BLOCK) void og_asset_resample(const float* __restrict__ src, uint64_t len, uint32_t channels,
                                                                       uint64_t out_len, double inv_ratio, float cutoff, float radius,
                                                                       float inv_radius, float* __restrict__ dst)
{
    const uint64_t n = (uint64_t)blockIdx.x * OG_RESAMPLE_BLOCK + threadIdx.x;
    if (n >= out_len) return;
    og_resample_frame<CH>(src, len, channels, n, inv_ratio, cutoff, radius, inv_radius, dst);
}

// SamplePlayerConsumer::build (sample_player/mod.rs:38-50) on the device: conformed frames of `channels` channels onto a player
// of `width` channels, frame-major -- one source channel broadcasts, otherwise target channel c takes source channel
// min(c, channels - 1).  One lane per float of the destination.
__global__ __launch_bounds__(OG_RESAMPLE_BLOCK) void og_asset_map_channels(const float* __restrict__ conformed, uint64_t frames,
                                                                           uint32_t channels, uint32_t width, float* __restrict__ dst)
{
    const uint64_t k = (uint64_t)blockIdx.x * OG_RESAMPLE_BLOCK + threadIdx.x;
    if (k >= frames * width) return;
    const uint64_t t = k / width;
    const uint32_t c = (uint32_t)(k % width);
    const uint32_t sc = channels == 1 ? 0u : (c < channels - 1u ? c : channels - 1u);
    dst[k] = conformed[t * channels + sc];
}

// `src` (len frames, interleaved, on the device) -> `dst` (plan.out_len frames), in stream order.  len >= 1, 1..8 channels,
// plan.out_len >= 1 and below 2^32 frames are the caller's checks.
static inline void og_resample_launch(const float* src, uint64_t len, uint32_t channels, const OgResamplePlan& p, float* dst, hipStream_t stream)
{
    const unsigned grid = (unsigned)((p.out_len + OG_RESAMPLE_BLOCK - 1) / OG_RESAMPLE_BLOCK);
    if (channels == 1)
        hipLaunchKernelGGL(og_asset_resample<1>, dim3(grid), dim3(OG_RESAMPLE_BLOCK), 0, stream, src, len, channels, p.out_len, p.inv_ratio,
                           p.cutoff, p.radius, p.inv_radius, dst);
    else if (channels == 2)
        hipLaunchKernelGGL(og_asset_resample<2>, dim3(grid), dim3(OG_RESAMPLE_BLOCK), 0, stream, src, len, channels, p.out_len, p.inv_ratio,
                           p.cutoff, p.radius, p.inv_radius, dst);
    else
        hipLaunchKernelGGL(og_asset_resample<OG_RESAMPLE_MAX_CHANNELS>, dim3(grid), dim3(OG_RESAMPLE_BLOCK), 0, stream, src, len, channels,
                           p.out_len, p.inv_ratio, p.cutoff, p.radius, p.inv_radius, dst);
}

static inline void og_map_channels_launch(const float* conformed, uint64_t frames, uint32_t channels, uint32_t width, float* dst, hipStream_t stream)
{
    const unsigned grid = (unsigned)((frames * width + OG_RESAMPLE_BLOCK - 1) / OG_RESAMPLE_BLOCK);
    hipLaunchKernelGGL(og_asset_map_channels, dim3(grid), dim3(OG_RESAMPLE_BLOCK), 0, stream, conformed, frames, channels, width, dst);
}
