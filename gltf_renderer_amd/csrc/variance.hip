// variance.hip -- the variance AOV outside the wavefront pipeline: pt_set_variance, which checks and keeps the config, and
// pt_noise_estimate: how noisy an accumulated image is, tile by tile, from the image and the variance target of pt_set_variance
// (include/mipt.h states it operation by operation; tests/variance_ref.py restates it in numpy float32).  A pure function
// of two images and the tiles' sample counts.  One launch on the context's stream, over 16 x 16 tiles (PT_TILE) numbered row-major:
//   k_noise_tiles     one 256-lane workgroup per tile, one lane per pixel.  A tile whose count is below 2 writes (-1, -1) and leaves
//                     (block-uniform).  Otherwise every in-image lane forms its pixel's relative standard error e; the tile's max and sum are
//                     reduced per wave64 by cross-lane swaps and the four waves combined through LDS (resolve_adaptive's reduction of E).
//                     Lanes off the image carry -infinity into the max and 0 into the sum; the mean divides by the in-image pixel count.
// The variance pass itself (k_wf_variance_resolve) reads the wavefront workspace and lives with the other pass resolves in wf_passes.hip.
// Compiled without floating-point contraction (Makefile), with IEEE division and square root.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pt_ctx.h"

namespace pt {
namespace {

constexpr int kNoiseTile = PT_TILE, kNoiseLanes = PT_TILE * PT_TILE;
static_assert(kNoiseLanes == 256, "k_noise_tiles reduces four waves of 64");

__global__ __launch_bounds__(kNoiseLanes) void k_noise_tiles(const float4* __restrict__ image, const float4* __restrict__ variance, uint32_t w, uint32_t h, uint32_t tiles_x,
                                                             const uint32_t* __restrict__ counts, uint32_t samples, float2* __restrict__ out) {
    __shared__ float s_max[kNoiseLanes / 64], s_sum[kNoiseLanes / 64];
    const uint32_t t = blockIdx.x, ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint32_t n = counts ? counts[t] : samples;                  // a uniform address: a scalar load
    if (n < 2u) {                                                     // (block-uniform) not estimated
        if (threadIdx.x == 0) out[t] = make_float2(-1.0f, -1.0f);
        return;
    }
    const uint32_t i = threadIdx.x;
    const uint32_t x = tx * kNoiseTile + (i & (kNoiseTile - 1)), y = ty * kNoiseTile + i / kNoiseTile;
    float emax = -INFINITY, esum = 0.0f;
    if (x < w && y < h) {
        const size_t p = (size_t)y * w + x;
        const float4 I = image[p], V = variance[p];
        const float s = (I.x + I.y) + I.z;
        float e = sqrtf(V.w / (float)(n - 1u)) / (1e-4f + sqrtf(fmaxf(s, 0.0f)));
        e = e != e ? INFINITY : e;
        emax = e; esum = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        emax = fmaxf(emax, __shfl_xor(emax, o, 64));
        esum = esum + __shfl_xor(esum, o, 64);
    }
    if ((i & 63u) == 0) { s_max[i >> 6] = emax; s_sum[i >> 6] = esum; }
    __syncthreads();
    if (i == 0) {
        const uint32_t cw = w - tx * kNoiseTile < (uint32_t)kNoiseTile ? w - tx * kNoiseTile : (uint32_t)kNoiseTile;
        const uint32_t ch = h - ty * kNoiseTile < (uint32_t)kNoiseTile ? h - ty * kNoiseTile : (uint32_t)kNoiseTile;
        const float M = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        const float S = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        out[t] = make_float2(S / (float)(cw * ch), M);
    }
}

}  // namespace

void launch_noise_tiles(const float4* image, const float4* variance, uint32_t w, uint32_t h, const uint32_t* counts, uint32_t samples, float2* out, hipStream_t stream) {
    const uint32_t tiles_x = (w + PT_TILE - 1) / PT_TILE, tiles_y = (h + PT_TILE - 1) / PT_TILE;
    hipLaunchKernelGGL(k_noise_tiles, dim3(tiles_x * tiles_y), dim3(kNoiseLanes), 0, stream, image, variance, w, h, tiles_x, counts, samples, out);
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_set_variance(pt_ctx* ctx, const pt_variance_config* config) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!config) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "variance: config is NULL");
    if (config->enable && !config->variance) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "variance: the target is NULL");
    ctx->variance = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_noise_estimate(pt_ctx* ctx, const void* image, const void* variance, uint32_t width, uint32_t height, const uint32_t* tile_samples, uint32_t samples,
                      float threshold, float* tile_mean_host, float* tile_max_host, pt_noise_summary* summary) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!image || !variance) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "noise_estimate: null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "noise_estimate: bad size");
    const uint64_t tiles_x = (width + PT_TILE - 1) / PT_TILE, tiles_y = (height + PT_TILE - 1) / PT_TILE, tiles = tiles_x * tiles_y;
    if (tiles > 0x7fffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "noise_estimate: more than 2^31 - 1 tiles");
    if (!std::isfinite(threshold) || threshold < 0.0f) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "noise_estimate: threshold must be finite and >= 0");
    if (!tile_samples && samples < 2u) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "noise_estimate: samples < 2 (a single sample has no variance)");
    ENTER(ctx);
    // the scratch: (mean, max) per tile, then the tiles' counts; for this tile count alone
    const size_t need = (size_t)tiles * (sizeof(float2) + sizeof(uint32_t));
    if (const int rc = exact_scratch(ctx, ctx->d_noise, need, "noise_estimate")) return rc;
    float2* d_out = ctx->d_noise.as<float2>();
    uint32_t* d_counts = tile_samples ? (uint32_t*)(d_out + tiles) : nullptr;
    // the caller's counts stay valid until this call returns, and it returns behind the stream
    if (d_counts) HIPOK(hipMemcpyAsync(d_counts, tile_samples, (size_t)tiles * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    launch_noise_tiles((const float4*)image, (const float4*)variance, width, height, d_counts, samples, d_out, ctx->stream);
    HIPOK(hipGetLastError());
    std::vector<float2> pairs((size_t)tiles);
    HIPOK(hipMemcpyAsync(pairs.data(), d_out, (size_t)tiles * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    HIPOK(hipStreamSynchronize(ctx->stream));
    // the summary: in double from the float32 tile values, each field rounded once
    pt_noise_summary sum = {(uint32_t)tiles, 0u, 0u, -1.0f, -1.0f};
    double weighted = 0.0, pixels = 0.0, top = -1.0;
    for (uint64_t t = 0; t < tiles; t++) {
        const uint32_t n = tile_samples ? tile_samples[t] : samples;
        if (n < 2u) continue;
        const uint64_t ty = t / tiles_x, tx = t - ty * tiles_x;
        const uint64_t cw = std::min<uint64_t>(PT_TILE, width - tx * PT_TILE), ch = std::min<uint64_t>(PT_TILE, height - ty * PT_TILE);
        sum.tiles_estimated++;
        if (pairs[t].y > threshold) sum.tiles_above++;
        weighted += (double)pairs[t].x * (double)(cw * ch);
        pixels += (double)(cw * ch);
        top = std::max(top, (double)pairs[t].y);
    }
    if (sum.tiles_estimated) { sum.mean = (float)(weighted / pixels); sum.max = (float)top; }
    for (uint64_t t = 0; t < tiles; t++) {
        if (tile_mean_host) tile_mean_host[t] = pairs[t].x;
        if (tile_max_host) tile_max_host[t] = pairs[t].y;
    }
    if (summary) *summary = sum;
    return PT_OK;
}

}  // extern "C"
