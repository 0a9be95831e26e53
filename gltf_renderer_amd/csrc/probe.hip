// probe.hip -- light-probe baking (include/mipt.h): pt_set_probes, which checks the config and keeps it with the probes' positions on the
// device (what a call makes of them -- probe_atlas_size, probe_args -- is inline in pt_ctx.h, for select_passes and a hook read it too), and
// pt_probe_project's reduction of the octahedral atlas to nine spherical-harmonic coefficients per channel and probe.
//
//   c[lm][ch] = (4 pi / n^2) * sum over the probe's n x n texels of L(i, j)[ch] * Y_lm(w(i, j))
//
// The map is equal-area, so every texel weighs the same and the quadrature is a midpoint rule over the texel centres w(i, j).  Those n^2
// directions are the same for every probe: k_probe_dirs builds them once per resolution into a table of the context (one pt_sincos per texel,
// not per probe and texel), and k_probe_project streams table and atlas side by side.
//   k_probe_project  one 256-lane workgroup per probe.  Lane t takes texels t, t + 256, ... of the map in row-major order: n is a multiple of
//                    16, so 16 consecutive lanes read 256 contiguous bytes of an atlas row (float4 loads) and the whole table row.  27 partial
//                    sums per lane (9 coefficients x rgb), reduced over the wave by shuffles, over the four waves through LDS.
// Compiled without floating-point contraction (Makefile): products and sums are the float32 operations tests/probe_ref.py bounds.
#include <cmath>

#include "pt_ctx.h"
#include "pt_probe.h"

namespace pt {
namespace {

constexpr int kProjBlock = 256;
constexpr int kProjSums = kProbeSh * 3;

__global__ __launch_bounds__(256) void k_probe_dirs(float4* __restrict__ dirs, uint32_t n) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n * n) return;
    const uint32_t j = t / n, i = t - j * n;
    const float fn = (float)n;
    const vec3 w = probe_direction(fdiv((float)i + 0.5f, fn), fdiv((float)j + 0.5f, fn));
    dirs[t] = make_float4(w.x, w.y, w.z, 0.0f);
}

__global__ __launch_bounds__(kProjBlock) void k_probe_project(const float4* __restrict__ atlas, const float4* __restrict__ dirs, uint32_t n, uint32_t columns,
                                                              uint32_t atlas_w, float scale, float band1, float band2, float band3, float* __restrict__ sh) {
    __shared__ float part[kProjBlock / 64][kProjSums];
    const uint32_t k = blockIdx.x;
    const uint32_t cy = k / columns, cx = k - cy * columns;
    const float4* __restrict__ base = atlas + ((size_t)cy * n) * atlas_w + (size_t)cx * n;
    float acc[kProjSums];
#pragma unroll
    for (int s = 0; s < kProjSums; s++) acc[s] = 0.0f;
    const uint32_t texels = n * n;
    for (uint32_t t = threadIdx.x; t < texels; t += kProjBlock) {
        const uint32_t j = t / n, i = t - j * n;
        float4 L = base[(size_t)j * atlas_w + i];
        const float4 w = dirs[t];
        if (!(isfinite(L.x) && isfinite(L.y) && isfinite(L.z))) L = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // a non-finite texel counts as 0
        float Y[kProbeSh];
        probe_sh_basis(v3(w.x, w.y, w.z), Y);
#pragma unroll
        for (int c = 0; c < kProbeSh; c++) {
            acc[3 * c + 0] = acc[3 * c + 0] + L.x * Y[c];
            acc[3 * c + 1] = acc[3 * c + 1] + L.y * Y[c];
            acc[3 * c + 2] = acc[3 * c + 2] + L.z * Y[c];
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < kProjSums; s++) {
        float v = acc[s];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
        if (lane == 0) part[wave][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < kProjSums) {
        const uint32_t s = threadIdx.x, c = s / 3;
        const float sum = ((part[0][s] + part[1][s]) + part[2][s]) + part[3][s];
        const float band = c == 0 ? band1 : (c < 4 ? band2 : band3);
        sh[(size_t)k * kProjSums + s] = (sum * scale) * band;
    }
}

}  // namespace

void launch_probe_dirs(float4* dirs, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_dirs, dim3((n * n + 255) / 256), dim3(256), 0, stream, dirs, n);
}

void launch_probe_project(const float4* atlas, const float4* dirs, uint32_t n, uint32_t count, uint32_t columns, int kind, float* sh, hipStream_t stream) {
    const float scale = (float)(4.0 * 3.14159265358979323846 / ((double)n * (double)n));
    const double pi = 3.14159265358979323846;
    const bool irradiance = kind == PT_PROBE_SH_IRRADIANCE;
    const float b1 = irradiance ? (float)pi : 1.0f, b2 = irradiance ? (float)(2.0 * pi / 3.0) : 1.0f, b3 = irradiance ? (float)(pi / 4.0) : 1.0f;
    hipLaunchKernelGGL(k_probe_project, dim3(count), dim3(kProjBlock), 0, stream, atlas, dirs, n, columns, columns * n, scale, b1, b2, b3, sh);
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_set_probes(pt_ctx* ctx, const pt_probe_config* config, const float* positions_xyz) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!config) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: config is NULL");
    if (!config->enable) {                        // nothing else of a disabled config is looked at; the layout and the positions go
        ctx->probes.enable = 0;
        ctx->restart_pending = true;
        return PT_OK;
    }
    if (!positions_xyz) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: positions_xyz is NULL");
    if (config->resolution < 16 || config->resolution > 1024 || config->resolution % 16 != 0)
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: resolution must be a multiple of 16 in 16..1024");
    if (config->count < 1) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: count must be >= 1");
    if (config->columns < 1) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: columns must be >= 1");
    if (!std::isfinite(config->max_distance) || !(config->max_distance > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: max_distance must be finite and > 0");
    uint64_t w, h;
    probe_atlas_size(*config, w, h);
    if (w > (1ull << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: columns * resolution = " + std::to_string(w) + " exceeds 2^30");
    if (h > (1ull << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: rows * resolution = " + std::to_string(h) + " (count / columns rows) exceeds 2^30");
    for (int64_t i = 0; i < (int64_t)config->count * 3; i++)
        if (!std::isfinite(positions_xyz[i])) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: the position of probe " + std::to_string(i / 3) + " is not finite");
    if (ctx->bake.enable) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: a bake is enabled (pt_set_bake): a trace renders one atlas or the other");
    ENTER(ctx);
    const size_t bytes = (size_t)config->count * 12;
    // a trace in flight may still read the old positions: the copy goes behind it on the stream, a larger array drains it first (DevBuf)
    if (const hipError_t e = ctx->d_probe_pos.reserve(ctx->stream, bytes, bytes)) {
        if (ctx->d_probe_pos.ptr == nullptr) { ctx->probes.enable = 0; ctx->restart_pending = true; }     // the old array went with the failed growth
        return grow_failed(ctx, e, "probe positions: " + std::to_string(bytes) + " bytes");
    }
    if (const hipError_t e = staged_upload(ctx, ctx->d_probe_pos.ptr, positions_xyz, bytes)) {
        ctx->probes.enable = 0; ctx->restart_pending = true;               // the array may hold part of either set: back to the camera
        return ctx->fail(PT_ERR_DEVICE, std::string("probe positions: ") + hipGetErrorString(e));
    }
    ctx->probes = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_probe_project(pt_ctx* ctx, const void* atlas_device, uint32_t width, uint32_t height, int kind, float* sh_host) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!atlas_device || !sh_host) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probe_project: NULL argument");
    if (kind != PT_PROBE_SH_RADIANCE && kind != PT_PROBE_SH_IRRADIANCE) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probe_project: kind must be PT_PROBE_SH_RADIANCE or PT_PROBE_SH_IRRADIANCE");
    if (!ctx->probes.enable) return ctx->fail(PT_ERR_NOT_READY, "probe_project: no probes are set");
    uint64_t w, h;
    probe_atlas_size(ctx->probes, w, h);
    if (width != w || height != h) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probe_project: the atlas is " + std::to_string(w) + " x " + std::to_string(h));
    ENTER(ctx);
    const uint32_t n = (uint32_t)ctx->probes.resolution, count = (uint32_t)ctx->probes.count;
    if (ctx->probe_dirs_n != n) {
        const size_t bytes = (size_t)n * n * 16;
        ctx->probe_dirs_n = 0;
        if (const hipError_t e = ctx->d_probe_dirs.reserve(ctx->stream, bytes, bytes)) return grow_failed(ctx, e, "probe direction table: " + std::to_string(bytes) + " bytes");
        launch_probe_dirs(ctx->d_probe_dirs.as<float4>(), n, ctx->stream);
        HIPOK(hipGetLastError());
        ctx->probe_dirs_n = n;
    }
    const size_t out_bytes = (size_t)count * 27 * 4;
    if (const hipError_t e = ctx->d_probe_sh.reserve(ctx->stream, out_bytes, out_bytes)) return grow_failed(ctx, e, "probe coefficients: " + std::to_string(out_bytes) + " bytes");
    launch_probe_project((const float4*)atlas_device, ctx->d_probe_dirs.as<float4>(), n, count, (uint32_t)ctx->probes.columns, kind, ctx->d_probe_sh.as<float>(), ctx->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(sh_host, ctx->d_probe_sh.ptr, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPOK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

}  // extern "C"
