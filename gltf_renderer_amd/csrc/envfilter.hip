// envfilter.hip -- pt_env_filter: the environment's GGX chain and diffuse cube (EnvironmentMap::GenerateGgxCube / GenerateDiffuseCube ->
// FilterCube, Source/EnvironmentMap.cpp:348-401, Shaders/FilterEnvironmentCubeMap.cs.hlsl) on gfx950.  include/mipt.h states the arithmetic
// operation by operation; tests/envfilter_ref.py restates it in numpy.  Filtered importance sampling: per output texel S samples of the
// BSDF's lobe around the texel's direction, each a trilinear lookup in the environment cube's mip chain at the level whose texels subtend
// the sample's solid angle.
//
// Two kernels a level.  k_env_filter_table computes what a sample has that no texel changes -- GGX: the half vector in the local frame
// and the clamped mip level; diffuse: the point on the unit sphere that is added to the normal -- one lane a sample.  k_env_filter sums
// one texel a lane, an 8 x 8 tile of texels a wave (neighbouring texels gather neighbouring taps), the table staged through LDS in pieces
// of kFilterChunk entries that every lane reads at the same address (a broadcast), beside the source chain's sizes and offsets: a diffuse
// lane picks its mip itself, and a per-lane index into kernel arguments would put them into scratch memory.
// This file calls the tracer's helpers (pt_shading.h) and changes none: no kernel of the tracer is compiled from it.
#include <cmath>

#include "pt_shading.h"
#include "pt_ctx.h"

namespace pt {
namespace {

constexpr int kFilterTile = 8;                                 // texels a side: one wave a tile
constexpr int kFilterLanes = kFilterTile * kFilterTile;
constexpr int kFilterChunk = 256;                              // table entries in LDS at a time: 4 KB
constexpr int kFilterMaxMips = 16;

struct FilterSource {                                          // the environment cube's chain, by value in the kernel's arguments
    const uint16_t* cube;
    size_t offset[kFilterMaxMips];                             // in halfs
    int n[kFilterMaxMips];
    int mips;
};
struct FilterParams {
    int samples;
    float roughness, mip_bias;
    float n0;                                                  // (float)N
    float last_mip;                                            // (float)(M - 1)
};

// The mip level of a sample of probability density pdf, clamped as D3D clamps: NaN -> 0, +inf -> the last mip
PT_DEV float filter_level(float pdf, const FilterParams& p) {
    const float omega_s = 1.0f / ((float)p.samples * pdf);
    const float omega_p = (4.0f * kPi) / ((6.0f * p.n0) * p.n0);
    const float level = 0.5f * co_log2(omega_s / omega_p) + p.mip_bias;
    return fminf(fmaxf(level, 0.0f), p.last_mip);
}

// R2(0.5, i) (Random.hlsli:80-85)
PT_DEV vec2 filter_r2(int i) {
    const float g = 1.324717957244746f;
    const float gg = g * g;
    const float c0 = 1.0f / g, c1 = 1.0f / gg;
    const float s0 = 0.5f + (float)i * c0, s1 = 0.5f + (float)i * c1;
    return {s0 - floorf(s0), s1 - floorf(s1)};
}

// GGX: (h.xyz, level);  diffuse: (the unit-sphere point, 0)
template <int KIND>
__global__ __launch_bounds__(256) void k_env_filter_table(const FilterParams p, float4* __restrict__ table) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.samples) return;
    const vec2 u = filter_r2(i);
    if (KIND == 0) {
        const vec3 h = sample_ggx_normal(p.roughness, u.x, u.y);
        const float pdf = ggx_d(p.roughness, h.z) / 4.0f;
        table[i] = make_float4(h.x, h.y, h.z, filter_level(pdf, p));
    } else {
        float sn, cs;
        pt_sincos(kTau * u.x, sn, cs);
        const float y = 2 * u.y - 1;
        const float r = sqrtf(1.0f - y * y);
        table[i] = make_float4(r * cs, r * sn, y, 0.0f);
    }
}

// SampleLevel(linear, l, level) of the chain: the oracle's SampleCubeLevel, k_importance0's blend
PT_DEV vec3 filter_fetch(const uint16_t* cube, const size_t* s_offset, const int* s_n, int mips, vec3 l, float level) {
    const int l0 = (int)floorf(level);
    const float f = level - (float)l0;
    const vec3 a = sample_cube(cube + s_offset[l0], s_n[l0], l);
    if (f == 0.0f || l0 + 1 >= mips) return a;
    const vec3 b = sample_cube(cube + s_offset[l0 + 1], s_n[l0 + 1], l);
    return a * (1 - f) + b * f;
}

template <int KIND>
__global__ __launch_bounds__(kFilterLanes) void k_env_filter(const FilterSource src, const float4* __restrict__ table, const FilterParams p,
                                                            uint16_t* __restrict__ out, int n) {
    __shared__ float4 s_table[kFilterChunk];
    __shared__ size_t s_offset[kFilterMaxMips];
    __shared__ int s_n[kFilterMaxMips];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kFilterMaxMips; k++)
        if (tid == k) { s_offset[k] = src.offset[k]; s_n[k] = src.n[k]; }
    const int x = blockIdx.x * kFilterTile + (tid % kFilterTile), y = blockIdx.y * kFilterTile + (tid / kFilterTile), face = blockIdx.z;
    const bool inside = x < n && y < n;                        // a lane outside the level only helps to stage the table
    const vec3 normal = cubemap_to_direction(face, ((float)x + .5f) / (float)n, ((float)y + .5f) / (float)n);
    vec3 t, b;
    basis_simple(normal, t, b);
    vec3 total = v3(0);
    float total_weight = 0;
    for (int base = 0; base < p.samples; base += kFilterChunk) {
        const int count = p.samples - base < kFilterChunk ? p.samples - base : kFilterChunk;
        __syncthreads();                                       // the piece before this one has been read (first: the chain's sizes are written)
        for (int k = tid; k < count; k += kFilterLanes) s_table[k] = table[base + k];
        __syncthreads();
        if (!inside) continue;
        for (int k = 0; k < count; k++) {
            const float4 e = s_table[k];
            vec3 l;
            float weight, level;
            if (KIND == 0) {
                const vec3 h = to_world(t, b, normal, v3(e.x, e.y, e.z));
                l = reflect(-normal, h);
                weight = saturate(dot(normal, l));
                level = e.w;
            } else {
                l = normalize(normal + v3(e.x, e.y, e.z));
                const float pdf = saturate(dot(l, normal) / kPi);
                weight = 1.0f;
                level = filter_level(pdf, p);
            }
            total += weight * filter_fetch(src.cube, s_offset, s_n, src.mips, l, level);
            total_weight += weight;
        }
    }
    if (!inside) return;
    const float r = total.x / total_weight, g = total.y / total_weight, bl = total.z / total_weight;
    const uint2 q = make_uint2((uint32_t)__half_as_ushort(__float2half_rn(r)) | ((uint32_t)__half_as_ushort(__float2half_rn(g)) << 16),
                               (uint32_t)__half_as_ushort(__float2half_rn(bl)));            // alpha 0, as k_cube_mip writes it
    *(uint2*)(out + (((size_t)face * n + y) * n + x) * 4) = q;
}

}  // namespace

hipError_t env_filter_level(const EnvDevice& e, const EnvFilterLevel& level, hipStream_t stream) {
    FilterSource src;
    src.cube = e.cube; src.mips = e.mips;
    for (int k = 0; k < kFilterMaxMips; k++) { src.offset[k] = k < e.mips ? e.mip_offset[k] : 0; src.n[k] = k < e.mips ? e.mip_n[k] : 1; }
    FilterParams p;
    p.samples = level.samples; p.roughness = level.roughness; p.mip_bias = level.mip_bias;
    p.n0 = (float)e.mip_n[0]; p.last_mip = (float)(e.mips - 1);
    const dim3 table_grid((level.samples + 255) / 256), tiles((level.n + kFilterTile - 1) / kFilterTile, (level.n + kFilterTile - 1) / kFilterTile, 6);
    if (level.kind == 0) {
        hipLaunchKernelGGL(k_env_filter_table<0>, table_grid, dim3(256), 0, stream, p, e.filter_table);
        hipLaunchKernelGGL(k_env_filter<0>, tiles, dim3(kFilterLanes), 0, stream, src, e.filter_table, p, level.out, level.n);
    } else {
        hipLaunchKernelGGL(k_env_filter_table<1>, table_grid, dim3(256), 0, stream, p, e.filter_table);
        hipLaunchKernelGGL(k_env_filter<1>, tiles, dim3(kFilterLanes), 0, stream, src, e.filter_table, p, level.out, level.n);
    }
    return hipGetLastError();
}

}  // namespace pt

using namespace pt;

namespace {

// The levels of a GGX chain over a cube of mip-0 size N: n_0 = N, n_{i+1} = n_i / 2 (FilterCube's `resolution /= 2`)
size_t ggx_layout(int N, int mips, size_t* offset, int* n) {
    size_t halfs = 0;
    int r = N;
    for (int i = 0; i < mips; i++) { n[i] = r; offset[i] = halfs; halfs += (size_t)6 * r * r * 4; r /= 2; }
    return halfs;
}

// Room for `halfs` halfs in `ptr`: kept if it holds exactly that, else the stream is drained (kernels enqueued may still write the old
// array, and a pointer handed out by pt_env_filter_read dies here) and the array allocated anew
int filter_room(pt_ctx* ctx, uint16_t*& ptr, size_t& have, size_t halfs, const char* what) {
    if (ptr && have == halfs) return PT_OK;
    HIPOK(hipStreamSynchronize(ctx->stream));
    hipFree(ptr);
    ptr = nullptr; have = 0;
    if (hipMalloc((void**)&ptr, halfs * 2) != hipSuccess) {
        (void)hipGetLastError();
        ptr = nullptr;
        return ctx->fail(PT_ERR_OUT_OF_MEMORY, std::string("env_filter: ") + std::to_string(halfs * 2) + " bytes for " + what);
    }
    have = halfs;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_env_filter(pt_ctx* ctx, int env, const pt_env_filter_config* config) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_env_filter");
    EnvDevice& e = *ctx->envs[env];
    pt_env_filter_config cfg = {256, 2.0f, 0, 512, 3.0f, 256};               // EnvironmentMap.cpp:395, 400, 114
    if (config) cfg = *config;
    const int N = e.mip_n[0], available = e.mips < kFilterMaxMips ? e.mips : kFilterMaxMips;
    if (cfg.ggx_samples < 1 || cfg.ggx_samples > kEnvFilterMaxSamples) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "env_filter: ggx_samples outside 1..4096");
    if (cfg.diffuse_samples < 1 || cfg.diffuse_samples > kEnvFilterMaxSamples) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "env_filter: diffuse_samples outside 1..4096");
    if (!std::isfinite(cfg.ggx_mip_bias) || !std::isfinite(cfg.diffuse_mip_bias)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "env_filter: a mip bias is not finite");
    if (cfg.ggx_mips < 0 || cfg.ggx_mips > available) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "env_filter: ggx_mips outside 0.." + std::to_string(available));
    if (cfg.diffuse_resolution < 1 || cfg.diffuse_resolution > kEnvFilterMaxResolution) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "env_filter: diffuse_resolution outside 1..1024");
    int mips = cfg.ggx_mips;
    if (mips == 0) {                                                         // EnvironmentMap.cpp:106-107
        mips = (int)std::floor(std::log2((float)N)) + 1 - 4;
        mips = mips > 1 ? mips : 1;
        if (mips > available) mips = available;
    }
    ENTER(ctx);
    size_t offset[kFilterMaxMips] = {0};
    int n[kFilterMaxMips] = {0};
    const size_t ggx_halfs = ggx_layout(N, mips, offset, n);
    const size_t diffuse_halfs = (size_t)6 * cfg.diffuse_resolution * cfg.diffuse_resolution * 4;
    e.filtered = false;                                                      // until every array stands
    if (const int rc = filter_room(ctx, e.ggx, e.ggx_halfs, ggx_halfs, "the GGX chain")) return rc;
    if (const int rc = filter_room(ctx, e.diffuse, e.diffuse_halfs, diffuse_halfs, "the diffuse cube")) return rc;
    if (!e.filter_table && hipMalloc((void**)&e.filter_table, (size_t)kEnvFilterMaxSamples * sizeof(float4)) != hipSuccess) {
        (void)hipGetLastError();
        e.filter_table = nullptr;
        return ctx->fail(PT_ERR_OUT_OF_MEMORY, "env_filter: the sample table");
    }
    e.ggx_mips = mips; e.diffuse_n = cfg.diffuse_resolution;
    for (int i = 0; i < kFilterMaxMips; i++) {
        e.ggx_offset[i] = offset[i]; e.ggx_n[i] = n[i];
        float r = 0.0f;
        if (i < mips && mips > 1) { r = (float)i / ((float)mips - 1.0f); r *= r; }      // MipToRoughness; one level: 0, not 0 / 0 (quirk q30)
        e.ggx_roughness[i] = r;
    }
    for (int i = 0; i < mips; i++) {
        if (n[i] < 1) continue;                                              // (cannot happen: mips <= the levels N >> i >= 1)
        const EnvFilterLevel level = {0, cfg.ggx_samples, e.ggx_roughness[i], cfg.ggx_mip_bias, e.ggx + offset[i], n[i]};
        HIPOK(env_filter_level(e, level, ctx->stream));
    }
    const EnvFilterLevel level = {1, cfg.diffuse_samples, 0.0f, cfg.diffuse_mip_bias, e.diffuse, cfg.diffuse_resolution};
    HIPOK(env_filter_level(e, level, ctx->stream));
    e.filtered = true;
    return PT_OK;
}

int pt_env_filter_info_get(pt_ctx* ctx, int env, pt_env_filter_info* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_env_filter_info_get");
    if (!out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_env_filter_info_get: null out");
    const EnvDevice& e = *ctx->envs[env];
    if (!e.filtered) return ctx->fail(PT_ERR_NOT_READY, "pt_env_filter_info_get: no pt_env_filter on this environment yet");
    out->ggx_resolution = e.ggx_n[0]; out->ggx_mips = e.ggx_mips; out->diffuse_resolution = e.diffuse_n;
    for (int i = 0; i < 16; i++) out->ggx_roughness[i] = e.ggx_roughness[i];
    return PT_OK;
}

int pt_env_filter_read(pt_ctx* ctx, int env, int which, int mip, int* size_out, uint16_t* host, void** device_out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_env_filter_read");
    const EnvDevice& e = *ctx->envs[env];
    if (!e.filtered) return ctx->fail(PT_ERR_NOT_READY, "pt_env_filter_read: no pt_env_filter on this environment yet");
    if (which != 0 && which != 1) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_env_filter_read: which is 0 (GGX) or 1 (diffuse)");
    if (mip < 0 || mip >= (which == 0 ? e.ggx_mips : 1)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_env_filter_read: no such mip");
    const int n = which == 0 ? e.ggx_n[mip] : e.diffuse_n;
    uint16_t* texels = which == 0 ? e.ggx + e.ggx_offset[mip] : e.diffuse;
    if (size_out) *size_out = n;
    if (device_out) *device_out = texels;
    if (host) {
        ENTER(ctx);
        HIPOK(hipStreamSynchronize(ctx->stream));
        HIPOK(hipMemcpy(host, texels, (size_t)6 * n * n * 4 * 2, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

}  // extern "C"
