// blur.hip -- pt_motion_blur: the shutter-time reconstruction filter along the motion vectors (include/mipt.h states it operation by
// operation; tests/blur_ref.py restates it in numpy float32, rounding for rounding).  A pure function of two images.  Three launches on the
// context's stream, over 16 x 16 tiles (PT_TILE) numbered row-major:
//   k_blur_prepare    one 256-lane workgroup per tile: V[p] = (half streak x, y, its length, depth) per pixel, and the tile's longest streak
//                     T[t] by a 64-bit key (length bits << 32 | 0xffffffff - index in tile): wave-64 shuffles, then four keys through LDS.
//                     The length is >= +0 and finite, so its bits order like its value; the key makes the result independent of the order
//                     of the reduction and gives a tie to the least (y, x).
//   k_blur_neighbour  one lane per tile: N[t] = the longest T within r tiles, at most 81 of them, dy outer, dx inner, strictly larger wins.
//   k_blur_gather     one workgroup per tile, so N[t] is wave-uniform (scalar registers) and a tile with a streak below half a pixel leaves
//                     by a plain copy.  A tap reads 16 B of V and 16 B of colour; the taps of a tile's lanes are the tile shifted along one
//                     direction, so neighbouring lanes read neighbouring texels.  Exclusion is by selects.
// Compiled without floating-point contraction (Makefile), with IEEE division and square root.
#include <cmath>

#include "pt_ctx.h"

namespace pt {
namespace {

constexpr int kBlurTile = PT_TILE, kBlurLanes = PT_TILE * PT_TILE;
static_assert(kBlurLanes == 256, "k_blur_prepare reduces four waves of 64");

__device__ __forceinline__ unsigned long long blur_max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ bool blur_finite3(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
__device__ __forceinline__ float blur_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float blur_cone(float d, float l) { return l > d ? 1.0f - d / l : 0.0f; }
__device__ __forceinline__ float blur_cyl(float d, float l) { return l >= d ? 1.0f : 0.0f; }

__global__ __launch_bounds__(kBlurLanes) void k_blur_prepare(const BlurArgs a) {
    __shared__ unsigned long long s_key[kBlurLanes / 64];
    const uint32_t t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const uint32_t i = threadIdx.x;
    const uint32_t x = tx * kBlurTile + (i & (kBlurTile - 1)), y = ty * kBlurTile + i / kBlurTile;
    float vx = 0.0f, vy = 0.0f, l = 0.0f;
    unsigned long long key = 0;                       // a lane off the image: below every pixel's key, and the tile's first pixel is one
    if (x < a.w && y < a.h) {
        const size_t p = (size_t)y * a.w + x;
        const float4 m = a.motion[p];
        const bool covered = isfinite(m.w) && m.w > 0.0f;
        const float z = covered ? m.w : INFINITY;
        vx = (-m.x) * a.half_shutter; vy = (-m.y) * a.half_shutter;
        l = sqrtf(vx * vx + vy * vy);
        const bool moving = covered && isfinite(m.x) && isfinite(m.y) && isfinite(m.z) && m.z > 0.0f && isfinite(l);
        if (l > a.max_radius) {
            const float k = a.max_radius / l;
            vx = vx * k; vy = vy * k; l = a.max_radius;
        }
        if (!moving) { vx = 0.0f; vy = 0.0f; l = 0.0f; }
        a.V[p] = make_float4(vx, vy, l, z);
        key = ((unsigned long long)__float_as_uint(l) << 32) | (unsigned long long)(0xffffffffu - i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)key, o, 64), hi = __shfl_xor((uint32_t)(key >> 32), o, 64);
        key = blur_max_u64(key, ((unsigned long long)hi << 32) | lo);
    }
    if ((i & 63) == 0) s_key[i >> 6] = key;
    __syncthreads();
    const unsigned long long best = blur_max_u64(blur_max_u64(s_key[0], s_key[1]), blur_max_u64(s_key[2], s_key[3]));
    if (i == 0xffffffffu - (uint32_t)best) a.T[t] = make_float4(vx, vy, l, 0.0f);
}

__global__ __launch_bounds__(kBlurLanes) void k_blur_neighbour(const BlurArgs a) {
    const uint32_t t = blockIdx.x * kBlurLanes + threadIdx.x;
    if (t >= a.tiles_x * a.tiles_y) return;
    const int ty = (int)(t / a.tiles_x), tx = (int)(t - (uint32_t)ty * a.tiles_x);
    float4 best = make_float4(0.0f, 0.0f, -1.0f, 0.0f);         // below every length: the first tile visited is taken
    for (int dy = -a.reach; dy <= a.reach; dy++) {
        const int yy = ty + dy;
        if (yy < 0 || yy >= (int)a.tiles_y) continue;
        for (int dx = -a.reach; dx <= a.reach; dx++) {
            const int xx = tx + dx;
            if (xx < 0 || xx >= (int)a.tiles_x) continue;
            const float4 c = a.T[(size_t)yy * a.tiles_x + (size_t)xx];
            if (c.z > best.z) best = c;
        }
    }
    a.N[t] = make_float4(best.x, best.y, best.z, 0.0f);
}

__global__ __launch_bounds__(kBlurLanes) void k_blur_gather(const BlurArgs a) {
    const uint32_t t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const float4 n = a.N[t];                          // a uniform address: scalar loads, scalar registers
    const uint32_t i = threadIdx.x;
    const uint32_t x = tx * kBlurTile + (i & (kBlurTile - 1)), y = ty * kBlurTile + i / kBlurTile;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 c = a.color[p];
    if (n.z < 0.5f) {                                 // the whole tile
        a.out[p] = c;
        return;
    }
    if (!blur_finite3(c)) {
        a.out[p] = c;
        return;
    }
    float g = 0.5f;
    if (a.jitter) {
        const float u = 0.06711056f * (float)x + 0.00583715f * (float)y;
        const float f = 52.9829189f * (u - floorf(u));
        g = f - floorf(f);
    }
    const float4 vp = a.V[p];
    const float lp = vp.z, zp = vp.w;
    const float wc = 1.0f / fmaxf(lp, 0.5f);
    float sw = wc, sr = wc * c.x, sg = wc * c.y, sb = wc * c.z;
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f, ftaps = (float)a.taps;
    for (int k = 0; k < a.taps; k++) {
        const float tau = (((float)k + g) / ftaps) * 2.0f - 1.0f;
        const int qx = (int)floorf(cx + tau * n.x), qy = (int)floorf(cy + tau * n.y);
        const bool inside = qx >= 0 && qy >= 0 && qx < (int)a.w && qy < (int)a.h;
        const size_t q = inside ? (size_t)qy * a.w + (size_t)qx : p;       // a tap off the image reads the centre and is not counted
        const float4 vq = a.V[q], cq = a.color[q];
        const float d = fabsf(tau) * n.z;
        const float lq = vq.z, zq = vq.w;
        float fg = 1.0f, bg = 1.0f;
        if (zp != zq) {
            const float e = a.depth_softness * fminf(zp, zq);
            fg = blur_clamp01(1.0f - (zq - zp) / e);
            bg = blur_clamp01(1.0f - (zp - zq) / e);
        }
        const float w = (fg * blur_cone(d, lq) + bg * blur_cone(d, lp)) + 2.0f * (blur_cyl(d, lq) * blur_cyl(d, lp));
        if (inside && blur_finite3(cq)) {             // a select: the weight of a skipped tap is never multiplied with anything
            sw = sw + w;
            sr = sr + w * cq.x; sg = sg + w * cq.y; sb = sb + w * cq.z;
        }
    }
    a.out[p] = make_float4(sr / sw, sg / sw, sb / sw, c.w);
}

}  // namespace

hipError_t launch_motion_blur(const BlurArgs& a, hipStream_t stream) {
    const uint32_t tiles = a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(k_blur_prepare, dim3(tiles), dim3(kBlurLanes), 0, stream, a);
    hipLaunchKernelGGL(k_blur_neighbour, dim3((tiles + kBlurLanes - 1) / kBlurLanes), dim3(kBlurLanes), 0, stream, a);
    hipLaunchKernelGGL(k_blur_gather, dim3(tiles), dim3(kBlurLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_motion_blur(pt_ctx* ctx, const pt_motion_blur_config* config, const void* color, const void* motion, uint32_t width, uint32_t height, void* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!color || !motion || !out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: bad size");
    if ((uint64_t)width * height > 0x7fffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: width * height exceeds 2^31 - 1");
    pt_motion_blur_config cfg = {0.5f, 32.0f, 16, 1, 0.05f};
    if (config) cfg = *config;
    if (!std::isfinite(cfg.shutter) || !(cfg.shutter > 0.0f && cfg.shutter <= 2.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: shutter must be finite, > 0 and <= 2");
    if (!std::isfinite(cfg.max_radius) || !(cfg.max_radius >= 1.0f && cfg.max_radius <= 64.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: max_radius outside 1..64");
    if (cfg.taps < 2 || cfg.taps > 64) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: taps outside 2..64");
    if (!std::isfinite(cfg.depth_softness) || !(cfg.depth_softness > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: depth_softness must be finite and > 0");
    const size_t n = (size_t)width * height, bytes = n * 16;
    if (ranges_overlap(out, bytes, color, bytes) || ranges_overlap(out, bytes, motion, bytes))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_blur: out overlaps an input (there is no in-place mode)");
    ENTER(ctx);
    BlurArgs a;
    a.w = width; a.h = height;
    a.tiles_x = (width + PT_TILE - 1) / PT_TILE; a.tiles_y = (height + PT_TILE - 1) / PT_TILE;
    const size_t tiles = (size_t)a.tiles_x * a.tiles_y;
    const size_t need = bytes + 2 * tiles * 16;         // V, then T, then N
    if (const int rc = exact_scratch(ctx, ctx->d_blur, need, "motion_blur")) return rc;      // for this size alone
    a.color = (const float4*)color; a.motion = (const float4*)motion; a.out = (float4*)out;
    a.V = ctx->d_blur.as<float4>(); a.T = a.V + n; a.N = a.T + tiles;
    a.half_shutter = 0.5f * cfg.shutter; a.max_radius = cfg.max_radius; a.depth_softness = cfg.depth_softness;
    a.taps = cfg.taps; a.jitter = cfg.jitter != 0;
    a.reach = (int)ceilf(cfg.max_radius / 16.0f);
    HIPOK(launch_motion_blur(a, ctx->stream));
    return PT_OK;
}

}  // extern "C"
