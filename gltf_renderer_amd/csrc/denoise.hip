// denoise.hip -- pt_denoise: the edge-avoiding a-trous filter over the first-hit AOVs (include/mipt.h states it operation by operation;
// tests/denoise_ref.py restates it in numpy).  Three kinds of launch on the context's stream:
//   k_dn_prepare   per pixel: the demodulated signal (S.rgb, L = (S.r + S.g) + S.b) and the guide (unit normal, depth); an invalid pixel
//                  gets a guide depth of 0, which is how the passes tell (a valid depth is > 0)
//   k_dn_pass      pass i: 25 taps at spacing 2^i, dy outer, dx inner, sequential sums -- from one signal image to the other
//   k_dn_pass<1>   the last pass, which multiplies the albedo back and writes the caller's image (invalid pixels: the input's bits)
// Compiled without floating-point contraction (Makefile), with IEEE division and square root: apart from expf the arithmetic is that of
// the float32 restatement, rounding for rounding.  (tools/denoise_host_rehearsal.py compiles the file's first anonymous namespace.)
#include <cmath>

#include "pt_ctx.h"

namespace pt {
namespace {

// A block is 32 x 8 pixels: a wave holds two rows of 32, so every tap row is two runs of 32 consecutive float4 (512 B) per image at
// every spacing, and the direct 16-byte loads are coalesced as they are.
constexpr int DN_BX = 32, DN_BY = 8;

// max(m, 1e-3) that keeps a NaN (fmaxf would drop it, and a pixel with a NaN albedo must come out invalid)
__device__ __forceinline__ float dn_floor(float m) { return m < 1e-3f ? 1e-3f : m; }

__device__ __forceinline__ float3 dn_albedo(const float4 A, int demodulate) {
    if (!demodulate) return make_float3(1.0f, 1.0f, 1.0f);
    const float m = 1.0f - A.w;                         // a miss counts as albedo 1
    return make_float3(dn_floor(A.x + m), dn_floor(A.y + m), dn_floor(A.z + m));
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_prepare(const float4* __restrict__ color, const float4* __restrict__ albedo,
                                                               const float4* __restrict__ normal_depth, uint32_t w, uint32_t h, int demodulate,
                                                               float4* __restrict__ S, float4* __restrict__ G) {
    const uint32_t x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 C = color[p], A = albedo[p], N = normal_depth[p];
    const float cov = A.w;
    const float3 a = dn_albedo(A, demodulate);
    const float sr = C.x / a.x, sg = C.y / a.y, sb = C.z / a.z;
    const float len = sqrtf((N.x * N.x + N.y * N.y) + N.z * N.z);
    const float nx = N.x / len, ny = N.y / len, nz = N.z / len;
    const float z = N.w / cov;
    const bool valid = cov > 0.0f && len > 0.0f && isfinite(z) && z > 0.0f && isfinite(sr) && isfinite(sg) && isfinite(sb) &&
                       isfinite(nx) && isfinite(ny) && isfinite(nz);
    S[p] = valid ? make_float4(sr, sg, sb, (sr + sg) + sb) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    G[p] = valid ? make_float4(nx, ny, nz, z) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

struct DnPass {
    const float4* S;          // the signal of the previous pass (or of k_dn_prepare)
    const float4* G;          // the guide
    float4* dst;              // the signal this pass writes (not the last pass)
    uint32_t w, h;
    int step;                 // 2^i
    int normal_squarings;     // normal_power_log2
    float zk;                 // sigma_depth * step
    float sig2;               // (sigma_color * 2^-i)^2
    int color_on;             // sigma_color != 0
    // the last pass
    const float4* color;
    const float4* albedo;
    float4* out;
    int demodulate;
};

struct DnSums { float w, r, g, b; };

// One tap: its weight, and the select that adds it.  hh = h[dy] h[dx] (exact).
__device__ __forceinline__ void dn_tap(const DnPass& a, const float4 Gp, const float4 Sp, float zden, float hh, const float4 Gq, const float4 Sq,
                                       bool in_image, DnSums& s) {
    float wn = fminf(fmaxf((Gp.x * Gq.x + Gp.y * Gq.y) + Gp.z * Gq.z, 0.0f), 1.0f);
    for (int j = 0; j < a.normal_squarings; j++) wn = wn * wn;
    const float ez = fabsf(Gp.w - Gq.w) / zden;
    float ec = 0.0f;
    if (a.color_on) {
        const float dr = Sp.x - Sq.x, dg = Sp.y - Sq.y, db = Sp.z - Sq.z;
        const float ls = Sp.w + Sq.w;
        ec = ((dr * dr + dg * dg) + db * db) / (a.sig2 * (ls * ls) + 1e-8f);
    }
    const float wt = (hh * wn) * expf(-(ez + ec));
    if (in_image && Gq.w > 0.0f) {              // a select: the weight of an invalid tap is never multiplied with anything
        s.w = s.w + wt;
        s.r = s.r + wt * Sq.x;
        s.g = s.g + wt * Sq.y;
        s.b = s.b + wt * Sq.z;
    }
}

template <bool LAST>
__device__ __forceinline__ void dn_write(const DnPass& a, size_t p, const DnSums& s) {
    const float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    if (LAST) {
        const float3 al = dn_albedo(a.albedo[p], a.demodulate);
        a.out[p] = make_float4(r * al.x, g * al.y, b * al.z, a.color[p].w);
    } else {
        a.dst[p] = make_float4(r, g, b, (r + g) + b);
    }
}

// The direct kernel: every tap is a 16-byte global load (25 x 32 B per pixel through L2), at any spacing.
template <bool LAST>
__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_pass(const DnPass a) {
    const uint32_t x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 Gp = a.G[p];
    if (!(Gp.w > 0.0f)) {                       // invalid: never filtered, never a neighbour; it leaves the call with the input's bits
        if (LAST) a.out[p] = a.color[p];
        return;
    }
    const float4 Sp = a.S[p];
    const float zden = a.zk * Gp.w + 1e-6f;
    const float h5[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    DnSums s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = (int)y + dy * a.step;
        if (qy < 0 || qy >= (int)a.h) continue;
        const size_t row = (size_t)qy * a.w;
        float4 Gq[5], Sq[5];
        bool ok[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {           // the row's ten loads first, from clamped (in-image) addresses
            const int qx = (int)x + (k - 2) * a.step;
            ok[k] = qx >= 0 && qx < (int)a.w;
            const size_t q = row + (size_t)(ok[k] ? qx : (int)x);
            Gq[k] = a.G[q];
            Sq[k] = a.S[q];
        }
#pragma unroll
        for (int k = 0; k < 5; k++) dn_tap(a, Gp, Sp, zden, h5[dy + 2] * h5[k], Gq[k], Sq[k], ok[k], s);
    }
    dn_write<LAST>(a, p, s);
}

}  // namespace

hipError_t launch_denoise(const pt_denoise_config& cfg, const float4* color, const float4* albedo, const float4* normal_depth, uint32_t w, uint32_t h,
                          float4* out, float4* ping, float4* pong, float4* guide, hipStream_t stream) {
    if (cfg.iterations <= 0) return hipSuccess;
    const dim3 block(DN_BX, DN_BY), grid((w + DN_BX - 1) / DN_BX, (h + DN_BY - 1) / DN_BY);
    k_dn_prepare<<<grid, block, 0, stream>>>(color, albedo, normal_depth, w, h, cfg.demodulate != 0, ping, guide);
    float4 *src = ping, *dst = pong;
    for (int i = 0; i < cfg.iterations; i++) {
        DnPass a;
        a.S = src; a.G = guide; a.dst = dst; a.w = w; a.h = h;
        a.step = 1 << i;
        a.normal_squarings = cfg.normal_power_log2;
        a.zk = cfg.sigma_depth * (float)a.step;
        const float sig = cfg.sigma_color * ldexpf(1.0f, -i);
        a.sig2 = sig * sig;
        a.color_on = cfg.sigma_color != 0.0f;
        a.color = color; a.albedo = albedo; a.out = out; a.demodulate = cfg.demodulate != 0;
        if (i == cfg.iterations - 1) k_dn_pass<true><<<grid, block, 0, stream>>>(a);
        else k_dn_pass<false><<<grid, block, 0, stream>>>(a);
        float4* t = src; src = dst; dst = t;
    }
    return hipGetLastError();
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_denoise(pt_ctx* ctx, const pt_denoise_config* config, const void* color, const void* albedo, const void* normal_depth,
               uint32_t width, uint32_t height, void* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!color || !albedo || !normal_depth || !out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: bad size");
    pt_denoise_config cfg = {5, 1, 7, 0.02f, 1.0f};
    if (config) cfg = *config;
    if (cfg.iterations < 0 || cfg.iterations > 6) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: iterations outside 0..6");
    if (cfg.normal_power_log2 < 0 || cfg.normal_power_log2 > 10) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: normal_power_log2 outside 0..10");
    if (!std::isfinite(cfg.sigma_depth) || !(cfg.sigma_depth > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: sigma_depth must be finite and > 0");
    if (!std::isfinite(cfg.sigma_color) || cfg.sigma_color < 0.0f) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: sigma_color must be finite and >= 0");
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    if (ranges_overlap(out, bytes, albedo, bytes) || ranges_overlap(out, bytes, normal_depth, bytes)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: out aliases a guide image");
    if (out != color && ranges_overlap(out, bytes, color, bytes)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise: out overlaps color without being color");
    ENTER(ctx);
    if (cfg.iterations == 0) {                  // the identity: a copy, or nothing in place
        if (out != color) HIPOK(hipMemcpyAsync(out, color, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PT_OK;
    }
    if (3 * bytes != ctx->d_denoise.cap) HIPOK(ctx->d_denoise.realloc(ctx->stream, 3 * bytes));      // for this size alone: a smaller image reallocates too
    float4* s = ctx->d_denoise.as<float4>();
    HIPOK(launch_denoise(cfg, (const float4*)color, (const float4*)albedo, (const float4*)normal_depth, width, height, (float4*)out, s, s + n, s + 2 * n, ctx->stream));
    return PT_OK;
}

}  // extern "C"
