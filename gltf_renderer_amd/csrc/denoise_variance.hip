// denoise_variance.hip -- pt_denoise_variance: the a-trous filter steered by the variance AOV, the spatial filter of SVGF (include/mipt.h
// states it operation by operation; tests/denoise_variance_ref.py restates it in numpy).  pt_denoise's guides, taps and edge terms with a
// colour term normalised by the measured variance of the pixels' means, and that variance carried from pass to pass.  Launches on the
// context's stream:
//   k_dv_prepare     per pixel: the demodulated signal and the variance of its mean (S.rgb, v) and the guide (unit normal, depth); an
//                    invalid pixel gets a guide depth of 0, which is how the other kernels tell (a valid depth is > 0)
//   k_dv_prefilter   before pass i: vt = the 3 x 3 binomial mean of v over the valid taps, into a plane of its own
//   k_dv_pass        pass i: 25 taps at spacing 2^i, dy outer, dx inner, sequential sums of w, w S and (w w) v -- from one signal image
//                    to the other
//   k_dv_pass<1>     the last pass, which multiplies the albedo back and writes the caller's image (invalid pixels: the input's bits);
//                    nothing reads its variance, so it does not form it
//   k_dv_pass_lds    the passes at spacings 1 and 2, where the taps of neighbouring lanes overlap: the block and its halo staged in LDS
//                    once, the same taps in the same order from there -- the direct kernel's bits, 7 % and 4 % faster a pass on the
//                    MI355X (profiles/EXPERIMENTS.md)
// Compiled without floating-point contraction (Makefile), with IEEE division and square root: apart from expf the arithmetic is that of
// the float32 restatement, rounding for rounding.  (tools/denoise_variance_host_rehearsal.py compiles the file's first anonymous namespace.)
#include <cmath>

#include "pt_ctx.h"

namespace pt {
namespace {

// pt_denoise's block: 32 x 8 pixels, a wave holds two rows of 32, so every tap row is two runs of 32 consecutive float4 per image
constexpr int DV_BX = 32, DV_BY = 8;

// max(m, 1e-3) that keeps a NaN (fmaxf would drop it, and a pixel with a NaN albedo must come out invalid)
__device__ __forceinline__ float dv_floor(float m) { return m < 1e-3f ? 1e-3f : m; }

__device__ __forceinline__ float3 dv_albedo(const float4 A, int demodulate) {
    if (!demodulate) return make_float3(1.0f, 1.0f, 1.0f);
    const float m = 1.0f - A.w;                         // a miss counts as albedo 1
    return make_float3(dv_floor(A.x + m), dv_floor(A.y + m), dv_floor(A.z + m));
}

// counts: one per 16 x 16 tile, row-major (nullptr: `samples` everywhere)
__global__ __launch_bounds__(DV_BX * DV_BY) void k_dv_prepare(const float4* __restrict__ color, const float4* __restrict__ albedo,
                                                               const float4* __restrict__ normal_depth, const float4* __restrict__ variance,
                                                               uint32_t w, uint32_t h, uint32_t tiles_x, const uint32_t* __restrict__ counts,
                                                               uint32_t samples, int demodulate, float4* __restrict__ S, float4* __restrict__ G) {
    const uint32_t x = blockIdx.x * DV_BX + threadIdx.x, y = blockIdx.y * DV_BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 C = color[p], A = albedo[p], N = normal_depth[p], V = variance[p];
    const uint32_t count = counts ? counts[(size_t)(y / PT_TILE) * tiles_x + x / PT_TILE] : samples;
    const float cov = A.w;
    const float3 a = dv_albedo(A, demodulate);
    const float sr = C.x / a.x, sg = C.y / a.y, sb = C.z / a.z;
    const float len = sqrtf((N.x * N.x + N.y * N.y) + N.z * N.z);
    const float nx = N.x / len, ny = N.y / len, nz = N.z / len;
    const float z = N.w / cov;
    const float k = (float)(count - 1u);                // a count below 2 is invalid whatever this gives
    const float ur = (V.x / k) / (a.x * a.x), ug = (V.y / k) / (a.y * a.y), ub = (V.z / k) / (a.z * a.z);
    const float v = (ur + ug) + ub;
    const bool valid = cov > 0.0f && len > 0.0f && isfinite(z) && z > 0.0f && isfinite(sr) && isfinite(sg) && isfinite(sb) &&
                       isfinite(nx) && isfinite(ny) && isfinite(nz) && count >= 2u && isfinite(v) && v >= 0.0f;
    S[p] = valid ? make_float4(sr, sg, sb, v) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    G[p] = valid ? make_float4(nx, ny, nz, z) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// vt of the valid pixels (0 for the others, which nothing uses): nine taps at unit spacing, the w channels of the two images
__global__ __launch_bounds__(DV_BX * DV_BY) void k_dv_prefilter(const float4* __restrict__ S, const float4* __restrict__ G, uint32_t w, uint32_t h,
                                                                 float* __restrict__ vt) {
    const uint32_t x = blockIdx.x * DV_BX + threadIdx.x, y = blockIdx.y * DV_BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    if (!(G[p].w > 0.0f)) { vt[p] = 0.0f; return; }
    const float k3[3] = {1.0f / 4, 1.0f / 2, 1.0f / 4};
    float sg = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)h) continue;
        const size_t row = (size_t)qy * w;
        float zq[3], vq[3];
        bool ok[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {           // the row's six loads first, from clamped (in-image) addresses
            const int qx = (int)x + (k - 1);
            ok[k] = qx >= 0 && qx < (int)w;
            const size_t q = row + (size_t)(ok[k] ? qx : (int)x);
            zq[k] = G[q].w;
            vq[k] = S[q].w;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float g = k3[dy + 1] * k3[k];
            if (ok[k] && zq[k] > 0.0f) {        // a select, as in the passes
                sg = sg + g;
                sv = sv + g * vq[k];
            }
        }
    }
    vt[p] = sv / sg;
}

struct DvPass {
    const float4* S;          // the signal and its variance after the previous pass (or k_dv_prepare)
    const float4* G;          // the guide
    const float* vt;          // the prefiltered variance of S
    float4* dst;              // what this pass writes (not the last pass)
    uint32_t w, h;
    int step;                 // 2^i
    int normal_squarings;     // normal_power_log2
    float zk;                 // sigma_depth * step
    float sv2;                // sigma_variance^2
    int color_on;             // sigma_variance != 0
    // the last pass
    const float4* color;
    const float4* albedo;
    float4* out;
    int demodulate;
};

struct DvSums { float w, r, g, b, v; };

// One tap: its weight, and the select that adds it.  hh = h[dy] h[dx] (exact).
template <bool LAST>
__device__ __forceinline__ void dv_tap(const DvPass& a, const float4 Gp, const float4 Sp, float vtp, float zden, float hh, const float4 Gq,
                                       const float4 Sq, float vtq, bool in_image, DvSums& s) {
    float wn = fminf(fmaxf((Gp.x * Gq.x + Gp.y * Gq.y) + Gp.z * Gq.z, 0.0f), 1.0f);
    for (int j = 0; j < a.normal_squarings; j++) wn = wn * wn;
    const float ez = fabsf(Gp.w - Gq.w) / zden;
    float ec = 0.0f;
    if (a.color_on) {
        const float dr = Sp.x - Sq.x, dg = Sp.y - Sq.y, db = Sp.z - Sq.z;
        ec = ((dr * dr + dg * dg) + db * db) / (a.sv2 * (vtp + vtq) + 1e-8f);
    }
    const float wt = (hh * wn) * expf(-(ez + ec));
    if (in_image && Gq.w > 0.0f) {              // a select: the weight of an invalid tap is never multiplied with anything
        s.w = s.w + wt;
        s.r = s.r + wt * Sq.x;
        s.g = s.g + wt * Sq.y;
        s.b = s.b + wt * Sq.z;
        if (!LAST) s.v = s.v + (wt * wt) * Sq.w;
    }
}

template <bool LAST>
__device__ __forceinline__ void dv_write(const DvPass& a, size_t p, const DvSums& s) {
    const float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    if (LAST) {
        const float3 al = dv_albedo(a.albedo[p], a.demodulate);
        a.out[p] = make_float4(r * al.x, g * al.y, b * al.z, a.color[p].w);
    } else {
        a.dst[p] = make_float4(r, g, b, s.v / (s.w * s.w));
    }
}

// The direct kernel: every tap is two 16-byte global loads and one of 4 bytes (25 x 36 B per pixel through L2), at any spacing.
template <bool LAST>
__global__ __launch_bounds__(DV_BX * DV_BY) void k_dv_pass(const DvPass a) {
    const uint32_t x = blockIdx.x * DV_BX + threadIdx.x, y = blockIdx.y * DV_BY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 Gp = a.G[p];
    if (!(Gp.w > 0.0f)) {                       // invalid: never filtered, never a neighbour; it leaves the call with the input's bits
        if (LAST) a.out[p] = a.color[p];
        return;
    }
    const float4 Sp = a.S[p];
    const float vtp = a.vt[p];
    const float zden = a.zk * Gp.w + 1e-6f;
    const float h5[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    DvSums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = (int)y + dy * a.step;
        if (qy < 0 || qy >= (int)a.h) continue;
        const size_t row = (size_t)qy * a.w;
        float4 Gq[5], Sq[5];
        float vtq[5];
        bool ok[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {           // the row's fifteen loads first, from clamped (in-image) addresses
            const int qx = (int)x + (k - 2) * a.step;
            ok[k] = qx >= 0 && qx < (int)a.w;
            const size_t q = row + (size_t)(ok[k] ? qx : (int)x);
            Gq[k] = a.G[q];
            Sq[k] = a.S[q];
            vtq[k] = a.vt[q];
        }
#pragma unroll
        for (int k = 0; k < 5; k++) dv_tap<LAST>(a, Gp, Sp, vtp, zden, h5[dy + 2] * h5[k], Gq[k], Sq[k], vtq[k], ok[k], s);
    }
    dv_write<LAST>(a, p, s);
}

// The staged kernel for the steps 1 and 2: the block's 32 x 8 pixels and a halo of 2 STEP on every side, three planes, in LDS; the 25 taps
// of neighbouring lanes overlap there.  An entry outside the image is a guide depth of 0, which the taps' select skips as the direct
// kernel skips the tap: the sums see the same terms in the same order.
template <bool LAST, int STEP>
__global__ __launch_bounds__(DV_BX * DV_BY) void k_dv_pass_lds(const DvPass a) {
    constexpr int HX = DV_BX + 4 * STEP, HY = DV_BY + 4 * STEP;
    __shared__ float4 sG[HY * HX], sS[HY * HX];
    __shared__ float sV[HY * HX];
    const int bx0 = (int)(blockIdx.x * DV_BX) - 2 * STEP, by0 = (int)(blockIdx.y * DV_BY) - 2 * STEP;
    for (int i = threadIdx.y * DV_BX + threadIdx.x; i < HX * HY; i += DV_BX * DV_BY) {
        const int ly = i / HX, lx = i - ly * HX, gx = bx0 + lx, gy = by0 + ly;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), s = g;
        float v = 0.0f;
        if (gx >= 0 && gx < (int)a.w && gy >= 0 && gy < (int)a.h) {
            const size_t q = (size_t)gy * a.w + gx;
            g = a.G[q]; s = a.S[q]; v = a.vt[q];
        }
        sG[i] = g; sS[i] = s; sV[i] = v;
    }
    __syncthreads();
    const uint32_t x = blockIdx.x * DV_BX + threadIdx.x, y = blockIdx.y * DV_BY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const int c = ((int)threadIdx.y + 2 * STEP) * HX + (int)threadIdx.x + 2 * STEP;
    const float4 Gp = sG[c];
    if (!(Gp.w > 0.0f)) {
        if (LAST) a.out[p] = a.color[p];
        return;
    }
    const float4 Sp = sS[c];
    const float vtp = sV[c];
    const float zden = a.zk * Gp.w + 1e-6f;
    const float h5[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    DvSums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int l = c + dy * STEP * HX + (k - 2) * STEP;
            dv_tap<LAST>(a, Gp, Sp, vtp, zden, h5[dy + 2] * h5[k], sG[l], sS[l], sV[l], true, s);
        }
    }
    dv_write<LAST>(a, p, s);
}

}  // namespace

// ping / pong / guide: w * h float4 each, vt: w * h floats (context-owned scratch); out may be color.  iterations >= 1 (the entry point answers 0
// with a copy).  counts: the tiles' counts on the device, or nullptr for `samples` everywhere.
static hipError_t launch_denoise_variance(const pt_denoise_variance_config& cfg, const float4* color, const float4* albedo, const float4* normal_depth,
                                          const float4* variance, uint32_t w, uint32_t h, const uint32_t* counts, uint32_t samples, float4* out,
                                          float4* ping, float4* pong, float4* guide, float* vt, hipStream_t stream) {
    const dim3 block(DV_BX, DV_BY), grid((w + DV_BX - 1) / DV_BX, (h + DV_BY - 1) / DV_BY);
    k_dv_prepare<<<grid, block, 0, stream>>>(color, albedo, normal_depth, variance, w, h, (w + PT_TILE - 1) / PT_TILE, counts, samples,
                                             cfg.demodulate != 0, ping, guide);
    float4 *src = ping, *dst = pong;
    for (int i = 0; i < cfg.iterations; i++) {
        DvPass a;
        a.S = src; a.G = guide; a.vt = vt; a.dst = dst; a.w = w; a.h = h;
        a.step = 1 << i;
        a.normal_squarings = cfg.normal_power_log2;
        a.zk = cfg.sigma_depth * (float)a.step;
        a.sv2 = cfg.sigma_variance * cfg.sigma_variance;
        a.color_on = cfg.sigma_variance != 0.0f;
        a.color = color; a.albedo = albedo; a.out = out; a.demodulate = cfg.demodulate != 0;
        k_dv_prefilter<<<grid, block, 0, stream>>>(src, guide, w, h, vt);
        const bool last = i == cfg.iterations - 1;
        if (i == 0 && last) k_dv_pass_lds<true, 1><<<grid, block, 0, stream>>>(a);
        else if (i == 0) k_dv_pass_lds<false, 1><<<grid, block, 0, stream>>>(a);
        else if (i == 1 && last) k_dv_pass_lds<true, 2><<<grid, block, 0, stream>>>(a);
        else if (i == 1) k_dv_pass_lds<false, 2><<<grid, block, 0, stream>>>(a);
        else if (last) k_dv_pass<true><<<grid, block, 0, stream>>>(a);
        else k_dv_pass<false><<<grid, block, 0, stream>>>(a);
        float4* t = src; src = dst; dst = t;
    }
    return hipGetLastError();
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_denoise_variance(pt_ctx* ctx, const pt_denoise_variance_config* config, const void* color, const void* albedo, const void* normal_depth,
                        const void* variance, uint32_t width, uint32_t height, const uint32_t* tile_samples, uint32_t samples, void* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!color || !albedo || !normal_depth || !variance || !out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: bad size");
    const uint64_t tiles_x = (width + PT_TILE - 1) / PT_TILE, tiles_y = (height + PT_TILE - 1) / PT_TILE, tiles = tiles_x * tiles_y;
    if (tiles > 0x7fffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: more than 2^31 - 1 tiles");
    pt_denoise_variance_config cfg = {5, 1, 7, 0.02f, 4.0f};
    if (config) cfg = *config;
    if (cfg.iterations < 0 || cfg.iterations > 6) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: iterations outside 0..6");
    if (cfg.normal_power_log2 < 0 || cfg.normal_power_log2 > 10) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: normal_power_log2 outside 0..10");
    if (!std::isfinite(cfg.sigma_depth) || !(cfg.sigma_depth > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: sigma_depth must be finite and > 0");
    if (!std::isfinite(cfg.sigma_variance) || cfg.sigma_variance < 0.0f) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: sigma_variance must be finite and >= 0");
    if (!tile_samples && samples < 2u) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: samples < 2 (a single sample has no variance)");
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    if (ranges_overlap(out, bytes, albedo, bytes) || ranges_overlap(out, bytes, normal_depth, bytes) || ranges_overlap(out, bytes, variance, bytes))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: out aliases a guide image or the variance");
    if (out != color && ranges_overlap(out, bytes, color, bytes)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "denoise_variance: out overlaps color without being color");
    ENTER(ctx);
    if (cfg.iterations == 0) {                  // the identity: a copy, or nothing in place
        if (out != color) HIPOK(hipMemcpyAsync(out, color, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PT_OK;
    }
    // the scratch: two signal images, the guide image, the plane of vt, the tiles' counts; for this size alone
    const size_t need = 3 * bytes + n * sizeof(float) + (size_t)tiles * sizeof(uint32_t);
    if (need != ctx->d_denoise_variance.cap) {
        if (const hipError_t e = ctx->d_denoise_variance.realloc(ctx->stream, need)) return grow_failed(ctx, e, "denoise_variance: " + std::to_string(need) + " bytes of scratch");
    }
    float4* s = ctx->d_denoise_variance.as<float4>();
    float* vt = (float*)(s + 3 * n);
    uint32_t* d_counts = tile_samples ? (uint32_t*)(vt + n) : nullptr;
    // through a pinned slot: the caller's counts are consumed before this call returns
    if (d_counts) HIPOK(staged_upload(ctx, d_counts, tile_samples, (size_t)tiles * sizeof(uint32_t)));
    HIPOK(launch_denoise_variance(cfg, (const float4*)color, (const float4*)albedo, (const float4*)normal_depth, (const float4*)variance, width, height,
                                  d_counts, samples, (float4*)out, s, s + n, s + 2 * n, vt, ctx->stream));
    return PT_OK;
}

}  // extern "C"
