// denoise.hip -- pt_denoise and pt_denoise_variance: one edge-avoiding a-trous filter over the first-hit AOVs, written once (include/mipt.h
// states both operation by operation; tests/denoise_ref.py and tests/denoise_variance_ref.py restate them in numpy).  The guides, the taps,
// the edge terms, the validity rule and the last pass are the same; VAR = false is pt_denoise, whose signal carries its luminance sum and
// whose colour term is normalised by it, VAR = true is pt_denoise_variance, the spatial filter of SVGF, whose signal carries the measured
// variance of the pixels' means from pass to pass and whose colour term is normalised by that.  Launches on the context's stream:
//   k_at_prepare<VAR>   per pixel: the demodulated signal (S.rgb, and in S.w: L = (S.r + S.g) + S.b, or the variance v of the mean) and the
//                       guide (unit normal, depth); an invalid pixel gets a guide depth of 0, which is how the other kernels tell (a valid
//                       depth is > 0)
//   k_at_prefilter      VAR, before pass i: vt = the 3 x 3 binomial mean of v over the valid taps, into a plane of its own
//   k_at_pass<VAR>      pass i: 25 taps at spacing 2^i, dy outer, dx inner, sequential sums of w, w S and (VAR) (w w) v -- from one signal
//                       image to the other
//   k_at_pass<VAR, 1>   the last pass, which multiplies the albedo back and writes the caller's image (invalid pixels: the input's bits);
//                       nothing reads its variance, so it does not form it
//   k_at_pass_lds       VAR, the passes at spacings 1 and 2, where the taps of neighbouring lanes overlap: the block and its halo staged in
//                       LDS once, the same taps in the same order from there -- the direct kernel's bits, 7 % and 4 % faster a pass on the
//                       MI355X (profiles/EXPERIMENTS.md).  pt_denoise runs the direct kernel at every spacing: staging it is NOT MEASURED
// Compiled without floating-point contraction (Makefile), with IEEE division and square root: apart from expf the arithmetic is that of
// the float32 restatements, rounding for rounding.  (tools/denoise_host_rehearsal.py compiles the file's first anonymous namespace.)
#include <cmath>

#include "pt_ctx.h"

namespace pt {
namespace {

// A block is 32 x 8 pixels: a wave holds two rows of 32, so every tap row is two runs of 32 consecutive float4 (512 B) per image at
// every spacing, and the direct 16-byte loads are coalesced as they are.
constexpr int AT_BX = 32, AT_BY = 8;

// max(m, 1e-3) that keeps a NaN (fmaxf would drop it, and a pixel with a NaN albedo must come out invalid)
__device__ __forceinline__ float at_floor(float m) { return m < 1e-3f ? 1e-3f : m; }

__device__ __forceinline__ float3 at_albedo(const float4 A, int demodulate) {
    if (!demodulate) return make_float3(1.0f, 1.0f, 1.0f);
    const float m = 1.0f - A.w;                         // a miss counts as albedo 1
    return make_float3(at_floor(A.x + m), at_floor(A.y + m), at_floor(A.z + m));
}

// VAR: variance, and counts: one per 16 x 16 tile, row-major (nullptr: `samples` everywhere); otherwise none of the four is read
template <bool VAR>
__global__ __launch_bounds__(AT_BX * AT_BY) void k_at_prepare(const float4* __restrict__ color, const float4* __restrict__ albedo,
                                                               const float4* __restrict__ normal_depth, const float4* __restrict__ variance,
                                                               uint32_t w, uint32_t h, uint32_t tiles_x, const uint32_t* __restrict__ counts,
                                                               uint32_t samples, int demodulate, float4* __restrict__ S, float4* __restrict__ G) {
    const uint32_t x = blockIdx.x * AT_BX + threadIdx.x, y = blockIdx.y * AT_BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 C = color[p], A = albedo[p], N = normal_depth[p], V = VAR ? variance[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t count = !VAR ? 0u : counts ? counts[(size_t)(y / PT_TILE) * tiles_x + x / PT_TILE] : samples;
    const float cov = A.w;
    const float3 a = at_albedo(A, demodulate);
    const float sr = C.x / a.x, sg = C.y / a.y, sb = C.z / a.z;
    const float len = sqrtf((N.x * N.x + N.y * N.y) + N.z * N.z);
    const float nx = N.x / len, ny = N.y / len, nz = N.z / len;
    const float z = N.w / cov;
    float sw;                                           // S.w: L, VAR: the variance of the mean
    if constexpr (VAR) {
        const float k = (float)(count - 1u);            // a count below 2 is invalid whatever this gives
        const float ur = (V.x / k) / (a.x * a.x), ug = (V.y / k) / (a.y * a.y), ub = (V.z / k) / (a.z * a.z);
        sw = (ur + ug) + ub;
    } else {
        sw = (sr + sg) + sb;
    }
    const bool valid = cov > 0.0f && len > 0.0f && isfinite(z) && z > 0.0f && isfinite(sr) && isfinite(sg) && isfinite(sb) &&
                       isfinite(nx) && isfinite(ny) && isfinite(nz) && (!VAR || (count >= 2u && isfinite(sw) && sw >= 0.0f));
    S[p] = valid ? make_float4(sr, sg, sb, sw) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    G[p] = valid ? make_float4(nx, ny, nz, z) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// vt of the valid pixels (0 for the others, which nothing uses): nine taps at unit spacing, the w channels of the two images
__global__ __launch_bounds__(AT_BX * AT_BY) void k_at_prefilter(const float4* __restrict__ S, const float4* __restrict__ G, uint32_t w, uint32_t h,
                                                                 float* __restrict__ vt) {
    const uint32_t x = blockIdx.x * AT_BX + threadIdx.x, y = blockIdx.y * AT_BY + threadIdx.y;
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

struct AtPass {
    const float4* S;          // the signal of the previous pass (or of k_at_prepare)
    const float4* G;          // the guide
    const float* vt;          // VAR: the prefiltered variance of S (otherwise nullptr, never read)
    float4* dst;              // the signal this pass writes (not the last pass)
    uint32_t w, h;
    int step;                 // 2^i
    int normal_squarings;     // normal_power_log2
    float zk;                 // sigma_depth * step
    float sig2;               // (sigma_color * 2^-i)^2, VAR: sigma_variance^2
    int color_on;             // sigma_color, VAR: sigma_variance != 0
    // the last pass
    const float4* color;
    const float4* albedo;
    float4* out;
    int demodulate;
};

// Two types, not one with a member the plain filter leaves alone: a fifth float in its sums changes no arithmetic of its pass and costs it 25
// register moves (profiles/EXPERIMENTS.md)
template <bool VAR> struct AtSums { float w, r, g, b; };
template <> struct AtSums<true> { float w, r, g, b, v; };         // v: VAR alone

// One tap: its weight, and the select that adds it.  hh = h[dy] h[dx] (exact).  vtp, vtq: VAR alone.
template <bool VAR, bool LAST>
__device__ __forceinline__ void at_tap(const AtPass& a, const float4 Gp, const float4 Sp, float vtp, float zden, float hh, const float4 Gq,
                                       const float4 Sq, float vtq, bool in_image, AtSums<VAR>& s) {
    float wn = fminf(fmaxf((Gp.x * Gq.x + Gp.y * Gq.y) + Gp.z * Gq.z, 0.0f), 1.0f);
    for (int j = 0; j < a.normal_squarings; j++) wn = wn * wn;
    const float ez = fabsf(Gp.w - Gq.w) / zden;
    float ec = 0.0f;
    if (a.color_on) {
        const float dr = Sp.x - Sq.x, dg = Sp.y - Sq.y, db = Sp.z - Sq.z;
        if constexpr (VAR) {
            ec = ((dr * dr + dg * dg) + db * db) / (a.sig2 * (vtp + vtq) + 1e-8f);
        } else {
            const float ls = Sp.w + Sq.w;
            ec = ((dr * dr + dg * dg) + db * db) / (a.sig2 * (ls * ls) + 1e-8f);
        }
    }
    const float wt = (hh * wn) * expf(-(ez + ec));
    if (in_image && Gq.w > 0.0f) {              // a select: the weight of an invalid tap is never multiplied with anything
        s.w = s.w + wt;
        s.r = s.r + wt * Sq.x;
        s.g = s.g + wt * Sq.y;
        s.b = s.b + wt * Sq.z;
        if constexpr (VAR && !LAST) s.v = s.v + (wt * wt) * Sq.w;
    }
}

template <bool VAR, bool LAST>
__device__ __forceinline__ void at_write(const AtPass& a, size_t p, const AtSums<VAR>& s) {
    const float r = s.r / s.w, g = s.g / s.w, b = s.b / s.w;
    if constexpr (LAST) {
        const float3 al = at_albedo(a.albedo[p], a.demodulate);
        a.out[p] = make_float4(r * al.x, g * al.y, b * al.z, a.color[p].w);
    } else if constexpr (VAR) {
        a.dst[p] = make_float4(r, g, b, s.v / (s.w * s.w));
    } else {
        a.dst[p] = make_float4(r, g, b, (r + g) + b);
    }
}

// The direct kernel: every tap is two 16-byte global loads and (VAR) one of 4 bytes (25 x 32 or 36 B per pixel through L2), at any spacing.
template <bool VAR, bool LAST>
__global__ __launch_bounds__(AT_BX * AT_BY) void k_at_pass(const AtPass a) {
    const uint32_t x = blockIdx.x * AT_BX + threadIdx.x, y = blockIdx.y * AT_BY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    const float4 Gp = a.G[p];
    if (!(Gp.w > 0.0f)) {                       // invalid: never filtered, never a neighbour; it leaves the call with the input's bits
        if (LAST) a.out[p] = a.color[p];
        return;
    }
    const float4 Sp = a.S[p];
    const float vtp = VAR ? a.vt[p] : 0.0f;
    const float zden = a.zk * Gp.w + 1e-6f;
    const float h5[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    AtSums<VAR> s = {};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = (int)y + dy * a.step;
        if (qy < 0 || qy >= (int)a.h) continue;
        const size_t row = (size_t)qy * a.w;
        float4 Gq[5], Sq[5];
        float vtq[5];
        bool ok[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {           // the row's ten or fifteen loads first, from clamped (in-image) addresses
            const int qx = (int)x + (k - 2) * a.step;
            ok[k] = qx >= 0 && qx < (int)a.w;
            const size_t q = row + (size_t)(ok[k] ? qx : (int)x);
            Gq[k] = a.G[q];
            Sq[k] = a.S[q];
            vtq[k] = VAR ? a.vt[q] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 5; k++) at_tap<VAR, LAST>(a, Gp, Sp, vtp, zden, h5[dy + 2] * h5[k], Gq[k], Sq[k], vtq[k], ok[k], s);
    }
    at_write<VAR, LAST>(a, p, s);
}

// The staged kernel for the steps 1 and 2: the block's 32 x 8 pixels and a halo of 2 STEP on every side, three planes, in LDS; the 25 taps
// of neighbouring lanes overlap there.  An entry outside the image is a guide depth of 0, which the taps' select skips as the direct
// kernel skips the tap: the sums see the same terms in the same order.  Instantiated for VAR alone (it stages vt whatever VAR is).
template <bool VAR, bool LAST, int STEP>
__global__ __launch_bounds__(AT_BX * AT_BY) void k_at_pass_lds(const AtPass a) {
    constexpr int HX = AT_BX + 4 * STEP, HY = AT_BY + 4 * STEP;
    __shared__ float4 sG[HY * HX], sS[HY * HX];
    __shared__ float sV[HY * HX];
    const int bx0 = (int)(blockIdx.x * AT_BX) - 2 * STEP, by0 = (int)(blockIdx.y * AT_BY) - 2 * STEP;
    for (int i = threadIdx.y * AT_BX + threadIdx.x; i < HX * HY; i += AT_BX * AT_BY) {
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
    const uint32_t x = blockIdx.x * AT_BX + threadIdx.x, y = blockIdx.y * AT_BY + threadIdx.y;
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
    AtSums<VAR> s = {};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int l = c + dy * STEP * HX + (k - 2) * STEP;
            at_tap<VAR, LAST>(a, Gp, Sp, vtp, zden, h5[dy + 2] * h5[k], sG[l], sS[l], sV[l], true, s);
        }
    }
    at_write<VAR, LAST>(a, p, s);
}

}  // namespace

namespace {        // the host side: the namespace above is what the rehearsal compiles

// A filter's config as both entry points hand it over: sigma is sigma_color, VAR: sigma_variance
struct AtConfig { int iterations, demodulate, normal_power_log2; float sigma_depth, sigma; };

// ping / pong / guide: w * h float4 each, VAR: vt: w * h floats (context-owned scratch); out may be color.  iterations >= 1.  VAR: counts: the
// tiles' counts on the device, or nullptr for `samples` everywhere.  The variance filter stages its passes at spacings 1 and 2.  Asynchronous.
template <bool VAR>
hipError_t launch_atrous(const AtConfig& cfg, const float4* color, const float4* albedo, const float4* normal_depth, const float4* variance,
                         uint32_t w, uint32_t h, const uint32_t* counts, uint32_t samples, float4* out, float4* ping, float4* pong, float4* guide,
                         float* vt, hipStream_t stream) {
    const dim3 block(AT_BX, AT_BY), grid((w + AT_BX - 1) / AT_BX, (h + AT_BY - 1) / AT_BY);
    k_at_prepare<VAR><<<grid, block, 0, stream>>>(color, albedo, normal_depth, variance, w, h, (w + PT_TILE - 1) / PT_TILE, counts, samples,
                                                  cfg.demodulate != 0, ping, guide);
    float4 *src = ping, *dst = pong;
    for (int i = 0; i < cfg.iterations; i++) {
        AtPass a;
        a.S = src; a.G = guide; a.vt = vt; a.dst = dst; a.w = w; a.h = h;
        a.step = 1 << i;
        a.normal_squarings = cfg.normal_power_log2;
        a.zk = cfg.sigma_depth * (float)a.step;
        const float sig = VAR ? cfg.sigma : cfg.sigma * ldexpf(1.0f, -i);
        a.sig2 = sig * sig;
        a.color_on = cfg.sigma != 0.0f;
        a.color = color; a.albedo = albedo; a.out = out; a.demodulate = cfg.demodulate != 0;
        if (VAR) k_at_prefilter<<<grid, block, 0, stream>>>(src, guide, w, h, vt);
        const bool last = i == cfg.iterations - 1;
        if (VAR && i == 0 && last) k_at_pass_lds<true, true, 1><<<grid, block, 0, stream>>>(a);
        else if (VAR && i == 0) k_at_pass_lds<true, false, 1><<<grid, block, 0, stream>>>(a);
        else if (VAR && i == 1 && last) k_at_pass_lds<true, true, 2><<<grid, block, 0, stream>>>(a);
        else if (VAR && i == 1) k_at_pass_lds<true, false, 2><<<grid, block, 0, stream>>>(a);
        else if (last) k_at_pass<VAR, true><<<grid, block, 0, stream>>>(a);
        else k_at_pass<VAR, false><<<grid, block, 0, stream>>>(a);
        float4* t = src; src = dst; dst = t;
    }
    return hipGetLastError();
}

// What the entry points share: the checks in their order, the identity, the scratch and the launches.  who: "denoise" or "denoise_variance", the
// prefix of every text; sigma_name: the config's name for cfg.sigma.  VAR alone: variance, tile_samples, samples.  (The entry points read the
// caller's config before they come here; reading it refuses nothing, so the refusals keep their order.)
template <bool VAR>
int atrous(pt_ctx* ctx, const char* who, const char* sigma_name, DevBuf& scratch, const AtConfig& cfg, const void* color, const void* albedo,
           const void* normal_depth, const void* variance, uint32_t width, uint32_t height, const uint32_t* tile_samples, uint32_t samples, void* out) {
    const auto bad = [&](const char* what) { return ctx->fail(PT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
    if (!color || !albedo || !normal_depth || (VAR && !variance) || !out) return bad("null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return bad("bad size");
    const uint64_t tiles_x = (width + PT_TILE - 1) / PT_TILE, tiles_y = (height + PT_TILE - 1) / PT_TILE, tiles = tiles_x * tiles_y;
    if (VAR && tiles > 0x7fffffffull) return bad("more than 2^31 - 1 tiles");
    if (cfg.iterations < 0 || cfg.iterations > 6) return bad("iterations outside 0..6");
    if (cfg.normal_power_log2 < 0 || cfg.normal_power_log2 > 10) return bad("normal_power_log2 outside 0..10");
    if (!std::isfinite(cfg.sigma_depth) || !(cfg.sigma_depth > 0.0f)) return bad("sigma_depth must be finite and > 0");
    if (!std::isfinite(cfg.sigma) || cfg.sigma < 0.0f) return bad((std::string(sigma_name) + " must be finite and >= 0").c_str());
    if (VAR && !tile_samples && samples < 2u) return bad("samples < 2 (a single sample has no variance)");
    const size_t n = (size_t)width * height, bytes = n * sizeof(float4);
    if (ranges_overlap(out, bytes, albedo, bytes) || ranges_overlap(out, bytes, normal_depth, bytes) || (VAR && ranges_overlap(out, bytes, variance, bytes)))
        return bad(VAR ? "out aliases a guide image or the variance" : "out aliases a guide image");
    if (out != color && ranges_overlap(out, bytes, color, bytes)) return bad("out overlaps color without being color");
    ENTER(ctx);
    if (cfg.iterations == 0) {                  // the identity: a copy, or nothing in place
        if (out != color) HIPOK(hipMemcpyAsync(out, color, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PT_OK;
    }
    // the scratch: two signal images and the guide image, VAR: the plane of vt and the tiles' counts
    const size_t need = 3 * bytes + (VAR ? n * sizeof(float) + (size_t)tiles * sizeof(uint32_t) : 0);
    if (const int rc = exact_scratch(ctx, scratch, need, who)) return rc;
    float4* s = scratch.as<float4>();
    float* vt = VAR ? (float*)(s + 3 * n) : nullptr;
    uint32_t* d_counts = VAR && tile_samples ? (uint32_t*)(vt + n) : nullptr;
    // through a pinned slot: the caller's counts are consumed before this call returns
    if (d_counts) HIPOK(staged_upload(ctx, d_counts, tile_samples, (size_t)tiles * sizeof(uint32_t)));
    HIPOK(launch_atrous<VAR>(cfg, (const float4*)color, (const float4*)albedo, (const float4*)normal_depth, (const float4*)variance, width, height, d_counts,
                             samples, (float4*)out, s, s + n, s + 2 * n, vt, ctx->stream));
    return PT_OK;
}

}  // namespace
}  // namespace pt

using namespace pt;

extern "C" {

int pt_denoise(pt_ctx* ctx, const pt_denoise_config* config, const void* color, const void* albedo, const void* normal_depth,
               uint32_t width, uint32_t height, void* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    AtConfig cfg = {5, 1, 7, 0.02f, 1.0f};
    if (config) cfg = {config->iterations, config->demodulate, config->normal_power_log2, config->sigma_depth, config->sigma_color};
    return atrous<false>(ctx, "denoise", "sigma_color", ctx->d_denoise, cfg, color, albedo, normal_depth, nullptr, width, height, nullptr, 0, out);
}

int pt_denoise_variance(pt_ctx* ctx, const pt_denoise_variance_config* config, const void* color, const void* albedo, const void* normal_depth,
                        const void* variance, uint32_t width, uint32_t height, const uint32_t* tile_samples, uint32_t samples, void* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    AtConfig cfg = {5, 1, 7, 0.02f, 4.0f};
    if (config) cfg = {config->iterations, config->demodulate, config->normal_power_log2, config->sigma_depth, config->sigma_variance};
    return atrous<true>(ctx, "denoise_variance", "sigma_variance", ctx->d_denoise_variance, cfg, color, albedo, normal_depth, variance, width, height,
                        tile_samples, samples, out);
}

}  // extern "C"
