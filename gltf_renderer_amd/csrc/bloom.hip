// bloom.hip -- pt_bloom: the reference's dual-filter bloom (Bloom::Execute, Source/Bloom.cpp:57-164) over a mip pyramid (include/mipt.h states
// it operation by operation; tests/bloom_ref.py restates it in numpy float32, rounding for rounding).  A pure function of one image.  2 n
// launches on the context's stream for n levels, one lane per output texel, one 256-lane workgroup per 16 x 16 tile (PT_TILE), tiles
// numbered row-major, so that a wave's taps fall on neighbouring texels:
//   k_bloom_down<FIRST>  M_k = down(M_{k-1}); the first instance reads `color` and applies the prefilter to each texel as it is fetched
//   k_bloom_up<LAST>     M_i = up(M_{i+1}), replacing M_i; the last instance is at full size and writes out = color + strength * U, or the
//                        copy of a pixel with a non-finite colour.  It reads the pyramid and the lane's own pixel only, so out may be color.
// A level's texels are float4 (w = 0) for 16-byte loads and stores.  The three x and three y coordinates of a step's taps are turned into
// (texel, texel, fraction) once per lane; a tap is then four loads and three lerps a channel.
//   The first down and the last up step carry most of the bytes, and their workgroups stage the tile's input footprint in LDS first: at most
// 36 x 36 texels of `color`, prefiltered once each where a lane's taps would prefilter each of their 20 fetches, and at most 12 x 12
// texels of M_1.  The taps then read LDS.  Same arithmetic, same order; 0.0900 -> 0.0766 ms at 1920 x 1080 (profiles/EXPERIMENTS.md).
// Compiled without floating-point contraction (Makefile), with IEEE division.
#include <cmath>

#include "pt_ctx.h"

namespace pt {
namespace {

constexpr int kBloomTile = PT_TILE, kBloomLanes = PT_TILE * PT_TILE;
constexpr int kBloomMaxLevels = 8;
constexpr float kBloomHalfMax = 65504.0f;
// The footprint of a 16 x 16 tile, in texels a side.  Down: the taps span (15 + 1) * wi / wo + 1 texels and their neighbours, and wi / wo
// is at most 2 + 1 / 16 under a whole tile: 36.  Up: (15 + 2) * wi / wo + 1 with wi / wo at most 1 / 2: 11.  A search over every width
// up to 20 000 and every 997th up to 2 000 000 found 35 and 11.  Above 2^24 texels a side float32 coordinates no longer resolve texels
// and a footprint comes out larger (38 for the down step at 2^25 - 3; 66 and 34 at 2^30 - 3): such a tile takes its taps from memory.
constexpr int kBloomPatchDown = 36, kBloomPatchUp = 12;

struct BloomAxis { int i0, i1; float f; };
struct BloomAxes { BloomAxis m, c, p; };                 // at u - o, u, u + o
struct BloomRgb { float r, g, b; };

// One axis of the bilinear tap at coordinate u of a level n texels long, clamp addressing.  i0 and i1 do not decrease as u grows.
__device__ __forceinline__ BloomAxis bloom_axis(float u, uint32_t n) {
    const float s = u * (float)n - 0.5f, i0f = floorf(s);
    const int i = (int)i0f, last = (int)n - 1;
    BloomAxis a;
    a.f = s - i0f;
    a.i0 = min(max(i, 0), last); a.i1 = min(max(i + 1, 0), last);
    return a;
}

// The three coordinates of output texel x of a level no texels long, o = offset / (float)no apart, in a source level ni texels long
__device__ __forceinline__ BloomAxes bloom_axes(uint32_t x, uint32_t no, uint32_t ni, float offset) {
    const float u = ((float)x + 0.5f) / (float)no, o = offset / (float)no;
    return BloomAxes{bloom_axis(u - o, ni), bloom_axis(u, ni), bloom_axis(u + o, ni)};
}

__device__ __forceinline__ BloomAxis bloom_shift(BloomAxis a, int lo) { a.i0 -= lo; a.i1 -= lo; return a; }
__device__ __forceinline__ BloomAxes bloom_shift(const BloomAxes& a, int lo) { return BloomAxes{bloom_shift(a.m, lo), bloom_shift(a.c, lo), bloom_shift(a.p, lo)}; }

__device__ __forceinline__ float bloom_clip(float c) { return c > 0.0f ? fminf(c, kBloomHalfMax) : 0.0f; }   // a select: NaN, negatives and -0 give +0

template <bool PREFILTER>
__device__ __forceinline__ BloomRgb bloom_texel(const float4* __restrict__ T, size_t i, float threshold) {
    const float4 t = T[i];
    BloomRgb b = {t.x, t.y, t.z};
    if (PREFILTER) {
        b.r = bloom_clip(b.r); b.g = bloom_clip(b.g); b.b = bloom_clip(b.b);
        if (threshold > 0.0f) {
            const float L = fmaxf(fmaxf(b.r, b.g), b.b);
            const float k = L > threshold ? (L - threshold) / L : 0.0f;
            b.r = b.r * k; b.g = b.g * k; b.b = b.b * k;
        }
    }
    return b;
}

__device__ __forceinline__ BloomRgb bloom_lerp(const BloomRgb a, const BloomRgb b, float f) {
    return BloomRgb{a.r + f * (b.r - a.r), a.g + f * (b.g - a.g), a.b + f * (b.b - a.b)};
}
__device__ __forceinline__ BloomRgb bloom_add(const BloomRgb a, const BloomRgb b) { return BloomRgb{a.r + b.r, a.g + b.g, a.b + b.b}; }
__device__ __forceinline__ BloomRgb bloom_scale(const BloomRgb a, float k) { return BloomRgb{a.r * k, a.g * k, a.b * k}; }

// S(T, u, v) of a level (or staged patch) `w` texels wide, the axes already formed
template <bool PREFILTER>
__device__ __forceinline__ BloomRgb bloom_tap(const float4* __restrict__ T, uint32_t w, const BloomAxis X, const BloomAxis Y, float threshold) {
    const size_t r0 = (size_t)Y.i0 * w, r1 = (size_t)Y.i1 * w;
    const BloomRgb a = bloom_lerp(bloom_texel<PREFILTER>(T, r0 + X.i0, threshold), bloom_texel<PREFILTER>(T, r0 + X.i1, threshold), X.f);
    const BloomRgb b = bloom_lerp(bloom_texel<PREFILTER>(T, r1 + X.i0, threshold), bloom_texel<PREFILTER>(T, r1 + X.i1, threshold), X.f);
    return bloom_lerp(a, b, Y.f);
}

// M = (4 S(u, v) + the four taps half a texel out) / 8
template <bool PREFILTER>
__device__ __forceinline__ BloomRgb bloom_down(const float4* __restrict__ T, uint32_t w, const BloomAxes& X, const BloomAxes& Y, float threshold) {
    BloomRgb r = bloom_scale(bloom_tap<PREFILTER>(T, w, X.c, Y.c, threshold), 4.0f);
    r = bloom_add(r, bloom_tap<PREFILTER>(T, w, X.p, Y.p, threshold));
    r = bloom_add(r, bloom_tap<PREFILTER>(T, w, X.m, Y.m, threshold));
    r = bloom_add(r, bloom_tap<PREFILTER>(T, w, X.m, Y.p, threshold));
    r = bloom_add(r, bloom_tap<PREFILTER>(T, w, X.p, Y.m, threshold));
    return BloomRgb{r.r / 8.0f, r.g / 8.0f, r.b / 8.0f};
}

// U = (2 (the four taps a texel out along the axes) + the four diagonal ones) / 12
__device__ __forceinline__ BloomRgb bloom_up(const float4* __restrict__ T, uint32_t w, const BloomAxes& X, const BloomAxes& Y) {
    BloomRgb r = bloom_tap<false>(T, w, X.p, Y.c, 0.0f);
    r = bloom_add(r, bloom_tap<false>(T, w, X.m, Y.c, 0.0f));
    r = bloom_add(r, bloom_tap<false>(T, w, X.c, Y.p, 0.0f));
    r = bloom_add(r, bloom_tap<false>(T, w, X.c, Y.m, 0.0f));
    r = bloom_scale(r, 2.0f);
    r = bloom_add(r, bloom_tap<false>(T, w, X.p, Y.p, 0.0f));
    r = bloom_add(r, bloom_tap<false>(T, w, X.m, Y.p, 0.0f));
    r = bloom_add(r, bloom_tap<false>(T, w, X.p, Y.m, 0.0f));
    r = bloom_add(r, bloom_tap<false>(T, w, X.m, Y.m, 0.0f));
    return BloomRgb{r.r / 12.0f, r.g / 12.0f, r.b / 12.0f};
}

// The workgroup's tile and the lane's output texel in it.  (x0, y0) .. (x1, y1): the tile's texels on the level, the same in every lane
struct BloomTile { uint32_t x0, y0, x1, y1, x, y; bool inside; };
__device__ __forceinline__ BloomTile bloom_tile(const BloomStep& s) {
    const uint32_t t = blockIdx.x, ty = t / s.tiles_x, tx = t - ty * s.tiles_x, i = threadIdx.x;
    BloomTile b;
    b.x0 = tx * kBloomTile; b.y0 = ty * kBloomTile;
    b.x1 = min(b.x0 + kBloomTile - 1, s.wo - 1); b.y1 = min(b.y0 + kBloomTile - 1, s.ho - 1);
    b.x = b.x0 + (i & (kBloomTile - 1)); b.y = b.y0 + i / kBloomTile;
    b.inside = b.x < s.wo && b.y < s.ho;
    return b;
}

// The tile's footprint on the source level -- texels (xlo, ylo) .. (xlo + pw - 1, ylo + ph - 1): a tap's texels do not decrease with its
// coordinate (bloom_axis), so those of the first texel's least and the last texel's greatest coordinate bound every lane's -- staged
// row-major in `patch` by the whole workgroup, PREFILTER applied once per texel.  False, with nothing staged, if it exceeds P texels a
// side.  The same in every lane; all lanes of the workgroup call it.
template <bool PREFILTER, int P>
__device__ __forceinline__ bool bloom_stage(const BloomStep& s, const BloomTile& b, float offset, float4* patch, int& xlo, int& ylo, int& pw) {
    xlo = bloom_axes(b.x0, s.wo, s.wi, offset).m.i0; ylo = bloom_axes(b.y0, s.ho, s.hi, offset).m.i0;
    pw = bloom_axes(b.x1, s.wo, s.wi, offset).p.i1 - xlo + 1;
    const int ph = bloom_axes(b.y1, s.ho, s.hi, offset).p.i1 - ylo + 1;
    if (pw > P || ph > P) return false;
    for (int j = (int)threadIdx.x; j < pw * ph; j += kBloomLanes) {
        const int py = j / pw, px = j - py * pw;
        const BloomRgb t = bloom_texel<PREFILTER>(s.src, (size_t)(ylo + py) * s.wi + (size_t)(xlo + px), s.threshold);
        patch[j] = make_float4(t.r, t.g, t.b, 0.0f);
    }
    __syncthreads();
    return true;
}

template <bool FIRST>
__global__ __launch_bounds__(kBloomLanes) void k_bloom_down(const BloomStep s) {
    __shared__ float4 patch[FIRST ? kBloomPatchDown * kBloomPatchDown : 1];
    const BloomTile b = bloom_tile(s);
    int xlo = 0, ylo = 0, pw = 0;
    const bool staged = FIRST && bloom_stage<true, kBloomPatchDown>(s, b, 0.5f, patch, xlo, ylo, pw);
    if (!b.inside) return;
    const BloomAxes X = bloom_axes(b.x, s.wo, s.wi, 0.5f), Y = bloom_axes(b.y, s.ho, s.hi, 0.5f);
    const BloomRgb m = staged ? bloom_down<false>(patch, pw, bloom_shift(X, xlo), bloom_shift(Y, ylo), 0.0f)
                              : bloom_down<FIRST>(s.src, s.wi, X, Y, s.threshold);
    s.dst[(size_t)b.y * s.wo + b.x] = make_float4(m.r, m.g, m.b, 0.0f);
}

template <bool LAST>
__global__ __launch_bounds__(kBloomLanes) void k_bloom_up(const BloomStep s) {
    __shared__ float4 patch[LAST ? kBloomPatchUp * kBloomPatchUp : 1];
    const BloomTile b = bloom_tile(s);
    const size_t p = (size_t)b.y * s.wo + b.x;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (LAST && b.inside) c = s.color[p];                  // before the barrier: it has as far to come as the patch
    int xlo = 0, ylo = 0, pw = 0;
    const bool staged = LAST && bloom_stage<false, kBloomPatchUp>(s, b, 1.0f, patch, xlo, ylo, pw);
    if (!b.inside) return;
    if (LAST && !(isfinite(c.x) && isfinite(c.y) && isfinite(c.z))) {
        s.dst[p] = c;
        return;
    }
    const BloomAxes X = bloom_axes(b.x, s.wo, s.wi, 1.0f), Y = bloom_axes(b.y, s.ho, s.hi, 1.0f);
    const BloomRgb U = staged ? bloom_up(patch, pw, bloom_shift(X, xlo), bloom_shift(Y, ylo)) : bloom_up(s.src, s.wi, X, Y);
    if (LAST) s.dst[p] = make_float4(c.x + s.strength * U.r, c.y + s.strength * U.g, c.z + s.strength * U.b, c.w);
    else s.dst[p] = make_float4(U.r, U.g, U.b, 0.0f);
}

template <typename K>
void bloom_launch(K kernel, BloomStep& s, hipStream_t stream) {
    s.tiles_x = (s.wo + kBloomTile - 1) / kBloomTile;
    const uint32_t tiles = s.tiles_x * ((s.ho + kBloomTile - 1) / kBloomTile);
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kBloomLanes), 0, stream, s);
}

}  // namespace

// Levels 1 .. n of a w x h image: NextMipSize level by level, stopping after the first level that is 1 x 1.  -> n; texels = their sum
int bloom_levels(uint32_t w, uint32_t h, int iterations, uint32_t* lw, uint32_t* lh, size_t* texels) {
    int n = 0;
    *texels = 0;
    while (n < iterations && !(w == 1 && h == 1)) {
        w = w / 2 > 1 ? w / 2 : 1; h = h / 2 > 1 ? h / 2 : 1;
        lw[n] = w; lh[n] = h; *texels += (size_t)w * h;
        n++;
    }
    return n;
}

hipError_t launch_bloom(const BloomArgs& a, hipStream_t stream) {
    const float4* level[kBloomMaxLevels + 1];                  // level[0] is the image itself
    uint32_t w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
    level[0] = a.color; w[0] = a.w; h[0] = a.h;
    float4* next = a.chain;
    for (int k = 1; k <= a.n; k++) {
        level[k] = next; w[k] = a.lw[k - 1]; h[k] = a.lh[k - 1];
        next += (size_t)w[k] * h[k];
    }
    BloomStep s;
    s.color = a.color; s.strength = a.strength; s.threshold = a.threshold;
    for (int k = 1; k <= a.n; k++) {
        s.src = level[k - 1]; s.wi = w[k - 1]; s.hi = h[k - 1];
        s.dst = (float4*)level[k]; s.wo = w[k]; s.ho = h[k];
        if (k == 1) bloom_launch(k_bloom_down<true>, s, stream); else bloom_launch(k_bloom_down<false>, s, stream);
    }
    for (int i = a.n - 1; i >= 0; i--) {
        s.src = level[i + 1]; s.wi = w[i + 1]; s.hi = h[i + 1];
        s.dst = i == 0 ? a.out : (float4*)level[i]; s.wo = w[i]; s.ho = h[i];
        if (i == 0) bloom_launch(k_bloom_up<true>, s, stream); else bloom_launch(k_bloom_up<false>, s, stream);
    }
    return hipGetLastError();
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_bloom(pt_ctx* ctx, const pt_bloom_config* config, const void* color, uint32_t width, uint32_t height, void* out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!color || !out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: bad size");
    if ((uint64_t)width * height > 0x7fffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: width * height exceeds 2^31 - 1");
    pt_bloom_config cfg = {4, 0.01f, 0.0f};
    if (config) cfg = *config;
    if (cfg.iterations < 0 || cfg.iterations > kBloomMaxLevels) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: iterations outside 0..8");
    if (!std::isfinite(cfg.strength) || !(cfg.strength >= 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: strength must be finite and >= 0");
    if (!std::isfinite(cfg.threshold) || !(cfg.threshold >= 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: threshold must be finite and >= 0");
    const size_t bytes = (size_t)width * height * 16;
    if (out != color && ranges_overlap(out, bytes, color, bytes))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bloom: out overlaps color without being color");
    ENTER(ctx);
    BloomArgs a;
    size_t texels = 0;
    a.n = bloom_levels(width, height, cfg.iterations, a.lw, a.lh, &texels);
    if (a.n == 0 || cfg.strength == 0.0f) {                  // out = color, bit for bit
        if (out != color) HIPOK(hipMemcpyAsync(out, color, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PT_OK;
    }
    const size_t need = texels * 16;
    if (const int rc = exact_scratch(ctx, ctx->d_bloom, need, "bloom")) return rc;      // for this size and level count alone
    a.color = (const float4*)color; a.out = (float4*)out; a.chain = ctx->d_bloom.as<float4>();
    a.w = width; a.h = height;
    a.strength = cfg.strength; a.threshold = cfg.threshold;
    HIPOK(launch_bloom(a, ctx->stream));
    return PT_OK;
}

}  // extern "C"
