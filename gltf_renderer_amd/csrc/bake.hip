// bake.hip -- texture-space baking (pt_set_bake, include/mipt.h): the coverage map's UV rasteriser, pt_bake_dilate's passes, and the host side:
// the setter, bake_setup -- which rebuilds the map when it no longer stands for the call's atlas size, config and state of the tree (pt_ctx's
// bake_ready, bake_w / bake_h, bake_built, bake_accel), for pt_trace and the hook pt_debug_bake_rays -- and the two entry points that read it.
//
// Coverage: which triangle owns each texel of the W x H atlas -- the covering triangle with the least (instance, primitive) pair.  The
// rasteriser runs over the built tree's TriPacket / ShadePacket arrays (UVs and ids are de-indexed there).  A chart may be two triangles
// that cover the whole atlas or 250 k triangles of a few texels each, so the unit of work is neither the triangle nor the texel but a BIN:
// a triangle's clipped bounding box cut into pieces of at most 64 x 64 texels.
//   k_bake_count    per triangle: its number of bins (0: not selected, no UV stream, a skip test, or off the atlas); their sum
//   exclusive scan  (sort_scan.hip) -> the first bin of every triangle
//   k_bake_bins<0>  one wave64 per bin: finds its triangle by bisection of the scan, walks the bin's texels row-major (lane = consecutive
//                   texels of a row: the atomics and stores of a wave coalesce) and takes the 64-bit minimum of (instance << 32 | primitive)
//                   on every covered texel
//   k_bake_bins<1>  the same walk again: the triangle whose key the texel holds writes its index into the owner map.  (instance, primitive)
//                   names one triangle, so a texel has one writer and the map depends on neither triangle order nor scheduling.
// Compiled without floating-point contraction (Makefile): the edge functions are pt_bake.h's, rounding for rounding tests/bake_ref.py's.
#include <cmath>

#include "pt_ctx.h"
#include "pt_bake.h"

namespace pt {
namespace {

constexpr int kBin = 64;                       // a bin's edge in texels

// The bins of triangle t: its UV triangle, its key and its bounding box on the atlas, widened by a texel (the cover test decides, not the
// box) and clipped: texels [x0, x1) x [y0, y1).  false: the triangle takes no part.
struct BinBox { uint32_t x0, y0, x1, y1, nbx, nby; };
__device__ __forceinline__ uint32_t clip_lo(float v, uint32_t n) { return (uint32_t)fminf(fmaxf(floorf(v) - 1.0f, 0.0f), (float)n); }
__device__ __forceinline__ uint32_t clip_hi(float v, uint32_t n) { return (uint32_t)fminf(fmaxf(floorf(v) + 2.0f, 0.0f), (float)n); }
__device__ __forceinline__ bool bake_tri_setup(const BakeRaster& a, uint32_t t, BakeTri& bt, unsigned long long& key, BinBox& box) {
    const float4* tp = (const float4*)(a.tris + t);
    const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
    const uint32_t inst = __float_as_uint(q0.w), prim = __float_as_uint(q1.w);
    if (a.instance >= 0 && inst != (uint32_t)a.instance) return false;
    if (a.instances[inst].p_texcoord[a.tex_coord] == nullptr) return false;
    if (!bake_tri_uv(a.shade + t, a.tex_coord, a.w, a.h, bt)) return false;                    // skip test 1
    vec3 n; float len;
    if (!bake_normal(v3(q1.x, q1.y, q1.z), v3(q2.x, q2.y, q2.z), n, len)) return false;        // skip test 2
    key = ((unsigned long long)inst << 32) | prim;
    box.x0 = clip_lo(fminf(fminf(bt.A.x, bt.B.x), bt.C.x), a.w); box.x1 = clip_hi(fmaxf(fmaxf(bt.A.x, bt.B.x), bt.C.x), a.w);
    box.y0 = clip_lo(fminf(fminf(bt.A.y, bt.B.y), bt.C.y), a.h); box.y1 = clip_hi(fmaxf(fmaxf(bt.A.y, bt.B.y), bt.C.y), a.h);
    if (box.x0 >= box.x1 || box.y0 >= box.y1) return false;
    box.nbx = (box.x1 - box.x0 + kBin - 1) / kBin; box.nby = (box.y1 - box.y0 + kBin - 1) / kBin;
    return true;
}

__global__ __launch_bounds__(256) void k_bake_count(BakeRaster a, uint32_t* __restrict__ counts, unsigned long long* __restrict__ total) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = 0;
    if (t < a.n_tris) {
        BakeTri bt; unsigned long long key; BinBox box;
        if (bake_tri_setup(a, t, bt, key, box)) n = box.nbx * box.nby;
        counts[t] = n;
    }
    unsigned long long sum = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(total, sum);
}

template <int PASS>
__global__ __launch_bounds__(256) void k_bake_bins(BakeRaster a, const uint32_t* __restrict__ first_bin, uint32_t n_bins, unsigned long long* __restrict__ keys,
                                                   uint32_t* __restrict__ owner) {
    const uint32_t bin = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (bin >= n_bins) return;                                   // (wave-uniform)
    // the last triangle whose first bin is <= bin: triangles without bins share their successor's first bin and lose the bisection
    uint32_t lo = 0, hi = a.n_tris;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first_bin[mid] <= bin) lo = mid; else hi = mid;
    }
    const uint32_t t = lo;
    BakeTri bt; unsigned long long key; BinBox box;
    if (!bake_tri_setup(a, t, bt, key, box)) return;             // (cannot happen: the triangle has bins)
    const uint32_t k = bin - first_bin[t];
    if (k >= box.nbx * box.nby) return;
    const uint32_t by = k / box.nbx, bx = k - by * box.nbx;
    const uint32_t X0 = box.x0 + bx * kBin, Y0 = box.y0 + by * kBin;
    const uint32_t bw = min(box.x1 - X0, (uint32_t)kBin), bh = min(box.y1 - Y0, (uint32_t)kBin);
    for (uint32_t i = lane; i < bw * bh; i += 64) {
        const uint32_t ry = i / bw, x = X0 + (i - ry * bw), y = Y0 + ry;      // x < a.w, y < a.h: the box is clipped
        const vec2 p = {(float)x + 0.5f, (float)y + 0.5f};
        if (!bake_covers(bt, p)) continue;
        const size_t at = (size_t)y * a.w + x;
        if (PASS == 0) atomicMin(&keys[at], key);
        else if (keys[at] == key) owner[at] = t;
    }
}

// ---- pt_bake_dilate: one pass per launch, image and fill mask ping-pong
__global__ __launch_bounds__(256) void k_bake_mask(const uint32_t* __restrict__ owner, size_t n, uint8_t* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mask[i] = owner[i] != kBakeNone ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_bake_dilate(const float4* __restrict__ src, const uint8_t* __restrict__ msrc, uint32_t w, uint32_t h, float4* __restrict__ dst,
                                                     uint8_t* __restrict__ mdst) {
    const uint32_t x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    float4 v = src[p];
    uint8_t filled = msrc[p];
    if (!filled) {
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int count = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                if (dx == 0 && dy == 0) continue;
                const int qx = (int)x + dx, qy = (int)y + dy;
                if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) continue;
                const size_t q = (size_t)qy * w + qx;
                if (!msrc[q]) continue;                            // an unfilled texel is never read as a neighbour
                const float4 c = src[q];
                s.x = s.x + c.x; s.y = s.y + c.y; s.z = s.z + c.z; s.w = s.w + c.w;
                count++;
            }
        if (count > 0) {
            const float n = (float)count;
            v = make_float4(s.x / n, s.y / n, s.z / n, s.w / n);
            filled = 1;
        }
    }
    dst[p] = v;
    mdst[p] = filled;
}

}  // namespace

// scratch: counts[n], first_bin[n], the total (8 B), the scan's temporaries
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t bake_coverage_scratch_bytes(uint32_t n_tris) {
    const size_t n = n_tris ? n_tris : 1;
    return 2 * up256(n * 4) + 256 + up256(exclusive_scan_temp_bytes(n));
}

hipError_t bake_coverage_build(const BakeRaster& r, unsigned long long* keys, uint32_t* owner, void* scratch, hipStream_t stream, std::string& why) {
    why.clear();
    const size_t texels = (size_t)r.w * r.h;
    hipError_t e = hipMemsetAsync(keys, 0xff, texels * 8, stream);
    if (!e) e = hipMemsetAsync(owner, 0xff, texels * 4, stream);
    if (e || r.n_tris == 0) return e;
    char* p = (char*)scratch;
    uint32_t* counts = (uint32_t*)p; p += up256((size_t)r.n_tris * 4);
    uint32_t* first_bin = (uint32_t*)p; p += up256((size_t)r.n_tris * 4);
    unsigned long long* d_total = (unsigned long long*)p; p += 256;
    if ((e = hipMemsetAsync(d_total, 0, 8, stream))) return e;
    const dim3 tri_grid((r.n_tris + 255) / 256);
    hipLaunchKernelGGL(k_bake_count, tri_grid, dim3(256), 0, stream, r, counts, d_total);
    if ((e = exclusive_scan_u32(p, counts, first_bin, r.n_tris, stream))) return e;
    unsigned long long total = 0;
    if ((e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream))) return e;
    if ((e = hipStreamSynchronize(stream))) return e;
    if (total == 0) return hipSuccess;
    if (total > 0x7fffffffull) { why = "the charts' bounding boxes make " + std::to_string(total) + " bins (limit 2^31 - 1)"; return hipErrorInvalidValue; }
    const dim3 bin_grid((uint32_t)((total + 3) / 4));
    hipLaunchKernelGGL(k_bake_bins<0>, bin_grid, dim3(256), 0, stream, r, first_bin, (uint32_t)total, keys, owner);
    hipLaunchKernelGGL(k_bake_bins<1>, bin_grid, dim3(256), 0, stream, r, first_bin, (uint32_t)total, keys, owner);
    return hipGetLastError();
}

hipError_t launch_bake_dilate(float4* image, const uint32_t* owner, uint32_t w, uint32_t h, int passes, float4* pong, uint8_t* mask, hipStream_t stream) {
    const size_t n = (size_t)w * h;
    hipLaunchKernelGGL(k_bake_mask, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, owner, n, mask);
    const dim3 block(16, 16), grid((w + 15) / 16, (h + 15) / 16);
    float4 *src = image, *dst = pong;
    uint8_t *msrc = mask, *mdst = mask + n;
    for (int i = 0; i < passes; i++) {
        hipLaunchKernelGGL(k_bake_dilate, grid, block, 0, stream, src, msrc, w, h, dst, mdst);
        float4* t = src; src = dst; dst = t;
        uint8_t* m = msrc; msrc = mdst; mdst = m;
    }
    if (src != image) { const hipError_t e = hipMemcpyAsync(image, src, n * 16, hipMemcpyDeviceToDevice, stream); if (e) return e; }
    return hipGetLastError();
}

int bake_setup(pt_ctx* ctx, uint32_t width, uint32_t height, BakeArgs& bake) {
    const uint64_t accel = (uint64_t)ctx->accel_builds + ctx->accel_refits;
    const size_t texels = (size_t)width * height;
    if (!ctx->bake_ready || ctx->bake_w != width || ctx->bake_h != height || memcmp(&ctx->bake_built, &ctx->bake, sizeof(pt_bake_config)) != 0 || ctx->bake_accel != accel) {
        ctx->bake_ready = false;
        hipError_t e = ctx->d_bake_keys.reserve(ctx->stream, texels * 8, texels * 8);
        if (e == hipSuccess) e = ctx->d_bake_owner.reserve(ctx->stream, texels * 4, texels * 4);
        const size_t scratch = bake_coverage_scratch_bytes(ctx->n_tris);
        if (e == hipSuccess) e = ctx->d_bake_scratch.reserve(ctx->stream, scratch, scratch + scratch / 8);
        if (e != hipSuccess) return grow_failed(ctx, e, "bake coverage map: " + std::to_string(texels * 12 + scratch) + " bytes");
        const BakeRaster r = {ctx->d_tris.as<TriPacket>(), ctx->d_shade.as<ShadePacket>(), ctx->d_instances.as<InstanceRec>(), ctx->n_tris, width, height,
                              ctx->bake.tex_coord, ctx->bake.instance};
        std::string why;
        e = bake_coverage_build(r, ctx->d_bake_keys.as<unsigned long long>(), ctx->d_bake_owner.as<uint32_t>(), ctx->d_bake_scratch.ptr, ctx->stream, why);
        if (e != hipSuccess) return why.empty() ? ctx->fail(PT_ERR_DEVICE, std::string("bake coverage map: ") + hipGetErrorString(e)) : ctx->fail(PT_ERR_CAPACITY, "bake coverage map: " + why);
        ctx->bake_w = width; ctx->bake_h = height; ctx->bake_built = ctx->bake; ctx->bake_accel = accel; ctx->bake_ready = true;
    }
    bake.owner = ctx->d_bake_owner.as<uint32_t>(); bake.tris = ctx->d_tris.as<TriPacket>(); bake.shade = ctx->d_shade.as<ShadePacket>();
    bake.surface_offset = ctx->bake.surface_offset; bake.tex_coord = ctx->bake.tex_coord;
    return PT_OK;
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_set_bake(pt_ctx* ctx, const pt_bake_config* config) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!config) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: config is NULL");
    if (config->enable) {
        if (config->tex_coord != 0 && config->tex_coord != 1) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: tex_coord must be 0 or 1");
        if (config->instance < -1) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: instance must be -1 or a row of the instance table");
        if (!std::isfinite(config->surface_offset) || !(config->surface_offset > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: surface_offset must be finite and > 0");
        if (ctx->probes.enable) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: probes are enabled (pt_set_probes): a trace renders one atlas or the other");
    }
    ctx->bake = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_bake_coverage(pt_ctx* ctx, uint32_t width, uint32_t height, int32_t* instance_out, uint32_t* primitive_out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->bake_ready) return ctx->fail(PT_ERR_NOT_READY, "no bake trace yet");
    if (width != ctx->bake_w || height != ctx->bake_h) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake_coverage: size differs from the coverage map's");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    const size_t n = (size_t)width * height;
    std::vector<unsigned long long> keys(n);
    HIPOK(hipMemcpy(keys.data(), ctx->d_bake_keys.ptr, n * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        const bool none = keys[i] == ~0ull;
        if (instance_out) instance_out[i] = none ? -1 : (int32_t)(keys[i] >> 32);
        if (primitive_out) primitive_out[i] = none ? 0xffffffffu : (uint32_t)keys[i];
    }
    return PT_OK;
}

int pt_bake_dilate(pt_ctx* ctx, void* image, uint32_t width, uint32_t height, int passes) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!image) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake_dilate: null image");
    if (width == 0 || height == 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake_dilate: bad size");
    if (passes < 1 || passes > 64) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake_dilate: passes outside 1..64");
    if (!ctx->bake_ready) return ctx->fail(PT_ERR_NOT_READY, "no bake trace yet");
    if (width != ctx->bake_w || height != ctx->bake_h) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake_dilate: size differs from the coverage map's");
    ENTER(ctx);
    const size_t n = (size_t)width * height, need = n * 16 + 2 * n;
    if (const hipError_t e = ctx->d_bake_dilate.reserve(ctx->stream, need, need)) return grow_failed(ctx, e, "bake_dilate scratch: " + std::to_string(need) + " bytes");
    HIPOK(launch_bake_dilate((float4*)image, ctx->d_bake_owner.as<uint32_t>(), width, height, passes, ctx->d_bake_dilate.as<float4>(),
                             ctx->d_bake_dilate.as<uint8_t>() + n * 16, ctx->stream));
    return PT_OK;
}

}  // extern "C"
