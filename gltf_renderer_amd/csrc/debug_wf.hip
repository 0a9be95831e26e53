// debug_wf.hip -- the device side of the test hooks (pt_debug_*, mipt_debug.hip) that run what the wavefront stages run, compiled as
// pt_wavefront.hip is (same Makefile flags, PT_LUT_LDS): the per-lane query kernels with their tables staged into LDS (pt_debug_kernels.h),
// the generate stage's ray functions on caller-supplied queries, and the traversal stages' launches on caller-filled queues.  No frame runs
// anything in this file.
#define PT_LUT_LDS 1          // as pt_wavefront.hip: the stage_* functions of pt_shading.h copy their tables into LDS
#include <algorithm>
#include <cstring>

#include "pt_debug_kernels.h"
#include "pt_wavefront.h"
#include "pt_workspace.h"
#include "pt_bake.h"
#include "pt_probe.h"

namespace pt {

DebugQueryLaunch debug_queries_wf() { return kDebugQueryLaunch; }
int debug_light_cache_max() { return kLightCacheMax; }
int debug_inst_cache_max() { return (int)kInstCacheMax; }
int debug_mat_cache_max() { return (int)kMatCacheMax; }

namespace {
// Test hooks (pt_debug_camera_rays, pt_debug_bake_rays, pt_debug_probe_rays): a generate kernel's ray function itself, one query
// q = {px, py, seed} per lane (for the probes the cells differ from lane to lane).  out: 8 floats per query (origin, tmin, direction, tmax); a
// query RAY_OF gives no ray keeps zeros with tmax = -1.
template <class Args, void (*RAY_OF)(const FrameConstants&, const Args&, const uint32_t* q, Ray&)>
__global__ __launch_bounds__(kBlock) void k_debug_rays(FrameConstants fc, Args args, const uint32_t* __restrict__ queries, uint32_t n, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = v3(0); r.d = v3(0); r.tmin = 0; r.tmax = -1.0f;
    RAY_OF(fc, args, queries + 3 * (size_t)i, r);
    float* o = out + (size_t)i * 8;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.tmin; o[4] = r.d.x; o[5] = r.d.y; o[6] = r.d.z; o[7] = r.tmax;
}
template <class Args, void (*RAY_OF)(const FrameConstants&, const Args&, const uint32_t*, Ray&)>
void launch_debug_rays(const FrameConstants& fc, const Args& args, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL((k_debug_rays<Args, RAY_OF>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, fc, args, d_queries, n, d_out);
}
// camera_ray under the context's lens, for every query (a pixel off the image has a ray too); bake_ray and probe_ray on the atlas only
PT_DEV void debug_camera_ray(const FrameConstants& fc, const LensArgs& lens, const uint32_t* q, Ray& r) { int rc = 0; r = camera_ray(fc, lens, q[2], q[0], q[1], rc); }
PT_DEV void debug_bake_ray(const FrameConstants& fc, const BakeArgs& bk, const uint32_t* q, Ray& r) {
    const uint32_t px = q[0], py = q[1];
    int rc = 0;
    if (px < fc.res_x && py < fc.res_y) bake_ray(fc, bk, q[2], px, py, rc, r);
}
PT_DEV void debug_probe_ray(const FrameConstants& fc, const ProbeArgs& pa, const uint32_t* q, Ray& r) {
    const uint32_t px = q[0], py = q[1];
    int rc = 0;
    if (px < fc.res_x && py < fc.res_y) probe_ray<false>(fc, pa, q[2], px, py, rc, r);
}
}  // namespace
void launch_debug_camera_rays(const FrameConstants& fc, const LensArgs& lens, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream) {
    launch_debug_rays<LensArgs, debug_camera_ray>(fc, lens, d_queries, n, d_out, stream);
}
void launch_debug_bake_rays(const FrameConstants& fc, const BakeArgs& bake, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream) {
    launch_debug_rays<BakeArgs, debug_bake_ray>(fc, bake, d_queries, n, d_out, stream);
}
void launch_debug_probe_rays(const FrameConstants& fc, const ProbeArgs& probes, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream) {
    launch_debug_rays<ProbeArgs, debug_probe_ray>(fc, probes, d_queries, n, d_out, stream);
}

// Test hook (pt_debug_trace_queues, mipt_debug.hip): the traversal kernels of a frame -- k_wf_trace, k_wf_shadow or the fused k_wf_traverse, through
// pt_wavefront.h's launch functions -- on queues the caller filled.  Owns a small WfBuffers: the seven counter arrays, one closest queue with its hit
// array, the shadow queue and the pending records, nothing else (sc.has_env must be 0, so no environment buffers are read).
// Every output word holds kDebugSentinel before the launch and each shard's segment ends in a guard entry nobody may write.
// `bounce` is the closest rays' bounce (which 0, 2) or the shadow rays' (which 1); the fused launch takes the shadow rays of bounce - 1 with it,
// as in a frame.  Synchronises the stream.
constexpr uint32_t kDebugSentinel = 0x7fc5a5a5u;           // a quiet NaN with a payload no kernel produces
hipError_t debug_trace_queues(const SceneRec& sc, const DebugQueues& q, Counters* counters, bool count, hipStream_t stream, std::string& why) {
    why.clear();
    const int cur = q.bounce & 1;                                                       // the closest queue of that bounce (launch_wavefront)
    const int shadow_bounce = q.which == 2 ? q.bounce - 1 : q.bounce;
    const int scnt = shadow_counter(shadow_bounce);
    std::vector<uint32_t> n_c(kShards, 0), n_s(kShards, 0);
    for (uint32_t i = 0; i < q.n_closest; i++) n_c[q.closest_shard[i]]++;
    for (uint32_t i = 0; i < q.n_shadow; i++) n_s[q.shadow_shard[i]]++;
    uint32_t seg = 0;
    for (uint32_t s = 0; s < kShards; s++) seg = std::max(seg, std::max(n_c[s], (n_s[s] + 1u) / 2u));
    WfBuffers wf;
    std::memset(&wf, 0, sizeof(wf));
    wf.seg_cap = seg + 1u;                                                              // the guard entry (two for the shadow queue)
    wf.blocks_per_shard = q.blocks_per_shard;
    wf.capacity = q.n_shadow + 1u;                                                      // slots: one per shadow ray and a guard
    const size_t qn = (size_t)kShards * wf.seg_cap, slots = state_slots_for(wf.capacity, kBlock), cnt_words = (size_t)kCounterArrays * kShards * kCounterStride;
    // host images of the buffers
    std::vector<uint32_t> h_cnt(cnt_words, kDebugSentinel);
    std::vector<float4> h_ro(qn), h_rd(qn), h_so(qn * 2), h_sd(qn * 2);
    const float sentinel = *(const float*)&kDebugSentinel;
    const float4 sent4 = make_float4(sentinel, sentinel, sentinel, sentinel);
    std::vector<float4> h_hit(qn, sent4), h_pend(slots * 2, sent4);
    std::memset(h_ro.data(), 0, qn * 16); std::memset(h_rd.data(), 0, qn * 16); std::memset(h_so.data(), 0, qn * 32); std::memset(h_sd.data(), 0, qn * 32);
    std::vector<uint32_t> at_c(q.n_closest), at_s(q.n_shadow), fill(kShards, 0);
    for (uint32_t i = 0; i < q.n_closest; i++) {
        const uint32_t s = q.closest_shard[i];
        const size_t e = (size_t)s * wf.seg_cap + fill[s]++;
        const float* r = q.closest + (size_t)i * 8;
        h_ro[e] = make_float4(r[0], r[1], r[2], r[7]);
        h_rd[e] = make_float4(r[4], r[5], r[6], *(const float*)&i);                     // (d.w = the path's slot: unused by the traversal)
        at_c[i] = (uint32_t)e;
    }
    std::fill(fill.begin(), fill.end(), 0u);
    for (uint32_t i = 0; i < q.n_shadow; i++) {
        const uint32_t s = q.shadow_shard[i];
        const size_t e = (size_t)s * wf.seg_cap * 2 + fill[s]++;
        const float* r = q.shadow + (size_t)i * 6;
        const uint32_t bits = i | (q.shadow_is_light[i] ? 0x80000000u : 0u);
        h_so[e] = make_float4(r[0], r[1], r[2], *(const float*)&bits);
        h_sd[e] = make_float4(r[3], r[4], r[5], *(const float*)&kNoHint);
        at_s[i] = (uint32_t)e;
    }
    for (uint32_t s = 0; s < kShards; s++) {
        if (q.which != 1) h_cnt[(size_t)cur * kShards * kCounterStride + s * kCounterStride] = n_c[s];      // (a counter no launched kernel reads keeps the sentinel)
        if (q.which != 0) h_cnt[(size_t)scnt * kShards * kCounterStride + s * kCounterStride] = n_s[s];
        h_cnt[(size_t)3 * kShards * kCounterStride + s * kCounterStride] = 0;           // the fetch heads: in a frame the shade stage rewinds them
        h_cnt[(size_t)4 * kShards * kCounterStride + s * kCounterStride] = 0;
    }
    char* d_all = nullptr;
    const size_t b_cnt = cnt_words * 4, b_q = qn * 16;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t total = up(b_cnt) + 3 * up(b_q) + 2 * up(b_q * 2) + up(slots * 32);
    if (hipMalloc((void**)&d_all, total) != hipSuccess) { (void)hipGetLastError(); why = "queue buffers"; return hipErrorOutOfMemory; }
    char* p = d_all;
    auto take = [&](size_t b) { char* r = p; p += up(b); return r; };
    uint32_t* d_cnt = (uint32_t*)take(b_cnt);
    for (int k = 0; k < kCounterArrays; k++) wf.cnt[k] = d_cnt + (size_t)k * kShards * kCounterStride;
    wf.ray_o[cur] = (float4*)take(b_q); wf.ray_d[cur] = (float4*)take(b_q); wf.hit = (float4*)take(b_q);
    wf.sh_o = (float4*)take(b_q * 2); wf.sh_d = (float4*)take(b_q * 2);
    wf.pend = (float4*)take(slots * 32);
    hipError_t e = hipMemcpyAsync(d_cnt, h_cnt.data(), b_cnt, hipMemcpyHostToDevice, stream);
    if (!e) e = hipMemcpyAsync(wf.ray_o[cur], h_ro.data(), b_q, hipMemcpyHostToDevice, stream);
    if (!e) e = hipMemcpyAsync(wf.ray_d[cur], h_rd.data(), b_q, hipMemcpyHostToDevice, stream);
    if (!e) e = hipMemcpyAsync(wf.hit, h_hit.data(), b_q, hipMemcpyHostToDevice, stream);
    if (!e) e = hipMemcpyAsync(wf.sh_o, h_so.data(), b_q * 2, hipMemcpyHostToDevice, stream);
    if (!e) e = hipMemcpyAsync(wf.sh_d, h_sd.data(), b_q * 2, hipMemcpyHostToDevice, stream);
    if (!e) e = hipMemcpyAsync(wf.pend, h_pend.data(), slots * 32, hipMemcpyHostToDevice, stream);
    if (!e) {
        FrameConstants fc;
        std::memset(&fc, 0, sizeof(fc));
        fc.flags = q.flags; fc.max_ray_length = q.shadow_tmax;
        uint32_t rf, rmask;
        traversal_ray_flags(q.flags, q.bounce, rf, rmask);
        const dim3 grid(kShards * wf.blocks_per_shard);
        if (q.which == 0) launch_wf_trace(grid, stream, count, sc, fc, wf, cur, q.bounce, rf, rmask, counters);
        else if (q.which == 1) launch_wf_shadow(grid, stream, count, sc, wf, q.bounce, q.flags, q.shadow_tmax, counters);
        else launch_wf_traverse(grid, stream, count, sc, fc, wf, cur, q.bounce - 1, rf, rmask, counters);
        e = hipGetLastError();
    }
    std::vector<TriPacket> h_tris(sc.num_tris);
    if (!e) e = hipMemcpyAsync(h_cnt.data(), d_cnt, b_cnt, hipMemcpyDeviceToHost, stream);
    if (!e) e = hipMemcpyAsync(h_hit.data(), wf.hit, b_q, hipMemcpyDeviceToHost, stream);
    if (!e) e = hipMemcpyAsync(h_pend.data(), wf.pend, slots * 32, hipMemcpyDeviceToHost, stream);
    if (!e && sc.num_tris) e = hipMemcpyAsync(h_tris.data(), sc.tris, (size_t)sc.num_tris * sizeof(TriPacket), hipMemcpyDeviceToHost, stream);
    if (!e) e = hipStreamSynchronize(stream);
    hipFree(d_all);
    if (e) { why = hipGetErrorString(e); return e; }
    // ---- translate
    auto is_sentinel = [](float v) { uint32_t b; std::memcpy(&b, &v, 4); return b == kDebugSentinel; };
    auto untouched = [&](const float4& v) { return is_sentinel(v.x) && is_sentinel(v.y) && is_sentinel(v.z) && is_sentinel(v.w); };
    std::vector<uint8_t> expected(qn, 0);
    for (uint32_t i = 0; i < q.n_closest; i++) {
        float* o = q.out_closest + (size_t)i * 8;
        const float4 h = h_hit[at_c[i]];
        expected[at_c[i]] = 1;
        if (untouched(h)) { for (int k = 0; k < 8; k++) o[k] = sentinel; continue; }
        uint32_t bits; std::memcpy(&bits, &h.w, 4);
        const bool hit = bits != kMissTri && (bits & 0x7fffffffu) < sc.num_tris;
        o[0] = hit ? 1.0f : 0.0f; o[1] = hit ? h.x : 0.0f; o[2] = hit ? h.y : 0.0f; o[3] = hit ? h.z : 0.0f;
        if (hit) { const TriPacket& t = h_tris[bits & 0x7fffffffu]; o[4] = (float)t.inst; o[5] = (float)t.prim; o[6] = (bits >> 31) ? 1.0f : 0.0f; }
        else { o[4] = -1.0f; o[5] = -1.0f; o[6] = 0.0f; if (bits != kMissTri) o[0] = sentinel; }                 // (a triangle index out of range: never a valid answer)
        o[7] = 0.0f;
    }
    uint32_t stray_hit = 0, stray_pend = 0;
    for (size_t k = 0; k < qn; k++) if (!expected[k] && !untouched(h_hit[k])) stray_hit++;
    std::vector<uint8_t> target(slots * 2, 0);
    for (uint32_t i = 0; i < q.n_shadow; i++) {
        const size_t k = 2 * (size_t)i + (q.shadow_is_light[i] ? 1u : 0u);
        target[k] = 1;
        q.out_shadow[i] = h_pend[k].w;
    }
    for (size_t k = 0; k < slots * 2; k++) {
        const float4& v = h_pend[k];
        if (!is_sentinel(v.x) || !is_sentinel(v.y) || !is_sentinel(v.z) || (!target[k] && !is_sentinel(v.w))) stray_pend++;
    }
    q.out_stray[0] = stray_hit; q.out_stray[1] = stray_pend;
    for (uint32_t s = 0; s < kShards; s++) for (int k = 0; k < kCounterArrays; k++) q.out_cnt[s * kCounterArrays + k] = h_cnt[(size_t)k * kShards * kCounterStride + s * kCounterStride];
    return hipSuccess;
}

}  // namespace pt
