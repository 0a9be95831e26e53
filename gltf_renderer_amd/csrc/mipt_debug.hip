// mipt_debug.hip -- the test hooks of libmipt.so (pt_debug_*, declared in mipt_debug.h, not part of include/mipt.h): the product's own
// device code run on the caller's queries, for tests/ and tools/ to compare with the oracle.  Host code only: this file has no kernel; what
// the hooks launch is in debug_wf.hip and debug_mk.hip (compiled as pt_wavefront.hip and pt_kernel.hip are) and motion.hip.  The product
// itself is mipt_api.hip and the feature files beside it.
#include <cstdio>
#include <cstdlib>

#include "mipt_debug.h"
#include "pt_ctx.h"

using namespace pt;

namespace {

// The shape the per-lane query hooks share.  Every input and output gets a temporary device array; the inputs are copied up on the context's
// stream, `launch(d_in, d_out)` runs on the device arrays (in the order given) and answers PT_OK or its own refusal, the outputs are copied
// back and the stream drained.  An output with a null host pointer is scratch the kernel writes and nobody reads; one with `preload` starts
// from the caller's values.  hook, noun: "<hook>: <noun>" is the text beside PT_ERR_OUT_OF_MEMORY, "<hook>: <HIP's>" beside PT_ERR_DEVICE.
struct QueryIn { const void* host; size_t bytes; };
struct QueryOut { void* host; size_t bytes; bool preload = false; };
using QueryBufs = std::vector<TempBuf>;
template <typename Launch>
int run_query(pt_ctx* ctx, const std::string& hook, const char* noun, std::initializer_list<QueryIn> ins, std::initializer_list<QueryOut> outs, Launch launch) {
    QueryBufs d_in(ins.size()), d_out(outs.size());
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < ins.size() && e == hipSuccess; k++) e = d_in[k].alloc(ins.begin()[k].bytes);
    for (size_t k = 0; k < outs.size() && e == hipSuccess; k++) e = d_out[k].alloc(outs.begin()[k].bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return ctx->fail(PT_ERR_OUT_OF_MEMORY, hook + ": " + noun); }
    for (size_t k = 0; k < ins.size() && e == hipSuccess; k++) e = hipMemcpyAsync(d_in[k].ptr, ins.begin()[k].host, ins.begin()[k].bytes, hipMemcpyHostToDevice, ctx->stream);
    for (size_t k = 0; k < outs.size() && e == hipSuccess; k++)
        if (const QueryOut& o = outs.begin()[k]; o.preload) e = hipMemcpyAsync(d_out[k].ptr, o.host, o.bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) { if (int r = launch(d_in, d_out)) return r; e = hipGetLastError(); }
    for (size_t k = 0; k < outs.size() && e == hipSuccess; k++)
        if (const QueryOut& o = outs.begin()[k]; o.host) e = hipMemcpyAsync(o.host, d_out[k].ptr, o.bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? PT_OK : ctx->fail(PT_ERR_DEVICE, hook + ": " + hipGetErrorString(e));
}

// the per-lane query kernels of unit 0: the wavefront stages' build (tables in LDS), 1: the megakernel's (global memory)
DebugQueryLaunch queries_of(int unit) { return unit == 0 ? debug_queries_wf() : debug_queries_mk(); }

}  // namespace

// diagnostic (not part of include/mipt.h): how many materials of the current table read the interleaved footprint
extern "C" int pt_debug_interleaved_materials(const pt_ctx* ctx) {
    int n = 0;
    if (ctx) for (const RMat& r : ctx->rmats_host) n += (r.bound_mask & RM_TRIO) ? 1 : 0;
    return n;
}

extern "C" int pt_debug_interleaved_emissive(const pt_ctx* ctx) {          // ... and how many of them carry their emissive texture in it
    int n = 0;
    if (ctx) for (const RMat& r : ctx->rmats_host) n += (r.bound_mask & RM_TRIO_EMISSIVE) ? 1 : 0;
    return n;
}

// test hook (not part of include/mipt.h): the camera rays pt_trace would generate for the queries {px, py, seed} under `params` and the context's
// lens (pt_set_lens) -- camera_ray itself, one query per lane (debug_wf.hip k_debug_rays).  queries: 3 uint32 each, out: 8 floats each
// (origin, tmin, direction, tmax), host arrays.  Needs no scene; leaves the accumulation and a pending restart as they are.
extern "C" int pt_debug_camera_rays(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const uint32_t* queries, uint32_t n, float* out) {
    if (!ctx || !settings || !params || (n && (!queries || !out)) || params->width == 0 || params->height == 0) return PT_ERR_INVALID_ARGUMENT;
    CameraSetup cam;
    if (!camera_setup(params, ctx->lens, cam)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "singular camera matrix");
    if (n == 0) return PT_OK;
    ENTER(ctx);
    FrameConstants fc;
    camera_constants(cam, params, fc);
    return run_query(ctx, "pt_debug_camera_rays", "buffers", {{queries, (size_t)n * 12}}, {{out, (size_t)n * 32}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        launch_debug_camera_rays(fc, cam.lens, d_in[0].as<uint32_t>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the rays pt_trace would start for the queries {px, py, seed} under the context's bake (pt_set_bake, which must
// be on) on a params->width x height atlas -- bake_ray itself, the generate kernel's ray function, one query per lane (debug_wf.hip
// k_debug_rays).  Builds the tree and the coverage map as that pt_trace would.  queries: 3 uint32 each, out: 8 floats each (origin, tmin,
// direction, tmax; zeros with tmax = -1 for an uncovered texel), host arrays.  Leaves the accumulation and a pending restart as they are.
extern "C" int pt_debug_bake_rays(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const uint32_t* queries, uint32_t n, float* out) {
    if (!ctx || !settings || !params || (n && (!queries || !out)) || params->width == 0 || params->height == 0) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->bake.enable) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_bake_rays: no bake is set");
    if (ctx->bake.instance >= (int)ctx->instances.size()) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: instance " + std::to_string(ctx->bake.instance) + " of " + std::to_string(ctx->instances.size()));
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    BakeArgs bk = {};
    if (int r = bake_setup(ctx, params->width, params->height, bk)) return r;
    if (n == 0) return PT_OK;
    FrameConstants fc;
    memset(&fc, 0, sizeof(fc));
    fc.res_x = params->width; fc.res_y = params->height;
    return run_query(ctx, "pt_debug_bake_rays", "buffers", {{queries, (size_t)n * 12}}, {{out, (size_t)n * 32}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        launch_debug_bake_rays(fc, bk, d_in[0].as<uint32_t>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the rays pt_trace would start for the queries {px, py, seed} under the context's probes (pt_set_probes,
// which must be on) on their atlas, which params->width x height must be -- probe_ray itself, the generate kernel's ray function, one query
// per lane (debug_wf.hip k_debug_rays).  queries: 3 uint32 each, out: 8 floats each (origin, tmin, direction, tmax; zeros with
// tmax = -1 for a cell without a probe), host arrays.  Leaves the accumulation and a pending restart as they are.
extern "C" int pt_debug_probe_rays(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const uint32_t* queries, uint32_t n, float* out) {
    if (!ctx || !settings || !params || (n && (!queries || !out))) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->probes.enable) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_probe_rays: no probes are set");
    uint64_t w, h;
    probe_atlas_size(ctx->probes, w, h);
    if (params->width != w || params->height != h) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_probe_rays: the atlas is " + std::to_string(w) + " x " + std::to_string(h));
    ENTER(ctx);
    if (n == 0) return PT_OK;
    FrameConstants fc;
    memset(&fc, 0, sizeof(fc));
    fc.res_x = params->width; fc.res_y = params->height;
    const ProbeArgs pa = probe_args(ctx);
    return run_query(ctx, "pt_debug_probe_rays", "buffers", {{queries, (size_t)n * 12}}, {{out, (size_t)n * 32}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        launch_debug_probe_rays(fc, pa, d_in[0].as<uint32_t>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): what the product's traversal finds for caller-supplied rays (host arrays: 8 floats per ray in,
// 8 floats per ray out, debug_mk.hip k_debug_intersect).  mode 0 = TraceRay's closest hit, 1 = TraceShadowRay's occlusion search.
extern "C" int pt_debug_intersect(pt_ctx* ctx, const float* rays, uint32_t n, uint32_t ray_flags, int mode, float* out) {
    if (!ctx || (n && (!rays || !out)) || mode < 0 || mode > 1) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    if (n == 0) return PT_OK;
    SceneRec sc = scene_fill(ctx);
    const uint32_t lanes = (n + 255u) & ~255u;
    TempBuf deep_buf;
    return run_query(ctx, "pt_debug_intersect", "ray buffers", {{rays, (size_t)n * 32}}, {{out, (size_t)n * 32}}, [&](const QueryBufs& in_buf, const QueryBufs& out_buf) -> int {
        if (int r = temp_deep_stack(ctx, sc, deep_buf, lanes, "pt_debug_intersect: deep stack")) return r;
        float *d_rays = in_buf[0].as<float>(), *d_out = out_buf[0].as<float>();
        launch_debug_intersect(sc, d_rays, n, ray_flags, mode, d_out, ctx->stream);
        if (hipPeekAtLastError() == hipSuccess && getenv("MIPT_DEBUG_INTERSECT_TIMING")) {           // probe (tools/ray_order_probe.py): the same launch timed, 5 repeats
            hipEvent_t ev[2]; hipEventCreate(&ev[0]); hipEventCreate(&ev[1]);
            hipEventRecord(ev[0], ctx->stream);
            for (int k = 0; k < 5; k++) launch_debug_intersect(sc, d_rays, n, ray_flags, mode, d_out, ctx->stream);
            hipEventRecord(ev[1], ctx->stream); hipEventSynchronize(ev[1]);
            float ms = 0; hipEventElapsedTime(&ms, ev[0], ev[1]);
            fprintf(stderr, "pt_debug_intersect: %u rays, %.3f ms per launch, %.1f Mrays/s\n", n, ms / 5, n / (ms / 5) * 1e-3);
            hipEventDestroy(ev[0]); hipEventDestroy(ev[1]);
        }
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the acceleration structure itself, as the device built or refitted it, for tests/accel_ref.py to check
// node by node.  Builds or refits what is pending (ensure_accel) and drains the stream.  info: n_tris, wide_nodes, root, stack_need, the
// scratch's seg_leaves, the builder in force (PT_BUILDER_*), scratch.fallbacks, and 1 if the collapse's ranges (scratch.wide_ranges) are there
// -- 0 once the scratch is released or too small for this tree: they are then not read.  Each non-null host array receives its copy: nodes
// wide_nodes x 64 B (Bvh4Node), ranges wide_nodes x 32 B (WideRanges; untouched when absent), tris n_tris x 64 B (TriPacket), shade
// n_tris x 128 B (ShadePacket); a first call with null arrays tells the sizes.  Leaves the accumulation and a pending restart as they are.
extern "C" int pt_debug_accel_read(pt_ctx* ctx, uint32_t info[8], void* nodes, void* ranges, void* tris, void* shade) {
    if (!ctx || !info) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    HIPOK(hipStreamSynchronize(ctx->stream));
    const AccelScratch& s = ctx->scratch;
    const size_t n = ctx->n_tris, w = ctx->wide_nodes;
    const bool have_ranges = s.wide_ranges != nullptr && s.capacity >= n && w <= s.capacity;
    info[0] = ctx->n_tris; info[1] = ctx->wide_nodes; info[2] = (uint32_t)ctx->root; info[3] = ctx->stack_need;
    info[4] = (uint32_t)s.seg_leaves; info[5] = (uint32_t)s.builder; info[6] = s.fallbacks; info[7] = have_ranges ? 1u : 0u;
    if (w > n) return ctx->fail(PT_ERR_DEVICE, "pt_debug_accel_read: " + std::to_string(w) + " wide nodes over " + std::to_string(n) + " triangles");   // the arrays hold n
    if (nodes && w) HIPOK(hipMemcpy(nodes, ctx->d_nodes.ptr, w * sizeof(Bvh4Node), hipMemcpyDeviceToHost));
    if (ranges && w && have_ranges) HIPOK(hipMemcpy(ranges, s.wide_ranges, w * sizeof(WideRanges), hipMemcpyDeviceToHost));
    if (tris && n) HIPOK(hipMemcpy(tris, ctx->d_tris.ptr, n * sizeof(TriPacket), hipMemcpyDeviceToHost));
    if (shade && n) HIPOK(hipMemcpy(shade, ctx->d_shade.ptr, n * sizeof(ShadePacket), hipMemcpyDeviceToHost));
    return PT_OK;
}

// test hook (not part of include/mipt.h): the sorted Morton keys of the last full build -- scratch.keys_b, which the sort writes and nothing
// overwrites afterwards -- for tests/builder_ref.py morton_keys to be compared on its own.  Builds what is pending and drains the stream.
// out: n uint64, n == n_tris.  An error once the scratch is released or too small for this tree, after a refit (the keys are those of the
// pose of the build), and for fewer than two triangles (no key is computed).
extern "C" int pt_debug_accel_keys(pt_ctx* ctx, uint64_t* out, size_t n) {
    if (!ctx || (n && !out)) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    HIPOK(hipStreamSynchronize(ctx->stream));
    const AccelScratch& s = ctx->scratch;
    if (n != ctx->n_tris) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_accel_keys: " + std::to_string(n) + " keys asked for, the tree has " + std::to_string(ctx->n_tris) + " triangles");
    if (n < 2) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_accel_keys: a build of fewer than two triangles computes no key");
    if (!s.keys_b || s.capacity < n) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_accel_keys: the build's scratch has been released");
    if (ctx->accel_last_was_refit) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_accel_keys: the last operation was a refit; the keys are those of the last full build");
    HIPOK(hipMemcpy(out, s.keys_b, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

// test hook (not part of include/mipt.h): the motion records (pt_set_motion) pt_trace would write for caller-supplied first rays under `settings`
// (its cull flag), `params` (the current camera, the image size) and the context's motion config (the previous camera) and snapshot --
// k_debug_intersect's closest hit, then k_wf_motion's own record function (motion.hip k_debug_motion).  rays: 8 floats each as
// pt_debug_intersect takes them; out: 8 floats each (record.xyzw, instance, primitive, u, v; zeros with instance = primitive = -1 for a miss),
// host arrays.  The config's enable and target are not looked at.  Leaves the accumulation and a pending restart as they are.
extern "C" int pt_debug_motion(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const float* rays, uint32_t n, float* out) {
    if (!ctx || !settings || !params || (n && (!rays || !out)) || params->width == 0 || params->height == 0) return PT_ERR_INVALID_ARGUMENT;
    CameraSetup cam;
    if (!camera_setup(params, ctx->lens, cam)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "singular camera matrix");
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    if (n == 0) return PT_OK;
    SceneRec sc = scene_fill(ctx);
    MotionArgs mo;
    motion_setup(ctx, cam.world_to_clip, params, mo);
    const uint32_t lanes = (n + 255u) & ~255u;
    TempBuf deep_buf;
    return run_query(ctx, "pt_debug_motion", "ray buffers", {{rays, (size_t)n * 32}}, {{out, (size_t)n * 32}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) -> int {
        if (int r = temp_deep_stack(ctx, sc, deep_buf, lanes, "pt_debug_motion: deep stack")) return r;
        launch_debug_motion(sc, mo, d_in[0].as<float>(), n, (settings->flags & PT_FLAG_CULL_BACKFACE) ? 1u : 0u, d_out[0].as<float>(), ctx->stream);   // RF_CULL_BACK (RayGeneration :747)
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the traversal kernels pt_trace launches in the wavefront mode -- which 0: k_wf_trace, 1: k_wf_shadow,
// 2: the fused k_wf_traverse -- on queues the caller fills (debug_wf.hip debug_trace_queues; host arrays).  closest: n_c rays of 8 floats
// (origin, tmin = 0: the queue format has none, direction, tmax) with the shard 0..255 each is queued in (the caller's order within a shard is
// the queue's); shadow: n_s rays of 6 floats (origin, direction) with shard and is_light bit, one shadow_tmax for all.  flags: PT_FLAG_*;
// bounce: of the closest rays (which 0, 2; the fused launch needs bounce >= 1 and takes the shadow rays of bounce - 1) or of the shadow rays
// (which 1).  Ray flags, instance mask, kernel copy and counting are chosen by the code launch_wavefront runs.  out_closest: 8 floats per ray
// as pt_debug_intersect's; out_shadow: the transmission written beside the ray's pending term; out_cnt: 256 x 7 counter words after the
// launch; out_stray: 2 words, see pt_host.h.  Leaves the accumulation, the workspace and a pending restart of the context as they are.
extern "C" int pt_debug_trace_queues(pt_ctx* ctx, const float* closest, const uint32_t* closest_shard, uint32_t n_c, const float* shadow, const uint32_t* shadow_shard,
                                     const uint8_t* shadow_is_light, uint32_t n_s, float shadow_tmax, uint32_t flags, int bounce, uint32_t blocks_per_shard, int which,
                                     float* out_closest, float* out_shadow, uint32_t* out_cnt, uint32_t* out_stray) {
    if (which < 0 || which > 2 || blocks_per_shard < 1 || blocks_per_shard > 64 || bounce < 0 || (which == 2 && bounce < 1)) return PT_ERR_INVALID_ARGUMENT;
    if ((n_c && (!closest || !closest_shard || !out_closest)) || (n_s && (!shadow || !shadow_shard || !shadow_is_light || !out_shadow)) || !out_cnt || !out_stray) return PT_ERR_INVALID_ARGUMENT;
    if (n_c > 0x0fffffffu || n_s > 0x0fffffffu) return PT_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n_c; i++) if (closest_shard[i] > 255u || closest[(size_t)i * 8 + 3] != 0.0f) return PT_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n_s; i++) if (shadow_shard[i] > 255u) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    SceneRec sc = scene_fill(ctx);                         // has_env = 0: the traversal stages draw no environment samples
    TempBuf d_deep;                                        // the deep stack as pt_trace sets it up, for this launch's grid
    if (int r = temp_deep_stack(ctx, sc, d_deep, (size_t)256 * blocks_per_shard * 256, "pt_debug_trace_queues: deep stack")) return r;
    const DebugQueues q = {closest, closest_shard, n_c, shadow, shadow_shard, shadow_is_light, n_s, shadow_tmax, flags, bounce, blocks_per_shard, which,
                           out_closest, out_shadow, out_cnt, out_stray};
    std::string why;
    const hipError_t e = debug_trace_queues(sc, q, ctx->d_counters.as<Counters>(), ctx->counters_enabled, ctx->stream, why);
    if (e == hipErrorOutOfMemory) return ctx->fail(PT_ERR_OUT_OF_MEMORY, "pt_debug_trace_queues: " + why);
    return e == hipSuccess ? PT_OK : ctx->fail(PT_ERR_DEVICE, "pt_debug_trace_queues: " + why);
}

// test hook (not part of include/mipt.h): the shade stage's texture sampler on caller-supplied queries, one per lane (pt_shading.h
// debug_sample_query).  mat_slot: 2 per query (material, slot 0..14 or 16..19); tc: 4 per query (tc0.xy, tc1.xy); out_rgba: 4 per query;
// out_taps (may be null): 5 per query (i0, i1, j0, j1, and ia: the first column of the texel pair loaded for each row).  unit 0: the wavefront stages' build (tables in LDS), 1: the megakernel's.
extern "C" int pt_debug_sample_texture(pt_ctx* ctx, int unit, const uint32_t* mat_slot, const float* tc, uint32_t n, float* out_rgba, int32_t* out_taps) {
    if (!ctx || unit < 0 || unit > 1 || (n && (!mat_slot || !tc || !out_rgba))) return PT_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t mat = mat_slot[2 * i], slot = mat_slot[2 * i + 1];
        if (mat >= (uint32_t)ctx->n_materials || !(slot < (uint32_t)SLOT_COUNT || (slot >= 16u && slot <= 19u)))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_sample_texture: query " + std::to_string(i) + " names material " + std::to_string(mat) +
                                                      " slot " + std::to_string(slot) + " (" + std::to_string(ctx->n_materials) + " materials)");
    }
    ENTER(ctx);
    if (n == 0) return PT_OK;
    const SceneRec sc = scene_fill(ctx);                   // (the sampler reads the materials and the lookup tables)
    return run_query(ctx, "pt_debug_sample_texture", "query buffers", {{mat_slot, (size_t)n * 8}, {tc, (size_t)n * 16}}, {{out_rgba, (size_t)n * 16}, {out_taps, (size_t)n * 20}},
                     [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        queries_of(unit).sample_texture(sc, d_in[0].as<uint32_t>(), d_in[1].as<float>(), n, d_out[0].as<float>(), d_out[1].as<int32_t>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the environment light on caller-supplied queries, one per lane (pt_vertex.h debug_env_query:
// op 0 SAMPLE, 1 PDF, 2 CUBE, 3 MISS; 8 input and 16 output floats per query).  unit 0: the wavefront stages' build (the coarse pyramid
// levels staged into LDS as env_prepass stages them), 1: the megakernel's (global memory).
extern "C" int pt_debug_env_query(pt_ctx* ctx, int env, int unit, int op, const float* in, uint32_t n, float* out) {
    if (!ctx || unit < 0 || unit > 1 || op < 0 || op > 3 || (n && (!in || !out))) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_debug_env_query: environment " + std::to_string(env));
    ENTER(ctx);
    if (n == 0) return PT_OK;
    SceneRec sc;
    memset(&sc, 0, sizeof(sc));
    scene_set_env(sc, *ctx->envs[env]);
    const size_t in_bytes = (size_t)n * 8 * 4, out_bytes = (size_t)n * 16 * 4;
    return run_query(ctx, "pt_debug_env_query", "query buffers", {{in, in_bytes}}, {{out, out_bytes, true}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {   // (true: unused outputs keep the caller's values)
        queries_of(unit).env_query(sc, op, d_in[0].as<float>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the material model on caller-supplied queries, one per lane (pt_vertex.h debug_bsdf_query:
// op 0 EVALUATE through evaluate_bsdf, 1 SAMPLE through sample_bsdf, after the vertex's prepare_bsdf; 48 input and 16 output floats per
// query, laid out there).  Part of the contract: query i runs in lane i % 64 of wave i / 64, and the lanes of the last wave past n are not
// active -- the sheen lobe is run or skipped by a vote of a wave's active lanes, so the caller composes the waves by ordering the queries.
// flags: PT_FLAG_*, of which PT_FLAG_MATERIAL_DIFFUSE_WHITE and PT_FLAG_MATERIAL_MIS are read.  unit 0: the wavefront stages' build (the
// sheen table staged into LDS), 1: the megakernel's (global memory).  Needs no scene.
extern "C" int pt_debug_bsdf_query(pt_ctx* ctx, int unit, int op, uint32_t flags, const float* in, uint32_t n, float* out) {
    if (!ctx || unit < 0 || unit > 1 || op < 0 || op > 1 || (n && (!in || !out))) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (n == 0) return PT_OK;
    const SceneRec sc = scene_fill(ctx);                   // (the BSDF reads the sheen table; stage_luts stages the sRGB table with it)
    const size_t in_bytes = (size_t)n * 48 * 4, out_bytes = (size_t)n * 16 * 4;
    return run_query(ctx, "pt_debug_bsdf_query", "query buffers", {{in, in_bytes}}, {{out, out_bytes}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        queries_of(unit).bsdf_query(sc, op, flags, d_in[0].as<float>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the punctual lights on caller-supplied queries, one per lane -- load_light, then light_ray, as the
// shade stage runs them for the light it picked (pt_vertex.h debug_light_query), on the first num_of_lights lights of the context's table
// (pt_scene_set_lights).  light_index: one per query, below num_of_lights; p: 3 floats per query, the shaded point; out: 8 floats per
// query (direction, colour, cone_terms_staged: 1 where the spot cone terms were read from the staged copy, 0).  unit 0: the wavefront
// stages' build, the first 32 lights staged into LDS with their cone terms; small_tables as the shade kernel's SMALL copy has it (every light
// is in LDS: at most 32 lights, else PT_ERR_INVALID_ARGUMENT).  unit 1: the megakernel's (global memory; small_tables is not looked at).
extern "C" int pt_debug_light_query(pt_ctx* ctx, int unit, int small_tables, int num_of_lights, const uint32_t* light_index, const float* p, uint32_t n, float* out) {
    if (!ctx || unit < 0 || unit > 1 || (n && (!light_index || !p || !out))) return PT_ERR_INVALID_ARGUMENT;
    if (num_of_lights < 0 || num_of_lights > ctx->n_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_light_query: " + std::to_string(num_of_lights) + " of " + std::to_string(ctx->n_lights) + " lights");
    if (unit == 0 && small_tables && num_of_lights > debug_light_cache_max()) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_light_query: small_tables with " + std::to_string(num_of_lights) + " lights");
    for (uint32_t i = 0; i < n; i++)
        if (light_index[i] >= (uint32_t)num_of_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_light_query: query " + std::to_string(i) + " names light " + std::to_string(light_index[i]) + " of " + std::to_string(num_of_lights));
    ENTER(ctx);
    if (n == 0) return PT_OK;
    const SceneRec sc = scene_fill(ctx);
    return run_query(ctx, "pt_debug_light_query", "query buffers", {{light_index, (size_t)n * 4}, {p, (size_t)n * 12}}, {{out, (size_t)n * 32}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        queries_of(unit).light_query(sc, small_tables != 0, num_of_lights, d_in[0].as<uint32_t>(), d_in[1].as<float>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): the vertex fetch and the material evaluation of a path vertex on caller-supplied hits, one per
// lane, through the shade stage's own functions in its order (pt_vertex.h debug_surface_query: load_shade_packet_raw, load_shade_inst, the
// voted load_shade_packet_extra, unpack_shade_packet, material_header, get_vertex_attributes, the back-face flip, offset_ray both ways,
// get_surface, emissive_of) and, separately, the any-hit path's candidate_alpha for the same hit.  Builds or refits what is pending.
//   in   8 words per query: the packet index (uint32: the hit's index in the TriPacket / ShadePacket arrays, pt_debug_accel_read; below
//        n_tris, else PT_ERR_INVALID_ARGUMENT), front (uint32: 0 or 1), u, v, the ray direction d.xyz (the view is -normalize(d)), 0
//   out 72 floats per query:
//        [0,24)   HitGeom after the flip: position, ng, n, t [9,12), tw [12], bt [13,16), colour [16,20), tc[0] [20,22), tc[1] [22,24)
//        [24,55)  Surface as the reference's SurfaceProperties floats [0,31), the order of pt_debug_bsdf_query's input: albedo, alpha,
//                 metalness, roughness_squared.xy, shading normal, anisotropy tangent, bitangent, ior, specular colour, specular factor,
//                 clearcoat, clearcoat roughness, clearcoat normal, sheen colour, sheen roughness squared, transmissive (thickness and
//                 attenuation, which the product does not keep, are not there)
//        [55,58)  the emissive value, [58,61) o_above, [61,64) o_below
//        [64]     the texture taps get_surface and emissive_of counted
//        [65,68)  candidate_alpha's base_alpha, alpha, cutoff; [68,72) 0
// Part of the contract: query i runs in lane i % 64 of wave i / 64, and the lanes of the last wave past n are not active -- the second
// packet fetch, the interleaved / general texel fetch and the edge reload are behind votes of a wave's active lanes, so the caller composes
// the waves by ordering the queries.  flags: PT_FLAG_*, of which PT_FLAG_SHADING_NORMAL_ADAPTATION and
// PT_FLAG_MATERIAL_USE_GEOMETRIC_NORMALS are read.  unit 0: the wavefront stages' build, the lookup tables, instance rows and materials
// staged into LDS as k_wf_shade stages them; small_tables as the shade kernel's SMALL copy has it (every row and material is in LDS: at most
// 128 instances and 96 materials, else PT_ERR_INVALID_ARGUMENT).  unit 1: the megakernel's (global memory; small_tables is not looked at).
extern "C" int pt_debug_surface_query(pt_ctx* ctx, int unit, int small_tables, uint32_t flags, const void* in, uint32_t n, float* out) {
    if (!ctx || unit < 0 || unit > 1 || (n && (!in || !out))) return PT_ERR_INVALID_ARGUMENT;
    if (unit == 0 && small_tables && ((int)ctx->instances.size() > debug_inst_cache_max() || ctx->n_materials > debug_mat_cache_max()))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_surface_query: small_tables with " + std::to_string(ctx->instances.size()) + " instances and " + std::to_string(ctx->n_materials) + " materials");
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    const uint32_t* words = (const uint32_t*)in;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t tri = words[(size_t)8 * i], front = words[(size_t)8 * i + 1];
        if (tri >= ctx->n_tris || front > 1u)
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_surface_query: query " + std::to_string(i) + " names packet " + std::to_string(tri) + " of " + std::to_string(ctx->n_tris) + ", front " + std::to_string(front));
    }
    if (n == 0) return PT_OK;
    const SceneRec sc = scene_fill(ctx);
    const size_t in_bytes = (size_t)n * 8 * 4, out_bytes = (size_t)n * 72 * 4;
    return run_query(ctx, "pt_debug_surface_query", "query buffers", {{in, in_bytes}}, {{out, out_bytes}}, [&](const QueryBufs& d_in, const QueryBufs& d_out) {
        queries_of(unit).surface_query(sc, small_tables != 0, flags, d_in[0].as<float>(), n, d_out[0].as<float>(), ctx->stream);
        return PT_OK;
    });
}

// test hook (not part of include/mipt.h): an environment map from a given cube mip 0 (6 x n x n RGBA16F) and a whole 1024^2 sum pyramid
// (level 0 first), as the oracle's orc_env_create_raw takes them -- so both sides can sample a crafted pyramid.
extern "C" int pt_debug_env_create_raw(pt_ctx* ctx, int cube_n, const uint16_t* cube_rgba16f, const float* pyramid, int* env_out) {
    if (!ctx || cube_n < 1 || cube_n > 16384 || !cube_rgba16f || !pyramid || !env_out) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    EnvDevice* env = new EnvDevice();
    hipError_t e = env_build_raw(*env, cube_n, cube_rgba16f, pyramid, ctx->stream);
    if (e) { env_free(*env); delete env; return ctx->fail(PT_ERR_DEVICE, std::string("pt_debug_env_create_raw: ") + hipGetErrorString(e)); }
    *env_out = take_slot(ctx->envs, ctx->free_envs, env);
    return PT_OK;
}

// test hook (not part of include/mipt.h): the five 4x4-blocked copies of pyramid levels 8, 6, 4, 2, 0 (EnvRec::blocked: 4^2 + 16^2 + 64^2 +
// 256^2 + 1024^2 = 1118480 floats, coarsest first), as the sampler reads them.
extern "C" int pt_debug_env_read_blocked(pt_ctx* ctx, int env, float* out) {
    if (!ctx || !out) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_debug_env_read_blocked: environment " + std::to_string(env));
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    const EnvDevice& ed = *ctx->envs[env];
    HIPOK(hipMemcpy(out, ed.blocked, (size_t)(ed.blocked_offset[4] + 1024u * 1024u) * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}
