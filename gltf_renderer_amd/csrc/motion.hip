// motion.hip -- motion vectors and temporal reprojection (include/mipt.h): what is not a stage of the wavefront pipeline.
//
//   pt_motion_snapshot  k_motion_snapshot: one lane per packet of the built tree copies (v0, e1, e2) to the packet's instance-major address
//                       instances[inst].tri_offset + prim, which no rebuild or reordering of the tree changes: the previous pose of every
//                       triangle, 48 bytes each.  The context keeps the row count and every row's triangle count the snapshot stands for.
//   pt_set_motion       checks and keeps the config; pt_trace (mipt_api.hip PathtraceScene) reads it through motion_setup, below.
//   pt_reproject        k_reproject: one lane per pixel, four taps of the previous frame at the pixel's motion vector, no LDS.  A pure function
//                       of its images; tests/motion_ref.py restates it in numpy float32, rounding for rounding.
//   pt_debug_motion     (mipt_debug.hip) launches k_debug_motion: k_debug_intersect's closest hit, then pt_motion.h motion_record.
// The record and resolve kernels (k_wf_motion, k_wf_motion_resolve) live in wf_passes.hip.  Compiled without floating-point contraction
// (Makefile), with IEEE division.
#include <cmath>

#include "pt_vertex.h"
#include "pt_ctx.h"
#include "pt_motion.h"

namespace pt {
namespace {

__global__ __launch_bounds__(kBlock) void k_motion_snapshot(const TriPacket* __restrict__ tris, uint32_t n_tris, const InstanceRec* __restrict__ instances,
                                                            uint32_t n_instances, float4* __restrict__ snap, uint32_t n_snap) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_tris) return;
    const float4* t = (const float4*)(tris + i);
    const float4 t0 = t[0], t1 = t[1], t2 = t[2];
    const uint32_t inst = __float_as_uint(t0.w), prim = __float_as_uint(t1.w);
    if (inst >= n_instances) return;
    const uint32_t at = instances[inst].tri_offset + prim;
    if (at >= n_snap) return;
    snap[3 * (size_t)at] = make_float4(t0.x, t0.y, t0.z, 0.0f);
    snap[3 * (size_t)at + 1] = make_float4(t1.x, t1.y, t1.z, 0.0f);
    snap[3 * (size_t)at + 2] = make_float4(t2.x, t2.y, t2.z, 0.0f);
}

__global__ __launch_bounds__(kBlock) void k_debug_motion(SceneRec sc, MotionArgs ma, const float* __restrict__ rays, uint32_t n, uint32_t rf, float* __restrict__ out) {
    __shared__ int s_stack[kStackLds * kBlock];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* q = rays + (size_t)i * 8;
    Ray r; r.o = v3(q[0], q[1], q[2]); r.tmin = q[3]; r.d = v3(q[4], q[5], q[6]); r.tmax = q[7];
    HitRec hit; LaneStats st = {0, 0, 0, 0, 0};
    float transmission = 0.0f;
    const bool got = traverse<false>(sc, s_stack + threadIdx.x, r, rf, 0xff, 0, hit, transmission, st);
    const bool have = got && hit.tri >= 0 && (uint32_t)hit.tri < sc.num_tris;
    float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (have) rec = motion_record(sc, ma, (uint32_t)hit.tri, hit.u, hit.v);
    float* o = out + (size_t)i * 8;
    o[0] = rec.x; o[1] = rec.y; o[2] = rec.z; o[3] = rec.w;
    o[4] = have ? (float)sc.tris[hit.tri].inst : -1.0f; o[5] = have ? (float)sc.tris[hit.tri].prim : -1.0f;
    o[6] = have ? hit.u : 0.0f; o[7] = have ? hit.v : 0.0f;
}

__device__ __forceinline__ bool rp_finite3(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// One lane per pixel.  A pixel reads its own colour and motion, then up to four taps of three (four with prev_length) previous images; the
// taps of a wave's neighbouring pixels are neighbouring texels wherever the motion field is smooth.  Exclusion is by selects.
__global__ __launch_bounds__(kBlock) void k_reproject(ReprojectArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.w * a.h) return;
    const uint32_t y = p / a.w, x = p - y * a.w;
    const float4 c = a.color[p], m = a.motion[p];
    const float sx = (float)x + m.x, sy = (float)y + m.y;
    bool usable = motion_finite(m) && m.w > 0.0f && m.z > 0.0f && sx > -1.0f && sx < (float)a.w && sy > -1.0f && sy < (float)a.h;
    float ws = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hl = 0.0f;
    if (usable) {
        const float x0 = floorf(sx), y0 = floorf(sy);
        const float fx = sx - x0, fy = sy - y0;
        const int ix = (int)x0, iy = (int)y0;
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int qx = ix + i, qy = iy + j;
                if (qx < 0 || qy < 0 || qx >= (int)a.w || qy >= (int)a.h) continue;
                const size_t q = (size_t)qy * a.w + (size_t)qx;
                const float4 pm = a.prev_motion[q], pc = a.prev_color[q];
                const float pl = a.prev_length ? a.prev_length[q] : 1.0f;
                const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                const bool counts = motion_finite(pm) && pm.w > 0.0f && fabsf(pm.w - m.z) <= a.depth_tolerance * m.z && rp_finite3(pc) &&
                                    isfinite(pl) && pl >= 1.0f;
                if (counts) {
                    ws = ws + b;
                    hr = hr + b * pc.x; hg = hg + b * pc.y; hb = hb + b * pc.z;
                    hl = hl + b * pl;
                }
            }
        }
    }
    if (!(usable && ws > 0.0f)) {
        a.out_color[p] = c;
        a.out_length[p] = 1.0f;
        return;
    }
    hr = hr / ws; hg = hg / ws; hb = hb / ws; hl = hl / ws;
    const float n = fminf(hl + 1.0f, a.max_history);
    const float al = fmaxf(1.0f / n, a.alpha_min);
    a.out_color[p] = make_float4(hr + al * (c.x - hr), hg + al * (c.y - hg), hb + al * (c.z - hb), c.w);
    a.out_length[p] = n;
}

}  // namespace

void launch_motion_snapshot(const TriPacket* tris, uint32_t n_tris, const InstanceRec* instances, uint32_t n_instances, float4* snap, uint32_t n_snap, hipStream_t stream) {
    if (n_tris == 0) return;
    hipLaunchKernelGGL(k_motion_snapshot, dim3((n_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, tris, n_tris, instances, n_instances, snap, n_snap);
}
void launch_debug_motion(const SceneRec& sc, const MotionArgs& ma, const float* d_rays, uint32_t n, uint32_t rf, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_motion, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, ma, d_rays, n, rf, d_out);
}
void launch_reproject(const ReprojectArgs& a, hipStream_t stream) {
    const uint32_t pixels = a.w * a.h;
    hipLaunchKernelGGL(k_reproject, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

int motion_snapshot_state(const pt_ctx* ctx) {
    if (!ctx->motion_snap_taken) return PT_MOTION_SNAPSHOT_NONE;
    if (ctx->motion_snap_counts.size() != ctx->instances.size()) return PT_MOTION_SNAPSHOT_STALE;
    for (size_t i = 0; i < ctx->instances.size(); i++)
        if (ctx->motion_snap_counts[i] != ctx->instances[i].tri_count) return PT_MOTION_SNAPSHOT_STALE;
    return PT_MOTION_SNAPSHOT_VALID;
}

void motion_setup(const pt_ctx* ctx, const float* world_to_clip, const pt_execute_params* ep, MotionArgs& mo) {
    memset(&mo, 0, sizeof(mo));
    if (motion_snapshot_state(ctx) == PT_MOTION_SNAPSHOT_VALID) {       // same rows, same counts: the same addresses, n_tris of them
        mo.snap = ctx->d_motion_snap.as<float4>();
        mo.n_snap = ctx->n_tris;
    }
    mo.width = ep->width; mo.height = ep->height;
    mo.target = (float4*)ctx->motion.motion;
    memcpy(mo.mc, world_to_clip, 64);
    world_to_clip_of(ctx->motion.prev_view_to_clip, ctx->motion.prev_world_to_view, mo.mp);
    memcpy(mo.vc, ep->world_to_view, 64);
    memcpy(mo.vp, ctx->motion.prev_world_to_view, 64);
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_motion_snapshot(pt_ctx* ctx, int take) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (!take) {
        HIPOK(hipStreamSynchronize(ctx->stream));                       // a trace in flight may still read it
        hipFree(ctx->d_motion_snap.ptr);
        ctx->d_motion_snap.ptr = nullptr; ctx->d_motion_snap.cap = 0;
        ctx->motion_snap_taken = false;
        ctx->motion_snap_counts.clear();
        return PT_OK;
    }
    if (int r = ensure_accel(ctx)) return r;
    ctx->motion_snap_taken = false;
    const size_t need = (size_t)(ctx->n_tris ? ctx->n_tris : 1) * 48;
    if (const hipError_t e = ctx->d_motion_snap.reserve(ctx->stream, need, need + need / 8)) {
        (void)hipGetLastError();
        return ctx->fail(e == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, "motion snapshot: " + std::to_string(need) + " bytes");
    }
    launch_motion_snapshot(ctx->d_tris.as<TriPacket>(), ctx->n_tris, ctx->d_instances.as<InstanceRec>(), (uint32_t)ctx->instances.size(),
                           ctx->d_motion_snap.as<float4>(), ctx->n_tris, ctx->stream);
    HIPOK(hipGetLastError());
    ctx->motion_snap_counts.resize(ctx->instances.size());
    for (size_t i = 0; i < ctx->instances.size(); i++) ctx->motion_snap_counts[i] = ctx->instances[i].tri_count;
    ctx->motion_snap_taken = true;
    return PT_OK;
}

int pt_motion_snapshot_state(pt_ctx* ctx, int32_t* state_out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!state_out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion_snapshot_state: state_out is NULL");
    *state_out = motion_snapshot_state(ctx);
    return PT_OK;
}

int pt_set_motion(pt_ctx* ctx, const pt_motion_config* config) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!config) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: config is NULL");
    if (!config->enable) {                         // nothing else of a disabled config is looked at; the target is no longer written
        ctx->motion.enable = 0;
        ctx->restart_pending = true;
        return PT_OK;
    }
    if (!config->motion) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: the target is NULL");
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(config->prev_world_to_view[i]) || !std::isfinite(config->prev_view_to_clip[i]))
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion: a previous camera matrix has a non-finite entry");
    ctx->motion = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_reproject(pt_ctx* ctx, const pt_reproject_config* config, const void* color, const void* motion, const void* prev_color, const void* prev_motion,
                 const void* prev_length, uint32_t width, uint32_t height, void* out_color, void* out_length) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!color || !motion || !prev_color || !prev_motion || !out_color || !out_length) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: null image");
    if (width == 0 || height == 0 || width > (1u << 30) || height > (1u << 30)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: bad size");
    if ((uint64_t)width * height > 0x7fffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: width * height exceeds 2^31 - 1");
    pt_reproject_config cfg = {0.1f, 32.0f, 0.02f};
    if (config) cfg = *config;
    if (!(cfg.alpha_min >= 0.0f && cfg.alpha_min <= 1.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: alpha_min outside 0..1");
    if (!std::isfinite(cfg.max_history) || !(cfg.max_history >= 1.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: max_history must be finite and >= 1");
    if (!std::isfinite(cfg.depth_tolerance) || !(cfg.depth_tolerance > 0.0f)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: depth_tolerance must be finite and > 0");
    const size_t n = (size_t)width * height, b4 = n * 16, b1 = n * 4;
    if (out_color != color && ranges_overlap(out_color, b4, color, b4)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: out_color overlaps color without being color");
    if (ranges_overlap(out_color, b4, motion, b4) || ranges_overlap(out_color, b4, prev_color, b4) || ranges_overlap(out_color, b4, prev_motion, b4) ||
        (prev_length && ranges_overlap(out_color, b4, prev_length, b1)) || ranges_overlap(out_color, b4, out_length, b1))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: out_color overlaps another image");
    if (ranges_overlap(out_length, b1, color, b4) || ranges_overlap(out_length, b1, motion, b4) || ranges_overlap(out_length, b1, prev_color, b4) ||
        ranges_overlap(out_length, b1, prev_motion, b4) || (prev_length && ranges_overlap(out_length, b1, prev_length, b1)))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "reproject: out_length overlaps an input");
    ENTER(ctx);
    const ReprojectArgs a = {(const float4*)color, (const float4*)motion, (const float4*)prev_color, (const float4*)prev_motion, (const float*)prev_length,
                             (float4*)out_color, (float*)out_length, width, height, cfg.alpha_min, cfg.max_history, cfg.depth_tolerance};
    launch_reproject(a, ctx->stream);
    HIPOK(hipGetLastError());
    return PT_OK;
}

}  // extern "C"
