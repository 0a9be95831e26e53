// wf_passes.hip -- the optional passes of a wavefront trace (pt_wavefront.hip: the stages every trace runs, and the driver): the generate
// stages of a bake and of a probe atlas, the first-hit stages between the primary traversal and the first shade stage (AOVs, ID mattes,
// motion vectors) and the pass resolves launched right before k_wf_resolve (mattes, motion vectors, the variance AOV).  All are off by
// default; each runs once per trace.  What they share with the hot path -- and the bodies they share among themselves -- is pt_wf_stage.h;
// launch_wavefront calls the four host functions at the end of this file.  Compiled as pt_wavefront.hip is.
#define PT_LUT_LDS 1          // k_wf_aov stages the shade stage's tables into LDS (pt_shading.h stage_luts)
#include "pt_wf_stage.h"
#include "pt_bake.h"
#include "pt_probe.h"
#include "pt_matte.h"
#include "pt_motion.h"

namespace pt {

// Texture-space baking (pt_set_bake): the generate stage of an image whose "camera" is a surface.  Slots, tiles, shards and the queue are
// k_wf_generate's; the ray of a (texel, sample) is bake_ray's (pt_bake.h) -- one coverage word, one ShadePacket and one TriPacket per covered
// sample -- and everything behind this launch is the code a camera frame runs.  An uncovered texel has no ray (generate_sparse).
template <bool ADAPTIVE>
__global__ __launch_bounds__(kBlock) void k_wf_generate_bake(FrameConstants fc, WfBuffers wf, Counters* __restrict__ counters, AdaptiveArgs ad, BakeArgs bk, AovArgs av) {
    generate_sparse<ADAPTIVE>(fc, wf, ad, av, [&](uint32_t seed, uint32_t px, uint32_t py, int& rc, Ray& ray) { return bake_ray(fc, bk, seed, px, py, rc, ray); });
}
// Light-probe baking (pt_set_probes): the generate stage of an atlas whose "camera" is a set of points -- k_wf_generate_bake with another ray,
// probe_ray's (pt_probe.h).  The resolution is a multiple of PT_TILE, so a workgroup-round (one tile of one sample) lies in one probe's map:
// the probe index is wave-uniform and the position is read once per wave.  A cell without a probe has no ray (generate_sparse).
template <bool ADAPTIVE>
__global__ __launch_bounds__(kBlock, 7) void k_wf_generate_probe(FrameConstants fc, WfBuffers wf, Counters* __restrict__ counters, AdaptiveArgs ad, ProbeArgs pa, AovArgs av) {
    generate_sparse<ADAPTIVE>(fc, wf, ad, av, [&](uint32_t seed, uint32_t px, uint32_t py, int& rc, Ray& ray) { return probe_ray<true>(fc, pa, seed, px, py, rc, ray); });
}

// First-hit AOVs (pt_set_aov): albedo, shading normal and depth of the vertex the camera ray reaches, one 32-B record per slot.  A stage
// of its own between the primary traversal and the first shade stage -- queue 0's rays and wf.hit are intact in that window -- so that
// the shade stage, priced by the register allocation of its one function, stays what it is.  It walks the shard's segment like every
// stage, stages the tables the vertex fetch and get_surface read, and runs exactly the code the shade stage runs up to the debug
// outputs COLOR / SHADING_NORMAL (shade_closest_hit): the records are those values bit for bit.  A miss writes zeros; so does a
// target whose sample has a non-finite component (no luminance clamp, SHOW_NAN / SHOW_INF do not apply).  Texture taps are not counted.
// The records are written once and read once by the resolve: non-temporal, like the queues.
PT_DEV bool aov_finite(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }
__global__ __launch_bounds__(kBlock) void k_wf_aov(SceneRec sc_in, FrameConstants fc, WfBuffers wf, AovArgs av) {
    SceneRec sc = sc_in; sc.small_tables = 0u;
    const FirstHits hits = first_hits(wf);
    if (hits.none()) return;
    stage_luts(sc);
    stage_tangent_lut(sc);
    stage_instances(sc);
    stage_materials(sc);
    hits.each([&](uint32_t i) {
        const float4 o = QLD(wf.ray_o[0][hits.base + i]), d = QLD(wf.ray_d[0][hits.base + i]), h = QLD(wf.hit[hits.base + i]);
        const uint32_t slot = __float_as_uint(d.w), hb = __float_as_uint(h.w);
        float4 ra = make_float4(0, 0, 0, 0), rn = ra;
        if (hb != kMissTri) {
            const ShadePacket* packet_at = sc.shade + (hb & 0x7fffffffu);
            RawPacket packet = load_shade_packet_raw(packet_at);
            const ShadeInst inst = load_shade_inst(sc, raw_packet_inst(packet));
            if (inst.streams & (SI_TEXCOORD1 | SI_COLOR)) load_shade_packet_extra(packet, packet_at);
            const PacketVerts pv = unpack_shade_packet(packet);
            const RMat* mat = sc.rmats + inst.material_id;
            const MatHeader mh = material_header(sc, inst.material_id);
            HitGeom va = get_vertex_attributes(sc, inst, pv, v3(1 - h.y - h.z, h.y, h.z));
            if (!(hb >> 31)) { va.ng = -va.ng; va.n = -va.n; va.t = -va.t; va.tw = -va.tw; }
            const vec3 view = -normalize(v3(d.x, d.y, d.z));
            unsigned taps = 0;
            const Surface sp = get_surface(sc, fc.flags, mat, mh, va, view, taps);
            ra = make_float4(sp.albedo.x, sp.albedo.y, sp.albedo.z, 1.0f);
            rn = make_float4(sp.n.x, sp.n.y, sp.n.z, h.x);
            if (!aov_finite(ra)) ra = make_float4(0, 0, 0, 0);
            if (!aov_finite(rn)) rn = make_float4(0, 0, 0, 0);
        }
        if (av.albedo) QST(av.rec_albedo[slot], ra);
        if (av.normal_depth) QST(av.rec_normal[slot], rn);
    });
}

// ID mattes (pt_set_matte): which object or material each sample's first ray sees, one 32-bit id per slot.  A stage of its own in k_wf_aov's
// window and far lighter: per entry the slot word of the ray, the hit word, the instance word of the hit's shading packet, for the material
// kind the row's material_id, the id of that row, and one store.  None of the shade stage's LDS tables is needed and none is staged.  The
// records were cleared before the generate stage, so a slot that never had a ray (an uncovered bake texel, a cell without a probe) reads 0
// like a miss.
__global__ __launch_bounds__(kBlock) void k_wf_matte(SceneRec sc, WfBuffers wf, MatteArgs ma) {
    const FirstHits hits = first_hits(wf);
    hits.each([&](uint32_t i) {
        const uint32_t slot = hits.slot(wf, i), hb = hits.hit_word(wf, i);
        uint32_t id = 0u;
        if (hb != kMissTri) {
            uint32_t row = sc.shade[hb & 0x7fffffffu].inst;
            if (ma.kind == PT_MATTE_MATERIAL) row = sc.instances[row].gpu.material_id;
            if (row < ma.n_ids) id = ma.ids[row];
        }
        if (slot < wf.capacity) QST(ma.rec[slot], id);
    });
}
// The matte part of a resolve, a kernel of its own launched right before k_wf_resolve (whose adaptive instantiations update the tiles'
// `active` flags this one reads) on the resolve's grid (resolve_pixel).  A thread reads its pixel's K / 2 float4 once, folds the batch's
// records in sample order with the output's counts (pt_matte.h), sorts and writes once; the K ranks stay in registers (RANKS is a template
// constant: every index is static).  A tile retired by adaptive sampling is not written.
template <int RANKS, bool ADAPTIVE>
__global__ __launch_bounds__(kBlock) void k_wf_matte_resolve(FrameConstants fc, AdaptiveArgs ad, MatteArgs ma) {
    resolve_pixel<ADAPTIVE>(fc, ad, [&](uint32_t pslot, size_t at, int first) {
        MatteRanks<RANKS> m;
#pragma unroll
        for (int j = 0; j < RANKS / 2; j++) matte_unpack(m, j, first > 0 ? ma.layers[j][at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (uint32_t k = 0; k < fc.spp; k++) {
            const uint32_t h = QLD(ma.rec[k * fc.pixel_slots + pslot]);
            matte_fold_sample(m, h, first < 0 ? 0 : first + (int)k);
        }
        matte_sort(m);
#pragma unroll
        for (int j = 0; j < RANKS / 2; j++) ma.layers[j][at] = matte_pack(m, j);
    });
}

// Motion vectors (pt_set_motion): where the surface each sample's first ray sees was in the previous frame, one float4 per slot.  A stage of
// its own in k_wf_aov's window, as light as k_wf_matte: per entry the slot word of the ray, the hit, the hit's TriPacket (one 64-byte line),
// the instance row's tri_offset and the 48-byte snapshot entry, then one non-temporal store.  The four matrices are kernel arguments, hence
// wave-uniform scalars; none of the shade stage's LDS tables is staged.  The records were cleared before the generate stage.
__global__ __launch_bounds__(kBlock) void k_wf_motion(SceneRec sc, WfBuffers wf, MotionArgs ma) {
    const FirstHits hits = first_hits(wf);
    hits.each([&](uint32_t i) {
        const uint32_t slot = hits.slot(wf, i);
        const float4 h = QLD(wf.hit[hits.base + i]);
        const uint32_t hb = __float_as_uint(h.w), tri = hb & 0x7fffffffu;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hb != kMissTri && tri < sc.num_tris) r = motion_record(sc, ma, tri, h.y, h.z);
        if (slot < wf.capacity) QST(ma.rec[slot], r);
    });
}
// The motion part of a resolve, launched as k_wf_matte_resolve is: the target is the running mean of the records with the output's counts,
// by resolve_aov_target.  A tile retired by adaptive sampling is not written.
template <bool ADAPTIVE>
__global__ __launch_bounds__(kBlock) void k_wf_motion_resolve(FrameConstants fc, WfBuffers wf, AdaptiveArgs ad, MotionArgs ma) {
    resolve_pixel<ADAPTIVE>(fc, ad, [&](uint32_t pslot, size_t at, int first) { resolve_aov_target(fc, wf, ma.rec, ma.target, pslot, at, first); });
}

// The variance AOV (pt_set_variance): the per-pixel population variance of the samples the output blends, a kernel of its own launched
// right before k_wf_resolve on the resolve's grid.  At that point the output still holds the means before the batch, every sample's radiance
// is still in the workspace, and the tiles' `active` flags are those the call started with.  A thread keeps the mean m and the variance V in
// registers over the batch: the output is read once, the target read and written once.  Each sample is resolved_sample's, the function the
// resolve itself calls, and m advances by blend_sample, the output's own blend -- so x and m' are the resolve's values, and nothing of m is
// written.  Welford's update in running-mean form (include/mipt.h states it operation by operation; tests/variance_ref.py restates it).
// A non-finite product is replaced by 0 (a select).  A tile retired by adaptive sampling is not written.
PT_DEV float variance_finite_or_zero(float q) { return isfinite(q) ? q : 0.0f; }
template <bool ADAPTIVE>
__global__ __launch_bounds__(kBlock) void k_wf_variance_resolve(FrameConstants fc, WfBuffers wf, const float4* __restrict__ output, AdaptiveArgs ad, VarianceArgs va) {
    resolve_pixel<ADAPTIVE>(fc, ad, [&](uint32_t pslot, size_t at, int first_or_none) {
        const int first = first_or_none < 0 ? 0 : first_or_none;        // samples already in the pixel (a call that does not accumulate has one sample: zeros)
        float4 m = make_float4(0, 0, 0, 0), V = m;
        if (first > 0) { m = output[at]; V = va.target[at]; }
        for (uint32_t k = 0; k < fc.spp; k++) {
            const vec3 x = resolved_sample(fc, wf, k * fc.pixel_slots + pslot);
            const int n = first + (int)k;
            if (n == 0) { V = make_float4(0, 0, 0, 0); m = make_float4(x.x, x.y, x.z, 1.0f); continue; }
            const float b = fdiv(1.0f, (float)n + 1.0f);
            const float4 mn = blend_sample(m, n, x);                    // m' = m + b * d0, the output's own blend
            const vec3 d0 = v3(x.x - m.x, x.y - m.y, x.z - m.z), d1 = v3(x.x - mn.x, x.y - mn.y, x.z - mn.z);
            const float qr = variance_finite_or_zero(d0.x * d1.x), qg = variance_finite_or_zero(d0.y * d1.y), qb = variance_finite_or_zero(d0.z * d1.z);
            const float s0 = (d0.x + d0.y) + d0.z, s1 = (d1.x + d1.y) + d1.z;
            const float qs = variance_finite_or_zero(s0 * s1);
            V = make_float4(V.x + b * (qr - V.x), V.y + b * (qg - V.y), V.z + b * (qb - V.z), V.w + b * (qs - V.w));
            m = mn;
        }
        va.target[at] = V;
    });
}

// ---- host side: what launch_wavefront calls (pt_wavefront.h) -----------------------------------------------------------------------------
// The matte and motion records start as misses: no generate kernel knows of them.
hipError_t passes_begin(PassArgs& a, void* workspace, const WorkspaceLayout& lay, uint32_t slots) {
    a.ad = a.on.adaptive ? a.on.ad : AdaptiveArgs{};
    a.av = a.on.aov ? a.on.av : AovArgs{};
    a.mt = a.on.matte ? a.on.mt : MatteArgs{};
    a.mo = a.on.motion ? a.on.mo : MotionArgs{};
    hipError_t e = hipSuccess;
    if (a.on.aov) { a.av.rec_albedo = (float4*)((char*)workspace + lay.rec_albedo); a.av.rec_normal = (float4*)((char*)workspace + lay.rec_normal); }
    if (a.on.matte) {
        a.mt.rec = (uint32_t*)((char*)workspace + lay.rec_matte);
        if ((e = hipMemsetAsync(a.mt.rec, 0, (size_t)slots * 4, a.stream)) != hipSuccess) return e;
    }
    if (a.on.motion) {
        a.mo.rec = (float4*)((char*)workspace + lay.rec_motion);
        e = hipMemsetAsync(a.mo.rec, 0, (size_t)slots * 16, a.stream);
    }
    return e;
}
void launch_pass_generate(const PassArgs& a, dim3 stage, const FrameConstants& fc, const WfBuffers& wf, Counters* counters) {
    pick(a.on.adaptive, [&](auto ADAPTIVE) {
        if (a.on.probes) hipLaunchKernelGGL((k_wf_generate_probe<ADAPTIVE.value>), stage, dim3(kBlock), 0, a.stream, fc, wf, counters, a.ad, a.on.pa, a.av);
        else hipLaunchKernelGGL((k_wf_generate_bake<ADAPTIVE.value>), stage, dim3(kBlock), 0, a.stream, fc, wf, counters, a.ad, a.on.bk, a.av);
    });
}
// the primary hits, on the stage grid before shade(0) + traverse(0) reuse the arrays
void launch_first_hit_passes(const PassArgs& a, dim3 stage, const SceneRec& sc, const FrameConstants& fc, const WfBuffers& wf) {
    if (a.on.aov) { hipLaunchKernelGGL(k_wf_aov, stage, dim3(kBlock), 0, a.stream, sc, fc, wf, a.av); mark_stage(a.timers, STAGE_SHADE, a.stream); }
    if (a.on.matte) { hipLaunchKernelGGL(k_wf_matte, stage, dim3(kBlock), 0, a.stream, sc, wf, a.mt); mark_stage(a.timers, STAGE_SHADE, a.stream); }
    if (a.on.motion) { hipLaunchKernelGGL(k_wf_motion, stage, dim3(kBlock), 0, a.stream, sc, wf, a.mo); mark_stage(a.timers, STAGE_SHADE, a.stream); }
}
// On the resolve's grid before k_wf_resolve retires tiles -- all see the call's `active` flags -- and, for the variance, before it replaces
// the means the output holds.
void launch_pass_resolves(const PassArgs& a, dim3 full, const FrameConstants& fc, const WfBuffers& wf, const float4* output) {
    const dim3 block(kBlock);
    if (a.on.matte) {
        pick(a.on.adaptive, [&](auto ADAPTIVE) {
            auto launch_matte = [&](auto ranks) { hipLaunchKernelGGL((k_wf_matte_resolve<decltype(ranks)::value, decltype(ADAPTIVE)::value>), full, block, 0, a.stream, fc, a.ad, a.mt); };
            switch (a.mt.ranks) {
                case 2: launch_matte(std::integral_constant<int, 2>()); break;
                case 4: launch_matte(std::integral_constant<int, 4>()); break;
                case 6: launch_matte(std::integral_constant<int, 6>()); break;
                default: launch_matte(std::integral_constant<int, 8>()); break;
            }
        });
        mark_stage(a.timers, STAGE_RESOLVE, a.stream);
    }
    if (a.on.motion) {
        pick(a.on.adaptive, [&](auto ADAPTIVE) { hipLaunchKernelGGL((k_wf_motion_resolve<ADAPTIVE.value>), full, block, 0, a.stream, fc, wf, a.ad, a.mo); });
        mark_stage(a.timers, STAGE_RESOLVE, a.stream);
    }
    if (a.on.variance) {
        pick(a.on.adaptive, [&](auto ADAPTIVE) { hipLaunchKernelGGL((k_wf_variance_resolve<ADAPTIVE.value>), full, block, 0, a.stream, fc, wf, output, a.ad, a.on.va); });
        mark_stage(a.timers, STAGE_RESOLVE, a.stream);
    }
}

}  // namespace pt
