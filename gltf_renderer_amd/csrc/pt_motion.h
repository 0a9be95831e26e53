// pt_motion.h -- motion vectors (pt_set_motion, include/mipt.h): the record of one sample, shared by k_wf_motion (wf_passes.hip), the
// hook's k_debug_motion and k_motion_snapshot (motion.hip).  Device code only; the arithmetic is that of the header, operation by operation,
// and both translation units compile it without floating-point contraction (Makefile), so that the hook's records are pt_trace's.
#pragma once
#include "pt_math.h"
#include "pt_types.h"
#include "pt_host.h"

namespace pt {

PT_DEV bool motion_finite(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }

// P = (v0 + u * e1) + v * e2, componentwise
PT_DEV vec3 motion_point(const float4 v0, const float4 e1, const float4 e2, float u, float v) {
    return v3((v0.x + u * e1.x) + v * e2.x, (v0.y + u * e1.y) + v * e2.y, (v0.z + u * e1.z) + v * e2.z);
}
// row k of a column-major matrix applied to (P, 1)
PT_DEV float motion_row(const float* M, int k, const vec3 P) { return ((M[k] * P.x + M[4 + k] * P.y) + M[8 + k] * P.z) + M[12 + k]; }
PT_DEV float motion_sx(const float* M, const vec3 P, float w) { return ((fdiv(motion_row(M, 0, P), motion_row(M, 3, P)) + 1.0f) * 0.5f) * w; }
PT_DEV float motion_sy(const float* M, const vec3 P, float h) { return ((1.0f - fdiv(motion_row(M, 1, P), motion_row(M, 3, P))) * 0.5f) * h; }

// The snapshot entry of packet T, or T's own three rows where there is no valid snapshot (or, never in a valid one, the address is outside it)
PT_DEV void motion_previous(const SceneRec& sc, const MotionArgs& ma, const float4 t0, const float4 t1, float4& s0, float4& s1, float4& s2) {
    if (ma.snap == nullptr) return;                                   // (uniform)
    const uint32_t inst = __float_as_uint(t0.w), prim = __float_as_uint(t1.w);
    if (inst >= sc.n_instances) return;
    const uint32_t at = sc.instances[inst].tri_offset + prim;
    if (at >= ma.n_snap) return;
    s0 = ma.snap[3 * (size_t)at]; s1 = ma.snap[3 * (size_t)at + 1]; s2 = ma.snap[3 * (size_t)at + 2];
}

// The record of a hit on packet `tri` with barycentrics (u, v): (previous - current screen position in pixels, previous and current view depth)
PT_DEV float4 motion_record(const SceneRec& sc, const MotionArgs& ma, uint32_t tri, float u, float v) {
    const float4* t = (const float4*)(sc.tris + tri);
    const float4 t0 = t[0], t1 = t[1], t2 = t[2];
    float4 s0 = t0, s1 = t1, s2 = t2;
    motion_previous(sc, ma, t0, t1, s0, s1, s2);
    const vec3 Pc = motion_point(t0, t1, t2, u, v), Pp = motion_point(s0, s1, s2, u, v);
    const float w = (float)ma.width, h = (float)ma.height;
    const float4 r = make_float4(motion_sx(ma.mp, Pp, w) - motion_sx(ma.mc, Pc, w), motion_sy(ma.mp, Pp, h) - motion_sy(ma.mc, Pc, h),
                                 -motion_row(ma.vp, 2, Pp), -motion_row(ma.vc, 2, Pc));
    return motion_finite(r) ? r : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace pt
