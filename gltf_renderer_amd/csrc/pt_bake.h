// pt_bake.h -- texture-space baking (pt_set_bake; include/mipt.h defines it operation by operation, tests/bake_ref.py restates it): the
// device functions the UV rasteriser (bake.hip) and the bake's generate kernel (wf_passes.hip k_wf_generate_bake) share, so that the
// triangle the coverage map chose and the triangle a sample starts on are told by ONE statement of the edge functions.
// Both translation units are compiled without floating-point contraction (Makefile) and `/` and sqrtf are the compiler's correctly rounded
// sequences: every operation below is the IEEE float32 operation, in the order written.
#pragma once
#include "pt_vertex.h"
#include "pt_host.h"

namespace pt {

// E(P, Q, p) = (Q.x - P.x)(p.y - P.y) - (Q.y - P.y)(p.x - P.x)
PT_DEV float bake_edge(vec2 P, vec2 Q, vec2 p) { return (Q.x - P.x) * (p.y - P.y) - (Q.y - P.y) * (p.x - P.x); }

// A triangle's UV vertices in texel units and area2 = E(A, B, C); false: skip test 1 (area2 == 0 or a non-finite coordinate)
struct BakeTri { vec2 A, B, C; float area2; };
PT_DEV bool bake_tri_uv(const ShadePacket* __restrict__ sp, int tex_coord, uint32_t w, uint32_t h, BakeTri& t) {
    const float(*uv)[2] = tex_coord ? sp->uv1 : sp->uv0;
    const float W = (float)w, H = (float)h;
    t.A = {uv[0][0] * W, uv[0][1] * H}; t.B = {uv[1][0] * W, uv[1][1] * H}; t.C = {uv[2][0] * W, uv[2][1] * H};
    t.area2 = bake_edge(t.A, t.B, t.C);
    const bool finite = isfinite(t.A.x) && isfinite(t.A.y) && isfinite(t.B.x) && isfinite(t.B.y) && isfinite(t.C.x) && isfinite(t.C.y);
    return finite && t.area2 != 0.0f;
}
// the triangle covers p iff each edge function is zero or has area2's sign
PT_DEV bool bake_edge_inside(float e, bool positive) { return e == 0.0f || (e > 0.0f) == positive; }
PT_DEV bool bake_covers(const BakeTri& t, vec2 p) {
    const bool positive = t.area2 > 0.0f;
    return bake_edge_inside(bake_edge(t.B, t.C, p), positive) && bake_edge_inside(bake_edge(t.C, t.A, p), positive) && bake_edge_inside(bake_edge(t.A, t.B, p), positive);
}
// n = cross(e1, e2) of the world-space packet and its length; false: skip test 2 (zero or non-finite length)
PT_DEV bool bake_normal(vec3 e1, vec3 e2, vec3& n, float& len) {
    n = cross(e1, e2);
    len = sqrtf(dot(n, n));
    return len > 0.0f && isfinite(len);
}

// The sample of texel (px, py) with `seed`: the one draw camera_ray makes (the path reaches its first vertex with kRcAfterCamera), then the
// ray from surface_offset above the owner's surface point straight down onto it.  false: the texel is uncovered, `ray` is untouched.
// px < fc.res_x and py < fc.res_y.
PT_DEV bool bake_ray(const FrameConstants& fc, const BakeArgs& bk, uint32_t seed, uint32_t px, uint32_t py, int& rc, Ray& ray) {
    const vec4 r = next_random(px, py, seed, rc);
    const uint32_t tri = bk.owner[(size_t)py * fc.res_x + px];
    if (tri == kBakeNone) return false;
    const float jx = r.x - 0.5f, jy = r.y - 0.5f;
    const vec2 p = {(float)px + 0.5f + jx, (float)py + 0.5f + jy};
    BakeTri t;
    bake_tri_uv(bk.shade + tri, bk.tex_coord, fc.res_x, fc.res_y, t);
    const float4* tp = (const float4*)(bk.tris + tri);
    const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
    const vec3 v0 = v3(q0.x, q0.y, q0.z), e1 = v3(q1.x, q1.y, q1.z), e2 = v3(q2.x, q2.y, q2.z);
    float b1 = bake_edge(t.C, t.A, p) / t.area2, b2 = bake_edge(t.A, t.B, p) / t.area2;
    b1 = fmaxf(b1, 0.0f); b2 = fmaxf(b2, 0.0f);                       // a jitter outside the triangle is clamped onto it
    const float b0 = fmaxf((1.0f - b1) - b2, 0.0f);
    const float s = (b0 + b1) + b2;
    b1 = b1 / s; b2 = b2 / s;
    const float keep = 1.0f - 0x1p-10f, third = (float)(0x1p-10 / 3.0);  // strictly inside: the ray cannot slip past an edge
    b1 = b1 * keep + third; b2 = b2 * keep + third;
    const vec3 P = (v0 + b1 * e1) + b2 * e2;
    vec3 n; float len;
    bake_normal(e1, e2, n, len);
    if (__float_as_uint(q2.w) & TF_MIRRORED) n = -n;
    const vec3 Ng = v3(n.x / len, n.y / len, n.z / len);             // the side the traversal reports as front (pt_traverse.h)
    ray.o = P + Ng * bk.surface_offset; ray.tmin = 0.0f;
    ray.d = -Ng; ray.tmax = 2.0f * bk.surface_offset;
    return true;
}

}  // namespace pt
