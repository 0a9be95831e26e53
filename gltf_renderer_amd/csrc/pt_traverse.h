// pt_traverse.h -- software BVH traversal for gfx950 (replaces DXR TraceRay).
//
// One lane = one ray.  Traversal of 64-B 4-wide nodes with 8-bit quantised child boxes (3 x dwordx4 + 1 x dwordx2
// loads per node; each word holds one bound of all four children, the near and the far word of each axis are picked by the sign of the
// ray's inverse direction).  The slab test of the four boxes is straight VALU on registers, in the NODE's frame: the ray is moved there
// once per node and axis (seven instructions an axis), and each of the 24 planes is a v_cvt_f32_ubyte and one v_fma instead of four
// instructions (pt_slab.h: the arithmetic, its pad, and the proof that no box is culled whose triangle the candidate gate lets stand).
// The stage is short of vector-issue slots, not of node data: about 5.5 waves per SIMD are resident, the VALU pipe is 57 % busy before
// counting its multi-cycle instructions, a wave waits on a memory counter for 22 % of its life (profiles/r03e_instruction_mix.txt), and
// the changes that paid here removed vector instructions from the step (profiles/EXPERIMENTS.md).  Children are visited near-to-far, 48-B world-space
// triangle packets (3 x dwordx4), a per-lane stack held in LDS ([depth][lane] layout: conflict-free
// ds_read/ds_write_b32) with a scratch spill for the rare deep path.
//
// Two drivers over the same step functions:
//   traverse()          one ray per lane until it finishes (megakernel).
//   trace_persistent()  wave-persistent "while-while" loop for the wavefront stages: all lanes first run node
//                       steps until none has an inner node pending, then the lanes holding a leaf test their
//                       triangle; lanes whose ray finished pull a NEW ray from the shard's queue (ballot +
//                       one atomic per wave) once enough lanes are idle.  Measured before this change the
//                       traversal kernels ran with 21-28 % of lanes active (a wave lived as long as its
//                       slowest ray) while the VALU pipe was ~50 % busy: lane refill is the lever.
//
// DXR semantics kept: hit interval tmin < t < tmax, object-space facing (mirrored instances flip), instance
// cull-disable / force-non-opaque flags, any-hit for MASK instances, accept-first-hit occlusion rays,
// the alpha-shadow transmittance product, and, with pt_set_watertight, a WATERTIGHT triangle test: a ray cannot pass
// between two triangles that share an edge or a vertex (edge_rule_inside below).
#pragma once
#include "pt_shading.h"

namespace pt {

#ifndef PT_STACK_LDS
#define PT_STACK_LDS 24
#endif
// Distance to a box plane: (plane - origin) * inv, the subtraction first: its rounding error is RELATIVE to the distance.  plane * inv -
// origin * inv as one fused multiply-add has an ABSOLUTE error, half an ulp of |origin * inv|, and for a short ray that starts
// far from the coordinate origin that is more than any padding -- measured at 1920x1080 on the Sponza-class scene, about one ray in ten
// million then missed a box whose triangle it hits (a wall's box has no thickness), left the scene through the wall and came back as a
// firefly: 43 pixels of a 64-sample frame beyond 1e-2 of the CPU oracle's, image metric 7.9e-4 of the 1e-3 allowed; subtracting first: 2 pixels,
// 4.0e-5.  The node step keeps the subtraction first where it matters, (node origin - ray origin) * inv once per node, and adds
// the plane's offset in the node, q * step * inv, to that: errors relative to the node and the ray, covered by an explicit pad (pt_slab.h).
constexpr int kStackLds = PT_STACK_LDS;       // entries per lane in LDS  (24 * 4 B * 256 lanes = 24 KiB per workgroup)
constexpr int kStackSpill = 40;     // further entries in scratch
constexpr int kBlock = 256;
constexpr int kTravDone = (int)0x80000000;   // `cur` value of a finished ray (leaf refs are ~tri > INT_MIN)

enum : uint32_t { RF_CULL_BACK = 1, RF_CULL_FRONT = 2, RF_FORCE_NON_OPAQUE = 4, RF_ACCEPT_FIRST = 8 };

struct Ray { vec3 o; float tmin; vec3 d; float tmax; };
struct HitRec { float t, u, v; int tri; bool front; };

struct LaneStats { unsigned nodes, tris, taps, overflow, deep; };

// Alpha of a candidate hit: AnyHit / ShadowAnyHit (PathTracer.lib.hlsl:1010-1035, 1053-1079).
PT_DEV void candidate_alpha(const SceneRec& sc, uint32_t inst, int tri, float u, float v, unsigned& taps, float& base_alpha,
                            float& alpha, float& cutoff) {
    const InstanceRec& in = sc.instances[inst];
    vec3 w = v3(1 - u - v, u, v);
    const PacketVerts pv = load_shade_packet(sc.shade + tri);
    vec4 c = fetch_vertex_color(in.p_color != nullptr, pv, w);
    vec2 tc[2] = {fetch_texcoord(in.p_texcoord[0] != nullptr, pv.uv0, w), fetch_texcoord(in.p_texcoord[1] != nullptr, pv.uv1, w)};
    base_color_alpha(sc, sc.rmats + in.gpu.material_id, tc, c, taps, base_alpha, alpha, cutoff);
}

// Per-lane traversal state.
struct Trav {
    vec3 o, d, inv;
    float tmin, tmax;          // original interval
    uint32_t rf, mask;
    int mode;                  // 0 closest hit, 1 occlusion
    bool all_candidates;       // alpha-shadow rays visit every candidate of the ORIGINAL interval (quirk q12)
    int cur, sp;
    HitRec best;
    float transmission;        // ShadowPayload
    bool committed;
};

PT_DEV void trav_init(Trav& t, const SceneRec& sc, const Ray& r, uint32_t rf, uint32_t mask, int mode, float transmission0) {
    t.o = r.o; t.d = r.d; t.tmin = r.tmin; t.tmax = r.tmax;
    // 1 / direction by the compiler's full division (a subnormal component must not give NaN), then CLAMPED to +-1e30: with inv = inf (a
    // direction component that is exactly zero: an orthographic camera looking along a world axis, a mirror bounce off an axis-aligned
    // wall) a slab test made of products with inv meets inf - inf and 0 * inf, both NaN -- the ray then missed every box whose slab it was
    // INSIDE of, i.e. the whole scene.  A huge finite inv keeps them finite: (plane - origin) * 1e30 is far beyond any ray interval with
    // the sign it should have, for every plane farther than |origin| * 2^-24 from the origin's coordinate (what still overflows: pt_slab.h).
    const float kInvMax = 1.0e30f;
    t.inv = v3(clampf(1.0f / r.d.x, -kInvMax, kInvMax), clampf(1.0f / r.d.y, -kInvMax, kInvMax), clampf(1.0f / r.d.z, -kInvMax, kInvMax));
    t.rf = rf; t.mask = mask; t.mode = mode;
    t.all_candidates = (mode == 1) && (rf & RF_FORCE_NON_OPAQUE);
    t.best.t = r.tmax; t.best.tri = -1; t.best.u = 0; t.best.v = 0; t.best.front = true;
    t.transmission = transmission0;
    t.committed = false;
    t.sp = 0;
    t.cur = (mask == 0 || sc.num_tris == 0) ? kTravDone : sc.root;
}

// FAST: the caller has established (wave-uniformly) that no active lane can leave the LDS part of the stack in this step, so
// a push is one predicated ds_write instead of a three-way LDS / scratch / overflow branch nest.
template <bool FAST = false>
PT_DEV void trav_push(Trav& t, const SceneRec& sc, int* lds_stack, int* spill, int ref, LaneStats& st) {
    if (FAST) { lds_stack[t.sp * kBlock] = ref; t.sp++; return; }
    if (t.sp < kStackLds) lds_stack[t.sp * kBlock] = ref;
    else if (t.sp < kStackLds + kStackSpill) spill[t.sp - kStackLds] = ref;
    else if (sc.deep_entries != 0 && t.sp < kStackLds + kStackSpill + (int)sc.deep_entries) {     // (scalar test first: no deep stack in ordinary scenes)
        sc.deep_stack[(size_t)(t.sp - (kStackLds + kStackSpill)) * sc.deep_lanes + blockIdx.x * kBlock + threadIdx.x] = ref;
        st.deep++;
    }
    else st.overflow++;
    if (t.sp < kStackLds + kStackSpill + (int)sc.deep_entries) t.sp++;
}
PT_DEV void trav_pop(Trav& t, const SceneRec& sc, const int* lds_stack, const int* spill) {
    if (t.sp == 0) { t.cur = kTravDone; return; }
    t.sp--;
    // always a ds_read (a select between the LDS and the scratch address would make this a flat_load on every pop)
    int v = lds_stack[min(t.sp, kStackLds - 1) * kBlock];
    asm volatile("" : "+v"(v));                            // keep the two loads apart (the optimiser would re-merge them)
    if (t.sp >= kStackLds) v = spill[min(t.sp, kStackLds + kStackSpill - 1) - kStackLds];
    if (sc.deep_entries != 0 && t.sp >= kStackLds + kStackSpill)
        v = sc.deep_stack[(size_t)(t.sp - (kStackLds + kStackSpill)) * sc.deep_lanes + blockIdx.x * kBlock + threadIdx.x];
    t.cur = v;
}

PT_DEV uint32_t watertight_on(const SceneRec& sc);
#define PT_CSWAP(a, b) { const bool _s = b < a; const uint64_t _lo = _s ? b : a, _hi = _s ? a : b; a = _lo; b = _hi; }

// One inner-node step: t.cur >= 0 on entry; on exit t.cur is the nearest hit child, or the popped entry, or kTravDone.
template <bool COUNT, bool ORDERED = true>
PT_DEV void trav_node_step(Trav& t, const SceneRec& sc, int* lds_stack, int* spill, LaneStats& st) {
#pragma clang fp contract(fast)       // box tests only decide the visiting order: fused multiply-adds here cannot change a hit (csrc/Makefile)
    const float4* np = (const float4*)sc.nodes + (size_t)t.cur * 4;
    const float4 hd = np[0], chf = np[1], qxy = np[2];
#ifdef PT_PROBE_NODE3         // diagnostic build only: no fourth load, the z planes are the x planes' bytes (wrong images: for timing a three-load step)
    const float2 qz = make_float2(qxy.x, qxy.y);
#else
    const float2 qz = *(const float2*)(np + 3);
#endif
    if (COUNT) st.nodes++;
#ifdef PT_PROBE_VALU          // diagnostic build only: PT_PROBE_VALU extra dependent VALU instructions per node step
    { float x = t.tmin; _Pragma("unroll") for (int i = 0; i < PT_PROBE_VALU; i++) asm volatile("v_fma_f32 %0, %0, %0, %0" : "+v"(x)); if (x == 123.456f) st.overflow++; }
#endif
    const float limit = t.all_candidates ? t.tmax : t.best.t;
    const int c0 = __float_as_int(chf.x), c1 = __float_as_int(chf.y), c2 = __float_as_int(chf.z), c3 = __float_as_int(chf.w);
    // the four boxes (pt_types.h Bvh4Node): plane = origin + q * 2^(exp - 127), byte k of each word = child k
    const uint32_t ex = __float_as_uint(hd.w);
    const float sx = bvh_step(ex & 0xffu), sy = bvh_step((ex >> 8) & 0xffu), sz = bvh_step((ex >> 16) & 0xffu);
    const uint32_t wlx = __float_as_uint(qxy.x), whx = __float_as_uint(qxy.y), wly = __float_as_uint(qxy.z), why = __float_as_uint(qxy.w);
    const uint32_t wlz = __float_as_uint(qz.x), whz = __float_as_uint(qz.y);
    // The ray in the node's frame, once per node and axis (pt_slab.h): a plane's distance is then fma((float)q, S, An or Af), a byte conversion
    // and one fused multiply-add instead of dequantise, subtract, multiply.
    const SlabAxis ax = slab_axis(sx, hd.x, t.o.x, t.inv.x), ay = slab_axis(sy, hd.y, t.o.y, t.inv.y), az = slab_axis(sz, hd.z, t.o.z, t.inv.z);
    // The near and the far plane word of all four children are picked by the sign of the ray's inv BEFORE their bytes are converted (two selects
    // per axis), and the slab test uses them directly instead of fminf / fmaxf of every pair of plane distances: 15 vector instructions fewer
    // in every copy of the step (tools/kernel_sizes.sh).  The choice is right: lo <= hi per child (the builder's quantisation keeps the
    // order) and inv is finite and not NaN for every finite direction (trav_init clamps it to +-1e30).  Measured: EXPERIMENTS.md.
    const bool nx = t.inv.x < 0.0f, ny = t.inv.y < 0.0f, nz = t.inv.z < 0.0f;
    const uint32_t wnx = nx ? whx : wlx, wfx = nx ? wlx : whx, wny = ny ? why : wly, wfy = ny ? wly : why, wnz = nz ? whz : wlz, wfz = nz ? wlz : whz;
    const float pad = exit_pad(watertight_on(sc));                  // (uniform: a scalar select)
    bool enters[4];
    float entry[4];
#define PT_Q(W, K) ((float)(((W) >> (8 * (K))) & 0xffu))
#define PT_SLAB(K, CH)                                                                                                    \
    {                                                                                                                     \
        float a0 = slab_near(PT_Q(wnx, K), ax), b0 = slab_far(PT_Q(wfx, K), ax), a1 = slab_near(PT_Q(wny, K), ay);          \
        float b1 = slab_far(PT_Q(wfy, K), ay), a2 = slab_near(PT_Q(wnz, K), az), b2 = slab_far(PT_Q(wfz, K), az);           \
        float tn = fmaxf(fmaxf(a0, a1), fmaxf(a2, t.tmin));                                                                \
        float tx = fminf(fminf(b0, b1), fminf(b2, limit)) * pad;                                                            \
        enters[K] = tn <= tx && CH != kEmptyChild; entry[K] = tn;                                                          \
    }
    PT_SLAB(0, c0) PT_SLAB(1, c1) PT_SLAB(2, c2) PT_SLAB(3, c3)
#undef PT_SLAB
#undef PT_Q
    // a step pushes at most three entries: if no active lane is within three of the LDS part's end, every push is a plain ds_write
    const bool shallow = __ballot(t.sp + 3 > kStackLds) == 0;
    if (!ORDERED) {
        // An accept-first occlusion ray ends at any hit, so its visiting order is free: it goes on with the entering child it enters FARTHEST
        // along the ray.  It starts on a surface, inside the boxes around that surface, which rarely hold its occluder; in an enclosed scene
        // the occluder is the shell at the ray's far end (profiles/EXPERIMENTS.md).  A max over four float keys (a miss is -1, tn >= 0) and
        // first-match selects, no sort; equal keys go to the lowest slot, the child of the largest area.  The other entering children are
        // pushed in ascending slot order.  Alpha-shadow rays multiply transmissions in visiting order: their keys all tie, which is the slot
        // order they always had, bit for bit (a constant in the DEFAULTS copies, which have no such rays).
#define PT_PICK_KEY(K) (enters[K] ? (t.all_candidates ? 0.0f : entry[K]) : -1.0f)
        const float k0 = PT_PICK_KEY(0), k1 = PT_PICK_KEY(1), k2 = PT_PICK_KEY(2), k3 = PT_PICK_KEY(3);
#undef PT_PICK_KEY
        const float far = fmaxf(fmaxf(k0, k1), fmaxf(k2, k3));
        const bool p0 = k0 == far, p1 = !p0 && k1 == far, p2 = !(p0 || p1) && k2 == far, p3 = !(p0 || p1 || p2);
        const int next = far < 0.0f ? kTravDone : (p0 ? c0 : (p1 ? c1 : (p2 ? c2 : c3)));
#define PT_PUSH_UNORDERED(F)                                                                                                        \
        if (enters[0] && !p0) trav_push<F>(t, sc, lds_stack, spill, c0, st);                                                       \
        if (enters[1] && !p1) trav_push<F>(t, sc, lds_stack, spill, c1, st);                                                       \
        if (enters[2] && !p2) trav_push<F>(t, sc, lds_stack, spill, c2, st);                                                       \
        if (enters[3] && !p3) trav_push<F>(t, sc, lds_stack, spill, c3, st);
        if (shallow) { PT_PUSH_UNORDERED(true) } else { PT_PUSH_UNORDERED(false) }
#undef PT_PUSH_UNORDERED
        if (next != kTravDone) t.cur = next; else trav_pop(t, sc, lds_stack, spill);
        return;
    }
    // sort the 4 children as 64-bit (bits of the entry distance, reference) pairs, ascending (tn >= 0, so its bit pattern orders like the
    // float); a miss is all ones and sinks to the end, equal distances go by reference.  The sorted key carries its child: no slot to look
    // up afterwards, and the distance keeps all its bits.
    constexpr uint64_t kMiss = ~0ull;
    uint64_t key[4];
#define PT_KEY(K, CH) key[K] = enters[K] ? ((uint64_t)__float_as_uint(entry[K]) << 32 | (uint32_t)CH) : kMiss;
    PT_KEY(0, c0) PT_KEY(1, c1) PT_KEY(2, c2) PT_KEY(3, c3)
#undef PT_KEY
    PT_CSWAP(key[0], key[1]) PT_CSWAP(key[2], key[3]) PT_CSWAP(key[0], key[2]) PT_CSWAP(key[1], key[3]) PT_CSWAP(key[1], key[2])
    if (key[0] != kMiss) {
#define PT_PUSH_ORDERED(F)                                                                                                          \
        if (key[3] != kMiss) trav_push<F>(t, sc, lds_stack, spill, (int)(uint32_t)key[3], st);                                          \
        if (key[2] != kMiss) trav_push<F>(t, sc, lds_stack, spill, (int)(uint32_t)key[2], st);                                          \
        if (key[1] != kMiss) trav_push<F>(t, sc, lds_stack, spill, (int)(uint32_t)key[1], st);
        if (shallow) { PT_PUSH_ORDERED(true) } else { PT_PUSH_ORDERED(false) }
#undef PT_PUSH_ORDERED
        t.cur = (int)(uint32_t)key[0];
    } else trav_pop(t, sc, lds_stack, spill);
}

// What makes a closed mesh WATERTIGHT (rare path: only for a candidate within the band of one of its triangle's edges).
//   The float Moeller-Trumbore test takes every triangle by its own (v0, e1, e2), and nothing in that arithmetic makes the two triangles of an
//   edge agree on which side of it a ray passes: of rays aimed at a shared edge of a closed mesh 2-14 % were refused by BOTH triangles, of rays
//   aimed at a shared vertex 2-10 % by every triangle of the fan (tests/test_watertight_host.py), and went through the surface.  So inside a
//   band around the edges, |min(u, v, 1 - (u + v))| < kEdgeBand * scale with scale = max(dot(|tv|, |p|), dot(|d|, |q|)) |1 / det|, the float
//   test does not decide.  The three edges are evaluated from the EXACT world-space end points, E = d . ((P - o) x (Q - o)) in float64 without
//   contraction, P and Q in the order of their bit patterns and the sign flipped back: the two triangles of an edge compute the SAME number,
//   and E == 0 counts as inside for both (the tie rule below then picks one).  The candidate is inside if the three signs are the one the
//   float determinant names (det = -(E01 + E12 + E20) in exact arithmetic).  Its t is the float test's, its (u, v) the float test's clamped
//   to u, v >= 0, u + v <= 1.  Outside the band the float test decides as it always did, to the bit: every disagreement between the float
//   test and the edge values that was found lay within 6.5 * 2^-24 * scale of an edge, and the band is 16.
//   The exact end points: the packet holds e1 = fl(w1 - w0), not w1, so they are recomputed as k_setup and k_refit_packets computed them,
//   mul_point of the instance row's transform on the object-space positions of the shading packet of the same index (both of which a refit
//   keeps current) -- two triangles get the same bits from the same vertex.
//   SceneRec::watertight (pt_set_watertight) switches it on, together with the wider exit pad it needs (pt_slab.h).  It is OFF by default:
//   where the float test and the edge values disagree the hit moves to the neighbouring triangle or appears at all, for about one unaimed
//   ray in 10^5 - 10^6, and every recorded parity figure of this repository was taken with the float test alone; off, every bit is as before.
constexpr float kEdgeBand = 16.0f * 0x1p-24f;
PT_DEV uint32_t watertight_on(const SceneRec& sc) {
#ifdef PT_PROBE_WATERTIGHT    // diagnostic build only: the setting on for every context, so that bench.py as it stands times the watertight path (tools/build_variant.sh)
    return 1u;
#else
    return sc.watertight;
#endif
}

PT_DEV double edge_value(vec3 o, vec3 d, vec3 P, vec3 Q) {
#pragma clang fp contract(off)
    const uint32_t px = __float_as_uint(P.x), py = __float_as_uint(P.y), pz = __float_as_uint(P.z);
    const uint32_t qx = __float_as_uint(Q.x), qy = __float_as_uint(Q.y), qz = __float_as_uint(Q.z);
    const bool swap = qx < px || (qx == px && (qy < py || (qy == py && qz < pz)));
    const vec3 A = swap ? Q : P, B = swap ? P : Q;
    const double ax = (double)A.x - (double)o.x, ay = (double)A.y - (double)o.y, az = (double)A.z - (double)o.z;
    const double bx = (double)B.x - (double)o.x, by = (double)B.y - (double)o.y, bz = (double)B.z - (double)o.z;
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double e = (double)d.x * cx + (double)d.y * cy + (double)d.z * cz;
    return swap ? -e : e;
}
// v0: the packet's, which IS the first exact vertex (k_setup stores mul_point's result); the other two are recomputed.
PT_DEV bool edge_rule_inside(vec3 o, vec3 d, vec3 v0, const float* __restrict__ M, const float4* __restrict__ pk, float det) {
#pragma clang fp contract(off)
    const float4 p1 = pk[1], p2 = pk[2];                              // ShadePacket::v[1..2].pos
    // mul_point (pt_math.h), written out so that no including file may contract it
    const vec3 w1 = v3(M[0] * p1.x + M[4] * p1.y + M[8] * p1.z + M[12], M[1] * p1.x + M[5] * p1.y + M[9] * p1.z + M[13], M[2] * p1.x + M[6] * p1.y + M[10] * p1.z + M[14]);
    const vec3 w2 = v3(M[0] * p2.x + M[4] * p2.y + M[8] * p2.z + M[12], M[1] * p2.x + M[5] * p2.y + M[9] * p2.z + M[13], M[2] * p2.x + M[6] * p2.y + M[10] * p2.z + M[14]);
    const double s = det > 0.0f ? -1.0 : 1.0;
    return edge_value(o, d, v0, w1) * s >= 0.0 && edge_value(o, d, w1, w2) * s >= 0.0 && edge_value(o, d, w2, v0) * s >= 0.0;
}

// What makes the answer independent of the TREE (rare path: only for a triangle the triangle test has just accepted).
//  (1) The box gate.  The float test does not decide "inside" exactly: it accepts rays that pass a few ulp (of the ray's length, more at
//      grazing incidence) outside the triangle, hence sometimes outside the triangle's box, and whether a tree's boxes cull such a ray
//      before the triangle is asked depends on the tree -- two trees (this one, the CPU oracle's binary one) then disagree on about one ray
//      in 10^8, each a different path: fireflies.  So a candidate also has to pass the box test of ITS OWN box, in the node test's
//      arithmetic, and its distance has to be consistent with that box.  Every ancestor's box contains the triangle's (the builder checks
//      the exact planes p + q s against it), and the node step's distances, taken in the node's frame with an explicit pad, are never on the
//      wrong side of the distances computed here (pt_slab.h: the inequality and its proof; tests/host/slab_check.cpp), so an ancestor
//      passes whenever the triangle's own box does: no tree culls a candidate that stands, and none is asked about one that does not.
//  (2) The tie rule.  Two triangles at EXACTLY the same distance (coplanar, overlapping surfaces): DXR leaves the winner to the order of the
//      walk; here the lower (instance, primitive) wins.
// The oracle states both the same way (oracle.cpp Tracer::intersect), and its exhaustive search over all triangles finds the same hits.
PT_DEV bool candidate_stands(const Trav& t, const SceneRec& sc, vec3 v0, vec3 e1, vec3 e2, float tt, float limit, uint32_t inst, uint32_t prim) {
    // (1) the box gate
    const vec3 v1 = v0 + e1, v2 = v0 + e2;                                          // the builder's expression for the box (accel.hip k_seg_pass)
    const vec3 lo = hmin(hmin(v0, v1), v2), hi = hmax(hmax(v0, v1), v2);
    const float a0 = own_box_t(lo.x, t.o.x, t.inv.x), b0 = own_box_t(hi.x, t.o.x, t.inv.x), a1 = own_box_t(lo.y, t.o.y, t.inv.y), b1 = own_box_t(hi.y, t.o.y, t.inv.y);
    const float a2 = own_box_t(lo.z, t.o.z, t.inv.z), b2 = own_box_t(hi.z, t.o.z, t.inv.z);
    const float tn = fmaxf(fmaxf(fminf(a0, b0), fminf(a1, b1)), fmaxf(fminf(a2, b2), t.tmin));
    const float tx = fminf(fminf(fmaxf(a0, b0), fmaxf(a1, b1)), fmaxf(a2, b2));
    const float pad = exit_pad(watertight_on(sc));
    if (!(tn <= tx * pad && tn <= tt * pad)) return false;
    if (tt < limit) return true;
    if (!(t.mode == 0 && t.best.tri >= 0)) return false;                // tt == limit: the interval's end, or a tie with the hit held
    const uint4 h0 = *(const uint4*)((const float4*)sc.tris + (size_t)t.best.tri * kTriFloat4), h1 = *(const uint4*)((const float4*)sc.tris + (size_t)t.best.tri * kTriFloat4 + 1);
    return inst < h0.w || (inst == h0.w && prim < h1.w);
}

// One leaf step: t.cur = leaf reference (1..kLeafMax contiguous triangles) on entry; on exit the popped entry or kTravDone.
template <bool COUNT>
PT_DEV void trav_leaf_step(Trav& t, const SceneRec& sc, const int* lds_stack, const int* spill, LaneStats& st) {
    const uint32_t leaf = (uint32_t)~t.cur;
    const int first = (int)(leaf & kLeafFirstMask), count = (int)(leaf >> 28) + 1;
    bool stop = false;
  for (int k = 0; k < count && !stop; k++) {
    const int tri = first + k;
    const float4* tp = (const float4*)sc.tris + (size_t)tri * kTriFloat4;
    float4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
    if (COUNT) st.tris++;
    vec3 v0 = v3(q0.x, q0.y, q0.z), e1 = v3(q1.x, q1.y, q1.z), e2 = v3(q2.x, q2.y, q2.z);
    uint32_t tflags = __float_as_uint(q2.w);
    // Moeller-Trumbore, barycentrics (u, v) = weights of vertex 1 and 2
    vec3 p = cross(t.d, e2);
    float det = dot(e1, p);
    if (det != 0.0f && det == det) {
        float invd = 1.0f / det;
        vec3 tv = t.o - v0;
        float u = dot(tv, p) * invd;
        vec3 q = cross(tv, e1);
        float v = dot(t.d, q) * invd;
        float tt = dot(e2, q) * invd;
        float limit = t.all_candidates ? t.tmax : t.best.t;
        bool inside = (u >= 0.0f) && (u <= 1.0f) && (v >= 0.0f) && (u + v <= 1.0f);
        const bool in_range = (tt > t.tmin) && (tt <= limit);
        if (watertight_on(sc)) {
            // the band around the triangle's edges inside which the float test does not decide (above): kEdgeBand * scale, scale = the larger
            // of dot(|tv|, |p|) and dot(|d|, |q|) times |1 / det| -- the products the sums of u and v are made of
            const float su = fabsf(tv.x * p.x) + fabsf(tv.y * p.y) + fabsf(tv.z * p.z), sv = fabsf(t.d.x * q.x) + fabsf(t.d.y * q.y) + fabsf(t.d.z * q.z);
            const float band = kEdgeBand * fmaxf(su, sv) * fabsf(invd);
            if (__builtin_expect(in_range && fabsf(fminf(fminf(u, v), 1.0f - (u + v))) < band, 0)) {
                inside = edge_rule_inside(t.o, t.d, v0, sc.instances[__float_as_uint(q0.w)].gpu.transform, (const float4*)(sc.shade + tri), det);
                u = fminf(fmaxf(u, 0.0f), 1.0f); v = fminf(fmaxf(v, 0.0f), 1.0f - u);
            }
        }
        bool ok = inside && in_range;
        if (ok) ok = candidate_stands(t, sc, v0, e1, e2, tt, limit, __float_as_uint(q0.w), __float_as_uint(q1.w));
        if (ok && (t.mask & tflags & 0xffu)) {
            bool front = (det > 0.0f) != ((tflags & TF_MIRRORED) != 0);
            bool culled = false;
            if (!(tflags & TF_CULL_DISABLE)) culled = ((t.rf & RF_CULL_BACK) && !front) || ((t.rf & RF_CULL_FRONT) && front);
            if (!culled) {
                bool accept = true;
                if ((tflags & TF_FORCE_NON_OPAQUE) || (t.rf & RF_FORCE_NON_OPAQUE)) {
                    float base_a, a, cutoff;
                    candidate_alpha(sc, __float_as_uint(q0.w), tri, u, v, st.taps, base_a, a, cutoff);
                    if (t.mode == 0) accept = !(base_a < cutoff);                 // IgnoreHit
                    else {
                        t.transmission *= 1 - a;
                        if (t.transmission == 0.0f) stop = true;                  // AcceptHitAndEndSearch
                    }
                }
                if (accept) {
                    t.committed = true;
                    if (!t.all_candidates || tt < t.best.t) { t.best.t = tt; t.best.u = u; t.best.v = v; t.best.tri = tri; t.best.front = front; }
                    if (t.rf & RF_ACCEPT_FIRST) stop = true;
                }
            }
        }
    }
  }
    if (stop) t.cur = kTravDone;
    else trav_pop(t, sc, lds_stack, spill);
}

// mode 0: closest hit (hit group 0).  mode 1: occlusion / shadow (hit group 1), `transmission` is the ShadowPayload.
// Returns true if a hit was committed.
template <bool COUNT>
PT_DEV bool traverse(const SceneRec& sc, int* lds_stack, const Ray& r, uint32_t rf, uint32_t mask, int mode, HitRec& best,
                     float& transmission, LaneStats& st) {
    Trav t;
    int spill[kStackSpill];
    trav_init(t, sc, r, rf, mask, mode, transmission);
    while (t.cur != kTravDone) {
        if (t.cur >= 0) trav_node_step<COUNT>(t, sc, lds_stack, spill, st);
        else trav_leaf_step<COUNT>(t, sc, lds_stack, spill, st);
    }
    best = t.best;
    transmission = t.transmission;
    return t.committed;
}

}  // namespace pt
