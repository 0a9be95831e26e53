// pt_slab.h -- the arithmetic of the box tests, in one place and free of every other header, so that the traversal (pt_traverse.h), the
// builder (accel.hip) and a host program (tests/host/slab_check.cpp) compile the very same expressions.
//
// A wide node says its children's planes on a grid: plane P* = p + q s, p the node origin, s a power of two, q a byte.  The node test wants the
// distance (P* - o) inv of 24 such planes along one ray.  slab_axis moves the ray into the node's frame once per node and axis,
//      S = s inv                      exact: s is a power of two (and s |inv| is a normal number: |inv| >= 1 for every direction of length <= 1)
//      A = (p - o) inv                the subtraction FIRST: its error is relative to |A|, not to the world coordinate
//      E = 2^-21 (|A| + 255 |S|)      the pad
//      An = A - E,  Af = A + E
// and a plane costs a byte conversion and one fused multiply-add: near = fma(q, S, An) on the side the ray enters, far = fma(q, S, Af) on
// the side it leaves.
//
// What the pad is for.  The candidate gate (pt_traverse.h candidate_stands) asks a triangle's OWN box with own_box_t below, and "no tree
// culls a candidate that stands" needs: whenever the own box passes, every ancestor's node test passes.  With identical arithmetic that was
// monotonicity; here it is an inequality.  u = 2^-24, lo / hi a bound of the triangle's box, inv > 0 (inv < 0 mirrors near and far):
//   - near = fl(q S + fl(A - E)) with A = A* (1 + d1)(1 + d2), A* = (p - o) inv, so near <= (P* - o) inv - E + u (4 |A| + 255 |S| + 2 E):
//     2 u |A| from A's two roundings, u (|A| + E) from the subtraction, u (255 |S| + |A| + E) from the fma;
//   - the gate's distance fl(fl(lo - o) inv) >= (lo - o) inv - 2 u |(lo - o) inv| >= (lo - o) inv - 2 u (|A| + 255 |S|), because lo lies
//     inside the node's box: p <= lo <= p + 255 s;
//   - the builder guarantees P* <= lo EXACTLY (bvh_plane_exceeds; the float check alone lets P* pass lo by half an ulp of a world
//     coordinate, the absolute error this scheme must not re-admit), so (P* - o) inv <= (lo - o) inv;
//   - hence near <= the gate's distance as soon as E (1 - 2 u) >= u (6 |A| + 765 |S|); E = 8 u (|A| + 255 |S|) (1 + d3) leaves room for its
//     own rounding (|A| 2^-21 and the constant 255 2^-21 are exact, the fma rounds once).
//   The far side: far >= the gate's fl(fl(hi - o) inv), the mirror image.  The node test's entry distance is then <= the gate's and its exit
//   distance >= the gate's, and max / min / the * exit_pad on the exit distance are monotone: the gate passing implies the node test passing.
//   The gate and the node test therefore share ONE pad, exit_pad(watertight).  With the watertight triangle test (pt_set_watertight) it is
//   wider: a ray the edge rule of pt_traverse.h accepts passes its triangle's box corner within the rounding of its float32 direction, and
//   with 1.0000004 the gate refuses 10 of the 210 000 edge, vertex and near rays of tests/test_watertight_host.py (printed there; with its edge
//   and vertex cases at 10 000 rays each: 59 of 700 000, up to 1.4e-3 of the vertex-aimed rays of a rotated box; 1 with 1.000001, none from
//   1.000002 on), with 1.000004 none.
// Overflow.  No clamp on S is needed, because E overflows with it: S = +-inf gives E = inf, An = -inf, Af = +inf, and fma(q, S, An / Af) is
//   NaN (q = 0: 0 inf; else inf - inf) or an infinity of the permissive sign; A = +-inf (|p - o| |inv| > 3.4e38 at inv = +-1e30) gives E = inf and
//   An or Af = NaN.  fmaxf / fminf drop a NaN, i.e. the plane is not tested: conservative.  A finite fma that rounds to +-inf does so only
//   where the exact distance is beyond 2^127, which is outside every ray interval.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_HD __host__ __device__ __forceinline__
#else
#define PT_HD inline
#endif
// every expression below is evaluated as written wherever it is inlined (pt_traverse.h's node step allows contraction)
#if defined(__clang__)
#define PT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PT_NO_CONTRACT          // g++: build with -ffp-contract=off
#endif

namespace pt {

// the slack on a box's exit distance, in the node test and in the candidate gate alike (above)
constexpr float kExitPad = 1.0000004f, kExitPadWatertight = 1.000004f;
PT_HD float exit_pad(uint32_t watertight) { return watertight ? kExitPadWatertight : kExitPad; }

// the grid step 2^(exp - 127) of a node axis, and the plane a quantised coordinate stands for in float: the builder checks its boxes
// against this expression (and against the exact sum, below)
PT_HD float bvh_step(uint32_t biased_exp) {
    union { uint32_t u; float f; } c; c.u = biased_exp << 23; return c.f;
}
PT_HD float bvh_dequant(uint32_t q, float step, float origin) { return __builtin_fmaf((float)q, step, origin); }

struct SlabAxis { float S, An, Af; };

PT_HD SlabAxis slab_axis(float step, float p, float o, float inv) {
    PT_NO_CONTRACT
    SlabAxis r;
    r.S = step * inv;
    const float A = (p - o) * inv;
    const float E = __builtin_fmaf(__builtin_fabsf(r.S), 255.0f * 0x1p-21f, __builtin_fabsf(A) * 0x1p-21f);
    r.An = A - E; r.Af = A + E;
    return r;
}
// q: the plane's byte, already a float
PT_HD float slab_near(float q, const SlabAxis& a) { return __builtin_fmaf(q, a.S, a.An); }
PT_HD float slab_far(float q, const SlabAxis& a) { return __builtin_fmaf(q, a.S, a.Af); }

// the candidate gate's distance to a plane of the triangle's own box
PT_HD float own_box_t(float plane, float o, float inv) {
    PT_NO_CONTRACT
    return (plane - o) * inv;
}

// The builder's exact side of the premise: p + q s <= lo, and >= hi, not only after rounding to float.  The sum is exact in double while
// |p| / s < 2^45 (the product has 8 significant bits, the sum spans at most 45 + 8 = 53).  wide_write stays far inside: an axis of non-zero
// extent spans at least one ulp of p, so its step is at least 2^-33 |p|, and on an axis of zero extent every q is 0.
// Both say when a plane must be turned down (false for a NaN bound, like the float comparisons beside them in wide_write).
PT_HD bool bvh_plane_exceeds(uint32_t q, float step, float p, float lo) { return (double)p + (double)q * (double)step > (double)lo; }
PT_HD bool bvh_plane_short_of(uint32_t q, float step, float p, float hi) { return (double)p + (double)q * (double)step < (double)hi; }

}  // namespace pt
