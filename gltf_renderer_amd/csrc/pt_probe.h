// pt_probe.h -- light-probe baking (pt_set_probes, pt_probe_project; include/mipt.h defines both operation by operation, tests/probe_ref.py
// restates them): the device functions the probes' generate kernel and its hook (wf_passes.hip k_wf_generate_probe, debug_wf.hip debug_probe_ray)
// and the projection (probe.hip) share, so that the direction a texel is traced along and the direction it is projected with are told by ONE
// mapping: square_to_sphere of pt_shading.h, the equal-area octahedral map of the environment importance map.
// Both translation units are compiled without floating-point contraction (Makefile): every operation below is the float32 operation, in the
// order written.
#pragma once
#include "pt_vertex.h"
#include "pt_host.h"

namespace pt {

// The atlas cell of pixel (px, py): the probe index k (>= pa.count: the cell is empty) and the texel (lx, ly) within the probe's map.
PT_DEV uint32_t probe_cell(const ProbeArgs& pa, uint32_t px, uint32_t py, uint32_t& lx, uint32_t& ly) {
    const uint32_t cx = fast_div(pa.div_n, px), cy = fast_div(pa.div_n, py);
    lx = px - cx * pa.n; ly = py - cy * pa.n;
    return cy * pa.columns + cx;
}

// The direction of map position (u, v) in [0, 1]^2, world axes, not renormalised (as the environment sample's direction is not)
PT_DEV vec3 probe_direction(float u, float v) { return square_to_sphere(uv_to_square({u, v})); }

// The sample of atlas pixel (px, py) with `seed`: the one draw camera_ray makes (the path reaches its first vertex with kRcAfterCamera), then
// the ray from the probe's position along the jittered texel's direction.  false: the cell holds no probe, `ray` is untouched.
// UNIFORM: every active lane of the wave is in the same cell (the generate kernel: a wave is an 8 x 8 quadrant of a 16 x 16 tile and the
// resolution is a multiple of 16), so the index is taken from the first of them and the position is read once per wave.
template <bool UNIFORM = false>
PT_DEV bool probe_ray(const FrameConstants& fc, const ProbeArgs& pa, uint32_t seed, uint32_t px, uint32_t py, int& rc, Ray& ray) {
    const vec4 r = next_random(px, py, seed, rc);
    uint32_t lx, ly;
    uint32_t k = probe_cell(pa, px, py, lx, ly);
    if (UNIFORM) k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    if (k >= pa.count) return false;
    vec3 o;
    if (UNIFORM) {
        // a wave-uniform address of memory no kernel writes: read through the constant address space, i.e. by scalar loads
        typedef const float __attribute__((address_space(4))) * const_float_p;
        const const_float_p p = (const_float_p)(uintptr_t)(pa.positions + 3 * (size_t)k);
        o = v3(p[0], p[1], p[2]);
    } else {
        const float* __restrict__ p = pa.positions + 3 * (size_t)k;
        o = v3(p[0], p[1], p[2]);
    }
    const float n = (float)pa.n;
    const float u = fdiv(((float)lx + 0.5f) + (r.x - 0.5f), n);      // r.x may be exactly 1 (quirk q17): u = 1 on the map's last column
    const float v = fdiv(((float)ly + 0.5f) + (r.y - 0.5f), n);
    ray.o = o; ray.tmin = 0.0f;
    ray.d = probe_direction(u, v); ray.tmax = pa.max_distance;
    return true;
}

// The real spherical harmonics of bands 0 .. 2 at direction w, in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2);
// the constants are the float32 nearest the exact ones.
constexpr int kProbeSh = 9;
PT_DEV void probe_sh_basis(vec3 w, float (&Y)[kProbeSh]) {
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * w.y;
    Y[2] = 0.488602512f * w.z;
    Y[3] = 0.488602512f * w.x;
    Y[4] = 1.092548431f * (w.x * w.y);
    Y[5] = 1.092548431f * (w.y * w.z);
    Y[6] = 0.315391565f * (3.0f * (w.z * w.z) - 1.0f);
    Y[7] = 1.092548431f * (w.x * w.z);
    Y[8] = 0.546274215f * (w.x * w.x - w.y * w.y);
}

}  // namespace pt
