// pt_vertex.h -- one path vertex of the iterative path tracer (shared by the megakernel and the wavefront
// shade stage).
//
// shade_closest_hit() is ClosestHit (Source/Shaders/PathTracer.lib.hlsl:788-1007) with the recursion removed:
// all random numbers of the vertex are drawn in the reference's order (env NEE, light NEE, BSDF, Russian
// roulette) and the up-to-three follow-up rays are returned as a queue, each shadow ray with its pending
// contribution already multiplied by the path weight beta.  shade_miss() is Miss (:1037-1051).
#pragma once
#include "pt_traverse.h"

namespace pt {

struct PathState {          // Payload (PathTracer.lib.hlsl:110-117) made iterative
    vec3 beta, thr;         // product of bounce weights / the reference's payload.throughput (feeds RR only)
    float prev_pdf;
    int rc, bounce;
    bool prev_mis;
};

struct Followups {
    vec3 add;               // beta-weighted radiance to add to L right away (emissive, untraced NEE, debug colour)
    bool overwrite;         // debug outputs of :969-990 overwrite payload.color
    bool q_env, q_light, q_bounce;
    vec3 pend_env, env_dir, pend_light, light_dir, origin_above;
    vec3 b_o, b_d, b_beta, b_thr;
    float b_pdf;
    bool b_mis;
    unsigned counted_shadow;   // shadow rays the reference traces but whose result a debug mode discards
    // DEAD: left from the rejected occluder cache.  light_index is written (shade_closest_hit), the hints are initialised, nothing reads
    // any of the three; they stay because removing them changes pt_megakernel's register assignment (profiles/EXPERIMENTS.md, "The
    // rejected compile-time alternatives removed": step 2).
    uint32_t light_index;
    uint32_t hint_env, hint_light;
};

// Where a vertex's two UV sets are from the vertex fetch until the last texture of the vertex is sampled (`Park`, a template argument of
// shade_closest_hit).  Every texture picks its set per lane (RT_TEXCOORD1), and a per-lane choice between two members of HitGeom makes the
// compiler keep the pair in scratch: a scratch_load and a wait for vector memory at the head of every texture's address computation.
//   ParkRegisters  the sets stay in HitGeom: the megakernel and the test hooks' kernels, which have no LDS to spare beside their traversal
//                  stack, compile to what they were without the policy (tools/kernel_asm_diff.py: every one of them identical).
//   ParkLds        the shade stage (k_wf_shade): the sets are written once to the lane's column of an LDS array float2[set][lane] -- a
//                  wave's accesses are conflict-free -- and texture_taps reads the chosen one with a single ds_read_b64, on the LDS
//                  counter, not behind vmcnt.  HitGeom::tc is then indexed by constants only and lives in registers.
// Parking more of the vertex's long-lived values this way (L, ps.thr, the environment sample, the follow-ups' origins, directions and
// pending terms, o_below) was measured and bought nothing: profiles/EXPERIMENTS.md, "Shade stage: the UV sets parked in LDS".
static_assert(kParkLanes == kBlock, "the parking's rows are one shade workgroup long");
struct ParkRegisters {
    static constexpr bool kBsdfViewPerVertex = false;
    PT_DEV UvInPlace uv(const HitGeom&) const { return UvInPlace(); }
};
struct ParkLds {
    static constexpr bool kBsdfViewPerVertex = true;
    float2* col;                                           // this lane's column: set s at col[s * kBlock]
    PT_DEV ParkedUv uv(const HitGeom& va) const {
        col[0] = make_float2(va.tc[0].x, va.tc[0].y); col[kBlock] = make_float2(va.tc[1].x, va.tc[1].y);
        return ParkedUv{col};
    }
};

// The environment-map branch of Miss, in three parts (shade_miss and the test hook pt_debug_env_query call them): the radiance along
// `dir`, the solid-angle pdf with which environment_light_sample would have drawn it, and the balance-heuristic weight.
PT_DEV vec3 miss_environment_color(const SceneRec& sc, float environment_intensity, vec3 dir) {
    return sc.has_env ? environment_intensity * sample_cube(sc.env.cube, sc.env.cube_n, dir) : v3(0);
}
PT_DEV float miss_environment_pdf(const SceneRec& sc, vec3 dir) {
    return sc.has_env ? fdiv(importance_map_pdf(sc.env, square_to_uv(sphere_to_square(normalize(dir)))), 4 * kPi) : 0.f;
}
// IEEE division, not fdiv: the previous bounce's pdf can be subnormal, and so can the quotient -- outside fdiv's contract, where its
// result parted from the oracle's (tests/test_gpu_envmap.py).  One division per escaping path.
PT_DEV float miss_mis_weight(float prev_pdf, float env_pdf) { return prev_pdf / (prev_pdf + env_pdf); }   // BalanceHeuristic :383-386

PT_DEV vec3 shade_miss(const SceneRec& sc, const FrameConstants& fc, vec3 dir, const PathState& ps) {
    const uint32_t flags = fc.flags;
    vec3 c;
    if (flags & PT_FLAG_ENVIRONMENT_MAP) {
        c = miss_environment_color(sc, fc.environment_intensity, dir);
        if ((flags & PT_FLAG_ENVIRONMENT_MIS) && ps.prev_mis) c *= miss_mis_weight(ps.prev_pdf, miss_environment_pdf(sc, dir));
    } else c = fc.environment_intensity * v3p(fc.environment_color);
    return ps.beta * c;
}

// Test hook (pt_debug_env_query): one environment-light query per lane, through the production functions.  `in` holds 8 floats and `out`
// 16 floats per query (unused outputs are left alone); `lds_top` as for sample_importance_map.
//   op 0 SAMPLE  in u0, u1, environment_intensity   out sample_importance_map's uv.x, uv.y, pdf, px, py; environment_light_sample's
//                                                    dir.xyz, pdf, color.rgb
//   op 1 PDF     in uv.x, uv.y                       out importance_map_pdf(uv)
//   op 2 CUBE    in dir.xyz                          out sample_cube(dir).rgb, then (face, i, j) of the taps 00, 10, 01, 11 after
//                                                    re-projection (-1 for a direction without a face)
//   op 3 MISS    in dir.xyz, prev_pdf, intensity     out miss colour.rgb, env_pdf, MIS-weighted colour.rgb
constexpr int kEnvQueryIn = 8, kEnvQueryOut = 16;
PT_DEV void debug_env_query(const SceneRec& sc, int op, const float* __restrict__ in, float* __restrict__ out, const float4* lds_top) {
    if (op == 0) {
        float pdf;
        uint32_t px, py;
        const vec2 uv = sample_importance_map_texel(sc.env, in[0], in[1], pdf, lds_top, px, py);
        const EnvSample e = environment_light_sample(sc, in[2], in[0], in[1], lds_top);
        out[0] = uv.x; out[1] = uv.y; out[2] = pdf; out[3] = (float)px; out[4] = (float)py;
        out[5] = e.dir.x; out[6] = e.dir.y; out[7] = e.dir.z; out[8] = e.pdf; out[9] = e.color.x; out[10] = e.color.y; out[11] = e.color.z;
    } else if (op == 1) {
        out[0] = importance_map_pdf(sc.env, {in[0], in[1]});
    } else if (op == 2) {
        const vec3 d = {in[0], in[1], in[2]};
        const vec3 c = sample_cube(sc.env.cube, sc.env.cube_n, d);
        out[0] = c.x; out[1] = c.y; out[2] = c.z;
        size_t a[4]; float w[4];
        const bool ok = cube_footprint(sc.env.cube_n, d, a, w);
        const size_t n = (size_t)sc.env.cube_n;
        for (int t = 0; t < 4; t++) {
            out[3 + 3 * t] = ok ? (float)(a[t] / (n * n)) : -1.0f;
            out[4 + 3 * t] = ok ? (float)(a[t] % n) : -1.0f;
            out[5 + 3 * t] = ok ? (float)(a[t] / n % n) : -1.0f;
        }
    } else {
        const vec3 d = {in[0], in[1], in[2]};
        const vec3 c = miss_environment_color(sc, in[4], d);
        const float env_pdf = miss_environment_pdf(sc, d);
        const vec3 m = c * miss_mis_weight(in[3], env_pdf);
        out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = env_pdf; out[4] = m.x; out[5] = m.y; out[6] = m.z;
    }
}

// Test hook (pt_debug_bsdf_query): one BSDF query per lane, through prepare_bsdf (pt_shading.h: the function shade_closest_hit prepares a
// vertex with) and evaluate_bsdf (op 0) or sample_bsdf (op 1).  Call it with every lane of the wave that has a query and with no other: the
// sheen terms are prepared, and the sheen lobe is run or skipped, by votes of the active lanes.
//   in  48 floats: the reference's SurfaceProperties [0,36) (albedo, alpha, metalness, roughness_squared.xy, shading normal, anisotropy
//       tangent, bitangent, ior, specular colour, specular factor, clearcoat, clearcoat roughness, clearcoat normal, sheen colour, sheen
//       roughness squared, transmissive; thickness and attenuation are not read), geometric normal [36,39), view [39,42), l (op 0) or
//       u.xyz (op 1) [42,45)
//   out 16 floats: f.rgb, pdf, l.xyz, is_transmission, use_mis (op 0: l echoed, both 0), the lobe probabilities alpha, clearcoat, sheen,
//       specular, diffuse, transmission, 0
constexpr int kBsdfQueryIn = 48, kBsdfQueryOut = 16;
template <class Park>
PT_DEV void debug_bsdf_query(const SceneRec& sc, int op, uint32_t flags, const float* __restrict__ in, float* __restrict__ out) {
    Surface sp;
    sp.albedo = v3(in[0], in[1], in[2]); sp.alpha = in[3]; sp.metalness = in[4]; sp.ax = in[5]; sp.ay = in[6];
    sp.n = v3(in[7], in[8], in[9]); sp.at = v3(in[10], in[11], in[12]); sp.ab = v3(in[13], in[14], in[15]); sp.ior = in[16];
    sp.spec_color = v3(in[17], in[18], in[19]); sp.spec_factor = in[20]; sp.clearcoat = in[21]; sp.cc_rough = in[22];
    sp.cc_n = v3(in[23], in[24], in[25]); sp.sheen_color = v3(in[26], in[27], in[28]); sp.sheen_a = in[29]; sp.transmissive = in[30];
    sp.emissive_texel = v3(0);
    const vec3 ng = v3(in[36], in[37], in[38]), view = v3(in[39], in[40], in[41]), a = v3(in[42], in[43], in[44]);
    constexpr bool kVertex = Park::kBsdfViewPerVertex;
    BsdfView bv;
    const Lobes lobes = prepare_bsdf<kVertex>(sc.sheen_e, sp, view, bv);
    vec3 f, l = a;
    float pdf = 0;
    bool is_tr = false, use_mis = false;
    if (op == 0) f = evaluate_bsdf<kVertex>(flags, sc.sheen_e, sp, bv, lobes, ng, view, a, pdf);
    else f = sample_bsdf<kVertex>(flags, sc.sheen_e, sp, bv, lobes, a, view, l, pdf, is_tr, use_mis);
    out[0] = f.x; out[1] = f.y; out[2] = f.z; out[3] = pdf; out[4] = l.x; out[5] = l.y; out[6] = l.z;
    out[7] = is_tr ? 1.0f : 0.0f; out[8] = use_mis ? 1.0f : 0.0f;
    out[9] = lobes.alpha; out[10] = lobes.clearcoat; out[11] = lobes.sheen; out[12] = lobes.specular; out[13] = lobes.diffuse; out[14] = lobes.transmission;
    out[15] = 0.0f;
}
// Test hook (pt_debug_light_query): load_light and light_ray as shade_closest_hit runs them for the light it picked.  out 8 floats:
// direction, colour, cone_terms_staged (1: the cone terms came from the staged copy), 0.
constexpr int kLightQueryOut = 8;
PT_DEV void debug_light_query(const SceneRec& sc, uint32_t li, vec3 p, float* __restrict__ out) {
    vec3 ldir, lcol;
    bool cone_terms_staged;
    const pt_light light = load_light(sc, li, cone_terms_staged);
    light_ray(light, p, ldir, lcol, cone_terms_staged);
    out[0] = ldir.x; out[1] = ldir.y; out[2] = ldir.z; out[3] = lcol.x; out[4] = lcol.y; out[5] = lcol.z;
    out[6] = cone_terms_staged ? 1.0f : 0.0f; out[7] = 0.0f;
}
// Test hook (pt_debug_surface_query): the vertex fetch and the material evaluation of one hit per lane, in shade_closest_hit's order and
// through its functions -- load_shade_packet_raw, load_shade_inst, the voted load_shade_packet_extra, unpack_shade_packet, material_header,
// get_vertex_attributes, the back-face flip, offset_ray both ways, get_surface, emissive_of -- and, separately, the any-hit path's
// candidate_alpha for the same hit.  The statements between the fetch and emissive_of are shade_closest_hit's own, restated here:
// they are not a function there, and the shade stage is not to change for a test hook; change both
// together.  Call it with every lane of the wave that has a query and with no other: the extra packet fetch and the interleaved / general
// and edge / interior texel fetches are behind votes of the active lanes.
//   in   8 words: the packet index (uint32, below sc.num_tris), front (uint32, 0 or 1), u, v, the ray direction d.xyz (view = -normalize(d)), 0
//   out 72 floats:
//       [0,24)   HitGeom after the flip: position, ng, n, t [9,12), tw [12], bt [13,16), colour [16,20), tc[0] [20,22), tc[1] [22,24)
//       [24,55)  Surface as the reference's SurfaceProperties floats [0,31), the order of pt_debug_bsdf_query's input: albedo, alpha, metalness,
//                roughness_squared.xy (ax, ay), shading normal, anisotropy tangent, bitangent, ior, specular colour, specular factor,
//                clearcoat, clearcoat roughness, clearcoat normal, sheen colour, sheen roughness squared, transmissive (thickness and
//                attenuation are not kept by the product and are not here)
//       [55,58)  emissive_of, [58,61) o_above, [61,64) o_below
//       [64]     the texture taps get_surface and emissive_of counted
//       [65,68)  candidate_alpha's base_alpha, alpha, cutoff; [68,72) 0
constexpr int kSurfQueryIn = 8, kSurfQueryOut = 72;
PT_DEV void debug_surface_query(const SceneRec& sc, uint32_t flags, const float* __restrict__ in, float* __restrict__ out) {
    const uint32_t tri = __float_as_uint(in[0]);
    const bool front = __float_as_uint(in[1]) != 0;
    const float hu = in[2], hv = in[3];
    const vec3 d = v3(in[4], in[5], in[6]);
    const ShadePacket* packet_at = sc.shade + tri;
    RawPacket packet = load_shade_packet_raw(packet_at);
    const ShadeInst inst = load_shade_inst(sc, raw_packet_inst(packet));
    if (__any((inst.streams & (SI_TEXCOORD1 | SI_COLOR)) != 0)) {
        if (inst.streams & (SI_TEXCOORD1 | SI_COLOR)) load_shade_packet_extra(packet, packet_at);
    }
    const PacketVerts pv = unpack_shade_packet(packet);
    const RMat* mat = sc.rmats + inst.material_id;
    const MatHeader mh = material_header(sc, inst.material_id);
    HitGeom va = get_vertex_attributes(sc, inst, pv, v3(1 - hu - hv, hu, hv));
    if (!front) { va.ng = -va.ng; va.n = -va.n; va.t = -va.t; va.tw = -va.tw; }                     // :842-846
    const vec3 o_above = offset_ray(va.position, va.ng), o_below = offset_ray(va.position, -va.ng);
    const vec3 view = -normalize(d);
    unsigned taps = 0, taps_any = 0;
    const Surface sp = get_surface(sc, flags, mat, mh, va, view, taps);
    const vec3 em = emissive_of(sc, mat, mh, va.tc, taps, sp.emissive_texel);
    float base_alpha, alpha, cutoff;
    candidate_alpha(sc, pv.inst, (int)tri, hu, hv, taps_any, base_alpha, alpha, cutoff);
    out[0] = va.position.x; out[1] = va.position.y; out[2] = va.position.z; out[3] = va.ng.x; out[4] = va.ng.y; out[5] = va.ng.z;
    out[6] = va.n.x; out[7] = va.n.y; out[8] = va.n.z; out[9] = va.t.x; out[10] = va.t.y; out[11] = va.t.z; out[12] = va.tw;
    out[13] = va.bt.x; out[14] = va.bt.y; out[15] = va.bt.z;
    out[16] = va.color.x; out[17] = va.color.y; out[18] = va.color.z; out[19] = va.color.w;
    out[20] = va.tc[0].x; out[21] = va.tc[0].y; out[22] = va.tc[1].x; out[23] = va.tc[1].y;
    float* s = out + 24;
    s[0] = sp.albedo.x; s[1] = sp.albedo.y; s[2] = sp.albedo.z; s[3] = sp.alpha; s[4] = sp.metalness; s[5] = sp.ax; s[6] = sp.ay;
    s[7] = sp.n.x; s[8] = sp.n.y; s[9] = sp.n.z; s[10] = sp.at.x; s[11] = sp.at.y; s[12] = sp.at.z; s[13] = sp.ab.x; s[14] = sp.ab.y; s[15] = sp.ab.z;
    s[16] = sp.ior; s[17] = sp.spec_color.x; s[18] = sp.spec_color.y; s[19] = sp.spec_color.z; s[20] = sp.spec_factor; s[21] = sp.clearcoat; s[22] = sp.cc_rough;
    s[23] = sp.cc_n.x; s[24] = sp.cc_n.y; s[25] = sp.cc_n.z; s[26] = sp.sheen_color.x; s[27] = sp.sheen_color.y; s[28] = sp.sheen_color.z;
    s[29] = sp.sheen_a; s[30] = sp.transmissive;
    out[55] = em.x; out[56] = em.y; out[57] = em.z;
    out[58] = o_above.x; out[59] = o_above.y; out[60] = o_above.z; out[61] = o_below.x; out[62] = o_below.y; out[63] = o_below.z;
    out[64] = (float)taps; out[65] = base_alpha; out[66] = alpha; out[67] = cutoff;
    out[68] = out[69] = out[70] = out[71] = 0.0f;
}

// Returns true when the path ends at this vertex for a debug output (fu.add holds beta * debug colour).
// -DPT_TIMING (pt_wavefront.hip only; tools/shade_sections.py): cycles per section of this function, summed per wave.
#ifdef PT_TIMING
extern __device__ unsigned long long pt_timing[12];
#define PT_TICK(K) { const unsigned long long _now = __builtin_readcyclecounter(); _sec[K] += _now - _t; _t = _now; }
#define PT_TICK_FLUSH() { if (__lane_id() == (unsigned)(__ffsll((long long)__ballot(1)) - 1)) { for (int _k = 0; _k < 11; _k++) atomicAdd(&pt_timing[_k], _sec[_k]); atomicAdd(&pt_timing[11], 1ull); } }
#else
#define PT_TICK(K)
#define PT_TICK_FLUSH()
#endif
// `packet_in`: the first 80 B of the hit triangle's shading packet (load_shade_packet_raw(packet_at)), fetched by the caller so that it can be
// in flight together with the caller's own fetches; `packet_at` = where the rest is.
// PRE: `pre` is the vertex's environment light sample, drawn ahead of time with this vertex's random numbers (wavefront pipeline:
// the in-place code, its LDS tables and its registers are not compiled in); otherwise it is drawn here.
// `park`: where the UV sets are while the vertex's textures are sampled (ParkRegisters / ParkLds above).
template <bool PRE = false, class Park = ParkRegisters>
PT_DEV bool shade_closest_hit(const SceneRec& sc, const FrameConstants& fc, uint32_t seed, uint32_t px, uint32_t py, const Ray& ray, const HitRec& hit,
                              const RawPacket& packet_in, const ShadePacket* packet_at, PathState& ps, Followups& fu, unsigned& taps, const EnvSample* pre = nullptr,
                              const Park park = Park()) {
    const uint32_t flags = fc.flags;
    fu.add = v3(0); fu.overwrite = false; fu.counted_shadow = 0; fu.light_index = 0; fu.hint_env = fu.hint_light = 0xffffffffu;
    fu.q_env = fu.q_light = fu.q_bounce = false;
#ifdef PT_TIMING
    unsigned long long _sec[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, _t = __builtin_readcyclecounter();
#endif
    const ShadeInst inst = load_shade_inst(sc, raw_packet_inst(packet_in));
    RawPacket packet = packet_in;
    // the second UV set / vertex colours: a second fetch, only in waves that hold a hit on a mesh with either stream
    if (__any((inst.streams & (SI_TEXCOORD1 | SI_COLOR)) != 0)) {
        if (inst.streams & (SI_TEXCOORD1 | SI_COLOR)) load_shade_packet_extra(packet, packet_at);
    }
    const PacketVerts pv = unpack_shade_packet(packet);               // the three vertices and the instance id
    const RMat* mat = sc.rmats + inst.material_id;
    const MatHeader mh = material_header(sc, inst.material_id);
    HitGeom va = get_vertex_attributes(sc, inst, pv, v3(1 - hit.u - hit.v, hit.u, hit.v));
    PT_TICK(0)
    const int dbg = fc.debug_output;
    if (dbg >= PT_DEBUG_OUTPUT_HIT_KIND && dbg <= PT_DEBUG_OUTPUT_TEXCOORD_1) {                       // :806-840
        vec3 c;
        switch (dbg) {
            case PT_DEBUG_OUTPUT_HIT_KIND: c = hit.front ? v3(1, 0, 0) : v3(0, 1, 0); break;
            case PT_DEBUG_OUTPUT_VERTEX_COLOR: c = xyz(va.color); break;
            case PT_DEBUG_OUTPUT_VERTEX_ALPHA: c = v3(va.color.w); break;
            case PT_DEBUG_OUTPUT_VERTEX_NORMAL: c = (va.n + 1) / 2; break;
            case PT_DEBUG_OUTPUT_VERTEX_TANGENT: c = (va.t + 1) / 2; break;
            case PT_DEBUG_OUTPUT_VERTEX_BITANGENT: c = (va.bt + 1) / 2; break;
            case PT_DEBUG_OUTPUT_TEXCOORD_0: c = v3(va.tc[0].x, va.tc[0].y, 0); break;
            default: c = v3(va.tc[1].x, va.tc[1].y, 0); break;
        }
        fu.add = ps.beta * c;
        return true;
    }
    if (!hit.front) { va.ng = -va.ng; va.n = -va.n; va.t = -va.t; va.tw = -va.tw; }                  // :842-846 (float4 negation: w too)
    const vec3 intersection = ray.o + (ray.d * hit.t);                                               // :849
    const vec3 o_above = offset_ray(va.position, va.ng), o_below = offset_ray(va.position, -va.ng);
    const vec3 view = -normalize(ray.d);
    const auto uvs = park.uv(va);
    Surface sp = get_surface(sc, flags, mat, mh, va, view, taps, uvs);
    PT_TICK(1)
    if (dbg >= PT_DEBUG_OUTPUT_COLOR && dbg <= PT_DEBUG_OUTPUT_TRANSMISSIVE) {                       // :863-917
        vec3 c;
        switch (dbg) {
            case PT_DEBUG_OUTPUT_COLOR: c = sp.albedo; break;
            case PT_DEBUG_OUTPUT_ALPHA: c = v3(sp.alpha); break;
            case PT_DEBUG_OUTPUT_SHADING_NORMAL: c = (sp.n + 1) / 2; break;
            case PT_DEBUG_OUTPUT_SHADING_TANGENT: c = (sp.at + 1) / 2; break;
            case PT_DEBUG_OUTPUT_SHADING_BITANGENT: c = (sp.ab + 1) / 2; break;
            case PT_DEBUG_OUTPUT_METALNESS: c = v3(sp.metalness); break;
            case PT_DEBUG_OUTPUT_ROUGHNESS: c = v3(sqrtf(sp.ay)); break;
            case PT_DEBUG_OUTPUT_SPECULAR: c = v3(sp.spec_factor); break;
            case PT_DEBUG_OUTPUT_SPECULAR_COLOR: c = sp.spec_color; break;
            case PT_DEBUG_OUTPUT_CLEARCOAT: c = v3(sp.clearcoat); break;
            case PT_DEBUG_OUTPUT_CLEARCOAT_ROUGHNESS: c = v3(sp.cc_rough); break;
            case PT_DEBUG_OUTPUT_CLEARCOAT_NORMAL: c = (sp.cc_n + 1) / 2; break;
            default: c = v3(sp.transmissive); break;
        }
        fu.add = ps.beta * c;
        return true;
    }
    if (dbg == PT_DEBUG_OUTPUT_HEMISPHERE_VIEW_SIDE) {                                               // :919-922
        fu.add = ps.beta * (dot(view, sp.n) > 0 ? v3(0, 1, 0) : v3(1, 0, 0));
        return true;
    }
    constexpr bool kVertex = Park::kBsdfViewPerVertex;                   // the light-independent terms of the up-to-three evaluations below: once here, or in each
    BsdfView bv;
    const Lobes lobes = prepare_bsdf<kVertex>(sc.sheen_e, sp, view, bv);
    vec3 c = emissive_of(sc, mat, mh, uvs.of(va), taps, sp.emissive_texel);                                                // :925-926
    fu.origin_above = o_above;
    PT_TICK(2)
    // environment NEE :929-942 (SampleEnvironmentMap :688-703)
    if (ps.bounce < fc.max_bounces && (flags & PT_FLAG_ENVIRONMENT_MAP) && (flags & PT_FLAG_ENVIRONMENT_MIS)) {
        EnvSample es;
        if (PRE) { es = *pre; ps.rc++; }                                    // the draw still counts
        else {
            vec4 r = next_random(px, py, seed, ps.rc);
            es = environment_light_sample(sc, fc.environment_intensity, r.x, r.y, importance_lds_top());
        }
        const float light_pdf = es.pdf;
        const vec3 ldir = es.dir, lcol = es.color;
        PT_TICK(6)                                                          // [6] the environment light sample (random numbers, descent, cube)
        vec3 contrib = v3(0);
        if (any_gt0(lcol)) {
            float bp = 0;
            vec3 f = evaluate_bsdf<kVertex>(flags, sc.sheen_e, sp, bv, lobes, va.ng, view, ldir, bp);
            float mis = fdiv(light_pdf, light_pdf + bp);
            contrib = (mis * f * lcol) / light_pdf;
        }
        if (flags & PT_FLAG_INDIRECT_ENVIRONMENT_ONLY) c += contrib;                                 // TraceShadowRay returns 1 untraced (:726-728)
        else {
            fu.pend_env = ps.beta * contrib;
            // The reference traces this ray before it knows the sample is worth anything (:932).  With null-ray culling on, a
            // sample whose weighted contribution is exactly (0,0,0) is not traced: T * 0 adds nothing whatever T is (a NaN term is
            // not zero and is still traced).  Off by default so ray counts match the reference's.
            if (!(fc.cull_null_shadow && fu.pend_env.x == 0.0f && fu.pend_env.y == 0.0f && fu.pend_env.z == 0.0f)) { fu.q_env = true; fu.env_dir = ldir; }
        }
    }
    PT_TICK(3)
    // punctual-light NEE :945-956 (SamplePointLight :680-686)
    if ((flags & PT_FLAG_POINT_LIGHTS) && fc.num_of_lights > 0) {
        float u = next_random(px, py, seed, ps.rc).x;
        uint32_t li = f2u(u * (float)fc.num_of_lights);
        li = min(li, (uint32_t)(fc.num_of_lights - 1));                                              // u may be exactly 1 (quirk q17)
        fu.light_index = li;                                                                         // (dead store, see Followups)
        float pdf = fdiv(1.0f, (float)fc.num_of_lights);
        vec3 ldir, lcol;
        bool cone_terms_staged;
        const pt_light light = load_light(sc, li, cone_terms_staged);
        light_ray(light, intersection, ldir, lcol, cone_terms_staged);
        vec3 contrib = v3(0);
        if (any_gt0(lcol)) {
            float bp = 0;
            vec3 f = evaluate_bsdf<kVertex>(flags, sc.sheen_e, sp, bv, lobes, va.ng, view, ldir, bp);
            contrib = (lcol * f) / pdf;
        }
        if ((flags & PT_FLAG_SHADOW_RAYS) && !(flags & PT_FLAG_INDIRECT_ENVIRONMENT_ONLY)) {
            fu.pend_light = ps.beta * contrib;
            if (!(fc.cull_null_shadow && fu.pend_light.x == 0.0f && fu.pend_light.y == 0.0f && fu.pend_light.z == 0.0f)) { fu.q_light = true; fu.light_dir = ldir; }
        }
        else c += contrib;
    }
    PT_TICK(4)
    fu.add = ps.beta * c;
    // BSDF sampling + Russian roulette :958-1006
    if (ps.bounce < fc.max_bounces) {
        vec4 r = next_random(px, py, seed, ps.rc);
        bool is_tr = false, use_mis = false;
        float bp = 1;
        vec3 l = v3(0);
        vec3 f = sample_bsdf<kVertex>(flags, sc.sheen_e, sp, bv, lobes, v3(r.x, r.y, r.z), view, l, bp, is_tr, use_mis);
        vec3 weight = bp != 0 ? f / bp : v3(0);
        vec3 throughput = ps.thr * weight;
        if (dbg >= PT_DEBUG_OUTPUT_BOUNCE_DIRECTION && dbg <= PT_DEBUG_BOUNCE_IS_TRANSMISSION) {     // :969-990
            vec3 dc;
            switch (dbg) {
                case PT_DEBUG_OUTPUT_BOUNCE_DIRECTION: dc = 0.5f * (l + 1); break;
                case PT_DEBUG_OUTPUT_BOUNCE_BSDF: dc = f; break;
                case PT_DEBUG_OUTPUT_BOUNCE_PDF: dc = v3(bp); break;
                case PT_DEBUG_OUTPUT_BOUNCE_WEIGHT: dc = weight; break;
                default: dc = is_tr ? v3(0, 1, 0) : v3(1, 0, 0); break;
            }
            // payload.color is OVERWRITTEN here: emissive / NEE are discarded; the reference has already traced the NEE
            // shadow rays by now, so they still count as rays.
            fu.counted_shadow = (fu.q_env ? 1u : 0u) + (fu.q_light ? 1u : 0u);
            fu.q_env = fu.q_light = false;
            fu.add = ps.beta * dc;
            fu.overwrite = true;
            return true;
        }
        if (any_gt0(throughput)) {
            float ur = next_random(px, py, seed, ps.rc).x;                                        // drawn even below min_bounces (quirk q6)
            bool cont = ps.bounce < fc.min_bounces;
            if (!cont) {                                                                             // RussianRoulette :712-722
                float p = clampf(max3(throughput), fc.min_rr, fc.max_rr);
                if (ur < p) { weight = weight / p; cont = true; }
            }
            if (cont) {
                fu.q_bounce = true;
                fu.b_o = is_tr ? o_below : o_above;
                fu.b_d = l;
                fu.b_beta = ps.beta * weight;
                fu.b_thr = throughput * weight;                                                      // weight applied twice (quirk q5)
                fu.b_pdf = bp; fu.b_mis = use_mis;
            }
        }
    }
    PT_TICK(5)
    PT_TICK_FLUSH()
    return false;
}

// RayGeneration prologue :744-758 (GenerateCameraRay :131-142)
// the pinhole ray through image position (sx, sy) in pixel units (pixel centres at + 0.5)
PT_DEV Ray pinhole_ray(const FrameConstants& fc, float sx, float sy) {
    float cx = fdiv(sx, (float)fc.res_x) * 2 - 1;
    float cy = fdiv(sy, (float)fc.res_y) * 2 - 1;
    cy = -cy;
    vec4 s = mul4(fc.clip_to_world, vec4{cx, cy, 1, 1});
    vec4 e = mul4(fc.clip_to_world, vec4{cx, cy, 0, 1});
    vec3 o = xyz(s) / s.w;
    vec3 d = xyz(e) / e.w - o;
    Ray ray;
    ray.o = o; ray.tmin = 0; ray.d = normalize(d); ray.tmax = length(d);
    return ray;
}
// Thin lens (absent upstream; include/mipt.h pt_set_lens defines it operation by operation, tests/lens_ref.py restates it in float64):
// the pinhole ray `ray` becomes the ray from lens sample L(u, v) through the pinhole ray's point on the plane in focus.
PT_DEV vec2 lens_sample(const LensArgs& lens, float u, float v) {
    if (lens.blades == 0) return square_to_disk(uv_to_square({u, v}));
    const float s = u * (float)lens.blades;
    const int k = min((int)s, lens.blades - 1);                                      // u may be exactly 1 (quirk q17)
    const float a = sqrtf(s - (float)k);
    // the two vertices by selects over the (wave-uniform) polygon: a per-lane index into the kernel argument would go through scratch
    vec2 v0 = {lens.vert[0][0], lens.vert[0][1]}, v1 = {lens.vert[1][0], lens.vert[1][1]};
    for (int j = 1; j < lens.blades; j++)
        if (j == k) { v0 = {lens.vert[j][0], lens.vert[j][1]}; v1 = {lens.vert[j + 1][0], lens.vert[j + 1][1]}; }
    return a * ((1 - v) * v0 + v * v1);
}
PT_DEV Ray lens_ray(const LensArgs& lens, const Ray& ray, float u, float v) {
    const vec3 c = v3p(lens.c), R = v3p(lens.R), U = v3p(lens.U), F = v3p(lens.F);
    const float zo = dot(ray.o - c, F), dn = dot(ray.d, F);
    const vec3 P = ray.o + ray.d * fdiv(lens.focus - zo, dn);
    const vec3 A = ray.o - ray.d * fdiv(zo, dn);
    const vec2 l = lens.radius * lens_sample(lens, u, v);
    const vec3 A2 = (A + l.x * R) + l.y * U;
    Ray out;
    out.d = normalize(P - A2);
    out.o = A2 + out.d * fdiv(zo, dot(out.d, F));
    out.tmin = 0; out.tmax = ray.tmax;
    return out;
}

// RayGeneration prologue :744-758 (GenerateCameraRay :131-142); with pt_set_lens, the lens ray from the draw's two unused numbers
PT_DEV Ray camera_ray(const FrameConstants& fc, const LensArgs& lens, uint32_t seed, uint32_t px, uint32_t py, int& rc) {
    vec4 r = next_random(px, py, seed, rc);
    float jx = r.x - 0.5f, jy = r.y - 0.5f;
    const Ray ray = pinhole_ray(fc, (float)px + 0.5f + jx, (float)py + 0.5f + jy);
    if (lens.enable) return lens_ray(lens, ray, r.z, r.w);                            // wave-uniform
    return ray;
}

// RayGeneration epilogue :760-785
// `accumulated` = frames already in the output when this sample is blended (SceneConstants.accumulated_frames).
PT_DEV vec3 sanitize_sample(const FrameConstants& fc, vec3 L) {
    const uint32_t flags = fc.flags;
    if (any_nan(L)) L = (flags & PT_FLAG_SHOW_NAN) ? v3(1, 0, 0) : v3(0);
    if (any_inf(L)) L = (flags & PT_FLAG_SHOW_INF) ? v3(1, 0, 0) : v3(0);
    if (flags & PT_FLAG_LUMINANCE_CLAMP) {
        float lum = luminance(L);
        if (lum > fc.luminance_clamp) L *= fdiv(fc.luminance_clamp, lum);
    }
    return L;
}
// the running mean: `h` is the pixel with `accumulated` frames in it
PT_DEV float4 blend_sample(float4 h, int accumulated, vec3 L) {
    float blend = fdiv(1.0f, (float)accumulated + 1.0f);
    return make_float4(h.x + blend * (L.x - h.x), h.y + blend * (L.y - h.y), h.z + blend * (L.z - h.z), h.w + blend * (1.0f - h.w));
}
PT_DEV void write_pixel(const FrameConstants& fc, int accumulated, float4* __restrict__ output, uint32_t px, uint32_t py, vec3 L) {
    L = sanitize_sample(fc, L);
    float4* outp = output + ((size_t)py * fc.res_x + px);
    if ((fc.flags & PT_FLAG_ACCUMULATE) && accumulated != 0) *outp = blend_sample(*outp, accumulated, L);
    else *outp = make_float4(L.x, L.y, L.z, 1.0f);
}

// tile-sharded pixel of a (rank-local) slot: slot -> (tile of this rank, lane in tile), one wave64 per 8x8 quadrant
// sample index of a slot in a sample batch (0 when spp == 1), and the seed that sample draws with
PT_DEV uint32_t fast_div(const FastDiv& f, uint32_t x) { return f.d == 1u ? x : (__umulhi(x, f.mul) >> f.shift); }      // x < 2^31 (pt_types.h FastDiv)
PT_DEV uint32_t slot_sample(const FrameConstants& fc, uint32_t slot) { return fc.spp > 1 ? fast_div(fc.div_pixel_slots, slot) : 0u; }
PT_DEV uint32_t sample_seed(const FrameConstants& fc, uint32_t sample) { return fc.seed + sample * fc.seed_step; }
PT_DEV bool slot_pixel(const FrameConstants& fc, uint32_t slot, uint32_t& px, uint32_t& py) {
    if (fc.spp > 1) slot -= fast_div(fc.div_pixel_slots, slot) * fc.pixel_slots;
    const uint32_t local_tile = slot >> 8, t = slot & 255;
    const uint32_t tile = fc.tile_rank + local_tile * fc.tile_rank_count;
    const uint32_t ty = fast_div(fc.div_tiles_x, tile), tx = tile - ty * fc.tiles_x;
    const uint32_t wave = t >> 6, lane = t & 63;
    px = tx * PT_TILE + (wave & 1) * 8 + (lane & 7);
    py = ty * PT_TILE + (wave >> 1) * 8 + (lane >> 3);
    return (px < fc.res_x) && (py < fc.res_y) && (tile < fc.tiles_x * fc.tiles_y);
}

// wave64 reduction of the per-lane tallies, one atomic per wave per counter
// occlusion: the node / triangle tallies go to Counters::nodes_shadow / tris_shadow (slots 8, 9) instead of nodes / tris (3, 4)
// the two tallies every build keeps (not only the counting instantiations): pushes a full stack dropped, pushes that went to the deep stack
PT_DEV void flush_rare(Counters* __restrict__ counters, const LaneStats& st) {
    if (st.overflow) atomicAdd(&counters->stack_overflow, (unsigned long long)st.overflow);
    if (st.deep) atomicAdd(&counters->deep_pushes, (unsigned long long)st.deep);
}
PT_DEV void flush_counters(Counters* __restrict__ counters, uint32_t lane, unsigned n_primary, unsigned n_bounce, unsigned n_shadow, unsigned n_hits,
                           const LaneStats& st, bool occlusion = false) {
    unsigned vals[8] = {n_primary, n_bounce, n_shadow, st.nodes, st.tris, n_hits, st.taps, st.overflow};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        unsigned v = vals[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        const int slot = (occlusion && (k == 3 || k == 4)) ? k + 5 : k;
        if (lane == 0 && v) atomicAdd(((unsigned long long*)counters) + slot, (unsigned long long)v);
    }
}
// The tallies of the generate and shade stages of the wavefront arrangement do not go to the Counters struct directly: every wave of a
// launch runs dry at the same moment, and their atomics on the struct's one 64-byte line queue up behind each other while the launch waits
// for them.  A wave adds its sums to 64-bit words of a line of its own shard instead (kTally* = the index of the word in that line, as
// unsigned long long; word 0 of the line is the shard counter's), and the resolve stage folds the shards' words into Counters once a
// trace (pt_wavefront.hip, fold_shard_tallies).  64-bit words: a shard's tallies of one trace are not bounded by 2^32.
constexpr int kTallyPrimary = 1, kTallyBounce = 2, kTallyShadow = 3, kTallyHits = 4, kTallyTaps = 5, kTallies = 5;
PT_DEV void flush_shard_tallies(unsigned long long* __restrict__ line, uint32_t lane, unsigned n_primary, unsigned n_bounce, unsigned n_shadow, unsigned n_hits, unsigned taps) {
#ifdef PT_PROBE_NO_FLUSH      // PROBE ONLY: the generate and shade stages count nothing -- wrong pt_stats, what the waves' closing atomics cost
    return;
#endif
    unsigned vals[kTallies] = {n_primary, n_bounce, n_shadow, n_hits, taps};
#pragma unroll
    for (int k = 0; k < kTallies; k++) {
        unsigned v = vals[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0 && v) atomicAdd(line + kTallyPrimary + k, (unsigned long long)v);
    }
}

}  // namespace pt
