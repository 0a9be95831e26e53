// pt_wavefront.hip -- staged (wavefront) arrangement of the path tracer for gfx950.
//
// The frame advances one path vertex at a time through three stages -- trace (closest hit) -> shade ->
// trace (shadow) -- over SoA ray / hit / path-state arrays in HBM (coalesced 16-B-per-lane float4 records).
// The trace stages are small-register kernels that run at 6 waves/SIMD to hide the dependent-load latency
// of BVH traversal; the heavy material code runs only on lanes that have a hit.  MI355X has HBM bandwidth
// to spare (the state traffic is ~300 B per vertex against 8 TB/s) but no RT cores, so occupancy and full
// waves are what buy ray throughput.
//
// Queues are SHARDED: kShards self-contained sub-pipelines.  Workgroup b of every stage launch belongs to
// shard b % kShards; it consumes only its shard's queue segment and pushes only into its shard's segments,
// so an entry never migrates and each segment's size is bounded by what the generate stage put there.
// Surviving paths are compacted with a wave64 ballot and ONE atomic per wave on the shard's counter --
// 32 waves per counter instead of 32 k on one word (a single word saturates at ~88 atomics/us on this
// chip, which made an unsharded queue the bottleneck of every stage).
//
// Determinism: a pixel's radiance is accumulated in its own slot in a fixed order (hit terms, then the
// env-shadow term, then the light-shadow term of that vertex), independent of queue order, so frames are
// bit-reproducible and N tile shards compose bit-exactly.
//
// This file: the stages every trace runs -- generate, trace, shade, fused traversal, shadow, resolve -- and the driver, launch_wavefront.  The
// optional passes (bake / probe generate, AOVs, mattes, motion vectors, variance) are wf_passes.hip's; pt_wf_stage.h is what the two share.
// Product code only: the test hooks that run this file's stages are compiled with its flags in debug_wf.hip (pt_wavefront.h: what they share).
#define PT_LUT_LDS 1          // every stage kernel of this file stages the sRGB table into LDS (pt_shading.h stage_luts)
#include "pt_wf_stage.h"

#ifdef PT_TIMING                 // diagnostic build only (tools/shade_sections.py); not part of the C-ABI
namespace pt { __device__ unsigned long long pt_timing[12]; }
extern "C" int pt_debug_read_timing(unsigned long long* out12, int reset) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out12, HIP_SYMBOL(pt::pt_timing), 96);
    if (reset) { unsigned long long z[12] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(pt::pt_timing), z, 96); }
    return 0;
}
// [8] / [9]: cycles a shade wave is parked behind the queue records of its chunk (round A) and behind what they name -- the packet head
// and the path's state records (round B); [10]: wave-iterations.  Each stamp drains vmcnt, so the rounds are timed apart, not overlapped.
// Since the hit record and the slot word are prefetched there is one round, stamped as [8]; [9] stays 0.
// (The stamp starts BEFORE the round's loads are issued: the compiler puts its own wait at the first use of a result, and it is free to
// schedule that use ahead of a stamp that follows the loads.)
#define PT_WAIT_BEGIN() unsigned long long _a = __builtin_readcyclecounter();
#define PT_WAIT_STAMP(K) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long _b = __builtin_readcyclecounter(); _wait[K] += _b - _a; _a = _b; }
#else
#define PT_WAIT_BEGIN()
#define PT_WAIT_STAMP(K)
#endif
#ifdef PT_UTIL_PROBE             // diagnostic build only (tools/util_probe.py): wave-iterations and active lanes of the traversal phases
namespace pt { __device__ unsigned long long pt_util[16]; }
extern "C" int pt_debug_read_util(unsigned long long* out16, int reset) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out16, HIP_SYMBOL(pt::pt_util), 128);
    if (reset) { unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(pt::pt_util), z, 128); }
    return 0;
}
#define PT_UTIL(i, v) u_acc[i] += (v)
#else
#define PT_UTIL(i, v)
#endif
namespace pt {

// A load that writes LDS and no register (gfx950 global_load_lds_dword / _dwordx4): every active lane's BYTES bytes at `src` land at
// wave_base + lane * BYTES; a lane that is masked off writes nothing.  It counts in vmcnt like any load.  lds_fetch_queue: the queues' non-temporal
// policy (the `nt` bit QLD's loads carry: 2).
#define PT_LDS_FETCH(src, wave_base, BYTES, POLICY) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), (__attribute__((address_space(3))) void*)(wave_base), BYTES, 0, POLICY)
PT_DEV void lds_fetch_queue(const float4* src, float4* wave_base) { PT_LDS_FETCH(src, wave_base, 16, 2); }
PT_DEV void lds_fetch_queue(const uint32_t* src, uint32_t* wave_base) { PT_LDS_FETCH(src, wave_base, 4, 2); }
// s_waitcnt with one counter at zero and the other two left alone (gfx9 encoding: vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8]);
// as the builtin, so that the compiler's own wait insertion sees it, and nothing that touches memory moves across it.
PT_DEV void wait_vector_memory() { __builtin_amdgcn_s_waitcnt(0x0f70); asm volatile("" ::: "memory"); }
PT_DEV void wait_lds() { asm volatile("" ::: "memory"); __builtin_amdgcn_s_waitcnt(0xc07f); asm volatile("" ::: "memory"); }

// The random-sequence counter every path holds after its camera ray (camera_ray draws once): the state of a path at its FIRST vertex is a
// constant -- L = 0, beta = 1, pdf = 0, throughput = 1, rc = kRcAfterCamera, nothing pending -- so the generate stage writes no state and
// the first shade stage reads none.
constexpr int kRcAfterCamera = 1;
// The shade stage is bound by the divergent vector-memory instructions it issues (tools/pmc_shade_attribution.sh: taking the radiance /
// pending records away -- 3 loads, 3 stores, 13 % of its fabric bytes -- made it 10 % faster).  beta / throughput are read by exactly one
// consumer, the shade stage of the next vertex, which already reads the path's queue entry: they ride in two more arrays parallel to the
// closest-ray queue (q_beta / q_thr, coalesced both ways) instead of two slot-indexed arrays (a divergent load and store each).

// One wave of the resolve's workgroup 0: four shards a lane, a wave64 sum, one atomic per field.  (Atomic because the counting copies of
// the traversal kernels and the megakernel book into the same struct.)
PT_DEV void fold_shard_tallies(const WfBuffers& wf, Counters* __restrict__ counters) {
    if (blockIdx.x != 0 || threadIdx.x >= 64u) return;
    unsigned long long v[kTallies] = {0, 0, 0, 0, 0};
    for (uint32_t s = threadIdx.x; s < kShards; s += 64u) {
        const unsigned long long* t = shard_tallies(wf, s);
#pragma unroll
        for (int k = 0; k < kTallies; k++) v[k] += t[kTallyPrimary + k];
    }
    unsigned long long* c[kTallies] = {&counters->rays_primary, &counters->rays_bounce, &counters->rays_shadow, &counters->hits, &counters->taps};
#pragma unroll
    for (int k = 0; k < kTallies; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
        if (threadIdx.x == 0 && v[k]) atomicAdd(c[k], v[k]);
    }
}

// Which pixel tiles a workgroup generates.  Workgroups are dispatched to the eight XCDs round-robin (XCD = blockIdx % 8), every later
// stage launch has the same grid, and shard s = blockIdx % kShards is only ever touched by workgroups with blockIdx % 8 == s % 8:
// a path lives its whole life on ONE XCD.  Tiles are dealt round-robin over all workgroups, so every XCD sees the whole screen: giving
// each XCD a contiguous band of tiles was slower, because the XCD whose band holds the expensive part of the picture finishes last
// while the others idle (profiles/EXPERIMENTS.md).  (kXcds: pt_workspace.h)
// LENS: the instantiations of calls with a thin lens (pt_set_lens); the others are compiled without the lens branch and its registers
// (82 against 34 VGPRs), so that a pinhole call runs the kernel it always ran.
template <bool ADAPTIVE, bool LENS>
__global__ __launch_bounds__(kBlock) void k_wf_generate(FrameConstants fc, WfBuffers wf, Counters* __restrict__ counters, AdaptiveArgs ad, LensArgs lens) {
    if (!LENS) lens.enable = 0;
    const ShardView sv = shard_view(wf);
    // DEAD: the next four lines are left from the rejected per-XCD tile bands; nothing below reads them (gen_region_tiles is always 0).
    // They stay because removing them changes k_wf_generate's code generation (operand order of three scalar multiplies), which puts the
    // removal under the measurement rule of profiles/EXPERIMENTS.md ("The rejected compile-time alternatives removed": step 2).
    const uint32_t per_xcd = gridDim.x / kXcds;
    const uint32_t xcd = blockIdx.x % kXcds, member = blockIdx.x / kXcds;
    uint32_t first_tile = xcd * wf.gen_region_tiles;
    uint32_t n_tiles = first_tile < fc.my_tiles ? min(wf.gen_region_tiles, fc.my_tiles - first_tile) : 0u;
    unsigned n_primary = 0;
    for (uint32_t rnd = 0; rnd < wf.gen_rounds; rnd++) {
        // a workgroup-round is one 16x16 tile of one sample: primary rays stay coherent per wave (8x8 quadrant)
        const uint32_t slot = (rnd * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        const uint32_t sample = slot_sample(fc, slot);
        uint32_t px = 0, py = 0;
        bool valid = slot < wf.capacity && slot_pixel(fc, slot, px, py);
        if (ADAPTIVE) { const bool tile_on = adaptive_tile_active(fc, ad, (rnd * gridDim.x + blockIdx.x) * kBlock); valid = valid && tile_on; }
        int rc = 0;
        Ray ray;
        ray.o = v3(0); ray.d = v3(0, 0, 1); ray.tmin = 0; ray.tmax = 0;
        if (valid) ray = camera_ray(fc, lens, sample_seed(fc, sample), px, py, rc);
        const uint32_t idx = queue_push(wf.cnt[0] + sv.shard * kCounterStride, valid);
        if (valid) {
            const size_t e = (size_t)sv.shard * wf.seg_cap + idx;
            QST(wf.ray_o[0][e], make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tmax));
            QST(wf.ray_d[0][e], make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(slot)));
            n_primary++;
        }
    }
    flush_shard_tallies(shard_tallies(wf, sv.shard), threadIdx.x & 63, n_primary, 0, 0, 0, 0);
}

// Wave-persistent "while-while" traversal of one shard segment with dynamic ray fetch (pt_traverse.h).
// MODE 0: closest hits of queue `cur` -> wf.hit.  MODE 1: occlusion of the shadow queue -> pend_*.w.
#ifndef PT_REFILL
#define PT_REFILL 32          // idle lanes that trigger a refill from the shard queue (swept 8..64 on MI355X: 48 was best in round 1; re-swept after the sample pre-pass: 16 / 24 / 32 / 40 / 48 / 56 -> 5470 / 5507 / 5538 / 5536 / 5500 / 5275 Mrays/s)
#endif
template <bool COUNT, int MODE>
PT_DEV void trace_persistent(const SceneRec& sc, const WfBuffers& wf, int* my_stack, const ShardView& sv, int cur, uint32_t rf_closest, uint32_t rmask,
                             uint32_t flags, LaneStats& st, float shadow_tmax = 0.0f) {
    // MODE 0: `cur` = closest queue (0 / 1).  MODE 1: `cur` = index of the shadow-queue counter (shadow_counter(bounce)).
    const uint32_t n = wf.cnt[cur][sv.shard * kCounterStride];
    uint32_t* head = wf.cnt[MODE == 0 ? 3 : 4] + sv.shard * kCounterStride;
    const size_t base = MODE == 0 ? (size_t)sv.shard * wf.seg_cap : (size_t)sv.shard * wf.seg_cap * 2;
    const uint32_t lane = threadIdx.x & 63;
    int spill[kStackSpill];
    Trav t;
    t.cur = kTravDone; t.sp = 0;
    bool has = false, exhausted = (n == 0);
    uint32_t entry = 0, slot_bits = 0;
#ifdef PT_UTIL_PROBE
    unsigned long long u_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // wave-level: [0] node iterations [1] lanes stepping [2] leaf iterations [3] lanes testing [4] refills [5] lanes refilled [6] lanes holding a ray, summed over node iterations
#endif
    for (;;) {
        // ---- refill idle lanes from the shard queue: ballot + one atomic per wave
        const unsigned long long idle = __ballot(!has);
        const uint32_t nidle = (uint32_t)__popcll(idle);
        if (!exhausted && nidle >= PT_REFILL) {
            const int leader = __ffsll((long long)idle) - 1;
            uint32_t first = 0;
            if ((int)lane == leader) first = atomicAdd(head, nidle);
            first = __shfl(first, leader, 64);
            PT_UTIL(4, 1); PT_UTIL(5, min(nidle, first < n ? n - first : 0u));
            if (!has) {
                const uint32_t i = first + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                if (i < n) {
                    Ray ray;
                    if (MODE == 0) {
                        const float4 o = QLD(wf.ray_o[cur][base + i]), d = QLD(wf.ray_d[cur][base + i]);
                        ray.o = v3(o.x, o.y, o.z); ray.tmin = 0; ray.d = v3(d.x, d.y, d.z); ray.tmax = o.w;
                        trav_init(t, sc, ray, rf_closest, rmask, 0, 0.0f);
                    } else {
                        const float4 o = QLD(wf.sh_o[base + i]), d = QLD(wf.sh_d[base + i]);
                        slot_bits = __float_as_uint(o.w);
                        ray.o = v3(o.x, o.y, o.z); ray.tmin = 0; ray.d = v3(d.x, d.y, d.z); ray.tmax = shadow_tmax;
                        const bool alpha_shadow = (slot_bits >> 31) && (flags & PT_FLAG_ALPHA_SHADOWS);          // TraceShadowRay :724-742
                        uint32_t srf = (flags & PT_FLAG_CULL_BACKFACE) ? RF_CULL_BACK : 0;
                        srf |= alpha_shadow ? RF_FORCE_NON_OPAQUE : RF_ACCEPT_FIRST;
                        trav_init(t, sc, ray, srf, 0xff, 1, alpha_shadow ? 1.0f : 0.0f);
                    }
                    entry = i;
                    has = true;
                }
            }
            if (first + nidle >= n) exhausted = true;
        }
        if (__ballot(has) == 0) {
            if (exhausted) break;
            continue;                                       // cannot happen (all idle -> nidle = 64 >= PT_REFILL), kept for safety
        }
        // ---- node phase: every lane that holds an inner node steps until none does
#ifndef PT_NODE_MIN
#define PT_NODE_MIN 16        // (swept 4..32 at 8 samples per launch: 16) leave the node phase early when fewer lanes than this hold an inner node AND some lane waits at a leaf
                              // (swept 1/4/8/12/16/32 on MI355X: 2195/2326/2359/2360/2356/2294 Mrays/s)
#endif
        for (;;) {
            const unsigned long long at_node = __ballot(has && t.cur >= 0);
            if (at_node == 0) break;
            if (PT_NODE_MIN > 1 && (int)__popcll(at_node) < PT_NODE_MIN && __ballot(has && t.cur < 0 && t.cur != kTravDone) != 0) break;
            PT_UTIL(0, 1); PT_UTIL(1, __popcll(at_node)); PT_UTIL(6, __popcll(__ballot(has)));
            if (has && t.cur >= 0) trav_node_step<COUNT, MODE == 0>(t, sc, my_stack, spill, st);
        }
        // ---- leaf phase
#ifdef PT_UTIL_PROBE
        { const unsigned long long at_leaf = __ballot(has && t.cur != kTravDone && t.cur < 0); if (at_leaf) { PT_UTIL(2, 1); PT_UTIL(3, __popcll(at_leaf)); } }
#endif
        if (has && t.cur != kTravDone && t.cur < 0) trav_leaf_step<COUNT>(t, sc, my_stack, spill, st);
        // ---- retire finished rays
        if (has && t.cur == kTravDone) {
            if (MODE == 0) {
                const uint32_t bits = t.committed ? ((uint32_t)t.best.tri | (t.best.front ? 0x80000000u : 0u)) : kMissTri;
                QST(wf.hit[base + entry], make_float4(t.best.t, t.best.u, t.best.v, __uint_as_float(bits)));
            } else {
                const float tr = t.committed ? t.transmission : 1.0f;                                              // ShadowMiss :1081-1085
                const uint32_t slot = slot_bits & 0x7fffffffu;
                float* w = (slot_bits >> 31) ? &PEND_LIGHT(slot).w : &PEND_ENV(slot).w;
                *w = tr;
            }
            has = false;
        }
    }
#ifdef PT_UTIL_PROBE
    if (lane == 0) for (int k = 0; k < 7; k++) atomicAdd(&pt_util[MODE * 8 + k], u_acc[k]);
#endif
}

// Environment light samples of the path vertices the closest-hit rays of queue `cur` will reach (SampleEnvironmentMap,
// PathTracer.lib.hlsl:688-703: random numbers -> importance-map descent -> direction -> cube-map radiance).  The sample depends on the
// pixel's random sequence only, not on the hit, so it is drawn HERE, by the small-register traversal kernel at 6 waves per SIMD,
// where its three dependent gathers hide behind other waves, instead of in the shade stage at 2 waves per SIMD, where they were a
// fifth of that stage's time (tools/shade_sections.py).  The shade stage reads the result with the queue entry (coalesced, no extra
// round trip) and still counts the draw.  LDS: the importance pyramid's coarse levels are staged into the traversal stack's memory,
// which is idle until the traversal starts.
// Every traversal workgroup draws its share of the shard's samples before it starts traversing.  Measured per 8-spp launch of the bench
// scene: the shade stage 12.1 -> 10.5 ms, the traversal stages 13.0 -> 14.4 ms -- the ~2 k vector instructions of a sample cost nearly as
// much here as there (+0.8 % overall, and 17 KB of LDS a shade workgroup no longer needs).  Handing the samples to dedicated workgroups
// prepended to the traversal launch (1-3 per shard), so that their arithmetic would fill the issue slots of the memory-bound traversal
// waves beside them, was slower still (traversal 14.9-15.0 ms): those slots are not idle.
PT_DEV bool env_prepass_wanted(const SceneRec& sc, const FrameConstants& fc, int vertex_bounce) {
    return sc.has_env && (fc.flags & PT_FLAG_ENVIRONMENT_MAP) && (fc.flags & PT_FLAG_ENVIRONMENT_MIS) && vertex_bounce < fc.max_bounces;
}
PT_DEV void env_prepass(const SceneRec& sc, const FrameConstants& fc, const WfBuffers& wf, int* stack_lds, const ShardView& sv, int cur, bool first_vertex) {
    static_assert((size_t)kStackLds * kBlock * sizeof(int) >= (size_t)kImpLdsFloat4 * sizeof(float4), "the traversal stack's LDS must hold the importance pyramid's coarse levels");
    float4* top = (float4*)stack_lds;
    stage_importance_top_into(sc, top);
    const uint32_t n = wf.cnt[cur][sv.shard * kCounterStride];
    const size_t base = (size_t)sv.shard * wf.seg_cap;
    for (uint32_t i = sv.member * kBlock + threadIdx.x; i < n; i += sv.stride) {
        const uint32_t slot = QLD(*((const uint32_t*)&wf.ray_d[cur][base + i] + 3));
        int rc = kRcAfterCamera;
        if (!first_vertex) rc = (int)(QLD(*((const uint32_t*)&wf.q_thr[cur][base + i] + 3)) & 0xffffu);
        uint32_t px, py;
        slot_pixel(fc, slot, px, py);
        const vec4 r = next_random(px, py, sample_seed(fc, slot_sample(fc, slot)), rc);
        const EnvSample e = environment_light_sample(sc, fc.environment_intensity, r.x, r.y, top);
        QST(wf.env_a[base + i], make_float4(e.dir.x, e.dir.y, e.dir.z, e.pdf));
        QST(wf.env_b[base + i], make_float4(e.color.x, e.color.y, e.color.z, 0.0f));
    }
    __syncthreads();                       // the stack memory goes back to the traversal
}

// Waves per SIMD the traversal kernels are compiled for.  Their 26-KiB LDS stacks admit six, and six need at most 80 VGPRs: the float64 edge
// rule of the leaf step (pt_traverse.h edge_rule_inside, a branch only candidates within rounding of an edge take) would otherwise raise the kernels to
// 101-117 VGPRs, four waves; bound to six the compiler spills inside that branch instead -- and one 8-byte value in the ray refill, which every build pays for,
// the setting on or off (scratch 192 -> 240-352 B; no loss measured: profiles/EXPERIMENTS.md).
#ifndef PT_TRACE_WAVES
#define PT_TRACE_WAVES 6
#endif
// `bounce` = the bounce whose shade stage follows: it fills closest queue cur ^ 1 and the shadow counter of that bounce.
// DEFAULTS (k_wf_trace, k_wf_traverse): a copy compiled for the settings that leave the rays' flags alone -- no back-face culling, no alpha
// shadows, no indirect-environment-only mask (the application's defaults): ray flags 0, mask 0xff and an accept-first shadow search as
// constants take the other searches' code out of the loop (13.87 against 14.04 ms of traversal per launch).  launch_wavefront picks it.
constexpr uint32_t kTravFlagMask = PT_FLAG_CULL_BACKFACE | PT_FLAG_ALPHA_SHADOWS | PT_FLAG_INDIRECT_ENVIRONMENT_ONLY;
template <bool COUNT, bool DEFAULTS>
__global__ __launch_bounds__(kBlock, PT_TRACE_WAVES) void k_wf_trace(SceneRec sc, FrameConstants fc, WfBuffers wf, int cur, int bounce, uint32_t rf, uint32_t rmask, Counters* __restrict__ counters) {
    if (DEFAULTS) { rf = 0; rmask = 0xff; }
    __shared__ int s_stack[kStackLds * kBlock];
    stage_luts(sc);
    const ShardView sv = shard_view(wf);
    if (env_prepass_wanted(sc, fc, bounce)) env_prepass(sc, fc, wf, s_stack, sv, cur, bounce == 0);
    // member 0 of each shard zeroes the counters the following shade stage fills
    if (sv.member == 0 && threadIdx.x == 0) { wf.cnt[cur ^ 1][sv.shard * kCounterStride] = 0; wf.cnt[shadow_counter(bounce)][sv.shard * kCounterStride] = 0; wf.cnt[6][sv.shard * kCounterStride] = 0; }
    LaneStats st = {0, 0, 0, 0};
    trace_persistent<COUNT, 0>(sc, wf, s_stack + threadIdx.x, sv, cur, rf, rmask, 0, st);
    if (COUNT) { flush_counters(counters, threadIdx.x & 63, 0, 0, 0, 0, st); if (st.deep) atomicAdd(&counters->deep_pushes, (unsigned long long)st.deep); }
    else if (st.overflow | st.deep) flush_rare(counters, st);
}

// Fused traversal stage: the occlusion rays of bounce `bounce` AND the closest-hit rays of bounce + 1.  Both were produced by the
// shade stage of `bounce` and neither needs the other's result (the shadow transmissions are only read by the NEXT shade stage), so
// one launch serves both: a wave that runs out of shadow rays goes straight on to pull bounce rays, and the frame has two
// grid-wide synchronisations per bounce instead of three (each one ends on its slowest wave: ~0.07 ms of a 5.5-ms 1-spp frame).
// `nxt` = closest queue the shade stage of `bounce` filled.  Zeroes what the shade stage of bounce + 1 fills.
template <bool COUNT, bool DEFAULTS>
__global__ __launch_bounds__(kBlock, PT_TRACE_WAVES) void k_wf_traverse(SceneRec sc, FrameConstants fc, WfBuffers wf, int nxt, int bounce, uint32_t rf, uint32_t rmask, uint32_t flags,
                                                                        Counters* __restrict__ counters) {
    if (DEFAULTS) { rf = 0; rmask = 0xff; flags &= ~kTravFlagMask; }
    __shared__ int s_stack[kStackLds * kBlock];
    stage_luts(sc);
    const ShardView sv = shard_view(wf);
    if (env_prepass_wanted(sc, fc, bounce + 1)) env_prepass(sc, fc, wf, s_stack, sv, nxt, false);
    if (sv.member == 0 && threadIdx.x == 0) { wf.cnt[nxt ^ 1][sv.shard * kCounterStride] = 0; wf.cnt[shadow_counter(bounce + 1)][sv.shard * kCounterStride] = 0; wf.cnt[6][sv.shard * kCounterStride] = 0; }
    LaneStats st_shadow = {0, 0, 0, 0}, st = {0, 0, 0, 0};
    trace_persistent<COUNT, 1>(sc, wf, s_stack + threadIdx.x, sv, shadow_counter(bounce), 0, 0xff, flags, st_shadow, fc.max_ray_length);
    trace_persistent<COUNT, 0>(sc, wf, s_stack + threadIdx.x, sv, nxt, rf, rmask, 0, st);
    if (COUNT) {
        flush_counters(counters, threadIdx.x & 63, 0, 0, 0, 0, st_shadow, true); flush_counters(counters, threadIdx.x & 63, 0, 0, 0, 0, st);
        if (st.deep | st_shadow.deep) atomicAdd(&counters->deep_pushes, (unsigned long long)st.deep + st_shadow.deep);
    } else if (st.overflow | st_shadow.overflow | st.deep | st_shadow.deep) { flush_rare(counters, st); flush_rare(counters, st_shadow); }
}

// Constants of the dead set-aside scaffolding in k_wf_shade (see the comment there): "no note held", notes in a wave that triggered the
// iteration over them, rare hits in a chunk from which it was shaded in place.
constexpr uint32_t kNoHeld = 0xffffffffu;
constexpr int kDeferFlush = 60;
constexpr uint32_t kDeferMajority = 4;
#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 2      // waves per SIMD the register allocator must leave room for (2 -> <= 256 VGPR+AGPR)
#endif
// SPECIAL != 0: a copy of the kernel compiled for ONE setting of the flags the shade stage reads (kShadeFlagMask) and no debug output -- the
// application's defaults (Main.cpp:462-469), with and without punctual lights.  The flag tests are wave-uniform branches either way; as
// constants they also take the code of the other settings (the non-MIS evaluation, the white-material override, 27 debug outputs ...) out of
// the function, and what that does to its register allocation is worth more than the branches: shade stage 9.02 -> 8.69 ms per launch, +1.6 %
// rays/s, images bit-identical.  launch_wavefront picks the copy whose bits match the frame's flags, else the general kernel (SPECIAL = 0).
constexpr uint32_t kShadeFlagMask = PT_FLAG_MATERIAL_DIFFUSE_WHITE | PT_FLAG_MATERIAL_MIS | PT_FLAG_MATERIAL_USE_GEOMETRIC_NORMALS | PT_FLAG_SHADING_NORMAL_ADAPTATION |
                                    PT_FLAG_ENVIRONMENT_MAP | PT_FLAG_ENVIRONMENT_MIS | PT_FLAG_INDIRECT_ENVIRONMENT_ONLY | PT_FLAG_POINT_LIGHTS | PT_FLAG_SHADOW_RAYS;
constexpr uint32_t kShadeSpecialised = 0x80000000u;          // marks a non-zero SPECIAL (a flag set could be 0)
constexpr uint32_t kShadeDefaultsNoLights = PT_FLAG_SHADOW_RAYS | PT_FLAG_ENVIRONMENT_MAP | PT_FLAG_ENVIRONMENT_MIS | PT_FLAG_MATERIAL_MIS | PT_FLAG_SHADING_NORMAL_ADAPTATION;
constexpr uint32_t kShadeDefaults = kShadeDefaultsNoLights | PT_FLAG_POINT_LIGHTS;
// SMALL: the scene's instance rows, materials and lights all fit the LDS copies (<= 128 / 96 / 32: every BASELINE config): as a constant this
// removes the global-memory branch of every table lookup (shade stage 8.70 -> 8.52 ms per launch).
// LDS of a workgroup, 59 904 B: the tables take 50 688 B (sRGB and sheen tables 2 048, tangent angles 8 192, 128 instance rows 12 288,
// 96 materials x 17 float4 26 112, 32 lights 2 048; the dead s_hand is compiled out), the parking of the two UV sets 4 096 B (ParkLds,
// pt_vertex.h: float2[2][256]) and the prefetch of the next chunk's hit records and slot words 5 120 B (s_pre below: 16 + 4 B a lane).
// 256 VGPRs put two workgroups on a CU; their 119 808 B fit its 160 KiB, and every copy's code object says Occupancy 2.
// With the parking no copy selects between the UV sets in scratch: the two specialised copies have no scratch frame at all
// (it was 100 B), and the shade stage went from 8.01 to 7.38 ms per 8-spp launch, images bit-identical.
// the shading packet a queue entry's hit word names; a miss reads packet 0 and uses nothing of it
PT_DEV const ShadePacket* packet_of(const SceneRec& sc, uint32_t hb) {
#ifdef PT_PROBE_NO_PACKET     // PROBE ONLY: every hit reads one of 64 packets -- wrong geometry, what the shading-packet gathers cost
    return sc.shade + (hb == kMissTri ? 0u : (hb & 63u));
#else
    return sc.shade + (hb == kMissTri ? 0u : (hb & 0x7fffffffu));
#endif
}
template <uint32_t SPECIAL, bool SMALL>
__global__ __launch_bounds__(kBlock, PT_SHADE_WAVES) void k_wf_shade(SceneRec sc_in, FrameConstants fc_in, WfBuffers wf, int cur, int bounce, Counters* __restrict__ counters) {
    SceneRec sc = sc_in; sc.small_tables = SMALL ? 1u : 0u;
    FrameConstants fc = fc_in;
    if (SPECIAL) { fc.flags = (fc_in.flags & ~kShadeFlagMask) | (SPECIAL & kShadeFlagMask); fc.debug_output = PT_DEBUG_OUTPUT_NONE; }
    {   // a workgroup whose share of the shard's queue is empty (most of them from the third bounce on) leaves before it stages
        // 67 KB of tables into LDS; member 0 stays for the head rewind below
        const ShardView sv0 = shard_view(wf);
        if (sv0.member != 0 && sv0.member * kBlock >= wf.cnt[cur][sv0.shard * kCounterStride]) return;
    }
    stage_luts(sc);
    stage_tangent_lut(sc);
    stage_lights(sc, fc.num_of_lights);
    stage_instances(sc);
    stage_materials(sc);
    const ShardView sv = shard_view(wf);
    const uint32_t n = wf.cnt[cur][sv.shard * kCounterStride];
    const int nxt = cur ^ 1;
    const size_t base = (size_t)sv.shard * wf.seg_cap, sbase = (size_t)sv.shard * wf.seg_cap * 2;
    uint32_t* cnt_next = wf.cnt[nxt] + sv.shard * kCounterStride;
    uint32_t* cnt_shadow = wf.cnt[shadow_counter(bounce)] + sv.shard * kCounterStride;
    // the dynamic-fetch heads of both trace stages are idle while shading runs: rewind them here
    if (sv.member == 0 && threadIdx.x == 0) { wf.cnt[3][sv.shard * kCounterStride] = 0; wf.cnt[4][sv.shard * kCounterStride] = 0; }
    unsigned n_bounce = 0, n_shadow = 0, n_hits = 0;
    LaneStats st = {0, 0, 0, 0};
    // Every WAVE pulls the next 64 entries of its shard's queue from the shard's head counter (one atomic per wave and chunk, the next
    // chunk requested before the current one is shaded, so its round trip is hidden).  Hits differ in cost and a queue is rarely a
    // multiple of the grid's stride: with static rounds a launch ran as long as the workgroups that had one chunk more (a 1-spp
    // 1080p frame: 5.27 rounds' worth of work took 6 rounds).
    uint32_t* shade_head = wf.cnt[6] + sv.shard * kCounterStride;
    const uint32_t lane64 = threadIdx.x & 63u;
    // What gates the addresses of a chunk's other fetches -- the hit record (its word 3 names the shading packet) and the slot word of ray_d
    // (it names the path's state records) -- is asked for ONE CHUNK AHEAD, by loads that write the wave's own LDS buffer (lds_fetch_queue: no
    // register holds them meanwhile; the kernel has none to spare).  Iteration k issues entry(k+1) at its top, as soon as k's copy is read out
    // -- chunk k+1 was reserved by the tail of iteration k-1, in the same atomic instruction as the queue space, so its index is there without
    // a wait.  Iteration k+1 then starts from two ds_reads and issues everything else at once -- ray_o, ray_d, env_a / env_b, q_beta / q_thr,
    // the packet head, L and the pending records -- in ONE round trip where there were two dependent ones.  The buffer is wave-private and
    // lane-linear, so the loop has no barrier; lanes past the queue's end fetch nothing; no address is read that was not read before.
    // (Fetching the packet head ahead as well, into five more pieces of 16 B a lane, was measured and was slower: profiles/EXPERIMENTS.md,
    // "Shade stage: the next chunk's hit record and slot word prefetched into LDS".)
    __shared__ float4 s_pre[kBlock + kBlock / 4];                    // [lane of the workgroup] wf.hit; behind it [lane of the workgroup] the slot words, 4 B each
    // (a wave's 64 lanes are contiguous in each image: a load's destination is a wave-uniform base, held in scalar registers like the sources')
    const uint32_t wave_lane0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    float4* const pre_wave = s_pre + wave_lane0;
    uint32_t* const pre_slot_wave = (uint32_t*)(s_pre + kBlock) + wave_lane0;
    // A lane's byte offset into the hit image and into a queue record array alike.  Formed anew wherever it is used, from a copy of the lane
    // number the compiler cannot see through: hoisted out of the loop it is one live register more across the vertex, and the timed copy for
    // punctual lights then spills.
    const auto lane_bytes = [&]() { uint32_t l = lane64; asm volatile("" : "+v"(l)); return l * 16u; };
    const auto fetch_entry = [&](uint32_t c, uint32_t lb) {         // c: wave-uniform
        if (c + lane64 < n) {
            lds_fetch_queue((const float4*)((const char*)(wf.hit + base + c) + lb), pre_wave);
            lds_fetch_queue((const uint32_t*)((const char*)(wf.ray_d[cur] + base + c) + 12 + lb), pre_slot_wave);
        }
    };
    uint32_t chunk = 0, next_chunk = 0;
    if (lane64 == 0) chunk = atomicAdd(shade_head, 64u);
    chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
    if (chunk < n) {                                                 // the wave's first chunk: nothing to hide its fetches behind
        if (lane64 == 0) next_chunk = atomicAdd(shade_head, 64u);
        fetch_entry(chunk, lane_bytes());
        wait_vector_memory();
    }
    next_chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_chunk);
    // DEAD CODE, kept on purpose: `defer_on`, `held`, `flush`, `s_hand` and `set_aside` are what is left of an experiment that set hits on
    // rare materials (sheen) aside and shaded them together, a wave's notes packed onto free lanes through LDS.  It was measured and
    // rejected, and its switch is gone: defer_on is false, so flush and set_aside are always false, held is always kNoHeld, and the block
    // under "2." below never runs.  The variables stay only because k_wf_shade sits at its register limit and taking them out changes its
    // code generation; that removal was measured too and fell below the parent's range (profiles/EXPERIMENTS.md, "The rejected
    // compile-time alternatives removed": step 2).  Read the loop as: every wave shades chunk after chunk until its shard's queue is empty.
    const bool defer_on = false;
    uint32_t held = kNoHeld;
    __shared__ uint32_t s_hand[kBlock];                              // the hand-over slots, 64 per wave
    uint32_t* hand = s_hand + (threadIdx.x & ~63u);
    __shared__ float2 s_park[2 * kBlock];                            // the UV sets of the hit each lane is shading: [set][lane]
    const ParkLds park = {s_park + threadIdx.x};
#ifdef PT_TIMING
    unsigned long long _wait[3] = {0, 0, 0};
#endif
    for (;;) {
        const bool more = chunk < n;
        const unsigned long long held_mask = __ballot(held != kNoHeld);
        if (!more && held_mask == 0) break;
        const bool flush = defer_on && (!more || __popcll(held_mask) >= kDeferFlush);       // (wave-uniform)
        const uint32_t i = flush ? held : chunk + lane64;
        const bool active = flush ? held != kNoHeld : i < n;
        if (flush) held = kNoHeld;
        bool push_env = false, push_light = false, push_bounce = false;
        Followups fu;
        fu.q_env = fu.q_light = fu.q_bounce = false;
        uint32_t slot = 0;
        PathState ps;
        ps.beta = v3(0); ps.thr = v3(0); ps.prev_pdf = 0; ps.rc = 0; ps.bounce = 0; ps.prev_mis = false;
        // ---- 1. the prefetched hit record and slot word from LDS; everything else the entry needs, fetched in one round trip
        float4 o = make_float4(0, 0, 0, 0), d = o, h = o, bp = o, tm = o, Lq = o, pe = o, pl = o;
        uint32_t hb = kMissTri;
        const ShadePacket* packet_at = sc.shade;
        RawPacket packet;
        EnvSample es;
        es.dir = v3(0, 0, 1); es.pdf = 1; es.color = v3(0);
        const bool with_state = bounce != 0;          // (wave-uniform: `bounce` is a kernel argument)
        const uint32_t lb = lane_bytes();
        if (active) {
            h = *(const float4*)((const char*)pre_wave + lb); slot = *(const uint32_t*)((const char*)pre_slot_wave + lb / 4u);
        }
        // the next chunk's entry goes where this one's was: once that is read out, and BEFORE the gathers below -- the first use of any of
        // their results waits for every load in flight, so the LDS loads must not be the youngest
        wait_lds();
        fetch_entry(next_chunk, lb);
        if (active) {
            PT_WAIT_BEGIN()
            o = QLD(wf.ray_o[cur][base + i]); d = QLD(wf.ray_d[cur][base + i]);
            // the vertex's environment light sample, drawn by the traversal stage (env_prepass); without an environment the sample is
            // the constant the in-place code produces.  Fetched with the entry whether or not this vertex will use it: no extra round trip.
            if (env_prepass_wanted(sc, fc, bounce)) {
                const float4 ea = QLD(wf.env_a[base + i]), eb = QLD(wf.env_b[base + i]);
                es.dir = v3(ea.x, ea.y, ea.z); es.pdf = ea.w; es.color = v3(eb.x, eb.y, eb.z);
            }
            hb = __float_as_uint(h.w);
            packet_at = packet_of(sc, hb);
            packet = load_shade_packet_raw(packet_at);
            if (with_state) {
                bp = QLD(wf.q_beta[cur][base + i]); tm = QLD(wf.q_thr[cur][base + i]);
#ifndef PT_PROBE_NO_LP        // PROBE ONLY: the radiance and pending-term records are neither read nor written -- black image, same paths: what that class of state costs
                Lq = wf.L[slot]; pe = PEND_ENV(slot); pl = PEND_LIGHT(slot);
#endif
            }
            PT_WAIT_STAMP(0)
#ifdef PT_TIMING
            _wait[2]++;
#endif
        }
        // ---- 2. (dead: defer_on is false; the rejected set-aside of rare hits, kept for k_wf_shade's code generation -- see above)
        bool set_aside = false;
        if (defer_on && !flush) {
            const bool rare = false;                              // (was: the hit's material has a rare feature)
            const unsigned long long R = __ballot(rare), F = ~held_mask;
            const uint32_t nR = (uint32_t)__popcll(R), nF = (uint32_t)__popcll(F);
            if (nR != 0 && nR < kDeferMajority) {                 // (a chunk made mostly of rare hits is shaded as it is: nothing to gain)
                const unsigned long long below = (1ull << lane64) - 1ull;
                const uint32_t rr = (uint32_t)__popcll(R & below), rf = (uint32_t)__popcll(F & below);
                if (rare && rr < nF) { hand[rr] = i; set_aside = true; }       // the k-th rare lane's note goes to the k-th free lane
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (held == kNoHeld && rf < min(nR, nF)) held = hand[rf];
            }
        }
        // ---- 3. shade
        if (active && !set_aside) {
            Ray ray;
            ray.o = v3(o.x, o.y, o.z); ray.tmin = 0; ray.d = v3(d.x, d.y, d.z); ray.tmax = o.w;
            vec3 L = v3(0);
            ps.beta = v3(1); ps.prev_pdf = 0; ps.thr = v3(1); ps.rc = kRcAfterCamera; ps.bounce = 0; ps.prev_mis = false;      // a path at its first vertex
            if (with_state) {
                const uint32_t misc = __float_as_uint(tm.w);
                ps.beta = v3(bp.x, bp.y, bp.z); ps.prev_pdf = bp.w; ps.thr = v3(tm.x, tm.y, tm.z);
                ps.rc = (int)(misc & 0xffffu); ps.bounce = (int)((misc >> 16) & 0x7fffu); ps.prev_mis = (misc >> 31) != 0;
#ifndef PT_PROBE_NO_LP
                L = v3(Lq.x, Lq.y, Lq.z);
                const uint32_t pfb = __float_as_uint(Lq.w);                      // the pending bits that travel in L.w
                if ((pfb & 1u) && pe.w > 0.0f) L += v3(pe.x, pe.y, pe.z) * pe.w;
                if ((pfb & 2u) && pl.w > 0.0f) L += v3(pl.x, pl.y, pl.z) * pl.w;
#endif
            }
            uint32_t pf = 0;
            if (hb == kMissTri) L += shade_miss(sc, fc, ray.d, ps);
            else {
                HitRec hit;
                hit.t = h.x; hit.u = h.y; hit.v = h.z; hit.tri = (int)(hb & 0x7fffffffu); hit.front = (hb >> 31) != 0;
                uint32_t px, py;
                slot_pixel(fc, slot, px, py);
                n_hits++;
                const bool done = shade_closest_hit<true>(sc, fc, sample_seed(fc, slot_sample(fc, slot)), px, py, ray, hit, packet, packet_at, ps, fu, st.taps, &es, park);
                if (fu.overwrite) L = v3(0);
                L += fu.add;
                n_shadow += fu.counted_shadow;
                if (!done) {
                    push_env = fu.q_env; push_light = fu.q_light; push_bounce = fu.q_bounce;
#ifndef PT_PROBE_NO_LP
                    if (push_env) { pf |= 1u; PEND_ENV(slot) = make_float4(fu.pend_env.x, fu.pend_env.y, fu.pend_env.z, 0.0f); }
                    if (push_light) { pf |= 2u; PEND_LIGHT(slot) = make_float4(fu.pend_light.x, fu.pend_light.y, fu.pend_light.z, 0.0f); }
#endif
                }
            }
#ifndef PT_PROBE_NO_LP
            wf.L[slot] = make_float4(L.x, L.y, L.z, __uint_as_float(pf));
#endif
        }
        // ---- compaction into this shard's shadow segment and next closest-ray segment (wave-uniform control flow)
        // ONE reservation per wave-iteration: the env and light shadow rays share a counter (env entries first, then light entries: the
        // order three queue_push calls gave a wave), the bounce rays' counter is independent of it, so lane 0 adds to the one and lane 1 to
        // the other in the same atomic instruction and both bases return behind one wait -- where three queue_push calls made three dependent
        // round trips, each also waiting for the previous push's stores.  Every queue store is issued after that wait.  A lane with nothing
        // to add issues no atomic.  Lane 2 reserves the chunk after next from the shard's head in the same instruction (nothing once the
        // queue's end is in sight): the index is back, behind the same wait, a whole iteration before entry(k+2) is asked for.  That wait is
        // also the one that covers the LDS loads of this iteration's top before the next iteration reads them -- explicit, for the iterations
        // that add nothing -- and it stands where no queue store is in flight yet.
        const bool reserve_chunk = !flush && next_chunk < n;
        const unsigned long long m_env = __ballot(push_env), m_light = __ballot(push_light), m_bounce = __ballot(push_bounce);
        const uint32_t c_env = (uint32_t)__popcll(m_env), c_shadow = c_env + (uint32_t)__popcll(m_light), c_bounce = (uint32_t)__popcll(m_bounce);
#ifdef PT_PROBE_ONE_WAIT      // PROBE ONLY (step 0 of the single reservation): queue_push's three atomics, issued back to back before anything waits for one
        uint32_t r_env = 0, r_light = 0, r_bounce = 0;
        if (m_env && (int)lane64 == __ffsll((long long)m_env) - 1) r_env = atomicAdd(cnt_shadow, c_env);
        if (m_light && (int)lane64 == __ffsll((long long)m_light) - 1) r_light = atomicAdd(cnt_shadow, c_shadow - c_env);
        if (m_bounce && (int)lane64 == __ffsll((long long)m_bounce) - 1) r_bounce = atomicAdd(cnt_next, c_bounce);
        const unsigned long long below = (1ull << lane64) - 1ull;
        const uint32_t ie = (m_env ? __shfl(r_env, __ffsll((long long)m_env) - 1, 64) : 0u) + (uint32_t)__popcll(m_env & below);
        const uint32_t il = (m_light ? __shfl(r_light, __ffsll((long long)m_light) - 1, 64) : 0u) + (uint32_t)__popcll(m_light & below);
        const uint32_t ib = (m_bounce ? __shfl(r_bounce, __ffsll((long long)m_bounce) - 1, 64) : 0u) + (uint32_t)__popcll(m_bounce & below);
        uint32_t r_head = 0;
        if (reserve_chunk && lane64 == 0) r_head = atomicAdd(shade_head, 64u);
        const uint32_t chunk_after_next = reserve_chunk ? (uint32_t)__builtin_amdgcn_readfirstlane((int)r_head) : next_chunk;
#else
        uint32_t reserved = 0;
        if (lane64 < 3u) {
            const uint32_t add = lane64 == 0u ? c_shadow : (lane64 == 1u ? c_bounce : (reserve_chunk ? 64u : 0u));
            if (add != 0u) reserved = atomicAdd(lane64 == 0u ? cnt_shadow : (lane64 == 1u ? cnt_next : shade_head), add);
        }
        const uint32_t base_shadow = (uint32_t)__builtin_amdgcn_readlane((int)reserved, 0), base_bounce = (uint32_t)__builtin_amdgcn_readlane((int)reserved, 1);
        const uint32_t chunk_after_next = reserve_chunk ? (uint32_t)__builtin_amdgcn_readlane((int)reserved, 2) : next_chunk;
        const unsigned long long below = (1ull << lane64) - 1ull;
        const uint32_t ie = base_shadow + (uint32_t)__popcll(m_env & below);
        const uint32_t il = base_shadow + c_env + (uint32_t)__popcll(m_light & below);
        const uint32_t ib = base_bounce + (uint32_t)__popcll(m_bounce & below);
#endif
        wait_vector_memory();
        if (push_env) {
            QST(wf.sh_o[sbase + ie], make_float4(fu.origin_above.x, fu.origin_above.y, fu.origin_above.z, __uint_as_float(slot)));
            QST(wf.sh_d[sbase + ie], make_float4(fu.env_dir.x, fu.env_dir.y, fu.env_dir.z, __uint_as_float(kNoHint)));
            n_shadow++;
        }
        if (push_light) {
            QST(wf.sh_o[sbase + il], make_float4(fu.origin_above.x, fu.origin_above.y, fu.origin_above.z, __uint_as_float(slot | 0x80000000u)));
            QST(wf.sh_d[sbase + il], make_float4(fu.light_dir.x, fu.light_dir.y, fu.light_dir.z, __uint_as_float(kNoHint)));
            n_shadow++;
        }
        if (push_bounce) {                                                                           // TraceBounceRay :669-678
            QST(wf.ray_o[nxt][base + ib], make_float4(fu.b_o.x, fu.b_o.y, fu.b_o.z, fc.max_ray_length));
            QST(wf.ray_d[nxt][base + ib], make_float4(fu.b_d.x, fu.b_d.y, fu.b_d.z, __uint_as_float(slot)));
            const uint32_t misc = ((uint32_t)ps.rc & 0xffffu) | ((uint32_t)(ps.bounce + 1) << 16) | (fu.b_mis ? 0x80000000u : 0u);
            QST(wf.q_beta[nxt][base + ib], make_float4(fu.b_beta.x, fu.b_beta.y, fu.b_beta.z, fu.b_pdf));
            QST(wf.q_thr[nxt][base + ib], make_float4(fu.b_thr.x, fu.b_thr.y, fu.b_thr.z, __uint_as_float(misc)));
            n_bounce++;
        }
        if (!flush) { chunk = next_chunk; next_chunk = chunk_after_next; }
    }
    flush_shard_tallies(shard_tallies(wf, sv.shard), threadIdx.x & 63, 0, n_bounce, n_shadow, n_hits, st.taps);
#ifdef PT_TIMING
    if (lane64 == 0) { for (int k = 0; k < 3; k++) atomicAdd(&pt_timing[8 + k], _wait[k]); }
#endif
}

// occlusion traversal of the shadow queue (TraceShadowRay :724-742); writes the transmission next to its pending term.
template <bool COUNT>
__global__ __launch_bounds__(kBlock, PT_TRACE_WAVES) void k_wf_shadow(SceneRec sc, WfBuffers wf, int bounce, uint32_t flags, float tmax, Counters* __restrict__ counters) {
    __shared__ int s_stack[kStackLds * kBlock];
    stage_luts(sc);
    const ShardView sv = shard_view(wf);
    LaneStats st = {0, 0, 0, 0};
    trace_persistent<COUNT, 1>(sc, wf, s_stack + threadIdx.x, sv, shadow_counter(bounce), 0, 0xff, flags, st, tmax);
    if (COUNT) { flush_counters(counters, threadIdx.x & 63, 0, 0, 0, 0, st, true); if (st.deep) atomicAdd(&counters->deep_pushes, (unsigned long long)st.deep); }
    else if (st.overflow | st.deep) flush_rare(counters, st);
}

// Adaptive sampling: the per-pixel error of the accumulated image I against the half buffer A (the mean of the samples with an even
// per-tile index), in float32 in this order with IEEE division and a correctly rounded square root; a NaN counts as +inf.
PT_DEV float adaptive_pixel_error(const float4 I, const float4 A) {
    const float d = (fabsf(I.x - A.x) + fabsf(I.y - A.y)) + fabsf(I.z - A.z);
    const float s = (I.x + I.y) + I.z;
    const float e = d / (1e-4f + sqrtf(fmaxf(s, 0.0f)));
    return e != e ? INFINITY : e;
}
// The adaptive resolve of one tile (one block): blend the batch into I and, on even per-tile indices, into A; the tile's error E is the
// max of its pixels' errors (wave64 max by cross-lane swaps, then the four waves through LDS), and one lane writes the tile's count, E and
// whether it retires.  A retired tile's block leaves at once: its output and half-buffer pixels are not written.  Active tiles all hold
// fc.accumulated_frames samples, so a tile's image is, bit for bit, the uniform accumulation after its own count.
template <bool AOV>
PT_DEV void resolve_adaptive(const FrameConstants& fc, const WfBuffers& wf, float4* __restrict__ output, const AdaptiveArgs& ad, const AovArgs& av) {
    const uint32_t tile = blockIdx.x;                                 // rank-local tile: the resolve grid is one block per tile
    if (ad.tiles[tile].active == 0) return;                           // (block-uniform)
    const uint32_t pslot = tile * kBlock + threadIdx.x;
    uint32_t px = 0, py = 0;
    const bool in_image = pslot < fc.pixel_slots && slot_pixel(fc, pslot, px, py);
    float e = -INFINITY;
    if (in_image) {
        const size_t at = (size_t)py * fc.res_x + px;
        float4 pixel = make_float4(0, 0, 0, 0), half = pixel;
        if (fc.accumulated_frames != 0) { pixel = output[at]; half = ad.half[at]; }
        for (uint32_t k = 0; k < fc.spp; k++) {
            const vec3 L = resolved_sample(fc, wf, k * fc.pixel_slots + pslot);
            const int n = fc.accumulated_frames + (int)k;             // the sample's per-tile index
            pixel = n != 0 ? blend_sample(pixel, n, L) : make_float4(L.x, L.y, L.z, 1.0f);
            if ((n & 1) == 0) half = n != 0 ? blend_sample(half, n >> 1, L) : make_float4(L.x, L.y, L.z, 1.0f);
        }
        output[at] = pixel;
        ad.half[at] = half;
        e = adaptive_pixel_error(pixel, half);
        if (AOV) resolve_aov(fc, wf, av, pslot, at, fc.accumulated_frames);       // (an adaptive call accumulates)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e = fmaxf(e, __shfl_xor(e, off, 64));
    __shared__ float s_err[kBlock / 64];
    if ((threadIdx.x & 63u) == 0) s_err[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        float E = s_err[0];
#pragma unroll
        for (uint32_t w = 1; w < kBlock / 64; w++) E = fmaxf(E, s_err[w]);
        const int n = fc.accumulated_frames + (int)fc.spp;
        const bool retire = n >= ad.cap || (n >= ad.min_samples && E <= ad.threshold);
        AdaptiveTile t;
        t.active = retire ? 0u : 1u; t.samples = (uint32_t)n; t.error = E; t.pad = 0;
        ad.tiles[tile] = t;
    }
}

// AOV: the instantiations of calls with AOV targets (pt_set_aov) also blend the records k_wf_aov wrote, next to the beauty pixel; the
// others take `av` and never look at it.  Being the launch that ends every trace, it also folds the stages' per-shard ray tallies into
// `counters` (fold_shard_tallies): one wave of workgroup 0, whatever becomes of that workgroup's tile.
template <bool ADAPTIVE, bool AOV>
__global__ __launch_bounds__(kBlock) void k_wf_resolve(FrameConstants fc, WfBuffers wf, float4* __restrict__ output, AdaptiveArgs ad, AovArgs av, Counters* __restrict__ counters) {
    fold_shard_tallies(wf, counters);       // the trace's ray counts (before any thread leaves: a retired tile's block, a slot off the image)
    if (ADAPTIVE) { resolve_adaptive<AOV>(fc, wf, output, ad, av); return; }
    const uint32_t pslot = blockIdx.x * kBlock + threadIdx.x;       // pixel slot; its samples sit pixel_slots apart
    uint32_t px, py;
    if (pslot >= fc.pixel_slots || !slot_pixel(fc, pslot, px, py)) return;
    // the samples of a batch are blended in sample order, exactly as consecutive PathtraceScene calls would (running mean); the
    // pixel stays in registers between them: one read and one write of the image however many samples the batch has
    float4* outp = output + ((size_t)py * fc.res_x + px);
    const bool accumulate = (fc.flags & PT_FLAG_ACCUMULATE) != 0;
    float4 pixel = make_float4(0, 0, 0, 0);
    if (accumulate && fc.accumulated_frames != 0) pixel = *outp;
    for (uint32_t k = 0; k < fc.spp; k++) {
        const vec3 L = resolved_sample(fc, wf, k * fc.pixel_slots + pslot);
        const int accumulated = fc.accumulated_frames + (int)k;
        pixel = (accumulate && accumulated != 0) ? blend_sample(pixel, accumulated, L) : make_float4(L.x, L.y, L.z, 1.0f);
    }
    *outp = pixel;
    if (AOV) resolve_aov(fc, wf, av, pslot, (size_t)py * fc.res_x + px, accumulate ? fc.accumulated_frames : -1);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// The workspace's layout is pt_workspace.h's, for the call's tiles, samples, stage workgroups and record arrays.
size_t wavefront_workspace_bytes(const FrameConstants& fc, int stage_blocks, const WavefrontPasses& passes) {
    return workspace_layout(fc.my_tiles, fc.spp, stage_blocks, passes.records(), kBlock).total;
}

static WfBuffers carve(void* workspace, const WorkspaceLayout& l, uint32_t slots) {
    auto at = [&](size_t offset) { return (float4*)((char*)workspace + offset); };
    WfBuffers wf;
    wf.chunks_per_shard = l.chunks_per_shard; wf.blocks_per_shard = l.blocks_per_shard; wf.seg_cap = l.seg_cap;
    wf.gen_region_tiles = 0; wf.gen_rounds = l.gen_rounds;
    for (int k = 0; k < kCounterArrays; k++) wf.cnt[k] = (uint32_t*)at(l.cnt[k]);
    wf.L = at(l.L); wf.beta_pdf = at(l.beta_pdf); wf.thr_misc = at(l.thr_misc); wf.pend = at(l.pend);
    for (int k = 0; k < 2; k++) { wf.ray_o[k] = at(l.ray_o[k]); wf.ray_d[k] = at(l.ray_d[k]); wf.q_beta[k] = at(l.q_beta[k]); wf.q_thr[k] = at(l.q_thr[k]); }
    wf.hit = at(l.hit); wf.env_a = at(l.env_a); wf.env_b = at(l.env_b); wf.sh_o = at(l.sh_o); wf.sh_d = at(l.sh_d);
    wf.sh_c = nullptr; wf.occ_cache = nullptr; wf.capacity = slots;
    return wf;
}

int traversal_stack_capacity() { return kStackLds + kStackSpill; }
size_t traversal_grid_lanes(int stage_blocks) { return (size_t)kShards * blocks_per_shard_for(stage_blocks) * kBlock; }

// ---- the traversal stages' kernel copies and launches (pt_wavefront.h: declared there, with the ray flags, for the test hook too)
// the traversal kernels compiled for rays with no flags, if that is what the frame's settings give them
static bool traversal_defaults(uint32_t flags) { return (flags & kTravFlagMask) == 0; }
void launch_wf_trace(dim3 grid, hipStream_t stream, bool count, const SceneRec& sc, const FrameConstants& fc, const WfBuffers& w, int cur, int b, uint32_t rf,
                     uint32_t rmask, Counters* counters) {
    pick2(count, traversal_defaults(fc.flags), [&](auto COUNT, auto DEFAULTS) { hipLaunchKernelGGL((k_wf_trace<COUNT.value, DEFAULTS.value>), grid, dim3(kBlock), 0, stream, sc, fc, w, cur, b, rf, rmask, counters); });
}
void launch_wf_traverse(dim3 grid, hipStream_t stream, bool count, const SceneRec& sc, const FrameConstants& fc, const WfBuffers& w, int nxt, int b, uint32_t rf,
                        uint32_t rmask, Counters* counters) {
    pick2(count, traversal_defaults(fc.flags), [&](auto COUNT, auto DEFAULTS) { hipLaunchKernelGGL((k_wf_traverse<COUNT.value, DEFAULTS.value>), grid, dim3(kBlock), 0, stream, sc, fc, w, nxt, b, rf, rmask, fc.flags, counters); });
}
void launch_wf_shadow(dim3 grid, hipStream_t stream, bool count, const SceneRec& sc, const WfBuffers& w, int b, uint32_t flags, float tmax, Counters* counters) {
    pick(count, [&](auto COUNT) { hipLaunchKernelGGL(k_wf_shadow<COUNT.value>, grid, dim3(kBlock), 0, stream, sc, w, b, flags, tmax, counters); });
}

// pt_enable_stage_timing: an event after every launch, so that the time of a launch can be split by stage (diagnostic: the
// events cost a few microseconds each)
hipEvent_t StageTimers::event_at(size_t i) {
    while (ev.size() <= i) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; ev.push_back(e); }
    return ev[i];
}
void StageTimers::mark(int stage_kind, hipStream_t stream) {
    const size_t k = used;
    hipEvent_t e = event_at(k + 1);
    if (!e) return;
    if (kind.size() < k + 1) kind.resize(k + 1);
    kind[k] = (uint8_t)stage_kind;
    hipEventRecord(e, stream);
    used = k + 1;
}

hipError_t launch_wavefront(const SceneRec& sc, const FrameConstants& fc, const LensArgs& lens, float4* output, Counters* counters, bool count, void* workspace,
                            int stage_blocks, StageTimers* timers, hipStream_t stream, const WavefrontPasses& passes) {
    if (timers) timers->used = 0;
    if (fc.my_tiles == 0) return hipSuccess;
    const uint32_t slots = fc.my_tiles * kBlock * fc.spp;
    const WorkspaceLayout lay = workspace_layout(fc.my_tiles, fc.spp, stage_blocks, passes.records(), kBlock);
    WfBuffers wf = carve(workspace, lay, slots);
    hipError_t e = hipMemsetAsync(wf.cnt[0], 0, (size_t)kCounterArrays * kShards * kCounterStride * 4, stream);     // the counter arrays are contiguous
    if (e) return e;
    const dim3 block(kBlock), full(fc.my_tiles), stage(kShards * wf.blocks_per_shard);
    if (timers) { hipEvent_t ev = timers->event_at(0); if (ev) hipEventRecord(ev, stream); else timers = nullptr; }
    PassArgs pass = {passes, stream, timers};                           // the optional passes (wf_passes.hip): their argument blocks, their records cleared
    if ((e = passes_begin(pass, workspace, lay, slots)) != hipSuccess) return e;
    if (passes.probes || passes.bake) launch_pass_generate(pass, stage, fc, wf, counters);
    else pick2(passes.adaptive, lens.enable != 0, [&](auto ADAPTIVE, auto LENS) { hipLaunchKernelGGL((k_wf_generate<ADAPTIVE.value, LENS.value>), stage, block, 0, stream, fc, wf, counters, pass.ad, lens); });
    mark_stage(timers, STAGE_GENERATE, stream);
    const uint32_t flags = fc.flags;
    const int iterations = fc.debug_output != PT_DEBUG_OUTPUT_NONE ? 1 : fc.max_bounces + 1;
    // the shade kernel compiled for this frame's flags, if there is one (k_wf_shade)
    const uint32_t shade_bits = flags & kShadeFlagMask;
    const int shade_variant = fc.debug_output != PT_DEBUG_OUTPUT_NONE ? 0 : (shade_bits == kShadeDefaults ? 1 : (shade_bits == kShadeDefaultsNoLights ? 2 : 0));
    const bool small_tables = sc.n_instances <= kInstCacheMax && sc.n_materials <= kMatCacheMax && fc.num_of_lights <= kLightCacheMax;
    auto launch_shade = [&](dim3 grid, const WfBuffers& w, int cur, int b) {
        if (small_tables && shade_variant == 1) hipLaunchKernelGGL((k_wf_shade<kShadeSpecialised | kShadeDefaults, true>), grid, block, 0, stream, sc, fc, w, cur, b, counters);
        else if (small_tables && shade_variant == 2) hipLaunchKernelGGL((k_wf_shade<kShadeSpecialised | kShadeDefaultsNoLights, true>), grid, block, 0, stream, sc, fc, w, cur, b, counters);
        else if (small_tables) hipLaunchKernelGGL((k_wf_shade<0u, true>), grid, block, 0, stream, sc, fc, w, cur, b, counters);
        else hipLaunchKernelGGL((k_wf_shade<0u, false>), grid, block, 0, stream, sc, fc, w, cur, b, counters);
    };
    // Late bounces carry few paths (Russian roulette starts after min_bounces and the reference's throughput drives the continuation
    // probability to its floor): a launch sized for the full queue then mostly starts workgroups that find nothing and, in the shade
    // stage, would stage 67 KB of tables for it.  The grid of a bounce follows the EXPECTED queue (a quarter of the paths per bounce
    // beyond min_bounces + 1); only speed depends on the guess -- any multiple of kShards workgroups walks the whole queue.
    // tuning aid (tools/overlap_probe.py): MIPT_SHADE_BPS / MIPT_TRACE_BPS = workgroups per shard of the shade / traversal launches
    static const int env_shade_bps = getenv("MIPT_SHADE_BPS") ? atoi(getenv("MIPT_SHADE_BPS")) : 0;
    static const int env_trace_bps = getenv("MIPT_TRACE_BPS") ? atoi(getenv("MIPT_TRACE_BPS")) : 0;
    auto grid_of = [&](int b) -> dim3 {
        uint32_t bps = wf.blocks_per_shard;
        if (b > fc.min_bounces + 1) {
            double expected = (double)slots;
            for (int k = fc.min_bounces + 1; k < b; k++) expected *= 0.25;
            const uint32_t want = expected >= 1200000.0 ? 6u : (expected >= 400000.0 ? 3u : 2u);
            bps = want < bps ? want : bps;
        }
        return dim3(kShards * bps);
    };
    auto cap = [&](dim3 g, int env) { if (env > 0 && (uint32_t)env * kShards < g.x) g.x = (uint32_t)env * kShards; return g; };
    auto wf_of = [&](dim3 g) { WfBuffers w = wf; w.blocks_per_shard = g.x / kShards; return w; };
    // generate -> trace(0) -> [shade(b) -> shadow(b) + trace(b + 1)] x (bounces) -> resolve: two grid-wide synchronisations per bounce
    {
        uint32_t rf, rmask;
        traversal_ray_flags(flags, 0, rf, rmask);
        const dim3 g0 = cap(stage, env_trace_bps);
        launch_wf_trace(g0, stream, count, sc, fc, wf_of(g0), 0, 0, rf, rmask, counters);
        mark_stage(timers, STAGE_TRACE, stream);
    }
    launch_first_hit_passes(pass, stage, sc, fc, wf);     // the primary hits, before shade(0) + traverse(0) reuse the arrays
    for (int b = 0; b < iterations; b++) {
        const int cur = b & 1;
        const dim3 gs = cap(grid_of(b), env_shade_bps), gt = cap(grid_of(b), env_trace_bps);
        const WfBuffers ws = wf_of(gs), wt = wf_of(gt);
        launch_shade(gs, ws, cur, b);
        mark_stage(timers, STAGE_SHADE, stream);
        uint32_t rf, rmask;
        traversal_ray_flags(flags, b + 1, rf, rmask);
        if (b + 1 < iterations) launch_wf_traverse(gt, stream, count, sc, fc, wt, cur ^ 1, b, rf, rmask, counters);
        else launch_wf_shadow(gt, stream, count, sc, wt, b, flags, fc.max_ray_length, counters);         // the last vertex pushes no bounce ray
        mark_stage(timers, STAGE_SHADOW, stream);
    }
    launch_pass_resolves(pass, full, fc, wf, output);     // before the resolve retires tiles and replaces the output's means
    pick2(passes.adaptive, passes.aov, [&](auto ADAPTIVE, auto AOV) { hipLaunchKernelGGL((k_wf_resolve<ADAPTIVE.value, AOV.value>), full, block, 0, stream, fc, wf, output, pass.ad, pass.av, counters); });
    mark_stage(timers, STAGE_RESOLVE, stream);
    return hipGetLastError();
}

}  // namespace pt
