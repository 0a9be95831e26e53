// pt_wf_stage.h -- the device-side vocabulary of the wavefront stages, shared by the hot path (pt_wavefront.hip) and the optional passes
// (wf_passes.hip): queue access, shard views and tallies, the adaptive tile test, the pending terms, the AOV blend, and the bodies more
// than one stage kernel runs (the resolved sample, a pass resolve's pixel, the first-hit walk, the generate body of a ray that may be
// absent).  The split: pt_wavefront.h is what the test hooks of debug_wf.hip see too -- WfBuffers, the constants, the traversal launches --
// and holds no device code; this header is for the two files that define stage kernels, and is compiled with their flags only.
#pragma once
#include <type_traits>

#include "pt_vertex.h"
#include "pt_wavefront.h"
#include "pt_workspace.h"

namespace pt {

// (WfBuffers, kMissTri, kNoHint and shadow_counter: pt_wavefront.h, shared with the test hooks of debug_wf.hip)
// Queue entries are written once and read once, a stage apart, by then long evicted from the 4-MiB L2s: they are moved with the
// non-temporal hint (QLD / QST) so that they do not push the tree's nodes and triangle packets out on their way through.  The per-path
// state records are accessed plainly.
typedef float nt_v4f __attribute__((ext_vector_type(4)));
PT_DEV float4 nt_load(const float4& p) { const nt_v4f v = __builtin_nontemporal_load((const nt_v4f*)&p); return make_float4(v.x, v.y, v.z, v.w); }
PT_DEV uint32_t nt_load(const uint32_t& p) { return __builtin_nontemporal_load(&p); }
PT_DEV void nt_store(float4& p, const float4 v) { nt_v4f q; q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w; __builtin_nontemporal_store(q, (nt_v4f*)&p); }
PT_DEV void nt_store(uint32_t& p, const uint32_t v) { __builtin_nontemporal_store(v, &p); }
#define QLD(p) nt_load(p)
#define QST(p, v) nt_store((p), (v))

#define PEND_ENV(s) wf.pend[2u * (s)]
#define PEND_LIGHT(s) wf.pend[2u * (s) + 1u]

// wave64 ballot compaction into a shard counter: lanes with `pred` get consecutive indices; one atomic per wave.
PT_DEV uint32_t queue_push(uint32_t* counter, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m == 0) return 0;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
    uint32_t base = 0;
    const int leader = __ffsll((long long)m) - 1;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    return base + rank;
}

// Every stage launch has the same grid: kShards * blocks_per_shard workgroups.  Workgroup b: shard b % kShards, member b / kShards.
struct ShardView { uint32_t shard, member, stride; };
PT_DEV ShardView shard_view(const WfBuffers& wf) {
    ShardView v;
    v.shard = blockIdx.x % kShards;
    v.member = blockIdx.x / kShards;
    v.stride = wf.blocks_per_shard * kBlock;
    return v;
}
// Where the generate and shade stages count (flush_shard_tallies, pt_vertex.h): the spare words of the shard's line of cnt[3], the closest
// trace stage's fetch head.  That line is quiet while either stage runs -- nothing fetches from it, the shade stage's member 0 only stores
// word 0 -- so a launch puts ~32 atomics on each of 256 lines where it used to put ~8 000 on the one line of Counters.  launch_wavefront's
// memset clears the words with the counters; k_wf_resolve, the last launch of every trace, folds them into Counters.  (The generate and
// shade kernels keep their `counters` argument, now unread: the kernel-argument layout stays what it was.)
static_assert((kTallyPrimary + kTallies) * 8 <= (int)kCounterStride * 4, "the tallies must fit the shard counter's line behind its word 0");
PT_DEV unsigned long long* shard_tallies(const WfBuffers& wf, uint32_t shard) { return (unsigned long long*)(wf.cnt[3] + shard * kCounterStride); }

// Adaptive sampling (pt_set_adaptive): is the tile of a workgroup-round's (tile, sample) pair still active?  `slot0` = the round's first
// slot (workgroup-uniform), so the state is read once per round; a retired tile pushes no ray and every later stage is unchanged.
PT_DEV bool adaptive_tile_active(const FrameConstants& fc, const AdaptiveArgs& ad, uint32_t slot0) {
    const uint32_t pair = slot0 >> 8;                                 // sample * my_tiles + rank-local tile
    if (pair >= fc.my_tiles * fc.spp) return false;
    const uint32_t local_tile = pair - slot_sample(fc, slot0) * fc.my_tiles;
    return ad.tiles[local_tile].active != 0;
}

// The generate stage of a ray that may be absent (an uncovered bake texel, a cell without a probe): `ray_of(seed, px, py, rc, ray)` says
// whether the (pixel, sample) has one.  A slot without a ray pushes none and counts none: no later stage would write it, so its records are
// written here -- radiance 0 with nothing pending and, with AOVs on, zero records (`av` as k_wf_aov takes it, all null without AOVs) -- and
// the unchanged resolve blends a defined value.  k_wf_generate (pt_wavefront.hip) is the hand-written third instance of this loop, with
// camera_ray and no absent branch: the benchmark measures it, and through this body none of its four copies kept its assembly.
template <bool ADAPTIVE, class RayOf>
PT_DEV void generate_sparse(const FrameConstants& fc, const WfBuffers& wf, const AdaptiveArgs& ad, const AovArgs& av, RayOf&& ray_of) {
    const ShardView sv = shard_view(wf);
    unsigned n_primary = 0;
    for (uint32_t rnd = 0; rnd < wf.gen_rounds; rnd++) {
        const uint32_t slot = (rnd * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        const uint32_t sample = slot_sample(fc, slot);
        uint32_t px = 0, py = 0;
        bool valid = slot < wf.capacity && slot_pixel(fc, slot, px, py);
        if (ADAPTIVE) { const bool tile_on = adaptive_tile_active(fc, ad, (rnd * gridDim.x + blockIdx.x) * kBlock); valid = valid && tile_on; }
        int rc = 0;
        Ray ray;
        ray.o = v3(0); ray.d = v3(0, 0, 1); ray.tmin = 0; ray.tmax = 0;
        bool present = false;
        if (valid) present = ray_of(sample_seed(fc, sample), px, py, rc, ray);
        const uint32_t idx = queue_push(wf.cnt[0] + sv.shard * kCounterStride, present);
        if (present) {
            const size_t e = (size_t)sv.shard * wf.seg_cap + idx;
            QST(wf.ray_o[0][e], make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tmax));
            QST(wf.ray_d[0][e], make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(slot)));
            n_primary++;
        } else if (valid) {
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            wf.L[slot] = zero;
            if (av.albedo) QST(av.rec_albedo[slot], zero);
            if (av.normal_depth) QST(av.rec_normal[slot], zero);
        }
    }
    flush_shard_tallies(shard_tallies(wf, sv.shard), threadIdx.x & 63, n_primary, 0, 0, 0, 0);
}

// The walk of the first-hit stages (k_wf_aov, k_wf_matte, k_wf_motion) over their workgroup's share of queue 0's shard segment, in the
// window between the primary traversal and the first shade stage, where the queue's rays and wf.hit are intact.  f(i): entry i of the
// segment, at index base + i of wf.ray_o[0] / wf.ray_d[0] / wf.hit.  The entry's slot is word 3 of its ray_d, its hit word (tri | front << 31,
// kMissTri) word 3 of its hit record: slot / hit_word load that one word, for a stage that does not read the whole record.
struct FirstHits {
    uint32_t n, first, stride;          // entries of the segment; the workgroup's first; the launch's stride
    size_t base;
    PT_DEV bool none() const { return first >= n; }                     // (workgroup-uniform) nothing of the segment is this workgroup's
    template <class F> PT_DEV void each(F&& f) const { for (uint32_t i = first + threadIdx.x; i < n; i += stride) f(i); }
    PT_DEV uint32_t slot(const WfBuffers& wf, uint32_t i) const { return QLD(((const uint32_t*)(wf.ray_d[0] + base + i))[3]); }
    PT_DEV uint32_t hit_word(const WfBuffers& wf, uint32_t i) const { return QLD(((const uint32_t*)(wf.hit + base + i))[3]); }
};
PT_DEV FirstHits first_hits(const WfBuffers& wf) {
    const ShardView sv = shard_view(wf);
    return {wf.cnt[0][sv.shard * kCounterStride], sv.member * kBlock, sv.stride, (size_t)sv.shard * wf.seg_cap};
}

// The reference multiplies the light colour by the shadow transmission BEFORE `if (any(color > 0))` and never evaluates
// the BSDF of an occluded sample: an occluded sample contributes nothing even when its pending term is NaN.
// Both pending records are fetched whatever the flags say (the slots always exist): three loads in one round trip instead of
// the flags first and the records behind them.
// `pf` = the pending bits that travel in L.w.
PT_DEV void apply_pending(const WfBuffers& wf, uint32_t slot, uint32_t pf, vec3& L) {
    const float4 pe = PEND_ENV(slot), pl = PEND_LIGHT(slot);
    if ((pf & 1u) && pe.w > 0.0f) L += v3(pe.x, pe.y, pe.z) * pe.w;
    if ((pf & 2u) && pl.w > 0.0f) L += v3(pl.x, pl.y, pl.z) * pl.w;
}
// A finished path's sample as the output blends it: the slot's radiance, its pending terms, the clamp.  ONE statement for k_wf_resolve,
// resolve_adaptive and k_wf_variance_resolve, whose x must be the resolve's value bit for bit.
PT_DEV vec3 resolved_sample(const FrameConstants& fc, const WfBuffers& wf, uint32_t slot) {
    const float4 Lq = wf.L[slot];
    vec3 L = v3(Lq.x, Lq.y, Lq.z);
    apply_pending(wf, slot, __float_as_uint(Lq.w), L);
    return sanitize_sample(fc, L);
}
// A pass resolve's thread on the resolve's grid (one block per rank-local tile, one thread per pixel slot): f(pslot, at, first) with its
// pixel slot, the pixel's index and `first` = samples already in the target, < 0: the call does not accumulate.  f is not called, and the
// thread writes nothing, where the tile is retired by adaptive sampling or the slot is off the image.
template <bool ADAPTIVE, class F>
PT_DEV void resolve_pixel(const FrameConstants& fc, const AdaptiveArgs& ad, F&& f) {
    if (ADAPTIVE) { if (ad.tiles[blockIdx.x].active == 0) return; }     // (block-uniform)
    const uint32_t pslot = blockIdx.x * kBlock + threadIdx.x;
    uint32_t px, py;
    if (pslot >= fc.pixel_slots || !slot_pixel(fc, pslot, px, py)) return;
    const bool accumulate = ADAPTIVE || (fc.flags & PT_FLAG_ACCUMULATE) != 0;     // (an adaptive call accumulates)
    f(pslot, (size_t)py * fc.res_x + px, accumulate ? fc.accumulated_frames : -1);
}

// the running mean of a four-component AOV record: blend_sample's weight on every component
PT_DEV float4 blend_aov(float4 h, int accumulated, float4 v) {
    const float blend = fdiv(1.0f, (float)accumulated + 1.0f);
    return make_float4(h.x + blend * (v.x - h.x), h.y + blend * (v.y - h.y), h.z + blend * (v.z - h.z), h.w + blend * (v.w - h.w));
}
// The AOV part of a resolve thread: the batch's records of pixel slot `pslot` blended in sample order into one target, with the
// beauty's counts (`first` = samples already in the target; < 0: the call does not accumulate and the target takes the one sample).
PT_DEV void resolve_aov_target(const FrameConstants& fc, const WfBuffers& wf, const float4* __restrict__ rec, float4* __restrict__ target, uint32_t pslot, size_t at, int first) {
    float4 pixel = make_float4(0, 0, 0, 0);
    if (first > 0) pixel = target[at];
    for (uint32_t k = 0; k < fc.spp; k++) {
        const float4 v = QLD(rec[k * fc.pixel_slots + pslot]);
        const int n = first + (int)k;
        pixel = n > 0 ? blend_aov(pixel, n, v) : v;
    }
    target[at] = pixel;
}
PT_DEV void resolve_aov(const FrameConstants& fc, const WfBuffers& wf, const AovArgs& av, uint32_t pslot, size_t at, int first) {
    if (av.albedo) resolve_aov_target(fc, wf, av.rec_albedo, av.albedo, pslot, at, first);
    if (av.normal_depth) resolve_aov_target(fc, wf, av.rec_normal, av.normal_depth, pslot, at, first);
}

// A run-time bool as a compile-time one (host): f(std::true_type()) or f(std::false_type()), so that a launch line is written once for both
// kernel copies.  pick2: two of them.
template <class F> static void pick(bool a, F&& f) { if (a) f(std::true_type()); else f(std::false_type()); }
template <class F> static void pick2(bool a, bool b, F&& f) { pick(a, [&](auto A) { pick(b, [&](auto B) { f(A, B); }); }); }

}  // namespace pt
