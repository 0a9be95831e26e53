// pt_wavefront.h -- what the wavefront stages (pt_wavefront.hip, wf_passes.hip) share with their test hooks (debug_wf.hip): the kernels' buffer
// record, the queue formats' constants and the traversal stages' ray flags and launches, so that the hook launches what a frame launches; and
// the host functions of the optional passes that launch_wavefront calls.  No device code: the stage kernels' own vocabulary is pt_wf_stage.h.
#pragma once
#include "pt_traverse.h"
#include "pt_host.h"

namespace pt {

// (kShards, kXcds, kCounterStride and kCounterArrays: pt_workspace.h, with the layout they size)
constexpr uint32_t kMissTri = 0x7fffffffu;
constexpr uint32_t kNoHint = 0xffffffffu;

struct WfBuffers {
    // per slot (one path per pixel of this rank)
    float4* L;            // xyz radiance so far; w = bits: bit 0 env term pending, bit 1 light term pending
    float4* beta_pdf;     // unused (beta and throughput travel in q_beta / q_thr): no kernel reads or writes these two; they keep the
    float4* thr_misc;     // kernel-argument layout
    float4* pend;         // [2 * slot] xyz pending env-NEE term (beta-weighted), w = its shadow transmission (written by the shadow stage);
                          // [2 * slot + 1] the same for the punctual-light term: one 32-B piece per path
    // closest-ray queues (ping-pong), kShards segments of seg_cap entries: (o.xyz, tmax), (d.xyz, slot)
    float4* ray_o[2];
    float4* ray_d[2];
    float4* q_beta[2];    // the path's (beta, prev_pdf) and (throughput, misc bits) travel with its closest-ray entry -- written
    float4* q_thr[2];     // compacted, read coalesced -- instead of living in slot-indexed arrays
    float4* hit;          // per entry of the current queue: t, u, v, bits: tri | front << 31 (kMissTri: miss)
    float4* env_a;        // per entry of the current closest queue: the vertex's environment light sample, drawn by the traversal stage that
    float4* env_b;        // traces the entry (env_prepass): (direction, pdf), (radiance, -)
    // shadow queue, kShards segments of 2 * seg_cap entries: (o.xyz, bits: slot | is_light << 31), (d.xyz, tmax)
    float4* sh_o;
    float4* sh_d;         // (d.xyz, kNoHint; the rays' tmax is the constant max_ray_length)
    uint32_t* sh_c;       // unused, nullptr (kernel-argument layout)
    uint32_t* occ_cache;  // unused, nullptr (kernel-argument layout)
    uint32_t* cnt[7];     // per shard (stride kCounterStride): entry counts of closest queue 0, closest queue 1, shadow queue (even bounces);
                          // [3], [4]: dynamic-fetch heads of the closest / shadow trace stages; [5]: shadow-queue count of odd bounces
                          // (the shadow count ping-pongs so that the fused traversal stage can zero the one the NEXT shade stage fills
                          // while it still reads the current one); [6]: dynamic-fetch head of the shade stage.  Only word 0 of a shard's
                          // line is the counter; words 2 .. 11 of the [3] line hold the generate and shade stages' ray tallies (shard_tallies)
    uint32_t capacity;    // slots
    uint32_t chunks_per_shard;   // path-state arrays: 256-slot chunks per shard (unused by the kernels)
    uint32_t seg_cap;     // entries per closest-queue segment
    uint32_t blocks_per_shard;
    uint32_t gen_region_tiles, gen_rounds;     // k_wf_generate: (unused, 0), workgroup-rounds to cover the (tile, sample) pairs
};

// index into WfBuffers::cnt of the shadow queue's counter at that bounce
PT_HD int shadow_counter(int bounce) { return (bounce & 1) ? 5 : 2; }

// ---- the traversal stages' ray flags and launches: ONE statement of each, called by launch_wavefront and by the test hook debug_trace_queues
// (debug_wf.hip).  The launch functions and the kernel copies they choose among are pt_wavefront.hip's.
// Ray flags and instance mask of the closest-hit rays of bounce b.
inline void traversal_ray_flags(uint32_t flags, int b, uint32_t& rf, uint32_t& rmask) {
    rmask = 0xff;
    if (b == 0) rf = (flags & PT_FLAG_CULL_BACKFACE) ? RF_CULL_BACK : 0;                              // RayGeneration :747
    else {                                                                                            // TraceBounceRay :671-672
        rf = (flags & PT_FLAG_CULL_BACKFACE) ? RF_CULL_FRONT : 0;
        rmask = (flags & PT_FLAG_INDIRECT_ENVIRONMENT_ONLY) ? 0 : 0xff;
    }
}
void launch_wf_trace(dim3 grid, hipStream_t stream, bool count, const SceneRec& sc, const FrameConstants& fc, const WfBuffers& w, int cur, int b, uint32_t rf,
                     uint32_t rmask, Counters* counters);
void launch_wf_traverse(dim3 grid, hipStream_t stream, bool count, const SceneRec& sc, const FrameConstants& fc, const WfBuffers& w, int nxt, int b, uint32_t rf,
                        uint32_t rmask, Counters* counters);
void launch_wf_shadow(dim3 grid, hipStream_t stream, bool count, const SceneRec& sc, const WfBuffers& w, int b, uint32_t flags, float tmax, Counters* counters);

// ---- the optional passes (wf_passes.hip), in the order launch_wavefront calls them.  PassArgs: the call's passes, stream and timers, and the
// argument blocks as the kernels take them (passes_begin: zeros for a pass that is off, the record pointers from the layout, the records cleared).
struct PassArgs { const WavefrontPasses& on; hipStream_t stream; StageTimers* timers; AdaptiveArgs ad; AovArgs av; MatteArgs mt; MotionArgs mo; };
hipError_t passes_begin(PassArgs& a, void* workspace, const WorkspaceLayout& lay, uint32_t slots);
void launch_pass_generate(const PassArgs& a, dim3 stage, const FrameConstants& fc, const WfBuffers& wf, Counters* counters);     // a bake's or a probe atlas's
void launch_first_hit_passes(const PassArgs& a, dim3 stage, const SceneRec& sc, const FrameConstants& fc, const WfBuffers& wf);  // AOV, matte, motion
void launch_pass_resolves(const PassArgs& a, dim3 full, const FrameConstants& fc, const WfBuffers& wf, const float4* output);    // matte, motion, variance

}  // namespace pt
