// pt_workspace.h -- the layout of a wavefront trace's workspace, stated once and on the host alone: plain integers in, byte offsets out.
// pt_wavefront.hip hands the arrays out by it (carve, launch_wavefront; the passes' records: wf_passes.hip passes_begin) and sizes the allocation by it (wavefront_workspace_bytes);
// tests/host/workspace_layout_check.cpp holds it against the formulas it replaced.  Nothing here knows of HIP.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pt {

constexpr uint32_t kShards = 256;
constexpr uint32_t kXcds = 8;                // a stage launch's workgroups go to the eight XCDs round-robin (pt_wavefront.hip, k_wf_generate)
constexpr uint32_t kCounterStride = 16;      // one 64-B line per shard counter
constexpr int kCounterArrays = 7;
// 13 KiB between the carved arrays and the records, kept from the size formula this header replaced (it allowed every array 256 bytes of
// rounding that none needs).  Whether a kernel leans on it has not been examined.
constexpr size_t kWorkspaceTailPad = 52 * 256;

inline uint32_t blocks_per_shard_for(int stage_blocks) {
    uint32_t b = (uint32_t)(stage_blocks > 0 ? stage_blocks : 1536) / kShards;
    return b < 1 ? 1 : b;
}
// entries of each path-state array: whole chunks of `block` slots, the same number for every shard
inline uint32_t chunks_per_shard_for(size_t slots, uint32_t block) { return (uint32_t)(((slots + block - 1) / block + kShards - 1) / kShards); }
inline size_t state_slots_for(size_t slots, uint32_t block) { return (size_t)chunks_per_shard_for(slots, block) * kShards * block; }

struct WorkspaceRecords { bool aov, matte, motion; };      // the record arrays a call's passes need (WavefrontPasses::records)

// Byte offsets from the workspace's base, one per array of WfBuffers, in the order they lie.  Every array is a multiple of 256 bytes (a
// counter array is kShards lines, a state array whole chunks for every shard, a queue array kShards segments of whole tiles), so every
// offset is one too.
struct WorkspaceLayout {
    uint32_t blocks_per_shard, gen_rounds, seg_cap, chunks_per_shard;
    size_t state_slots;                       // entries of a path-state array and of each record array
    size_t cnt[kCounterArrays];               // contiguous: launch_wavefront clears them with one memset
    size_t L, beta_pdf, thr_misc, pend, ray_o[2], ray_d[2], q_beta[2], q_thr[2], hit, env_a, env_b, sh_o, sh_d;
    // The record arrays keep their places whether or not the earlier ones are in use: the AOV space is reserved under the matte records,
    // and both under the motion records.  An offset is valid if `total` covers its array.
    size_t rec_albedo, rec_normal;            // AovArgs: state_slots float4 each
    size_t rec_matte, rec_motion;             // MatteArgs::rec: state_slots uint32; MotionArgs::rec: state_slots float4
    size_t total;                             // bytes of a workspace with the records asked for
};

// block: slots of a tile = lanes of a workgroup (kBlock)
inline WorkspaceLayout workspace_layout(uint32_t my_tiles, uint32_t spp, int stage_blocks, WorkspaceRecords rec, uint32_t block) {
    WorkspaceLayout l;
    const size_t slots = (size_t)my_tiles * block * spp;
    l.blocks_per_shard = blocks_per_shard_for(stage_blocks);
    // k_wf_generate: workgroup-rounds that cover the (tile, sample) pairs.  Counted per XCD -- an eighth of the tiles, rounded up, against an
    // eighth of the kShards * blocks_per_shard workgroups -- which is what sizes the queue segments and the workspace.
    const uint32_t per_xcd = kShards * l.blocks_per_shard / kXcds, pairs = (my_tiles + kXcds - 1) / kXcds * spp;
    l.gen_rounds = (pairs + per_xcd - 1) / per_xcd;
    // a generate round gives shard s one tile from each of its blocks_per_shard workgroups {s, s + kShards, ...}
    l.seg_cap = l.gen_rounds * l.blocks_per_shard * block;
    l.chunks_per_shard = chunks_per_shard_for(slots, block);
    l.state_slots = state_slots_for(slots, block);
    const size_t s16 = l.state_slots * 16, q16 = (size_t)kShards * l.seg_cap * 16;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t r = at; at += (bytes + 255) & ~(size_t)255; return r; };
    for (int k = 0; k < kCounterArrays; k++) l.cnt[k] = take((size_t)kShards * kCounterStride * 4);
    l.L = take(s16); l.beta_pdf = take(s16); l.thr_misc = take(s16); l.pend = take(2 * s16);
    for (int k = 0; k < 2; k++) { l.ray_o[k] = take(q16); l.ray_d[k] = take(q16); }
    for (int k = 0; k < 2; k++) { l.q_beta[k] = take(q16); l.q_thr[k] = take(q16); }
    l.hit = take(q16); l.env_a = take(q16); l.env_b = take(q16); l.sh_o = take(2 * q16); l.sh_d = take(2 * q16);
    l.total = at += kWorkspaceTailPad;        // without records
    l.rec_albedo = take(s16); l.rec_normal = take(s16);
    if (rec.aov) l.total = at;
    l.rec_matte = take(l.state_slots * 4);
    if (rec.matte) l.total = at;
    l.rec_motion = take(s16);
    if (rec.motion) l.total = at;
    return l;
}

}  // namespace pt
