// pt_host.h -- host-visible declarations shared by the translation units of libmipt.so.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pt_types.h"
#include "pt_workspace.h"

namespace pt {

// ---- accel.hip --------------------------------------------------------------------------------
struct AccelScratch {
    TriPacket* tris_unsorted = nullptr;
    uint64_t *keys_a = nullptr, *keys_b = nullptr;
    uint32_t *vals_a = nullptr, *vals_b = nullptr;
    int32_t* leaf_parent = nullptr;
    int32_t* node_parent = nullptr;
    void* seg = nullptr;             // min/max segment tree over the sorted triangles' boxes (2 * seg_leaves entries of 32 B)
    size_t seg_leaves = 0;           // power of two >= capacity
    float* block_bounds = nullptr;   // k_setup's per-block centroid bounds
    uint32_t* bounds = nullptr;      // 6 sortable-uint floats: min xyz, max xyz
    void* sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
    BvhNode* nodes2 = nullptr;       // the binary LBVH (intermediate)
    uint32_t* kept = nullptr;        // collapse frontier (ping): binary nodes that become wide nodes
    uint32_t* widx = nullptr;        // ... and the wide-node index each was given
    uint32_t* collapse_counters = nullptr;   // greedy collapse: [0] wide nodes allocated, [1 + L] frontier size of level L
    WideRanges* wide_ranges = nullptr;       // per wide node: the sorted-triangle range under each child (kept for accel_refit)
    // PLOC builder (accel.hip 4b)
    int builder = 2;                         // PT_BUILDER_*: 0 radix tree (Karras LBVH); 1 PLOC clustering over the same Morton order; 2 PLOC + reinsertion passes (default)
    float reinsert_min_gain = 1e-3f;         // ... a move must gain this fraction of its parent's surface area
    int reinsert_passes = 8;                 // builder 2: passes of parallel reinsertion over the clustered tree (accel.hip 4c)
    void* reins_box = nullptr; int32_t *reins_parent = nullptr, *reins_top = nullptr; float* reins_gain = nullptr; uint32_t* reins_out = nullptr;
    unsigned long long* reins_lock = nullptr; uint8_t* reins_state = nullptr;
    void* ploc_c[2] = {nullptr, nullptr};    // cluster arrays (ping-pong)
    uint32_t *ploc_nn = nullptr, *ploc_valid = nullptr, *ploc_pos = nullptr, *ploc_count = nullptr, *ploc_perm = nullptr, *ploc_counters = nullptr;
    int32_t *ploc_left = nullptr, *ploc_right = nullptr;
    void* ploc_scan_temp = nullptr; size_t ploc_scan_bytes = 0;
    size_t capacity = 0;
    std::string why;                         // what a failed build ran into (the hipError_t alone says "unknown error")
    uint32_t fallbacks = 0;                  // builds in which the PLOC clustering gave up and the radix tree took over
    std::string fallback_why;                // ... and why, the last time
};
void accel_scratch_free(AccelScratch& s);
// Builds the 4-wide BVH (<= n_tris nodes), the sorted intersection packets and their shading packets (n_tris each).
// root_out: 0, or ~0 for a single triangle.  wide_nodes_out: the node count; stack_need_out: the most traversal-stack entries any
// ray can hold in this tree (max over nodes of the siblings pushed on the way down).  Synchronises the stream (a full build is
// the rare event).
hipError_t accel_build(AccelScratch& s, const BufferRec* d_buffers, const InstanceRec* d_instances, int n_inst, uint32_t n_tris, Bvh4Node* d_nodes,
                       TriPacket* d_tris, ShadePacket* d_shade, int32_t* root_out, uint32_t* wide_nodes_out, uint32_t* stack_need_out, hipStream_t stream);
// Refit after vertices or instance transforms changed (topology and triangle order kept): rewrites the intersection and shading
// packets of the instances marked in d_touched[instance], rebuilds the segment tree over the triangles' boxes and requantises
// every wide node from it.  Asynchronous.  Hits equal those of a full rebuild; only the tree's quality follows the old pose.
hipError_t accel_refit(AccelScratch& s, const InstanceRec* d_instances, const uint8_t* d_touched, uint32_t n_tris, uint32_t wide_nodes,
                       Bvh4Node* d_nodes, TriPacket* d_tris, ShadePacket* d_shade, hipStream_t stream);

// ---- pt_kernel.hip: 1024 x (sin, cos) of the packed tangent angle
hipError_t build_tangent_lut(float2* d_lut, hipStream_t stream);

// ---- envmap.hip -------------------------------------------------------------------------------
struct EnvDevice {
    uint16_t* cube = nullptr;          // all mips, RGBA16F
    size_t mip_offset[16] = {0};       // in halfs
    int mip_n[16] = {0};
    int mips = 0;
    float* importance = nullptr;       // sum pyramid
    uint32_t level_offset[12] = {0};
    int levels = 0;
    int imp_res = 1024;
    float* blocked = nullptr;          // 4x4-blocked copies of levels 4^2, 16^2, 64^2, 256^2, 1024^2 (EnvRec::blocked)
    uint32_t blocked_offset[5] = {0};
    float total = 0.f;                 // the pyramid's apex (sum of the whole map), read back once: a kernel argument instead of a load per sample
    // pt_env_filter (envfilter.hip): the GGX chain and the diffuse cube, RGBA16F, face-major level by level; absent until the first filter
    bool filtered = false;
    uint16_t* ggx = nullptr; size_t ggx_halfs = 0;         // allocated halfs: a filter with other sizes reallocates
    size_t ggx_offset[16] = {0};       // in halfs
    int ggx_n[16] = {0};
    int ggx_mips = 0;
    float ggx_roughness[16] = {0};
    uint16_t* diffuse = nullptr; size_t diffuse_halfs = 0;
    int diffuse_n = 0;
    float4* filter_table = nullptr;    // the per-sample table of one level's launch (kEnvFilterMaxSamples entries)
};
constexpr int kEnvFilterMaxSamples = 4096;
constexpr int kEnvFilterMaxResolution = 1024;
// One level of a filtered cube: what the two kernels of a level take beside the source cube (envfilter.hip).
struct EnvFilterLevel {
    int kind;                          // 0 GGX, 1 diffuse
    int samples;
    float roughness, mip_bias;
    uint16_t* out; int n;              // 6 * n * n RGBA16F texels
};
// Enqueues the table and filter kernels of one level.  e.filter_table must exist.  Asynchronous.
hipError_t env_filter_level(const EnvDevice& e, const EnvFilterLevel& level, hipStream_t stream);
hipError_t env_build(EnvDevice& e, const float* d_equirect, int w, int h, hipStream_t stream);
// A map from a cube mip 0 (n x n RGBA16F faces) and a whole sum pyramid given on the host (test hook pt_debug_env_create_raw)
hipError_t env_build_raw(EnvDevice& e, int n, const uint16_t* cube_rgba16f, const float* pyramid, hipStream_t stream);
void env_free(EnvDevice& e);

// ---- skin_tonemap.hip -------------------------------------------------------------------------
struct SkinArgs {
    uint32_t num_of_vertices, input_mesh_flags, output_mesh_flags;
    int32_t num_of_morph_targets;
    float morph_weight[4];
    const float* morph_position[4];
    const uint32_t* morph_tangent_space[4];
    const float* in_position;
    const uint32_t* in_tangent_space;
    const uint4* in_joint_weight;
    const pt_bone* bones;
    int32_t bone_count;
    float* out_position;
    uint32_t* out_tangent_space;
};
void launch_skin(const SkinArgs& a, bool use_mfma, hipStream_t stream);
void launch_tonemap(const float4* in, uint32_t w, uint32_t h, const pt_tonemap_config& cfg, float* out_rgb, uint32_t* out_rgba8, hipStream_t stream);

// ---- pt_wavefront.hip / wf_passes.hip / pt_kernel.hip -----------------------------------------
size_t traversal_grid_lanes(int stage_blocks);   // lanes of the widest traversal launch of a wavefront trace with that many stage workgroups
constexpr uint32_t kDeepStackMax = 1024;      // most stack entries a tree may ask for (64 on chip + a deep stack in memory); a clustered tree beyond it is rebuilt as a radix tree
int traversal_stack_capacity();          // entries a ray's traversal stack holds on chip (LDS part + scratch spill); deeper trees get SceneRec::deep_stack
// Optional per-stage timing of one wavefront launch (pt_enable_stage_timing): an event after every stage launch.
enum { STAGE_GENERATE = 0, STAGE_TRACE = 1, STAGE_SHADE = 2, STAGE_SHADOW = 3, STAGE_RESOLVE = 4, STAGE_COUNT = 5 };
struct StageTimers {
    std::vector<hipEvent_t> ev;          // ev[0] = start; ev[k + 1] = after the k-th launch
    std::vector<uint8_t> kind;           // STAGE_* of the k-th launch
    size_t used = 0;                     // launches recorded by the last pt_trace
    hipEvent_t event_at(size_t i);       // ev[i], created on first use; nullptr if it cannot be
    void mark(int kind, hipStream_t stream);     // the launch just enqueued on `stream` was of stage `kind`
};
inline void mark_stage(StageTimers* timers, int kind, hipStream_t stream) { if (timers) timers->mark(kind, stream); }     // (null: timing is off)
void launch_megakernel(const SceneRec& sc, const FrameConstants& fc, const LensArgs& lens, float4* output, Counters* counters, bool count, hipStream_t stream);
// pt_lens_focus_at: d_out = 2 floats {hit, view-space depth}
void launch_lens_focus(const SceneRec& sc, const FrameConstants& fc, const LensArgs& lens, float sx, float sy, uint32_t rf, float* d_out, hipStream_t stream);
// Adaptive sampling (pt_set_adaptive): the state of one of this rank's tiles, indexed by the rank-local tile (the resolve block).
// An active tile holds the context's accumulated_frames samples; a retired one keeps the count it retired with.
struct AdaptiveTile {
    uint32_t active;          // 1: gets the call's samples; 0: retired, no rays, its pixels are not written
    uint32_t samples;         // samples in the tile after the last call that reached it
    float error;              // its last error estimate E (max over its pixels)
    uint32_t pad;
};
// What the adaptive instantiations of k_wf_generate / k_wf_resolve take as their own argument (FrameConstants stays as it is).
struct AdaptiveArgs {
    AdaptiveTile* tiles;      // my_tiles entries
    float4* half;             // res_x * res_y: running mean of the samples with an even per-tile index
    int32_t min_samples;
    int32_t cap;              // min(max_samples, max_accumulated_frames)
    float threshold;
};
// First-hit AOVs (pt_set_aov): what k_wf_aov and the AOV instantiations of k_wf_resolve take as their own argument.  One record per
// slot and target, written by k_wf_aov between the primary traversal and the first shade stage, blended by the resolve.
struct AovArgs {
    float4* rec_albedo;       // per slot: (sp.albedo, 1); zeros for a miss or a non-finite sample (workspace, set by passes_begin)
    float4* rec_normal;       // per slot: (sp.n, hit.t); zeros likewise
    float4* albedo;           // the caller's targets, res_x * res_y each; either may be nullptr
    float4* normal_depth;
};
// Texture-space baking (pt_set_bake): what k_wf_generate_bake takes as its own argument, beside the tree's two packet arrays.
constexpr uint32_t kBakeNone = 0xffffffffu;
struct BakeArgs {
    const uint32_t* owner;    // res_x * res_y: the coverage map -- per texel the owner's index into tris / shade, kBakeNone where none covers
    const TriPacket* tris;
    const ShadePacket* shade;
    float surface_offset;
    int32_t tex_coord;
};
// Light-probe baking (pt_set_probes): what k_wf_generate_probe takes as its own argument.
struct ProbeArgs {
    const float* positions;   // count * 3, world space (owned by the context)
    uint32_t n, count, columns;   // each probe is an n x n octahedral map; probe k sits at atlas cell (k % columns, k / columns)
    FastDiv div_n;
    float max_distance;       // the probe ray's tmax
};
// ID mattes (pt_set_matte): what k_wf_matte and k_wf_matte_resolve take as their own argument.  One id per slot, written by k_wf_matte
// between the primary traversal and the first shade stage (beside k_wf_aov), folded into the caller's layers by k_wf_matte_resolve.
struct MatteArgs {
    uint32_t* rec;            // per slot: the id of the first ray's closest hit, 0 for a miss or a slot without a ray (workspace, set by passes_begin)
    const uint32_t* ids;      // the id of every row of the instance table (PT_MATTE_INSTANCE) or the material table (owned by the context)
    uint32_t n_ids;
    int32_t kind, ranks;      // PT_MATTE_*; K = 2, 4, 6 or 8
    float4* layers[4];        // the caller's layers, res_x * res_y each: the first K / 2
};
// Motion vectors (pt_set_motion): what k_wf_motion and k_wf_motion_resolve take as their own argument.  One record per slot, written by
// k_wf_motion between the primary traversal and the first shade stage (beside k_wf_aov), blended into the caller's target by
// k_wf_motion_resolve.  The matrices are wave-uniform kernel arguments (scalar registers).
struct MotionArgs {
    float4* rec;              // per slot: the sample's record, zeros for a miss or a non-finite record (workspace, set by passes_begin)
    const float4* snap;       // the previous pose: 3 float4 (v0, e1, e2) per triangle at InstanceRec::tri_offset + prim; nullptr = the current packets
    uint32_t n_snap;          // entries of snap
    uint32_t width, height;
    float4* target;           // the caller's target, res_x * res_y
    float mc[16], mp[16];     // world_to_clip of this call and of the previous frame
    float vc[16], vp[16];     // world_to_view likewise
};
// The variance AOV (pt_set_variance): what k_wf_variance_resolve takes as its own argument.  The pass has no record array: at resolve time
// every sample's radiance is still in the workspace (wf.L and the pending records), and the output still holds the means before the batch.
struct VarianceArgs {
    float4* target;           // the caller's target, res_x * res_y: (population variance of r, g, b; of the channel sum)
};
// The optional passes of one wavefront trace: which are on, and the argument block of each that is (the block of a pass that is off is
// not looked at).  PathtraceScene fills it (select_passes and the *_setup functions); launch_wavefront, wf_passes.hip
// (the passes' kernels and their launches) and wavefront_workspace_bytes read it.
struct WavefrontPasses {
    bool adaptive = false; AdaptiveArgs ad = {};   // off: every tile of the rank is rendered (the plain kernels); on: the adaptive generate / resolve run
    bool aov = false; AovArgs av = {};             // off: the plain resolve, no k_wf_aov launch; on: the caller's targets (the workspace holds the records; so below)
    bool bake = false; BakeArgs bk = {};           // off: camera rays (k_wf_generate); on: k_wf_generate_bake starts the paths on the atlas's texels, `lens` is not looked at
    bool probes = false; ProbeArgs pa = {};        // off likewise; on: k_wf_generate_probe starts the paths at the probes' positions (never together with `bake`)
    bool matte = false; MatteArgs mt = {};         // off: no k_wf_matte / k_wf_matte_resolve launch; on: the id table and the caller's layers
    bool motion = false; MotionArgs mo = {};       // off: no k_wf_motion / k_wf_motion_resolve launch; on: the cameras, the snapshot and the caller's target
    bool variance = false; VarianceArgs va = {};   // off: no k_wf_variance_resolve launch; on: the caller's target (no record array: records() below does not know it)
    WorkspaceRecords records() const { return {aov, matte, motion}; }     // the record arrays the workspace holds for them (pt_workspace.h)
};
// bytes of the workspace launch_wavefront needs for these frame constants, stage workgroups and passes (pt_workspace.h: the layout)
size_t wavefront_workspace_bytes(const FrameConstants& fc, int stage_blocks, const WavefrontPasses& passes);
// lens: pt_set_lens as k_wf_generate takes it (enable == 0: the pinhole)
hipError_t launch_wavefront(const SceneRec& sc, const FrameConstants& fc, const LensArgs& lens, float4* output, Counters* counters, bool count, void* workspace,
                            int stage_blocks, StageTimers* timers, hipStream_t stream, const WavefrontPasses& passes);

// ---- debug_wf.hip / debug_mk.hip: the device side of the test hooks (mipt_debug.hip), compiled as pt_wavefront.hip / pt_kernel.hip are ----
// The per-lane query hooks, one text (pt_debug_kernels.h) in both builds: sampler; environment light (8 floats in, 16 out per query); BSDF
// (48 in, 16 out); punctual lights (an index and a point in, 8 out); vertex fetch and material evaluation (8 words in, 72 out).  Only
// the wavefront build looks at small_tables; the three sizes below are its shade stage's LDS copies (kLightCacheMax, kInstCacheMax, kMatCacheMax).
struct DebugQueryLaunch {
    void (*sample_texture)(const SceneRec& sc, const uint32_t* d_mat_slot, const float* d_tc, uint32_t n, float* d_out, int32_t* d_taps, hipStream_t stream);
    void (*env_query)(const SceneRec& sc, int op, const float* d_in, uint32_t n, float* d_out, hipStream_t stream);
    void (*bsdf_query)(const SceneRec& sc, int op, uint32_t flags, const float* d_in, uint32_t n, float* d_out, hipStream_t stream);
    void (*light_query)(const SceneRec& sc, bool small_tables, int num_of_lights, const uint32_t* d_index, const float* d_p, uint32_t n, float* d_out, hipStream_t stream);
    void (*surface_query)(const SceneRec& sc, bool small_tables, uint32_t flags, const float* d_in, uint32_t n, float* d_out, hipStream_t stream);
};
DebugQueryLaunch debug_queries_wf(), debug_queries_mk();     // (functions: a const table of host functions would be emitted as device data too)
int debug_light_cache_max(), debug_inst_cache_max(), debug_mat_cache_max();
void launch_debug_intersect(const SceneRec& sc, const float* d_rays, uint32_t n, uint32_t rf, int mode, float* d_out, hipStream_t stream);
// pt_debug_camera_rays: d_out = 8 floats per query {px, py, seed}, camera_ray's ray
void launch_debug_camera_rays(const FrameConstants& fc, const LensArgs& lens, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream);
// pt_debug_bake_rays: d_out = 8 floats per query {px, py, seed}, bake_ray's ray; zeros with tmax = -1 for an uncovered texel or one off the atlas
void launch_debug_bake_rays(const FrameConstants& fc, const BakeArgs& bake, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream);
// pt_debug_probe_rays: d_out = 8 floats per query {px, py, seed}, probe_ray's ray; zeros with tmax = -1 for an absent probe or a texel off the atlas
void launch_debug_probe_rays(const FrameConstants& fc, const ProbeArgs& probes, const uint32_t* d_queries, uint32_t n, float* d_out, hipStream_t stream);
// pt_debug_trace_queues (test hook): host arrays.  closest: 8 floats per ray (origin, tmin = 0, direction, tmax); shadow: 6 floats per ray (origin,
// direction).  out_closest: 8 floats per ray as pt_debug_intersect writes them (all kDebugSentinel bits where the kernel wrote no hit record);
// out_shadow: the transmission written beside ray i's pending term; out_cnt: the counter words [shard][0..6] after the launch;
// out_stray: {hit entries, pending records} outside the rays' own that no longer hold the sentinel.
struct DebugQueues {
    const float* closest; const uint32_t* closest_shard; uint32_t n_closest;
    const float* shadow; const uint32_t* shadow_shard; const uint8_t* shadow_is_light; uint32_t n_shadow;
    float shadow_tmax;
    uint32_t flags; int bounce; uint32_t blocks_per_shard; int which;
    float* out_closest; float* out_shadow; uint32_t* out_cnt; uint32_t* out_stray;
};
hipError_t debug_trace_queues(const SceneRec& sc, const DebugQueues& q, Counters* counters, bool count, hipStream_t stream, std::string& why);

// ---- matte.hip: pt_matte_extract's mask of a set of ids ----------------------------------------------------------------------------
constexpr int kMatteExtractMaxIds = 64;
struct MatteExtractIds { uint32_t id[kMatteExtractMaxIds]; };     // after the exponent fix; by value in the kernel's arguments
// mask[p] = the sequential float32 sum over ranks 0 .. ranks - 1 of the coverages whose id is among ids.id[0 .. count - 1].  Asynchronous.
void launch_matte_extract(const float4* const layers[4], int ranks, uint32_t pixels, const MatteExtractIds& ids, int count, float* mask, hipStream_t stream);

// ---- motion.hip: the previous pose, the hook's records and pt_reproject ---------------------------------------------------------------
// snap[instances[T.inst].tri_offset + T.prim] = (T.v0, T.e1, T.e2) with w lanes 0, for every packet T of the built tree.  Asynchronous.
void launch_motion_snapshot(const TriPacket* tris, uint32_t n_tris, const InstanceRec* instances, uint32_t n_instances, float4* snap, uint32_t n_snap, hipStream_t stream);
// pt_debug_motion: d_rays = 8 floats per ray as pt_debug_intersect takes them; d_out = 8 floats per ray (record.xyzw, instance, primitive, u, v),
// zeros with instance = primitive = -1 for a miss.  The closest hit is k_debug_intersect's, the record k_wf_motion's own function.
void launch_debug_motion(const SceneRec& sc, const MotionArgs& ma, const float* d_rays, uint32_t n, uint32_t rf, float* d_out, hipStream_t stream);
struct ReprojectArgs {
    const float4 *color, *motion, *prev_color, *prev_motion;
    const float* prev_length;     // nullptr = 1 everywhere
    float4* out_color;
    float* out_length;
    uint32_t w, h;
    float alpha_min, max_history, depth_tolerance;
};
void launch_reproject(const ReprojectArgs& a, hipStream_t stream);

// ---- blur.hip: pt_motion_blur's three kernels ------------------------------------------------------------------------------------------
// V: w * h float4 (half streak x, y, its length, depth); T, N: tiles_x * tiles_y float4 each (a tile's longest streak; the longest within
// `reach` tiles) -- context-owned scratch.  out overlaps neither input.  Asynchronous.
struct BlurArgs {
    const float4 *color, *motion;
    float4 *V, *T, *N, *out;
    uint32_t w, h, tiles_x, tiles_y;
    float half_shutter;           // 0.5f * shutter, formed once
    float max_radius, depth_softness;
    int taps, jitter;
    int reach;                    // (int)ceilf(max_radius / 16.0f): 1..4
};
hipError_t launch_motion_blur(const BlurArgs& a, hipStream_t stream);

// ---- bloom.hip: pt_bloom's down and up steps over the mip chain ----------------------------------------------------------------------
// One step as a kernel takes it: level `src` (wi x hi) into level `dst` (wo x ho), 16 x 16 tiles numbered row-major, tiles_x a row.  color,
// strength: the last up step's own pixel and scale (dst is then the caller's out); threshold: the first down step's prefilter.
struct BloomStep {
    const float4 *src, *color;
    float4* dst;
    uint32_t wi, hi, wo, ho, tiles_x;
    float strength, threshold;
};
// chain: levels 1 .. n one after the other, lw[k - 1] x lh[k - 1] float4 each -- context-owned scratch.  n >= 1.  out is color or does not
// overlap it.  Asynchronous: n down steps, then n up steps.
struct BloomArgs {
    const float4* color;
    float4 *chain, *out;
    uint32_t w, h;
    int n;
    uint32_t lw[8], lh[8];
    float strength, threshold;
};
int bloom_levels(uint32_t w, uint32_t h, int iterations, uint32_t* lw, uint32_t* lh, size_t* texels);
hipError_t launch_bloom(const BloomArgs& a, hipStream_t stream);

// ---- variance.hip: pt_noise_estimate's per-tile reduction ---------------------------------------------------------------------------
// out[t] = (mean, max) of the per-pixel relative standard error over the in-image pixels of tile t (row-major 16 x 16 tiles), (-1, -1) for
// a tile whose count is below 2.  counts: one uint32 per tile on the device, nullptr = `samples` everywhere.  Asynchronous.
void launch_noise_tiles(const float4* image, const float4* variance, uint32_t w, uint32_t h, const uint32_t* counts, uint32_t samples, float2* out, hipStream_t stream);

// ---- probe.hip: pt_probe_project's reduction of an octahedral atlas to spherical harmonics --------------------------------------
// dirs: n * n float4, the texel-centre directions of an n x n octahedral map (w unused), row-major.  Asynchronous.
void launch_probe_dirs(float4* dirs, uint32_t n, hipStream_t stream);
// sh: count * 27 floats on the device, [probe][coefficient][rgb]; atlas: the (columns * n) wide float4 image.  kind: PT_PROBE_SH_*.  Asynchronous.
void launch_probe_project(const float4* atlas, const float4* dirs, uint32_t n, uint32_t count, uint32_t columns, int kind, float* sh, hipStream_t stream);

// ---- bake.hip: the coverage map of pt_set_bake and pt_bake_dilate's passes ---------------------------------------------------
// The UV rasteriser over the built tree's packets.  keys: w * h (instance << 32 | primitive of the owner, all ones where none covers);
// owner: w * h (BakeArgs::owner).  scratch: bake_coverage_scratch_bytes(n_tris).  Synchronises the stream once (the bin count).
struct BakeRaster {
    const TriPacket* tris; const ShadePacket* shade; const InstanceRec* instances;
    uint32_t n_tris, w, h;
    int32_t tex_coord, instance;      // instance -1: every instance that has the UV set
};
size_t bake_coverage_scratch_bytes(uint32_t n_tris);
hipError_t bake_coverage_build(const BakeRaster& r, unsigned long long* keys, uint32_t* owner, void* scratch, hipStream_t stream, std::string& why);
// `passes` dilation passes over image (w * h float4) from the coverage `owner`; pong: w * h float4, mask: 2 * w * h bytes.  Asynchronous.
hipError_t launch_bake_dilate(float4* image, const uint32_t* owner, uint32_t w, uint32_t h, int passes, float4* pong, uint8_t* mask, hipStream_t stream);

// ---- sort_scan.hip: the build's two data-parallel primitives, hand-written (stable LSD radix sort of (u64, u32) pairs over 63 key bits; u32 exclusive scan)
size_t radix_sort_temp_bytes(size_t n);
hipError_t radix_sort_pairs_u64_u32(void* temp, uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n, hipStream_t stream);   // keys_in / vals_in are scratch
size_t exclusive_scan_temp_bytes(size_t n);
hipError_t exclusive_scan_u32(void* temp, const uint32_t* in, uint32_t* out, size_t n, hipStream_t stream);

// ---- exchange.hip: the per-frame tile exchange of the sharded renderer (RCCL bound at run time) ---------------------------
struct ExchangeState;
uint32_t tiles_of_rank(uint32_t w, uint32_t h, uint32_t rank, uint32_t world);
hipError_t tiles_pack(const void* image, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, void* packed, hipStream_t stream);
hipError_t tiles_unpack(const void* packed, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, void* image, hipStream_t stream);
int exchange_unique_id(void* out128, std::string& err);
int exchange_probe(std::string& err);
int exchange_create(ExchangeState** out, int rank, int world, const void* id128, std::string& err);
int exchange_create_loopback(ExchangeState** out, int rank, int world, uint64_t group, int device, std::string& err);
const char* exchange_transport_name(const ExchangeState* x);
int exchange_frame(ExchangeState* x, const void* local, void* frame, uint32_t w, uint32_t h, int mode, int dst, hipStream_t stream, std::string& err);
void exchange_free(ExchangeState* x);

}  // namespace pt
