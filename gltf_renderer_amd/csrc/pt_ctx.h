// pt_ctx.h -- the context behind the C-ABI of include/mipt.h, and what the translation units with entry points need of it: mipt_api.hip (the
// core of the product), a feature's own file (bake, probe, matte, motion, blur, bloom, envfilter, variance, denoise .hip) and mipt_debug.hip (the test hooks).
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "dev_buf.h"
#include "pt_host.h"

// Pinned upload slots for the per-frame tables (materials, lights, instances, bones, vertex updates).  The reference hands those
// over in a transient upload heap that stays valid for the frame (Source/Renderer.cpp:490,496); here the caller's memory may be
// reused as soon as the call returns, so the bytes are copied into a pinned slot and go to the device asynchronously.  The host
// only ever waits when it comes round to a slot whose copy is still in flight -- not once per call.
struct StagingRing {
    static constexpr int kSlots = 8;
    void* host[kSlots] = {};
    size_t cap[kSlots] = {};
    hipEvent_t done[kSlots] = {};
    bool pending[kSlots] = {};
    int next = 0;
};

enum AccelState { ACCEL_CLEAN = 0, ACCEL_REFIT = 1, ACCEL_REBUILD = 2 };

// Every device array below that is not handle-indexed is a DevBuf: it carries its capacity and goes with the context (pt_destroy).
struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
    StagingRing staging;

    // ---- ResourceTable ("descriptor heap")
    std::vector<pt::BufferRec> buffers;
    std::vector<pt::TextureRec> textures;
    std::vector<pt::SamplerRec> samplers;
    pt::DevBuf d_buffers; bool buffers_dirty = true;               // device copy (BufferRec): BVH build only
    pt::DevBuf d_white;                                            // 1x1 white texel behind every unbound material slot
    // interleaved albedo / normal / metal-rough texels of the materials whose three textures share one footprint (pt_types.h RM_TRIO),
    // keyed by the three texel pointers (nullptr = slot unbound); owned here, rebuilt / released by pt_scene_set_materials
    struct TrioRec { const uint32_t *a, *n, *m, *e; uint4* ptr; };
    std::vector<TrioRec> trios;

    // ---- per-frame arrays (Renderer::GatherMaterials / GatherLights)
    pt::DevBuf d_rmats; int n_materials = 0;                       // RMat, resolved on the host in pt_scene_set_materials
    std::vector<pt::RMat> rmats_host;                              // what was uploaded (pt_texture_destroy checks it)
    pt::DevBuf d_lights; int n_lights = 0;                         // pt_light

    // ---- instance table + acceleration structure
    std::vector<pt::InstanceRec> instances;
    pt::DevBuf d_instances;                                        // InstanceRec
    uint32_t n_tris = 0;
    pt::DevBuf d_nodes, d_tris, d_shade;                           // Bvh4Node, TriPacket, ShadePacket: one capacity in triangles for the three
    uint32_t wide_nodes = 0, stack_need = 0;
    int32_t root = 0;
    pt::AccelScratch scratch;
    // What the next pt_build_accel / pt_trace has to do: nothing, a refit of the instances marked in `touched` (vertices or
    // transform changed: UpdateDynamicBlas + the per-frame TLAS rebuild upstream), or a full build (topology changed).
    int accel_state = ACCEL_REBUILD;
    bool accel_built = false;                 // a full build of the current instance table exists (a refit needs one)
    bool instances_dirty = true;              // the device copy of the instance table is stale
    std::vector<uint8_t> touched;             // per instance
    pt::DevBuf d_touched;
    uint32_t accel_refits = 0, accel_builds = 0;
    bool accel_last_was_refit = false;        // the last thing BuildAccel did: the scratch's sorted keys are those of the last full build (pt_debug_accel_keys)
    std::vector<int> free_buffers, free_textures, free_envs;      // destroyed handles, reused by the next create

    std::vector<pt::EnvDevice*> envs;
    pt::DevBuf d_sheen, d_srgb, d_tangent_lut, d_counters;        // float[256] twice, float2[1024], Counters: allocated by pt_create
    pt::DevBuf d_bones; size_t bones_used = 0;                     // bone arena: one slice per pt_skin_run, wraps behind a fence
    hipEvent_t bones_fence = nullptr; bool bones_fence_pending = false;
    pt::DevBuf d_workspace;                                        // wavefront ray / hit / path-state arrays
    pt::DevBuf d_tonemap;                                          // pt_tonemap's device scratch (float RGB + RGBA8), reused
    pt::ExchangeState* exchange = nullptr;                         // pt_exchange_* (exchange.hip)
    pt::DevBuf d_deep;                                             // deep traversal stack (SceneRec::deep_stack), only for trees that need > 64 entries
    bool stage_timing = false;                                 // pt_enable_stage_timing
    pt::StageTimers timers;
    int kernel_mode = PT_MODE_WAVEFRONT;
    int stage_blocks = 0;         // workgroups per stage launch; 0 = by the size of the launch (stage_blocks_for)
    hipEvent_t ev_trace[2] = {nullptr, nullptr}, ev_accel[2] = {nullptr, nullptr}, ev_skin[2] = {nullptr, nullptr};
    bool have_trace = false, have_accel = false, have_skin = false;
    int bounce_limit = PT_REFERENCE_MAX_BOUNCES;
    int samples_per_trace = 1;
    // pt_set_adaptive / _aov / _lens / _bake / _probes / _matte / _motion / _variance since the last trace: the next pt_trace that gets as far as its
    // reset starts a new accumulation (PathtraceScene consumes it; pt_accum_save refuses while it stands; pt_accum_load clears it)
    bool restart_pending = false;
    bool cull_null_shadow = false;
    bool watertight = false;                                       // pt_set_watertight
    bool counters_enabled = false;
    // ---- adaptive sampling (pt_set_adaptive): per rank-local tile state and the half buffer, for one size and tile shard
    pt_adaptive_config adaptive = {0, 2, 2, 0.0f};
    pt::DevBuf d_ad_tiles, d_ad_half;             // AdaptiveTile per tile, float4 per pixel
    uint32_t ad_w = 0, ad_h = 0, ad_rank = 0, ad_rank_count = 0, ad_my_tiles = 0;
    bool ad_ready = false;                        // an adaptive trace ran for (ad_w, ad_h, ad_rank, ad_rank_count)
    int ad_frames = -1;                           // accumulated_frames the tile state stands for (-1: none)
    // ---- pt_accum_save / pt_accum_load: the packed sections of one blob (one pt_tiles_pack image each), reused between calls
    pt::DevBuf d_accum;
    // ---- first-hit AOVs (pt_set_aov): the caller's targets
    pt_aov_config aov = {0, nullptr, nullptr};
    // ---- thin lens (pt_set_lens)
    pt_lens_config lens = {0, 0.0f, 1.0f, 0, 0.0f};
    // ---- texture-space baking (pt_set_bake): the config, and the coverage map of one atlas size, config and state of the tree
    pt_bake_config bake = {0, 0, -1, 0.0f};
    pt::DevBuf d_bake_keys, d_bake_owner;         // per texel: the owner's (instance << 32 | primitive); its index into d_tris / d_shade (BakeArgs::owner)
    pt::DevBuf d_bake_scratch;                    // the rasteriser's bin counts and scan (bake.hip)
    pt::DevBuf d_bake_dilate;                     // pt_bake_dilate: one image and two fill masks
    bool bake_ready = false;                      // the map stands for (bake_w, bake_h, bake_built, bake_accel)
    uint32_t bake_w = 0, bake_h = 0;
    pt_bake_config bake_built = {0, 0, -1, 0.0f};
    uint64_t bake_accel = 0;                      // accel_builds + accel_refits when the map was built: the packets it was rasterised from
    // ---- light-probe baking (pt_set_probes): the config, the probes' positions, and pt_probe_project's direction table and result
    pt_probe_config probes = {0, 16, 1, 1, 1000.0f};
    pt::DevBuf d_probe_pos;                       // float[3] per probe (ProbeArgs::positions): probes.count of them while probes.enable != 0
    pt::DevBuf d_probe_dirs; uint32_t probe_dirs_n = 0;   // the texel-centre directions of a probe_dirs_n^2 map, built by the first pt_probe_project of a resolution
    pt::DevBuf d_probe_sh;                        // pt_probe_project's 27 floats per probe
    // ---- ID mattes (pt_set_matte): the config with the caller's layers, the caller's ids, and the device table of one id per table row
    pt_matte_config matte = {0, PT_MATTE_INSTANCE, 2, 0, {nullptr, nullptr, nullptr, nullptr}};
    std::vector<uint32_t> matte_user_ids;         // fix(ids[i]) of pt_set_matte; rows beyond it get the ids of their default names
    pt::DevBuf d_matte_ids;                       // uint32 per row (MatteArgs::ids), made by pt_trace for ...
    int matte_table_kind = -1; size_t matte_table_rows = 0;   // ... this kind (-1: stale) and this many rows of the instance / material table
    // ---- motion vectors (pt_set_motion): the config with the caller's target, and the previous pose (pt_motion_snapshot)
    pt_motion_config motion = {};
    pt::DevBuf d_motion_snap;                     // 3 float4 per triangle of the instance table, at InstanceRec::tri_offset + prim (MotionArgs::snap)
    bool motion_snap_taken = false;               // a snapshot exists; it stands for a table of ...
    std::vector<uint32_t> motion_snap_counts;     // ... these tri_count, row by row
    // ---- the variance AOV (pt_set_variance): the config with the caller's target; pt_noise_estimate's per-tile counts and (mean, max) pairs
    pt_variance_config variance = {0, 0, nullptr};
    pt::DevBuf d_noise;                           // one uint32 and one float2 per tile, for one tile count
    // ---- pt_motion_blur: the per-pixel streak image V, then the tile maxima T and their neighbourhood maxima N, for one image size
    pt::DevBuf d_blur;
    // ---- pt_bloom: the mip chain, levels 1 .. n one after the other, one float4 a texel, for one image size and level count
    pt::DevBuf d_bloom;
    // ---- pt_denoise: two ping-pong signal images and the guide image, one float4 a pixel each, for one image size
    pt::DevBuf d_denoise;
    // ---- pt_denoise_variance: two signal images (S.rgb, v) and the guide image, one float4 a pixel each, the plane of vt, one float a pixel,
    // and one uint32 per tile for the counts; for one image size.  Its own, so that alternating the two filters reallocates nothing
    pt::DevBuf d_denoise_variance;

    // ---- Pathtracer cross-frame state (Source/Pathtracer.h:152-153)
    float previous_world_to_clip[16] = {0};
    int accumulated_frames = 0;

    int fail(int code, const std::string& msg) { error = msg; return code; }
};

#define HIPOK(call)                                                                                          \
    do {                                                                                                     \
        hipError_t _e = (call);                                                                              \
        if (_e != hipSuccess) return ctx->fail(PT_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)
// Every entry point that touches the device makes the context's device current first: two contexts on two GPUs in one process
// (one per rank thread, or a host that drives several GPUs itself) must not launch or allocate on each other's device.
#define ENTER(ctx)                                                                                           \
    do {                                                                                                     \
        hipError_t _e = hipSetDevice((ctx)->device);                                                         \
        if (_e != hipSuccess) return (ctx)->fail(PT_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(_e)); \
    } while (0)

namespace pt {

// Host -> device through a pinned slot of the context's ring, asynchronous on its stream.  grow_failed: what a grow that answers an exhausted
// device with PT_ERR_OUT_OF_MEMORY and its own text returns (anything else DevBuf::realloc fails with is its synchronise).  (mipt_api.hip)
hipError_t staged_upload(pt_ctx* ctx, void* dst, const void* src, size_t bytes);
int grow_failed(pt_ctx* ctx, hipError_t e, const std::string& what);
// A post filter's scratch stands for one size alone: exactly `need` bytes, reallocated when it holds any other amount (a smaller image
// reallocates too).  who: the filter's name, the prefix of its text beside PT_ERR_OUT_OF_MEMORY
inline int exact_scratch(pt_ctx* ctx, DevBuf& d, size_t need, const char* who) {
    if (need == d.cap) return PT_OK;
    const hipError_t e = d.realloc(ctx->stream, need);
    return e == hipSuccess ? PT_OK : grow_failed(ctx, e, std::string(who) + ": " + std::to_string(need) + " bytes of scratch");
}
// Do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte: the entry points that take several device images refuse aliases by it
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// The camera of a call, from pt_execute_params and the lens config: world_to_clip as pt_trace compares it between calls, its inverse and
// view_to_world (fp64, rounded once) and the lens as camera_ray takes it (include/mipt.h pt_set_lens).  PathtraceScene, pt_lens_focus_at
// and the hook pt_debug_camera_rays all come through here, so that the rays they speak of are the same rays.  (mipt_api.hip)
struct CameraSetup {
    float world_to_clip[16], clip_to_world[16], view_to_world[16];
    LensArgs lens;
};
bool camera_setup(const pt_execute_params* ep, const pt_lens_config& cfg, CameraSetup& cam);
// What pinhole_ray reads of FrameConstants, the rest zero (the two camera hooks; PathtraceScene fills the rest as well)
void camera_constants(const CameraSetup& cam, const pt_execute_params* ep, FrameConstants& fc);

// The bake of a call (pt_set_bake): the coverage map for a width x height atlas -- built now unless it stands for this size, config and
// state of the tree -- and what k_wf_generate_bake takes.  After ensure_accel.  pt_trace and the hook pt_debug_bake_rays both come through
// here.  (bake.hip)
int bake_setup(pt_ctx* ctx, uint32_t width, uint32_t height, BakeArgs& bake);

// The probes of a call (pt_set_probes, probe.hip) as k_wf_generate_probe takes them, and the atlas they make: inline, for select_passes
// (mipt_api.hip) and the hook pt_debug_probe_rays read them too
inline void probe_atlas_size(const pt_probe_config& c, uint64_t& w, uint64_t& h) {
    w = (uint64_t)c.columns * (uint64_t)c.resolution;
    h = (((uint64_t)c.count + (uint64_t)c.columns - 1) / (uint64_t)c.columns) * (uint64_t)c.resolution;
}
inline ProbeArgs probe_args(const pt_ctx* ctx) {
    ProbeArgs pa;
    pa.positions = ctx->d_probe_pos.as<float>();
    pa.n = (uint32_t)ctx->probes.resolution; pa.count = (uint32_t)ctx->probes.count; pa.columns = (uint32_t)ctx->probes.columns;
    pa.div_n = FastDiv::make(pa.n); pa.max_distance = ctx->probes.max_distance;
    return pa;
}

// The optional passes of a call: which are on for these settings, the refusals -- no pass runs in the megakernel mode, a bake's instance,
// the probes' atlas size, no motion vectors under a bake or probes -- and the blocks that are plain copies of the context (the AOV targets,
// the probes, the variance target).  The blocks that need the device are filled by the *_setup functions, each where its failure has its place among the call's
// other refusals.  adaptive_setup: the tile state and half buffer for this size and shard, fresh if the call starts an accumulation;
// frame_cap: where that ends.  (mipt_api.hip)
int select_passes(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* ep, WavefrontPasses& passes);
int adaptive_setup(pt_ctx* ctx, const pt_execute_params* ep, const FrameConstants& fc, int frame_cap, AdaptiveArgs& adaptive);

// The mattes of a call (pt_set_matte): the device table of ids -- made now unless it stands for this kind and this many rows -- and what
// k_wf_matte / k_wf_matte_resolve take.  (matte.hip)
int matte_setup(pt_ctx* ctx, MatteArgs& matte);

// The motion vectors of a call (pt_set_motion): the two cameras, the snapshot if it is valid for the current instance table, the caller's
// target.  mc = the call's world_to_clip (CameraSetup).  motion_snapshot_state: PT_MOTION_SNAPSHOT_*.  (motion.hip)
int motion_snapshot_state(const pt_ctx* ctx);
void motion_setup(const pt_ctx* ctx, const float* world_to_clip, const pt_execute_params* ep, MotionArgs& motion);
// world_to_clip = view_to_clip * world_to_view by the routine camera_setup forms a call's with (mipt_api.hip)
void world_to_clip_of(const float* view_to_clip, const float* world_to_view, float* out);

// Pathtracer::BuildAccel (mipt_api.hip) if the tree does not stand for the current tables, as every call that traces rays begins
int ensure_accel(pt_ctx* ctx);

inline bool live_env(const pt_ctx* ctx, int env) { return env >= 0 && env < (int)ctx->envs.size() && ctx->envs[env] != nullptr; }

// A handle for `rec`: one a destroy gave back, else a new one at the end of the table.
template <typename T>
int take_slot(std::vector<T>& table, std::vector<int>& free_list, const T& rec) {
    if (free_list.empty()) { table.push_back(rec); return (int)table.size() - 1; }
    const int h = free_list.back();
    free_list.pop_back();
    table[h] = rec;
    return h;
}

// The scene as the kernels take it: tables, tree and lookup tables, no environment and no deep stack (the caller adds those)
inline SceneRec scene_fill(const pt_ctx* ctx) {
    SceneRec sc;
    memset(&sc, 0, sizeof(sc));
    sc.rmats = ctx->d_rmats.as<RMat>(); sc.lights = ctx->d_lights.as<pt_light>(); sc.instances = ctx->d_instances.as<InstanceRec>();
    sc.n_materials = (uint32_t)ctx->n_materials; sc.n_instances = (uint32_t)ctx->instances.size();
    sc.nodes = ctx->d_nodes.as<Bvh4Node>(); sc.tris = ctx->d_tris.as<TriPacket>(); sc.shade = ctx->d_shade.as<ShadePacket>(); sc.root = ctx->root; sc.num_tris = ctx->n_tris;
    sc.sheen_e = ctx->d_sheen.as<float>(); sc.srgb_lut = ctx->d_srgb.as<float>(); sc.tangent_lut = ctx->d_tangent_lut.as<float2>();
    sc.watertight = ctx->watertight ? 1u : 0u;
    return sc;
}
inline void scene_set_env(SceneRec& sc, const EnvDevice& ed) {
    sc.env.cube = ed.cube; sc.env.cube_n = ed.mip_n[0]; sc.env.importance = ed.importance;
    for (int i = 0; i < 12; i++) sc.env.level_offset[i] = ed.level_offset[i];
    sc.env.imp_res = ed.imp_res; sc.env.imp_levels = ed.levels; sc.env.imp_total = ed.total;
    sc.env.blocked = ed.blocked;
    for (int i = 0; i < 5; i++) sc.env.blocked_offset[i] = ed.blocked_offset[i];
    sc.has_env = 1;
}

// Entries a lane's deep stack holds in memory, beyond those on chip (SceneRec::deep_entries); 0: the tree needs none
inline uint32_t deep_stack_entries(const pt_ctx* ctx) {
    const uint32_t on_chip = (uint32_t)traversal_stack_capacity();
    return ctx->stack_need > on_chip ? (ctx->stack_need - on_chip + 7u) & ~7u : 0u;
}
// The deep stack of one call outside pt_trace (which keeps its own in d_deep), if the tree needs one: deep_stack_entries(ctx) entries for
// each of `lanes` lanes in `buf`, attached to `sc`.  what: the text beside PT_ERR_OUT_OF_MEMORY when the device has no room for it.
inline int temp_deep_stack(pt_ctx* ctx, SceneRec& sc, TempBuf& buf, size_t lanes, const char* what) {
    const uint32_t entries = deep_stack_entries(ctx);
    if (entries == 0) return PT_OK;
    if (buf.alloc((size_t)entries * lanes * 4) != hipSuccess) { (void)hipGetLastError(); return ctx->fail(PT_ERR_OUT_OF_MEMORY, what); }
    sc.deep_stack = buf.as<int32_t>(); sc.deep_entries = entries; sc.deep_lanes = (uint32_t)lanes;
    return PT_OK;
}

}  // namespace pt
