// mipt_api.hip -- host side of libmipt.so: the C-ABI of include/mipt.h over C++ mirrors of the
// reference's hot-path classes.
//
//   class Pathtracer   <- Source/Pathtracer.{h,cpp}: Init / PathtraceScene / Shutdown, the cross-frame
//                         state (accumulated_frames, previous_world_to_clip), BuildAllBlas/UpdateAllBlas/BuildTlas
//                         folded into one on-device LBVH build (accel.hip)
//   class GpuSkin      <- Source/GpuSkin.{h,cpp}: Create / Run
//   class EnvironmentMap <- Source/EnvironmentMap.{h,cpp}: CreateEnvironmentMap (cube + importance only)
//   ResourceTable      <- the bindless descriptor heap (DescriptorAllocator.h), as raw device pointers
// This file is the core of the product: context lifetime, resources, scene tables, trace (with select_passes, where a call's optional passes
// are weighed against each other), camera and lens, adaptive sampling and pt_accum_*, skin, post, exchange.  A feature that has a file keeps
// its setter, *_setup and entry points there (bake, probe, matte, motion, blur, variance, denoise .hip).  The context itself is
// in pt_ctx.h, the owner of its device arrays in dev_buf.h, the test hooks (pt_debug_*) in mipt_debug.hip.
// There is no CPU fallback anywhere in this file: every compute entry point launches HIP kernels.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pt_ctx.h"
#include "host/accum_state.h"

using namespace pt;

// (pt_ctx.h)
hipError_t pt::staged_upload(pt_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    StagingRing& r = ctx->staging;
    const int k = r.next;
    r.next = (r.next + 1) % StagingRing::kSlots;
    hipError_t e;
    if (r.pending[k]) { if ((e = hipEventSynchronize(r.done[k]))) return e; r.pending[k] = false; }
    if (bytes > r.cap[k]) {
        if (r.host[k]) hipHostFree(r.host[k]);
        r.host[k] = nullptr; r.cap[k] = 0;
        const size_t nc = bytes + bytes / 2 + 4096;
        if ((e = hipHostMalloc(&r.host[k], nc, hipHostMallocDefault))) return e;
        r.cap[k] = nc;
    }
    if (!r.done[k] && (e = hipEventCreateWithFlags(&r.done[k], hipEventDisableTiming))) return e;
    memcpy(r.host[k], src, bytes);
    if ((e = hipMemcpyAsync(dst, r.host[k], bytes, hipMemcpyHostToDevice, ctx->stream))) return e;
    if ((e = hipEventRecord(r.done[k], ctx->stream))) return e;
    r.pending[k] = true;
    return hipSuccess;
}
int pt::grow_failed(pt_ctx* ctx, hipError_t e, const std::string& what) {
    if (e != hipErrorOutOfMemory) return ctx->fail(PT_ERR_DEVICE, std::string("hipStreamSynchronize(ctx->stream): ") + hipGetErrorString(e));
    (void)hipGetLastError();
    return ctx->fail(PT_ERR_OUT_OF_MEMORY, what);
}

namespace {

template <typename T>
hipError_t upload_table(pt_ctx* ctx, DevBuf& d, const std::vector<T>& h) {
    const size_t n = h.size() ? h.size() : 1;
    const hipError_t e = d.reserve(ctx->stream, n * sizeof(T), (n + n / 2 + 8) * sizeof(T));
    if (e || h.empty()) return e;
    return staged_upload(ctx, d.ptr, h.data(), h.size() * sizeof(T));
}

// The adaptive tile state (`tiles` AdaptiveTile) and half buffer (`px` float4), reallocated together when either is too small; what they
// held is gone then, and with it what pt_adaptive_read could show (PathtraceScene and pt_accum_load fill them next)
int adaptive_state(pt_ctx* ctx, size_t tiles, size_t px) {
    if (tiles * sizeof(AdaptiveTile) <= ctx->d_ad_tiles.cap && px * 16 <= ctx->d_ad_half.cap) return PT_OK;
    ctx->ad_ready = false;
    hipError_t e = ctx->d_ad_tiles.realloc(ctx->stream, tiles * sizeof(AdaptiveTile));
    if (e == hipSuccess) e = ctx->d_ad_half.realloc(ctx->stream, px * 16);
    return e == hipSuccess ? PT_OK : grow_failed(ctx, e, "adaptive tile state");
}

// glm closed forms.  Inverses in fp64, rounded once.
void mat4_mul(const float* a, const float* b, float* out) {
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) {
            float s = 0;
            for (int k = 0; k < 4; k++) s += a[k * 4 + r] * b[c * 4 + k];
            out[c * 4 + r] = s;
        }
}
bool mat4_inverse_d(const float* mf, double* inv) {
    double m[16];
    for (int i = 0; i < 16; i++) m[i] = mf[i];
    double s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[9] - m[8] * m[1], s2 = m[0] * m[13] - m[12] * m[1];
    double s3 = m[4] * m[9] - m[8] * m[5], s4 = m[4] * m[13] - m[12] * m[5], s5 = m[8] * m[13] - m[12] * m[9];
    double c5 = m[10] * m[15] - m[14] * m[11], c4 = m[6] * m[15] - m[14] * m[7], c3 = m[6] * m[11] - m[10] * m[7];
    double c2 = m[2] * m[15] - m[14] * m[3], c1 = m[2] * m[11] - m[10] * m[3], c0 = m[2] * m[7] - m[6] * m[3];
    double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    if (det == 0) return false;
    double id = 1.0 / det;
    inv[0] = (m[5] * c5 - m[9] * c4 + m[13] * c3) * id;
    inv[4] = (-m[4] * c5 + m[8] * c4 - m[12] * c3) * id;
    inv[8] = (m[7] * s5 - m[11] * s4 + m[15] * s3) * id;
    inv[12] = (-m[6] * s5 + m[10] * s4 - m[14] * s3) * id;
    inv[1] = (-m[1] * c5 + m[9] * c2 - m[13] * c1) * id;
    inv[5] = (m[0] * c5 - m[8] * c2 + m[12] * c1) * id;
    inv[9] = (-m[3] * s5 + m[11] * s2 - m[15] * s1) * id;
    inv[13] = (m[2] * s5 - m[10] * s2 + m[14] * s1) * id;
    inv[2] = (m[1] * c4 - m[5] * c2 + m[13] * c0) * id;
    inv[6] = (-m[0] * c4 + m[4] * c2 - m[12] * c0) * id;
    inv[10] = (m[3] * s4 - m[7] * s2 + m[15] * s0) * id;
    inv[14] = (-m[2] * s4 + m[6] * s2 - m[14] * s0) * id;
    inv[3] = (-m[1] * c3 + m[5] * c1 - m[9] * c0) * id;
    inv[7] = (m[0] * c3 - m[4] * c1 + m[8] * c0) * id;
    inv[11] = (-m[3] * s3 + m[7] * s1 - m[11] * s0) * id;
    inv[15] = (m[2] * s3 - m[6] * s1 + m[10] * s0) * id;
    return true;
}
bool mat4_inverse(const float* mf, float* out) {
    double inv[16];
    if (!mat4_inverse_d(mf, inv)) return false;
    for (int i = 0; i < 16; i++) out[i] = (float)inv[i];
    return true;
}

size_t format_stride(int f) {
    switch (f) {
        case PT_FORMAT_R16_UINT: return 2;
        case PT_FORMAT_R32_UINT: return 4;
        case PT_FORMAT_R32G32B32_FLOAT: return 12;
        case PT_FORMAT_R10G10B10A2_UNORM: return 4;
        case PT_FORMAT_R32G32_FLOAT: return 8;
        case PT_FORMAT_R16G16B16A16_UNORM: return 8;
        case PT_FORMAT_JOINT_WEIGHT: return 16;
        default: return 0;
    }
}

// A material's texture slots in the order of RMat::tex (pt_types.h SLOT_*)
std::array<const pt_texture_sample*, SLOT_COUNT> material_slots(const pt_material& s) {
    return {&s.normal, &s.albedo, &s.metallic_roughness, &s.occlusion, &s.emissive, &s.specular, &s.specular_color, &s.clearcoat,
            &s.clearcoat_roughness, &s.clearcoat_normal, &s.anisotropy, &s.sheen_color, &s.sheen_roughness, &s.transmission, &s.thickness};
}

// Workgroups per stage launch.  256 CUs hold 6 resident 256-thread workgroups of the trace stages (LDS- and VGPR-limited): 1536
// for a launch that has the rays to feed them.  A small launch (a 1/8 tile shard of one sample) is better off with fewer
// persistent workgroups -- each stages its LDS tables and polls the shard queues whether it gets rays or not.  Measured
// (tools/stage_blocks_probe.py, Mrays/s at 512 / 768 / 1536 workgroups): 259 k slots 1121 / 1099 / 1065, 518 k slots
// 1632 / 1685 / 1551, 2.07 M slots 2500 / 2697 / 3149.
int stage_blocks_for(size_t slots) { return slots >= 1200000 ? 1536 : (slots >= 400000 ? 768 : 512); }

// A vertex stream was rewritten (pt_skin_run, pt_buffer_update): the instances that read it need their packets rebuilt (refit);
// a rewritten index stream changes which vertices form a triangle, which the refit also handles (it re-reads the indices), but
// the Morton order was made for the old triangles -- still correct, only slower -- so that stays a refit too.
bool reads_buffer(const InstanceRec& r, const void* ptr) {
    return r.p_index == ptr || r.p_position == ptr || r.p_tangent_space == ptr || r.p_texcoord[0] == ptr || r.p_texcoord[1] == ptr || r.p_color == ptr;
}
void mark_buffer_users(pt_ctx* ctx, int handle) {
    if (handle < 0) return;
    if (ctx->touched.size() != ctx->instances.size()) ctx->touched.assign(ctx->instances.size(), 0);
    const void* ptr = ctx->buffers[handle].ptr;
    bool any = false;
    for (size_t i = 0; i < ctx->instances.size(); i++) {
        if (reads_buffer(ctx->instances[i], ptr)) {
            ctx->touched[i] = 1;
            any = true;
        }
    }
    if (any && ctx->accel_state == ACCEL_CLEAN) ctx->accel_state = ACCEL_REFIT;
}

}  // namespace

// (pt_ctx.h)
void pt::world_to_clip_of(const float* view_to_clip, const float* world_to_view, float* out) { mat4_mul(view_to_clip, world_to_view, out); }
bool pt::camera_setup(const pt_execute_params* ep, const pt_lens_config& cfg, CameraSetup& cam) {
    mat4_mul(ep->view_to_clip, ep->world_to_view, cam.world_to_clip);               // Pathtracer.cpp:262
    double v2w[16];
    if (!mat4_inverse_d(ep->world_to_view, v2w) || !mat4_inverse(cam.world_to_clip, cam.clip_to_world)) return false;
    for (int i = 0; i < 16; i++) cam.view_to_world[i] = (float)v2w[i];
    LensArgs& l = cam.lens;
    memset(&l, 0, sizeof(l));
    l.enable = (cfg.enable != 0 && cfg.aperture_radius > 0.0f) ? 1 : 0;
    l.radius = cfg.aperture_radius; l.focus = cfg.focus_distance;
    const int col[3] = {0, 1, 2};
    float* dst[3] = {l.R, l.U, l.F};
    for (int a = 0; a < 3; a++) {
        const double* v = v2w + 4 * col[a];
        const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), sgn = a == 2 ? -1.0 : 1.0;
        for (int k = 0; k < 3; k++) dst[a][k] = (float)(sgn * v[k] / len);
    }
    for (int k = 0; k < 3; k++) l.c[k] = (float)v2w[12 + k];
    l.blades = cfg.enable ? cfg.blades : 0;
    if (l.blades < 3 || l.blades > kLensMaxBlades) l.blades = 0;                    // (pt_set_lens lets nothing else through)
    for (int k = 0; k <= l.blades && l.blades; k++) {
        const double ang = (double)cfg.blade_rotation + 2.0 * 3.14159265358979323846 * (double)(k % l.blades) / (double)l.blades;
        l.vert[k][0] = (float)std::cos(ang); l.vert[k][1] = (float)std::sin(ang);
    }
    return true;
}
void pt::camera_constants(const CameraSetup& cam, const pt_execute_params* ep, FrameConstants& fc) {
    memset(&fc, 0, sizeof(fc));
    memcpy(fc.clip_to_world, cam.clip_to_world, 64);
    fc.camera_pos[0] = cam.view_to_world[12]; fc.camera_pos[1] = cam.view_to_world[13]; fc.camera_pos[2] = cam.view_to_world[14];
    fc.res_x = ep->width; fc.res_y = ep->height;
}

// =================================================================================================
// class Pathtracer (Source/Pathtracer.h:16-157)
namespace pt {
class Pathtracer {
public:
    // Pathtracer::BuildAllBlas + UpdateAllBlas + BuildTlas (Source/Pathtracer.cpp:138-257).  Upstream builds a BLAS once per
    // primitive, refits the dynamic ones every frame (UpdateDynamicBlas, RayTracingAccelerationStructure.cpp:110-158) and rebuilds a
    // small TLAS every frame.  Here: ONE full build of the flattened soup when the set of triangles changes, and a refit -- packets
    // of the touched instances rewritten in place, every box re-derived -- when only vertices or transforms moved.
    static int BuildAccel(pt_ctx* ctx) {
        if (ctx->buffers_dirty) { HIPOK(upload_table(ctx, ctx->d_buffers, ctx->buffers)); ctx->buffers_dirty = false; }
        if (ctx->instances_dirty) { HIPOK(upload_table(ctx, ctx->d_instances, ctx->instances)); ctx->instances_dirty = false; }
        if (ctx->accel_state == ACCEL_CLEAN && ctx->accel_built) return PT_OK;
        const bool refit = ctx->accel_built && ctx->accel_state == ACCEL_REFIT;
        if (!refit) {
            const size_t need = ctx->n_tris ? ctx->n_tris : 1, cap = need + need / 8 + 64;
            HIPOK(ctx->d_nodes.reserve(ctx->stream, need * sizeof(Bvh4Node), cap * sizeof(Bvh4Node)));
            HIPOK(ctx->d_tris.reserve(ctx->stream, need * sizeof(TriPacket), cap * sizeof(TriPacket)));
            HIPOK(ctx->d_shade.reserve(ctx->stream, need * sizeof(ShadePacket), cap * sizeof(ShadePacket)));
        }
        const InstanceRec* d_instances = ctx->d_instances.as<InstanceRec>();
        Bvh4Node* d_nodes = ctx->d_nodes.as<Bvh4Node>(); TriPacket* d_tris = ctx->d_tris.as<TriPacket>(); ShadePacket* d_shade = ctx->d_shade.as<ShadePacket>();
        HIPOK(hipEventRecord(ctx->ev_accel[0], ctx->stream));
        if (refit) {
            const size_t n = ctx->instances.size();
            HIPOK(ctx->d_touched.reserve(ctx->stream, n, n + 64));
            HIPOK(staged_upload(ctx, ctx->d_touched.ptr, ctx->touched.data(), n));
            HIPOK(accel_refit(ctx->scratch, d_instances, ctx->d_touched.as<uint8_t>(), ctx->n_tris, ctx->wide_nodes, d_nodes, d_tris, d_shade, ctx->stream));
            ctx->accel_refits++;
        } else {
            ctx->scratch.why.clear();
            const hipError_t be = accel_build(ctx->scratch, ctx->d_buffers.as<BufferRec>(), d_instances, (int)ctx->instances.size(), ctx->n_tris, d_nodes, d_tris,
                                              d_shade, &ctx->root, &ctx->wide_nodes, &ctx->stack_need, ctx->stream);
            if (be != hipSuccess) {
                ctx->accel_built = false; ctx->accel_state = ACCEL_REBUILD;
                return ctx->fail(PT_ERR_DEVICE, std::string("acceleration-structure build: ") + (ctx->scratch.why.empty() ? hipGetErrorString(be) : ctx->scratch.why.c_str()));
            }
            ctx->accel_builds++;
        }
        HIPOK(hipEventRecord(ctx->ev_accel[1], ctx->stream));
        ctx->have_accel = true;
        ctx->accel_state = ACCEL_CLEAN;
        ctx->accel_built = true;
        ctx->accel_last_was_refit = refit;
        std::fill(ctx->touched.begin(), ctx->touched.end(), (uint8_t)0);
        // The build reports the most stack entries any ray can hold in this tree (a node pushes its other children).  A lane holds 64
        // on chip (LDS + scratch).  A tree that needs more -- long chains of coincident centroids; the reference's driver BVH logs and
        // skips only a primitive it cannot build, RayTracingAccelerationStructure.cpp:137-140 -- is never refused and never drops pushes:
        // its rays get a deep stack in memory for the entries beyond 64 (SceneRec::deep_stack, sized at the next pt_trace).  Only a
        // clustered tree deeper than kDeepStackMax entries is rebuilt as a radix tree, whose depth is bounded by the key (64 Morton
        // bits + 32 index bits: at most 3 x 96 entries).  A refit keeps the topology, so the figure of the build stands.
        if (!refit && ctx->stack_need > kDeepStackMax && ctx->scratch.builder != 0) {
            const int chosen = ctx->scratch.builder;
            ctx->scratch.builder = 0;
            ctx->scratch.fallbacks++;
            ctx->scratch.fallback_why = "clustered tree needs a traversal stack of " + std::to_string(ctx->stack_need) + " entries";
            const hipError_t be = accel_build(ctx->scratch, ctx->d_buffers.as<BufferRec>(), d_instances, (int)ctx->instances.size(), ctx->n_tris, d_nodes, d_tris,
                                              d_shade, &ctx->root, &ctx->wide_nodes, &ctx->stack_need, ctx->stream);
            ctx->scratch.builder = chosen;
            if (be != hipSuccess) {
                ctx->accel_built = false; ctx->accel_state = ACCEL_REBUILD;
                return ctx->fail(PT_ERR_DEVICE, std::string("acceleration-structure build (radix fallback): ") + (ctx->scratch.why.empty() ? hipGetErrorString(be) : ctx->scratch.why.c_str()));
            }
            HIPOK(hipEventRecord(ctx->ev_accel[1], ctx->stream));
        }
        if (!refit && ctx->stack_need > kDeepStackMax) {
            ctx->accel_built = false; ctx->accel_state = ACCEL_REBUILD;
            return ctx->fail(PT_ERR_CAPACITY, "acceleration structure needs a traversal stack of " + std::to_string(ctx->stack_need) + " entries (limit " +
                                              std::to_string(kDeepStackMax) + ")");
        }
        return PT_OK;
    }

    // Pathtracer::PathtraceScene (Source/Pathtracer.cpp:259-367)
    static int PathtraceScene(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* ep) {
        CameraSetup cam;
        if (!camera_setup(ep, ctx->lens, cam)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "singular camera matrix");
        const float* world_to_clip = cam.world_to_clip;                                  // :262
        bool reset = memcmp(world_to_clip, ctx->previous_world_to_clip, 64) != 0 || settings->reset;   // :267-271
        WavefrontPasses passes;                                                          // the call's optional passes, or why it cannot run them
        if (int r = select_passes(ctx, settings, ep, passes)) return r;
        if (ctx->restart_pending) { reset = true; ctx->restart_pending = false; }        // a pt_set_* since the last trace (pt_ctx.h)
        // The adaptive tile state describes the output only if the last accumulation step was adaptive and of the same size and tile
        // shard: otherwise the call starts a new one.
        if (passes.adaptive && (ep->width != ctx->ad_w || ep->height != ctx->ad_h || ep->tile_rank != ctx->ad_rank ||
                         (ep->tile_rank_count ? ep->tile_rank_count : 1u) != ctx->ad_rank_count || ctx->accumulated_frames != ctx->ad_frames))
            reset = true;
        if (reset) ctx->accumulated_frames = 0;
        // an adaptive accumulation ends where its tiles must stop: min(max_samples, max_accumulated_frames)
        const int frame_cap = passes.adaptive ? std::min(ctx->adaptive.max_samples, settings->max_accumulated_frames) : settings->max_accumulated_frames;
        if (ctx->accumulated_frames < frame_cap) {                                       // :273
            if (ep->light_count > ctx->n_lights) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "light_count exceeds uploaded lights");
            if (ep->environment_map >= 0 && !live_env(ctx, ep->environment_map))
                return ctx->fail(PT_ERR_BAD_HANDLE, "bad environment map handle");
            if (!ep->output) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "output is null");
            if (int r = ensure_accel(ctx)) return r;
            if (passes.bake) { if (int r = bake_setup(ctx, ep->width, ep->height, passes.bk)) return r; }
            if (passes.matte) { if (int r = matte_setup(ctx, passes.mt)) return r; }

            SceneRec sc = scene_fill(ctx);
            if (ep->environment_map >= 0) scene_set_env(sc, *ctx->envs[ep->environment_map]);

            FrameConstants fc;                                                          // :287-331
            camera_constants(cam, ep, fc);
            fc.num_of_lights = ep->light_count;
            fc.seed = settings->use_frame_as_seed ? (uint32_t)ep->frame : settings->seed;   // :316
            fc.accumulated_frames = ctx->accumulated_frames;
            memcpy(fc.environment_color, settings->environment_color, 12);
            fc.environment_intensity = settings->environment_intensity;
            fc.debug_output = settings->debug_output;
            fc.flags = settings->flags;
            fc.max_ray_length = 1000;                                                   // :322 (the setting is ignored)
            auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
            fc.min_bounces = clampi(settings->min_bounces, 0, ctx->bounce_limit);        // :323-324
            fc.max_bounces = clampi(settings->max_bounces, 0, ctx->bounce_limit);
            fc.luminance_clamp = settings->luminance_clamp;
            fc.min_rr = settings->min_russian_roulette_continue_prob;
            fc.max_rr = settings->max_russian_roulette_continue_prob;
            fc.tiles_x = (ep->width + PT_TILE - 1) / PT_TILE;
            fc.tiles_y = (ep->height + PT_TILE - 1) / PT_TILE;
            fc.tile_rank_count = ep->tile_rank_count ? ep->tile_rank_count : 1;
            fc.tile_rank = ep->tile_rank;
            if (fc.tile_rank >= fc.tile_rank_count) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "tile_rank >= tile_rank_count");
            uint32_t ntiles = fc.tiles_x * fc.tiles_y;
            fc.my_tiles = ntiles > fc.tile_rank ? (ntiles - fc.tile_rank + fc.tile_rank_count - 1) / fc.tile_rank_count : 0;

            // Sample batch (pt_set_samples_per_trace): this call stands for `batch` consecutive PathtraceScene calls of frames
            // frame .. frame + batch - 1 with an unchanged camera.  Only accumulation makes more than the last one observable,
            // and the batch may not run past max_accumulated_frames (the calls beyond it would have been no-ops, :273).
            int batch = 1;
            if ((settings->flags & PT_FLAG_ACCUMULATE) && settings->debug_output == PT_DEBUG_OUTPUT_NONE) {
                batch = ctx->samples_per_trace;
                const long long room = (long long)frame_cap - ctx->accumulated_frames;
                if ((long long)batch > room) batch = (int)room;
            }
            fc.cull_null_shadow = ctx->cull_null_shadow ? 1u : 0u;
            fc.defer_rare = 0;                     // (unused member, pt_types.h)
            fc.spp = 1; fc.pixel_slots = fc.my_tiles * 256u;
            fc.div_pixel_slots = FastDiv::make(fc.pixel_slots); fc.div_tiles_x = FastDiv::make(fc.tiles_x);
            fc.seed_step = settings->use_frame_as_seed ? 1u : 0u;

            // workgroups of a wavefront stage launch: the caller's (pt_set_kernel_mode), else by the slots of the batch
            const int stage_blocks = ctx->stage_blocks > 0 ? ctx->stage_blocks : stage_blocks_for((size_t)fc.pixel_slots * (size_t)batch);
            // deep traversal stack (trees that need more than the 64 on-chip entries): (need - 64) entries for every lane of the widest
            // traversal launch of this call
            if (const uint32_t entries = deep_stack_entries(ctx)) {
                const size_t lanes = ctx->kernel_mode == PT_MODE_MEGAKERNEL ? (size_t)fc.my_tiles * 256 : traversal_grid_lanes(stage_blocks);
                const size_t need = (size_t)entries * lanes * 4;
                if (const hipError_t e = ctx->d_deep.reserve(ctx->stream, need, need)) return grow_failed(ctx, e, "deep traversal stack: " + std::to_string(need) + " bytes");
                sc.deep_stack = ctx->d_deep.as<int32_t>(); sc.deep_entries = entries; sc.deep_lanes = (uint32_t)lanes;
            }
            HIPOK(hipEventRecord(ctx->ev_trace[0], ctx->stream));
            if (ctx->kernel_mode == PT_MODE_MEGAKERNEL) {
                for (int k = 0; k < batch; k++) {                                        // the megakernel has no batch form: one launch per sample
                    FrameConstants fk = fc;
                    fk.seed = fc.seed + (uint32_t)k * fc.seed_step;
                    fk.accumulated_frames = fc.accumulated_frames + k;
                    launch_megakernel(sc, fk, cam.lens, (float4*)ep->output, ctx->d_counters.as<Counters>(), ctx->counters_enabled, ctx->stream);   // :344-353
                }
            } else {
                fc.spp = (uint32_t)batch;
                if ((unsigned long long)fc.pixel_slots * fc.spp > 0x7fffffffull) return ctx->fail(PT_ERR_CAPACITY, "sample batch too large for this resolution");
                const size_t need = wavefront_workspace_bytes(fc, stage_blocks, passes);
                HIPOK(ctx->d_workspace.reserve(ctx->stream, need, need));
                if (passes.adaptive) { if (int r = adaptive_setup(ctx, ep, fc, frame_cap, passes.ad)) return r; }
                if (passes.motion) motion_setup(ctx, world_to_clip, ep, passes.mo);
                HIPOK(launch_wavefront(sc, fc, cam.lens, (float4*)ep->output, ctx->d_counters.as<Counters>(), ctx->counters_enabled, ctx->d_workspace.ptr, stage_blocks,
                                       ctx->stage_timing ? &ctx->timers : nullptr, ctx->stream, passes));
            }
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(ctx->ev_trace[1], ctx->stream));
            ctx->have_trace = true;
            if (settings->flags & PT_FLAG_ACCUMULATE) ctx->accumulated_frames += batch;   // :355-359
            else ctx->accumulated_frames = 0;
            ctx->ad_frames = passes.adaptive ? ctx->accumulated_frames : -1;
        }
        memcpy(ctx->previous_world_to_clip, world_to_clip, 64);                          // :366
        return PT_OK;
    }
};

// class GpuSkin (Source/GpuSkin.h:9-37)
class GpuSkin {
public:
    static int Run(pt_ctx* ctx, const pt_skin_params* p, const pt_bone* bones, int bone_count) {      // GpuSkin.cpp:57-118
        auto buf = [&](int h, int fmt, size_t count, const void** out) -> bool {
            if (h < 0 || h >= (int)ctx->buffers.size()) return false;
            const BufferRec& b = ctx->buffers[h];
            if ((int)b.format != fmt || b.bytes < count * format_stride(fmt)) return false;
            *out = b.ptr;
            return true;
        };
        SkinArgs a;
        memset(&a, 0, sizeof(a));
        a.num_of_vertices = p->num_of_vertices;
        a.input_mesh_flags = p->input_mesh_flags;
        a.output_mesh_flags = p->output_mesh_flags;
        a.num_of_morph_targets = p->num_of_morph_targets < PT_MAX_SIMULTANEOUS_MORPH_TARGETS ? p->num_of_morph_targets : PT_MAX_SIMULTANEOUS_MORPH_TARGETS;
        if (a.num_of_morph_targets < 0) a.num_of_morph_targets = 0;
        // If no bones are supplied, `input_mesh_flags &= !FLAG_JOINT_WEIGHT` clears ALL input flags (quirk q19, GpuSkin.cpp:94)
        if (!bones || bone_count <= 0) a.input_mesh_flags &= (uint32_t)!PT_MESH_FLAG_JOINT_WEIGHT;
        const void* ptr = nullptr;
        if (!buf(p->input_position, PT_FORMAT_R32G32B32_FLOAT, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: input_position");
        a.in_position = (const float*)ptr;
        if (a.input_mesh_flags & PT_MESH_FLAG_TANGENT_SPACE) {
            if (!buf(p->input_tangent_space, PT_FORMAT_R10G10B10A2_UNORM, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: input_tangent_space");
            a.in_tangent_space = (const uint32_t*)ptr;
        }
        if (a.input_mesh_flags & PT_MESH_FLAG_JOINT_WEIGHT) {
            if (!buf(p->input_joint_weight, PT_FORMAT_JOINT_WEIGHT, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: input_joint_weight");
            a.in_joint_weight = (const uint4*)ptr;
        }
        if (a.output_mesh_flags & PT_DYNAMIC_MESH_FLAG_POSITION) {
            if (!buf(p->output_position, PT_FORMAT_R32G32B32_FLOAT, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: output_position");
            a.out_position = (float*)ptr;
        }
        if (a.output_mesh_flags & PT_DYNAMIC_MESH_FLAG_TANGENT_SPACE) {
            if (!buf(p->output_tangent_space, PT_FORMAT_R10G10B10A2_UNORM, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: output_tangent_space");
            a.out_tangent_space = (uint32_t*)ptr;
        }
        for (int i = 0; i < a.num_of_morph_targets; i++) {
            a.morph_weight[i] = p->morph_weights[i];
            if (p->morph_position[i] != -1) {
                if (!buf(p->morph_position[i], PT_FORMAT_R32G32B32_FLOAT, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: morph_position");
                a.morph_position[i] = (const float*)ptr;
            }
            if (p->morph_tangent_space[i] != -1) {
                if (!buf(p->morph_tangent_space[i], PT_FORMAT_R10G10B10A2_UNORM, p->num_of_vertices, &ptr)) return ctx->fail(PT_ERR_BAD_HANDLE, "skin: morph_tangent_space");
                a.morph_tangent_space[i] = (const uint32_t*)ptr;
            }
        }
        if (a.input_mesh_flags & PT_MESH_FLAG_JOINT_WEIGHT) {
            size_t bytes = (size_t)bone_count * sizeof(pt_bone);
            // Each call gets its own slice of the bone arena: a frame skins several primitives back to back on one stream, and the
            // kernel of the previous call may not have read its bones yet (they live in the caller's transient heap, Renderer.cpp:411).
            if (ctx->bones_used + bytes > ctx->d_bones.cap) {
                if (bytes > ctx->d_bones.cap) HIPOK(ctx->d_bones.realloc(ctx->stream, bytes * 8 + 4096));
                else if (ctx->bones_fence_pending) HIPOK(hipEventSynchronize(ctx->bones_fence));      // wrap: the arena's earlier readers must be done
                ctx->bones_used = 0;
            }
            void* dst = ctx->d_bones.as<char>() + ctx->bones_used;
            ctx->bones_used += (bytes + 255) & ~(size_t)255;
            HIPOK(staged_upload(ctx, dst, bones, bytes));
            a.bones = (const pt_bone*)dst;
            a.bone_count = bone_count;
        }
        // k_skin_mfma multiplies every bone into every vertex (weight 0 where the vertex does not list it), and 0 * NaN = NaN: one non-finite
        // bone -- the inverse_transpose of a joint scaled to zero is all NaN -- would reach every vertex of the mesh.  Such a call takes k_skin,
        // which like the shader reads only the four bones a vertex lists.  The bones are still on the host here: 32 floats each.
        bool use_mfma = p->use_mfma != 0;
        if (use_mfma && a.bones) {
            const float* f = (const float*)bones;
            for (size_t i = 0, n = (size_t)bone_count * 32; i < n; i++) if (!std::isfinite(f[i])) { use_mfma = false; break; }
        }
        HIPOK(hipEventRecord(ctx->ev_skin[0], ctx->stream));
        launch_skin(a, use_mfma, ctx->stream);
        HIPOK(hipGetLastError());
        HIPOK(hipEventRecord(ctx->ev_skin[1], ctx->stream));
        if (a.bones) { HIPOK(hipEventRecord(ctx->bones_fence, ctx->stream)); ctx->bones_fence_pending = true; }
        ctx->have_skin = true;
        // UpdateAllBlas refits every dynamic primitive every frame (Pathtracer.cpp:168-183): the instances that read the streams
        // just written are refitted by the next pt_build_accel / pt_trace
        if (a.out_position) mark_buffer_users(ctx, p->output_position);
        if (a.out_tangent_space) mark_buffer_users(ctx, p->output_tangent_space);
        return PT_OK;
    }
};
int select_passes(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* ep, WavefrontPasses& p) {
    const bool plain = settings->debug_output == PT_DEBUG_OUTPUT_NONE, megakernel = ctx->kernel_mode == PT_MODE_MEGAKERNEL;
    // Adaptive sampling (pt_set_adaptive) applies to accumulating calls without a debug output.
    p.adaptive = ctx->adaptive.enable != 0 && (settings->flags & PT_FLAG_ACCUMULATE) && plain;
    if (p.adaptive && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "adaptive sampling runs in the wavefront mode only");
    // First-hit AOVs (pt_set_aov) are written by every call without a debug output, under the output's counts and resets.
    p.aov = ctx->aov.enable != 0 && plain;
    if (p.aov && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "AOVs are written in the wavefront mode only");
    // Texture-space baking (pt_set_bake): the generate stage starts the paths on the atlas's texels; everything else is PathtraceScene as it is.
    p.bake = ctx->bake.enable != 0;
    if (p.bake && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "a bake runs in the wavefront mode only");
    if (p.bake && ctx->bake.instance >= (int)ctx->instances.size())
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "bake: instance " + std::to_string(ctx->bake.instance) + " of " + std::to_string(ctx->instances.size()));
    // Light-probe baking (pt_set_probes): likewise, the paths start at the probes' positions and width x height is the probes' atlas.
    p.probes = ctx->probes.enable != 0;
    if (p.probes && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes are traced in the wavefront mode only");
    if (p.probes) {
        uint64_t pw, ph;
        probe_atlas_size(ctx->probes, pw, ph);
        if (ep->width != pw || ep->height != ph)
            return ctx->fail(PT_ERR_INVALID_ARGUMENT, "probes: the atlas is " + std::to_string(pw) + " x " + std::to_string(ph) + ", not " + std::to_string(ep->width) + " x " + std::to_string(ep->height));
    }
    // ID mattes (pt_set_matte) are written, like the AOVs, by every call without a debug output, under the output's counts and resets.
    p.matte = ctx->matte.enable != 0 && plain;
    if (p.matte && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "mattes are written in the wavefront mode only");
    // Motion vectors (pt_set_motion) likewise; they describe camera rays, so not under a bake or probes.
    p.motion = ctx->motion.enable != 0 && plain;
    if (p.motion && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion vectors are written in the wavefront mode only");
    if (p.motion && (p.bake || p.probes)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "motion vectors describe camera rays: not under a bake or probes");
    // The variance AOV (pt_set_variance) likewise; it follows the output, so it works under a bake or probes as for any image.
    p.variance = ctx->variance.enable != 0 && plain;
    if (p.variance && megakernel) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "the variance is written in the wavefront mode only");
    if (p.aov) p.av = {nullptr, nullptr, (float4*)ctx->aov.albedo, (float4*)ctx->aov.normal_depth};
    if (p.variance) p.va = {(float4*)ctx->variance.variance};
    if (p.probes) p.pa = probe_args(ctx);
    return PT_OK;
}
int adaptive_setup(pt_ctx* ctx, const pt_execute_params* ep, const FrameConstants& fc, int frame_cap, AdaptiveArgs& ad) {
    // tile state (rank-local tiles) and half buffer; a new accumulation makes every tile active with 0 samples
    const size_t px = (size_t)ep->width * ep->height, tiles = fc.my_tiles ? fc.my_tiles : 1;
    if (int r = adaptive_state(ctx, tiles, px)) return r;
    if (ctx->accumulated_frames == 0) {
        const AdaptiveTile fresh = {1u, 0u, 0.0f, 0u};
        const std::vector<AdaptiveTile> init(tiles, fresh);
        HIPOK(staged_upload(ctx, ctx->d_ad_tiles.ptr, init.data(), tiles * sizeof(AdaptiveTile)));
        HIPOK(hipMemsetAsync(ctx->d_ad_half.ptr, 0, px * 16, ctx->stream));
    }
    ad.tiles = ctx->d_ad_tiles.as<AdaptiveTile>(); ad.half = ctx->d_ad_half.as<float4>();
    ad.min_samples = ctx->adaptive.min_samples; ad.cap = frame_cap; ad.threshold = ctx->adaptive.threshold;
    ctx->ad_w = ep->width; ctx->ad_h = ep->height; ctx->ad_rank = fc.tile_rank; ctx->ad_rank_count = fc.tile_rank_count;
    ctx->ad_my_tiles = fc.my_tiles; ctx->ad_ready = true;
    return PT_OK;
}
int ensure_accel(pt_ctx* ctx) {
    return ctx->accel_state != ACCEL_CLEAN || !ctx->accel_built || ctx->instances_dirty ? Pathtracer::BuildAccel(ctx) : PT_OK;
}
}  // namespace pt

static int exchange_frame_checked(pt_ctx* ctx, const void* local, void* frame, uint32_t w, uint32_t h, int mode, int dst, std::string& err) {
    // (rank / world live in the exchange state; the root needs somewhere to put the frame)
    return exchange_frame(ctx->exchange, local, frame ? frame : const_cast<void*>(local), w, h, mode, dst, ctx->stream, err);
}

// =================================================================================================
// C-ABI
extern "C" {

int pt_abi_version(void) { return MIPT_ABI_VERSION; }

int pt_create(int device, void* hip_stream, const float* sheen_e_16x16, pt_ctx** out) {
    if (!out || !sheen_e_16x16) return PT_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return PT_ERR_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return PT_ERR_DEVICE;
    pt_ctx* ctx = new pt_ctx();
    ctx->device = device;
    ctx->stream = (hipStream_t)hip_stream;
    float srgb[256];
    for (int i = 0; i < 256; i++) {
        double c = i / 255.0;
        srgb[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
    // The fills go on the context's stream, where the kernels that read or overwrite this memory run: hipMemset on the null stream need
    // not be done when it returns, and a non-blocking stream does not wait for the null stream.  (The copies are from pageable memory:
    // done when hipMemcpy returns.)
    bool ok = ctx->d_sheen.realloc(ctx->stream, 256 * 4) == hipSuccess && ctx->d_srgb.realloc(ctx->stream, 256 * 4) == hipSuccess &&
              ctx->d_counters.realloc(ctx->stream, sizeof(Counters)) == hipSuccess && ctx->d_white.realloc(ctx->stream, 16) == hipSuccess &&
              hipMemsetAsync(ctx->d_white.ptr, 0xff, 16, ctx->stream) == hipSuccess &&
              hipMemcpy(ctx->d_sheen.ptr, sheen_e_16x16, 256 * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(ctx->d_srgb.ptr, srgb, 256 * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemsetAsync(ctx->d_counters.ptr, 0, sizeof(Counters), ctx->stream) == hipSuccess &&
              ctx->d_tangent_lut.realloc(ctx->stream, 1024 * sizeof(float2)) == hipSuccess &&
              build_tangent_lut(ctx->d_tangent_lut.as<float2>(), ctx->stream) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++)
        ok = hipEventCreate(&ctx->ev_trace[i]) == hipSuccess && hipEventCreate(&ctx->ev_accel[i]) == hipSuccess && hipEventCreate(&ctx->ev_skin[i]) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->bones_fence, hipEventDisableTiming) == hipSuccess;
    if (!ok) { pt_destroy(ctx); return PT_ERR_DEVICE; }
    ctx->samplers.push_back({PT_ADDRESS_WRAP, PT_ADDRESS_WRAP, PT_FILTER_LINEAR, PT_FILTER_LINEAR});   // sampler 0 (GpuResources.cpp:47-59)
    if (const char* b = getenv("MIPT_ACCEL_BUILDER")) {      // initial builder of new contexts (pt_set_accel_builder overrides): "lbvh" | "ploc" | "reinsert"
        if (!strcmp(b, "ploc")) ctx->scratch.builder = PT_BUILDER_PLOC;
        else if (!strcmp(b, "lbvh")) ctx->scratch.builder = PT_BUILDER_LBVH;
        else if (!strcmp(b, "reinsert")) ctx->scratch.builder = PT_BUILDER_PLOC_REINSERT;
    }
    if (const char* b = getenv("MIPT_REINSERT_PASSES")) {    // tuning aid (tools/builder_probe.py): passes of PT_BUILDER_PLOC_REINSERT
        const int v = atoi(b);
        if (v >= 0 && v <= 64) ctx->scratch.reinsert_passes = v;
    }
    if (const char* b = getenv("MIPT_REINSERT_MIN_GAIN")) {
        const float v = (float)atof(b);
        if (v >= 0.0f && v < 1.0f) ctx->scratch.reinsert_min_gain = v;
    }
    *out = ctx;
    return PT_OK;
}

void pt_destroy(pt_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (auto& b : ctx->buffers) hipFree((void*)b.ptr);
    for (auto& t : ctx->textures) hipFree((void*)t.texels);
    for (auto& t : ctx->trios) hipFree((void*)t.ptr);
    for (auto* e : ctx->envs) if (e) { env_free(*e); delete e; }
    accel_scratch_free(ctx->scratch);
    exchange_free(ctx->exchange);
    for (int k = 0; k < StagingRing::kSlots; k++) {
        if (ctx->staging.host[k]) hipHostFree(ctx->staging.host[k]);
        if (ctx->staging.done[k]) hipEventDestroy(ctx->staging.done[k]);
    }
    for (hipEvent_t e : ctx->timers.ev) hipEventDestroy(e);
    if (ctx->bones_fence) hipEventDestroy(ctx->bones_fence);
    for (int i = 0; i < 2; i++) {
        if (ctx->ev_trace[i]) hipEventDestroy(ctx->ev_trace[i]);
        if (ctx->ev_accel[i]) hipEventDestroy(ctx->ev_accel[i]);
        if (ctx->ev_skin[i]) hipEventDestroy(ctx->ev_skin[i]);
    }
    delete ctx;                 // ... and every DevBuf with it: the device is current, the stream drained
}

const char* pt_last_error(const pt_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

int pt_buffer_create(pt_ctx* ctx, const void* host, size_t bytes, int format, int* handle_out) {
    if (!ctx || !handle_out) return PT_ERR_INVALID_ARGUMENT;
    if (format_stride(format) == 0 || bytes == 0 || bytes > 0xffffffffull) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_buffer_create: bad format or size");
    ENTER(ctx);
    void* d = nullptr;
    HIPOK(hipMalloc(&d, bytes + 16));
    hipError_t e = host ? hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) : hipMemsetAsync(d, 0, bytes, ctx->stream);   // (the fill: on the stream of the kernels that write it next)
    if (e) { hipFree(d); return ctx->fail(PT_ERR_DEVICE, std::string("pt_buffer_create: ") + hipGetErrorString(e)); }
    const BufferRec rec = {d, (uint32_t)format, (uint32_t)bytes};
    *handle_out = take_slot(ctx->buffers, ctx->free_buffers, rec);
    ctx->buffers_dirty = true;
    return PT_OK;
}

static bool live_buffer(const pt_ctx* ctx, int h) { return h >= 0 && h < (int)ctx->buffers.size() && ctx->buffers[h].ptr != nullptr; }

int pt_buffer_update(pt_ctx* ctx, int handle, const void* host, size_t bytes) {
    if (!ctx || !host) return PT_ERR_INVALID_ARGUMENT;
    if (!live_buffer(ctx, handle) || bytes > ctx->buffers[handle].bytes) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_buffer_update");
    ENTER(ctx);
    HIPOK(staged_upload(ctx, (void*)ctx->buffers[handle].ptr, host, bytes));
    mark_buffer_users(ctx, handle);
    return PT_OK;
}

int pt_buffer_read(pt_ctx* ctx, int handle, void* host, size_t bytes) {
    if (!ctx || !host) return PT_ERR_INVALID_ARGUMENT;
    if (!live_buffer(ctx, handle) || bytes > ctx->buffers[handle].bytes) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_buffer_read");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    HIPOK(hipMemcpy(host, ctx->buffers[handle].ptr, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Gltf::Unload (Source/Gltf.cpp:123-157) destroys every mesh, texture and dynamic mesh of the old scene before the next is loaded
// (Source/Main.cpp:43-54).  A resource the current instance table / material table still points at cannot go: the host replaces
// those tables first (pt_scene_set_instances / pt_scene_set_materials with the new scene, or with count 0), as upstream's
// per-frame tables are rebuilt from the new scene.
int pt_buffer_destroy(pt_ctx* ctx, int handle) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!live_buffer(ctx, handle)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_buffer_destroy");
    const void* ptr = ctx->buffers[handle].ptr;
    for (const InstanceRec& r : ctx->instances)
        if (reads_buffer(r, ptr))
            return ctx->fail(PT_ERR_NOT_READY, "pt_buffer_destroy: the buffer is used by the current instance table (replace it with pt_scene_set_instances first)");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));                // enqueued kernels (skinning, an earlier trace) may still read or write it
    hipFree((void*)ptr);
    ctx->buffers[handle] = BufferRec{nullptr, 0u, 0u};
    ctx->free_buffers.push_back(handle);
    ctx->buffers_dirty = true;
    return PT_OK;
}

int pt_texture_create(pt_ctx* ctx, const uint8_t* rgba8, int width, int height, int srgb, int* handle_out) {
    if (!ctx || !rgba8 || !handle_out || width <= 0 || height <= 0) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    void* d = nullptr;
    size_t bytes = (size_t)width * height * 4;
    HIPOK(hipMalloc(&d, bytes + 4));                         // (+ 4: the sampler reads the two texels of a row as one 8-byte pair, pt_shading.h texture_taps)
    hipError_t e = hipMemcpy(d, rgba8, bytes, hipMemcpyHostToDevice);
    if (e) { hipFree(d); return ctx->fail(PT_ERR_DEVICE, std::string("pt_texture_create: ") + hipGetErrorString(e)); }
    const TextureRec rec = {(const uint32_t*)d, width, height, srgb ? 1u : 0u, 0u};
    *handle_out = take_slot(ctx->textures, ctx->free_textures, rec);
    return PT_OK;
}

int pt_texture_destroy(pt_ctx* ctx, int handle) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (handle < 0 || handle >= (int)ctx->textures.size() || !ctx->textures[handle].texels) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_texture_destroy");
    for (const RMat& m : ctx->rmats_host)
        for (int k = 0; k < SLOT_COUNT; k++)
            if (m.tex[k].texels == ctx->textures[handle].texels)
                return ctx->fail(PT_ERR_NOT_READY, "pt_texture_destroy: the texture is used by the current material table (replace it with pt_scene_set_materials first)");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    hipFree((void*)ctx->textures[handle].texels);
    ctx->textures[handle] = TextureRec{nullptr, 0, 0, 0u, 0u};
    ctx->free_textures.push_back(handle);
    return PT_OK;
}

int pt_sampler_create(pt_ctx* ctx, const pt_sampler_desc* d, int* handle_out) {
    if (!ctx || !d || !handle_out) return PT_ERR_INVALID_ARGUMENT;
    if (d->address_u < 0 || d->address_u > 2 || d->address_v < 0 || d->address_v > 2) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_sampler_create: address mode");
    ctx->samplers.push_back({d->address_u, d->address_v, d->min_filter, d->mag_filter});
    *handle_out = (int)ctx->samplers.size() - 1;
    return PT_OK;
}

// {albedo, normal, metal-rough, -} per texel from the three RGBA8 images of one size (an unbound one reads as white, like d_white)
__global__ void k_trio_interleave(uint4* __restrict__ dst, const uint32_t* __restrict__ a, const uint32_t* __restrict__ n, const uint32_t* __restrict__ m,
                                  const uint32_t* __restrict__ e, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = make_uint4(a[i], n ? n[i] : 0xffffffffu, m ? m[i] : 0xffffffffu, e ? e[i] : 0xffffffffu);
}

int pt_scene_set_materials(pt_ctx* ctx, const pt_material* m, int count) {
    if (!ctx || (count > 0 && !m) || count < 0) return PT_ERR_INVALID_ARGUMENT;
    // the instance table's material ids index this table: a shorter table must not leave one dangling (device reads of rmats[] and
    // of the LDS material cache are not bounds-checked)
    for (const InstanceRec& r : ctx->instances)
        if (r.gpu.material_id >= count)
            return ctx->fail(PT_ERR_BAD_HANDLE, "pt_scene_set_materials: the current instance table uses material " + std::to_string(r.gpu.material_id) +
                                                ", the new table has " + std::to_string(count) + " (replace the instances first)");
    ENTER(ctx);
    for (int i = 0; i < count; i++) {
        for (auto* s : material_slots(m[i])) {
            if (s->descriptor < -1 || s->descriptor >= (int)ctx->textures.size() || (s->descriptor >= 0 && !ctx->textures[s->descriptor].texels))
                return ctx->fail(PT_ERR_BAD_HANDLE, "material texture descriptor out of range or destroyed");
            if (s->sampler < 0 || s->sampler >= (int)ctx->samplers.size()) return ctx->fail(PT_ERR_BAD_HANDLE, "material sampler out of range");
        }
    }
    // Resolve every material into the kernel-side record (pt_types.h RMat): descriptor/sampler indices become pointers and
    // packed flags, the UV transform T*(R*S) (Material.hlsli:68-88) is multiplied out once in fp32.
    std::vector<RMat> rm((size_t)count);
    for (int i = 0; i < count; i++) {
        const pt_material& s = m[i];
        RMat& r = rm[i];
        memset(&r, 0, sizeof(r));
        r.flags = s.flags; r.alpha_mode = s.alpha_mode; r.metalness_factor = s.metalness_factor; r.roughness_factor = s.roughness_factor;
        memcpy(r.base_color_factor, s.base_color_factor, 16);
        memcpy(r.emissive_factor, s.emissive_factor, 12); r.alpha_cutoff = s.alpha_cutoff;
        r.ior = s.ior; r.normal_scale = s.normal_scale; r.specular_factor = s.specular_factor; r.clearcoat_normal_scale = s.clearcoat_normal_scale;
        memcpy(r.specular_color_factor, s.specular_color_factor, 12); r.clearcoat_factor = s.clearcoat_factor;
        r.clearcoat_roughness_factor = s.clearcoat_roughness_factor; r.anisotropy_strength = s.anisotropy_strength;
        r.anisotropy_cos = (float)cos((double)s.anisotropy_rotation); r.anisotropy_sin = (float)sin((double)s.anisotropy_rotation);   // correctly rounded, like the kernels' (pt_math.h pt_sincos)
        memcpy(r.sheen_color_factor, s.sheen_color_factor, 12); r.sheen_roughness_factor = s.sheen_roughness_factor;
        r.transmission_factor = s.transmission_factor;
        const auto slots = material_slots(s);
        for (int k = 0; k < SLOT_COUNT; k++) {
            const pt_texture_sample& a = *slots[k];
            RTex& t = r.tex[k];
            if (a.descriptor == -1) {                     // unbound: a 1x1 white texel keeps the batched fetch branch-free
                t.texels = ctx->d_white.as<uint32_t>(); t.width = 1; t.height = 1; t.flags = RT_POINT;
                t.m00 = 0; t.m01 = 0; t.ox = 0; t.m10 = 0; t.m11 = 0; t.oy = 0;
                continue;
            }
            const TextureRec& tx = ctx->textures[a.descriptor];
            const SamplerRec& sm = ctx->samplers[a.sampler];
            float sn = 0.0f, cs = 1.0f;                   // sin(0) = 0, cos(0) = 1 exactly
            if (a.rotation != 0.0f) { sn = (float)sin((double)a.rotation); cs = (float)cos((double)a.rotation); }
            t.texels = tx.texels; t.width = tx.width; t.height = tx.height;
            t.flags = (tx.srgb ? RT_SRGB : 0u) | ((uint32_t)sm.address_u << 1) | ((uint32_t)sm.address_v << 3) |
                      (sm.mag_filter == PT_FILTER_POINT ? RT_POINT : 0u) | ((a.tex_coord & 1) ? RT_TEXCOORD1 : 0u);
            t.m00 = cs * a.scale[0]; t.m01 = sn * a.scale[1]; t.ox = a.offset[0];
            t.m10 = -sn * a.scale[0]; t.m11 = cs * a.scale[1]; t.oy = a.offset[1];
            r.bound_mask |= 1u << k;
        }
    }
    // Interleaved footprint (RM_TRIO): the albedo texture plus whichever of the normal and metal-rough textures are bound, when they
    // have its size, sampler state, UV set and UV transform -- the three bilinear footprints are then the same four texels, and the
    // shade stage reads them from one 16-B-a-texel copy (two cache lines a hit instead of six).  Same texels, same weights: images are
    // bit-identical either way (MIPT_TEXTURE_INTERLEAVE=0 keeps every material on the general path; tested).
    const char* env_trio = getenv("MIPT_TEXTURE_INTERLEAVE");
    const bool use_trio = !(env_trio && env_trio[0] == '0');
    std::vector<char> trio_live(ctx->trios.size(), 0);
    for (int i = 0; i < count && use_trio; i++) {
        RMat& r = rm[i];
        const RTex& A = r.tex[SLOT_ALBEDO];
        const RTex& N = r.tex[SLOT_NORMAL];
        const RTex& M = r.tex[SLOT_METALLIC_ROUGHNESS];
        const RTex& E = r.tex[SLOT_EMISSIVE];
        const bool ba = (r.bound_mask >> SLOT_ALBEDO) & 1u, bn = (r.bound_mask >> SLOT_NORMAL) & 1u, bm = (r.bound_mask >> SLOT_METALLIC_ROUGHNESS) & 1u;
        auto same_footprint = [&](const RTex& t) {
            return t.width == A.width && t.height == A.height && ((t.flags ^ A.flags) & ~(uint32_t)RT_SRGB) == 0 && memcmp(&t.m00, &A.m00, 6 * sizeof(float)) == 0;
        };
        // the emissive texture joins when it has the footprint (it is fetched on its own otherwise); it does not make a copy worth building alone
        const bool be = ((r.bound_mask >> SLOT_EMISSIVE) & 1u) && same_footprint(E);
        if (!ba || !(bn || bm) || (bn && !same_footprint(N)) || (bm && !same_footprint(M))) continue;
        const uint32_t* kn = bn ? N.texels : nullptr;
        const uint32_t* km = bm ? M.texels : nullptr;
        const uint32_t* ke = be ? E.texels : nullptr;
        size_t at = ctx->trios.size();
        for (size_t k = 0; k < ctx->trios.size(); k++)
            if (ctx->trios[k].a == A.texels && ctx->trios[k].n == kn && ctx->trios[k].m == km && ctx->trios[k].e == ke) { at = k; break; }
        if (at == ctx->trios.size()) {
            const size_t texels = (size_t)A.width * A.height;
            uint4* d = nullptr;
            if (hipMalloc((void**)&d, texels * 16 + 32) != hipSuccess) { (void)hipGetLastError(); continue; }     // no room: this material stays on the general path
            hipLaunchKernelGGL(k_trio_interleave, dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, ctx->stream, d, A.texels, kn, km, ke, texels);
            HIPOK(hipMemsetAsync((char*)d + texels * 16, 0xff, 32, ctx->stream));
            ctx->trios.push_back({A.texels, kn, km, ke, d});
            trio_live.push_back(0);
        }
        trio_live[at] = 1;
        r.trio = ctx->trios[at].ptr;
        r.bound_mask |= RM_TRIO | ((bn && (N.flags & RT_SRGB)) ? RM_TRIO_SRGB_N : 0u) | ((bm && (M.flags & RT_SRGB)) ? RM_TRIO_SRGB_M : 0u) |
                        (be ? (RM_TRIO_EMISSIVE | ((E.flags & RT_SRGB) ? RM_TRIO_SRGB_E : 0u)) : 0u);
    }
    HIPOK(upload_table(ctx, ctx->d_rmats, rm));
    ctx->rmats_host.swap(rm);
    ctx->n_materials = count;
    // copies the new table no longer names: enqueued frames may still read them, so drain the stream first (a scene change, not a per-frame event)
    bool any_dead = false;
    for (char l : trio_live) any_dead |= !l;
    if (any_dead) {
        HIPOK(hipStreamSynchronize(ctx->stream));
        std::vector<pt_ctx::TrioRec> keep;
        for (size_t k = 0; k < ctx->trios.size(); k++) { if (trio_live[k]) keep.push_back(ctx->trios[k]); else hipFree((void*)ctx->trios[k].ptr); }
        ctx->trios.swap(keep);
    }
    return PT_OK;
}

int pt_scene_set_lights(pt_ctx* ctx, const pt_light* l, int count) {
    if (!ctx || (count > 0 && !l) || count < 0) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    std::vector<pt_light> h(l, l + count);
    HIPOK(upload_table(ctx, ctx->d_lights, h));
    ctx->n_lights = count;
    return PT_OK;
}

int pt_scene_set_instances(pt_ctx* ctx, const pt_instance_desc* in, int count) {
    if (!ctx || (count > 0 && !in) || count < 0) return PT_ERR_INVALID_ARGUMENT;
    if (count > PT_MAX_TLAS_INSTANCES) return ctx->fail(PT_ERR_CAPACITY, "more than PT_MAX_TLAS_INSTANCES instances");   // RayTracingAccelerationStructure.cpp:294-297
    std::vector<InstanceRec> recs;
    uint64_t tris = 0;
    auto check = [&](int h, int fmt_a, int fmt_b, size_t count_needed) -> bool {
        if (h == -1) return true;
        if (!live_buffer(ctx, h)) return false;
        const BufferRec& b = ctx->buffers[h];
        if ((int)b.format != fmt_a && (int)b.format != fmt_b) return false;
        return b.bytes >= count_needed * format_stride(b.format);
    };
    for (int i = 0; i < count; i++) {
        const pt_instance_desc& d = in[i];
        const pt_mesh_instance& g = d.gpu;
        if (g.position_descriptor == -1 || !check(g.position_descriptor, PT_FORMAT_R32G32B32_FLOAT, PT_FORMAT_R32G32B32_FLOAT, d.num_of_vertices))
            return ctx->fail(PT_ERR_BAD_HANDLE, "instance position stream");
        if (!check(g.index_descriptor, PT_FORMAT_R16_UINT, PT_FORMAT_R32_UINT, d.num_of_indices)) return ctx->fail(PT_ERR_BAD_HANDLE, "instance index stream");
        if (g.index_descriptor == -1 && d.num_of_indices > d.num_of_vertices) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "non-indexed instance: num_of_indices > num_of_vertices");
        if (!check(g.tangent_space_descriptor, PT_FORMAT_R10G10B10A2_UNORM, PT_FORMAT_R10G10B10A2_UNORM, d.num_of_vertices)) return ctx->fail(PT_ERR_BAD_HANDLE, "instance tangent-space stream");
        if (!check(g.texcoord_descriptors[0], PT_FORMAT_R32G32_FLOAT, PT_FORMAT_R32G32_FLOAT, d.num_of_vertices) ||
            !check(g.texcoord_descriptors[1], PT_FORMAT_R32G32_FLOAT, PT_FORMAT_R32G32_FLOAT, d.num_of_vertices))
            return ctx->fail(PT_ERR_BAD_HANDLE, "instance texcoord stream");
        if (!check(g.color_descriptor, PT_FORMAT_R16G16B16A16_UNORM, PT_FORMAT_R16G16B16A16_UNORM, d.num_of_vertices)) return ctx->fail(PT_ERR_BAD_HANDLE, "instance colour stream");
        if (g.material_id < 0 || g.material_id >= ctx->n_materials) return ctx->fail(PT_ERR_BAD_HANDLE, "instance material_id out of range (set materials first)");
        InstanceRec r;
        memset(&r, 0, sizeof(r));
        r.gpu = g;
        const float* M = g.transform;
        double det = (double)M[0] * ((double)M[5] * M[10] - (double)M[9] * M[6]) - (double)M[4] * ((double)M[1] * M[10] - (double)M[9] * M[2]) +
                     (double)M[8] * ((double)M[1] * M[6] - (double)M[5] * M[2]);
        r.mask_flags = (d.instance_mask & 0xffu) | ((d.instance_flags & PT_INSTANCE_FLAG_TRIANGLE_CULL_DISABLE) ? TF_CULL_DISABLE : 0u) |
                       ((d.instance_flags & PT_INSTANCE_FLAG_FORCE_NON_OPAQUE) ? TF_FORCE_NON_OPAQUE : 0u) | (det < 0 ? TF_MIRRORED : 0u);
        auto ptr_of = [&](int h) -> const void* { return h == -1 ? nullptr : ctx->buffers[h].ptr; };
        r.p_index = ptr_of(g.index_descriptor);
        r.index_is16 = g.index_descriptor != -1 && ctx->buffers[g.index_descriptor].format == PT_FORMAT_R16_UINT;
        r.p_position = (const float*)ptr_of(g.position_descriptor);
        r.p_tangent_space = (const uint32_t*)ptr_of(g.tangent_space_descriptor);
        r.p_texcoord[0] = (const float2*)ptr_of(g.texcoord_descriptors[0]);
        r.p_texcoord[1] = (const float2*)ptr_of(g.texcoord_descriptors[1]);
        r.p_color = (const uint2*)ptr_of(g.color_descriptor);
        r.tri_offset = (uint32_t)tris;
        r.tri_count = d.num_of_indices / 3;
        tris += r.tri_count;
        if (tris > 0x0fffffffull) return ctx->fail(PT_ERR_CAPACITY, "too many triangles (leaf references hold 28 bits of triangle index)");
        recs.push_back(r);
    }
    // What the new table asks of the acceleration structure (the reference rebuilds its TLAS every frame, Pathtracer.cpp:282, which
    // makes a moved instance free; here instances are flattened into one tree):
    //   identical table            -> nothing (gs_frame re-sends the table every frame, also for a static scene);
    //   same triangles, rows differ -> refit of the rows that differ (transform, flags, streams re-pointed at same-sized buffers);
    //   anything else              -> full build.
    const std::vector<InstanceRec>& old = ctx->instances;
    bool same_shape = ctx->accel_built && old.size() == recs.size() && ctx->n_tris == (uint32_t)tris;
    for (size_t i = 0; same_shape && i < recs.size(); i++)
        same_shape = old[i].tri_count == recs[i].tri_count && old[i].tri_offset == recs[i].tri_offset;
    if (same_shape) {
        if (ctx->touched.size() != recs.size()) ctx->touched.assign(recs.size(), 0);
        bool any = false;
        for (size_t i = 0; i < recs.size(); i++) {
            if (memcmp(&old[i], &recs[i], sizeof(InstanceRec)) == 0) continue;
            any = true;
            // a row that differs only in its material id leaves every packet as it is (the packets name the instance, not the material)
            InstanceRec a = old[i], b = recs[i];
            a.gpu.material_id = b.gpu.material_id = 0;
            if (memcmp(&a, &b, sizeof(InstanceRec)) != 0) ctx->touched[i] = 1;
        }
        if (!any) return PT_OK;
        bool refit = false;
        for (uint8_t t : ctx->touched) refit = refit || t != 0;
        if (refit && ctx->accel_state == ACCEL_CLEAN) ctx->accel_state = ACCEL_REFIT;
    } else {
        ctx->accel_state = ACCEL_REBUILD;
        ctx->touched.assign(recs.size(), 0);
    }
    ctx->instances.swap(recs);
    ctx->instances_dirty = true;
    ctx->n_tris = (uint32_t)tris;
    return PT_OK;
}

int pt_env_create(pt_ctx* ctx, const float* rgb, int width, int height, int* env_out) {
    if (!ctx || !rgb || !env_out || width <= 0 || height <= 0) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    float* d = nullptr;
    size_t bytes = (size_t)width * height * 12;
    HIPOK(hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemcpy(d, rgb, bytes, hipMemcpyHostToDevice);
    EnvDevice* env = new EnvDevice();
    if (!e) e = env_build(*env, d, width, height, ctx->stream);
    if (!e) e = hipStreamSynchronize(ctx->stream);
    hipFree(d);
    if (e) { env_free(*env); delete env; return ctx->fail(PT_ERR_DEVICE, std::string("pt_env_create: ") + hipGetErrorString(e)); }
    *env_out = take_slot(ctx->envs, ctx->free_envs, env);
    return PT_OK;
}

// EnvironmentMap::Destroy: the maps of one environment (the reference replaces its single environment map in place when a new
// image is loaded, Source/EnvironmentMap.cpp:84-130).
int pt_env_destroy(pt_ctx* ctx, int env) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_env_destroy");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    env_free(*ctx->envs[env]);
    delete ctx->envs[env];
    ctx->envs[env] = nullptr;
    ctx->free_envs.push_back(env);
    return PT_OK;
}

int pt_env_read(pt_ctx* ctx, int env, int* cube_size_out, uint16_t* cube, float* pyramid) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!live_env(ctx, env)) return ctx->fail(PT_ERR_BAD_HANDLE, "pt_env_read");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    const EnvDevice& ed = *ctx->envs[env];
    int n = ed.mip_n[0];
    size_t pyr = 0;
    for (int r = ed.imp_res; r >= 1; r >>= 1) pyr += (size_t)r * r;
    const uint16_t* dc = ed.cube; const float* dp = ed.importance;
    if (cube_size_out) *cube_size_out = n;
    if (cube) HIPOK(hipMemcpy(cube, dc, (size_t)6 * n * n * 4 * 2, hipMemcpyDeviceToHost));
    if (pyramid) HIPOK(hipMemcpy(pyramid, dp, pyr * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_build_accel(pt_ctx* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    return Pathtracer::BuildAccel(ctx);
}

int pt_accel_request_rebuild(pt_ctx* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ctx->accel_state = ACCEL_REBUILD;
    return PT_OK;
}

int pt_set_accel_builder(pt_ctx* ctx, int builder) {
    if (!ctx || builder < PT_BUILDER_LBVH || builder > PT_BUILDER_PLOC_REINSERT) return PT_ERR_INVALID_ARGUMENT;
    if (ctx->scratch.builder != builder) { ctx->scratch.builder = builder; ctx->accel_state = ACCEL_REBUILD; }
    return PT_OK;
}

int pt_skin_run(pt_ctx* ctx, const pt_skin_params* params, const pt_bone* bones, int bone_count) {
    if (!ctx || !params) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    return GpuSkin::Run(ctx, params, bones, bone_count);
}

int pt_trace(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params) {
    if (!ctx || !settings || !params) return PT_ERR_INVALID_ARGUMENT;
    if (params->width == 0 || params->height == 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "zero resolution");
    ENTER(ctx);
    return Pathtracer::PathtraceScene(ctx, settings, params);
}

int pt_set_bounce_limit(pt_ctx* ctx, int limit) {
    if (!ctx || limit < 0) return PT_ERR_INVALID_ARGUMENT;
    ctx->bounce_limit = limit;
    return PT_OK;
}

int pt_set_samples_per_trace(pt_ctx* ctx, int samples) {
    if (!ctx || samples < 1 || samples > PT_MAX_SAMPLES_PER_TRACE) return PT_ERR_INVALID_ARGUMENT;
    ctx->samples_per_trace = samples;
    return PT_OK;
}

int pt_set_adaptive(pt_ctx* ctx, const pt_adaptive_config* config) {
    if (!ctx || !config) return PT_ERR_INVALID_ARGUMENT;
    if (config->enable) {
        if (config->min_samples < 2) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "adaptive: min_samples < 2");
        if (config->max_samples < config->min_samples) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "adaptive: max_samples < min_samples");
        if (!std::isfinite(config->threshold) || config->threshold < 0.0f) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "adaptive: threshold must be finite and >= 0");
    }
    ctx->adaptive = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_set_aov(pt_ctx* ctx, const pt_aov_config* config) {
    if (!ctx || !config) return PT_ERR_INVALID_ARGUMENT;
    if (config->enable && !config->albedo && !config->normal_depth) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "aov: enabled without a target");
    ctx->aov = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_set_lens(pt_ctx* ctx, const pt_lens_config* config) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!config) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens: config is NULL");
    if (config->enable) {
        if (!std::isfinite(config->aperture_radius) || config->aperture_radius < 0.0f) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens: aperture_radius must be finite and >= 0");
        if (!std::isfinite(config->focus_distance) || config->focus_distance <= 0.0f) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens: focus_distance must be finite and > 0");
        if (config->blades != 0 && (config->blades < 3 || config->blades > kLensMaxBlades)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens: blades must be 0 or 3..16");
        if (!std::isfinite(config->blade_rotation)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens: blade_rotation must be finite");
    }
    ctx->lens = *config;
    ctx->restart_pending = true;
    return PT_OK;
}

int pt_lens_focus_at(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, float px, float py, float* focus_distance_out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!settings || !params || !focus_distance_out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens_focus_at: NULL argument");
    if (params->width == 0 || params->height == 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens_focus_at: zero resolution");
    if (!(px >= 0.0f && px <= (float)params->width && py >= 0.0f && py <= (float)params->height))
        return ctx->fail(PT_ERR_INVALID_ARGUMENT, "lens_focus_at: position outside the image");
    CameraSetup cam;
    if (!camera_setup(params, ctx->lens, cam)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "singular camera matrix");
    ENTER(ctx);
    if (int r = ensure_accel(ctx)) return r;
    SceneRec sc = scene_fill(ctx);
    FrameConstants fc;
    camera_constants(cam, params, fc);
    TempBuf d_out, d_deep;
    if (d_out.alloc(8) != hipSuccess) { (void)hipGetLastError(); return ctx->fail(PT_ERR_OUT_OF_MEMORY, "lens_focus_at: result buffer"); }
    if (int r = temp_deep_stack(ctx, sc, d_deep, 256, "lens_focus_at: deep stack")) return r;
    launch_lens_focus(sc, fc, cam.lens, px, py, (settings->flags & PT_FLAG_CULL_BACKFACE) ? 1u : 0u, d_out.as<float>(), ctx->stream);   // RF_CULL_BACK (RayGeneration :747)
    float res[2] = {0.0f, 0.0f};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_out.ptr, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ctx->fail(PT_ERR_DEVICE, std::string("lens_focus_at: ") + hipGetErrorString(e));
    if (res[0] == 0.0f) return ctx->fail(PT_ERR_NOT_READY, "lens_focus_at: the ray hits nothing");
    *focus_distance_out = res[1];
    return PT_OK;
}

int pt_adaptive_read(pt_ctx* ctx, uint32_t width, uint32_t height, int32_t* active_tiles, uint32_t* tile_samples, float* tile_error, float* half_rgba32f) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->ad_ready) return ctx->fail(PT_ERR_NOT_READY, "no adaptive trace yet");
    if (width != ctx->ad_w || height != ctx->ad_h) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "adaptive_read: size differs from the traced one");
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    std::vector<AdaptiveTile> t(ctx->ad_my_tiles);
    if (!t.empty()) HIPOK(hipMemcpy(t.data(), ctx->d_ad_tiles.ptr, t.size() * sizeof(AdaptiveTile), hipMemcpyDeviceToHost));
    const size_t ntiles = (size_t)((width + PT_TILE - 1) / PT_TILE) * ((height + PT_TILE - 1) / PT_TILE);
    if (tile_samples) memset(tile_samples, 0, ntiles * sizeof(uint32_t));
    if (tile_error) memset(tile_error, 0, ntiles * sizeof(float));
    int32_t active = 0;
    for (size_t l = 0; l < t.size(); l++) {                     // rank-local tile l is global tile rank + l * rank_count
        const size_t g = ctx->ad_rank + l * ctx->ad_rank_count;
        if (g >= ntiles) break;
        if (tile_samples) tile_samples[g] = t[l].samples;
        if (tile_error) tile_error[g] = t[l].error;
        active += t[l].active ? 1 : 0;
    }
    if (active_tiles) *active_tiles = active;
    if (half_rgba32f) HIPOK(hipMemcpy(half_rgba32f, ctx->d_ad_half.ptr, (size_t)width * height * 16, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_set_null_shadow_culling(pt_ctx* ctx, int enable) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ctx->cull_null_shadow = enable != 0;
    return PT_OK;
}

int pt_set_watertight(pt_ctx* ctx, int enable) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (ctx->watertight != (enable != 0)) ctx->restart_pending = true;        // samples of two intersection rules do not share an image
    ctx->watertight = enable != 0;
    return PT_OK;
}

int pt_set_kernel_mode(pt_ctx* ctx, int mode, int stage_blocks) {
    if (!ctx || (mode != PT_MODE_WAVEFRONT && mode != PT_MODE_MEGAKERNEL)) return PT_ERR_INVALID_ARGUMENT;
    ctx->kernel_mode = mode;
    if (stage_blocks > 0) ctx->stage_blocks = stage_blocks;
    return PT_OK;
}

int pt_enable_counters(pt_ctx* ctx, int enable) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ctx->counters_enabled = enable != 0;
    return PT_OK;
}

int pt_enable_stage_timing(pt_ctx* ctx, int enable) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ctx->stage_timing = enable != 0;
    if (!ctx->stage_timing) ctx->timers.used = 0;
    return PT_OK;
}

int pt_reset_stats(pt_ctx* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    HIPOK(hipMemsetAsync(ctx->d_counters.ptr, 0, sizeof(Counters), ctx->stream));
    return PT_OK;
}

int pt_get_stats(pt_ctx* ctx, pt_stats* out) {
    if (!ctx || !out) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    Counters c;
    HIPOK(hipMemcpy(&c, ctx->d_counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->rays_primary = c.rays_primary; out->rays_bounce = c.rays_bounce; out->rays_shadow = c.rays_shadow;
    out->rays = c.rays_primary + c.rays_bounce + c.rays_shadow;
    out->nodes_visited = c.nodes + c.nodes_shadow; out->tris_tested = c.tris + c.tris_shadow; out->closest_hits = c.hits; out->texture_taps = c.taps;
    out->nodes_visited_shadow = c.nodes_shadow; out->tris_tested_shadow = c.tris_shadow;
    if (ctx->have_trace) hipEventElapsedTime(&out->trace_ms, ctx->ev_trace[0], ctx->ev_trace[1]);
    if (ctx->have_accel) hipEventElapsedTime(&out->accel_ms, ctx->ev_accel[0], ctx->ev_accel[1]);
    if (ctx->have_skin) hipEventElapsedTime(&out->skin_ms, ctx->ev_skin[0], ctx->ev_skin[1]);
    for (size_t k = 0; k < ctx->timers.used; k++) {          // per-stage times of the last pt_trace (pt_enable_stage_timing)
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->timers.ev[k], ctx->timers.ev[k + 1]) == hipSuccess) out->stage_ms[ctx->timers.kind[k]] += ms;
    }
    out->accumulated_frames = ctx->accumulated_frames;
    out->bvh_nodes = ctx->wide_nodes;
    out->bvh_triangles = ctx->n_tris;
    out->bvh_stack_need = ctx->stack_need;
    out->bvh_stack_capacity = deep_stack_entries(ctx) + (uint32_t)traversal_stack_capacity();
    out->accel_builder_fallbacks = ctx->scratch.fallbacks;
    out->deep_stack_pushes = c.deep_pushes;
    out->accel_builds = ctx->accel_builds; out->accel_refits = ctx->accel_refits;
    if (c.stack_overflow) return ctx->fail(PT_ERR_CAPACITY, "traversal stack overflow: " + std::to_string(c.stack_overflow) + " pushes dropped");
    return PT_OK;
}

int pt_readback(pt_ctx* ctx, const void* device_rgba32f, uint32_t width, uint32_t height, float* host) {
    if (!ctx || !device_rgba32f || !host) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    HIPOK(hipStreamSynchronize(ctx->stream));
    HIPOK(hipMemcpy(host, device_rgba32f, (size_t)width * height * 16, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_tonemap(pt_ctx* ctx, const pt_tonemap_config* cfg, const void* device_rgba32f, uint32_t width, uint32_t height, float* host_rgb, uint8_t* host_rgba8) {
    if (!ctx || !cfg || !device_rgba32f || width == 0 || height == 0) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    const size_t n = (size_t)width * height, need = n * 16;      // float RGB (12 B) + RGBA8 (4 B) per pixel, kept between calls
    HIPOK(ctx->d_tonemap.reserve(ctx->stream, need, need));
    float* d_rgb = host_rgb ? ctx->d_tonemap.as<float>() : nullptr;
    uint32_t* d_q = host_rgba8 ? (uint32_t*)(ctx->d_tonemap.as<char>() + n * 12) : nullptr;
    launch_tonemap((const float4*)device_rgba32f, width, height, *cfg, d_rgb, d_q, ctx->stream);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(ctx->stream));
    if (host_rgb) HIPOK(hipMemcpy(host_rgb, d_rgb, n * 12, hipMemcpyDeviceToHost));
    if (host_rgba8) HIPOK(hipMemcpy(host_rgba8, d_q, n * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

// ---- saving and resuming an accumulation (host/accum_state.h holds the format and its validator) ----------------------------------
static int accum_scratch(pt_ctx* ctx, size_t need) {
    const hipError_t e = ctx->d_accum.reserve(ctx->stream, need, need);
    return e == hipSuccess ? PT_OK : grow_failed(ctx, e, "accumulation scratch: " + std::to_string(need) + " bytes");
}

int pt_accum_save(pt_ctx* ctx, const pt_accum_images* images, uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count,
                  uint64_t next_frame, void* host_blob, size_t capacity, size_t* bytes_out) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!bytes_out) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_save: bytes_out is null");
    if (!images || !images->output) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_save: images->output is null");
    if (width == 0 || height == 0 || width > accum::kMaxExtent || height > accum::kMaxExtent) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_save: bad size");
    const uint32_t world = tile_rank_count ? tile_rank_count : 1u;
    if (tile_rank >= world) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_save: tile_rank >= tile_rank_count");
    if (ctx->accumulated_frames == 0) return ctx->fail(PT_ERR_NOT_READY, "accum_save: nothing accumulated");
    if (ctx->restart_pending) return ctx->fail(PT_ERR_NOT_READY, "accum_save: pt_set_adaptive / pt_set_aov / pt_set_lens / pt_set_bake / pt_set_probes / pt_set_matte / pt_set_motion since the last trace: the next trace starts anew");
    // the tile state is part of the accumulation under the condition PathtraceScene continues an adaptive one
    const bool adaptive = ctx->adaptive.enable != 0 && ctx->ad_ready && ctx->ad_w == width && ctx->ad_h == height && ctx->ad_rank == tile_rank &&
                          ctx->ad_rank_count == world && ctx->ad_frames == ctx->accumulated_frames;
    pt_accum_info info;
    memset(&info, 0, sizeof(info));
    info.sections = PT_ACCUM_OUTPUT | (images->albedo ? PT_ACCUM_ALBEDO : 0) | (images->normal_depth ? PT_ACCUM_NORMAL_DEPTH : 0) | (adaptive ? PT_ACCUM_ADAPTIVE : 0);
    info.width = width; info.height = height; info.tile_rank = tile_rank; info.tile_rank_count = world;
    info.accumulated_frames = ctx->accumulated_frames;
    info.tiles = tiles_of_rank(width, height, tile_rank, world);
    info.next_frame = next_frame;
    if (adaptive) info.adaptive = ctx->adaptive;
    const accum::Layout l = accum::layout(info.sections, info.tiles);
    info.total_bytes = l.total_bytes;
    *bytes_out = (size_t)l.total_bytes;
    if (!host_blob) return PT_OK;
    if ((uint64_t)capacity < l.total_bytes) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_save: capacity below the " + std::to_string(l.total_bytes) + " bytes needed");
    ENTER(ctx);
    const void* src[4] = {images->output, images->albedo, images->normal_depth, adaptive ? ctx->d_ad_half.ptr : nullptr};
    const uint64_t at[4] = {l.image[0], l.image[1], l.image[2], l.half};
    const size_t P = (size_t)l.packed_bytes;
    int slot[4], slots = 0;                       // one packed image of scratch per section present
    for (int k = 0; k < 4; k++) slot[k] = src[k] ? slots++ : -1;
    if (P) {
        int r = accum_scratch(ctx, slots * P);
        if (r) return r;
        for (int k = 0; k < 4; k++)
            if (src[k]) HIPOK(tiles_pack(src[k], width, height, tile_rank, world, ctx->d_accum.as<char>() + slot[k] * P, ctx->stream));
    }
    HIPOK(hipStreamSynchronize(ctx->stream));
    accum::write_header(host_blob, info, ctx->previous_world_to_clip);
    for (int k = 0; k < 4 && P; k++)
        if (src[k]) HIPOK(hipMemcpy((char*)host_blob + at[k], ctx->d_accum.as<char>() + slot[k] * P, P, hipMemcpyDeviceToHost));
    if (adaptive && info.tiles) {
        static_assert(sizeof(AdaptiveTile) == accum::kRecordBytes, "a tile record is an AdaptiveTile");
        std::vector<AdaptiveTile> t(info.tiles);
        HIPOK(hipMemcpy(t.data(), ctx->d_ad_tiles.ptr, t.size() * sizeof(AdaptiveTile), hipMemcpyDeviceToHost));
        for (AdaptiveTile& x : t) x.pad = 0;
        memcpy((char*)host_blob + l.records, t.data(), t.size() * sizeof(AdaptiveTile));
    }
    accum::seal(host_blob, l.total_bytes);
    return PT_OK;
}

int pt_accum_load(pt_ctx* ctx, const void* host_blob, size_t bytes, const pt_accum_images* targets) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    if (!targets) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: targets is null");
    pt_accum_info info;
    float world_to_clip[16];
    std::string err;
    if (!accum::validate(host_blob, bytes, info, world_to_clip, err)) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: " + err);
    void* dst[3] = {targets->output, targets->albedo, targets->normal_depth};
    static const char* const names[3] = {"output", "albedo", "normal_depth"};
    for (int k = 0; k < 3; k++) {
        const bool section = (info.sections & (1u << k)) != 0;
        if (section && !dst[k]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, std::string("accum_load: the blob holds ") + names[k] + " but no target is given");
        if (!section && dst[k]) return ctx->fail(PT_ERR_INVALID_ARGUMENT, std::string("accum_load: a target for ") + names[k] + " but the blob holds none");
    }
    const bool adaptive = (info.sections & PT_ACCUM_ADAPTIVE) != 0;
    if (adaptive) {
        const pt_adaptive_config& a = ctx->adaptive;
        if (a.enable == 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: adaptive.enable: the blob is an adaptive accumulation, the context has adaptive sampling off");
        if (a.enable != info.adaptive.enable) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: adaptive.enable differs from the context's");
        if (a.min_samples != info.adaptive.min_samples) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: adaptive.min_samples differs from the context's");
        if (a.max_samples != info.adaptive.max_samples) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: adaptive.max_samples differs from the context's");
        if (memcmp(&a.threshold, &info.adaptive.threshold, 4) != 0) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "accum_load: adaptive.threshold differs from the context's");
    }
    if (adaptive && (uint64_t)info.width * info.height > SIZE_MAX / 16) return ctx->fail(PT_ERR_OUT_OF_MEMORY, "accum_load: half buffer of width x height float4");
    ENTER(ctx);
    const accum::Layout l = accum::layout(info.sections, info.tiles);
    const size_t P = (size_t)l.packed_bytes, px = (size_t)info.width * info.height, tiles = info.tiles ? info.tiles : 1;
    void* out[4] = {dst[0], dst[1], dst[2], adaptive ? (void*)1 : nullptr};        // [3]: the half buffer, once it is allocated
    int slot[4], slots = 0;                       // one packed image of scratch per section present
    for (int k = 0; k < 4; k++) slot[k] = out[k] ? slots++ : -1;
    if (P) { int r = accum_scratch(ctx, slots * P); if (r) return r; }
    if (adaptive) { int r = adaptive_state(ctx, tiles, px); if (r) return r; }                     // grown as PathtraceScene grows them
    // every check has passed.  The caller may free the blob on return: its bytes are on the device before that, the unpacking is enqueued.
    const uint64_t at[4] = {l.image[0], l.image[1], l.image[2], l.half};
    out[3] = adaptive ? ctx->d_ad_half.ptr : nullptr;
    for (int k = 0; k < 4 && P; k++)
        if (out[k]) HIPOK(hipMemcpyAsync(ctx->d_accum.as<char>() + slot[k] * P, (const char*)host_blob + at[k], P, hipMemcpyHostToDevice, ctx->stream));
    if (adaptive) {
        if (info.tiles) HIPOK(hipMemcpyAsync(ctx->d_ad_tiles.ptr, (const char*)host_blob + l.records, info.tiles * sizeof(AdaptiveTile), hipMemcpyHostToDevice, ctx->stream));
        HIPOK(hipMemsetAsync(ctx->d_ad_half.ptr, 0, px * 16, ctx->stream));        // other ranks' pixels: as a new accumulation leaves them
    }
    HIPOK(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4 && P; k++)
        if (out[k]) HIPOK(tiles_unpack(ctx->d_accum.as<char>() + slot[k] * P, info.width, info.height, info.tile_rank, info.tile_rank_count, out[k], ctx->stream));
    ctx->accumulated_frames = info.accumulated_frames;
    memcpy(ctx->previous_world_to_clip, world_to_clip, 64);
    if (adaptive) {
        ctx->ad_w = info.width; ctx->ad_h = info.height; ctx->ad_rank = info.tile_rank; ctx->ad_rank_count = info.tile_rank_count;
        ctx->ad_my_tiles = info.tiles; ctx->ad_ready = true;
    }
    ctx->ad_frames = adaptive ? info.accumulated_frames : -1;
    ctx->restart_pending = false;
    return PT_OK;
}

int pt_accum_inspect(const void* host_blob, size_t bytes, pt_accum_info* out) {
    if (!host_blob || !out) return PT_ERR_INVALID_ARGUMENT;
    std::string err;
    pt_accum_info info;
    if (!accum::validate(host_blob, bytes, info, nullptr, err)) return PT_ERR_INVALID_ARGUMENT;
    *out = info;
    return PT_OK;
}

// ---- the per-frame exchange of the tile-sharded renderer (exchange.hip) ------------------------------------------------------
int pt_exchange_unique_id(void* id_out) {
    if (!id_out) return PT_ERR_INVALID_ARGUMENT;
    std::string err;
    return exchange_unique_id(id_out, err);
}

int pt_exchange_create(pt_ctx* ctx, int rank, int world, const void* unique_id) {
    if (!ctx || world < 1 || rank < 0 || rank >= world) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (ctx->exchange) { HIPOK(hipStreamSynchronize(ctx->stream)); exchange_free(ctx->exchange); ctx->exchange = nullptr; }
    std::string err;
    const int rc = exchange_create(&ctx->exchange, rank, world, unique_id, err);
    return rc == PT_OK ? PT_OK : ctx->fail(rc, err);
}

int pt_exchange_probe(void) {
    std::string err;
    return exchange_probe(err);
}

int pt_exchange_create_loopback(pt_ctx* ctx, int rank, int world, uint64_t group) {
    if (!ctx || world < 1 || rank < 0 || rank >= world) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (ctx->exchange) { HIPOK(hipStreamSynchronize(ctx->stream)); exchange_free(ctx->exchange); ctx->exchange = nullptr; }
    std::string err;
    const int rc = exchange_create_loopback(&ctx->exchange, rank, world, group, ctx->device, err);
    return rc == PT_OK ? PT_OK : ctx->fail(rc, err);
}

int pt_exchange_frame(pt_ctx* ctx, const void* local_image, void* frame, uint32_t width, uint32_t height, int mode, int dst_rank) {
    if (!ctx || !local_image || width == 0 || height == 0) return PT_ERR_INVALID_ARGUMENT;
    if (!ctx->exchange) return ctx->fail(PT_ERR_NOT_READY, "pt_exchange_frame: call pt_exchange_create first");
    if (mode != PT_EXCHANGE_GATHER && mode != PT_EXCHANGE_REDUCE) return ctx->fail(PT_ERR_INVALID_ARGUMENT, "pt_exchange_frame: mode");
    ENTER(ctx);
    std::string err;
    const int rc = exchange_frame_checked(ctx, local_image, frame, width, height, mode, dst_rank, err);
    return rc == PT_OK ? PT_OK : ctx->fail(rc, err);
}

int pt_exchange_destroy(pt_ctx* ctx) {
    if (!ctx) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    if (ctx->exchange) { HIPOK(hipStreamSynchronize(ctx->stream)); exchange_free(ctx->exchange); ctx->exchange = nullptr; }
    return PT_OK;
}

size_t pt_tiles_packed_bytes(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count) {
    if (tile_rank_count == 0 || tile_rank >= tile_rank_count) return 0;
    return (size_t)tiles_of_rank(width, height, tile_rank, tile_rank_count) * 256 * 16;
}

int pt_tiles_pack(pt_ctx* ctx, const void* image, uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count, void* packed) {
    if (!ctx || !image || !packed || width == 0 || height == 0 || tile_rank_count == 0 || tile_rank >= tile_rank_count) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    HIPOK(tiles_pack(image, width, height, tile_rank, tile_rank_count, packed, ctx->stream));
    return PT_OK;
}

int pt_tiles_unpack(pt_ctx* ctx, const void* packed, uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count, void* image) {
    if (!ctx || !image || !packed || width == 0 || height == 0 || tile_rank_count == 0 || tile_rank >= tile_rank_count) return PT_ERR_INVALID_ARGUMENT;
    ENTER(ctx);
    HIPOK(tiles_unpack(packed, width, height, tile_rank, tile_rank_count, image, ctx->stream));
    return PT_OK;
}

}  // extern "C"
