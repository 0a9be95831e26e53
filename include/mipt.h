/*
 * mipt.h -- C-ABI of the MI355X-native glTF path tracer (libmipt.so).
 *
 * This is the drop-in boundary for ONE hot path of l-johnson-code/glTF-Renderer: the
 * Pathtracer.cpp render loop (+ GpuSkin, the acceleration structure and the environment map
 * prerequisites it consumes).  The reference has no FFI; its seam is two C++ classes called from
 * Renderer::DrawFrame.  Every entry point below names the reference interface it replaces
 * (file:line relative to the reference root).  D3D12 types cannot cross the boundary, so:
 *   - "descriptors" (ints into ResourceDescriptorHeap[]) become ints into a context-owned
 *     resource table (pt_buffer_create / pt_texture_create / pt_sampler_create);  -1 = absent,
 *     exactly as in GpuMeshInstance (Source/Pathtracer.h:131-140);
 *   - GPU virtual addresses of the per-frame material / light arrays become host pointers that
 *     pt_scene_set_materials / pt_scene_set_lights upload (Source/Renderer.cpp:459-500);
 *   - the output UAV becomes a caller-owned device pointer to W*H RGBA32F texels
 *     (Source/Renderer.cpp:384, Source/Pathtracer.h:98-99).
 * All structs are plain data, byte-identical to the layouts the reference uploads to the GPU
 * (SURVEY.md section 8(a) A1-A6), so scene data drops in unchanged.
 *
 * Conventions: every function returns PT_OK (0) or a negative pt_status; pt_last_error() gives
 * the message.  No exceptions or aborts cross the boundary.  One caller thread per context
 * (as the reference: Source/Renderer.cpp:215-227); what is per context, per thread and process-wide: INTEGRATION.md, "Threads".
 * All device work is enqueued on the HIP stream
 * given to pt_create and is asynchronous unless stated; pt_readback / pt_tonemap / pt_get_stats
 * synchronise that stream.
 */
#ifndef MIPT_H
#define MIPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPT_ABI_VERSION 2

typedef enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID_ARGUMENT = -1,
    PT_ERR_OUT_OF_MEMORY = -2,
    PT_ERR_DEVICE = -3,        /* a HIP call failed; message holds hipGetErrorString */
    PT_ERR_BAD_HANDLE = -4,
    PT_ERR_CAPACITY = -5,      /* > PT_MAX_TLAS_INSTANCES etc. (reference logs and skips) */
    PT_ERR_NOT_READY = -6
} pt_status;

/* ---- Pathtracer::DebugOutput (Source/Pathtracer.h:19-49) -------------------------------- */
enum {
    PT_DEBUG_OUTPUT_NONE = 0,
    PT_DEBUG_OUTPUT_HIT_KIND,
    PT_DEBUG_OUTPUT_VERTEX_COLOR,
    PT_DEBUG_OUTPUT_VERTEX_ALPHA,
    PT_DEBUG_OUTPUT_VERTEX_NORMAL,
    PT_DEBUG_OUTPUT_VERTEX_TANGENT,
    PT_DEBUG_OUTPUT_VERTEX_BITANGENT,
    PT_DEBUG_OUTPUT_TEXCOORD_0,
    PT_DEBUG_OUTPUT_TEXCOORD_1,
    PT_DEBUG_OUTPUT_COLOR,
    PT_DEBUG_OUTPUT_ALPHA,
    PT_DEBUG_OUTPUT_SHADING_NORMAL,
    PT_DEBUG_OUTPUT_SHADING_TANGENT,
    PT_DEBUG_OUTPUT_SHADING_BITANGENT,
    PT_DEBUG_OUTPUT_METALNESS,
    PT_DEBUG_OUTPUT_ROUGHNESS,
    PT_DEBUG_OUTPUT_SPECULAR,
    PT_DEBUG_OUTPUT_SPECULAR_COLOR,
    PT_DEBUG_OUTPUT_CLEARCOAT,
    PT_DEBUG_OUTPUT_CLEARCOAT_ROUGHNESS,
    PT_DEBUG_OUTPUT_CLEARCOAT_NORMAL,
    PT_DEBUG_OUTPUT_TRANSMISSIVE,
    PT_DEBUG_OUTPUT_BOUNCE_DIRECTION,
    PT_DEBUG_OUTPUT_BOUNCE_BSDF,
    PT_DEBUG_OUTPUT_BOUNCE_PDF,
    PT_DEBUG_OUTPUT_BOUNCE_WEIGHT,
    PT_DEBUG_BOUNCE_IS_TRANSMISSION,
    PT_DEBUG_OUTPUT_HEMISPHERE_VIEW_SIDE,
    PT_DEBUG_OUTPUT_COUNT
};

/* ---- Pathtracer::Flags (Source/Pathtracer.h:51-68). FLAG_NONE really is bit 0. ------------ */
enum {
    PT_FLAG_NONE                            = 1 << 0,
    PT_FLAG_CULL_BACKFACE                   = 1 << 1,
    PT_FLAG_ACCUMULATE                      = 1 << 2,
    PT_FLAG_LUMINANCE_CLAMP                 = 1 << 3,
    PT_FLAG_INDIRECT_ENVIRONMENT_ONLY       = 1 << 4,
    PT_FLAG_POINT_LIGHTS                    = 1 << 5,
    PT_FLAG_SHADOW_RAYS                     = 1 << 6,
    PT_FLAG_ALPHA_SHADOWS                   = 1 << 7,
    PT_FLAG_ENVIRONMENT_MAP                 = 1 << 8,
    PT_FLAG_ENVIRONMENT_MIS                 = 1 << 9,
    PT_FLAG_MATERIAL_DIFFUSE_WHITE          = 1 << 10,
    PT_FLAG_MATERIAL_USE_GEOMETRIC_NORMALS  = 1 << 11,
    PT_FLAG_MATERIAL_MIS                    = 1 << 12,
    PT_FLAG_SHOW_NAN                        = 1 << 13,
    PT_FLAG_SHOW_INF                        = 1 << 14,
    PT_FLAG_SHADING_NORMAL_ADAPTATION       = 1 << 15
};

/* Pathtracer::MAX_BOUNCES (Source/Pathtracer.h:102).  pt_trace clamps min/max bounces to
 * [0, bounce_limit]; bounce_limit defaults to this and is raised with pt_set_bounce_limit
 * (the iterative kernel has no recursion-depth limit; BASELINE.json configs use 8 and 16). */
#define PT_REFERENCE_MAX_BOUNCES 5
#define PT_MAX_TLAS_INSTANCES 1000        /* Config::MAX_TLAS_INSTANCES, Source/Config.h:24 */
#define PT_MAX_SIMULTANEOUS_MORPH_TARGETS 4 /* Source/Config.h:21 */

/* ---- Pathtracer::Settings (Source/Pathtracer.h:70-85), field for field, 64 bytes ---------- */
typedef struct pt_settings {
    int32_t  min_bounces;                        /* default 2 */
    int32_t  max_bounces;                        /* default 2 */
    uint8_t  reset;  uint8_t _pad0[3];           /* bool reset */
    int32_t  debug_output;                       /* PT_DEBUG_OUTPUT_* */
    uint32_t flags;                              /* PT_FLAG_* */
    float    environment_color[3];               /* no initialiser upstream (quirk q28) */
    float    environment_intensity;              /* default 1 */
    uint8_t  use_frame_as_seed; uint8_t _pad1[3];/* default true */
    uint32_t seed;
    float    luminance_clamp;                    /* default 1000 */
    float    min_russian_roulette_continue_prob; /* default 0.1 */
    float    max_russian_roulette_continue_prob; /* default 0.9 */
    int32_t  max_accumulated_frames;             /* default 65536 */
    float    max_ray_length;                     /* ignored, as upstream: the host sends 1000
                                                    (Source/Pathtracer.cpp:322) */
} pt_settings;

/* ---- Renderer::GpuLight (Source/Renderer.h:53-68) == Light (Shaders/Lights.hlsli:9-19), 64 B */
enum { PT_LIGHT_POINT = 0, PT_LIGHT_SPOT = 1, PT_LIGHT_DIRECTIONAL = 2 };
typedef struct pt_light {
    int32_t type;
    float   position[3];
    float   cutoff;
    float   direction[3];
    float   intensity;
    float   color[3];
    float   inner_angle;
    float   outer_angle;
    uint8_t pad[8];
} pt_light;

/* ---- Renderer::TextureSample (Source/Renderer.h:70-86) == TextureAddress
 *      (Shaders/Material.hlsli:14-21), 32 B --------------------------------------------------- */
typedef struct pt_texture_sample {
    int32_t descriptor;   /* texture handle from pt_texture_create, -1 = none */
    int32_t sampler;      /* sampler handle, 0 = default linear/wrap (GpuResources.cpp:47-59) */
    int32_t tex_coord;    /* 0 or 1 */
    float   rotation;
    float   offset[2];
    float   scale[2];
} pt_texture_sample;

/* ---- Renderer::GpuMaterial (Source/Renderer.h:88-171) == Material
 *      (Shaders/Material.hlsli:23-66), 640 B -------------------------------------------------- */
enum { PT_MATERIAL_FLAG_DOUBLE_SIDED = 1 << 0 };
enum { PT_ALPHA_MODE_OPAQUE = 0, PT_ALPHA_MODE_MASK = 1, PT_ALPHA_MODE_BLEND = 2 };
typedef struct pt_material {
    uint32_t flags;
    int32_t  alpha_mode;
    float    metalness_factor;
    float    roughness_factor;
    float    base_color_factor[4];
    float    occlusion_factor;
    float    emissive_factor[3];           /* already multiplied by emissive_strength */
    float    alpha_cutoff;                 /* 0 unless MASK (Renderer.h:145) */
    float    ior;
    float    normal_scale;
    float    pad_0;
    pt_texture_sample normal;
    pt_texture_sample albedo;
    pt_texture_sample metallic_roughness;
    pt_texture_sample occlusion;
    pt_texture_sample emissive;
    float    specular_factor;
    float    specular_color_factor[3];
    pt_texture_sample specular;
    pt_texture_sample specular_color;
    float    clearcoat_factor;
    float    clearcoat_roughness_factor;
    float    clearcoat_normal_scale;
    float    pad_1;
    pt_texture_sample clearcoat;
    pt_texture_sample clearcoat_roughness;
    pt_texture_sample clearcoat_normal;
    float    anisotropy_strength;
    float    anisotropy_rotation;
    float    pad_2[2];
    pt_texture_sample anisotropy;
    float    sheen_color_factor[3];
    float    sheen_roughness_factor;
    pt_texture_sample sheen_color;
    pt_texture_sample sheen_roughness;
    float    transmission_factor;
    float    thickness_factor;
    float    pad_3[2];
    pt_texture_sample transmission;
    float    attenuation_distance;
    float    attenuation_color[3];
    pt_texture_sample thickness;
} pt_material;

/* ---- Pathtracer::GpuMeshInstance (Source/Pathtracer.h:131-140) == Instance
 *      (Shaders/PathTracer.lib.hlsl:32-41), 156 B.  Matrices are glm column-major. ----------- */
typedef struct pt_mesh_instance {
    float   transform[16];
    float   normal_transform[16];        /* inverseTranspose(transform), Pathtracer.cpp:205 */
    int32_t index_descriptor;            /* buffer handles; -1 = absent */
    int32_t position_descriptor;
    int32_t tangent_space_descriptor;
    int32_t texcoord_descriptors[2];
    int32_t color_descriptor;
    int32_t material_id;
} pt_mesh_instance;

/* D3D12_RAYTRACING_INSTANCE_FLAG_* values the reference sets (Source/Pathtracer.cpp:216-222) */
enum {
    PT_INSTANCE_FLAG_NONE                  = 0,
    PT_INSTANCE_FLAG_TRIANGLE_CULL_DISABLE = 0x1,
    PT_INSTANCE_FLAG_FORCE_NON_OPAQUE      = 0x8
};
/* InstanceMask (Source/Pathtracer.cpp:191-194) */
enum { PT_MASK_NONE = 1 << 0, PT_MASK_ALPHA_BLEND = 1 << 1 };

/* One TLAS instance: what Pathtracer::BuildTlas hands to AddTlasInstance plus the table row
 * (Source/Pathtracer.cpp:185-257, Source/RayTracingAccelerationStructure.cpp:292-317). */
typedef struct pt_instance_desc {
    pt_mesh_instance gpu;
    uint32_t instance_mask;      /* PT_MASK_* */
    uint32_t instance_flags;     /* PT_INSTANCE_FLAG_* */
    uint32_t num_of_vertices;
    uint32_t num_of_indices;     /* = 3 * triangles; with index_descriptor -1: vertex count */
    int32_t  dynamic;            /* non-zero: positions are rewritten by pt_skin_run each frame
                                    (DynamicBlas, ALLOW_UPDATE) */
} pt_instance_desc;

/* ---- resource formats (Source/Mesh.cpp:124-132) ------------------------------------------- */
typedef enum pt_format {
    PT_FORMAT_R16_UINT = 1,            /* index */
    PT_FORMAT_R32_UINT = 2,            /* index */
    PT_FORMAT_R32G32B32_FLOAT = 3,     /* position, morph position */
    PT_FORMAT_R10G10B10A2_UNORM = 4,   /* tangent space */
    PT_FORMAT_R32G32_FLOAT = 5,        /* texcoord */
    PT_FORMAT_R16G16B16A16_UNORM = 6,  /* color */
    PT_FORMAT_JOINT_WEIGHT = 7         /* 16 B {u16 x4 joints, unorm16 x4 weights} */
} pt_format;

/* glTF sampler (Source/TinyGltfTools.h:16-43) */
enum { PT_ADDRESS_WRAP = 0, PT_ADDRESS_MIRROR = 1, PT_ADDRESS_CLAMP = 2 };
enum { PT_FILTER_POINT = 0, PT_FILTER_LINEAR = 1 };
typedef struct pt_sampler_desc {
    int32_t address_u, address_v;
    int32_t min_filter, mag_filter;   /* one mip only: mag filter decides (LOD 0) */
} pt_sampler_desc;

/* ---- Pathtracer::ExecuteParams (Source/Pathtracer.h:87-100) -------------------------------- */
typedef struct pt_execute_params {
    float    world_to_view[16];   /* Camera::GetWorldToView, glm column-major */
    float    view_to_clip[16];    /* Camera::GetViewToClip (reversed-Z, Camera.h:80-92) */
    uint32_t width, height;
    uint64_t frame;               /* renderer's global frame counter (Renderer.h:193) */
    int32_t  light_count;
    int32_t  environment_map;     /* handle from pt_env_create, -1 = none */
    void*    output;              /* device pointer, width*height float4, caller-owned */
    /* Multi-GPU pixel-tile sharding (new capability).  Tile t (PT_TILE x PT_TILE
     * pixels, row-major) is rendered iff t % tile_rank_count == tile_rank.  {0,1} = whole frame. */
    uint32_t tile_rank, tile_rank_count;
} pt_execute_params;
#define PT_TILE 16

/* ---- GpuSkin (Source/GpuSkin.h:17-19, Shaders/Skin.cs.hlsl) -------------------------------- */
typedef struct pt_bone {          /* GpuSkin::Bone, 128 B */
    float transform[16];
    float inverse_transpose[16];
} pt_bone;
enum {                             /* Mesh::Flags as the shader sees them (Skin.cs.hlsl:4-11) */
    PT_MESH_FLAG_INDEX = 1 << 0, PT_MESH_FLAG_TANGENT_SPACE = 1 << 1, PT_MESH_FLAG_TEXCOORD_0 = 1 << 2,
    PT_MESH_FLAG_TEXCOORD_1 = 1 << 3, PT_MESH_FLAG_COLOR = 1 << 4, PT_MESH_FLAG_JOINT_WEIGHT = 1 << 5
};
enum { PT_DYNAMIC_MESH_FLAG_POSITION = 1 << 0, PT_DYNAMIC_MESH_FLAG_TANGENT_SPACE = 1 << 1 };
typedef struct pt_skin_params {
    uint32_t num_of_vertices;
    uint32_t input_mesh_flags;         /* PT_MESH_FLAG_* */
    uint32_t output_mesh_flags;        /* PT_DYNAMIC_MESH_FLAG_* */
    int32_t  input_position;           /* buffer handles */
    int32_t  input_tangent_space;
    int32_t  input_joint_weight;
    int32_t  output_position;
    int32_t  output_tangent_space;
    int32_t  num_of_morph_targets;     /* clamped to 4 */
    float    morph_weights[PT_MAX_SIMULTANEOUS_MORPH_TARGETS];
    int32_t  morph_position[PT_MAX_SIMULTANEOUS_MORPH_TARGETS];       /* handles, -1 = absent */
    int32_t  morph_tangent_space[PT_MAX_SIMULTANEOUS_MORPH_TARGETS];
    int32_t  use_mfma;                 /* 0: per-vertex VALU blend; 1: v_mfma_f32_16x16x4_f32 blend.  The matrix-core blend is used
                                          only for a call whose bones are all finite: with a NaN or an infinity in any of the
                                          bone_count * 32 floats the call takes the per-vertex blend, which like the shader confines
                                          the damage to the vertices that list the bad bone (a joint scaled to zero has an all-NaN
                                          inverse_transpose) */
} pt_skin_params;

/* ---- ToneMapper::Config (Source/ToneMapper.h:11-20) ---------------------------------------- */
enum { PT_TONEMAPPER_NONE = 0, PT_TONEMAPPER_AGX = 1 };
typedef struct pt_tonemap_config {
    int32_t tonemapper;   /* default AGX */
    float   exposure;     /* default 1 */
    int32_t frame;        /* dither seed; upstream never sets it (quirk q21) */
    int32_t dither;       /* 0 = off (parity metric is taken before dither) */
} pt_tonemap_config;

/* ---- counters ------------------------------------------------------------------------------ */
typedef struct pt_stats {
    uint64_t rays;              /* traversals started since pt_reset_stats (all kinds) */
    uint64_t rays_primary, rays_bounce, rays_shadow;
    uint64_t nodes_visited;     /* 128-B 4-wide BVH nodes fetched (0 unless counters enabled) */
    uint64_t tris_tested;       /* 48-B triangle packets fetched (0 unless counters enabled) */
    uint64_t closest_hits;      /* shading invocations */
    uint64_t texture_taps;      /* bilinear footprints fetched in shading */
    float    trace_ms;          /* hipEvent time of the last pt_trace's kernels */
    float    accel_ms;          /* last pt_build_accel */
    float    skin_ms;           /* last pt_skin_run */
    int32_t  accumulated_frames;
    uint32_t bvh_nodes, bvh_triangles;
    /* ABI 2 */
    uint64_t nodes_visited_shadow;   /* the occlusion stage's share of nodes_visited / tris_tested (wavefront mode, counters on) */
    uint64_t tris_tested_shadow;
    float    stage_ms[5];       /* last pt_trace with pt_enable_stage_timing(1): generate, closest-hit trace, shade, shadow trace,
                                   resolve -- summed over the bounces of the launch */
    uint32_t bvh_stack_need;    /* most traversal-stack entries any ray can hold in the current tree (build-time bound) */
    uint32_t accel_builds;      /* full builds / refits since pt_create */
    uint32_t accel_refits;
    uint32_t bvh_stack_capacity;       /* entries a ray's traversal stack holds for the current tree: 64 on chip, more (in memory) when
                                          bvh_stack_need asks for it -- a deep tree is never refused and never drops geometry */
    uint32_t accel_builder_fallbacks;  /* builds in which the clustering builder gave up (or made a tree too deep) and the radix
                                          tree over the same Morton order took over */
    uint64_t deep_stack_pushes;        /* stack entries rays wrote beyond the 64 on-chip ones since pt_reset_stats (0 for ordinary scenes) */
} pt_stats;

typedef struct pt_ctx pt_ctx;

/* Pathtracer::Init + GpuSkin::Create + EnvironmentMap::Init + GpuResources::LoadLookupTables
 * (Source/Pathtracer.h:104, GpuSkin.h:17, Renderer.cpp:161-170).  `device` = HIP device ordinal,
 * `hip_stream` = hipStream_t all work is enqueued on (NULL = the device's default stream).
 * `sheen_e_16x16` = the 256-float Sheen_E table (row = alpha, column = cos_theta). */
int pt_create(int device, void* hip_stream, const float* sheen_e_16x16, pt_ctx** out);
/* Pathtracer::Shutdown (Source/Pathtracer.h:106) */
void pt_destroy(pt_ctx* ctx);
const char* pt_last_error(const pt_ctx* ctx);
int pt_abi_version(void);

/* Vertex / index streams: Mesh::Create sub-allocations + descriptors (Source/Mesh.cpp:103-190).
 * host may be NULL (DynamicMesh outputs, Source/Mesh.cpp:236-290): the buffer is then zero-filled on the context's stream, ahead of
 * the pt_skin_run that writes it. */
int pt_buffer_create(pt_ctx* ctx, const void* host, size_t bytes, int format, int* handle_out);
int pt_buffer_update(pt_ctx* ctx, int handle, const void* host, size_t bytes);
int pt_buffer_read(pt_ctx* ctx, int handle, void* host, size_t bytes);
/* Gltf::Unload (Source/Gltf.cpp:123-157; called before the next scene loads, Source/Main.cpp:43-54): release one stream / texture.
 * Fails with PT_ERR_NOT_READY while the current instance table (buffers) or material table (textures) still refers to it --
 * replace those tables first, as the reference's per-frame tables are rebuilt from the new scene.  Handles are reused. */
int pt_buffer_destroy(pt_ctx* ctx, int handle);
int pt_texture_destroy(pt_ctx* ctx, int handle);
/* Gltf::LoadTexture (Source/Gltf.cpp:1047-1078): RGBA8, one mip, optional sRGB view. */
int pt_texture_create(pt_ctx* ctx, const uint8_t* rgba8, int width, int height, int srgb, int* handle_out);
/* Gltf::LoadSamplers (Source/Gltf.cpp:935, TinyGltfTools.h:16-43). Handle 0 pre-exists. */
int pt_sampler_create(pt_ctx* ctx, const pt_sampler_desc* desc, int* handle_out);

/* Renderer::GatherMaterials / GatherLights outputs (Source/Renderer.cpp:459-500) */
int pt_scene_set_materials(pt_ctx* ctx, const pt_material* materials, int count);
int pt_scene_set_lights(pt_ctx* ctx, const pt_light* lights, int count);
/* Pathtracer::BuildTlas instance list (Source/Pathtracer.cpp:185-257); marks the accel dirty. */
int pt_scene_set_instances(pt_ctx* ctx, const pt_instance_desc* instances, int count);

/* EnvironmentMap::CreateEnvironmentMap (Source/EnvironmentMap.cpp:84-130), the part the path tracer reads:
 * equirect RGB32F -> RGBA16F cube (+mips) -> 1024^2 importance pyramid.  The GGX / diffuse cubes of the raster
 * pass are made on request by pt_env_filter (below). */
int pt_env_create(pt_ctx* ctx, const float* equirect_rgb32f, int width, int height, int* env_out);
/* Test hook: copy out the preprocessed maps.  cube_rgba16f: 6*N*N*4 halfs of mip 0 (may be NULL);
 * importance: the whole pyramid, level 0 first (may be NULL).  Sizes via the out params. */
int pt_env_read(pt_ctx* ctx, int env, int* cube_size_out, uint16_t* cube_rgba16f, float* importance_pyramid);
/* EnvironmentMap::Destroy (the reference replaces its one environment in place, Source/EnvironmentMap.cpp:84-130). */
int pt_env_destroy(pt_ctx* ctx, int env);
/* The environment's GGX and diffuse cubes: EnvironmentMap::GenerateGgxCube / GenerateDiffuseCube -> FilterCube
 * (Source/EnvironmentMap.cpp:348-401, Shaders/FilterEnvironmentCubeMap.cs.hlsl) -- the prefiltered specular chain and the irradiance cube a
 * host's raster pass lights with (EnvironmentMap::Map::ggx / ::diffuse).  pt_trace never reads them: the call changes nothing the path tracer
 * sees (the cube, the pyramid, images, ray counts).  Enqueued on the context's stream, asynchronous like pt_trace; a second call on the same
 * environment replaces the cubes (a call whose sizes differ from the last one's waits for the stream before it reallocates); pt_env_destroy
 * and pt_destroy free them.  An environment from the test hook pt_debug_env_create_raw filters like any other.
 *   Everything below is float32 in the order written, products and sums not fused; / is the correctly rounded division, sqrt the correctly
 * rounded root; sin, cos are those of pt_trace (evaluated in double, rounded once), log2 is pt_trace's defined log2 (csrc/pt_math.h co_log2);
 * fmin / fmax return the operand that is not a NaN, saturate(x) = fmin(fmax(x, 0), 1), so saturate(NaN) = 0.  PI = 3.14159265359f, TAU = 2 PI.
 * N, M: the environment cube's mip-0 size and mip count (sizes N >> k down to 1).
 *   Levels.  GGX level i = 0 .. ggx_mips - 1 has resolution n_0 = N, n_{i+1} = n_i / 2 (integer: 33, 16, 8) and roughness
 * a_i = r r with r = (float)i / ((float)ggx_mips - 1.0f) (MipToRoughness, EnvironmentMap.cpp:17-22).  Upstream divides 0 by 0 there when
 * the chain has ONE level; here a chain of one level has roughness 0 (quirk q30).  The diffuse cube has one level of diffuse_resolution.
 *   Per output texel (face, x, y) of a level of resolution n, with S = the level's sample count:
 *     uu = ((float)x + 0.5f) / (float)n;  vv likewise;  d = F + (2 uu - 1) U + (2 vv - 1) V with (F, U, V) of the face
 *         (CubemapToDirection, Transforms.hlsli:10-50);  normal = d / sqrt((d.x d.x + d.y d.y) + d.z d.z)
 *     CreateBasis (Common.hlsli:33-42): b = |normal.x| > |normal.z| ? (-normal.y, normal.x, 0) : (0, -normal.z, normal.y), normalised as
 *         above;  t = cross(b, normal)
 *     total = (0, 0, 0);  total_weight = 0;  for i = 0 .. S - 1, in this order (one lane sums one texel):
 *       R2 (Random.hlsli:80-85): g = 1.324717957244746f, c = (1.0f / g, 1.0f / (g g));  s = 0.5f + (float)i c;  u = s - floor(s)
 *       GGX:      cs, sn = cos, sin(TAU u.x);  ct = sqrt((1 - u.y) / (1 + (a a - 1) u.y));  st = sqrt(1 - ct ct);  h = (st cs, st sn, ct)
 *                 D = (a a) (h.z > 0 ? 1 : 0) / (e (PI e)) with e = (h.z h.z) (a a - 1) + 1;   pdf = D / 4
 *                 hw = t h.x + b h.y + normal h.z (per component, summed left to right);  v = -normal;
 *                 l = v - (2 dot(hw, v)) hw;  weight = saturate(dot(normal, l))
 *       diffuse:  cs, sn = cos, sin(TAU u.x);  y = 2 u.y - 1;  r = sqrt(1 - y y);  l = normal + (r cs, r sn, y), normalised as above;
 *                 pdf = saturate(dot(l, normal) / PI);  weight = 1
 *       omega_s = 1.0f / ((float)S pdf);  omega_p = (4.0f PI) / ((6.0f (float)N) (float)N);  level = 0.5f log2(omega_s / omega_p) + mip_bias
 *       level = fmin(fmax(level, 0), (float)(M - 1)): D3D's clamp, so a NaN level becomes 0 and +infinity becomes M - 1.  Both occur: at
 *           a = 0 (GGX level 0) e is 0 and D is 0 / 0, so every sample reads mip 0; a diffuse sample with pdf 0 reads the last mip
 *       l0 = (int)floor(level);  f = level - (float)l0;  A = the bilinear cube lookup along l in mip l0 (the seamless four-tap lookup of
 *           pt_trace's environment, csrc/pt_shading.h sample_cube);  c = A if f == 0 or l0 == M - 1, else A (1 - f) + B f with B the
 *           lookup in mip l0 + 1 (what pt_env_create's importance map does)
 *       total = total + weight c;  total_weight = total_weight + weight
 *     out.rgb = total / total_weight rounded to nearest-even half; out.a = 0, as the cube's own mips write it.
 *   The per-sample values that do not depend on the texel (GGX: h and the clamped level; diffuse: the point (r cs, r sn, y)) are computed
 * once per level; the result is the per-texel text above bit for bit.  Non-finite texels get no special treatment.  Upstream's sampler
 * weights are the hardware's fixed-point ones, so parity with real D3D output is unpinned, as everywhere else in this project.
 *   PT_ERR_BAD_HANDLE for an env that is not live; PT_ERR_INVALID_ARGUMENT, with nothing changed, for a config value out of range;
 * pt_env_filter_info_get and pt_env_filter_read answer PT_ERR_NOT_READY before the first pt_env_filter of the environment. */
typedef struct pt_env_filter_config {
    int32_t ggx_samples;         /* 1..4096, default 256  (EnvironmentMap.cpp:395) */
    float   ggx_mip_bias;        /* finite,  default 2 */
    int32_t ggx_mips;            /* 0 = the reference's rule max((int)floor(log2((float)N)) + 1 - 4, 1) (EnvironmentMap.cpp:106-107);
                                    otherwise 1 .. the number of levels whose resolution N >> i is >= 1 (at most 16) */
    int32_t diffuse_samples;     /* 1..4096, default 512  (EnvironmentMap.cpp:400) */
    float   diffuse_mip_bias;    /* finite,  default 3 */
    int32_t diffuse_resolution;  /* 1..1024, default 256  (EnvironmentMap.cpp:114) */
} pt_env_filter_config;          /* 24 bytes */
typedef struct pt_env_filter_info {
    int32_t ggx_resolution, ggx_mips, diffuse_resolution;
    float   ggx_roughness[16];   /* a_i of level i; 0 beyond ggx_mips */
} pt_env_filter_info;            /* 76 bytes */
int pt_env_filter(pt_ctx* ctx, int env, const pt_env_filter_config* config /* NULL = the reference's values */);
int pt_env_filter_info_get(pt_ctx* ctx, int env, pt_env_filter_info* out);
/* One level of one of the two cubes.  which: 0 = GGX, 1 = diffuse (mip 0 only).  *size_out = the level's resolution n.  host and device_out
 * may each be NULL.  host receives 6 * n * n * 4 halfs (face-major, like pt_env_read) after the stream has been synchronised; device_out
 * receives the context-owned device pointer to the same texels, valid until the next pt_env_filter on this environment or its
 * pt_env_destroy, for a host's raster pass (without host the call does not wait: order the reader behind the context's stream).
 * PT_ERR_INVALID_ARGUMENT for a `which` or `mip` that does not exist. */
int pt_env_filter_read(pt_ctx* ctx, int env, int which, int mip, int* size_out, uint16_t* host, void** device_out);

/* BuildAllBlas / UpdateAllBlas / BuildTlas (Source/Pathtracer.cpp:138-257).  Called implicitly
 * by pt_trace when the scene is dirty; exposed so it can be timed on its own.
 *   - a new set of triangles (instance count, index counts) -> full build: Morton sort, LBVH, 4-wide collapse;
 *   - only vertices moved (pt_skin_run, pt_buffer_update) or instance rows changed (transform, flags) -> REFIT, like
 *     UpdateDynamicBlas (Source/RayTracingAccelerationStructure.cpp:110-158): topology and triangle order stay, the touched
 *     instances' packets are rewritten and every box re-derived.  Hits equal a full rebuild's; the tree's quality follows the
 *     pose it was built for, as upstream's refitted BLAS does (upstream never rebuilds one);
 *   - an instance table identical to the current one -> nothing.
 * A row that differs from the current one in its material_id alone leaves the tree and its packets as they are (the packets name the row,
 * not the material): neither a build nor a refit.  A pt_buffer_update or pt_skin_run that writes a buffer no row of the current instance
 * table reads changes nothing for the tree.  A call that is refused (any return code but PT_OK from pt_scene_set_instances,
 * pt_scene_set_materials or pt_buffer_update) changes nothing: tables, buffers, what is pending and the motion snapshot's state stay.
 * pt_accel_request_rebuild forces the next call to build from scratch (e.g. after a pose has drifted far from the built one). */
int pt_build_accel(pt_ctx* ctx);
int pt_accel_request_rebuild(pt_ctx* ctx);
/* Which builder a full build uses (all on-device, all over the Morton order of the triangles' centroids):
 *   PT_BUILDER_LBVH  the radix tree of the sorted codes (Karras 2012): the fastest build (0.6 ms at 257 k triangles);
 *   PT_BUILDER_PLOC  parallel locally-ordered clustering (Meister & Bittner 2018) over the same order: neighbours
 *                    merge by joint surface area, bottom-up -- a better tree (7-35 % fewer node visits per ray on the BASELINE
 *                    scenes) for four times the build time (2.3 ms): the counterpart of the reference's PREFER_FAST_TRACE
 *                    static BLAS (RayTracingAccelerationStructure.cpp:228-290);
 *   PT_BUILDER_PLOC_REINSERT  (default) the PLOC tree improved by passes of parallel reinsertion (Meister & Bittner 2018): every
 *                    node looks for the place in the tree where it costs the least surface area and the moves that do not
 *                    touch each other are carried out, eight times over.
 * Same hits whichever builds.  Changing it makes the next pt_build_accel a full build.  The refit works on all.  The environment
 * variable MIPT_ACCEL_BUILDER = "lbvh" | "ploc" | "reinsert" sets the builder new contexts start with. */
enum { PT_BUILDER_LBVH = 0, PT_BUILDER_PLOC = 1, PT_BUILDER_PLOC_REINSERT = 2 };
int pt_set_accel_builder(pt_ctx* ctx, int builder);

/* GpuSkin::Run (Source/GpuSkin.cpp:57-118).  bones may be NULL (no skinning, quirk q19 kept). */
int pt_skin_run(pt_ctx* ctx, const pt_skin_params* params, const pt_bone* bones, int bone_count);

/* Pathtracer::PathtraceScene (Source/Pathtracer.cpp:259-367): one sample per pixel blended into
 * params->output with weight 1/(n+1); no-op once accumulated_frames >= max_accumulated_frames;
 * accumulation resets when world_to_clip changes or settings->reset. */
int pt_trace(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params);
int pt_set_bounce_limit(pt_ctx* ctx, int limit);      /* default PT_REFERENCE_MAX_BOUNCES */
/* Sample batch: with samples > 1 one pt_trace stands for `samples` consecutive PathtraceScene calls (frames frame ..
 * frame + samples - 1, camera unchanged) carried by ONE set of kernel launches, so a small image or a small tile shard
 * still fills the GPU.  The output is bit-identical to issuing the calls one by one: sample k draws with the seed of frame
 * frame + k (or settings->seed when use_frame_as_seed is 0) and is blended with weight 1 / (accumulated_frames + k + 1)
 * in order; accumulated_frames advances by the batch and never passes max_accumulated_frames.  Without FLAG_ACCUMULATE,
 * or with a debug output, the batch is ignored: the call renders the one sample of `frame`, as always.  Default 1. */
#define PT_MAX_SAMPLES_PER_TRACE 64
int pt_set_samples_per_trace(pt_ctx* ctx, int samples);
/* Tile-level adaptive sampling (absent upstream: the reference renders every pixel every frame).  Off by default; with it off, or on a
 * call without FLAG_ACCUMULATE or with a debug output, pt_trace is exactly as described above.  On an adaptive call every 16x16 tile
 * of the rank that is still ACTIVE gets the call's samples, with the seeds and blend weights of the uniform accumulation (active tiles
 * all hold the context's accumulated_frames samples); a RETIRED tile gets no rays and its output pixels are not written.  Besides the
 * output the context keeps a W x H RGBA32F half buffer A: the running mean of the samples with an even per-tile index (0, 2, 4 ...).
 * After the call's samples each active tile gets an error E, the max over its in-image pixels of
 *     e = ((|I.r-A.r| + |I.g-A.g|) + |I.b-A.b|) / (1e-4 + sqrt(max((I.r + I.g) + I.b, 0)))   (float32, a NaN counts as +inf)
 * with I the accumulated output, and retires once its count n >= min(max_samples, max_accumulated_frames), or n >= min_samples and
 * E <= threshold.  Tile t of the output is then bit-identical to tile t of the uniform accumulation after tile_samples[t] frames.
 * A new accumulation (accumulated_frames 0 after the reset check, a new size or tile shard, or the first trace after pt_set_adaptive)
 * makes every tile active again.  The batch is clamped to min(max_samples, max_accumulated_frames) - accumulated_frames.
 * Wavefront mode only: an adaptive call in PT_MODE_MEGAKERNEL fails with PT_ERR_INVALID_ARGUMENT and leaves the output untouched. */
typedef struct pt_adaptive_config {
    int32_t enable;        /* 0 = off (default) */
    int32_t min_samples;   /* >= 2: samples every tile takes before it may stop */
    int32_t max_samples;   /* >= min_samples: a tile stops here (and at settings->max_accumulated_frames) */
    float   threshold;     /* finite, >= 0: a tile stops once its error <= threshold */
} pt_adaptive_config;
/* PT_ERR_INVALID_ARGUMENT for a bad config (checked when enable != 0).  Forces a new accumulation on the next pt_trace. */
int pt_set_adaptive(pt_ctx* ctx, const pt_adaptive_config* config);
/* The state after the last adaptive trace.  Synchronises the stream.  Tiles are row-major, ceil(W/16) x ceil(H/16), GLOBAL tile ids:
 * active_tiles = this rank's tiles still active; tile_samples = each tile's count (at retirement, or the current one); tile_error = its
 * last E; half_rgba32f = the half buffer (W * H * 4 floats).  Tiles another rank owns read 0.  Every pointer may be NULL.
 * PT_ERR_NOT_READY before the first adaptive trace, PT_ERR_INVALID_ARGUMENT for a size other than the one traced. */
int pt_adaptive_read(pt_ctx* ctx, uint32_t width, uint32_t height, int32_t* active_tiles,
                     uint32_t* tile_samples, float* tile_error, float* half_rgba32f);
/* First-hit AOVs (absent upstream): albedo, shading normal and depth of the vertex each pixel-sample's camera ray reaches, accumulated
 * beside the output for denoisers and compositing.  Off by default; with it off pt_trace is exactly as described above, and with it on
 * the output, the ray counts and accumulated_frames are what they are without it.  The targets are device pointers to W * H float4,
 * caller-owned like pt_execute_params.output (so pt_readback, pt_tonemap, pt_tiles_pack and pt_exchange_frame take them as they are);
 * either may be NULL.  Per sample, under the call's flags:
 *     albedo        rgb = the surface's base colour (what PT_DEBUG_OUTPUT_COLOR shows), w = 1 (coverage)
 *     normal_depth  xyz = the signed world-space shading normal after the back-face flip (PT_DEBUG_OUTPUT_SHADING_NORMAL shows
 *                   (xyz + 1) / 2), w = the camera ray's hit distance t
 * A miss contributes zeros to both; so does, to its target, a sample with a non-finite component (the luminance clamp, FLAG_SHOW_NAN
 * and FLAG_SHOW_INF do not apply).  Each target is the running mean of its samples with the output's weights 1 / (n + 1), in sample
 * order, under the output's counts and resets: a sample batch equals the calls one by one, a call without FLAG_ACCUMULATE leaves the
 * one sample, a tile shard writes only the rank's tiles, and a tile retired by adaptive sampling is not written (it equals the uniform
 * AOV after its own count).  albedo.rgb / albedo.w is the mean over the samples that hit; the mean of normals is not unit length.
 * A call with a debug output leaves the targets untouched.  Wavefront mode only: a call with AOVs enabled in PT_MODE_MEGAKERNEL fails
 * with PT_ERR_INVALID_ARGUMENT and writes nothing. */
typedef struct pt_aov_config {
    int32_t enable;          /* 0 = off (default) */
    void*   albedo;          /* device, W*H float4, caller-owned, may be NULL */
    void*   normal_depth;    /* device, W*H float4, caller-owned, may be NULL */
} pt_aov_config;
/* PT_ERR_INVALID_ARGUMENT if enable != 0 and both targets are NULL.  Forces a new accumulation on the next pt_trace, so that the
 * targets and the output always hold the same samples. */
int pt_set_aov(pt_ctx* ctx, const pt_aov_config* config);
/* Denoiser (absent upstream): an edge-avoiding a-trous filter over an image and its first-hit AOVs.  One pure function of three images,
 * C = color, A = albedo, N = normal_depth in the layout pt_set_aov writes: it reads no pt_trace state, so it takes the images after an
 * exchange, after adaptive sampling, or a rank's partial image alike.  All four images are device pointers to W * H float4, caller-owned
 * like pt_execute_params.output; out == color filters in place.  Enqueued on the context's stream, asynchronous like pt_trace.  The
 * scratch (two signal images and one guide image of W * H float4) belongs to the context: reallocated when the size changes, freed by
 * pt_destroy.  All arithmetic is float32, in the order written; cov = A.w.
 *   Prepare, per pixel:
 *     a' = max(A.rgb + (1 - cov), 1e-3) channel-wise if demodulate, else 1 (a miss counts as albedo 1, so a silhouette pixel demodulates
 *          consistently);  signal S = C.rgb / a';  guide n = N.xyz / |N.xyz| with |N.xyz| = sqrt((x x + y y) + z z), and z = N.w / cov.
 *     The pixel is VALID iff cov > 0, |N.xyz| > 0, z is finite and > 0, and every component of S and n is finite.  An invalid pixel is
 *     never a neighbour -- its weight is 0 by a select, not by a product, so a NaN cannot leak -- and leaves the call with out = C, all
 *     four channels bit for bit: background, tiles another rank renders, non-finite samples.
 *   Pass i = 0 .. iterations - 1, step s = 2^i: for a valid centre p the taps are q = p + s (dx, dy), dx, dy in -2 .. 2, dy outer, dx
 *     inner; taps outside the image or invalid are skipped.  With h = (1/16, 1/4, 3/8, 1/4, 1/16) and L = (S.r + S.g) + S.b,
 *         w  = ((h[dy] h[dx]) wn) exp(-(ez + ec))
 *         wn = clamp((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0, 1), squared normal_power_log2 times
 *         ez = |z_p - z_q| / ((sigma_depth s) z_p + 1e-6)
 *         ec = ((dr dr + dg dg) + db db) / (sigma_i^2 ((L_p + L_q)(L_p + L_q)) + 1e-8), d = S_p - S_q, sigma_i = sigma_color 2^-i;
 *              0 when sigma_color == 0
 *     and S'_p = (sum of w S_q) / (sum of w), the sums sequential in tap order.  The centre tap keeps the sum of w near 9/64 or above.
 *     The colour term is relative and symmetric: an absolute sigma removes almost no noise at low sample counts, and a centre-only
 *     relative term leaves black drop-out pixels black.
 *   After the passes a valid pixel gets out.rgb = S a' and out.w = C.w.  iterations = 0 gives out = C bit for bit everywhere.
 * PT_ERR_INVALID_ARGUMENT, with nothing written: a NULL ctx (answered before any device call), a NULL image, a zero width or height, a
 * width or height above 2^30, a config value outside the ranges below, out overlapping albedo or normal_depth (or color without being
 * color). */
typedef struct pt_denoise_config {
    int32_t iterations;         /* 0..6 passes; pass i taps at spacing 2^i.  default 5 */
    int32_t demodulate;         /* non-zero: filter colour / albedo', multiply back.  default 1 */
    int32_t normal_power_log2;  /* 0..10: normal weight = max(0, n_p . n_q)^(2^k) by k squarings.  default 7 */
    float   sigma_depth;        /* finite, > 0.  default 0.02 */
    float   sigma_color;        /* finite, >= 0; 0 = colour term off.  default 1 */
} pt_denoise_config;            /* 20 bytes */
int pt_denoise(pt_ctx* ctx, const pt_denoise_config* config /* NULL = defaults */,
               const void* color, const void* albedo, const void* normal_depth,
               uint32_t width, uint32_t height, void* out);
/* Saving and resuming an accumulation (absent upstream).  The state of a running accumulation is the caller's images (the output and, with
 * pt_set_aov, the two AOV targets), the context's count and camera (accumulated_frames, the previous world_to_clip) and, with pt_set_adaptive,
 * the per-tile records and the half buffer.  pt_accum_save writes all of it to one host blob; pt_accum_load puts it into another context --
 * a new process, another day -- so that pt_trace continues: save, pt_destroy, pt_create, upload the scene, pt_set_adaptive / pt_set_aov /
 * pt_set_samples_per_trace as for a fresh run, load, trace on with reset = 0 and the saved camera gives bit for bit the images and the
 * tile state of the run that was never interrupted.  A rank of the tile-sharded renderer saves what it owns: its tiles, 1 / N of each image.
 *
 * The blob, little-endian.  Header, 160 bytes:
 *     offset  0  char[8]   "MIPTACC1"
 *             8  u32       version = 1
 *            12  u32       header_bytes = 160
 *            16  u64       total_bytes: the whole blob
 *            24  u32       crc32 of bytes [28, total_bytes): the IEEE 802.3 polynomial, zlib's crc32
 *            28  u32       sections: PT_ACCUM_* bits
 *            32  u32       width
 *            36  u32       height
 *            40  u32       tile_rank
 *            44  u32       tile_rank_count (>= 1; a 0 given to pt_accum_save is stored as 1)
 *            48  i32       accumulated_frames (>= 1)
 *            52  u32       tiles: the 16x16 tiles t of the ceil(width / 16) x ceil(height / 16) grid with t % tile_rank_count == tile_rank
 *            56  u64       next_frame: the caller's value, the frame number to continue with
 *            64  f32[16]   previous_world_to_clip, as pt_trace compares it
 *           128  pt_adaptive_config {i32 enable, i32 min_samples, i32 max_samples, f32 threshold}; zeros without PT_ACCUM_ADAPTIVE
 *           144  u32[4]    reserved = 0
 * Payload, from offset 160, with P = pt_tiles_packed_bytes(width, height, tile_rank, tile_rank_count) = tiles * 256 * 16:
 *     for each image bit present, in the order OUTPUT, ALBEDO, NORMAL_DEPTH: the rank's tiles in pt_tiles_pack's layout, P bytes;
 *     with PT_ACCUM_ADAPTIVE: `tiles` records of 16 bytes {u32 active, u32 samples, f32 error, u32 0}, rank-local tile k being tile
 *     tile_rank + k * tile_rank_count, then the half buffer packed like an image, P bytes.
 * total_bytes = 160 + images * P + (ADAPTIVE ? tiles * 16 + P : 0). */
enum { PT_ACCUM_OUTPUT = 1 << 0, PT_ACCUM_ALBEDO = 1 << 1, PT_ACCUM_NORMAL_DEPTH = 1 << 2, PT_ACCUM_ADAPTIVE = 1 << 3 };
typedef struct pt_accum_images {      /* device pointers, W*H float4, caller-owned; NULL = not part of the state */
    void* output; void* albedo; void* normal_depth;
} pt_accum_images;
typedef struct pt_accum_info {        /* what a blob holds; filled by pt_accum_inspect */
    uint32_t sections;                /* PT_ACCUM_OUTPUT | _ALBEDO | _NORMAL_DEPTH | _ADAPTIVE = bits 0..3 */
    uint32_t width, height, tile_rank, tile_rank_count;
    int32_t  accumulated_frames;
    uint32_t tiles;                   /* tiles of that rank */
    uint64_t next_frame;              /* caller's value from save: the frame number to continue with */
    uint64_t total_bytes;
    pt_adaptive_config adaptive;      /* zeros without PT_ACCUM_ADAPTIVE */
} pt_accum_info;                      /* 64 bytes */
/* Writes the state to host_blob.  Synchronises the stream.  images->output is required; an AOV image is a section iff its pointer is given
 * (the caller passes the targets of pt_set_aov, which hold the output's samples).  tile_rank / tile_rank_count as in pt_execute_params
 * (a count of 0 means 1).  host_blob == NULL: only the size needed goes to *bytes_out.  PT_ERR_INVALID_ARGUMENT, with *bytes_out set, for
 * a capacity below it.  PT_ERR_NOT_READY, with nothing written, while there is nothing to save: accumulated_frames is 0, or pt_set_adaptive /
 * pt_set_aov was called after the last trace (the next trace starts a new accumulation anyway).  The ADAPTIVE section is present iff
 * adaptive sampling is enabled and the tile state describes this accumulation (the last accumulating trace was adaptive, of this size and
 * tile shard): exactly when the next adaptive pt_trace would continue rather than restart.  Otherwise the blob is a uniform one, and an
 * adaptive trace after its load restarts as the uninterrupted one would.  The images are packed through device scratch that belongs to
 * the context (one packed image per section; freed by pt_destroy). */
int pt_accum_save(pt_ctx* ctx, const pt_accum_images* images, uint32_t width, uint32_t height,
                  uint32_t tile_rank, uint32_t tile_rank_count, uint64_t next_frame,
                  void* host_blob, size_t capacity, size_t* bytes_out);
/* Puts a blob's state into the context and the targets.  The order for a caller: pt_create, the scene, pt_set_adaptive / pt_set_aov as for a
 * fresh run, then this.  The blob is validated as by pt_accum_inspect; then a target must be given for every image section and none without
 * one, and with PT_ACCUM_ADAPTIVE the context's adaptive config must be enabled and equal the blob's field by field (the threshold by its
 * bits).  Only then is anything written: any of these failures is PT_ERR_INVALID_ARGUMENT with a message naming the field, the context and
 * the targets as they were.  The sections are unpacked into the targets -- the rank's tiles only, other pixels are not touched -- the tile
 * records and the half buffer go into the context, accumulated_frames and the previous world_to_clip are set, and a pending restart from
 * pt_set_adaptive / pt_set_aov is cleared.  The blob is consumed before the call returns (it waits for its own uploads); the unpacking is
 * enqueued on the stream like pt_trace.  Afterwards a pt_trace with the saved camera and reset == 0 continues; another camera or reset
 * starts anew as always.  The kernel mode is no part of the state: a uniform accumulation resumes in either. */
int pt_accum_load(pt_ctx* ctx, const void* host_blob, size_t bytes, const pt_accum_images* targets);
/* Parses and checks a blob: no context, no device call.  PT_ERR_INVALID_ARGUMENT for: bytes < 160, a wrong magic, version or header_bytes,
 * total_bytes != bytes; unknown section bits, no OUTPUT, a non-zero reserved word; a width or height of 0 or above 2^30, tile_rank_count 0,
 * tile_rank >= tile_rank_count; `tiles` other than the rank's tile count, accumulated_frames < 1; a total_bytes other than the formula
 * above (64-bit arithmetic); with ADAPTIVE a config pt_set_adaptive refuses or one not enabled, without it a non-zero config byte; a crc
 * mismatch; with ADAPTIVE a tile record with active > 1, samples > accumulated_frames, an active tile whose samples != accumulated_frames,
 * a NaN error or a non-zero pad. */
int pt_accum_inspect(const void* host_blob, size_t bytes, pt_accum_info* out);
/* Thin-lens depth of field (absent upstream: the reference's camera is a pinhole).  Off by default; with enable == 0 or aperture_radius == 0
 * none of the arithmetic below runs and the rays, the images, the AOVs and the ray counts are bit for bit those of the pinhole.  With the
 * lens on it applies to the camera ray of every pt_trace: both kernel modes, every sample of a batch, calls with a debug output.  The lens
 * sample comes from the two numbers of the camera ray's own random draw that the pixel jitter leaves unused (r.z, r.w of the draw whose
 * r.x, r.y jitter the pixel): no extra draw, so the random sequence of every later vertex is what it is without a lens.
 *   The host derives four vectors from view_to_world = inverse(world_to_view), computed in fp64, each component rounded once to float:
 *     c = column 3 (the camera position), R, U, F = columns 0, 1 and MINUS column 2, each normalised in fp64 before the rounding.
 *   Let (o, d, tmax) be the pinhole ray (o on the near plane, d unit, tmin = 0) and r its random draw.  All float32, in the order written:
 *     zo = dot(o - c, F)                       the near distance           (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z)
 *     dn = dot(d, F)
 *     P  = o + d * ((focus_distance - zo) / dn)          the point in focus
 *     A  = o - d * (zo / dn)                   where the ray crosses the lens plane: c for a perspective camera; the same definition
 *                                              gives an orthographic camera a lens too
 *     (lx, ly) = aperture_radius * L(r.z, r.w):
 *         blades == 0:  L = square_to_disk(uv_to_square({r.z, r.w}))       (the reference's concentric mapping, Transforms.hlsli)
 *         blades == n:  with v_k = (cos, sin)(blade_rotation + 2 pi k / n), k = 0 .. n, computed on the host in fp64 and rounded once
 *                       (v_n = v_0):  s = r.z * n;  k = min((int)s, n - 1) (r.z may be exactly 1);  a = sqrt(s - k);
 *                       L = a * ((1 - r.w) * v_k + r.w * v_{k+1})          uniform over the polygon inscribed in the unit circle
 *     A' = (A + lx * R) + ly * U
 *     d' = normalize(P - A')
 *     o' = A' + d' * (zo / dot(d', F))         back on the near plane, so near clipping is kept
 *     tmin = 0, tmax' = tmax
 *   The divisions are correctly rounded (operands and quotients in the normal range); normalize(v) = v / sqrt(dot(v, v)).  The first-hit AOV depth (pt_set_aov) is t along this lens ray.
 * The lens is a setting, like pt_settings: it is NOT part of the blob of pt_accum_save, whose format is unchanged -- a caller who resumes
 * calls pt_set_lens with the same config before pt_accum_load. */
typedef struct pt_lens_config {
    int32_t enable;           /* 0 = pinhole (default) */
    float   aperture_radius;  /* world units; finite, >= 0.  0 gives the pinhole ray bit for bit */
    float   focus_distance;   /* view-space depth of the plane in focus; finite, > 0 */
    int32_t blades;           /* 0 = circular aperture; 3..16 = regular polygon inscribed in the circle */
    float   blade_rotation;   /* radians, finite: angle of polygon vertex 0 */
} pt_lens_config;             /* 20 bytes */
/* PT_ERR_INVALID_ARGUMENT for a NULL pointer or a bad config (checked only when enable != 0; the message names the field): the old config
 * stays and no restart is pending.  A good config forces a new accumulation on the next pt_trace, as pt_set_aov does: until that trace
 * pt_accum_save answers PT_ERR_NOT_READY, and pt_accum_load clears the pending restart. */
int pt_set_lens(pt_ctx* ctx, const pt_lens_config* config);
/* Autofocus: the view-space depth of what the pinhole ray through image position (px, py) sees -- pixel units, pixel centres at + 0.5, no
 * jitter, no lens -- for pt_lens_config.focus_distance.  TraceRay's closest hit under the settings' cull flag (FLAG_CULL_BACKFACE); builds
 * the acceleration structure if it is dirty; synchronises the stream; *focus_distance_out = zo + t * dn in float32 (zo, dn as above).
 * PT_ERR_NOT_READY on a miss, with nothing written.  PT_ERR_INVALID_ARGUMENT for a NULL pointer, a zero size or a position outside
 * [0, width] x [0, height].  Does not touch the accumulation. */
int pt_lens_focus_at(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params,
                     float px, float py, float* focus_distance_out);
/* Texture-space baking (absent upstream).  With a bake on, pt_trace renders into a UV atlas instead of through a camera: params->width x
 * height is the atlas, and every (texel, sample) whose texel a triangle covers starts a path on that triangle's surface.  Only the first ray
 * differs -- from its first closest hit on, a path is the path of a camera frame -- so sample batches, tile shards, adaptive sampling, AOVs,
 * pt_denoise, pt_accum_save / load and pt_exchange_frame apply to the atlas as to any W x H image, bit for bit.  With the bake off (the
 * default) every image, ray count and stat is what it is without this section.  world_to_view / view_to_clip generate no rays under a bake
 * but must still be valid (identity will do) and still drive the reset comparison; the lens (pt_set_lens) does not apply, pt_lens_focus_at
 * is unaffected; debug outputs work, the first vertex being the texel's surface point.  Wavefront mode only: a bake call in
 * PT_MODE_MEGAKERNEL fails with PT_ERR_INVALID_ARGUMENT and writes nothing.  An `instance` >= the current instance table's count is
 * reported by the pt_trace that meets it (PT_ERR_INVALID_ARGUMENT, nothing written).
 *   The coverage map (owned by the context, the whole atlas on every rank) is built by the pt_trace that needs it and rebuilt after
 * pt_build_accel had work to do (a build or a refit), after pt_set_bake and after a change of size.  float32 throughout, every operation in
 * the order written, products and sums not fused:
 *     texel (x, y) has the centre p = (x + 0.5, y + 0.5), in texel units
 *     a triangle's UV vertices (set tex_coord) are A, B, C = (u * (float)W, v * (float)H): no wrap, no flip; UVs outside [0, 1] fall off the atlas
 *     E(P, Q, p) = (Q.x - P.x)(p.y - P.y) - (Q.y - P.y)(p.x - P.x)        area2 = E(A, B, C)
 *     a triangle takes part if its instance is selected (instance == -1, or that row) and has the UV stream, and unless
 *         area2 == 0 or one of the six coordinates is not finite, or
 *         n = cross(e1, e2) of its world-space edges (e1 = v1 - v0, e2 = v2 - v0) has sqrt(dot(n, n)) zero or not finite
 *     it covers p iff each of E(B, C, p), E(C, A, p), E(A, B, p) is zero or has area2's sign
 *     the texel's owner is the covering triangle with the least (instance, primitive) pair -- whatever the builder (PT_BUILDER_*), the
 *     order of the triangles or the scheduling.  (The rasteriser visits a triangle's bounding box widened by a texel.)
 *   The sample of texel (px, py) with seed s (divisions and sqrt correctly rounded):
 *     r = the draw the camera ray would make: next_random(px, py, s, 0).  It is the sample's only draw here too, so every later vertex sees
 *         the random sequence it sees in a camera frame.
 *     p = (px + 0.5 + (r.x - 0.5), py + 0.5 + (r.y - 0.5))               the camera ray's jittered position
 *     uncovered texel: no ray, no primary ray counted; the sample is radiance (0, 0, 0) and, with pt_set_aov, zero AOV records: the
 *         output holds exactly (0, 0, 0, 1) and the AOV targets zeros, after any number of samples.
 *     covered texel, owner (v0, e1, e2; A, B, C):
 *     b1 = E(C, A, p) / area2,  b2 = E(A, B, p) / area2
 *     b1 = max(b1, 0),  b2 = max(b2, 0),  b0 = max((1 - b1) - b2, 0),  s = (b0 + b1) + b2,  b1 = b1 / s,  b2 = b2 / s      (a jitter outside
 *         the triangle is clamped onto it)
 *     b1 = b1 * (1 - 2^-10) + (float)(2^-10 / 3), b2 likewise          strictly inside, so that the ray cannot slip past an edge
 *     P  = (v0 + b1 * e1) + b2 * e2
 *     n  = cross(e1, e2), negated for a mirrored instance;  Ng = n / sqrt(dot(n, n)), component by component: the side the traversal
 *         reports as the front face
 *     o = P + Ng * surface_offset,  d = -Ng,  tmin = 0,  tmax = 2 * surface_offset
 *   The first closest hit is the surface itself at t ~ surface_offset, or whatever lies closer than that above it; the image holds the
 * radiance that leaves each texel along its front normal under the call's settings and flags -- for a diffuse surface, the lightmap.  With
 * pt_set_aov, albedo.w is the coverage, albedo.rgb demodulates the lightmap and normal_depth.w ~ surface_offset.  An ambient-occlusion map:
 * PT_FLAG_MATERIAL_DIFFUSE_WHITE, a constant white environment, max_bounces = 1, no lights.
 * The bake is a setting, like the lens: it is NOT part of the blob of pt_accum_save, whose format is unchanged -- a caller who resumes calls
 * pt_set_bake with the same config before pt_accum_load. */
typedef struct pt_bake_config {
    int32_t enable;           /* 0 = camera (default) */
    int32_t tex_coord;        /* 0 or 1: the UV set that addresses the atlas */
    int32_t instance;         /* -1 = every instance that has that UV set, else one row of the instance table */
    float   surface_offset;   /* world units, finite, > 0: the ray starts this far above the surface */
} pt_bake_config;             /* 16 bytes */
/* PT_ERR_INVALID_ARGUMENT for a NULL pointer or a bad config (checked only when enable != 0; the message names the field): the old config
 * stays and no restart is pending.  A good config forces a new accumulation on the next pt_trace, as pt_set_lens does: until that trace
 * pt_accum_save answers PT_ERR_NOT_READY, and pt_accum_load clears the pending restart. */
int pt_set_bake(pt_ctx* ctx, const pt_bake_config* config);
/* Copies the coverage map's owners out (host arrays of width * height, either may be NULL): instance_out the instance row, -1 where no
 * triangle covers; primitive_out the triangle within the instance (0xffffffff where none).  Synchronises the stream.  PT_ERR_NOT_READY
 * before the first bake trace, PT_ERR_INVALID_ARGUMENT for a size other than the map's. */
int pt_bake_coverage(pt_ctx* ctx, uint32_t width, uint32_t height, int32_t* instance_out, uint32_t* primitive_out);
/* Fills the uncovered texels of a W*H float4 device image from the coverage map of that size, in place, enqueued on the stream.  A texel
 * is `filled` if it has an owner.  In each of the `passes` (1..64) passes an unfilled texel looks at its 8 neighbours, dy = -1..1 outer,
 * dx = -1..1 inner, the centre skipped, and counts those inside the atlas that were filled at the start of the pass; with count > 0 it
 * becomes (the sequential float32 sum of those neighbours, all four channels) / (float)count and is filled from the next pass on.
 * Filled texels are never changed and unfilled ones never read as neighbours.  The scratch (one image, two masks) belongs to the context.
 * PT_ERR_INVALID_ARGUMENT, with nothing written: a NULL ctx (answered before any device call), a NULL image, a zero width or height, passes
 * outside 1..64, a size other than the map's.  PT_ERR_NOT_READY before the first bake trace. */
int pt_bake_dilate(pt_ctx* ctx, void* image, uint32_t width, uint32_t height, int passes);
/* Light-probe baking (absent upstream).  A lightmap (pt_set_bake) lights static, UV-mapped surfaces; what moves, and a raster pass, is lit
 * from light probes: the radiance that arrives at a point from every direction.  With probes on, pt_trace renders an atlas of octahedral
 * maps instead of a camera image -- one n x n map per probe position -- and pt_probe_project reduces such an atlas to nine
 * spherical-harmonic (SH) coefficients per probe and channel.  As under a bake only the first ray differs: from its first closest hit on, a
 * path is the path of a camera frame, so sample batches, tile shards, adaptive sampling, AOVs, pt_accum_save / load and pt_exchange_frame
 * apply to the atlas as to any W x H image, bit for bit.  With probes off (the default) every image, ray count and stat is what it is without
 * this section.
 *   The atlas.  rows = ceil(count / columns), W = columns * n, H = rows * n.  Pixel (px, py) lies in cell cx = px / n, cy = py / n (integer
 * division) of probe k = cy * columns + cx, at the map texel lx = px - cx * n, ly = py - cy * n.  n is a multiple of 16, so every 16 x 16
 * tile belongs to one probe: adaptive sampling retires tiles probe by probe.  A cell with k >= count holds no probe (the last row's tail).
 *   The sample of (px, py) with seed s, float32 throughout, every operation in the order written, products and sums not fused:
 *     r = the draw the camera ray would make: next_random(px, py, s, 0).  It is the sample's only draw here too, so every later vertex sees
 *         the random sequence it sees in a camera frame.
 *     u = fdiv(((float)lx + 0.5) + (r.x - 0.5), (float)n),  v likewise from ly and r.y          (r.x may be exactly 1: u = 1 on the last column)
 *     d = SquareToSphere(UvToSquare({u, v}))     the reference's equal-area octahedral map (Transforms.hlsli), that of the environment
 *         importance map; not renormalised, as the environment sample's direction is not; in world axes: the map's +z is world +z
 *     o = positions[k],  tmin = 0,  tmax = max_distance
 *     a cell without a probe: no ray, no primary ray counted; the sample is radiance (0, 0, 0) and, with pt_set_aov, zero AOV records: the
 *         output holds exactly (0, 0, 0, 1) and the AOV targets zeros, after any number of samples (what an uncovered bake texel gets).
 *   pt_trace under probes: params->width x height must be W x H, else PT_ERR_INVALID_ARGUMENT with nothing written.  Wavefront mode only: a
 * call in PT_MODE_MEGAKERNEL fails with PT_ERR_INVALID_ARGUMENT and writes nothing.  world_to_view / view_to_clip generate no rays but must
 * still be valid (identity will do) and still drive the reset comparison; the lens (pt_set_lens) does not apply; debug outputs work, the first
 * vertex being the probe ray's hit.  With pt_set_aov, normal_depth.w is the mean hit distance from the probe -- its distance map -- and
 * albedo.w the fraction of rays that hit.  Probes and a bake exclude each other: whichever is enabled second is refused.
 * Probes are a setting, like the lens and the bake: NOT part of the blob of pt_accum_save, whose format is unchanged -- a caller who resumes
 * calls pt_set_probes with the same config and positions before pt_accum_load. */
typedef struct pt_probe_config {
    int32_t enable;           /* 0 = camera (default) */
    int32_t resolution;       /* n: each probe is an n x n octahedral map; a multiple of 16 in 16..1024 */
    int32_t count;            /* K >= 1 probes */
    int32_t columns;          /* C >= 1 probes per atlas row */
    float   max_distance;     /* finite, > 0: tmax of the probe's ray */
} pt_probe_config;            /* 20 bytes */
/* positions_xyz: host array of count * 3 floats, world space; copied into an array the context owns.  PT_ERR_INVALID_ARGUMENT (the message
 * names the field or the probe index) for a NULL pointer, a bad field, a non-finite position, W or H above 2^30, or enabling probes while a
 * bake is enabled (pt_set_bake likewise refuses to enable a bake while probes are on).  All of these are checked only when enable != 0;
 * with enable == 0 nothing else of the config is looked at and positions_xyz may be NULL.  After such a refusal the old config and the old
 * positions stay and no restart is pending.  (A device error while the positions are stored -- PT_ERR_OUT_OF_MEMORY, PT_ERR_DEVICE --
 * may have cost the old positions: it leaves probes off and a restart pending.)  A good config forces a new accumulation on the next
 * pt_trace, as pt_set_bake does: until that trace pt_accum_save answers PT_ERR_NOT_READY, and pt_accum_load clears the pending restart. */
int pt_set_probes(pt_ctx* ctx, const pt_probe_config* config, const float* positions_xyz);
/* Projects every probe of a W x H float4 device atlas (width, height must be the W, H of the context's current probe layout) onto the real
 * spherical harmonics of bands 0..2: sh_host receives count * 9 * 3 floats, [probe][coefficient][rgb].  A pure function of the atlas and
 * the layout; the atlas's w channel is not read.  Synchronises the stream.  For probe k, with the texel-centre direction
 *     w(i, j) = SquareToSphere(UvToSquare({fdiv(i + 0.5, n), fdiv(j + 0.5, n)}))
 *     c[lm][ch] = (4 pi / n^2) * sum over i, j of L(i, j)[ch] * Y_lm(w(i, j))                (float32; the order of the sum is not defined)
 * Y in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), each constant rounded once to float:
 *     0.282094792    0.488602512 y    0.488602512 z    0.488602512 x    1.092548431 xy    1.092548431 yz    0.315391565 (3 z^2 - 1)
 *     1.092548431 xz    0.546274215 (x^2 - y^2)
 * A texel with a non-finite r, g or b counts as (0, 0, 0).  PT_PROBE_SH_RADIANCE gives c as written: L(w) ~ sum c_lm Y_lm(w).
 * PT_PROBE_SH_IRRADIANCE multiplies band l by pi, 2 pi / 3, pi / 4 (the clamped-cosine kernel), so that E(n) = sum c_lm Y_lm(n) is the
 * irradiance on a surface with normal n; a diffuse surface of albedo a then leaves a / pi * E(n).
 * The texel-centre quadrature is a midpoint rule: its Gram matrix sum Y Y' 4 pi / n^2 differs from the identity by at most (the largest
 * entry of |G - I|, to two digits) 9.6e-3 at n = 16, 2.4e-3 at n = 32 and 6.1e-4 at n = 64, computed on the CPU in float64 for this
 * mapping; the error is O(1 / n^2).  Callers who want SH to a part in a thousand bake at n >= 64.
 * PT_ERR_NOT_READY if no probes are set; PT_ERR_INVALID_ARGUMENT for a NULL ctx (answered before any device call), a NULL pointer, a size
 * other than W x H, a bad kind. */
enum { PT_PROBE_SH_RADIANCE = 0, PT_PROBE_SH_IRRADIANCE = 1 };
int pt_probe_project(pt_ctx* ctx, const void* atlas_device, uint32_t width, uint32_t height, int kind, float* sh_host);
/* ID mattes (absent upstream): which object or material every pixel sees, and with how much coverage -- per pixel a ranked list of
 * (id, coverage) pairs in Cryptomatte's layout, accumulated beside the output for compositors, annotation and lightmap editors.  Off by
 * default; with it off every image, ray count and stat is what it is without this section, and with it on the output, the AOV targets, the
 * ray counts and accumulated_frames are bit for bit what they are without it.
 *   Ids.  pt_matte_id(name, length) = fix(MurmurHash3_x86_32(name bytes, seed 0)), with Cryptomatte's exponent fix
 *     fix(h):  if ((h >> 23) & 0xff) is 0 or 255:  h ^= 1 << 23
 * after which an id read as a float is finite and normal, and never 0.  The id of table row i -- a row of the instance table
 * (PT_MATTE_INSTANCE) or of the material table (PT_MATTE_MATERIAL) -- is fix(ids[i]) for i < id_count, else pt_matte_id of the ASCII name
 * "instance_<i>" / "material_<i>", i in decimal without padding.  The context keeps its own device copy of the ids, which pt_trace
 * materialises for the current instance or material table (a table that grew gets the default ids for its new rows).  Bit pattern 0 means
 * "empty rank" in a layer and "miss" in a sample's record.
 *   Layout.  Layer j holds ranks 2j and 2j + 1 of each pixel as (id_2j bits, cov_2j, id_2j+1 bits, cov_2j+1): Cryptomatte's RGBA layout,
 * W * H float4, caller-owned like pt_execute_params.output.  Ids are moved and compared as 32-bit integers, never as floats; a caller
 * reinterprets the x and z channels' bits.  An empty rank is (0, +0).
 *   One sample.  For pixel p, the record h of a sample is the id of the first closest hit of the sample's first ray -- the camera ray, the
 * lens ray, the bake texel's ray or the probe's ray: the hit the AOVs describe, after the any-hit alpha test, under the call's cull flag --
 * where the hit's row is the hit triangle's instance-table row or, for PT_MATTE_MATERIAL, that row's material_id.  A miss gives h = 0; so
 * does a pixel that starts no ray (an uncovered bake texel, a probe cell without a probe).
 *   The fold.  n = the samples already in the layers, which follows the output's count (accumulated_frames + the sample's index in the
 * batch); in a call without FLAG_ACCUMULATE every sample is the first (n = 0).  float32 throughout, in the order written, not fused:
 *     n == 0:  all ranks become empty; if h != 0, rank 0 = (h, 1.0f)
 *     n  > 0:  b = fdiv(1.0f, (float)n + 1.0f)
 *              every non-empty rank:  c = c + b * (x - c),  x = 1.0f if its id == h (and h != 0), else 0.0f       (the AOVs' running mean)
 *              if h != 0 and no rank holds h:  an empty rank becomes (h, b); if NO RANK IS EMPTY THE SAMPLE'S ID IS DROPPED
 * After a call's last sample the ranks are sorted: non-empty before empty, then coverage descending, then id ascending as unsigned.  The
 * order is total, so the state after a call depends only on the multiset of pairs and a batch of S samples equals S calls one by one, bit
 * for bit.  A pixel that met more than K ids has dropped samples: its coverages then sum to LESS than its hit fraction (albedo.w of
 * pt_set_aov); a caller who sees that raises `ranks`.  Which id is dropped depends on the order of the samples, never on the batch size.
 *   Composition, as for pt_set_aov: a tile shard writes only the rank's tiles; a tile retired by adaptive sampling is not written (it
 * equals the uniform matte after its own count); a call with a debug output, or one past max_accumulated_frames, leaves the layers
 * untouched.  Wavefront mode only: a matte call in PT_MODE_MEGAKERNEL fails with PT_ERR_INVALID_ARGUMENT and writes nothing.
 *   The layers are NOT part of the blob of pt_accum_save, whose format is unchanged: they are caller-owned and, with the count, the whole
 * matte state.  A caller who resumes keeps (or restores) them and calls pt_set_matte before pt_accum_load.
 *   pt_tiles_pack, pt_tiles_unpack and pt_exchange_frame in PT_EXCHANGE_GATHER mode take a layer as any float4 image (they copy bits).
 * PT_EXCHANGE_REDUCE must not be used on a layer: it would add ids as floats. */
enum { PT_MATTE_INSTANCE = 0, PT_MATTE_MATERIAL = 1 };
#define PT_MATTE_MAX_RANKS 8
typedef struct pt_matte_config {
    int32_t enable;      /* 0 = off (default) */
    int32_t kind;        /* PT_MATTE_INSTANCE: the hit's row of the instance table; PT_MATTE_MATERIAL: that row's material_id */
    int32_t ranks;       /* K = 2, 4, 6 or 8 (id, coverage) pairs per pixel */
    int32_t id_count;    /* entries of `ids`; 0 = default ids only */
    void*   layers[4];   /* device, W*H float4 each, caller-owned like pt_execute_params.output; the first K/2 non-NULL */
} pt_matte_config;       /* 48 bytes */
/* ids: host array of id_count entries, copied (after fix); may be NULL with id_count == 0.  PT_ERR_INVALID_ARGUMENT (the message names the
 * field) for a NULL config and, checked only when enable != 0: a bad kind or ranks, a NULL layer among the first K/2, id_count < 0,
 * id_count > 0 with ids NULL.  After such a refusal the old config stays and no restart is pending.  A good config forces a new
 * accumulation on the next pt_trace, so that the layers and the output always hold the same samples: until that trace pt_accum_save
 * answers PT_ERR_NOT_READY, and pt_accum_load clears the pending restart. */
int      pt_set_matte(pt_ctx* ctx, const pt_matte_config* config, const uint32_t* ids);
/* Cryptomatte's id of a name (see above).  Pure: no context, no device. */
uint32_t pt_matte_id(const char* name, size_t length);
/* The anti-aliased mask of a set of ids: per pixel, mask = the sequential float32 sum, over ranks 0 .. K - 1 in this order and starting from
 * 0.0f, of cov_r where id_r is among fix(ids[0 .. id_count - 1]).  layers: host array of the K/2 device layers; mask: device, W * H float.
 * A pure function of the layers (no pt_trace state: it takes layers after an exchange or from a file alike), enqueued on the context's
 * stream.  PT_ERR_INVALID_ARGUMENT, with nothing written, for a NULL ctx (answered before any device call), a NULL pointer, a zero size,
 * ranks other than 2, 4, 6, 8, id_count outside 1..64. */
int      pt_matte_extract(pt_ctx* ctx, const void* const* layers, int ranks, uint32_t width, uint32_t height,
                          const uint32_t* ids, int id_count, void* mask);
/* Motion vectors and temporal reprojection (absent upstream): for each pixel, where the surface it sees was in the previous frame of an
 * animation -- the motion AOV a compositor blurs with, and the history read of a temporal filter.  Off by default; with it off every image,
 * ray count and stat is what it is without this section, and with it on the output, the AOV targets, the matte layers, every ray count and
 * accumulated_frames are bit for bit what they are without it.  Everything below is float32 in the order written, products and sums not
 * fused; fdiv is the correctly rounded division; matrices are glm column-major, M[4 * c + r].
 *   The previous pose.  pt_motion_snapshot(ctx, take != 0) builds or refits the acceleration structure if it is dirty (as pt_lens_focus_at
 * does) and copies, for every triangle packet T of the tree, (T.v0, T.e1, T.e2) -- world space, 3 float4 with w = 0, 48 bytes -- to
 *     snap[instances[T.inst].tri_offset + T.prim]
 * an instance-major address that no rebuild or reordering of the tree changes.  The array belongs to the context, has one entry per
 * triangle of the instance table, is regrown when the table grows and freed by pt_destroy or by take == 0.  The context records the
 * table's row count and every row's triangle count.  A snapshot is VALID for a trace iff the current instance table has the same row
 * count and the same per-row triangle counts: it survives refits (moved instances, pt_buffer_update, pt_skin_run),
 * pt_accel_request_rebuild and a change of builder, and goes STALE when the triangle set changes.  With no valid snapshot the previous
 * geometry is the current geometry: right for a camera moving through a static scene, and for the first frame of a sequence.  It covers
 * rigid, skinned and morphed meshes alike.  A caller poses frame f - 1, takes the snapshot, poses frame f and traces. */
enum { PT_MOTION_SNAPSHOT_NONE = 0, PT_MOTION_SNAPSHOT_VALID = 1, PT_MOTION_SNAPSHOT_STALE = 2 };
int pt_motion_snapshot(pt_ctx* ctx, int take);
int pt_motion_snapshot_state(pt_ctx* ctx, int32_t* state_out);
/*   One sample.  A sample's first ray is the camera ray or the lens ray; its first closest hit -- the hit the AOVs describe, after the
 * any-hit alpha test, under the call's cull flag -- lies on packet T with barycentrics (u, v):
 *     Pc = (T.v0 + u * T.e1) + v * T.e2                                      componentwise
 *     S  = snap[instances[T.inst].tri_offset + T.prim] if the snapshot is valid, else T
 *     Pp = (S.v0 + u * S.e1) + v * S.e2
 *     Mc = the world_to_clip this pt_trace forms for its reset comparison;  Mp = the same routine applied to the two prev_ matrices
 *     Vc = params->world_to_view;  Vp = prev_world_to_view
 *     clip_k(M, P) = ((M[k] P.x + M[4+k] P.y) + M[8+k] P.z) + M[12+k]        k = 0, 1, 3
 *     sx(M, P) = ((fdiv(clip_0, clip_3) + 1.0f) * 0.5f) * (float)W
 *     sy(M, P) = ((1.0f - fdiv(clip_1, clip_3)) * 0.5f) * (float)H           the inverse of the pinhole ray's pixel-to-clip map
 *     z(V, P)  = -(((V[2] P.x + V[6] P.y) + V[10] P.z) + V[14])              view depth, positive in front
 *     record   = (sx(Mp, Pp) - sx(Mc, Pc),  sy(Mp, Pp) - sy(Mc, Pc),  z(Vp, Pp),  z(Vc, Pc))
 * xy is "where the point was minus where it is", in pixels: the offset at which a history image is read.  A triangle that did not move,
 * under an unchanged camera, runs the same operations on the same inputs: its record is exactly (0, 0, z, z).  Both projections go through
 * the matrices, not the pixel centre, so the jitter cancels; under a lens the point is projected through the pinhole.  record.z <= 0: the
 * point was behind the previous camera and xy is meaningless.  A miss gives zeros; so does a record with a non-finite component.
 *   The target is the running mean of its samples with the output's weights, in sample order, under the output's counts and resets (the
 * AOVs' arithmetic): a batch equals the calls one by one; a call without FLAG_ACCUMULATE leaves the one sample; a tile shard writes only
 * the rank's tiles; a tile retired by adaptive sampling is not written; a call with a debug output, or one past max_accumulated_frames,
 * leaves the target untouched.  Wavefront mode only: a motion call in PT_MODE_MEGAKERNEL, or under a bake or probes, fails with
 * PT_ERR_INVALID_ARGUMENT and writes nothing.
 *   Neither the target nor the snapshot is part of the blob of pt_accum_save, whose format is unchanged.  A caller who resumes keeps the
 * target, poses frame f - 1, takes the snapshot again and calls pt_set_motion before pt_accum_load. */
typedef struct pt_motion_config {
    int32_t enable;                 /* 0 = off (default) */
    int32_t _pad;
    void*   motion;                 /* device, W*H float4, caller-owned like pt_execute_params.output */
    float   prev_world_to_view[16];
    float   prev_view_to_clip[16];
} pt_motion_config;                 /* 144 bytes */
/* PT_ERR_INVALID_ARGUMENT for a NULL config and, when enabled, a NULL target or a non-finite matrix entry; after a refusal the old config
 * stays and no restart is pending.  A good config forces a new accumulation on the next pt_trace, as pt_set_aov does: until that trace
 * pt_accum_save answers PT_ERR_NOT_READY, and pt_accum_load clears the pending restart. */
int pt_set_motion(pt_ctx* ctx, const pt_motion_config* config);
/* The temporal filter: blends a frame with the previous frame's result read at the motion vector.  A pure function of its images, like
 * pt_denoise: it reads no pt_trace state and is enqueued on the context's stream.  color, prev_color, out_color: W*H float4; motion,
 * prev_motion: W*H float4 in the layout above (prev_motion.w is the previous frame's own view depth, so the two motion images are all the
 * geometry it needs); prev_length, out_length: W*H float, the history length (prev_length NULL = 1 everywhere).  Pixel (x, y), c = color,
 * m = motion:
 *     USABLE iff every component of m is finite, m.w > 0, m.z > 0, and s = ((float)x + m.x, (float)y + m.y) has -1 < s.x < W, -1 < s.y < H
 *     otherwise out_color = c, all four channels bit for bit, and out_length = 1
 *     x0 = floorf(s.x), fx = s.x - x0; y likewise.  Taps q = (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner,
 *     b = (i ? fx : 1 - fx) * (j ? fy : 1 - fy)
 *     a tap COUNTS iff q is in the image, prev_motion[q] is finite with .w > 0, fabsf(prev_motion[q].w - m.z) <= depth_tolerance * m.z,
 *         prev_color[q].rgb is finite, and prev_length[q] is finite and >= 1        (exclusion is a select: a NaN cannot leak)
 *     ws, hist.rgb, hl = the sequential sums of b, b * prev_color[q].rgb, b * prev_length[q] over the taps that count
 *     ws <= 0: the pixel is treated as not usable.  Otherwise
 *     hist = hist / ws;  hl = hl / ws;  n = fminf(hl + 1.0f, max_history);  a = fmaxf(fdiv(1.0f, n), alpha_min)
 *     out.rgb = hist + a * (c.rgb - hist);  out.w = c.w;  out_length = n
 * A silhouette pixel whose samples partly miss has a mean depth that matches nothing: it simply keeps its current colour -- the filter is
 * conservative there by construction.  There is no neighbourhood colour clamp, no normal test and no variance estimate.
 * PT_ERR_INVALID_ARGUMENT with nothing written for a NULL ctx (answered before any device call), a NULL required image, a zero size or one
 * above 2^30 (or W * H above 2^31 - 1), a config value out of range, out_color overlapping anything but color (which it may BE: in place),
 * out_length overlapping any input. */
typedef struct pt_reproject_config {
    float alpha_min;        /* 0..1: least weight of the current frame.  default 0.1 */
    float max_history;      /* finite, >= 1: cap of the history length.   default 32 */
    float depth_tolerance;  /* finite, > 0, relative.                      default 0.02 */
} pt_reproject_config;      /* 12 bytes */
int pt_reproject(pt_ctx* ctx, const pt_reproject_config* config /* NULL = defaults */,
                 const void* color, const void* motion,
                 const void* prev_color, const void* prev_motion, const void* prev_length /* W*H float; NULL = 1 everywhere */,
                 uint32_t width, uint32_t height, void* out_color, void* out_length /* W*H float */);
/* Motion blur (absent upstream): a shutter-time blur of a finished frame along its motion vectors, after McGuire, Hennessy, Bukowski and
 * Osman, "A Reconstruction Filter for Plausible Motion Blur" (2012).  A pure function of two images, like pt_denoise and pt_reproject: it
 * reads no pt_trace state and works on images after an exchange, after pt_denoise or pt_reproject, or loaded from a file.  color, out: W*H
 * float4; motion: W*H float4 in pt_set_motion's layout (xy = previous minus current screen position in pixels, z = previous view depth,
 * w = current view depth).  All three are caller-owned device pointers; the call is enqueued on the context's stream and is asynchronous.
 * Everything below is float32 in the order written, products and sums not fused; / is the correctly rounded division, sqrtf the correctly
 * rounded square root; clamp(a, 0, 1) = fminf(fmaxf(a, 0), 1); fract(a) = a - floorf(a).
 *   Prepare.  Pixel p = (x, y), m = motion[p], h = 0.5f * shutter (formed once, on the host):
 *     covered = isfinite(m.w) && m.w > 0;  z = covered ? m.w : +infinity                     a miss lies behind everything
 *     vx = (-m.x) * h;  vy = (-m.y) * h;  l = sqrtf(vx * vx + vy * vy)
 *     moving = covered && m.x, m.y, m.z finite && m.z > 0 && isfinite(l)
 *     if l > max_radius:  k = max_radius / l;  vx = vx * k;  vy = vy * k;  l = max_radius
 *     if not moving:  vx = vy = l = 0
 *     V[p] = (vx, vy, l, z)                                                                  V holds no NaN
 *   Tile maximum.  Tiles are PT_TILE x PT_TILE on a ceil(W/16) x ceil(H/16) grid.  T[t] = V[p*].xyz, p* the in-image pixel of tile t with
 * the largest l; on a tie the one with the least (y, x).
 *   Neighbour maximum.  r = (int)ceilf(max_radius / 16.0f), 1..4.  N[t] = T[t'] with the largest l over t' = (tx + dx, ty + dy), dy = -r..r
 * in the outer loop, dx = -r..r in the inner; only tiles inside the grid are visited; a later tile replaces the held one only if its l is
 * strictly larger.
 *   Gather.  Pixel p of tile t, (nx, ny, ln) = N[t], c = color[p]:
 *     if ln < 0.5f, or a component of c.rgb is not finite:  out[p] = c, all four channels bit for bit.  Otherwise
 *     g = jitter ? fract(52.9829189f * fract(0.06711056f * (float)x + 0.00583715f * (float)y)) : 0.5f
 *     (.., lp, zp) = V[p];  wc = 1.0f / fmaxf(lp, 0.5f);  sw = wc;  s = wc * c.rgb
 *     for tap i = 0 .. taps - 1, in order:
 *         tau = (((float)i + g) / (float)taps) * 2.0f - 1.0f
 *         qx = (int)floorf(((float)x + 0.5f) + tau * nx), qy likewise; a tap outside the image is skipped
 *         d = fabsf(tau) * ln;  (.., lq, zq) = V[q];  cq = color[q]; a tap with a non-finite cq.rgb is skipped (a select: a NaN cannot leak)
 *         zp == zq (both infinite included):  fg = bg = 1;  otherwise  e = depth_softness * fminf(zp, zq),
 *             fg = clamp(1 - (zq - zp) / e, 0, 1),  bg = clamp(1 - (zp - zq) / e, 0, 1)
 *         cone(d, l) = l > d ? 1 - d / l : 0;  cyl(d, l) = l >= d ? 1 : 0
 *         w = (fg * cone(d, lq) + bg * cone(d, lp)) + 2.0f * (cyl(d, lq) * cyl(d, lp))
 *         sw = sw + w;  s = s + w * cq.rgb
 *     out.rgb = s / sw;  out.w = c.w
 * What follows from it: a frame with no motion, or with ln < 0.5 in every tile, leaves out == color bit for bit; a tile farther than r
 * tiles from every moving pixel is copied; a static pixel none of whose counted taps lands on a moving pixel keeps its colour exactly
 * (wc = 2 and every w = 0, so (2c) / 2 = c for colours in the normal range); a moving object nearer than what is behind it spreads over
 * it; a moving object does not pull in what is in front of it.
 *   Limits.  This is a reconstruction filter, not ray-traced motion blur: in a CPU prototype an 8 x 8 block of radiance 4 moving 20 px per
 * frame over ground of radiance 0.2 kept 3.97 at its centre where an exact box exposure gives 3.2, and the image's sum rose by 12 %.
 * Pixels that miss all geometry carry no motion record, so an environment seen behind a panning camera does not blur.  The shutter is
 * centred on the frame.  Motion is taken as linear over the frame.
 *   Scratch (V: W*H float4; T, N: one float4 a tile) belongs to the context, is regrown on a change of size and freed by pt_destroy.
 * PT_ERR_INVALID_ARGUMENT with nothing written for a NULL ctx (answered before any device call), a NULL image, a zero size or one above
 * 2^30 (or W * H above 2^31 - 1), a config value out of range, out overlapping color or motion in any way (there is no in-place mode:
 * the gather reads neighbours). */
typedef struct pt_motion_blur_config {
    float   shutter;         /* finite, > 0, <= 2: the open share of the frame interval, centred on the frame.  default 0.5 */
    float   max_radius;      /* finite, 1..64: cap of the half streak, in pixels.  default 32 */
    int32_t taps;            /* 2..64 taps along the streak.  default 16 */
    int32_t jitter;          /* 0: taps at the centres of their intervals; non-zero: shifted per pixel by interleaved gradient noise.  default 1 */
    float   depth_softness;  /* finite, > 0: relative depth extent of the soft foreground test.  default 0.05 */
} pt_motion_blur_config;     /* 20 bytes */
int pt_motion_blur(pt_ctx* ctx, const pt_motion_blur_config* config /* NULL = defaults */,
                   const void* color, const void* motion, uint32_t width, uint32_t height, void* out);
/* Bloom: the reference's dual-filter bloom over a mip pyramid (Bloom::Execute, Source/Bloom.cpp:57-164, with BloomDownsample.cs.hlsl and
 * BloomUpsample.cs.hlsl; the filters are those of "Bandwidth-Efficient Rendering", Marius Bjorge).  A pure function of one image, like
 * pt_denoise and pt_motion_blur: it reads no pt_trace state.  color, out: caller-owned device pointers to W*H float4; the call is enqueued
 * on the context's stream and is asynchronous.  out == color filters in place: the last step reads only the pyramid and each lane's own
 * pixel.  Everything below is float32 in the order written, products and sums not fused; / is the correctly rounded division.
 *   Sizes.  (w_0, h_0) = (W, H);  w_k = max(w_{k-1} / 2, 1), h_k likewise (the reference's NextMipSize).  n = the number of levels
 * k = 1 .. iterations, stopping after the first level that is 1 x 1; a 1 x 1 image has n = 0.  If n = 0 or strength == 0, out = color, all
 * four channels bit for bit.
 *   Prefilter, applied to each texel of color as it is fetched (there is no level 0 in memory).  Per channel
 *     b = (c > 0) ? fminf(c, 65504.0f) : 0.0f                  a select: NaN, negatives and -0 become +0, +infinity becomes 65504
 * 65504 is the largest value of the reference's R16G16B16A16_FLOAT chain; with it no sum below can overflow.  With threshold > 0:
 *     L = fmaxf(fmaxf(b.r, b.g), b.b);  k = L > threshold ? (L - threshold) / L : 0.0f;  b = b * k
 *   Bilinear tap S(T, u, v) of a level T of w x h texels, clamp addressing:
 *     sx = u * (float)w - 0.5f;  x0f = floorf(sx);  fx = sx - x0f
 *     x0 = clamp((int)x0f, 0, w - 1);  x1 = clamp((int)x0f + 1, 0, w - 1);  y likewise
 *     a = T[y0][x0] + fx * (T[y0][x1] - T[y0][x0]);  b = the same on row y1;  S = a + fy * (b - a)
 *   Down into a level of wo x ho, pixel (x, y):
 *     u = ((float)x + 0.5f) / (float)wo, v likewise;  ox = 0.5f / (float)wo;  oy = 0.5f / (float)ho
 *     r = 4.0f * S(u, v);  then r = r + S(.) for (u + ox, v + oy), (u - ox, v - oy), (u - ox, v + oy), (u + ox, v - oy), in that order
 *     M = r / 8.0f
 * M_1 = down(prefiltered color);  M_k = down(M_{k-1}).
 *   Up into wo x ho, u and v as above, ox = 1.0f / (float)wo, oy = 1.0f / (float)ho:
 *     r = S(u + ox, v);  then + S(u - ox, v);  then + S(u, v + oy);  then + S(u, v - oy);  r = r * 2.0f
 *     then + S(u + ox, v + oy), S(u - ox, v + oy), S(u + ox, v - oy), S(u - ox, v - oy), in that order;  U = r / 12.0f
 *   Pyramid walk.  For i = n - 1 .. 1:  M_i = up(M_{i+1}).  This REPLACES M_i, as upstream does with output_scale = 0: it is the dual-filter
 * blur, not an accumulating pyramid.  Last step, at full size: U = up(M_1); a pixel with a non-finite component in c.rgb is copied, all
 * four channels bit for bit; otherwise out.rgb = c.rgb + strength * U and out.w = c.w.
 *   Against upstream.  The chain here is float32 where upstream's is half, and upstream's sampler weights are the hardware's fixed-point
 * ones, so parity with real D3D output is unpinned, as everywhere else in this project.  A non-finite pixel neither spreads nor changes.
 * Tiles another rank renders are black and darken their neighbours' glow: run it after the exchange.  float32 against the same text in
 * float64, at the defaults: 1.7e-8 to 3.2e-8 of the image's maximum on the test images (tests/test_bloom_host.py has the bound).
 *   Scratch (the chain: levels 1 .. n, one float4 a texel for 16-byte loads) belongs to the context, is regrown on a change of size and
 * freed by pt_destroy.  PT_ERR_INVALID_ARGUMENT with nothing written for a NULL ctx (answered before any device call), a NULL image, a
 * zero size or one above 2^30 (or W * H above 2^31 - 1), a config value out of range, out overlapping color without being color. */
typedef struct pt_bloom_config {
    int32_t iterations;  /* 0..8 pyramid levels; default 4 (Rasterizer.h:15 bloom_radius).  0 = out is color bit for bit */
    float   strength;    /* finite, >= 0; default 0.01 (Rasterizer.h:14).  0 = out is color bit for bit */
    float   threshold;   /* finite, >= 0; default 0 = off, as upstream, which has none */
} pt_bloom_config;       /* 12 bytes */
int pt_bloom(pt_ctx* ctx, const pt_bloom_config* config /* NULL = defaults */,
             const void* color, uint32_t width, uint32_t height, void* out);
/* The variance AOV (absent upstream): how noisy the accumulated image is, per pixel.  With a variance config enabled, pt_trace keeps, beside
 * the output, a W*H float4 target V: V.rgb is the population variance, per channel, of the samples in the pixel, V.w the population variance
 * of their channel sum (r + g) + b -- the quantity adaptive sampling's error is normalised by, so V.w carries the channels' covariance.  The
 * sample variance is V * n / (n - 1); the variance of the pixel's mean, which is what "noise" means, is V / (n - 1), n the pixel's count.
 * Everything below is float32 in the order written, products and sums not fused; fdiv is the correctly rounded division.
 *   For one pixel, x is a sample's radiance as the output blends it: after the pending environment and light records are added and after
 * the NaN / Inf paint and the luminance clamp under the call's flags.  n is the number of samples already in the pixel -- the output's
 * count: accumulated_frames plus the sample's index in the batch, or the tile's own count under adaptive sampling.  m is the output
 * pixel's rgb before this sample.
 *     n == 0:  V = (0, 0, 0, 0);  m' = x
 *     n  > 0:  b  = fdiv(1.0f, (float)n + 1.0f)
 *              d0 = x - m                      per channel
 *              m' = m + b * d0                 the output's own blend, recomputed, not written
 *              d1 = x - m'
 *              q  = d0 * d1                    per channel; a non-finite q is replaced by 0.0f (a select)
 *              V.rgb = V.rgb + b * (q - V.rgb)
 *              s0 = (d0.r + d0.g) + d0.b;  s1 = (d1.r + d1.g) + d1.b;  qs = s0 * s1   (non-finite -> 0.0f)
 *              V.w   = V.w + b * (qs - V.w)
 * This is Welford's update in running-mean form.  What follows from it: constant samples give exactly 0; a pixel with one sample holds
 * zeros; in a CPU restatement against float64 no entry was negative and the largest relative error was 6.5e-5 at n = 2 and at most 2.7e-6
 * for n = 3 .. 1024 (DESIGN.md section 4 has the table).
 *   The target follows the output's counts and resets (the AOVs' rules): a batch of S samples equals S calls one by one, bit for bit; a call
 * without FLAG_ACCUMULATE leaves zeros (a single sample has no variance); a tile shard writes only the rank's tiles; a tile retired by
 * adaptive sampling is not written and then equals the uniform target after that tile's own count; a call with a debug output, or one past
 * max_accumulated_frames, leaves the target untouched; under pt_set_bake and pt_set_probes it works as for any W x H image.  The output,
 * the AOV targets, the matte layers, the motion target, every ray count and accumulated_frames are bit for bit what they are without the
 * pass.  Wavefront mode only: a call with the pass on in PT_MODE_MEGAKERNEL fails with PT_ERR_INVALID_ARGUMENT and writes nothing.
 *   The target is caller-owned and, together with the count, the whole state: it is not part of the blob of pt_accum_save, whose format is
 * unchanged.  A caller who resumes keeps or restores the target and calls pt_set_variance before pt_accum_load.  pt_tiles_pack,
 * pt_tiles_unpack and pt_exchange_frame (both modes) take the target as any float4 image. */
typedef struct pt_variance_config {
    int32_t enable;                 /* 0 = off (default) */
    int32_t _pad;
    void*   variance;               /* device, W*H float4, caller-owned like pt_execute_params.output */
} pt_variance_config;               /* 16 bytes */
/* PT_ERR_INVALID_ARGUMENT for a NULL config and, when enabled, a NULL target; after a refusal the old config stays and no restart is
 * pending.  A good config forces a new accumulation on the next pt_trace, as pt_set_aov does: until that trace pt_accum_save answers
 * PT_ERR_NOT_READY, and pt_accum_load clears the pending restart. */
int pt_set_variance(pt_ctx* ctx, const pt_variance_config* config);
/* The noise report: the relative standard error of an accumulated image, tile by tile.  A pure function of two images and the tiles'
 * counts, like pt_probe_project: it reads no pt_trace state, and it synchronises the stream.  image: the output, W*H float4; variance: the
 * target above (or any image of that layout), both device pointers.  Tiles are PT_TILE x PT_TILE on a ceil(W/16) x ceil(H/16) grid,
 * numbered row-major.  Tile t has the count n = tile_samples[t] (a host array of global tile ids, as pt_adaptive_read returns it), or
 * `samples` everywhere if tile_samples is NULL.  For pixel p of a tile with n >= 2, I = image[p], V = variance[p]:
 *     s = (I.r + I.g) + I.b
 *     e = sqrtf(V.w / (float)(n - 1)) / (1e-4f + sqrtf(fmaxf(s, 0.0f)))          a NaN counts as +infinity
 * float32 in the order written, / the correctly rounded division, sqrtf the correctly rounded square root, fmaxf(NaN, 0) = 0.  It is the
 * standard error of the pixel's mean under adaptive sampling's own normalisation: `threshold` here and pt_adaptive_config.threshold speak
 * of the same quantity.
 *   tile_max[t] is the max of e over the tile's in-image pixels (order-free, hence exact); tile_mean[t] is their float32 sum divided by
 * their count (the order of the sum is not defined: within 256 * 2^-24 relative of any other order).  A tile with n < 2 gets -1 in both
 * arrays and is not estimated -- this is how a sharded caller passes pt_adaptive_read's zeros for the other ranks' tiles.
 *   The summary is computed on the host in double from the float32 tile values, each field rounded once; mean weights a tile's mean by its
 * in-image pixel count.  With no tile estimated, mean = max = -1.
 *   The per-tile scratch belongs to the context, is regrown on a change of size and freed by pt_destroy.  PT_ERR_INVALID_ARGUMENT with
 * nothing written for a NULL ctx (answered before any device call), a NULL image or variance, a zero size or one above 2^30 (or more than
 * 2^31 - 1 tiles), a non-finite or negative threshold, tile_samples == NULL with samples < 2. */
typedef struct pt_noise_summary {
    uint32_t tiles;                 /* ceil(W/16) * ceil(H/16) */
    uint32_t tiles_estimated;       /* tiles with a count >= 2 */
    uint32_t tiles_above;           /* estimated tiles whose max > threshold */
    float    mean;                  /* pixel-weighted mean of the estimated tiles' means */
    float    max;                   /* max of the estimated tiles' maxima */
} pt_noise_summary;                 /* 20 bytes */
int pt_noise_estimate(pt_ctx* ctx, const void* image, const void* variance, uint32_t width, uint32_t height,
                      const uint32_t* tile_samples /* host, global tile ids; NULL = `samples` everywhere */, uint32_t samples, float threshold,
                      float* tile_mean_host /* tiles floats, may be NULL */, float* tile_max_host /* likewise */,
                      pt_noise_summary* summary /* may be NULL */);
/* The denoiser steered by the variance (absent upstream): the spatial filter of SVGF (Schied et al., "Spatiotemporal Variance-Guided
 * Filtering", 2017) over an image, its first-hit AOVs and the variance target above.  The denoiser above is blind to the variance: its colour term is
 * relative to the two pixels' luminance, its sigma halves every pass, and it cannot know whether a pixel holds 2 samples or 2000 -- so it
 * blurs a converged frame and treats tiles that adaptive sampling retired at different counts alike.  Here the colour term is normalised by
 * the measured variance of the two pixels' means, and that variance is carried through every pass with the squared weights: as the image
 * gets cleaner the filter switches itself off.  One pure function of four images and the tiles' counts, like the denoiser above, pt_reproject and
 * pt_motion_blur: it reads no pt_trace state.  C = color, A = albedo, N = normal_depth, V = variance, all device pointers to W * H float4,
 * caller-owned; V has the layout pt_set_variance writes; out == color filters in place.  The pixel's count is that of its PT_TILE x PT_TILE
 * tile: tile_samples[t] (a host array of global tile ids, row-major, as pt_adaptive_read returns it), or `samples` everywhere if
 * tile_samples is NULL, as for pt_noise_estimate.  The counts are consumed before the call returns; the filter itself is enqueued on the
 * context's stream, asynchronous like pt_trace.  The scratch (two signal images and a guide image of W * H float4, one W * H float plane,
 * the tiles' counts) belongs to the context and is not the other denoiser's: reallocated when the size changes, freed by pt_destroy.
 *   All arithmetic is float32, in the order written, nothing fused; / and sqrt are correctly rounded, exp is the only function whose
 * rounding is not defined.
 *   Prepare, per pixel: a', S, n, z and cov are exactly as the denoiser above defines them.  With n_t the count of the pixel's tile and
 *     k = (float)(n_t - 1):
 *         u_c = (V.c / k) / (a'_c a'_c)   for c = r, g, b          the variance of the mean of the demodulated channel
 *         v   = (u_r + u_g) + u_b
 *     The pixel is VALID iff it is valid for the denoiser above, n_t >= 2, and v is finite and >= 0 (a NaN is invalid).  V.w is not used:
 *     demodulation is per channel, so the variance of the raw channel sum does not survive it; and for two pixels of equal mean the sum of
 *     squared channel differences has the expectation v_p + v_q whatever the channels' covariance.  An invalid pixel is never a neighbour
 *     -- by a select, not by a product -- and leaves the call with out = C, all four channels bit for bit.
 *   Pass i = 0 .. iterations - 1, step s = 2^i, on the current S and v:
 *     1. Prefilter, for a valid p: the taps are q = p + (dx, dy) at unit spacing, dx, dy in -1 .. 1, dy outer, dx inner; taps outside the
 *        image or invalid are skipped.  With k3 = (1/4, 1/2, 1/4) and g = k3[dy] k3[dx]:
 *            vt_p = (sum of g v_q) / (sum of g), the sums sequential in tap order.
 *     2. Filter: the taps, their order, h, wn and ez are the denoiser's above.  With sv2 = sigma_variance sigma_variance and d = S_p - S_q:
 *            ec = ((dr dr + dg dg) + db db) / (sv2 (vt_p + vt_q) + 1e-8);  0 when sigma_variance == 0
 *            w  = ((h[dy] h[dx]) wn) exp(-(ez + ec))
 *        and, sequential in tap order, sw += w, sc += w S_q (per channel), sv += (w w) v_q; then
 *            S'_p = sc / sw   and   v'_p = sv / (sw sw).
 *        sigma_variance does not shrink from pass to pass; the variance does.
 *   After the passes a valid pixel gets out.rgb = S a' and out.w = C.w.  iterations = 0 gives out = C bit for bit everywhere.
 *   A known limit: at 2 samples a pixel under heavy-tailed noise the variance estimate is itself too noisy to steer anything (on the
 * synthetic scene of tests/denoise_variance_ref.py: RMSE 0.106 against the other denoiser's 0.075); for frames of very few samples the denoiser
 * above remains the tool.  From 8 samples on this one is ahead, and it alone leaves a converged frame alone.
 * PT_ERR_INVALID_ARGUMENT, with nothing written: a NULL ctx (answered before any device call), a NULL image, a zero width or height, a
 * width or height above 2^30 (or more than 2^31 - 1 tiles), a config value outside the ranges below, tile_samples == NULL with samples < 2,
 * out overlapping albedo, normal_depth or variance (or color without being color). */
typedef struct pt_denoise_variance_config {
    int32_t iterations;         /* 0..6 passes; pass i taps at spacing 2^i.  default 5 */
    int32_t demodulate;         /* non-zero: filter colour / albedo', multiply back.  default 1 */
    int32_t normal_power_log2;  /* 0..10: normal weight = max(0, n_p . n_q)^(2^k) by k squarings.  default 7 */
    float   sigma_depth;        /* finite, > 0.  default 0.02 */
    float   sigma_variance;     /* finite, >= 0; 0 = colour term off.  default 4 (SVGF's luminance sigma) */
} pt_denoise_variance_config;   /* 20 bytes */
int pt_denoise_variance(pt_ctx* ctx, const pt_denoise_variance_config* config /* NULL = defaults */,
                        const void* color, const void* albedo, const void* normal_depth, const void* variance,
                        uint32_t width, uint32_t height,
                        const uint32_t* tile_samples /* host, global tile ids; NULL = `samples` everywhere */, uint32_t samples,
                        void* out);
/* Null shadow rays.  The reference traces every NEE shadow ray before it evaluates the BSDF (PathTracer.lib.hlsl:932, 948), also
 * when the sample then contributes nothing (light behind the surface, black texel, light out of range).  With culling enabled a
 * shadow ray whose weighted contribution is exactly (0,0,0) is not traced: the image is unchanged (T * 0 adds nothing), the ray
 * counts drop.  Default 0, so that rays-per-frame and Mrays/s mean what they mean for the reference. */
int pt_set_null_shadow_culling(pt_ctx* ctx, int enable);
/* Watertight triangle test.  The float ray/triangle test takes every triangle by its own vertices, so a ray within rounding of an edge or
 * vertex that two or more triangles share can be refused by all of them and pass through a closed surface (measured: 2-14 % of rays AIMED
 * at a shared edge; about one unaimed ray in 10^5 - 10^6 lies that close).  Enabled, a candidate within rounding of an edge is decided from
 * the edge's exact end points in float64, the same number for both triangles of the edge: no ray passes between them, as DXR requires.
 * Which of the two triangles such a ray hits can change with it, and a ray that leaked now hits.  Default 0: every hit is then, to the bit,
 * what it was before this call existed.  Takes effect with the next call that traces; a change of the setting restarts the accumulation, as pt_set_lens does.  No measurable
 * cost (profiles/EXPERIMENTS.md). */
int pt_set_watertight(pt_ctx* ctx, int enable);
int pt_enable_counters(pt_ctx* ctx, int enable);      /* node / triangle / tap counters (slower) */
int pt_enable_stage_timing(pt_ctx* ctx, int enable);  /* pt_stats.stage_ms: an event after every stage launch (diagnostic) */
/* Kernel arrangement (same per-vertex code, same results up to fp32 accumulation order): PT_MODE_WAVEFRONT (default) =
 * staged trace / shade / shadow kernels over SoA ray queues in HBM with ballot compaction; PT_MODE_MEGAKERNEL = one
 * lane per pixel-sample for the whole path.  stage_blocks: workgroups per wavefront stage launch (<= 0 keeps the current setting; the
 * initial setting sizes it by the launch: 1536 for a full 1080p frame, fewer for a small tile shard). */
enum { PT_MODE_WAVEFRONT = 0, PT_MODE_MEGAKERNEL = 1 };
int pt_set_kernel_mode(pt_ctx* ctx, int mode, int stage_blocks);
/* Counters accumulate over pt_trace calls since the last pt_reset_stats; the *_ms fields are the
 * hipEvent times of the most recent call of each kind. */
int pt_get_stats(pt_ctx* ctx, pt_stats* out);
int pt_reset_stats(pt_ctx* ctx);

/* Absent upstream (the reference only presents to a swapchain): offline output. */
int pt_readback(pt_ctx* ctx, const void* device_rgba32f, uint32_t width, uint32_t height, float* host_rgba32f);
/* ToneMapper::Run (Source/ToneMapper.cpp:60-91, Shaders/ToneMapper.ps.hlsl:83-101).  Writes
 * float RGB (pre-quantisation, what the parity metric uses) and/or RGBA8; either may be NULL. */
int pt_tonemap(pt_ctx* ctx, const pt_tonemap_config* config, const void* device_rgba32f,
               uint32_t width, uint32_t height, float* host_rgb32f, uint8_t* host_rgba8);

/* ---- multi-GPU: the one exchange per output frame (new capability; the reference is single-GPU) -------------
 * One process per GPU, scene replicated, rank r renders tiles t % world == r (pt_execute_params.tile_rank / tile_rank_count)
 * into ITS OWN full-size accumulation image; per reported frame pt_exchange_frame assembles the image on rank dst_rank with one
 * RCCL exchange on the context's stream (asynchronous).  RCCL is bound at run time (librccl.so.1); PT_ERR_NOT_READY if absent.
 *   PT_EXCHANGE_GATHER  own tiles packed (1/N of the image), grouped ncclSend / ncclRecv to the root over direct xGMI links,
 *                       unpacked into `frame`: bit-identical to a 1-rank frame.
 *   PT_EXCHANGE_REDUCE  ncclReduce(sum) of a zero-masked copy (own tiles, zeros elsewhere) into `frame`.
 * `local_image` is this rank's accumulation image and is only read, so accumulation composes with the exchange; `frame` is
 * written on the root only (NULL or == local_image: assemble in place over the other ranks' tiles, which the root never renders).
 * pt_exchange_unique_id: ncclGetUniqueId on one rank; the host hands the PT_EXCHANGE_ID_BYTES to every rank (file, socket, MPI,
 * torch.distributed ...).  world == 1 with unique_id NULL creates no communicator (the frame is the local image). */
#define PT_EXCHANGE_ID_BYTES 128
enum { PT_EXCHANGE_GATHER = 0, PT_EXCHANGE_REDUCE = 1 };
int pt_exchange_unique_id(void* id_out);
/* PT_OK if RCCL can be loaded in this process, PT_ERR_NOT_READY otherwise.  No GPU call, no communicator: a job lets every rank
 * probe and agree on the outcome BEFORE any rank enters pt_exchange_unique_id / pt_exchange_create (ncclCommInitRank is collective:
 * a rank that cannot load RCCL would leave the others waiting in it). */
int pt_exchange_probe(void);
int pt_exchange_create(pt_ctx* ctx, int rank, int world, const void* unique_id);
/* The same exchange for N contexts of ONE process (on one GPU or several): no RCCL, the transfers are stream-ordered
 * device-to-device copies between the contexts that joined the same `group` (any host-chosen number).  Transfers are posted, not
 * blocking: call pt_exchange_frame on the root AFTER the other ranks, every frame (PT_ERR_NOT_READY otherwise).  This is also how
 * the N > 1 logic of the exchange is tested on a one-GPU box. */
int pt_exchange_create_loopback(pt_ctx* ctx, int rank, int world, uint64_t group);
int pt_exchange_frame(pt_ctx* ctx, const void* local_image, void* frame, uint32_t width, uint32_t height, int mode, int dst_rank);
int pt_exchange_destroy(pt_ctx* ctx);
/* The transport-free halves of the gather, for hosts with their own transport (and the tests): a rank's tiles in slot order,
 * 256 float4 per 16x16 tile (pixels outside a ragged edge tile pack as zeros). */
size_t pt_tiles_packed_bytes(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count);
int pt_tiles_pack(pt_ctx* ctx, const void* image, uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count, void* packed_device);
int pt_tiles_unpack(pt_ctx* ctx, const void* packed_device, uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_rank_count, void* image);

#ifdef __cplusplus
}
#endif
#endif /* MIPT_H */
