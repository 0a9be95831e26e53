// pt_debug_kernels.h -- the per-lane query hooks' kernels and launchers (pt_debug_sample_texture / env_query / bsdf_query / light_query /
// surface_query, mipt_debug.hip): ONE text, compiled twice.  debug_wf.hip includes it with PT_LUT_LDS defined, as pt_wavefront.hip's stages
// are compiled: the stage_* calls copy the tables into LDS and the query functions read them there.  debug_mk.hip includes it without, as
// pt_kernel.hip's megakernel is compiled: the stage_* calls are empty functions, every table is read from global memory and `small_tables`
// is looked at by nothing.  Internal linkage throughout; each build hands its copy to mipt_debug.hip as one DebugQueryLaunch (pt_host.h).
// In every kernel query i runs in lane i % 64 of wave i / 64, and every lane stages before any lane without a query leaves.
#include "pt_vertex.h"
#include "pt_host.h"

namespace pt {
namespace {

// pt_debug_sample_texture: the sampler, over the sRGB table and the material records.
__global__ __launch_bounds__(kBlock) void k_debug_sample_texture(SceneRec sc, const uint32_t* __restrict__ mat_slot, const float* __restrict__ tc,
                                                              uint32_t n, float* __restrict__ out, int32_t* __restrict__ taps) {
    stage_luts(sc);
    stage_materials(sc);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const vec2 uv[2] = {{tc[4 * i], tc[4 * i + 1]}, {tc[4 * i + 2], tc[4 * i + 3]}};
    int32_t t5[5];
    const vec4 r = debug_sample_query(sc, mat_slot[2 * i], (int)mat_slot[2 * i + 1], uv, t5);
    out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
    for (int c = 0; c < 5; c++) taps[5 * i + c] = t5[c];
}
void launch_debug_sample_texture(const SceneRec& sc, const uint32_t* d_mat_slot, const float* d_tc, uint32_t n, float* d_out, int32_t* d_taps, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_sample_texture, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, d_mat_slot, d_tc, n, d_out, d_taps);
}
// pt_debug_env_query: the environment light.  The one place where the two builds differ in text: the wavefront stages read the three
// coarsest level pairs of the importance pyramid from LDS of the traversal stack's type and size, staged as env_prepass stages them;
// the megakernel reads the whole pyramid from global memory.
__global__ __launch_bounds__(kBlock) void k_debug_env_query(SceneRec sc, int op, const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
#ifdef PT_LUT_LDS
    __shared__ int s_stack[kStackLds * kBlock];
    static_assert((size_t)kStackLds * kBlock * sizeof(int) >= (size_t)kImpLdsFloat4 * sizeof(float4), "the traversal stack's LDS must hold the importance pyramid's coarse levels");
    float4* top = (float4*)s_stack;
    stage_importance_top_into(sc, top);
#else
    const float4* top = importance_lds_top();
#endif
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    debug_env_query(sc, op, in + (size_t)kEnvQueryIn * i, out + (size_t)kEnvQueryOut * i, top);
}
void launch_debug_env_query(const SceneRec& sc, int op, const float* d_in, uint32_t n, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_env_query, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, op, d_in, n, d_out);
}
// pt_debug_bsdf_query: the BSDF, over the sheen table (stage_luts stages it with the sRGB table).
__global__ __launch_bounds__(kBlock) void k_debug_bsdf_query(SceneRec sc, int op, uint32_t flags, const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
    stage_luts(sc);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
#ifdef PT_LUT_LDS
    debug_bsdf_query<ParkLds>(sc, op, flags, in + (size_t)kBsdfQueryIn * i, out + (size_t)kBsdfQueryOut * i);       // the shade stage's form of the BSDF
#else
    debug_bsdf_query<ParkRegisters>(sc, op, flags, in + (size_t)kBsdfQueryIn * i, out + (size_t)kBsdfQueryOut * i);  // the megakernel's
#endif
}
void launch_debug_bsdf_query(const SceneRec& sc, int op, uint32_t flags, const float* d_in, uint32_t n, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_bsdf_query, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, op, flags, d_in, n, d_out);
}
// pt_debug_light_query: the punctual lights.  Staged: the first kLightCacheMax lights with their cone terms (stage_lights), `small_tables`
// as k_wf_shade's SMALL; unstaged, the table in global memory and the cone terms computed in place.  The host checks that small_tables
// comes with at most kLightCacheMax lights and that every index is below num_of_lights.
__global__ __launch_bounds__(kBlock) void k_debug_light_query(SceneRec sc_in, uint32_t small_tables, int num_of_lights, const uint32_t* __restrict__ index,
                                                           const float* __restrict__ p, uint32_t n, float* __restrict__ out) {
    SceneRec sc = sc_in; sc.small_tables = small_tables ? 1u : 0u;
    stage_lights(sc, num_of_lights);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    debug_light_query(sc, index[i], v3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]), out + (size_t)kLightQueryOut * i);
}
void launch_debug_light_query(const SceneRec& sc, bool small_tables, int num_of_lights, const uint32_t* d_index, const float* d_p, uint32_t n, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_light_query, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, small_tables ? 1u : 0u, num_of_lights, d_index, d_p, n, d_out);
}
// pt_debug_surface_query: the vertex fetch and the material evaluation, over the sRGB, sheen and tangent tables, the instance rows and the
// material records -- staged as k_wf_shade stages them, `small_tables` as its SMALL.  The host checks that small_tables comes with at most
// kInstCacheMax instances and kMatCacheMax materials and that every packet index is below num_tris.
__global__ __launch_bounds__(kBlock) void k_debug_surface_query(SceneRec sc_in, uint32_t small_tables, uint32_t flags, const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
    SceneRec sc = sc_in; sc.small_tables = small_tables ? 1u : 0u;
    stage_luts(sc);
    stage_tangent_lut(sc);
    stage_instances(sc);
    stage_materials(sc);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    debug_surface_query(sc, flags, in + (size_t)kSurfQueryIn * i, out + (size_t)kSurfQueryOut * i);
}
void launch_debug_surface_query(const SceneRec& sc, bool small_tables, uint32_t flags, const float* d_in, uint32_t n, float* d_out, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_debug_surface_query, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, sc, small_tables ? 1u : 0u, flags, d_in, n, d_out);
}
constexpr DebugQueryLaunch kDebugQueryLaunch = {launch_debug_sample_texture, launch_debug_env_query, launch_debug_bsdf_query, launch_debug_light_query, launch_debug_surface_query};

}  // namespace
}  // namespace pt
