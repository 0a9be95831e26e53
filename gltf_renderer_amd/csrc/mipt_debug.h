/* mipt_debug.h -- the test hooks of libmipt.so (pt_debug_*), declared once.  INTERNAL: not under include/, NOT part of the ABI of
 * include/mipt.h -- a hook's parameters change whenever a test needs them to, without an ABI version.  Each hook is documented at its
 * definition (mipt_debug.hip, debug_mk.hip, sort_scan.hip); the defining files include this header, so a definition that parts from its
 * declaration does not compile (extern "C" functions cannot be overloaded).  tests/hooks.py mirrors these prototypes for ctypes and
 * tests/test_host_abi.py holds that table to this file.  Only mipt.h is included: a plain host compiler parses this file.
 * The two hooks of the diagnostic builds (pt_debug_read_timing, pt_debug_read_util: pt_wavefront.hip under PT_TIMING / PT_UTIL_PROBE) are
 * not in the library as shipped and not here. */
#ifndef MIPT_DEBUG_H
#define MIPT_DEBUG_H

#include "mipt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mipt_debug.hip */
int pt_debug_interleaved_materials(const pt_ctx* ctx);
int pt_debug_interleaved_emissive(const pt_ctx* ctx);
int pt_debug_camera_rays(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const uint32_t* queries, uint32_t n, float* out);
int pt_debug_bake_rays(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const uint32_t* queries, uint32_t n, float* out);
int pt_debug_probe_rays(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const uint32_t* queries, uint32_t n, float* out);
int pt_debug_intersect(pt_ctx* ctx, const float* rays, uint32_t n, uint32_t ray_flags, int mode, float* out);
int pt_debug_accel_read(pt_ctx* ctx, uint32_t info[8], void* nodes, void* ranges, void* tris, void* shade);
int pt_debug_accel_keys(pt_ctx* ctx, uint64_t* out, size_t n);
int pt_debug_motion(pt_ctx* ctx, const pt_settings* settings, const pt_execute_params* params, const float* rays, uint32_t n, float* out);
int pt_debug_trace_queues(pt_ctx* ctx, const float* closest, const uint32_t* closest_shard, uint32_t n_c, const float* shadow, const uint32_t* shadow_shard,
                          const uint8_t* shadow_is_light, uint32_t n_s, float shadow_tmax, uint32_t flags, int bounce, uint32_t blocks_per_shard, int which,
                          float* out_closest, float* out_shadow, uint32_t* out_cnt, uint32_t* out_stray);
int pt_debug_sample_texture(pt_ctx* ctx, int unit, const uint32_t* mat_slot, const float* tc, uint32_t n, float* out_rgba, int32_t* out_taps);
int pt_debug_env_query(pt_ctx* ctx, int env, int unit, int op, const float* in, uint32_t n, float* out);
int pt_debug_bsdf_query(pt_ctx* ctx, int unit, int op, uint32_t flags, const float* in, uint32_t n, float* out);
int pt_debug_light_query(pt_ctx* ctx, int unit, int small_tables, int num_of_lights, const uint32_t* light_index, const float* p, uint32_t n, float* out);
int pt_debug_surface_query(pt_ctx* ctx, int unit, int small_tables, uint32_t flags, const void* in, uint32_t n, float* out);
int pt_debug_env_create_raw(pt_ctx* ctx, int cube_n, const uint16_t* cube_rgba16f, const float* pyramid, int* env_out);
int pt_debug_env_read_blocked(pt_ctx* ctx, int env, float* out);

/* debug_mk.hip */
int pt_debug_math(int op, const float* a, const float* b, float* out, uint32_t n);

/* sort_scan.hip */
int pt_debug_sort_pairs(uint64_t* keys, uint32_t* vals, size_t n);
int pt_debug_exclusive_scan(uint32_t* data, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* MIPT_DEBUG_H */
