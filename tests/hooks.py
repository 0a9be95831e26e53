"""The test hooks of libmipt.so (pt_debug_*, declared in gltf_renderer_amd/csrc/mipt_debug.h -- not part of the ABI) for ctypes, stated
once: name -> (restype, argtypes), as abi.PROTOTYPES states include/mipt.h.  lib() is the library with them bound; no test assigns an
argtypes of its own.  tests/test_host_abi.py has the compiler compare every row with the header."""
import ctypes as C

from gltf_renderer_amd import abi, renderer

HEADER = "gltf_renderer_amd/csrc/mipt_debug.h"
_vp, _ci, _u32, _sz, _f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t, C.c_float
_RAYS = (_ci, [_vp, _vp, _vp, _vp, _u32, _vp])              # (ctx, settings, params, queries or rays, n, out)
HOOKS = {
    "pt_debug_interleaved_materials": (_ci, [_vp]),
    "pt_debug_interleaved_emissive": (_ci, [_vp]),
    "pt_debug_camera_rays": _RAYS,
    "pt_debug_bake_rays": _RAYS,
    "pt_debug_probe_rays": _RAYS,
    "pt_debug_motion": _RAYS,
    "pt_debug_intersect": (_ci, [_vp, _vp, _u32, _u32, _ci, _vp]),
    "pt_debug_accel_read": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "pt_debug_accel_keys": (_ci, [_vp, _vp, _sz]),
    "pt_debug_trace_queues": (_ci, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _f32, _u32, _ci, _u32, _ci, _vp, _vp, _vp, _vp]),
    "pt_debug_sample_texture": (_ci, [_vp, _ci, _vp, _vp, _u32, _vp, _vp]),
    "pt_debug_env_query": (_ci, [_vp, _ci, _ci, _ci, _vp, _u32, _vp]),
    "pt_debug_bsdf_query": (_ci, [_vp, _ci, _ci, _u32, _vp, _u32, _vp]),
    "pt_debug_light_query": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _u32, _vp]),
    "pt_debug_surface_query": (_ci, [_vp, _ci, _ci, _u32, _vp, _u32, _vp]),
    "pt_debug_env_create_raw": (_ci, [_vp, _ci, _vp, _vp, _vp]),
    "pt_debug_env_read_blocked": (_ci, [_vp, _ci, _vp]),
    "pt_debug_math": (_ci, [_ci, _vp, _vp, _vp, _u32]),
    "pt_debug_sort_pairs": (_ci, [_vp, _vp, _sz]),
    "pt_debug_exclusive_scan": (_ci, [_vp, _sz]),
}

_BOUND = False


def lib():
    """libmipt.so (the one renderer.load_library() and every Renderer.L hold) with the hooks bound."""
    global _BOUND
    L = renderer.load_library()
    if not _BOUND:
        abi.bind(L, HOOKS, HEADER)
        _BOUND = True
    return L
