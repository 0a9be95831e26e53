"""Test helper: the acceleration structure as the device holds it -- pt_debug_accel_read, a test hook of libmipt.so that is not part of
include/mipt.h (csrc/mipt_debug.hip).  tests/accel_ref.py checks what it returns; accel_keys reads the sorted Morton keys of the last full
build (pt_debug_accel_keys) for tests/builder_ref.py."""
import ctypes as C
import numpy as np

from tests import hooks


def accel_read(renderer):
    """Builds or refits what is pending, then -> (info [8] uint32, nodes [wide_nodes, 64] uint8, ranges [wide_nodes, 32] uint8 or None if the
    scratch no longer holds them, tris [n_tris, 64] uint8, shade [n_tris, 128] uint8).  info: n_tris, wide_nodes, root, stack_need,
    seg_leaves, builder, fallbacks, ranges present (accel_ref.INFO_*)."""
    f = hooks.lib().pt_debug_accel_read
    vp = C.c_void_p
    info = np.zeros(8, np.uint32)

    def call(*arrays):
        rc = f(renderer.h, info.ctypes.data_as(vp), *[a.ctypes.data_as(vp) if a is not None and a.size else None for a in arrays])
        if rc != 0: raise RuntimeError("pt_debug_accel_read: %d %s" % (rc, renderer.L.pt_last_error(renderer.h).decode()))

    call(None, None, None, None)                                         # the sizes
    n, w = int(info[0]), int(info[1])
    nodes = np.zeros((w, 64), np.uint8); tris = np.zeros((n, 64), np.uint8); shade = np.zeros((n, 128), np.uint8)
    ranges = np.zeros((w, 32), np.uint8) if info[7] else None
    call(nodes, ranges, tris, shade)
    return info.copy(), nodes, ranges, tris, shade


def accel_keys(renderer):
    """Builds what is pending, then -> [n_tris] uint64, the sorted Morton keys of the last full build.  Raises RuntimeError with the library's
    message after a refit, once the scratch is released, and for fewer than two triangles."""
    f = hooks.lib().pt_debug_accel_keys
    n = int(accel_read(renderer)[0][0])
    out = np.zeros(n, np.uint64)
    rc = f(renderer.h, out.ctypes.data_as(C.c_void_p), n)
    if rc != 0: raise RuntimeError("pt_debug_accel_keys: %d %s" % (rc, renderer.L.pt_last_error(renderer.h).decode()))
    return out
