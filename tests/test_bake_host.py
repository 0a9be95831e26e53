"""CPU-only checks of texture-space baking (include/mipt.h pt_set_bake): the calls that answer without a device and the
restatement (tests/bake_ref.py) that tests/test_gpu_bake.py holds the GPU to, on hand-worked
cases.  (The pt_bake_config mirror and the prototypes: tests/test_host_abi.py.)"""
import ctypes as C

import numpy as np

from gltf_renderer_amd import abi, renderer
from tests import bake_ref as br
from tests import hooks

f32, f64 = np.float32, np.float64


def tri(inst, prim, uv, v0=(0, 0, 0), e1=(1, 0, 0), e2=(0, 1, 0), mirrored=False):
    return br.Tri(inst, prim, [np.asarray(uv, f32), None], v0, e1, e2, mirrored)


def test_the_library_exports_the_bake_symbols_and_the_header_declares_them():
    """(The declarations against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    for name in ("pt_set_bake", "pt_bake_coverage", "pt_bake_dilate"):
        assert name in renderer.EXPORTS and hasattr(L, name), name
    assert hasattr(L, "pt_debug_bake_rays") and "pt_debug_bake_rays" not in renderer.EXPORTS      # the test hook: exported, not part of the header


def test_calls_without_a_context_return_minus_one_and_write_nothing():
    """The argument check answers before anything touches a device: this test runs where there is none."""
    L = renderer.load_library()
    cfg = abi.PtBakeConfig(1, 0, -1, 0.01)
    assert L.pt_set_bake(None, C.byref(cfg)) == -1
    inst, prim = np.full(4, 7, np.int32), np.full(4, 9, np.uint32)
    assert L.pt_bake_coverage(None, 2, 2, inst.ctypes.data_as(C.c_void_p), prim.ctypes.data_as(C.c_void_p)) == -1
    assert (inst == 7).all() and (prim == 9).all()
    img = np.full((2, 2, 4), 3.0, f32)
    assert L.pt_bake_dilate(None, img.ctypes.data_as(C.c_void_p), 2, 2, 1) == -1
    assert (img == 3.0).all()
    f = hooks.lib().pt_debug_bake_rays
    out = np.full(8, 5.0, f32)
    q = np.zeros(3, np.uint32)
    assert f(None, None, None, q.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == -1 and (out == 5.0).all()


def test_a_texel_centre_exactly_on_a_shared_edge_goes_to_the_lesser_pair():
    """A 4 x 4 atlas; two triangles share the diagonal u = v, on which the centres (k + 0.5, k + 0.5) lie exactly: E = 0 for both, both cover,
    the lesser (instance, primitive) owns -- in either order of the list, and by instance before primitive."""
    lower = [(0, 0), (1, 0), (1, 1)]           # below the diagonal (v <= u)
    upper = [(0, 0), (1, 1), (0, 1)]
    for a, b, want in (((0, 0), (0, 1), (0, 0)), ((0, 5), (1, 0), (0, 5)), ((2, 0), (1, 7), (1, 7))):
        for order in (0, 1):
            tris = [tri(*a, lower), tri(*b, upper)][:: 1 if order == 0 else -1]
            inst, prim, _ = br.coverage(tris, 4, 4)
            assert (inst >= 0).all()                                       # the two triangles tile the atlas
            for k in range(4):
                assert (inst[k, k], prim[k, k]) == want, (a, b, order, k)
            assert (inst[0, 3], prim[0, 3]) == a and (inst[3, 0], prim[3, 0]) == b      # y = 0, x = 3: v < u, the lower triangle's alone


def test_a_zero_area_uv_triangle_and_a_world_degenerate_one_are_skipped():
    full = [(0, 0), (2, 0), (0, 2)]                                        # covers the whole 4 x 4 atlas
    line = [(0, 0), (0.5, 0.5), (1, 1)]                                    # area2 == 0: on its line every edge function is 0, which would cover
    tris = [tri(0, 0, line), tri(1, 0, full)]
    inst, _, _ = br.coverage(tris, 4, 4)
    assert (inst == 1).all()
    tris = [tri(0, 0, full, e1=(1, 0, 0), e2=(2, 0, 0)), tri(1, 0, full)]  # cross(e1, e2) = 0
    inst, _, _ = br.coverage(tris, 4, 4)
    assert (inst == 1).all()
    tris = [tri(0, 0, [(0, 0), (np.inf, 0), (0, 2)]), tri(1, 0, full)]     # a non-finite coordinate
    inst, _, _ = br.coverage(tris, 4, 4)
    assert (inst == 1).all()
    inst, _, _ = br.coverage([tri(0, 0, full), tri(1, 0, full)], 4, 4, instance=1)      # one row selected
    assert (inst == 1).all()
    inst, _, _ = br.coverage([tri(0, 0, full)], 4, 4, tex_coord=1)         # no such stream
    assert (inst == -1).all()


def test_uvs_neither_wrap_nor_flip_and_fall_off_the_atlas():
    t = tri(0, 0, [(0.5, 0.5), (1.5, 0.5), (0.5, 1.5)])                    # the right angle at the atlas centre, legs running off it
    inst, _, _ = br.coverage([t], 4, 4)
    assert (inst[2:, 2:] == 0).all() and (inst[:2, :] == -1).all() and (inst[:, :2] == -1).all()     # v grows with the row y: no flip


def test_a_jitter_outside_the_triangle_is_clamped_onto_it():
    A, B, C = (0, 0), (4, 0), (0, 4)
    b0, b1, b2 = br.clamped_barycentrics(A, B, C, (-1.0, 2.0))             # left of the edge A-C: b1 = -1/4 -> 0, b2 = 1/2
    assert (b1, b2) == (f32(0), f32(0.5)) and b0 == f32(0.5)
    b0, b1, b2 = br.clamped_barycentrics(A, B, C, (3.0, 3.0))              # beyond the hypotenuse: b0 = -1/2 -> 0, renormalised
    assert b0 == 0 and (b1, b2) == (f32(0.5), f32(0.5))
    b0, b1, b2 = br.clamped_barycentrics(A, B, C, (1.0, 2.0))              # inside: unchanged
    assert (b0, b1, b2) == (f32(0.25), f32(0.25), f32(0.5))
    # the ray of a clamped sample starts above the triangle's edge, moved strictly inside by the shrink
    t = tri(0, 0, [(0, 0), (1, 0), (0, 1)], v0=(0, 0, 0), e1=(4, 0, 0), e2=(0, 4, 0))
    o, d, tmax, bo, bd = br.ray(t, 0, 4, 4, 3, 3, (f32(0.5), f32(0.5)), 0.25)           # p = (3.5, 3.5): outside
    k, c = f64(br.KEEP), f64(br.THIRD)
    assert np.allclose(o, [4 * (0.5 * k + c), 4 * (0.5 * k + c), 0.25], rtol=0, atol=1e-12)
    assert np.array_equal(d, [0, 0, -1]) and tmax == 0.5
    assert o[0] + o[1] < 4.0                                               # strictly inside the hypotenuse
    t.mirrored = True
    o, d, _, _, _ = br.ray(t, 0, 4, 4, 3, 3, (f32(0.5), f32(0.5)), 0.25)
    assert o[2] == -0.25 and np.array_equal(d, [0, 0, 1])                  # a mirrored instance's front is the other side


def test_one_dilation_pass_on_a_three_by_three_case():
    """filled: the left column.  Pass 1 fills the middle column: (1, 0) sees (0, 0), (0, 1) -- dy = -1 is out, then dy = 0: (0, 0), dy = 1: (0, 1):
    the sum in that order; (1, 1) sees all three.  The right column has no filled neighbour and keeps its bits (a NaN that must not spread)."""
    img = np.zeros((3, 3, 4), f32)
    img[:, 0] = [[1, 2, 3, 1], [3, 1e8, 5, 1], [8, -1e8, 9, 1]]
    img[:, 1] = 77.0
    img[:, 2] = np.nan
    filled = np.zeros((3, 3), bool)
    filled[:, 0] = True
    out, fill = br.dilate(img, filled, 1)
    assert np.array_equal(out[:, 0], img[:, 0])                            # filled texels are never changed
    assert np.array_equal(out[0, 1], (img[0, 0] + img[1, 0]) / f32(2))
    assert np.array_equal(out[1, 1], ((img[0, 0] + img[1, 0]) + img[2, 0]) / f32(3))
    assert out[1, 1, 1] == f32(f32(f32(2) + f32(1e8)) + f32(-1e8)) / f32(3) == 0.0      # sequential float32: 2 is lost in 1e8
    assert np.array_equal(out[2, 1], (img[1, 0] + img[2, 0]) / f32(2))
    assert np.isnan(out[:, 2]).all() and fill[:, :2].all() and not fill[:, 2].any()
    out2, fill2 = br.dilate(img, filled, 2)                                # the second pass reads the first's results, not the NaNs
    assert fill2.all() and np.isfinite(out2).all()
    assert np.array_equal(out2[0, 2], (out[0, 1] + out[1, 1]) / f32(2))
