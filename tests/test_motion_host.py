"""CPU-only checks of motion vectors and temporal reprojection (include/mipt.h pt_set_motion, pt_motion_snapshot, pt_reproject): the documented
defaults and snapshot states (the mirrors and the prototypes: tests/test_host_abi.py), the calls that answer without a device, and the restatement (tests/motion_ref.py) that
tests/test_gpu_motion.py holds the GPU to -- its own properties: an unmoved triangle under an unchanged camera gives exactly (0, 0, z, z), the
float32 record stays within the derived bound of the float64 one, and the filter's pass-through, integer-vector and rejection cases."""
import ctypes as C
import os
import re

import numpy as np

from gltf_renderer_amd import abi, camera, renderer
from tests import header_check as hc
from tests import motion_ref as mo

f32, f64, u32 = np.float32, np.float64, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def test_config_defaults_and_snapshot_states_match_the_header():
    h = hc.header_text()
    d = abi.PtReprojectConfig.defaults()
    assert (f32(d.alpha_min), f32(d.max_history), f32(d.depth_tolerance)) == (f32(0.1), f32(32.0), f32(0.02))
    assert re.search(r"PT_MOTION_SNAPSHOT_NONE\s*=\s*0\s*,\s*PT_MOTION_SNAPSHOT_VALID\s*=\s*1\s*,\s*PT_MOTION_SNAPSHOT_STALE\s*=\s*2", h)
    assert (abi.MOTION_SNAPSHOT_NONE, abi.MOTION_SNAPSHOT_VALID, abi.MOTION_SNAPSHOT_STALE) == (0, 1, 2)
    assert "conservative there by construction" in h            # the silhouette pixels: the header says what the filter does with them


def test_the_library_exports_the_motion_symbols():
    """(The declarations against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    for name in ("pt_motion_snapshot", "pt_motion_snapshot_state", "pt_set_motion", "pt_reproject"):
        assert name in renderer.EXPORTS and hasattr(L, name), name
    assert hasattr(L, "pt_debug_motion") and "pt_debug_motion" not in renderer.EXPORTS            # a hook, not part of the header


def test_calls_without_a_context_return_minus_one_and_write_nothing():
    """The argument check answers before anything touches a device: this test runs where there is none."""
    L = renderer.load_library()
    target = np.full((4, 4, 4), 3.0, f32)
    cfg = abi.PtMotionConfig()
    cfg.enable = 1
    cfg.motion = target.ctypes.data
    assert L.pt_set_motion(None, C.byref(cfg)) == -1
    assert L.pt_set_motion(None, None) == -1
    assert L.pt_motion_snapshot(None, 1) == -1 and L.pt_motion_snapshot(None, 0) == -1
    state = C.c_int32(77)
    assert L.pt_motion_snapshot_state(None, C.byref(state)) == -1 and state.value == 77
    assert L.pt_motion_snapshot_state(None, None) == -1
    img = [np.full((4, 4, 4), 2.0, f32) for _ in range(5)]
    ln = [np.full((4, 4), 9.0, f32) for _ in range(2)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pt_reproject(None, None, p(img[0]), p(img[1]), p(img[2]), p(img[3]), p(ln[0]), 4, 4, p(img[4]), p(ln[1])) == -1
    assert L.pt_reproject(None, None, None, None, None, None, None, 0, 0, None, None) == -1
    assert (img[4] == 2.0).all() and (ln[1] == 9.0).all() and (target == 3.0).all()


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def cameras(aspect, dx=0.0, yaw=0.0):
    V = camera.free_world_to_view((0.3 + dx, -6.0, 0.4), yaw, -0.05)
    P = camera.view_to_clip(aspect, np.pi / 3, 0.01, 100.0)
    return camera.cm(V), camera.cm(P)


def triangles(rng, n):
    """Object-space vertices, indices and one transform of float32 values; every triangle within a unit or so of the origin."""
    pos = rng.uniform(-1.5, 1.5, (3 * n, 3)).astype(f32)
    tri = np.arange(3 * n).reshape(n, 3)
    T = camera.trs((0.25, 0.5, -0.125), (0.0, 0.0, np.sin(0.2), np.cos(0.2)), (1.5, 0.75, 1.25)).astype(f32)
    return pos, tri, T


def packets(pos, tri, T):
    """The tree's packets as the build forms them: mul_point in float32, left to right, then the two differences."""
    T = np.asarray(T, f32)
    p = np.asarray(pos, f32)[tri]
    w = np.stack([((T[i, 0] * p[..., 0] + T[i, 1] * p[..., 1]) + T[i, 2] * p[..., 2]) + T[i, 3] for i in range(3)], axis=-1).astype(f32)
    return w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]


def test_an_unmoved_triangle_under_an_unchanged_camera_gives_exactly_zero_zero_z_z():
    rng = np.random.default_rng(5)
    pos, tri, T = triangles(rng, 500)
    cur = packets(pos, tri, T)
    u = rng.random(500).astype(f32); v = (rng.random(500) * (1 - u)).astype(f32)
    for W, H in ((40, 24), (17, 33)):
        Vc, Pc = cameras(W / H)
        M = mo.world_to_clip(Pc, Vc)
        rec = mo.record(cur, cur, u, v, M, M, Vc, Vc, W, H, f32)
        assert rec.dtype == f32
        assert np.all(bits(rec[:, 0]) == 0) and np.all(bits(rec[:, 1]) == 0)                 # +0.0, not merely == 0
        assert np.array_equal(bits(rec[:, 2]), bits(rec[:, 3])) and np.all(rec[:, 2] > 3.0)
    # a point behind the previous camera: z <= 0 flags it; a record with a non-finite component is all zeros
    Vb, Pb = cameras(1.0, yaw=np.pi)
    rec = mo.record(cur, cur, u, v, M, mo.world_to_clip(Pb, Vb), Vc, Vb, 17, 33, f32)
    assert np.all(rec[:, 2] < 0) and np.all(rec[:, 3] > 0)
    nan_cur = tuple(a.copy() for a in cur); nan_cur[1][7, 1] = np.nan
    rec = mo.record(nan_cur, cur, u, v, M, M, Vc, Vc, 17, 33, f32)
    assert np.all(bits(rec[7]) == 0) and np.all(rec[6, 2:] > 0)


def test_the_float32_record_stays_within_the_derived_bound_of_the_float64_one():
    """The float64 reference starts from the object-space vertices, the float32 one from packets formed as the build forms them."""
    rng = np.random.default_rng(6)
    pos, tri, T = triangles(rng, 4000)
    T2 = (camera.translate((0.3, -0.2, 0.1)) @ T.astype(f64)).astype(f32)                    # the previous pose: the instance elsewhere
    pos2 = (pos + rng.uniform(-0.05, 0.05, pos.shape)).astype(f32)                            # ... and its vertices rewritten
    cur, prev = packets(pos, tri, T), packets(pos2, tri, T2)
    u = rng.random(4000).astype(f32); v = (rng.random(4000) * (1 - u)).astype(f32)
    worst = 0.0
    for W, H in ((40, 24), (17, 33)):
        Vc, Pc = cameras(W / H)
        Vp, Pp = cameras(W / H, dx=0.4, yaw=0.1)
        Mc, Mp = mo.world_to_clip(Pc, Vc), mo.world_to_clip(Pp, Vp)
        got = mo.record(cur, prev, u, v, Mc, Mp, Vc, Vp, W, H, f32)
        P1, S1 = mo.world_points(pos, T, tri, u, v)
        P0, S0 = mo.world_points(pos2, T2, tri, u, v)
        assert mo.clip_w(Mc, P1).min() > 2.0 and mo.clip_w(Mp, P0).min() > 2.0               # in front of both cameras by a clear margin
        want = mo.record_points(P1, P0, Mc, Mp, Vc, Vp, W, H)
        bound = mo.record_bound(P1, S1, P0, S0, Mc, Mp, Vc, Vp, W, H, want)
        err = np.abs(got.astype(f64) - want)
        assert np.all(err <= bound), (err / bound).max()
        worst = max(worst, (err / bound).max())
        assert bound[:, :2].max() < 2e-3 and bound[:, 2:].max() < 2e-5                        # the bound itself says something: well under a pixel
        assert np.abs(want[:, :2]).max() > 1.0                                               # and the poses differ by whole pixels
    print("largest error / bound: %.3f" % worst)


def test_world_to_clip_is_the_float32_product_in_the_stated_order():
    Vc, Pc = cameras(40 / 24)
    M = mo.world_to_clip(Pc, Vc)
    exact = (camera.from_cm(Pc) @ camera.from_cm(Vc))
    assert M.dtype == f32 and np.allclose(camera.from_cm(M), exact, rtol=0, atol=4 * 2.0 ** -24 * np.abs(camera.from_cm(Pc)) @ np.abs(camera.from_cm(Vc)) + 1e-30)


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
def frame(rng, W, H):
    color = rng.random((H, W, 4)).astype(f32)
    motion = np.zeros((H, W, 4), f32)
    motion[..., 2] = motion[..., 3] = (5.0 + rng.random((H, W))).astype(f32)
    return color, motion


def test_filter_restatement_pass_through_integer_vectors_and_rejections():
    rng = np.random.default_rng(7)
    W, H = 17, 33
    c, m = frame(rng, W, H)
    pc, pm = frame(rng, W, H)
    pm[..., 3] = m[..., 2]                                              # the previous frame's own depth agrees everywhere
    # zero vectors, no history: n = 2, a = 1 / 2 exactly
    out, ln, used = mo.reproject(c, m, pc, pm)
    assert used.all() and np.all(ln == 2.0)
    assert np.array_equal(bits(out[..., :3]), bits(pc[..., :3] + f32(0.5) * (c[..., :3] - pc[..., :3]))) and np.array_equal(bits(out[..., 3]), bits(c[..., 3]))
    # an integer vector reads one texel; the pixels it carries off the image pass through, all four channels bit for bit
    m2 = m.copy(); m2[..., 0] = 3.0; m2[..., 1] = -2.0
    pm2 = np.roll(pm, (2, -3), axis=(0, 1))                             # irrelevant where depths agree: make them agree at the read position
    pm2[..., 3] = 0
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    inside = (xs + 3 < W) & (ys - 2 >= 0)
    pm2[np.clip(ys - 2, 0, H - 1), np.clip(xs + 3, 0, W - 1), 3] = np.where(inside, m2[..., 2], 0)
    out, ln, used = mo.reproject(c, m2, pc, pm2, prev_length=np.full((H, W), 40.0, f32), max_history=8.0, alpha_min=0.25)
    # (a read position that another pixel's depth overwrote may fail the depth test: only the pixels that blended are held to the value)
    assert np.array_equal(used & ~inside, np.zeros((H, W), bool)) and used.sum() > W * H // 2
    src = pc[np.clip(ys - 2, 0, H - 1), np.clip(xs + 3, 0, W - 1), :3]
    assert np.array_equal(bits(out[..., :3][used]), bits((src + f32(0.25) * (c[..., :3] - src))[used])) and np.all(ln[used] == 8.0)
    assert np.array_equal(bits(out[~used]), bits(c[~used])) and np.all(ln[~used] == 1.0)
    # every reason to reject, one pixel each; a NaN in a rejected tap does not leak
    m3, pm3, pc3, pl3 = m.copy(), pm.copy(), pc.copy(), np.full((H, W), 3.0, f32)
    m3[0, 0, 0] = np.nan; m3[1, 1, 3] = 0.0; m3[2, 2, 2] = -1.0; m3[3, 3, 0] = float(W); m3[4, 4, 1] = -5.0 - 1.0
    pm3[5, 5, 3] = m[5, 5, 2] * f32(1.5); pm3[6, 6, 1] = np.inf; pc3[7, 7, 2] = np.nan; pl3[8, 8] = 0.5; pl3[9, 9] = np.nan
    c3 = c.copy(); c3[0, 0, 1] = np.nan
    out, ln, used = mo.reproject(c3, m3, pc3, pm3, pl3)
    for k in range(10):
        assert not used[k, k] and np.array_equal(bits(out[k, k]), bits(c3[k, k])) and ln[k, k] == 1.0, k
    assert used.sum() == W * H - 10 and np.isfinite(out[used]).all() and np.all(ln[used] == 4.0)
    # a fractional vector with one of its four taps rejected renormalises over the other three
    m4 = m.copy(); m4[10, 10, 0] = 0.25; m4[10, 10, 1] = 0.5
    pm4 = pm.copy(); pm4[10:12, 10:12, 3] = m4[10, 10, 2]; pm4[11, 11, 3] = 0.0
    out, ln, used = mo.reproject(c, m4, pc, pm4)
    b = [f32(0.75) * f32(0.5), f32(0.25) * f32(0.5), f32(0.75) * f32(0.5)]
    taps = [pc[10, 10, :3], pc[10, 11, :3], pc[11, 10, :3]]
    ws = (b[0] + b[1]) + b[2]
    hist = ((b[0] * taps[0] + b[1] * taps[1]) + b[2] * taps[2]) / ws
    assert used[10, 10] and np.array_equal(bits(out[10, 10, :3]), bits(hist + f32(0.5) * (c[10, 10, :3] - hist)))


def test_render_gltf_sequence_times_and_frame_names():
    """tools/render_gltf.py --sequence T0:T1:FPS: the frame times and the numbered files."""
    import importlib.util
    import pytest
    spec = importlib.util.spec_from_file_location("render_gltf", os.path.join(ROOT, "tools", "render_gltf.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.sequence_frames("0:1:4") == [0.0, 0.25, 0.5, 0.75, 1.0] and m.sequence_frames("0.5:0.5:24") == [0.5]
    assert len(m.sequence_frames("0:2:24")) == 49 and len(m.sequence_frames("0:0.99:10")) == 10
    assert m.numbered_path("shots/a.png", 3) == "shots/a_0003.png" and m.numbered_path("a.exr", 12) == "a_0012.exr"
    for bad in ("1:0:4", "0:1:0", "0:1:-2", "0:1", "x:1:2", "0:inf:2", "0:1:nan"):
        with pytest.raises(ValueError):
            m.sequence_frames(bad)
