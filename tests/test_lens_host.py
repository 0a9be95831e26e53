"""CPU-only checks of the thin lens (include/mipt.h pt_set_lens): the float64 restatement (tests/lens_ref.py) that tests/test_gpu_lens.py
holds the GPU to.  (The pt_lens_config mirror and the prototypes: tests/test_host_abi.py.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, renderer
from tests import lens_ref as lr

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 72, 40


def test_the_library_exports_the_lens_symbols_and_the_header_declares_them():
    """(The declarations against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    for name in ("pt_set_lens", "pt_lens_focus_at"):
        assert name in renderer.EXPORTS and hasattr(L, name), name
    # no context: the argument check answers before anything touches a device
    cfg = abi.PtLensConfig(0, 0.0, 1.0, 0, 0.0)
    assert L.pt_set_lens(None, C.byref(cfg)) == -1
    out = C.c_float(7.0)
    assert L.pt_lens_focus_at(None, None, None, 1.0, 1.0, C.byref(out)) == -1 and out.value == 7.0


def uniforms(n, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.random(n, dtype=f32), rng.random(n, dtype=f32)
    u[:4], v[:4] = (0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0)          # the corners of the unit square: next_random can return exactly 1 (quirk q17)
    return u, v


def test_disc_samples_lie_within_the_radius_and_fill_it():
    u, v = uniforms(100_000, 1)
    L = lr.disk_sample(u, v)
    r = np.sqrt((L ** 2).sum(axis=1))
    assert r.max() <= 1.0 + 1e-12
    assert r.max() > 0.999 and (r < 0.05).any()
    assert np.abs(L.mean(axis=0)).max() < 5 * 0.5 / math.sqrt(len(L))        # uniform disc: variance 1/4 per axis


@pytest.mark.parametrize("blades", [3, 5, 6, 16])
def test_polygon_samples_lie_inside_the_polygon(blades):
    rot = 0.37
    u, v = uniforms(100_000, 2 + blades)
    L = lr.polygon_sample(blades, rot, u, v)
    verts = lr.polygon_vertices(blades, rot)
    assert np.abs(np.sqrt((verts ** 2).sum(axis=1)) - 1).max() < 2.0 ** -23        # float32 roundings of unit vectors
    assert np.array_equal(verts[0], verts[blades])
    assert lr.inside_polygon(verts, L, slack=1e-12).all()
    assert not lr.inside_polygon(verts, L * 1.3, slack=1e-12).all()               # the check can fail
    assert lr.inside_polygon(verts, verts[:-1] * 0.999).all() and not lr.inside_polygon(verts, verts[:-1] * 1.001).any()


@pytest.mark.parametrize("blades", [3, 5, 6, 16])
def test_polygon_moments_match_the_analytic_ones_within_five_sigma(blades):
    """Uniformity: the first and second moments of 10^5 samples against those of the polygon; sigma is the sampling error of each mean,
    computed from the samples themselves."""
    rot = 0.37
    n = 100_000
    u, v = uniforms(n, 20 + blades)
    L = lr.polygon_sample(blades, rot, u, v)
    mean, second = lr.polygon_moments(lr.polygon_vertices(blades, rot))
    x, y = L[:, 0], L[:, 1]
    for name, sample, want in (("x", x, mean[0]), ("y", y, mean[1]), ("xx", x * x, second[0, 0]), ("yy", y * y, second[1, 1]), ("xy", x * y, second[0, 1])):
        sigma = sample.std(ddof=1) / math.sqrt(n)
        print("%d blades, E[%s]: %.6f against %.6f, sigma %.2e" % (blades, name, sample.mean(), want, sigma))
        assert abs(sample.mean() - want) <= 5 * sigma, (blades, name, sample.mean(), want, sigma)
    # a regular polygon: isotropic second moment (2 + cos(2 pi / n)) / 12 per axis, no mean, no correlation
    iso = (2 + math.cos(2 * math.pi / blades)) / 12
    assert abs(second[0, 0] - iso) < 1e-6 and abs(second[1, 1] - iso) < 1e-6 and abs(second[0, 1]) < 1e-6 and np.abs(mean).max() < 1e-6
    # a mapping that is not uniform fails: a = s - k instead of its square root crowds the centre
    bad = L * np.sqrt((L ** 2).sum(axis=1, keepdims=True))
    assert abs((bad[:, 0] ** 2).mean() - second[0, 0]) > 5 * (bad[:, 0] ** 2).std() / math.sqrt(n)


def cameras():
    w2v = camera.cm(camera.orbit_world_to_view((0, 0, 0.6), 5.0, 0.35, -0.45))
    persp = lr.Camera(w2v, camera.cm(camera.view_to_clip(W / H)), W, H)
    ortho = lr.Camera(w2v, camera.cm(camera.ortho_view_to_clip(0.25, 0.45)), W, H)
    return persp, ortho


def test_camera_vectors_are_an_orthonormal_frame_and_the_pinhole_ray_starts_on_the_near_plane():
    for cam in cameras():
        for a, b in ((cam.R, cam.U), (cam.R, cam.F), (cam.U, cam.F)):
            assert abs(float(a @ b)) < 1e-6
        for a in (cam.R, cam.U, cam.F):
            assert abs(float(a @ a) - 1) < 1e-6
        o, d, tmax = lr.pinhole_ray(cam, [0.5, 36.0, 71.5], [0.5, 20.0, 39.5])
        assert np.abs(lr.dot(o - cam.c, cam.F) - 0.01).max() < 1e-5                 # z_near
        assert np.abs(lr.dot(d, d) - 1).max() < 1e-12 and (lr.dot(d, cam.F) > 0).all()
        assert abs(float(lr.dot(d[1:2], cam.F)[0]) - 1) < 1e-6                       # the centre of the image looks along F
    o, d, _ = lr.pinhole_ray(cameras()[0], [10.0], [30.0])
    assert np.abs(o + d * (-0.01 / lr.dot(d, cameras()[0].F))[:, None] - cameras()[0].c).max() < 1e-5    # perspective: through c


@pytest.mark.parametrize("blades", [0, 5])
def test_every_lens_ray_passes_through_the_focus_point_and_starts_on_the_near_plane(blades):
    n = 20_000
    u, v = uniforms(n, 40 + blades)
    rng = np.random.default_rng(5)
    for cam in cameras():
        sx, sy = rng.random(n) * W, rng.random(n) * H
        o, d, tmax = lr.pinhole_ray(cam, sx, sy)
        L = lr.lens_sample(blades, 0.2, u, v)
        o2, d2, tmax2, P, A2, zo = lr.lens_ray(cam, o, d, tmax, L, 0.5, 2.0)
        assert np.abs(lr.dot(P - cam.c, cam.F) - 2.0).max() < 1e-9                  # P lies on the plane in focus
        assert lr.distance_to_line(P, o2, d2).max() < 1e-9
        # R, U and F are float32 roundings of an orthonormal frame: orthogonal within a few 2^-24, times the radius
        assert np.abs(lr.dot(o2 - cam.c, cam.F) - zo).max() < 1e-7
        assert np.abs(lr.dot(d2, d2) - 1).max() < 1e-12 and np.array_equal(tmax2, tmax)
        got, _ = lr.lens_point_of(cam, o2, d2, centre=lr.lens_point_of(cam, o, d)[1])
        assert np.abs(got - 0.5 * L).max() < 1e-7
        assert (np.abs(o2 - o).max(axis=1) > 0).mean() > 0.99                       # the lens moves the ray


def test_a_zero_radius_gives_the_pinhole_ray():
    cam = cameras()[0]
    o, d, tmax = lr.pinhole_ray(cam, [3.25, 50.5], [7.75, 20.5])
    o2, d2, tmax2, _, _, _ = lr.lens_ray(cam, o, d, tmax, lr.disk_sample([0.3, 0.9], [0.6, 0.1]), 0.0, 2.0)
    assert o2 is o and d2 is d and tmax2 is tmax


def test_the_quad_case_leaves_out_at_most_half_a_percent_of_the_samples(oracle_lib):
    """Item 4 of tests/test_gpu_lens.py compares hit or miss except where the restatement's ray passes within the bound of an edge: the
    share left out, from the restatement alone, for the frames and the geometry that test uses.  Also: the case is worth testing -- the quad
    is hit and missed by many samples, and the lens changes the answer for a good share of them."""
    frames = 16
    cam = lr.Camera(camera.cm(camera.orbit_world_to_view((0, 0, 0), lr.QUAD_CAMERA, 0.0, 0.0)), camera.cm(camera.view_to_clip(W / H)), W, H)
    rnd = lr.randoms(oracle_lib, W, H, range(frames))
    sx, sy = lr.jittered(rnd, W, H)
    o, d, tmax = lr.pinhole_ray(cam, sx.ravel(), sy.ravel())
    L = lr.disk_sample(rnd[..., 2].ravel(), rnd[..., 3].ravel())
    o2, d2, tmax2, P, A2, zo = lr.lens_ray(cam, o, d, tmax, L, lr.QUAD_APERTURE, lr.QUAD_FOCUS)
    slack = lr.bound(o2, cam.c[None], P, lr.QUAD_FOCUS)
    hit, near = lr.quad_coverage(o2, d2, tmax2, slack)
    hit0, _ = lr.quad_coverage(o, d, tmax, slack)
    share = float(near.mean())
    print("left out %.5f of %d samples; hit %.3f; the lens changes %.3f" % (share, len(near), hit.mean(), (hit != hit0).mean()))
    assert share <= 0.005
    assert 0.1 < hit.mean() < 0.5 and (hit != hit0).mean() > 0.02
