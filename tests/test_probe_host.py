"""CPU-only checks of light-probe baking (include/mipt.h pt_set_probes, pt_probe_project): the SH kinds against the header's enum (the
pt_probe_config mirror and the prototypes: tests/test_host_abi.py), the calls that answer without a device, and the restatement (tests/probe_ref.py) that tests/test_gpu_probe.py
holds the GPU to -- its own properties: the Gram matrix of the texel-centre quadrature, a constant field, a clamped-cosine lobe, the atlas
layout, and the cube-face quadrature the end-to-end test compares with."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from gltf_renderer_amd import abi, renderer
from tests import header_check as hc
from tests import probe_ref as pr

f32, f64 = np.float32, np.float64
# max |G - I| of the texel-centre quadrature, float64; include/mipt.h states them to two digits
GRAM = {16: 9.6294e-3, 32: 2.4335e-3, 64: 6.0984e-4}


def test_the_sh_kinds_are_the_headers_enum():
    assert (abi.PROBE_SH_RADIANCE, abi.PROBE_SH_IRRADIANCE) == (0, 1)
    assert re.search(r"enum\s*\{\s*PT_PROBE_SH_RADIANCE\s*=\s*0\s*,\s*PT_PROBE_SH_IRRADIANCE\s*=\s*1\s*\}", hc.header_text())


def test_the_library_exports_the_probe_symbols_and_the_header_declares_them():
    """(The declarations against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    for name in ("pt_set_probes", "pt_probe_project"):
        assert name in renderer.EXPORTS and hasattr(L, name), name
    assert hasattr(L, "pt_debug_probe_rays") and "pt_debug_probe_rays" not in renderer.EXPORTS    # the test hook: exported, not part of the header


def test_calls_without_a_context_return_minus_one_and_write_nothing():
    """The argument check answers before anything touches a device: this test runs where there is none."""
    L = renderer.load_library()
    cfg = abi.PtProbeConfig(1, 16, 1, 1, 10.0)
    pos = np.zeros(3, f32)
    assert L.pt_set_probes(None, C.byref(cfg), pos.ctypes.data_as(C.c_void_p)) == -1
    sh = np.full(27, 5.0, f32)
    img = np.full((16, 16, 4), 3.0, f32)
    assert L.pt_probe_project(None, img.ctypes.data_as(C.c_void_p), 16, 16, 0, sh.ctypes.data_as(C.c_void_p)) == -1
    assert (sh == 5.0).all()


def test_the_header_states_the_quadratures_gram_deviation():
    text = re.sub(r"\s*\n \*\s*", " ", hc.header_text())
    for n, g in (("16", "9.6e-3"), ("32", "2.4e-3"), ("64", "6.1e-4")):
        assert (g + " at n = " + n) in text, n
        assert abs(float(g) - GRAM[int(n)]) <= 0.5 * 10.0 ** (math.floor(math.log10(GRAM[int(n)])) - 1) * 1.0001, n     # the figure to two digits


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
def test_atlas_layout():
    assert pr.atlas_size(16, 5, 2) == (32, 48)
    assert pr.atlas_size(32, 1, 1) == (32, 32)
    assert pr.atlas_size(16, 6, 3) == (48, 32)
    k, lx, ly = pr.cell(16, 2, [0, 15, 16, 31, 0, 17, 16], [0, 15, 0, 16, 47, 33, 32])
    assert k.tolist() == [0, 0, 1, 3, 4, 5, 5] and lx.tolist() == [0, 15, 0, 15, 0, 1, 0] and ly.tolist() == [0, 15, 0, 0, 15, 1, 0]


# ---- the mapping and the basis -----------------------------------------------------------------------------------------------------------
def test_the_mapping_is_the_equal_area_octahedral_map():
    """Unit directions; the square's centre is +z, its corners -z, the diagonals |s.x| + |s.y| = 1 the equator; equal area: z is uniform."""
    d = pr.centre_dirs64(64)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-7
    assert np.allclose(pr.square_to_sphere64(0.0, 0.0), [0, 0, 1]) and np.allclose(pr.square_to_sphere64(1.0, -1.0), [0, 0, -1])
    eq = pr.square_to_sphere64(np.array([0.25, -0.5, 1.0]), np.array([0.75, 0.5, 0.0]))
    assert np.abs(eq[:, 2]).max() < 1e-15 and np.allclose(np.linalg.norm(eq, axis=-1), 1)
    assert np.allclose(pr.square_to_sphere64(1.0, 0.0), [1, 0, 0], atol=1e-7) and np.allclose(pr.square_to_sphere64(0.0, 1.0), [0, 1, 0], atol=1e-7)
    z = np.sort(d[..., 2].ravel())
    assert np.abs(z - np.linspace(-1, 1, z.size)).max() < 2.0 / 64                       # the quantiles of a uniform z
    # uv = (0, 0) is the square's corner (-1, 1); +u is +x of the square, +v is -y
    sx, sy = pr.uv_to_square32(f32(0.75), f32(0.25))
    assert (sx, sy) == (0.5, 0.5)


def test_the_basis_is_orthonormal_under_a_fine_quadrature():
    assert pr.gram_deviation(512) < 1.1e-5                                              # O(1 / n^2): 9.6e-3 / 32^2
    Y = pr.sh_basis(np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    assert np.allclose(Y[0], [0.282094792, 0, 0.488602512, 0, 0, 0, 2 * 0.315391565, 0, 0], atol=1e-7)
    assert np.allclose(Y[1], [0.282094792, 0, 0, 0.488602512, 0, 0, -0.315391565, 0, 0.546274215], atol=1e-7)
    assert np.allclose(Y[2], [0.282094792, 0.488602512, 0, 0, 0, 0, -0.315391565, 0, -0.546274215], atol=1e-7)


@pytest.mark.parametrize("n", [16, 32, 64])
def test_gram_deviation_is_what_the_header_states(n):
    g = pr.gram_deviation(n)
    print("n = %d: max |G - I| = %.4e" % (n, g))
    assert abs(g - GRAM[n]) <= 0.01 * GRAM[n], (n, g)


@pytest.mark.parametrize("n", [16, 32, 64])
def test_a_constant_field(n):
    """c00 = 2 sqrt(pi) L to rounding (the map is equal-area: the weights sum to 4 pi exactly).  Every other coefficient is
    L * G[lm, 00] / Y00, so it is bounded by the Gram deviation times L / Y00 = 2 sqrt(pi) L."""
    L = 0.75
    c = pr.project_map(np.full((n, n, 3), L), pr.centre_dirs64(n))
    assert np.abs(c[0] - 2 * math.sqrt(math.pi) * L).max() < 1e-6
    assert np.abs(c[1:]).max() <= 1.01 * GRAM[n] * 2 * math.sqrt(math.pi) * L


@pytest.mark.parametrize("n,tol", [(16, 7.5e-3), (32, 1.7e-3)])
def test_a_clamped_cosine_lobe_about_a_random_axis(n, tol):
    """max(dot(w, a), 0) projects to A_l Y_lm(a).  The axis is the first of numpy's default_rng(1): 7.46e-3 at n = 16 and 1.66e-3 at n = 32.
    The figure depends on the axis -- see the sweep below."""
    a = np.random.default_rng(1).standard_normal(3)
    a /= np.linalg.norm(a)
    d = pr.centre_dirs64(n)
    c = pr.project_map(np.maximum(d @ a, 0.0)[..., None].repeat(3, -1), d)[:, 0]
    e = np.abs(c - pr.clamped_cosine_sh(a)).max()
    print("n = %d: lobe error %.3e" % (n, e))
    assert e <= tol, e


@pytest.mark.parametrize("n,tol", [(16, 1.3e-2), (32, 3.3e-3)])
def test_clamped_cosine_lobes_about_many_axes(n, tol):
    """The same over 500 axes.  The worst of them is the midpoint rule's error on a field with a kink: 1.25e-2 at n = 16 and 3.1e-3 at n = 32
    over 2000 axes (the Y20 coefficient, axes near the poles, where the map's diagonals meet), O(1 / n^2) like the Gram deviation and
    about 1.3 times it.  The bound is that figure with 5 % of room, as the reference's own error, not a property of any GPU code."""
    rng = np.random.default_rng(0)
    d = pr.centre_dirs64(n)
    Y = pr.sh_basis(d)
    worst = 0.0
    for _ in range(500):
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        c = (4.0 * math.pi / (n * n)) * np.einsum("ji,jil->l", np.maximum(d @ a, 0.0), Y)
        worst = max(worst, np.abs(c - pr.clamped_cosine_sh(a)).max())
    print("n = %d: worst lobe error %.3e" % (n, worst))
    assert 0.5 * tol < worst <= tol, worst


def test_irradiance_is_the_band_scaled_radiance_and_a_non_finite_texel_counts_as_zero():
    n = 16
    rng = np.random.default_rng(3)
    atlas = rng.uniform(0, 2, (n, 2 * n, 4))
    atlas[3, 5, 1] = np.nan
    atlas[7, 20, 0] = np.inf
    d = pr.centre_dirs64(n)
    rad, mag = pr.project_atlas(atlas, d, n, 2, 2, 0)
    irr, _ = pr.project_atlas(atlas, d, n, 2, 2, 1)
    assert np.isfinite(rad).all() and np.allclose(irr[:, 0], math.pi * rad[:, 0]) and np.allclose(irr[:, 2], 2 * math.pi / 3 * rad[:, 2]) and np.allclose(irr[:, 8], math.pi / 4 * rad[:, 8])
    clean = atlas.copy()
    clean[3, 5, :3] = 0
    clean[7, 20, :3] = 0
    assert np.array_equal(pr.project_atlas(clean, d, n, 2, 2, 0)[0], rad)
    assert np.allclose(mag, np.abs(clean[..., :3]).reshape(n, 2, n, 3).sum(axis=(0, 2)))
    assert (pr.projection_bound(n, mag) < 1e-4 * mag / (n * n) * 4 * math.pi).all()


# ---- the cube faces ----------------------------------------------------------------------------------------------------------------------
def test_cube_face_quadrature():
    """The six faces' solid angles sum to 4 pi (the formula integrates exactly to 2 pi / 3 a face; the midpoint rule at m = 32 is within 1e-3),
    the cameras' matrices put the pixel directions where cube_pixel_dirs says, and the clamped-cosine field projects to its coefficients
    within the cube grid's own midpoint error."""
    m = 32
    total = sum(pr.cube_pixel_dirs(f, m)[1].sum() for f in range(6))
    assert abs(total - 4 * math.pi) < 1e-3 * 4 * math.pi
    from gltf_renderer_amd import camera
    from tests import lens_ref as lr
    for f in range(6):
        cam = lr.Camera(camera.cm(pr.cube_world_to_view((0.3, -0.2, 0.5), f)), camera.cm(camera.view_to_clip(1.0, math.pi / 2, 0.01, 100.0)), m, m)
        i, j = np.meshgrid(np.arange(m) + 0.5, np.arange(m) + 0.5)
        o, d, _ = lr.pinhole_ray(cam, i.ravel(), j.ravel())
        assert np.abs(d.reshape(m, m, 3) - pr.cube_pixel_dirs(f, m)[0]).max() < 1e-5, f
    a = np.array([0.364, 0.864, 0.348])
    a /= np.linalg.norm(a)
    faces = [np.maximum(pr.cube_pixel_dirs(f, m)[0] @ a, 0.0)[..., None].repeat(3, -1) for f in range(6)]
    e = np.abs(pr.cube_sh(faces)[:, 0] - pr.clamped_cosine_sh(a)).max()
    print("cube quadrature, m = %d: lobe error %.3e" % (m, e))
    assert e < 2e-3
