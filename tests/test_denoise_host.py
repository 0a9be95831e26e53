"""CPU-only checks of pt_denoise (its config mirror and prototype: tests/test_host_abi.py): the documented defaults, the call without a
context, and the numpy restatement (tests/denoise_ref.py) that tests/test_gpu_denoise.py holds the GPU to -- its exact properties, what
it does to the noise of the synthetic scene, and its own float32 conditioning."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, renderer
from tests import denoise_ref as dr

f32, f64 = np.float32, np.float64
SEED = 3                           # the scene's random stream; the restatement alone meets the bounds below with it


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_the_config_defaults_are_the_documented_ones():
    d = abi.PtDenoiseConfig.default()
    assert (d.iterations, d.demodulate, d.normal_power_log2) == (5, 1, 7)
    assert (d.sigma_depth, d.sigma_color) == (float(f32(0.02)), 1.0)
    r = dr.Config()                                                    # the restatement's defaults are the header's
    assert (r.iterations, r.demodulate, r.normal_power_log2, r.sigma_depth, r.sigma_color) == (5, 1, 7, d.sigma_depth, d.sigma_color)


def test_the_library_exports_pt_denoise_and_the_header_declares_it():
    """(The declaration against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    assert "pt_denoise" in renderer.EXPORTS and hasattr(L, "pt_denoise")
    # no context: the argument check answers before anything touches a device
    cfg = abi.PtDenoiseConfig.default()
    assert L.pt_denoise(None, C.byref(cfg), None, None, None, 4, 4, None) == -1
    assert L.pt_denoise(None, None, C.c_void_p(16), C.c_void_p(32), C.c_void_p(48), 1, 1, C.c_void_p(64)) == -1


@pytest.fixture(scope="module")
def scene8():
    sc = dr.scene(spp=8, seed=SEED)
    sc["ref64"], sc["valid"] = dr.denoise(sc["color"], sc["albedo"], sc["normal_depth"], dtype=f64)
    sc["ref32"], v32 = dr.denoise(sc["color"], sc["albedo"], sc["normal_depth"], dtype=f32)
    assert np.array_equal(v32, sc["valid"])
    return sc


def test_the_scene_holds_what_it_is_meant_to_hold(scene8):
    c, a, v = scene8["color"], scene8["albedo"], scene8["valid"]
    assert c.shape == (40, 72, 4) and c.dtype == f32
    assert np.isnan(c).sum() == 1 and np.isposinf(c).sum() == 1
    assert np.all(c[12, 40, :3] == 0) and v[12, 40]                   # the drop-out is a valid pixel
    assert (a[..., 3] == 0).sum() >= 100 and (a[..., 3] == 0.5).sum() >= 10 and not v[a[..., 3] == 0].any()
    assert not v[5, 7] and not v[9, 50]                               # the NaN and the inf pixel
    assert np.array_equal(v, scene8["rendered"])
    assert scene8["band"].sum() >= 24 * 30


def test_invalid_pixels_keep_their_bits_and_no_finite_pixel_becomes_non_finite(scene8):
    c, v = scene8["color"], scene8["valid"]
    for out in (scene8["ref32"], scene8["ref64"].astype(f32)):
        assert same(out[~v], c[~v])
        assert same(out[..., 3], c[..., 3])
    assert scene8["ref32"].dtype == f32
    finite_in = np.all(np.isfinite(c), axis=-1)
    assert np.all(np.isfinite(scene8["ref32"][finite_in])) and np.all(np.isfinite(scene8["ref64"][finite_in]))
    assert np.all(np.isfinite(scene8["ref32"][v]))
    # the NaN and the inf are still where they were, and nowhere else
    assert np.array_equal(np.isnan(scene8["ref32"]), np.isnan(c)) and np.array_equal(np.isinf(scene8["ref32"]), np.isinf(c))
    # ... and the valid pixels did change
    assert (bits(scene8["ref32"][v][:, :3]) != bits(c[v][:, :3])).mean() > 0.9


def test_a_zero_normal_weight_is_exactly_zero():
    """Two half-images with normals (1, 0, 0) and (0, 0, 1): other colours in the right half leave the left half's result as it is, in bits."""
    for cfg in (dr.Config(), dr.Config(normal_power_log2=0), dr.Config(iterations=6, demodulate=0)):
        for dtype in (f32, f64):
            a, _ = dr.denoise(*dr.half_planes(right_scale=1.0), cfg=cfg, dtype=dtype)
            b, _ = dr.denoise(*dr.half_planes(right_scale=7.0), cfg=cfg, dtype=dtype)
            w = a.shape[1]
            assert np.array_equal(a[:, :w // 2].view(np.uint8), b[:, :w // 2].view(np.uint8))
            assert not np.array_equal(a[:, w // 2:], b[:, w // 2:])
    # with the normal term at power 1 and a slanted second normal the halves do mix: the test above is not vacuous
    c, al, nd = dr.half_planes(right_scale=1.0)
    c7 = dr.half_planes(right_scale=7.0)[0]
    nd[:, nd.shape[1] // 2:, :3] = (0.6, 0.0, 0.8)
    a, _ = dr.denoise(c, al, nd, cfg=dr.Config(normal_power_log2=0, sigma_color=0))
    b, _ = dr.denoise(c7, al, nd, cfg=dr.Config(normal_power_log2=0, sigma_color=0))
    assert not np.array_equal(a[:, :a.shape[1] // 2], b[:, :a.shape[1] // 2])


def test_zero_iterations_is_the_identity_in_bits(scene8):
    out, _ = dr.denoise(scene8["color"], scene8["albedo"], scene8["normal_depth"], cfg=dr.Config(iterations=0), dtype=f32)
    assert out.dtype == f32 and same(out, scene8["color"])
    assert np.array_equal(out.view(np.uint32), scene8["color"].view(np.uint32))      # NaN payload and all


def test_the_float64_restatement_removes_noise_and_keeps_the_shadow_edge(scene8):
    """Item (d): at 8 spp with the defaults the RMSE against the clean image falls by at least 3x, and the RMSE in the 6-pixel band around the
    shadow column, which no guide shows, does not rise."""
    m, band = scene8["rendered"], scene8["band"]
    before, after = dr.rmse(scene8["color"], scene8["clean"], m), dr.rmse(scene8["ref64"], scene8["clean"], m)
    b_before, b_after = dr.rmse(scene8["color"], scene8["clean"], band), dr.rmse(scene8["ref64"], scene8["clean"], band)
    print("rmse %.4f -> %.4f (%.2fx), shadow band %.4f -> %.4f" % (before, after, before / after, b_before, b_after))
    assert before / after >= 3.0, (before, after)
    assert b_after <= b_before, (b_before, b_after)
    # the black drop-out is filled from its neighbours
    assert np.all(np.abs(scene8["ref64"][12, 40, :3] - scene8["clean"][12, 40, :3]) <= 0.05 * scene8["clean"][12, 40, :3])
    # the shadow is still there: the column's mean stays well under the lit mean either side
    full = scene8["valid"] & (scene8["albedo"][..., 3] == 1)
    irradiance = scene8["ref64"][..., :3].sum(axis=-1) / np.where(full, scene8["albedo"][..., :3].sum(axis=-1), 1.0)
    col = np.array([irradiance[:, x][full[:, x]].mean() for x in range(40)])
    assert col[dr.SHADOW[0] + 2:dr.SHADOW[1] - 2].mean() < 0.6 * col[:dr.SHADOW[0] - 6].mean()


def test_the_float32_restatement_is_well_conditioned(scene8):
    """Item (e): E32 = max over valid pixels and channels of |ref32 - ref64| / (|ref64| + 1e-3) < 1e-5."""
    e32 = dr.rel_error(scene8["ref32"], scene8["ref64"], scene8["valid"])
    print("E32 = %.3e" % e32)
    assert 0 < e32 < 1e-5, e32


def test_steps_reach_as_far_as_they_should():
    """An impulse on a flat guide: after pass i alone (iterations = i + 1 minus what came before is not separable, so: one pass at a time
    through one_pass) the support is the 5 x 5 comb of spacing 2^i, with the weights h[dy] h[dx] up to the colour term switched off."""
    h, w = 80, 80
    S = np.zeros((h, w, 3), f64); S[40, 40] = 1.0
    n = np.zeros((h, w, 3), f64); n[..., 2] = 1.0
    z = np.full((h, w), 2.0)
    valid = np.ones((h, w), bool)
    cfg = dr.Config(sigma_color=0)
    for i in range(6):
        out = dr.one_pass(S, n, z, valid, i, cfg, f64)
        s = 1 << i
        ys, xs = np.nonzero(out[..., 0])
        assert sorted(set(ys.tolist())) == [40 + s * d for d in range(-2, 3) if 0 <= 40 + s * d < h], i
        assert sorted(set(xs.tolist())) == [40 + s * d for d in range(-2, 3) if 0 <= 40 + s * d < w], i
        if 40 + 4 * s < h:                                           # every pixel of the comb sees all of its own 25 taps
            want = np.outer(dr.H5, dr.H5)
            got = out[40 - 2 * s:40 + 2 * s + 1:s, 40 - 2 * s:40 + 2 * s + 1:s, 0]
            assert np.allclose(got, want, rtol=1e-12), i
