"""CPU-only checks of pt_denoise_variance (its config mirror and prototype: tests/test_host_abi.py): the size and the defaults the header
states, the call without a context, and the numpy restatement (tests/denoise_variance_ref.py) that tests/test_gpu_denoise_variance.py holds the GPU
to -- its exact properties, what it does to the noise of the synthetic scene where pt_denoise's restatement is the yardstick, and its own
float32 conditioning."""
import ctypes as C
import re

import numpy as np
import pytest

from gltf_renderer_amd import abi, renderer
from tests import denoise_ref as dr
from tests import denoise_variance_ref as dv
from tests import header_check as hc

f32, f64 = np.float32, np.float64
SEED = 3                           # the scene's random stream; the restatement alone meets the bounds below with it
W, H = 72, 40


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_config_layout_and_defaults_match_the_header():
    """The size and the defaults the header's comments state (the layout itself: tests/test_host_abi.py)."""
    body, _ = hc.typedef_struct("pt_denoise_variance_config")
    defaults = re.findall(r"default (\S+?)[ .]*(?:\(.*?\))? \*/", body)
    D = abi.PtDenoiseVarianceConfig
    assert hc.stated_bytes("pt_denoise_variance_config") == C.sizeof(D) == 20
    d = D.default()
    assert (d.iterations, d.demodulate, d.normal_power_log2) == (5, 1, 7)
    assert (d.sigma_depth, d.sigma_variance) == (float(f32(0.02)), 4.0)
    assert [float(x) for x in defaults] == [5, 1, 7, 0.02, 4], defaults          # the header's comments say the same
    r = dv.Config()                                                    # the restatement's defaults are the header's
    assert (r.iterations, r.demodulate, r.normal_power_log2, r.sigma_depth, r.sigma_variance) == (5, 1, 7, d.sigma_depth, d.sigma_variance)


def test_the_library_exports_pt_denoise_variance_and_the_header_declares_it():
    """(The declaration against the binding: tests/test_host_abi.py.)"""
    L = renderer.load_library()
    assert "pt_denoise_variance" in renderer.EXPORTS and hasattr(L, "pt_denoise_variance")
    # no context: the argument check answers before anything touches a device
    cfg = abi.PtDenoiseVarianceConfig.default()
    assert L.pt_denoise_variance(None, C.byref(cfg), None, None, None, None, 4, 4, None, 8, None) == -1
    ts = np.full(1, 8, np.uint32)
    assert L.pt_denoise_variance(None, None, C.c_void_p(16), C.c_void_p(32), C.c_void_p(48), C.c_void_p(64), 1, 1,
                                 ts.ctypes.data_as(C.c_void_p), 8, C.c_void_p(80)) == -1


# ---- what the filter does to the noise: three renderings of the scene, each with pt_denoise's float64 restatement beside it ------------
def split_counts():
    """4 samples in the tile columns left of x = 32, 64 in the rest: per-tile counts, as adaptive sampling leaves them."""
    ts = np.where(np.arange((W + dv.TILE - 1) // dv.TILE)[None, :] < 32 // dv.TILE, 4, 64) * np.ones(((H + dv.TILE - 1) // dv.TILE, 1), np.int64)
    return ts.astype(np.uint32)


CASES = dict(uniform_8=lambda: dv.pixel_counts(8, W, H), split_4_64=lambda: dv.pixel_counts(split_counts(), W, H),
             uniform_1024=lambda: dv.pixel_counts(1024, W, H))


@pytest.fixture(scope="module")
def rendered():
    out = {}
    for name, counts in CASES.items():
        sc = dv.scene(W, H, counts=counts(), seed=SEED)
        args = (sc["color"], sc["albedo"], sc["normal_depth"], sc["variance"], sc["counts"])
        sc["ref64"], sc["valid"] = dv.denoise_variance(*args, dtype=f64)
        sc["ref32"], v32 = dv.denoise_variance(*args, dtype=f32)
        assert np.array_equal(v32, sc["valid"]) and np.array_equal(sc["valid"], sc["rendered"])
        sc["old64"], _ = dr.denoise(sc["color"], sc["albedo"], sc["normal_depth"], dtype=f64)
        m, b = sc["rendered"], sc["band"]
        sc["rmse"] = {k: (dr.rmse(sc[k], sc["clean"], m), dr.rmse(sc[k], sc["clean"], b)) for k in ("color", "old64", "ref64")}
        print("%s: RMSE over the rendered pixels / the shadow band: noisy %.4f / %.4f, pt_denoise %.4f / %.4f, pt_denoise_variance %.4f / %.4f"
              % ((name,) + sc["rmse"]["color"] + sc["rmse"]["old64"] + sc["rmse"]["ref64"]))
        out[name] = sc
    return out


def test_the_scene_holds_what_it_is_meant_to_hold(rendered):
    sc = rendered["split_4_64"]
    c, a, v = sc["color"], sc["albedo"], sc["valid"]
    assert c.shape == (H, W, 4) and c.dtype == f32 and sc["variance"].dtype == f32
    assert np.isnan(c).sum() == 1 and np.isposinf(c).sum() == 1 and not v[5, 7] and not v[9, 50]
    assert (a[..., 3] == 0).sum() >= 100 and (a[..., 3] == 0.5).sum() >= 10 and not v[a[..., 3] == 0].any()
    assert np.all(sc["counts"][:, :32] == 4) and np.all(sc["counts"][:, 32:] == 64)
    assert sc["band"].sum() >= 24 * 30
    # the variance target is the population variance of the draws: over the fully covered pixels, variance / (n - 1) predicts the
    # squared error of the mean (each draw is gamma(0.5, 2) times the clean value: relative variance 2)
    full = v & (a[..., 3] == 1)
    for cols, n in ((slice(0, 32), 4), (slice(32, W), 64)):
        f = full[:, cols]
        rel = (sc["variance"][:, cols, :3][f].astype(f64) * n / (n - 1) / sc["clean"][:, cols, :3][f].astype(f64) ** 2).mean()
        assert 1.5 < rel < 2.5, (n, rel)
    # the same stream whatever the map: a pixel with 64 samples holds the same mean in both renderings that give it 64
    other = dv.scene(W, H, counts=64, seed=SEED)
    assert same(other["color"][:, 32:], c[:, 32:]) and same(other["variance"][:, 32:], sc["variance"][:, 32:])


def test_at_8_spp_it_is_no_worse_than_pt_denoise_overall_and_in_the_shadow_band(rendered):
    r = rendered["uniform_8"]["rmse"]
    assert r["ref64"][0] <= r["old64"][0], r
    assert r["ref64"][1] <= r["old64"][1], r


def test_tiles_of_4_and_64_samples_in_one_call_are_no_worse_than_pt_denoise(rendered):
    r = rendered["split_4_64"]["rmse"]
    assert r["ref64"][0] <= r["old64"][0], r


def test_a_converged_frame_is_improved_where_pt_denoise_damages_it(rendered):
    """The reason for the filter: at 1024 spp pt_denoise's restatement at its defaults raises the RMSE, this one cuts it to a quarter or less."""
    r = rendered["uniform_1024"]["rmse"]
    assert r["old64"][0] > r["color"][0], r
    assert r["ref64"][0] <= 0.25 * r["color"][0], r


def test_the_float32_restatement_is_well_conditioned(rendered):
    """E32 = max over valid pixels and channels of |ref32 - ref64| / (|ref64| + 1e-3), > 0 and < 1e-5 on each case."""
    for name, sc in rendered.items():
        e32 = dr.rel_error(sc["ref32"], sc["ref64"], sc["valid"])
        print("%s: E32 = %.3e" % (name, e32))
        assert 0 < e32 < 1e-5, (name, e32)


# ---- exact properties ---------------------------------------------------------------------------------------------------------------------
def test_invalid_pixels_keep_their_bits_and_no_finite_pixel_becomes_non_finite():
    ts = np.array([[8, 0, 8, 8, 8], [8, 8, 8, 1, 8], [8, 8, 8, 8, 8]], np.uint32)          # one tile without samples, one with a single one
    counts = dv.pixel_counts(ts, W, H)
    sc = dv.scene(W, H, counts=counts, seed=SEED)
    c = sc["color"]
    c[..., 3] = np.random.default_rng(5).random((H, W)).astype(f32)
    args = (c, sc["albedo"], sc["normal_depth"], sc["variance"], counts)
    for dtype in (f32, f64):
        out, v = dv.denoise_variance(*args, dtype=dtype)
        assert not v[0:16, 16:32].any() and not v[16:32, 48:64].any()                    # the two tiles
        assert not v[5, 7] and not v[9, 50] and not v[28:35, 3:11].any()                 # the NaN and the inf pixel, the cov == 0 block
        assert not v[sc["albedo"][..., 3] == 0].any() and v[0:16, 0:16].sum() == 255 and v[32:, 32:48].all()
        assert np.array_equal(v, sc["rendered"])
        out = out.astype(f32)
        assert same(out[~v], c[~v])
        assert same(out[..., 3], c[..., 3])
        finite_in = np.all(np.isfinite(c), axis=-1)
        assert np.all(np.isfinite(out[finite_in])) and np.all(np.isfinite(out[v]))
        assert np.array_equal(np.isnan(out), np.isnan(c)) and np.array_equal(np.isinf(out), np.isinf(c))
        assert (bits(out[v][:, :3]) != bits(c[v][:, :3])).mean() > 0.9                    # ... and the valid pixels did change
    # a variance that is negative, NaN or infinite makes its pixel invalid, and only it
    var = sc["variance"].copy()
    var[20, 20, 0], var[21, 30, 1], var[22, 40, 2] = -1.0, np.nan, np.inf
    var[23, 45, 3] = np.nan                                                              # V.w is not read
    out, v = dv.denoise_variance(c, sc["albedo"], sc["normal_depth"], var, counts)
    want = sc["rendered"].copy()
    want[20, 20] = want[21, 30] = want[22, 40] = False
    assert np.array_equal(v, want) and same(out[~v], c[~v]) and np.all(np.isfinite(out[v]))


def test_zero_iterations_is_the_identity_in_bits():
    sc = dv.scene(W, H, counts=8, seed=SEED)
    out, _ = dv.denoise_variance(sc["color"], sc["albedo"], sc["normal_depth"], sc["variance"], sc["counts"], dv.Config(iterations=0), f32)
    assert out.dtype == f32 and np.array_equal(out.view(np.uint32), sc["color"].view(np.uint32))      # NaN payload and all


def half_planes_with_variance(w=24, h=12, right_scale=1.0):
    """denoise_ref.half_planes with a variance target (the same for every right_scale) and 8 samples everywhere."""
    c, a, nd = dr.half_planes(w, h, right_scale=right_scale)
    var = (np.random.default_rng(17).random(c.shape) * 0.05 + 0.01).astype(f32)
    return c, a, nd, var, np.full(c.shape[:2], 8, np.int64)


def test_a_zero_normal_weight_is_exactly_zero():
    """Two half-images with normals (1, 0, 0) and (0, 0, 1): other colours in the right half leave the left half's colour and variance as
    they are, in bits.  What does cross the middle is the prefilter, whose nine taps are gated by validity alone: the right half's
    propagated variance depends on the right half's colours from the second pass on, and reaches vt of the left half's last column.  So
    the property is stated where the definition gives it: for one pass at any setting, and for any number of passes with the colour
    term off (the weights, and with them every variance, then do not depend on a colour)."""
    one = (dv.Config(iterations=1), dv.Config(iterations=1, normal_power_log2=0), dv.Config(iterations=1, demodulate=0, sigma_variance=1))
    off = (dv.Config(sigma_variance=0), dv.Config(sigma_variance=0, normal_power_log2=0), dv.Config(sigma_variance=0, iterations=6, demodulate=0))
    for cfg in one + off:
        for dtype in (f32, f64):
            a, _, va = dv.denoise_variance(*half_planes_with_variance(right_scale=1.0), cfg=cfg, dtype=dtype, return_variance=True)
            b, _, vb = dv.denoise_variance(*half_planes_with_variance(right_scale=7.0), cfg=cfg, dtype=dtype, return_variance=True)
            w = a.shape[1]
            assert np.array_equal(a[:, :w // 2].view(np.uint8), b[:, :w // 2].view(np.uint8))
            assert np.array_equal(va[:, :w // 2].view(np.uint8), vb[:, :w // 2].view(np.uint8))
            assert not np.array_equal(a[:, w // 2:], b[:, w // 2:])
            assert not np.array_equal(a[:, :w // 2, :3], half_planes_with_variance()[0][:, :w // 2, :3].astype(dtype))      # and it was filtered
    # with the normal term at power 1 and a slanted second normal the halves do mix: the test above is not vacuous
    c, al, nd, var, n = half_planes_with_variance()
    c7 = half_planes_with_variance(right_scale=7.0)[0]
    nd[:, nd.shape[1] // 2:, :3] = (0.6, 0.0, 0.8)
    a, _ = dv.denoise_variance(c, al, nd, var, n, cfg=dv.Config(normal_power_log2=0, sigma_variance=0))
    b, _ = dv.denoise_variance(c7, al, nd, var, n, cfg=dv.Config(normal_power_log2=0, sigma_variance=0))
    assert not np.array_equal(a[:, :a.shape[1] // 2], b[:, :a.shape[1] // 2])


def test_zero_variance_and_a_constant_colour_stay_finite_and_equal():
    """vt = 0 everywhere: the colour term's denominator is its 1e-8 alone.  Over the scene's guides a constant colour comes back finite and
    equal to itself within the E32 line of the other tests (the demodulated signal is a checker, which a zero variance forbids to mix)."""
    sc = dv.scene(W, H, counts=8, seed=SEED, specials=False)
    c = np.empty((H, W, 4), f32)
    c[...] = (0.5, 0.375, 0.25, 1.0)
    var = np.zeros((H, W, 4), f32)
    for cfg in (dv.Config(), dv.Config(demodulate=0), dv.Config(iterations=6, sigma_variance=1)):
        for dtype in (f32, f64):
            out, v, vv = dv.denoise_variance(c, sc["albedo"], sc["normal_depth"], var, sc["counts"], cfg, dtype, return_variance=True)
            assert v.sum() == (sc["albedo"][..., 3] > 0).sum() and np.all(np.isfinite(out)) and np.all(vv == 0)
            err = dr.rel_error(out, c.astype(f64), v)
            print("demodulate %d, %d passes, %s: distance from the input %.3e" % (cfg.demodulate, cfg.iterations, np.dtype(dtype).name, err))
            assert err < 1e-5, err


def test_an_impulse_of_variance_spreads_by_the_squared_weights():
    """One pass on a flat guide with the colour term off: w = h[dy] h[dx] and sw = 1, so an impulse v0 at c leaves v' = (h[dy] h[dx])^2 v0 on
    the 5 x 5 comb of spacing 2^i around c and 0 elsewhere, and a uniform variance shrinks by (sum of h^2)^2 = the sum of the comb."""
    h, w = 80, 80
    S = np.full((h, w, 3), 0.5, f64)
    n = np.zeros((h, w, 3), f64); n[..., 2] = 1.0
    z = np.full((h, w), 2.0)
    valid = np.ones((h, w), bool)
    cfg = dv.Config(sigma_variance=0)
    h4 = np.outer(dr.H5, dr.H5) ** 2
    for i in range(6):
        s = 1 << i
        v = np.zeros((h, w), f64); v[40, 40] = 3.0
        S1, v1 = dv.one_pass(S, v, n, z, valid, i, cfg, f64)
        assert np.allclose(S1, 0.5, rtol=1e-12)
        ys, xs = np.nonzero(v1)
        assert sorted(set(ys.tolist())) == [40 + s * d for d in range(-2, 3) if 0 <= 40 + s * d < h], i
        assert sorted(set(xs.tolist())) == [40 + s * d for d in range(-2, 3) if 0 <= 40 + s * d < w], i
        if 40 + 4 * s < h:                                           # every pixel of the comb sees all of its own 25 taps
            got = v1[40 - 2 * s:40 + 2 * s + 1:s, 40 - 2 * s:40 + 2 * s + 1:s]
            assert np.allclose(got, 3.0 * h4, rtol=1e-12), i
            _, flat = dv.one_pass(S, np.full((h, w), 3.0), n, z, valid, i, cfg, f64)
            assert np.isclose(flat[40, 40], 3.0 * h4.sum(), rtol=1e-12) and np.isclose(h4.sum(), sum(x * x for x in dr.H5) ** 2)
    # the prefilter: the binomial mean over the valid taps, renormalised at the border and beside an invalid pixel
    v = np.zeros((5, 5), f64); v[2, 2] = 16.0
    ok = np.ones((5, 5), bool)
    assert np.array_equal(dv.prefilter(v, ok, f64)[1:4, 1:4], np.outer((1, 2, 1), (1, 2, 1)).astype(f64))
    assert dv.prefilter(np.full((5, 5), 2.0), ok, f64)[0, 0] == 2.0
    ok[2, 2] = False
    assert np.all(dv.prefilter(v, ok, f64) == 0)
