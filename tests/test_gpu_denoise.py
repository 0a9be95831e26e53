"""pt_denoise (include/mipt.h) on the MI355X against the numpy restatement tests/denoise_ref.py.

What is exact by construction is compared in bits: the invalid pixels and every alpha, iterations = 0, the locality across a zero normal
weight, determinism, the in-place call, the scratch across an adaptive trace, the argument refusals, and that pt_trace does not notice the call.  The filtered values are held to
    max over valid pixels and channels of |gpu - ref64| / (|ref64| + 1e-3)  <=  8 * E32,
E32 being the same figure of the float32 restatement, computed in the same test from the same inputs: the margin of 8 over the reference's
own float32 rounding allows the kernel its own expf (and another summation order inside the 25 taps, which it does not use); a wrong tap,
weight or step shows at 1e-3 or more.

Measured on the MI355X: NOT MEASURED yet -- every case prints E32, the kernel's figure and their ratio; the ratio belongs here and in
DESIGN.md section 4.  Rehearsed on the CPU by tools/denoise_host_rehearsal.py (the kernels' source compiled for the host, the C library's expf): 0.85 .. 1.15 on every case
below, E32 between 9e-8 (1 x 1) and 5e-7."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes
from tests import denoise_ref as dr

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, H = 72, 40                      # 5 x 3 tiles of 16 (3 x 5 blocks of 32 x 8), ragged in both directions
POISON = 7.0
ENV = (0.25, 0.5, 0.75)
MARGIN = 8.0


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def native(cfg):
    return abi.PtDenoiseConfig(cfg.iterations, cfg.demodulate, cfg.normal_power_log2, cfg.sigma_depth, cfg.sigma_color)


@pytest.fixture(scope="module")
def r():
    from gltf_renderer_amd.renderer import Renderer
    ctx = Renderer(0)
    yield ctx
    ctx.close()


def dev(r, a):
    return r.torch.from_numpy(np.ascontiguousarray(a, f32)).to("cuda:%d" % r.device)


def run(r, color, albedo, nd, cfg=None, in_place=False):
    c, a, n = dev(r, color), dev(r, albedo), dev(r, nd)
    out = r.denoise(c, a, n, out=c if in_place else None, config=native(cfg) if cfg is not None else None)
    got = r.readback(out)
    if not in_place:
        assert same(r.readback(c), color)                              # the inputs are only read
    assert same(r.readback(a), albedo) and same(r.readback(n), nd)
    return got


def synthetic(w, h):
    sc = dr.scene(w, h, spp=8, seed=3)
    rng = np.random.default_rng(w * 1000 + h)
    sc["color"][..., 3] = rng.random((h, w)).astype(f32)               # an alpha worth comparing
    return sc


def check_against_ref64(got, color, albedo, nd, cfg, label):
    ref64, valid = dr.denoise(color, albedo, nd, cfg, f64)
    ref32, _ = dr.denoise(color, albedo, nd, cfg, f32)
    e32 = dr.rel_error(ref32, ref64, valid)
    err = dr.rel_error(got, ref64, valid)
    print("%s: valid %d of %d, E32 %.3e, gpu %.3e, ratio %.2f, gpu == ref32 in %.1f %% of the valid values" % (
        label, valid.sum(), valid.size, e32, err, err / e32 if e32 else 0.0,
        100.0 * (bits(got[valid][:, :3]) == bits(ref32[valid][:, :3])).mean() if valid.any() else 100.0))
    assert same(got[~valid], color[~valid]), label                     # invalid pixels: the input, all four channels
    assert same(got[..., 3], color[..., 3]), label                     # every alpha
    finite_in = np.all(np.isfinite(color), axis=-1)
    assert np.all(np.isfinite(got[finite_in])), label
    assert err <= MARGIN * e32, (label, err, e32)
    return err, e32


VARIANTS = dict(defaults=dr.Config(), no_demodulation=dr.Config(demodulate=0), colour_term_off=dr.Config(sigma_color=0),
                normal_power_1=dr.Config(normal_power_log2=0), one_pass=dr.Config(iterations=1), two_passes=dr.Config(iterations=2),
                six_passes_wide_sigmas=dr.Config(iterations=6, normal_power_log2=10, sigma_depth=0.5, sigma_color=4.0))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_synthetic_scene_against_the_float64_restatement(r, name):
    sc = synthetic(W, H)
    assert (~sc["rendered"]).sum() > 100 and np.isnan(sc["color"]).any() and np.isinf(sc["color"]).any()
    got = run(r, sc["color"], sc["albedo"], sc["normal_depth"], VARIANTS[name])
    check_against_ref64(got, sc["color"], sc["albedo"], sc["normal_depth"], VARIANTS[name], name)


def test_null_config_means_the_defaults(r):
    sc = synthetic(W, H)
    assert same(run(r, sc["color"], sc["albedo"], sc["normal_depth"], None), run(r, sc["color"], sc["albedo"], sc["normal_depth"], dr.Config()))


@pytest.mark.parametrize("w,h", [(17, 33), (5, 3), (1, 1)])
def test_small_images_where_most_taps_fall_outside(r, w, h):
    sc = synthetic(w, h)
    cfg = dr.Config(iterations=6)
    got = run(r, sc["color"], sc["albedo"], sc["normal_depth"], cfg)
    check_against_ref64(got, sc["color"], sc["albedo"], sc["normal_depth"], cfg, "%dx%d" % (w, h))


def test_zero_iterations_is_the_identity_in_bits(r):
    sc = synthetic(W, H)
    cfg = dr.Config(iterations=0)
    assert same(run(r, sc["color"], sc["albedo"], sc["normal_depth"], cfg), sc["color"])
    assert same(run(r, sc["color"], sc["albedo"], sc["normal_depth"], cfg, in_place=True), sc["color"])


@pytest.mark.parametrize("cfg", [dr.Config(), dr.Config(normal_power_log2=0), dr.Config(iterations=6, demodulate=0)], ids=["defaults", "power_1", "six_raw"])
def test_a_zero_normal_weight_is_exactly_zero(r, cfg):
    """Two half-images with normals (1, 0, 0) and (0, 0, 1), wider than a block: other colours in the right half leave the left half's
    result as it is, in bits."""
    a = run(r, *dr.half_planes(80, 20, right_scale=1.0), cfg=cfg)
    b = run(r, *dr.half_planes(80, 20, right_scale=7.0), cfg=cfg)
    assert same(a[:, :40], b[:, :40])
    assert not same(a[:, 40:], b[:, 40:])
    assert not same(a[:, :40], dr.half_planes(80, 20)[0][:, :40])      # and it was filtered


def test_two_calls_and_the_in_place_call_give_the_same_bits(r):
    sc = synthetic(W, H)
    for cfg in (dr.Config(), dr.Config(iterations=1), dr.Config(iterations=2)):
        first = run(r, sc["color"], sc["albedo"], sc["normal_depth"], cfg)
        other = run(r, *dr.half_planes(80, 20), cfg=cfg)                 # another size in between: the scratch is reallocated
        assert same(run(r, sc["color"], sc["albedo"], sc["normal_depth"], cfg), first)
        assert same(run(r, sc["color"], sc["albedo"], sc["normal_depth"], cfg, in_place=True), first)
        assert other.shape == (20, 80, 4)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def small_scene():
    """The scene of tests/test_gpu_aov.py: test_scene without an environment map from a distance at which about a quarter of the picture is
    geometry -- sky tiles, a tile nearly full of hits, silhouettes in between."""
    s = scenes.test_scene(W, 16, with_env=False)
    s.width, s.height = W, H
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.6), 5.0, 0.35, -0.45)
    s.settings.environment_color[:] = ENV
    s.settings.max_accumulated_frames = 64
    return s


def render(s, frames, denoise_at=()):
    """`frames` accumulated samples with both AOVs on; after each frame count in denoise_at a pt_denoise into a separate image.  Returns the
    read-backs (output, albedo, normal_depth), the stats, and the last denoised image (or None)."""
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    s.upload(r)
    out, alb, nd = (r.create_output(W, H) for _ in range(3))
    r.set_aov(alb, nd)
    st = copy_settings(s.settings); st.reset = 1
    r.reset_stats()
    den = None
    for f in range(frames):
        r.trace(st, s.execute_params(f), out); st.reset = 0
        if f + 1 in denoise_at:
            den = r.readback(r.denoise(out, alb, nd))
    imgs = tuple(r.readback(t) for t in (out, alb, nd))
    stats = r.stats()
    r.close()
    return imgs, stats, den


def test_end_to_end_on_the_test_scene_and_pt_trace_does_not_notice():
    s = small_scene()
    (out, alb, nd), st_d, den = render(s, 8, denoise_at=(3, 8))
    cov = alb[..., 3]
    assert (cov == 0).mean() > 0.1 and (cov == 1).mean() > 0.1 and ((cov > 0) & (cov < 1)).sum() > 10
    check_against_ref64(den, out, alb, nd, dr.Config(), "test_scene 8 spp")
    assert same(den[cov == 0], out[cov == 0])                          # the background comes out unchanged
    assert not same(den[cov == 1], out[cov == 1])
    (out0, alb0, nd0), st_0, _ = render(s, 8)
    assert same(out, out0) and same(alb, alb0) and same(nd, nd0)
    for name in ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames"):
        assert getattr(st_d, name) == getattr(st_0, name), (name, getattr(st_d, name), getattr(st_0, name))
    assert st_d.accumulated_frames == 8


def test_an_adaptive_trace_between_two_calls_leaves_the_scratch_alone():
    """pt_denoise, then pt_set_adaptive and the first adaptive pt_trace (which allocates the adaptive state), then pt_denoise at the same
    size: the context's denoiser scratch is its own, and the second call gives the bits of the first."""
    from gltf_renderer_amd.renderer import Renderer
    s = small_scene()
    sc = synthetic(W, H)
    r = Renderer(0)
    s.upload(r)
    c, a, n = dev(r, sc["color"]), dev(r, sc["albedo"]), dev(r, sc["normal_depth"])
    first = r.readback(r.denoise(c, a, n))
    out = r.create_output(W, H)
    r.set_samples_per_trace(2)
    r.set_adaptive(2, 4, 0.05)
    st = copy_settings(s.settings); st.reset = 1
    r.trace(st, s.execute_params(0), out)
    active, samples, _, _ = r.adaptive_read(W, H)
    assert samples.max() == 2
    second = r.readback(r.denoise(c, a, n))
    assert same(second, first)
    st.reset = 0
    r.trace(st, s.execute_params(2), out)                               # the adaptive state is intact too
    assert r.adaptive_read(W, H)[1].max() == 4
    check_against_ref64(second, sc["color"], sc["albedo"], sc["normal_depth"], dr.Config(), "after an adaptive trace")
    r.close()


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_invalid_argument_and_writes_nothing(r):
    sc = synthetic(W, H)
    c, a, n = dev(r, sc["color"]), dev(r, sc["albedo"]), dev(r, sc["normal_depth"])
    out = r.torch.full((H, W, 4), POISON, dtype=r.torch.float32, device=c.device)
    L = r.L

    def call(ctx=r.h, cfg=None, color=c, albedo=a, nd=n, w=W, h=H, o=out):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return L.pt_denoise(ctx, C.byref(cfg) if cfg is not None else None, p(color), p(albedo), p(nd), w, h, p(o))

    def cfg(**kw):
        d = abi.PtDenoiseConfig.default()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    nan, inf = float("nan"), float("inf")
    refusals = dict(
        null_ctx=dict(ctx=None), null_color=dict(color=None), null_albedo=dict(albedo=None), null_normal_depth=dict(nd=None), null_out=dict(o=None),
        zero_width=dict(w=0), zero_height=dict(h=0), width_above_2_30=dict(w=(1 << 30) + 1), height_above_2_30=dict(h=(1 << 30) + 1),
        iterations_below=dict(cfg=cfg(iterations=-1)), iterations_above=dict(cfg=cfg(iterations=7)),
        power_below=dict(cfg=cfg(normal_power_log2=-1)), power_above=dict(cfg=cfg(normal_power_log2=11)),
        sigma_depth_zero=dict(cfg=cfg(sigma_depth=0.0)), sigma_depth_negative=dict(cfg=cfg(sigma_depth=-0.02)),
        sigma_depth_nan=dict(cfg=cfg(sigma_depth=nan)), sigma_depth_inf=dict(cfg=cfg(sigma_depth=inf)),
        sigma_color_negative=dict(cfg=cfg(sigma_color=-1.0)), sigma_color_nan=dict(cfg=cfg(sigma_color=nan)), sigma_color_inf=dict(cfg=cfg(sigma_color=inf)))
    for name, kw in refusals.items():
        assert call(**kw) == -1, name
    r.torch.cuda.synchronize()
    assert np.all(r.readback(out) == POISON)
    # out aliasing a guide image: that image is what would be written, and it stays as it is
    assert call(o=a) == -1 and call(o=n) == -1
    assert call(o=a, cfg=cfg(iterations=0)) == -1
    assert same(r.readback(a), sc["albedo"]) and same(r.readback(n), sc["normal_depth"]) and same(r.readback(c), sc["color"])
    # out overlapping color without being color (one row further on in the same allocation)
    both = r.torch.full((H + 1, W, 4), POISON, dtype=r.torch.float32, device=c.device)
    assert call(color=both[:H], o=both[1:]) == -1 and call(color=both[1:], o=both[:H]) == -1
    r.torch.cuda.synchronize()
    assert bool((both == POISON).all())
    # the edges of the ranges are accepted
    for ok in (cfg(iterations=0), cfg(iterations=6), cfg(normal_power_log2=0), cfg(normal_power_log2=10), cfg(sigma_color=0.0), cfg(demodulate=-5)):
        assert call(cfg=ok) == 0
    assert not np.any(r.readback(out) == POISON)
