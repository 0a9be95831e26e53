"""pt_denoise_variance (include/mipt.h) on the MI355X against the numpy restatement tests/denoise_variance_ref.py, held to it the way
tests/test_gpu_denoise.py holds pt_denoise to its own.

What is exact by construction is compared in bits: the invalid pixels and every alpha, iterations = 0, determinism, the in-place call, the
two filters' scratch side by side, the argument refusals, and that pt_trace does not notice the call.  The filtered values are held to
    max over valid pixels and channels of |gpu - ref64| / (|ref64| + 1e-3)  <=  8 * E32,
E32 being the same figure of the float32 restatement, computed in the same test from the same inputs: the margin of 8 over the reference's
own float32 rounding is test_gpu_denoise.py's, for the kernel's own expf; a wrong tap, weight, count or step shows at 1e-3 or more.
Every case prints E32, the kernel's figure, their ratio and the share of values bit-equal to the float32 restatement; DESIGN.md section 4
records them."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import denoise_ref as dr
from tests import denoise_variance_ref as dv
from tests.test_gpu_denoise import small_scene, copy_settings

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, H = 72, 40                      # 5 x 3 tiles of 16 (3 x 5 blocks of 32 x 8), ragged in both directions
POISON = 7.0
MARGIN = 8.0
TILES_0_1_2_64 = np.array([[64, 0, 2, 64, 2], [2, 64, 64, 1, 64], [64, 2, 64, 2, 2]], np.uint32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def native(cfg):
    return abi.PtDenoiseVarianceConfig(cfg.iterations, cfg.demodulate, cfg.normal_power_log2, cfg.sigma_depth, cfg.sigma_variance)


@pytest.fixture(scope="module")
def r():
    from gltf_renderer_amd.renderer import Renderer
    ctx = Renderer(0)
    yield ctx
    ctx.close()


def dev(r, a):
    return r.torch.from_numpy(np.array(a, f32, order="C")).to("cuda:%d" % r.device)      # a copy: the scenes are read-only


def run(r, sc, cfg=None, in_place=False):
    """sc: a scene of synthetic(); its `tiles` (per-tile counts) or `samples` say how the counts are passed."""
    imgs = [sc[k] for k in ("color", "albedo", "normal_depth", "variance")]
    c, a, n, v = (dev(r, x) for x in imgs)
    out = r.denoise_variance(c, a, n, v, samples=sc["samples"], tile_samples=sc["tiles"], out=c if in_place else None,
                             config=native(cfg) if cfg is not None else None)
    got = r.readback(out)
    for t, x in zip((c, a, n, v), imgs):                               # the inputs are only read
        assert (in_place and t is c) or same(r.readback(t), x)
    return got


_SCENES = {}


def synthetic(w, h, tiles=None, samples=8):
    """The scene at per-tile counts `tiles`, or `samples` everywhere; made once per key and never written."""
    key = (w, h, None if tiles is None else tiles.tobytes(), samples)
    if key not in _SCENES:
        counts = dv.pixel_counts(tiles if tiles is not None else samples, w, h)
        sc = dv.scene(w, h, counts=counts, seed=3)
        sc["color"][..., 3] = np.random.default_rng(w * 1000 + h).random((h, w)).astype(f32)      # an alpha worth comparing
        sc.update(tiles=tiles, samples=0 if tiles is not None else samples)
        for x in sc.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _SCENES[key] = sc
    return _SCENES[key]


def check_against_ref64(got, color, albedo, nd, variance, counts, cfg, label):
    ref64, valid = dv.denoise_variance(color, albedo, nd, variance, counts, cfg, f64)
    ref32, _ = dv.denoise_variance(color, albedo, nd, variance, counts, cfg, f32)
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
    return valid


def check(got, sc, cfg, label):
    return check_against_ref64(got, sc["color"], sc["albedo"], sc["normal_depth"], sc["variance"], sc["counts"], cfg or dv.Config(), label)


VARIANTS = dict(defaults=dv.Config(), no_demodulation=dv.Config(demodulate=0), colour_term_off=dv.Config(sigma_variance=0),
                normal_power_1=dv.Config(normal_power_log2=0), one_pass=dv.Config(iterations=1), two_passes=dv.Config(iterations=2),
                six_passes_wide_sigmas=dv.Config(iterations=6, normal_power_log2=10, sigma_depth=0.5, sigma_variance=16.0))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_synthetic_scene_against_the_float64_restatement(r, name):
    sc = synthetic(W, H)
    assert (~sc["rendered"]).sum() > 100 and np.isnan(sc["color"]).any() and np.isinf(sc["color"]).any()
    valid = check(run(r, sc, VARIANTS[name]), sc, VARIANTS[name], name)
    assert np.array_equal(valid, sc["rendered"])


@pytest.mark.parametrize("cfg", [dv.Config(), dv.Config(iterations=1)], ids=["defaults", "one_pass"])
def test_per_tile_counts_of_0_1_2_and_64(r, cfg):
    """Tiles without samples, with one, with two and with 64 side by side: the first two kinds come out as they went in."""
    sc = synthetic(W, H, tiles=TILES_0_1_2_64)
    got = run(r, sc, cfg)
    valid = check(got, sc, cfg, "tiles of 0, 1, 2 and 64 samples, %d pass(es)" % cfg.iterations)
    low = dv.pixel_counts(TILES_0_1_2_64, W, H) < 2
    assert low.sum() == 2 * 256 and not valid[low].any() and same(got[low], sc["color"][low])
    assert valid[dv.pixel_counts(TILES_0_1_2_64, W, H) == 2].sum() > 500              # of 960 such pixels, some behind the wedge
    # the same counts given as one number are the same call
    uni = synthetic(W, H)
    eights = np.full((3, 5), 8, np.uint32)
    as_tiles = dict(uni, tiles=eights, samples=0)
    assert same(run(r, as_tiles, cfg), run(r, uni, cfg))


def test_null_config_means_the_defaults(r):
    sc = synthetic(W, H)
    assert same(run(r, sc, None), run(r, sc, dv.Config()))


@pytest.mark.parametrize("w,h", [(17, 33), (5, 3), (1, 1)])
def test_small_images_where_most_taps_fall_outside(r, w, h):
    sc = synthetic(w, h)
    cfg = dv.Config(iterations=6)
    valid = check(run(r, sc, cfg), sc, cfg, "%dx%d" % (w, h))
    assert valid.any()


def test_zero_iterations_is_the_identity_in_bits(r):
    sc = synthetic(W, H, tiles=TILES_0_1_2_64)
    cfg = dv.Config(iterations=0)
    assert same(run(r, sc, cfg), sc["color"])
    assert same(run(r, sc, cfg, in_place=True), sc["color"])


def test_two_calls_the_in_place_call_and_pt_denoise_in_between_give_the_same_bits(r):
    """The two filters keep their scratch apart: a pt_denoise call at the same size between two calls changes neither's result."""
    sc = synthetic(W, H, tiles=TILES_0_1_2_64)
    old_args = [dev(r, sc[k]) for k in ("color", "albedo", "normal_depth")]
    old_first = r.readback(r.denoise(*old_args))
    for cfg in (dv.Config(), dv.Config(iterations=1), dv.Config(iterations=2)):
        first = run(r, sc, cfg)
        assert same(r.readback(r.denoise(*old_args)), old_first)
        assert same(run(r, sc, cfg), first)
        other = run(r, synthetic(17, 33), cfg)                          # another size in between: the scratch is reallocated
        assert same(run(r, sc, cfg), first)
        assert same(run(r, sc, cfg, in_place=True), first)
        assert same(r.readback(r.denoise(*old_args)), old_first)
        assert other.shape == (33, 17, 4)
    assert not same(first, old_first)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def render(s, frames, adaptive=None, filter_it=True):
    """`frames` accumulated samples with both AOVs and the variance pass on, one call a frame; adaptive: (min, max, threshold) or None.
    Then the filter into a separate image.  Returns the read-backs (output, albedo, normal_depth, variance), the stats, the per-tile counts
    (or None) and the filtered image (or None)."""
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    s.upload(r)
    out, alb, nd, var = (r.create_output(W, H) for _ in range(4))
    r.set_aov(alb, nd)
    r.set_variance(var)
    if adaptive:
        r.set_adaptive(*adaptive)
    st = copy_settings(s.settings); st.reset = 1
    r.reset_stats()
    for f in range(frames):
        r.trace(st, s.execute_params(f), out); st.reset = 0
    tiles = None
    if adaptive:
        _, tiles, error, _ = r.adaptive_read(W, H)
        print("tile samples", tiles.tolist(), "tile errors", np.round(error, 3).tolist())
    den = None
    if filter_it:
        den = r.readback(r.denoise_variance(out, alb, nd, var, samples=frames, tile_samples=tiles))
    imgs = tuple(r.readback(t) for t in (out, alb, nd, var))
    stats = r.stats()
    r.close()
    return imgs, stats, tiles, den


def test_end_to_end_on_the_test_scene_and_pt_trace_does_not_notice():
    s = small_scene()
    (out, alb, nd, var), st_d, _, den = render(s, 8)
    cov = alb[..., 3]
    assert (cov == 0).mean() > 0.1 and (cov == 1).mean() > 0.1 and ((cov > 0) & (cov < 1)).sum() > 10
    valid = check_against_ref64(den, out, alb, nd, var, dv.pixel_counts(8, W, H), dv.Config(), "test_scene 8 spp")
    assert valid[cov == 1].mean() > 0.9
    assert same(den[cov == 0], out[cov == 0])                          # the background comes out unchanged
    assert not same(den[cov == 1], out[cov == 1])
    (out0, alb0, nd0, var0), st_0, _, _ = render(s, 8, filter_it=False)
    assert same(out, out0) and same(alb, alb0) and same(nd, nd0) and same(var, var0)
    for name in ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames"):
        assert getattr(st_d, name) == getattr(st_0, name), (name, getattr(st_d, name), getattr(st_0, name))
    assert st_d.accumulated_frames == 8


# the tiles' errors at 8 samples are 0 (sky), 0.12 (one tile with geometry) and 0.29 .. 1.26: at this threshold the sky retires at 2, that
# tile on the way and the rest never, so valid pixels of different counts meet
ADAPTIVE_THRESHOLD = 0.2


def test_end_to_end_under_adaptive_sampling_tiles_of_different_counts_meet_in_one_call():
    s = small_scene()
    (out, alb, nd, var), _, tiles, den = render(s, 8, adaptive=(2, 8, ADAPTIVE_THRESHOLD))
    assert len(set(int(t) for t in tiles.ravel() if t >= 2)) >= 2, tiles
    check_against_ref64(den, out, alb, nd, var, dv.pixel_counts(tiles, W, H), dv.Config(), "test_scene, adaptive 2..8")


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_invalid_argument_and_writes_nothing(r):
    sc = synthetic(W, H)
    c, a, n, v = (dev(r, sc[k]) for k in ("color", "albedo", "normal_depth", "variance"))
    out = r.torch.full((H, W, 4), POISON, dtype=r.torch.float32, device=c.device)
    ts = np.full(15, 8, np.uint32)
    L = r.L

    def call(ctx=r.h, cfg=None, color=c, albedo=a, nd=n, var=v, w=W, h=H, tiles=ts, samples=8, o=out):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return L.pt_denoise_variance(ctx, C.byref(cfg) if cfg is not None else None, p(color), p(albedo), p(nd), p(var), w, h,
                                     tiles.ctypes.data_as(C.c_void_p) if tiles is not None else None, samples, p(o))

    def cfg(**kw):
        d = abi.PtDenoiseVarianceConfig.default()
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    nan, inf = float("nan"), float("inf")
    refusals = dict(
        null_ctx=dict(ctx=None), null_color=dict(color=None), null_albedo=dict(albedo=None), null_normal_depth=dict(nd=None),
        null_variance=dict(var=None), null_out=dict(o=None),
        zero_width=dict(w=0), zero_height=dict(h=0), width_above_2_30=dict(w=(1 << 30) + 1), height_above_2_30=dict(h=(1 << 30) + 1),
        too_many_tiles=dict(w=1 << 30, h=1 << 30),
        iterations_below=dict(cfg=cfg(iterations=-1)), iterations_above=dict(cfg=cfg(iterations=7)),
        power_below=dict(cfg=cfg(normal_power_log2=-1)), power_above=dict(cfg=cfg(normal_power_log2=11)),
        sigma_depth_zero=dict(cfg=cfg(sigma_depth=0.0)), sigma_depth_negative=dict(cfg=cfg(sigma_depth=-0.02)),
        sigma_depth_nan=dict(cfg=cfg(sigma_depth=nan)), sigma_depth_inf=dict(cfg=cfg(sigma_depth=inf)),
        sigma_variance_negative=dict(cfg=cfg(sigma_variance=-1.0)), sigma_variance_nan=dict(cfg=cfg(sigma_variance=nan)),
        sigma_variance_inf=dict(cfg=cfg(sigma_variance=inf)),
        no_counts_and_one_sample=dict(tiles=None, samples=1), no_counts_and_no_sample=dict(tiles=None, samples=0))
    for name, kw in refusals.items():
        assert call(**kw) == -1, name
    r.torch.cuda.synchronize()
    assert np.all(r.readback(out) == POISON)
    # out aliasing a guide image or the variance: that image is what would be written, and it stays as it is
    assert call(o=a) == -1 and call(o=n) == -1 and call(o=v) == -1
    assert call(o=a, cfg=cfg(iterations=0)) == -1 and call(o=v, cfg=cfg(iterations=0)) == -1
    for t, k in ((a, "albedo"), (n, "normal_depth"), (v, "variance"), (c, "color")):
        assert same(r.readback(t), sc[k]), k
    # out overlapping color without being color (one row further on in the same allocation)
    both = r.torch.full((H + 1, W, 4), POISON, dtype=r.torch.float32, device=c.device)
    assert call(color=both[:H], o=both[1:]) == -1 and call(color=both[1:], o=both[:H]) == -1
    r.torch.cuda.synchronize()
    assert bool((both == POISON).all())
    # the edges of the ranges are accepted; with a count array `samples` is not looked at
    for ok in (cfg(iterations=0), cfg(iterations=6), cfg(normal_power_log2=0), cfg(normal_power_log2=10), cfg(sigma_variance=0.0), cfg(demodulate=-5)):
        assert call(cfg=ok) == 0
    assert call(tiles=None, samples=2) == 0 and call(samples=0) == 0
    assert not np.any(r.readback(out) == POISON)
