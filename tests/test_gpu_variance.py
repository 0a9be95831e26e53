"""The variance AOV and the noise report (include/mipt.h pt_set_variance / pt_noise_estimate) on the MI355X, bit for bit against
tests/variance_ref.py.

The per-sample radiance x the definition speaks of is what a call without FLAG_ACCUMULATE writes: the sample after the pending records and
sanitize_sample.  So the frames rendered one by one without accumulation are the inputs, and the target of the accumulated run must be the
restatement's fold of them in all four channels.  Nothing here is compared with a tolerance except a tile's mean error, whose bound
256 * 2^-24 is that of a float32 sum of at most 256 non-negative terms in any order and one division."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes
from tests import adaptive_ref as ar
from tests import variance_ref as vr

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 40, 24                      # 3 x 2 tiles, ragged in both axes
N = 6
POISON = 7.0
CLAMP = 0.5
STATS = ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames")


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def single(st):
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE
    return s1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def main_scene():
    s = scenes.test_scene(W, 16)
    s.width, s.height = W, H
    s.settings.max_accumulated_frames = 64
    assert s.settings.use_frame_as_seed
    return s


def sky_scene():
    """test_scene without an environment map, from a distance at which the right-hand tiles see only the constant environment colour."""
    s = scenes.test_scene(W, 16, with_env=False)
    s.width, s.height = W, H
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.6), 5.0, 0.35, -0.45)
    s.settings.environment_color[:] = (0.25, 0.5, 0.75)
    s.settings.max_accumulated_frames = 64
    return s


class Ctx:
    def __init__(self, s, variance=True, poison=None, size=None):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        self.handles = s.upload(self.r)
        self.env = self.handles["env"]
        w, h = size or (s.width, s.height)
        self.out = self.r.create_output(w, h)
        self.var = self.r.create_output(w, h)
        if poison is not None:
            self.var.fill_(poison)
        if variance:
            self.r.set_variance(self.var)

    def params(self, frame, **kw):
        return self.s.execute_params(frame, env_handle=self.env, **kw)

    def trace(self, st, frame, **kw):
        self.r.trace(st, self.params(frame, **kw), self.out)

    def output(self):
        return self.r.readback(self.out)

    def target(self):
        return self.r.readback(self.var)

    def close(self):
        self.r.close()


def singles_of(c, st, frames=N):
    out = []
    for f in range(frames):
        c.trace(single(st), f)
        out.append(c.output())
    return out


def accumulate(c, st, frames=N, first=0, reset=True, **kw):
    sa = copy_settings(st); sa.reset = 1 if reset else 0
    for f in range(first, first + frames):
        c.trace(sa, f, **kw); sa.reset = 0


def render(s, st):
    """The per-sample frames, and the outputs and targets of an accumulation traced frame by frame, with its stats."""
    c = Ctx(s, poison=POISON)
    x = singles_of(c, st)
    assert np.all(bits(c.target()) == 0)                               # a call without FLAG_ACCUMULATE leaves zeros
    outs, tgts = [], []
    sa = copy_settings(st); sa.reset = 1
    c.r.reset_stats()
    for f in range(N):
        c.trace(sa, f); sa.reset = 0
        outs.append(c.output()); tgts.append(c.target())
    stats = c.r.stats()
    c.close()
    means, want = vr.fold(x)
    return dict(scene=s, st=st, x=x, outs=outs, tgts=tgts, stats=stats, means=means, want=want)


@pytest.fixture(scope="module")
def data():
    s = main_scene()
    return render(s, copy_settings(s.settings))


def check_fold(d):
    for k in range(N):
        assert same(d["outs"][k][..., :3], d["means"][k]), k           # the restatement's m' is the output's own blend
        assert same(d["tgts"][k], d["want"][k]), (k, int((bits(d["tgts"][k]) != bits(d["want"][k])).sum()))
    assert np.all(bits(d["tgts"][0]) == 0)
    V = d["tgts"][N - 1]
    assert np.all(V >= 0) and np.all(np.isfinite(V)) and (V[..., 3] > 0).mean() > 0.25


def test_the_target_is_the_fold_of_the_single_samples_bit_for_bit(data):
    check_fold(data)


def test_the_fold_under_a_luminance_clamp_that_bites(data):
    s = data["scene"]
    st = copy_settings(data["st"]); st.flags |= abi.FLAG_LUMINANCE_CLAMP; st.luminance_clamp = CLAMP
    d = render(s, st)
    bites = sum(int((np.abs(a[..., :3] - b[..., :3]).max(axis=-1) > 0).sum()) for a, b in zip(d["x"], data["x"]))
    print("samples the clamp changed: %d of %d" % (bites, N * W * H))
    assert bites >= 20, bites
    assert not same(d["tgts"][N - 1], data["tgts"][N - 1])
    check_fold(d)


def all_passes(s, st, variance):
    from tests import matte_ref as mr
    c = Ctx(s, variance=variance, poison=POISON)
    imgs = [c.r.create_output(W, H) for _ in range(4)]                 # albedo, normal_depth, a matte layer, motion
    c.r.set_aov(imgs[0], imgs[1])
    c.r.set_matte(mr.INSTANCE, [imgs[2]])
    p = c.params(0)
    c.r.set_motion(imgs[3], list(p.world_to_view), list(p.view_to_clip))
    c.r.reset_stats()
    accumulate(c, st)
    got = [c.output()] + [c.r.readback(t) for t in imgs], c.r.stats(), c.target()
    c.close()
    return got


def test_the_pass_leaves_everything_else_untouched(data):
    s, st = data["scene"], data["st"]
    # the output, ray counts and frame count of a context that never heard of the pass
    c = Ctx(s, variance=False, poison=POISON)
    c.r.reset_stats()
    sa = copy_settings(st); sa.reset = 1
    for f in range(N):
        c.trace(sa, f); sa.reset = 0
        assert same(c.output(), data["outs"][f]), f
    q = c.r.stats()
    for name in STATS:
        assert getattr(q, name) == getattr(data["stats"], name), name
    assert q.accumulated_frames == N and q.rays_primary > 0
    assert np.all(c.target() == POISON)
    c.close()
    # all four optional passes together, with and without the variance
    on, off = all_passes(s, st, True), all_passes(s, st, False)
    for k, (a, b) in enumerate(zip(on[0], off[0])):
        assert same(a, b), k
    for name in STATS:
        assert getattr(on[1], name) == getattr(off[1], name), name
    assert same(on[0][0], data["outs"][N - 1]) and same(on[2], data["want"][N - 1]) and np.all(off[2] == POISON)


@pytest.mark.parametrize("batches", [(6,), (2, 4), (1, 5)], ids=["6", "2+4", "1+5"])
def test_batches_equal_the_calls_one_by_one(data, batches):
    c = Ctx(data["scene"], poison=POISON)
    sa = copy_settings(data["st"]); sa.reset = 1
    frame = 0
    for b in batches:
        c.r.set_samples_per_trace(b)
        c.trace(sa, frame); sa.reset = 0
        frame += b
        assert same(c.target(), data["want"][frame - 1]) and same(c.output(), data["outs"][frame - 1]), (batches, frame)
    assert c.r.stats().accumulated_frames == N
    c.close()


def test_a_tile_shard_writes_only_its_own_tiles(data):
    c = Ctx(data["scene"], poison=POISON)
    accumulate(c, data["st"], tile_rank=1, tile_rank_count=2)
    img = c.target()
    ty, tx = vr.tile_grid(W, H)
    for g in range(ty * tx):
        y, x = divmod(g, tx)
        if g % 2 == 1:
            assert same(ar.tile_view(img, y, x), ar.tile_view(data["want"][N - 1], y, x)), g
        else:
            assert np.all(ar.tile_view(img, y, x) == POISON), g
    c.close()


def test_adaptive_tiles_hold_the_uniform_fold_at_their_own_count():
    s = sky_scene()
    st = copy_settings(s.settings)
    c = Ctx(s, poison=POISON)
    x = singles_of(c, st)
    _, want = vr.fold(x)
    c.var.fill_(POISON)
    c.r.set_adaptive(2, N, 0.0)
    frame, active = 0, 1
    while active and frame < N:
        c.trace(st, frame)
        frame += 1
        active, samples, error, _ = c.r.adaptive_read(W, H)
    got = c.target()
    sky = [t for t in np.ndindex(samples.shape) if samples[t] == 2]
    geometry = [t for t in np.ndindex(samples.shape) if samples[t] == N]
    print("tile samples", samples.tolist())
    assert sky and geometry and len(sky) + len(geometry) == samples.size, samples
    for (y, x_) in np.ndindex(samples.shape):
        n = int(samples[y, x_])
        assert same(ar.tile_view(got, y, x_), ar.tile_view(want[n - 1], y, x_)), (y, x_, n)
    for (y, x_) in sky:
        assert error[y, x_] == 0 and np.all(bits(ar.tile_view(got, y, x_)) == 0), (y, x_)
    for (y, x_) in geometry:
        assert ar.tile_view(got, y, x_)[..., 3].max() > 0, (y, x_)
    c.close()


def test_calls_that_write_nothing_and_the_refusals(data):
    from gltf_renderer_amd.renderer import MiptError
    s, st = data["scene"], data["st"]
    c = Ctx(s, poison=POISON)
    r, L = c.r, c.r.L
    # a debug-output call leaves the sentinel
    sd = copy_settings(st); sd.debug_output = abi.DEBUG_OUTPUT_COLOR; sd.reset = 1
    c.trace(sd, 0)
    assert np.all(c.target() == POISON)
    # a call without FLAG_ACCUMULATE writes zeros
    c.trace(single(st), 0)
    assert np.all(bits(c.target()) == 0)
    sm = copy_settings(st); sm.max_accumulated_frames = 2; sm.reset = 1
    c.trace(sm, 0); sm.reset = 0
    c.trace(sm, 1)
    assert same(c.target(), data["want"][1])
    # enable with a NULL target, and a NULL config, are refused: the old config stays and no restart is pending
    bad = abi.PtVarianceConfig(1, 0, None)
    assert L.pt_set_variance(r.h, C.byref(bad)) == -1 and "target" in L.pt_last_error(r.h).decode()
    assert L.pt_set_variance(r.h, None) == -1 and "config" in L.pt_last_error(r.h).decode()
    r.accum_save(W, H, c.out)
    sa = copy_settings(st)
    c.trace(sa, 2)
    assert r.stats().accumulated_frames == 3 and same(c.target(), data["want"][2])
    # a call past max_accumulated_frames leaves the sentinel
    c.var.fill_(POISON)
    before = c.output()
    c.trace(sm, 3)
    assert np.all(c.target() == POISON) and same(c.output(), before) and r.stats().accumulated_frames == 3
    # a good config: a restart is pending until the next trace, and pt_accum_save answers PT_ERR_NOT_READY
    r.set_variance(c.var)
    with pytest.raises(MiptError, match="^-6"):
        r.accum_save(W, H, c.out)
    c.trace(sa, 0)
    assert r.stats().accumulated_frames == 1 and np.all(bits(c.target()) == 0)
    # the megakernel: refused, output and target untouched
    r.set_kernel_mode(abi.MODE_MEGAKERNEL)
    c.out.fill_(POISON); c.var.fill_(POISON)
    p = c.params(0)
    p.output = c.out.data_ptr()
    for sx in (sa, single(st)):
        assert L.pt_trace(r.h, C.byref(sx), C.byref(p)) == -1 and "wavefront" in L.pt_last_error(r.h).decode()
    assert np.all(c.output() == POISON) and np.all(c.target() == POISON)
    # ... with the pass off the megakernel runs as always and the target stays
    r.set_variance(None)
    c.trace(sa, 0)
    assert not np.any(c.output() == POISON) and np.all(c.target() == POISON)
    r.set_kernel_mode(abi.MODE_WAVEFRONT)
    r.set_variance(c.var)
    sa.reset = 1
    c.trace(sa, 0); sa.reset = 0
    c.trace(sa, 1)
    assert same(c.target(), data["want"][1])
    c.close()


def test_one_probe_atlas(data):
    s, st = data["scene"], data["st"]
    c = Ctx(s, variance=False, size=(16, 16))
    aw, ah = c.r.set_probes([(0.0, -0.5, 1.2)], 16, columns=1)
    assert (aw, ah) == (16, 16)
    c.r.set_variance(c.var)

    def trace(sx, frame):
        p = c.params(frame)
        p.width, p.height = aw, ah
        c.r.trace(sx, p, c.out)

    x = []
    for f in range(N):
        trace(single(st), f)
        x.append(c.output())
    means, want = vr.fold(x)
    sa = copy_settings(st); sa.reset = 1
    for f in range(N):
        trace(sa, f); sa.reset = 0
        assert same(c.target(), want[f]) and same(c.output()[..., :3], means[f]), f
    assert (want[N - 1][..., 3] > 0).mean() > 0.25
    c.close()


def test_a_checkpoint_resumes_the_output_and_the_kept_target(data):
    from gltf_renderer_amd.renderer import MiptError
    s, st = data["scene"], data["st"]
    a = Ctx(s, poison=POISON)
    with pytest.raises(MiptError, match="^-6"):                        # between pt_set_variance and the next trace
        a.r.accum_save(W, H, a.out)
    accumulate(a, st, frames=3)
    blob = a.r.accum_save(W, H, a.out, next_frame=3)
    kept = a.var.clone()
    a.close()
    b = Ctx(s, variance=False)
    b.var = kept
    b.r.set_variance(kept)
    assert b.r.accum_load(blob, b.out).accumulated_frames == 3
    accumulate(b, st, frames=3, first=3, reset=False)
    assert b.r.stats().accumulated_frames == N
    assert same(b.output(), data["outs"][N - 1]) and same(b.target(), data["want"][N - 1])
    b.close()


# ---- pt_noise_estimate -------------------------------------------------------------------------------------------------------------
def device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def check_estimate(r, img, var, ts, samples, threshold):
    """One call against the restatement; ts: (tiles_y, tiles_x) counts or None for `samples` everywhere."""
    ty, tx = vr.tile_grid(img.shape[1], img.shape[0])
    counts = np.full((ty, tx), samples, np.uint32) if ts is None else np.asarray(ts, np.uint32)
    mean, mx, summ = r.noise_estimate(device(img), device(var), samples=samples, tile_samples=ts, threshold=threshold)
    wmean, wmax, px = vr.noise_tiles(img, var, counts)
    assert same(mx, wmax), (mx, wmax)                                  # order-free, hence exact
    est = counts >= 2
    assert np.all(mean[~est] == -1) and np.all(mx[~est] == -1)
    inf = np.isinf(wmean)
    assert np.array_equal(np.isinf(mean), inf)
    ok = est & ~inf
    with np.errstate(invalid="ignore"):                                # inf - inf where both say +infinity: compared above, masked here
        err = np.abs(mean.astype(np.float64) - wmean)[ok]
    assert np.all(err <= 256 * 2.0 ** -24 * wmean[ok]), float((err / np.maximum(wmean[ok], 1e-300)).max())
    tiles, n_est, above, smean, smax = vr.summary(mean, mx, px, counts, threshold)
    assert (summ.tiles, summ.tiles_estimated, summ.tiles_above) == (tiles, n_est, above)
    assert same(f32(summ.mean), smean) and same(f32(summ.max), smax), (summ.mean, smean, summ.max, smax)
    return mean, mx, summ


def test_noise_estimate_against_the_restatement(data):
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    img, var = data["outs"][N - 1], data["tgts"][N - 1]
    mean, mx, summ = check_estimate(r, img, var, None, N, 0.1)
    assert summ.tiles == 6 and summ.tiles_estimated == 6 and summ.max > 0 and 0 < summ.mean <= summ.max
    # a threshold between the tiles' maxima splits them
    mid = float(np.sort(mx.ravel())[2])
    assert check_estimate(r, img, var, None, N, mid)[2].tiles_above == int((mx > f32(mid)).sum())
    # counts with zeros (another rank's tiles) and a one: -1 entries, fewer tiles estimated
    ts = np.array([[N, 0, N], [1, N, 3]], np.uint32)
    m2, x2, s2 = check_estimate(r, img, var, ts, 0, 0.1)
    assert s2.tiles_estimated == 4 and m2[0, 1] == -1 and x2[1, 0] == -1 and same(x2[0, 0], mx[0, 0]) and x2[1, 2] > mx[1, 2]
    s0 = check_estimate(r, img, var, np.zeros((2, 3), np.uint32), 0, 0.1)[2]
    assert (s0.tiles_estimated, s0.tiles_above, s0.mean, s0.max) == (0, 0, -1.0, -1.0)
    # a NaN planted in V.w gives +infinity in that tile, in the ragged corner tile too; a negative V.w is a NaN under the root
    v2 = var.copy(); v2[20, 35, 3] = np.nan; v2[3, 3, 3] = -1.0
    m3, x3, s3 = check_estimate(r, img, v2, None, N, 0.1)
    assert np.isinf(x3[1, 2]) and np.isinf(m3[1, 2]) and np.isinf(x3[0, 0]) and np.isinf(s3.max) and same(x3[0, 1], mx[0, 1])
    # ragged tiles count only in-image pixels: a constant error is its own mean in every tile
    ci = np.full((H, W, 4), 0.25, f32); cv = np.full((H, W, 4), 0.03, f32)
    m4, x4, _ = check_estimate(r, ci, cv, None, 4, 0.1)
    e = vr.pixel_error(ci[:1, :1], cv[:1, :1], 4)[0, 0]
    assert np.all(x4 == e) and np.all(np.abs(m4 - e) <= 256 * 2.0 ** -24 * e)
    # a size that is a single ragged tile, and one with many tiles: the scratch is regrown
    rng = np.random.default_rng(21)
    for (w, h) in ((5, 3), (100, 70)):
        check_estimate(r, rng.random((h, w, 4)).astype(f32), (rng.random((h, w, 4)) * 0.2).astype(f32), None, 9, 0.05)
    r.close()


def test_noise_estimate_refusals_write_nothing(data):
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    L = r.L
    img, var = device(data["outs"][N - 1]), device(data["tgts"][N - 1])
    mean, mx = np.full(6, 3.0, f32), np.full(6, 5.0, f32)
    summ = abi.PtNoiseSummary(9, 9, 9, 9.0, 9.0)
    ts = np.full(6, 4, np.uint32)

    def call(image=img.data_ptr(), variance=var.data_ptr(), w=W, h=H, counts=None, samples=4, threshold=0.1):
        return L.pt_noise_estimate(r.h, C.c_void_p(image), C.c_void_p(variance), w, h, counts.ctypes.data_as(C.c_void_p) if counts is not None else None,
                                   samples, threshold, mean.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p), C.byref(summ))

    cases = [dict(image=None), dict(variance=None), dict(w=0), dict(h=0), dict(w=(1 << 30) + 1), dict(h=(1 << 30) + 1), dict(threshold=float("nan")),
             dict(threshold=float("inf")), dict(threshold=-0.5), dict(samples=1), dict(samples=0)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert "noise_estimate" in L.pt_last_error(r.h).decode()
        assert np.all(mean == 3.0) and np.all(mx == 5.0) and (summ.tiles, summ.tiles_estimated, summ.tiles_above, summ.mean, summ.max) == (9, 9, 9, 9.0, 9.0), kw
    assert L.pt_noise_estimate(None, C.c_void_p(img.data_ptr()), C.c_void_p(var.data_ptr()), W, H, None, 4, 0.1, None, None, None) == -1
    # with counts given, `samples` is not looked at; every output may be NULL
    assert call(counts=ts, samples=0) == 0 and summ.tiles_estimated == 6 and np.all(mx > 0)
    assert L.pt_noise_estimate(r.h, C.c_void_p(img.data_ptr()), C.c_void_p(var.data_ptr()), W, H, None, 4, 0.0, None, None, None) == 0
    r.close()
