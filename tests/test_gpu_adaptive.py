"""Tile-level adaptive sampling (include/mipt.h pt_set_adaptive / pt_adaptive_read) on the MI355X.

The yardstick is the uniform accumulation: every tile of an adaptive image must equal, bit for bit, the same tile of the uniform
accumulation after that tile's own sample count, and which call retires a tile must follow from the raw samples through the numpy
restatement in tests/adaptive_ref.py (blend_sample, the half buffer, the float32 error metric)."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes
from tests import adaptive_ref as ar

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 72, 40                      # 5 x 3 tiles, ragged in both directions
N = 16                             # max_samples of the runs below


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def sky_scene():
    """test_scene without an environment map, seen from far away: the tiles round the picture see only environment_color."""
    s = scenes.test_scene(W, 16, with_env=False)
    s.width, s.height = W, H
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.6), 16.0, 0.35, -0.45)
    return s


class Ctx:
    def __init__(self, s, env=True):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        h = s.upload(self.r)
        self.env = h.get("env") if env else None

    def params(self, frame, **kw):
        return self.s.execute_params(frame, env_handle=self.env, **kw)

    def close(self):
        self.r.close()


def raw_and_uniform(s, frames):
    """Raw samples (one frame each, accumulation off) and the uniform accumulation snapshots U[n - 1] from a second context traced
    frame by frame."""
    a = Ctx(s)
    st = copy_settings(s.settings); st.flags &= ~abi.FLAG_ACCUMULATE
    out = a.r.create_output(W, H)
    raw = []
    for f in range(frames):
        a.r.trace(st, a.params(f), out)
        raw.append(a.r.readback(out))
    a.close()
    b = Ctx(s)
    st = copy_settings(s.settings); st.reset = 1
    out = b.r.create_output(W, H)
    uni = []
    for f in range(frames):
        b.r.trace(st, b.params(f), out); st.reset = 0
        uni.append(b.r.readback(out))
    b.close()
    return raw, uni


@pytest.fixture(scope="module")
def scene_data():
    s = scenes.test_scene(W, 16)
    s.width, s.height = W, H
    raw, uni = raw_and_uniform(s, N)
    I, A = ar.fold(raw)
    E = {n: ar.tile_errors(I[n - 1], A[n - 1]) for n in range(1, N + 1)}
    E64 = {n: ar.tile_errors(I[n - 1], A[n - 1], np.float64) for n in range(1, N + 1)}
    return dict(scene=s, raw=raw, uni=uni, I=I, A=A, E=E, E64=E64)


def thresholds(E):
    """Thresholds that retire tiles at several different counts: quantiles of the tiles' errors after 4 samples."""
    e = np.sort(E[4].ravel())
    return [float(e[len(e) // 4]), float(e[len(e) // 2]), float(e[(3 * len(e)) // 4])]


def run_adaptive(ctx, spp, min_s, max_s, thr, frame0=0, st=None, kw=None):
    """Host loop: trace calls of `spp` samples until no tile is active or the cap is reached.  Returns the output tensor."""
    r = ctx.r
    st = copy_settings(st or ctx.s.settings)
    kw = kw or {}
    r.set_samples_per_trace(spp)
    r.set_adaptive(min_s, max_s, thr)
    out = r.create_output(W, H)
    frame, cap = frame0, min(max_s, st.max_accumulated_frames)
    active = 1
    while active and frame - frame0 < cap:
        r.trace(st, ctx.params(frame, **kw), out)
        frame += spp
        active = r.adaptive_read(W, H)[0]
    return out


def assert_tiles_equal_uniform(img, samples, uni):
    ty, tx = samples.shape
    for y in range(ty):
        for x in range(tx):
            n = int(samples[y, x])
            assert n >= 1
            assert np.array_equal(ar.tile_view(img, y, x), ar.tile_view(uni[n - 1], y, x)), (y, x, n)


@pytest.mark.parametrize("spp", [1, 4])
def test_adaptive_tiles_equal_the_uniform_accumulation_at_their_own_count(scene_data, spp):
    d = scene_data
    ctx = Ctx(d["scene"])
    counts = set()
    for thr in thresholds(d["E"]):
        out = run_adaptive(ctx, spp, 2, N, thr)
        _, samples, _, _ = ctx.r.adaptive_read(W, H)
        assert_tiles_equal_uniform(ctx.r.readback(out), samples, d["uni"])
        counts |= set(samples.ravel().tolist())
    ctx.close()
    assert len(counts) >= 3, counts               # tiles retired at several different counts


@pytest.mark.parametrize("spp,min_s", [(1, 2), (2, 3), (4, 2)])
def test_retirement_error_and_half_buffer_are_predicted_exactly(scene_data, spp, min_s):
    d = scene_data
    # the numpy fold of the raw samples reproduces the GPU's uniform accumulation bit for bit
    for n in range(1, N + 1):
        assert np.array_equal(d["I"][n - 1], d["uni"][n - 1]), n
    ctx = Ctx(d["scene"])
    for thr in thresholds(d["E"]):
        want_samples, want_err, _ = ar.predict(lambda n: d["E"][n], spp, min_s, N, thr, d["E"][1].shape)
        out = run_adaptive(ctx, spp, min_s, N, thr)
        active, samples, err, half = ctx.r.adaptive_read(W, H)
        assert active == 0
        assert np.array_equal(samples, want_samples), (thr, samples, want_samples)
        assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32)), (thr, err, want_err)
        want64 = np.zeros(err.shape)
        for y, x in np.ndindex(err.shape):
            want64[y, x] = d["E64"][int(samples[y, x])][y, x]
        fin = np.isfinite(want64)
        assert np.array_equal(np.isfinite(err), fin)
        assert np.all(np.abs(err[fin] - want64[fin]) <= 1e-6 * np.abs(want64[fin]))
        for y, x in np.ndindex(samples.shape):
            n = int(samples[y, x])
            assert np.array_equal(ar.tile_view(half, y, x), ar.tile_view(d["A"][n - 1], y, x)), (y, x, n)
            assert np.array_equal(ar.tile_view(ctx.r.readback(out), y, x), ar.tile_view(d["I"][n - 1], y, x))
    ctx.close()


def test_retired_tiles_cost_no_rays_and_are_not_written(scene_data):
    d = scene_data
    ctx = Ctx(d["scene"])
    r = ctx.r
    pix = ar.tile_pixels(W, H)
    thr = thresholds(d["E"])[1]
    spp, min_s = 2, 2
    r.set_samples_per_trace(spp)
    r.set_adaptive(min_s, N, thr)
    st = copy_settings(ctx.s.settings)
    out = r.create_output(W, H)
    # a tile is active at the start of a call iff its final count (predicted exactly, see the test above) is past the samples so far
    final, _, _ = ar.predict(lambda n: d["E"][n], spp, min_s, N, thr, pix.shape)
    frame, retired_seen = 0, 0
    prev = None
    while frame < N and (final > frame).any():
        active_mask = final > frame
        r.reset_stats()
        r.trace(st, ctx.params(frame), out)
        got = r.stats().rays_primary
        assert got == int((pix * active_mask).sum()) * spp, (frame, got)
        assert r.adaptive_read(W, H)[0] == int((final > frame + spp).sum())
        img = r.readback(out)
        if prev is not None:
            for y, x in zip(*np.nonzero(~active_mask)):
                assert ar.tile_view(img, y, x).tobytes() == ar.tile_view(prev, y, x).tobytes()
                retired_seen += 1
        prev = img
        frame += spp
    assert retired_seen > 0
    assert np.array_equal(r.adaptive_read(W, H)[1], final)
    ctx.close()


def test_constant_background_tiles_retire_at_the_first_boundary_with_zero_error():
    s = sky_scene()
    raw, _ = raw_and_uniform(s, 4)
    stack = np.stack([x[..., :3] for x in raw])
    ty, tx = (H + 15) // 16, (W + 15) // 16
    const = np.ones((ty * 16, tx * 16), bool)                       # pixels outside the image do not count
    const[:H, :W] = np.all(stack == stack[0:1], axis=(0, 3))        # per pixel: every sample equal
    const_tile = const.reshape(ty, 16, tx, 16).all(axis=(1, 3))
    assert const_tile.any() and not const_tile.all(), const_tile
    ctx = Ctx(s, env=False)
    run_adaptive(ctx, 2, 3, 12, 0.0)                                # boundaries 2, 4, ...: the first at or after min_samples = 3 is 4
    _, samples, err, _ = ctx.r.adaptive_read(W, H)
    assert np.all(samples[const_tile] == 4) and np.all(err[const_tile] == 0.0), (samples, err)
    assert np.all(samples[~const_tile] == 12)                       # threshold 0: a tile with any variation runs to the maximum
    ctx.close()


def test_a_lower_threshold_never_gives_a_tile_fewer_samples(scene_data):
    d = scene_data
    ctx = Ctx(d["scene"])
    prev = None
    for thr in [1e30] + sorted(thresholds(d["E"]), reverse=True) + [0.0]:
        run_adaptive(ctx, 1, 2, N, thr)
        _, samples, _, _ = ctx.r.adaptive_read(W, H)
        if prev is not None:
            assert np.all(samples >= prev), (thr, samples, prev)
        prev = samples
    assert np.all(prev == N) or np.any(prev > 2)
    ctx.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_tile_shards_compose_to_the_one_rank_adaptive_image(scene_data, ranks):
    d = scene_data
    thr = thresholds(d["E"])[1]
    one = Ctx(d["scene"])
    img1 = one.r.readback(run_adaptive(one, 2, 2, N, thr))
    _, samples1, err1, half1 = one.r.adaptive_read(W, H)
    one.close()
    comp = np.zeros_like(img1)
    samples, err, half = np.zeros_like(samples1), np.zeros_like(err1), np.zeros_like(half1)
    ty, tx = samples1.shape
    for rank in range(ranks):
        c = Ctx(d["scene"])
        img = c.r.readback(run_adaptive(c, 2, 2, N, thr, kw=dict(tile_rank=rank, tile_rank_count=ranks)))
        _, s_r, e_r, h_r = c.r.adaptive_read(W, H)
        c.close()
        for g in range(ty * tx):
            y, x = divmod(g, tx)
            if g % ranks == rank:
                ar.tile_view(comp, y, x)[...] = ar.tile_view(img, y, x)
                ar.tile_view(half, y, x)[...] = ar.tile_view(h_r, y, x)
                assert s_r[y, x] > 0
            else:
                assert s_r[y, x] == 0 and e_r[y, x] == 0      # another rank's tile reads 0
        samples += s_r
        err += e_r
    assert np.array_equal(samples, samples1)
    assert np.array_equal(err.view(np.uint32), err1.view(np.uint32))
    assert np.array_equal(comp, img1)
    assert np.array_equal(half, half1)


def test_resets_restart_with_every_tile_active(scene_data):
    d = scene_data
    ctx = Ctx(d["scene"])
    r = ctx.r
    ntiles = d["E"][1].size
    thr = thresholds(d["E"])[2]
    out = run_adaptive(ctx, 2, 2, N, thr)
    assert r.adaptive_read(W, H)[0] == 0
    st = copy_settings(ctx.s.settings)
    r.set_samples_per_trace(1)

    def check_restarted():
        active, samples, _, _ = r.adaptive_read(W, H)
        assert active == ntiles and np.all(samples == 1)           # min_samples 2: nothing retires after one sample

    # settings.reset
    st.reset = 1
    r.trace(st, ctx.params(0), out); st.reset = 0
    check_restarted()
    assert np.array_equal(r.readback(out), d["uni"][0])
    for f in range(1, 6):
        r.trace(st, ctx.params(f), out)
    assert r.adaptive_read(W, H)[0] < ntiles
    # a camera change
    p = ctx.params(6)
    p.world_to_view[:] = camera.cm(camera.orbit_world_to_view((0, 0, 0.6), 3.7, 0.35, -0.45))
    r.trace(st, p, out)
    check_restarted()
    for f in range(7, 12):
        r.trace(st, ctx.params(f), out)
    # pt_set_adaptive
    r.set_adaptive(2, N, thr)
    r.trace(st, ctx.params(0), out)
    check_restarted()
    assert np.array_equal(r.readback(out), d["uni"][0])
    ctx.close()


def test_calls_outside_adaptive_mode_are_untouched(scene_data):
    d = scene_data
    s = d["scene"]
    a, ref = Ctx(s), Ctx(s)                                          # `ref` never enables adaptive sampling
    a.r.set_adaptive(2, N, thresholds(d["E"])[1])
    a.r.set_samples_per_trace(4); ref.r.set_samples_per_trace(4)
    oa, orf = a.r.create_output(W, H), ref.r.create_output(W, H)
    # without FLAG_ACCUMULATE
    st = copy_settings(s.settings); st.flags &= ~abi.FLAG_ACCUMULATE
    for f in (3, 4):
        a.r.trace(st, a.params(f), oa); ref.r.trace(st, ref.params(f), orf)
        assert np.array_equal(a.r.readback(oa), ref.r.readback(orf))
    # with a debug output (and FLAG_ACCUMULATE)
    st = copy_settings(s.settings); st.debug_output = abi.DEBUG_OUTPUT_SHADING_NORMAL; st.reset = 1
    for f in (5, 6):
        a.r.trace(st, a.params(f), oa); ref.r.trace(st, ref.params(f), orf); st.reset = 0
        assert np.array_equal(a.r.readback(oa), ref.r.readback(orf))
    # an adaptive run, then enable = 0: traces are those of a context that never enabled it
    run_adaptive(a, 2, 2, N, thresholds(d["E"])[1])
    a.r.set_adaptive(2, N, 0.0, enable=False)
    st = copy_settings(s.settings)
    oa = a.r.create_output(W, H)
    ref.close(); ref = Ctx(s); ref.r.set_samples_per_trace(2); orf = ref.r.create_output(W, H)
    for f in (0, 2, 4):
        a.r.trace(st, a.params(f), oa); ref.r.trace(st, ref.params(f), orf)
        assert np.array_equal(a.r.readback(oa), ref.r.readback(orf))
    assert np.array_equal(a.r.readback(oa), d["uni"][5])
    a.close(); ref.close()


def test_max_accumulated_frames_caps_the_tiles(scene_data):
    d = scene_data
    ctx = Ctx(d["scene"])
    st = copy_settings(d["scene"].settings); st.max_accumulated_frames = 5
    out = run_adaptive(ctx, 2, 2, N, 0.0, st=st)                    # calls of 2, 2, then 1 (clamped)
    active, samples, _, _ = ctx.r.adaptive_read(W, H)
    assert active == 0 and samples.max() == 5 and ctx.r.stats().accumulated_frames == 5
    assert_tiles_equal_uniform(ctx.r.readback(out), samples, d["uni"])
    before = ctx.r.readback(out)
    ctx.r.trace(st, ctx.params(10), out)                            # past the cap: a no-op
    assert np.array_equal(ctx.r.readback(out), before) and ctx.r.stats().accumulated_frames == 5
    ctx.close()


def test_argument_errors_not_ready_and_the_megakernel_refusal(scene_data):
    d = scene_data
    ctx = Ctx(d["scene"])
    r = ctx.r
    L = r.L

    def set_rc(enable, mn, mx, thr):
        cfg = abi.PtAdaptiveConfig(enable, mn, mx, thr)
        return L.pt_set_adaptive(r.h, C.byref(cfg))

    assert set_rc(1, 1, 8, 0.1) == -1                                # min_samples < 2
    assert set_rc(1, 4, 3, 0.1) == -1                                # max_samples < min_samples
    assert set_rc(1, 2, 8, -0.5) == -1
    assert set_rc(1, 2, 8, float("nan")) == -1
    assert set_rc(1, 2, 8, float("inf")) == -1
    assert L.pt_set_adaptive(r.h, None) == -1
    assert set_rc(0, 0, 0, 0.0) == 0                                 # a disabled config is not checked
    assert set_rc(1, 2, 2, 0.0) == 0
    n = C.c_int32()
    assert L.pt_adaptive_read(r.h, W, H, C.byref(n), None, None, None) == -6     # before the first adaptive trace
    st = copy_settings(d["scene"].settings)
    out = r.create_output(W, H)
    r.trace(st, ctx.params(0), out)
    assert L.pt_adaptive_read(r.h, W, H, C.byref(n), None, None, None) == 0 and n.value == ar.tile_pixels(W, H).size
    assert L.pt_adaptive_read(r.h, W + 1, H, C.byref(n), None, None, None) == -1
    assert L.pt_adaptive_read(r.h, W, H - 16, None, None, None, None) == -1
    # megakernel: refused, the output untouched
    r.set_kernel_mode(abi.MODE_MEGAKERNEL)
    out.fill_(7.0)
    p = ctx.params(1)
    p.output = out.data_ptr()
    assert L.pt_trace(r.h, C.byref(st), C.byref(p)) == -1
    assert np.all(r.readback(out) == 7.0)
    # ... but a call outside adaptive mode runs as always
    st2 = copy_settings(st); st2.flags &= ~abi.FLAG_ACCUMULATE
    r.trace(st2, ctx.params(1), out)
    assert not np.all(r.readback(out) == 7.0)
    ctx.close()
