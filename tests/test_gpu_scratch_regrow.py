"""The context's device scratch across a grow and back (run with -m gpu on an MI355X).

Every array of pt_ctx that is reallocated when a call needs more room than the last one left (csrc/pt_ctx.h: each a DevBuf of
csrc/dev_buf.h) is taken small -> large -> small inside one long-lived context A.  After every step A's result is compared bit for bit
(np.array_equal on the raw words) with that of a fresh context B which is set up identically and does only that step: an array that
was reallocated, or kept with room to spare, must not change what the call computes.  Every case ends by destroying A and B and by
creating and destroying one more context.  Sizes are the smallest that cross each slack rule:

  pt_tonemap             need = 16 B a pixel, exact
  pt_denoise             3 float4 a pixel, reallocated whenever the pixel count differs (also when it shrinks)
  pt_trace (wavefront)   workspace, exact; adaptive tile state and half buffer, exact; deep stack, exact
  scene tables           n + n / 2 + 8 rows; accel arrays need + need / 8 + 64 triangles; refit marks n + 64 bytes
  pt_skin_run            bone arena bytes * 8 + 4096
  pt_accum_save / load   one packed image per section, exact"""
import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes
from tests import skin_ref as sr
from tests import traversal_scenes as tscenes
from tests.ray_hook import gpu_intersect

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same(a, b, what):
    assert a.shape == b.shape and np.array_equal(words(a), words(b)), (what, int((words(a) != words(b)).sum()), "words differ")


def teardown(R, *contexts):
    """Both contexts go, and the next one comes and goes, with everything freed once."""
    for r in contexts:
        r.close()
    R().close()


def images(torch, seed, w, h, n):
    """n random (h, w, 4) float32 device images, the same for a given seed."""
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.random((h, w, 4), dtype=f32)).cuda() for _ in range(n)]


# ---- pt_tonemap ---------------------------------------------------------------------------------------------------------------------------
def test_tonemap_scratch_grows_and_is_reused(R):
    import torch
    a = R()
    for k, (w, h) in enumerate([(8, 8), (40, 24), (8, 8)]):
        img, = images(torch, 10 + k, w, h, 1)
        img *= 4.0
        b = R()
        for rgba8 in (False, True):
            ga, gb = a.tonemap(img, want_rgba8=rgba8), b.tonemap(img, want_rgba8=rgba8)
            if rgba8:
                same(ga[1], gb[1], ("tonemap rgba8", w, h))
                ga, gb = ga[0], gb[0]
            same(ga, gb, ("tonemap rgb", w, h, rgba8))
            assert np.isfinite(ga).all() and ga.std() > 0
        b.close()
    teardown(R, a)


# ---- pt_denoise ---------------------------------------------------------------------------------------------------------------------------
def test_denoise_scratch_follows_the_image_size_up_and_down(R):
    import torch
    cfg = abi.PtDenoiseConfig.default()
    cfg.iterations = 2
    a = R()
    for k, (w, h) in enumerate([(16, 16), (48, 32), (16, 16)]):
        color, albedo, nd = images(torch, 20 + k, w, h, 3)
        b = R()
        ga = a.denoise(color, albedo, nd, config=cfg)
        gb = b.denoise(color, albedo, nd, config=cfg)
        torch.cuda.synchronize()
        same(ga.cpu().numpy(), gb.cpu().numpy(), ("denoise", w, h))
        assert not torch.equal(ga, color)
        b.close()
    teardown(R, a)


# ---- pt_trace in the wavefront mode; pt_accum_save / pt_accum_load ------------------------------------------------------------------------
def trace_scene():
    s = tscenes.layered_alpha_scene()
    s.world_to_view = camera.orbit_world_to_view(centre=(0.0, 0.0, 1.75), radius=3.0, inclination=1.0)      # the sheets fill a third of the image
    s.settings.flags = (s.settings.flags | abi.FLAG_ACCUMULATE) & ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    s.settings.environment_color[:] = (1.0, 1.0, 1.0)                          # no map, no lights: the constant colour lights the scene
    s.settings.use_frame_as_seed = 1
    return s


# (width, height, samples per trace, AOVs and adaptive sampling on)
TRACE_STEPS = [(16, 16, 1, False), (64, 48, 4, True), (16, 16, 1, False)]


class Tracing:
    """A context with the scene uploaded; step() configures it for one of TRACE_STEPS and traces one call into fresh images."""

    def __init__(self, R, s):
        self.s, self.r = s, R()
        s.upload(self.r)

    def configure(self, w, h, spp, extras):
        r = self.r
        self.s.width, self.s.height = w, h
        r.set_samples_per_trace(spp)
        self.out = r.create_output(w, h)
        self.aov = (r.create_output(w, h), r.create_output(w, h)) if extras else (None, None)
        r.set_aov(*self.aov)
        r.set_adaptive(2, 16, 0.05, enable=extras)

    def trace(self, frame):
        r = self.r
        r.trace(self.s.settings, self.s.execute_params(frame), self.out)
        return [r.readback(t) for t in (self.out,) + self.aov if t is not None]

    def close(self):
        self.r.close()


def test_trace_workspace_and_adaptive_state_grow_and_are_reused(R):
    s = trace_scene()
    a = Tracing(R, s)
    for k, (w, h, spp, extras) in enumerate(TRACE_STEPS):
        b = Tracing(R, s)
        got = []
        for t in (a, b):
            t.configure(w, h, spp, extras)
            got.append(t.trace(100 * k))
        assert len(got[0]) == (3 if extras else 1)
        for x, y, name in zip(got[0], got[1], ("output", "albedo", "normal_depth")):
            same(x, y, (name, w, h, spp))
        assert got[0][0][..., :3].std() > 0                                    # a picture, not one colour
        if extras:
            assert 0.05 < (got[0][1][..., 3] > 0).mean() < 1.0                 # the sheets cover part of the image: hits and misses
            assert a.r.adaptive_read(w, h)[1].max() == spp
        b.close()
    teardown(R, a)


def test_accum_scratch_grows_and_a_loaded_accumulation_continues_alike(R):
    """After the steps at 16 x 16 and at 64 x 48: A saves, a fresh B loads, both trace once more -- equal images."""
    s = trace_scene()
    a = Tracing(R, s)
    for k, (w, h, spp, extras) in enumerate(TRACE_STEPS[:2]):
        a.configure(w, h, spp, extras)
        a.trace(100 * k)
        blob = a.r.accum_save(w, h, a.out, *a.aov, next_frame=100 * k + spp)
        b = Tracing(R, s)
        b.configure(w, h, spp, extras)
        info = b.r.accum_load(blob, b.out, *b.aov)
        assert info.accumulated_frames == spp and bool(info.sections & 8) == extras      # PT_ACCUM_ADAPTIVE
        ga, gb = a.trace(100 * k + spp), b.trace(100 * k + spp)
        for x, y, name in zip(ga, gb, ("output", "albedo", "normal_depth")):
            same(x, y, ("after load: " + name, w, h, spp))
        assert a.r.stats().accumulated_frames == b.r.stats().accumulated_frames == 2 * spp
        b.close()
    teardown(R, a)


# (AOVs, mattes, motion vectors, adaptive sampling): each record array is in turn in front of and behind a gap the call does not use
PASS_STEPS = [(False, False, False, False), (False, False, True, False), (True, True, True, False), (False, True, False, False),
              (True, False, True, True), (False, False, False, False)]
PASS_SIZES = [(16, 16, 1), (40, 24, 3)]                                         # the second: partial tiles and a batch


def trace_passes(t, w, h, spp, aov, matte, motion, adaptive, frame):
    """One call of context t (a Tracing) with exactly these passes on, into fresh targets.  Returns {name: image} of every target written."""
    r, s = t.r, t.s
    s.width, s.height = w, h
    r.set_samples_per_trace(spp)
    names = ["output"] + ["albedo", "normal_depth"] * aov + ["matte"] * matte + ["motion"] * motion
    img = {n: r.create_output(w, h) for n in names}
    r.set_aov(img.get("albedo"), img.get("normal_depth"))
    r.set_matte(abi.MATTE_INSTANCE, [img["matte"]] if matte else None)
    p = s.execute_params(frame)
    prev = camera.cm(camera.orbit_world_to_view(centre=(0.0, 0.0, 1.75), radius=3.0, inclination=1.05))      # the camera has moved a little
    r.set_motion(img.get("motion"), prev, list(p.view_to_clip)) if motion else r.set_motion(None)
    r.set_adaptive(2, 16, 0.05, enable=adaptive)
    r.trace(s.settings, p, img["output"])
    return {n: r.readback(x) for n, x in img.items()}


def test_record_arrays_keep_their_places_across_pass_combinations(R):
    """The AOV, matte and motion records lie behind the workspace's other arrays at fixed places, whichever of them a call uses.  One
    long-lived context goes through the combinations at two sizes; after every step each target written equals, bit for bit, that of a
    fresh context which does only that step."""
    s = trace_scene()
    a = Tracing(R, s)
    k = 0
    for aov, matte, motion, adaptive in PASS_STEPS:
        for w, h, spp in PASS_SIZES:
            b = Tracing(R, s)
            ga, gb = (trace_passes(t, w, h, spp, aov, matte, motion, adaptive, 100 * k) for t in (a, b))
            assert sorted(ga) == sorted(gb) and len(ga) == 1 + 2 * aov + matte + motion
            for name in ga:
                same(ga[name], gb[name], (name, k, w, h, spp))
                assert ga[name].astype(np.float64).std() > 0, (name, k)        # (an all-zero target must not pass as equal)
            k += 1
            b.close()
    teardown(R, a)


# ---- the deep traversal stack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [abi.MODE_WAVEFRONT, abi.MODE_MEGAKERNEL], ids=["wavefront", "megakernel"])
def test_deep_stack_grows_with_the_launch(R, mode):
    """The tree of test_tree_deeper_than_the_on_chip_stack_is_rendered_not_refused (radix builder) at 16 x 16, then 32 x 32: the megakernel's
    deep stack has an entry set per pixel slot and grows, the wavefront stages' is sized by their grid and is kept.  pt_debug_intersect
    brings a deep stack of its own."""
    s, n = tscenes._deep_chain_scene(size=16)
    st = abi.PtSettings.from_buffer_copy(bytes(s.settings))
    st.flags &= ~abi.FLAG_ACCUMULATE
    rays = np.zeros((256, 8), f32)
    yz = (np.random.default_rng(5).random((256, 2)) - 0.5) * 2.0 ** -12          # inside every sheet
    rays[:, 0] = -0.5; rays[:, 1:3] = yz; rays[:, 4] = 1.0; rays[:, 7] = 1000.0

    def fresh():
        r = R(); r.set_kernel_mode(mode); r.set_accel_builder(abi.BUILDER_LBVH); s.upload(r)
        return r
    a = fresh()
    for size in (16, 32):
        s.width = s.height = size
        b = fresh()
        got = []
        for r in (a, b):
            out = r.create_output(size, size)
            r.reset_stats()
            r.trace(st, s.execute_params(7), out)
            got.append((r.readback(out), gpu_intersect(r, rays)))
            q = r.stats()                                                          # raises if a push was dropped
            assert q.bvh_triangles == n and q.bvh_stack_need > 64 and q.deep_stack_pushes > 0, (q.bvh_stack_need, q.deep_stack_pushes)
        same(got[0][0], got[1][0], ("deep image", size))
        same(got[0][1], got[1][1], ("deep hits", size))
        assert (got[0][1][:, 0] > 0).all() and got[0][0][..., :3].mean() > 0.05
        b.close()
    teardown(R, a)


# ---- scene tables, acceleration structure, refit marks --------------------------------------------------------------------------------------
def tables_scene():
    """Instance 0: one quad (2 triangles); instances 1..69: 3 x 2 quads each (12 triangles), laid out on a 10-wide raster at their own heights
    so that no two triangles share a point."""
    s = scenes.SceneData("regrow_tables")
    s.add_mesh(meshgen.grid(1, 1, (-0.4, -0.4, 0.0), (0.8, 0.0, 0.0), (0.0, 0.8, 0.0)), None, 0)
    part = meshgen.grid(3, 2, (-0.4, -0.4, 0.0), (0.8, 0.0, 0.0), (0.0, 0.8, 0.0))
    for i in range(1, 70):
        s.add_mesh(part, camera.trs((float(i % 10) - 4.5, float(i // 10) - 3.0, 0.1 + 0.01 * i)), 0)
    assert s.triangles >= 600
    return s


def test_scene_tables_and_accel_grow_refit_and_shrink(R):
    s = tables_scene()
    rng = np.random.default_rng(9)
    rays = np.zeros((256, 8), f32)
    rays[:, 0:3] = np.stack([rng.uniform(-5.5, 5.5, 256), rng.uniform(-4, 4, 256), np.full(256, 3.0)], axis=1)
    target = np.stack([rng.uniform(-5.5, 5.5, 256), rng.uniform(-4, 4, 256), np.zeros(256)], axis=1)
    target[::4] = np.stack([rng.uniform(-0.3, 0.3, 64), rng.uniform(-0.3, 0.3, 64), np.zeros(64)], axis=1)      # a quarter at instance 0
    d = target - rays[:, 0:3]
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True); rays[:, 7] = 100.0
    pos0 = s.buffers[s.instances[0].gpu.position_descriptor][0]

    def step(r, h, count, k):
        """The table of `count` instances built in full, then instance 0's vertices moved: the rays meet a refitted tree."""
        r.set_instances(h["instances"][:count])
        r.build_accel()
        r.buffer_update(h["buffers"][s.instances[0].gpu.position_descriptor], pos0 + f32([0.0, 0.0, 0.001 * (k + 1)]))
        hits = gpu_intersect(r, rays)
        q = r.stats()
        return hits, (q.accel_builds, q.accel_refits, q.bvh_triangles)
    a = R(); ha = s.upload(a)
    for k, count in enumerate([1, 70, 1]):
        b = R(); hb = s.upload(b)
        (xa, qa), (xb, qb) = step(a, ha, count, k), step(b, hb, count, k)
        same(xa, xb, ("hits", count))
        assert qa == (k + 1, k + 1, 2 if count == 1 else s.triangles) and qb == (1, 1, qa[2]), (qa, qb)
        assert (xa[::4, 0] > 0).all() and (count == 1 or (xa[:, 0] > 0).mean() > 0.3)
        assert count == 1 or (xa[xa[:, 0] > 0, 4] > 0).any()                  # ... and instances beyond the first are among the hits
        b.close()
    teardown(R, a)


# ---- the bone arena -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1], ids=["k_skin", "k_skin_mfma"])
def test_bone_arena_grows_and_is_reused(R, kernel):
    """2 -> 96 -> 2 bones on 64 vertices: 96 bones do not fit the arena the first call allocates (8 x its own bytes + 4096)."""
    a = R()
    for k, bones in enumerate([2, 96, 2]):
        c = sr.Case("regrow_%d" % bones, 40 + k, 64, bones, "rigid", positive=True)
        assert k != 1 or len(c.bones()) * 128 > 2 * 128 * 8 + 4096
        b = R()
        (pa, ta), (pb, tb) = sr.run(a, c, kernel), sr.run(b, c, kernel)
        same(pa, pb, ("skinned positions", bones))
        same(ta, tb, ("skinned tangent spaces", bones))
        assert not (sr.bits(pa) == sr.POSITION_FILL).any() and not (ta == sr.TANGENT_SPACE_FILL).all()
        b.close()
    teardown(R, a)
