"""Thin-lens depth of field (include/mipt.h pt_set_lens, pt_lens_focus_at) on the MI355X.

The camera rays come out of the test hook pt_debug_camera_rays, which runs the kernels' own camera_ray under the context's lens; they are
held to tests/lens_ref.py, a float64 restatement of the header's definition fed with the oracle's random numbers, within
    bound = 64 * 2^-24 * M,   M = the largest magnitude among o, c, P and focus_distance of the query
(64 float32 roundings between the inputs and the lens ray, counted in tests/lens_ref.py; a length such as tmax is held to 64 * 2^-24 of
itself).  Everything else is bit for bit: that pt_trace traces exactly the hook's rays, that a lens that is off changes nothing, and that
the lens composes with batches, tile shards, adaptive sampling and checkpoints.  Radius 0.25 and focus distance 1 put all of the scene's
geometry at least 4 pixels out of focus (asserted below): a lens that is accepted and ignored fails items 2(f), 3 and 4."""
import ctypes as C
import math

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes
from tests import hooks
from tests import adaptive_ref as ar
from tests import lens_ref as lr
from tests import ray_hook

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, H = 72, 40                      # 5 x 3 tiles, ragged in both directions (the frame of tests/test_gpu_aov.py)
N = 8
ENV = (0.25, 0.5, 0.75)
APERTURE, FOCUS = 0.25, 1.0         # the floor comes as near as depth 2: focused in front of everything, so that nothing is sharp
LENSES = {"disc": (0, 0.0), "pentagon": (5, 0.37), "triangle": (3, -1.1)}
ULP1 = 2.0 ** -23                  # the spacing of float32 at 1


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def small_scene():
    """test_scene without an environment map from a distance at which about a quarter of the picture is geometry (tests/test_gpu_aov.py)."""
    s = scenes.test_scene(W, 16, with_env=False)
    s.width, s.height = W, H
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.6), 5.0, 0.35, -0.45)
    s.settings.environment_color[:] = ENV
    s.settings.max_accumulated_frames = 64
    return s


def quad_scene():
    """One quad facing the camera at view-space depth 4 (tests/lens_ref.py QUAD_*), default material, constant environment."""
    s = scenes.SceneData("lens_quad")
    x, z = lr.QUAD_HALF_X, lr.QUAD_HALF_Z
    s.add_mesh(meshgen.grid(1, 1, (-x, lr.QUAD_Y, -z), (2 * x, 0, 0), (0, 0, 2 * z)), None, 0)
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0), lr.QUAD_CAMERA, 0.0, 0.0)
    s.width, s.height = W, H
    st = abi.PtSettings.app_defaults()
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    st.environment_color[:] = ENV
    s.settings = st
    return s


class Ctx:
    """A renderer with the scene uploaded, an output and (aov) the two AOV targets; lens = None (never set) or set_lens's arguments."""

    def __init__(self, s, lens=None, aov=True, mode=None):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        s.upload(self.r)
        self.out = self.r.create_output(s.width, s.height)
        self.alb = self.r.create_output(s.width, s.height) if aov else None
        self.nd = self.r.create_output(s.width, s.height) if aov else None
        if mode is not None:
            self.r.set_kernel_mode(mode)
        if aov:
            self.r.set_aov(self.alb, self.nd)
        if lens is not None:
            self.r.set_lens(*lens)

    def trace(self, st, frame, out=None, **kw):
        self.r.trace(st, self.s.execute_params(frame, **kw), self.out if out is None else out)

    def read(self):
        return tuple(self.r.readback(t) if t is not None else None for t in (self.out, self.alb, self.nd))

    def close(self):
        self.r.close()


ON = (APERTURE, FOCUS)


def hook_rays(r, st, params, queries):
    """pt_debug_camera_rays: queries [n, 3] uint32 {px, py, seed} -> [n, 8] float32 (origin, tmin, direction, tmax)."""
    q = np.ascontiguousarray(queries, np.uint32).reshape(-1, 3)
    out = np.zeros((len(q), 8), f32)
    f = hooks.lib().pt_debug_camera_rays
    rc = f(r.h, C.byref(st), C.byref(params), q.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (rc, r.L.pt_last_error(r.h))
    return out


def pixel_queries(seeds):
    """{px, py, seed} for every pixel and seed, in the order [seed, y, x] of lens_ref.randoms."""
    sd, y, x = np.meshgrid(np.asarray(list(seeds), np.uint32), np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), sd.ravel()], axis=1)


@pytest.fixture(scope="module")
def rnd(oracle_lib):
    """orc_random(px, py, seed, 0) for seeds 0 .. 15 (bit-identical to the product's by tests/test_gpu_parity.py)."""
    return lr.randoms(oracle_lib, W, H, range(16))


@pytest.fixture(scope="module")
def scene():
    return small_scene()


def rf_of(st):
    return ray_hook.RF_CULL_BACK if st.flags & abi.FLAG_CULL_BACKFACE else 0


# ---- 1. off is off ---------------------------------------------------------------------------------------------------------------------
def run_config(s, lens, batch, mode):
    """8 accumulated frames: (output, albedo, normal_depth, ray counts); the megakernel writes no AOVs."""
    aov = mode == abi.MODE_WAVEFRONT
    c = Ctx(s, lens=lens, aov=aov, mode=mode)
    c.r.set_samples_per_trace(batch)
    st = copy_settings(s.settings); st.reset = 1
    c.r.reset_stats()
    for f in range(0, N, batch):
        c.trace(st, f); st.reset = 0
    img = c.read()
    t = c.r.stats()
    assert t.accumulated_frames == N
    c.close()
    return img, (t.rays, t.rays_primary, t.rays_bounce, t.rays_shadow, t.closest_hits)


@pytest.mark.parametrize("batch,mode", [(1, abi.MODE_WAVEFRONT), (4, abi.MODE_WAVEFRONT), (1, abi.MODE_MEGAKERNEL)])
def test_a_lens_that_is_off_changes_nothing(scene, batch, mode):
    """Never set, enable = 0 (with a radius that would blur) and enable = 1 with radius 0: output, both AOV targets and the ray counts of 8
    accumulated frames, bit for bit.  Control: the lens switched on does change the picture."""
    want, rays = run_config(scene, None, batch, mode)
    for lens in ((APERTURE, FOCUS, 5, 0.3, False), (0.0, FOCUS, 5, 0.3, True)):
        got, rays_got = run_config(scene, lens, batch, mode)
        for a, b in zip(got, want):
            assert (a is None and b is None) or same(a, b), lens
        assert rays_got == rays, (lens, rays_got, rays)
    on, _ = run_config(scene, ON, batch, mode)
    assert (bits(on[0]) != bits(want[0])).any(axis=-1).mean() > 0.1


# ---- 2. the rays are the definition ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hook_ctx(scene):
    c = Ctx(scene, aov=False)
    yield c
    c.close()


@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])
@pytest.mark.parametrize("shape", list(LENSES))
def test_camera_rays_are_the_definition(hook_ctx, scene, rnd, oracle_lib, shape, ortho):
    """Every pixel at seeds 0 .. 7 through pt_debug_camera_rays, lens off and lens on, against tests/lens_ref.py in float64 with the oracle's
    random numbers (and, for the disc, the oracle's square_to_disk(uv_to_square(.))).  Bound: 64 * 2^-24 * M per query -- 64 float32
    roundings, each at most 2^-24 of the largest operand (the count: pinhole ray 17, focus point and lens-plane crossing 18, lens sample and
    lens point 13, direction and origin 16; tests/lens_ref.py).
      (a) the lens ray's line passes the lens-off ray's focus point P;  (b) the lens point -- the ray taken back to depth 0, projected on R,
      U -- is aperture_radius * L(r.z, r.w) and lies inside the aperture;  (c) the origin is on the near plane: dot(o' - c, F) = zo;
      (d) d' is unit within 4 ulp, tmin = 0, tmax is the pinhole's bit for bit;  (e) control: the lens-off rays are the restatement's pinhole
      rays;  (f) control: more than 99 % of the lens-on rays differ from their lens-off ray."""
    blades, rot = LENSES[shape]
    r, st = hook_ctx.r, scene.settings
    saved = scene.ortho
    scene.ortho = (0.25, 0.45) if ortho else None
    params = scene.execute_params(0)
    scene.ortho = saved
    q = pixel_queries(range(N))
    r.set_lens(APERTURE, FOCUS, blades, rot, False)
    off = hook_rays(r, st, params, q)
    r.set_lens(APERTURE, FOCUS, blades, rot)
    on = hook_rays(r, st, params, q)
    r.set_lens(0, 1, enable=False)
    cam = lr.Camera(params.world_to_view, params.view_to_clip, W, H)
    rn = rnd[:N].reshape(-1, 4)
    sx, sy = lr.jittered(rnd[:N], W, H)
    o_ref, d_ref, tmax_ref = lr.pinhole_ray(cam, sx.ravel(), sy.ravel())
    o, d, tmax = off[:, 0:3].astype(f64), off[:, 4:7].astype(f64), off[:, 7].astype(f64)
    o2, d2 = on[:, 0:3].astype(f64), on[:, 4:7].astype(f64)
    P, zo, dn = lr.focus_point(cam, o, d, FOCUS)                    # of the product's own lens-off ray
    b = lr.bound(o, o2, cam.c[None], P, FOCUS)
    report = {}
    # (e) control: the pinhole rays
    report["e origin"] = np.abs(o - o_ref).max(axis=1) / b
    report["e direction"] = np.abs(d - d_ref).max(axis=1) / b
    report["e tmax"] = np.abs(tmax - tmax_ref) / (lr.BOUND_ROUNDINGS * 2.0 ** -24 * tmax_ref)
    # (a) focus
    report["a focus"] = lr.distance_to_line(P, o2, d2) / b
    # (b) lens sample
    L = lr.oracle_disk(oracle_lib, rn[:, 2], rn[:, 3]) if blades == 0 else lr.polygon_sample(blades, rot, rn[:, 2], rn[:, 3])
    # about the lens-off ray's own crossing A of the lens plane: c for the perspective camera, the pixel's own point for the orthographic one
    got, _ = lr.lens_point_of(cam, o2, d2, centre=lr.lens_point_of(cam, o, d)[1])
    report["b lens sample"] = np.abs(got - APERTURE * L).max(axis=1) / b
    if blades == 0:
        inside = np.sqrt((got ** 2).sum(axis=1)) <= APERTURE + b
    else:
        inside = lr.inside_polygon(APERTURE * lr.polygon_vertices(blades, rot), got, slack=b)
    # (c) near plane
    report["c near plane"] = np.abs(lr.dot(o2 - cam.c, cam.F) - zo) / b
    for name, v in report.items():
        print("%-16s worst %.4f of the bound" % (name, float(v.max())))
    unit = np.abs(np.sqrt(lr.dot(d2, d2)) - 1)
    print("d unit           worst %.2f ulp; rays moved %.4f" % (float(unit.max() / ULP1), float((on[:, 0:7] != off[:, 0:7]).any(axis=1).mean())))
    for name, v in report.items():
        assert (v <= 1.0).all(), (name, float(v.max()))
    assert inside.all(), int((~inside).sum())
    assert (unit <= 4 * ULP1).all()                                                              # (d)
    assert (bits(on[:, 3]) == 0).all() and (bits(off[:, 3]) == 0).all()
    assert np.array_equal(bits(on[:, 7]), bits(off[:, 7]))
    assert (on[:, 0:7] != off[:, 0:7]).any(axis=1).mean() > 0.99                                 # (f)
    # the lens samples fill the aperture: some reach beyond 95 % of its circumradius, their centroid is at the lens centre
    assert np.sqrt((got ** 2).sum(axis=1)).max() > 0.95 * APERTURE and np.abs(got.mean(axis=0)).max() < 0.02 * APERTURE


# ---- 3. pt_trace traces exactly those rays ---------------------------------------------------------------------------------------------
def test_the_circle_of_confusion_on_the_nearest_geometry_is_at_least_four_pixels(hook_ctx, scene):
    """The parameters of this file: view-space depth z of what the centre rays see, blur diameter 2 a |z - f| / f at that depth, a pixel
    being 2 z / H there (y_fov = 90 degrees)."""
    r, st = hook_ctx.r, scene.settings
    z = [r.focus_at(st, scene.execute_params(0), x + 0.5, y + 0.5) for y in range(0, H, 2) for x in range(0, W, 2)]
    z = np.array([v for v in z if v is not None])
    assert len(z) > 50
    px = 2 * APERTURE * np.abs(z - FOCUS) / FOCUS / (2 * z / H)
    print("depths %.2f .. %.2f, circle of confusion %.1f .. %.1f pixels" % (z.min(), z.max(), px.min(), px.max()))
    assert px.min() >= 4.0 and scene.y_fov == math.pi / 2


def test_trace_traces_exactly_the_hooks_rays(scene, oracle_lib):
    """Single-sample frames 0 .. 7 with the lens and the AOVs on: normal_depth.w is, bit for bit, the t that pt_debug_intersect finds along
    the hook's ray of (px, py, seed = frame), albedo.w is 1 exactly where that ray hits, and the oracle's traversal finds the same hits
    along those rays."""
    st = copy_settings(scene.settings); st.flags &= ~abi.FLAG_ACCUMULATE
    assert st.use_frame_as_seed
    c = Ctx(scene, lens=ON)
    o = oracle_lib.Oracle()
    scene.upload(o)
    hits = 0
    for f in range(N):
        c.trace(st, f)
        _, alb, nd = c.read()
        rays = hook_rays(c.r, st, scene.execute_params(f), pixel_queries([f]))
        g = ray_hook.gpu_intersect(c.r, rays, rf_of(st), 0)
        hit = g[:, 0] > 0
        assert same(nd[..., 3].ravel(), np.where(hit, g[:, 1], f32(0))), f
        assert np.array_equal(alb[..., 3].ravel(), hit.astype(f32)), f
        ref = o.intersect_many(rays, ray_hook.dxr_flags(rf_of(st)), 0)
        assert np.array_equal(bits(g[:, 0:7]), bits(ref[:, 0:7])), (f, int((bits(g[:, 0:7]) != bits(ref[:, 0:7])).any(axis=1).sum()))
        hits += int(hit.sum())
    c.close(); o.close()
    assert 0.05 < hits / (N * W * H) < 0.95


def test_the_megakernel_traces_the_same_lens_rays(scene):
    """Megakernel mode writes no AOVs: a first-vertex debug image with the lens on equals the wavefront mode's bit for bit.  The output is
    SHADING_NORMAL if the two modes agree on it with the lens OFF (the control), else the first of VERTEX_NORMAL, HIT_KIND on which they do."""
    def frames(dbg, lens, mode):
        st = copy_settings(scene.settings); st.debug_output = dbg
        c = Ctx(scene, lens=lens, aov=False, mode=mode)
        out = []
        for f in range(3):
            c.trace(st, f)
            out.append(c.read()[0])
        c.close()
        return np.stack(out)

    chosen = None
    for dbg in (abi.DEBUG_OUTPUT_SHADING_NORMAL, abi.DEBUG_OUTPUT_VERTEX_NORMAL, abi.DEBUG_OUTPUT_HIT_KIND):
        off_wf = frames(dbg, None, abi.MODE_WAVEFRONT)
        if same(off_wf, frames(dbg, None, abi.MODE_MEGAKERNEL)):                                     # control: lens off
            chosen = dbg
            break
    assert chosen is not None, "the two kernel modes agree on no first-vertex debug output even without a lens"
    print("debug output compared:", abi.DEBUG_OUTPUT_NAMES[chosen])
    on_wf = frames(chosen, ON, abi.MODE_WAVEFRONT)
    assert same(on_wf, frames(chosen, ON, abi.MODE_MEGAKERNEL))
    assert (bits(on_wf) != bits(off_wf)).any(axis=-1).mean() > 0.05


# ---- 4. a blurred edge, sample for sample ----------------------------------------------------------------------------------------------
def test_a_blurred_quad_edge_sample_for_sample(rnd):
    """One quad at depth 4, focus at 2: single-sample coverage (albedo.w) of frames 0 .. 15 against the restatement's lens rays intersected
    with the quad's plane in float64.  Hit or miss must agree except where the restatement's ray passes within the bound of item 2 of a
    quad edge (or of the diagonal the two triangles share); tests/test_lens_host.py holds that share below 0.5 % (it is below 0.01 %)."""
    s = quad_scene()
    frames = 16
    st = copy_settings(s.settings); st.flags &= ~abi.FLAG_ACCUMULATE
    c = Ctx(s, lens=(lr.QUAD_APERTURE, lr.QUAD_FOCUS))
    cov = []
    for f in range(frames):
        c.trace(st, f)
        cov.append(c.read()[1][..., 3])
    params = s.execute_params(0)
    c.close()
    cov = np.stack(cov).ravel()
    assert set(np.unique(cov).tolist()) <= {0.0, 1.0}
    cam = lr.Camera(params.world_to_view, params.view_to_clip, W, H)
    sx, sy = lr.jittered(rnd[:frames], W, H)
    o, d, tmax = lr.pinhole_ray(cam, sx.ravel(), sy.ravel())
    L = lr.disk_sample(rnd[:frames, ..., 2].ravel(), rnd[:frames, ..., 3].ravel())
    o2, d2, tmax2, P, A2, zo = lr.lens_ray(cam, o, d, tmax, L, lr.QUAD_APERTURE, lr.QUAD_FOCUS)
    hit, near = lr.quad_coverage(o2, d2, tmax2, lr.bound(o2, cam.c[None], P, lr.QUAD_FOCUS))
    hit0, _ = lr.quad_coverage(o, d, tmax, 0.0)
    wrong = (cov > 0) != hit
    print("left out %.5f; hit %.3f; disagreements %d (near an edge %d); a pinhole would disagree on %d" %
          (near.mean(), hit.mean(), int(wrong.sum()), int((wrong & near).sum()), int(((cov > 0) != hit0).sum())))
    assert near.mean() <= 0.005
    assert not (wrong & ~near).any(), int((wrong & ~near).sum())
    assert ((cov > 0) != hit0).mean() > 0.02                      # an ignored lens could not pass


# ---- 5. composition with the lens on ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uniform(scene):
    """The uninterrupted accumulation with the lens on, traced frame by frame: snapshots [n - 1] = (output, albedo, normal_depth)."""
    c = Ctx(scene, lens=ON)
    st = copy_settings(scene.settings); st.reset = 1
    snaps = []
    for f in range(N):
        c.trace(st, f); st.reset = 0
        snaps.append(c.read())
    c.close()
    return snaps


def test_a_batch_of_four_equals_four_calls(scene, uniform):
    c = Ctx(scene, lens=ON)
    c.r.set_samples_per_trace(4)
    st = copy_settings(scene.settings); st.reset = 1
    for f in (0, 4):
        c.trace(st, f); st.reset = 0
        for a, b in zip(c.read(), uniform[f + 3]):
            assert same(a, b), f
    c.close()


def test_three_tile_shards_pack_to_the_one_rank_image(scene, uniform):
    ranks = 3
    root = Ctx(scene, lens=ON)
    dst = [root.r.create_output(W, H) for _ in range(3)]
    for k in range(ranks):
        c = Ctx(scene, lens=ON)
        st = copy_settings(scene.settings); st.reset = 1
        for f in range(N):
            c.trace(st, f, tile_rank=k, tile_rank_count=ranks); st.reset = 0
        for img, into in zip((c.out, c.alb, c.nd), dst):
            packed = c.r.tiles_pack(img, k, ranks)
            assert packed.numel() * 4 == c.r.tiles_packed_bytes(W, H, k, ranks)
            root.r.tiles_unpack(packed.clone(), into, k, ranks)
        c.r.readback(c.out)                                          # the pack has run before the context goes
        c.close()
    for into, want in zip(dst, uniform[N - 1]):
        assert same(root.r.readback(into), want)
    root.close()


def test_adaptive_tiles_equal_the_uniform_accumulation_at_their_own_counts(scene, uniform):
    """tests/adaptive_ref.py's rule with the lens on: tile t of every image equals tile t of the uniform accumulation after tile_samples[t]."""
    # a threshold between the tiles' errors after 4 samples, so that tiles retire at different counts
    I = [u[0] for u in uniform]
    _, A = ar.fold([u for u in raw_frames(scene)])
    E4 = np.sort(ar.tile_errors(I[3], A[3]).ravel())
    thr = float(E4[len(E4) // 2])
    c = Ctx(scene, lens=ON)
    c.r.set_adaptive(2, N, thr)
    st = copy_settings(scene.settings)
    active, f = 1, 0
    while active and f < N:
        c.trace(st, f); f += 1
        active = c.r.adaptive_read(W, H)[0]
    _, samples, _, _ = c.r.adaptive_read(W, H)
    imgs = c.read()
    c.close()
    assert len(set(samples.ravel().tolist())) >= 2, samples
    for y in range(samples.shape[0]):
        for x in range(samples.shape[1]):
            n = int(samples[y, x])
            assert n >= 2
            for got, want in zip(imgs, uniform[n - 1]):
                assert same(ar.tile_view(got, y, x), ar.tile_view(want, y, x)), (y, x, n)


def raw_frames(s):
    """The single samples of frames 0 .. N - 1 with the lens on (accumulation off)."""
    c = Ctx(s, lens=ON, aov=False)
    st = copy_settings(s.settings); st.flags &= ~abi.FLAG_ACCUMULATE
    raw = []
    for f in range(N):
        c.trace(st, f)
        raw.append(c.read()[0])
    c.close()
    return raw


def test_save_destroy_create_set_lens_load_continue_equals_the_uninterrupted_run(scene, uniform):
    a = Ctx(scene, lens=ON)
    st = copy_settings(scene.settings); st.reset = 1
    for f in range(3):
        a.trace(st, f); st.reset = 0
    blob = a.r.accum_save(W, H, a.out, a.alb, a.nd, next_frame=3)
    a.close()
    b = Ctx(scene, lens=ON)                                          # the lens is a setting, not part of the blob: set before the load
    info = b.r.accum_load(blob, b.out, b.alb, b.nd)
    assert info.accumulated_frames == 3 and info.next_frame == 3
    for f in range(3, N):
        b.trace(st, f)
        for x, y in zip(b.read(), uniform[f]):
            assert same(x, y), f
    assert b.r.stats().accumulated_frames == N
    b.close()


# ---- 6. restart and validation ---------------------------------------------------------------------------------------------------------
def test_set_lens_restarts_the_accumulation_and_refuses_bad_configs(scene):
    c = Ctx(scene, lens=ON)
    L, h = c.r.L, c.r.h
    st = copy_settings(scene.settings); st.reset = 1
    for f in range(3):
        c.trace(st, f); st.reset = 0
    assert c.r.stats().accumulated_frames == 3

    def set_rc(enable, radius, focus, blades, rot):
        cfg = abi.PtLensConfig(enable, radius, focus, blades, rot)
        rc = L.pt_set_lens(h, C.byref(cfg))
        return rc, L.pt_last_error(h).decode()

    nan, inf = float("nan"), float("inf")
    bad = [((1, nan, 2.0, 0, 0.0), "aperture_radius"), ((1, -0.1, 2.0, 0, 0.0), "aperture_radius"), ((1, inf, 2.0, 0, 0.0), "aperture_radius"),
           ((1, 0.5, 0.0, 0, 0.0), "focus_distance"), ((1, 0.5, -1.0, 0, 0.0), "focus_distance"), ((1, 0.5, inf, 0, 0.0), "focus_distance"),
           ((1, 0.5, nan, 0, 0.0), "focus_distance"), ((1, 0.5, 2.0, 1, 0.0), "blades"), ((1, 0.5, 2.0, 2, 0.0), "blades"),
           ((1, 0.5, 2.0, 17, 0.0), "blades"), ((1, 0.5, 2.0, -3, 0.0), "blades"), ((1, 0.5, 2.0, 5, nan), "blade_rotation"),
           ((1, 0.5, 2.0, 5, inf), "blade_rotation")]
    for cfg, field in bad:
        rc, msg = set_rc(*cfg)
        assert rc == -1 and field in msg, (cfg, rc, msg)
    assert L.pt_set_lens(h, None) == -1 and "config" in L.pt_last_error(h).decode()
    # the old config stays and no restart is pending: the accumulation can be saved and goes on -- with the old lens
    blob = c.r.accum_save(W, H, c.out, c.alb, c.nd, next_frame=3)
    assert c.r.accum_inspect(blob).accumulated_frames == 3
    c.trace(st, 3)
    assert c.r.stats().accumulated_frames == 4
    ref = Ctx(scene, lens=ON)
    st2 = copy_settings(scene.settings); st2.reset = 1
    for f in range(4):
        ref.trace(st2, f); st2.reset = 0
    assert same(c.read()[0], ref.read()[0])
    # a config that is not enabled is not checked
    assert set_rc(0, nan, -1.0, 99, inf)[0] == 0
    c.trace(st, 0)
    assert c.r.stats().accumulated_frames == 1
    for f in range(1, 3):
        c.trace(st, f)
    # a good config: nothing to save until the next trace, which starts anew
    assert set_rc(1, 0.25, 3.0, 6, 0.1)[0] == 0
    need = C.c_size_t()
    img = abi.PtAccumImages(c.out.data_ptr(), c.alb.data_ptr(), c.nd.data_ptr())
    assert L.pt_accum_save(h, C.byref(img), W, H, 0, 1, 0, None, 0, C.byref(need)) == -6
    c.trace(st, 3)
    assert c.r.stats().accumulated_frames == 1
    # pt_accum_load clears the pending restart
    assert set_rc(1, APERTURE, FOCUS, 0, 0.0)[0] == 0
    c.r.accum_load(blob, c.out, c.alb, c.nd)
    c.trace(st, 3)
    assert c.r.stats().accumulated_frames == 4
    assert same(c.read()[0], ref.read()[0])
    c.close(); ref.close()


# ---- 7. autofocus ----------------------------------------------------------------------------------------------------------------------
def test_focus_at_is_the_view_space_depth_of_the_hooks_ray(scene, rnd, oracle_lib):
    """pt_lens_focus_at casts the pinhole ray through a position, without jitter or lens.  The hook's lens-off ray of (px, py, seed) is the
    pinhole ray through (px + 0.5) + (r.x - 0.5), (py + 0.5) + (r.y - 0.5): asked for that position, focus_at must return zo + t * dn of
    that ray (float64) with t from the oracle's intersect of it, within the bound of item 2.  A position over the sky is NOT_READY with the output untouched, one outside the image INVALID_ARGUMENT."""
    c = Ctx(scene, lens=ON)                                          # focus_at ignores the lens
    r, st, params = c.r, scene.settings, scene.execute_params(0)
    o = oracle_lib.Oracle()
    scene.upload(o)
    cam = lr.Camera(params.world_to_view, params.view_to_clip, W, H)
    sx, sy = lr.jittered(rnd[:1], W, H)
    picks = [(x, y) for y in range(1, H, 3) for x in range(2, W, 5)]
    r.set_lens(0, 1, enable=False)
    rays = hook_rays(r, st, params, np.array([(x, y, 0) for x, y in picks], np.uint32))
    r.set_lens(*ON)
    hits, sky = 0, []
    for k, (x, y) in enumerate(picks):
        ray = rays[k]
        h = o.intersect(ray[0:3], ray[4:7], 0.0, float(ray[7]), ray_hook.dxr_flags(rf_of(st)))
        got = r.focus_at(st, params, float(sx[0, y, x]), float(sy[0, y, x]))
        if h[0] <= 0:
            assert got is None, (x, y)
            sky.append((float(sx[0, y, x]), float(sy[0, y, x])))
            continue
        hits += 1
        od, dd = ray[0:3].astype(f64), ray[4:7].astype(f64)
        zo, dn = float((od - cam.c) @ cam.F), float(dd @ cam.F)
        want = zo + float(h[1]) * dn
        P = od + dd * float(h[1])
        assert abs(got - want) <= float(lr.bound(od[None], cam.c[None], P[None], want)[0]), (x, y, got, want)
    assert hits >= 20 and sky, (hits, len(sky))
    # sky: NOT_READY, the output value untouched; outside the image and NULL: INVALID_ARGUMENT
    out = C.c_float(-7.5)
    assert r.L.pt_lens_focus_at(r.h, C.byref(st), C.byref(params), sky[0][0], sky[0][1], C.byref(out)) == -6 and out.value == -7.5
    for px, py in ((-0.5, 3.0), (W + 0.5, 3.0), (3.0, -1.0), (3.0, H + 1.0), (float("nan"), 3.0)):
        assert r.L.pt_lens_focus_at(r.h, C.byref(st), C.byref(params), px, py, C.byref(out)) == -1 and out.value == -7.5
    assert r.L.pt_lens_focus_at(r.h, C.byref(st), C.byref(params), 3.0, 3.0, None) == -1
    c.close(); o.close()


def test_focus_at_in_the_middle_of_an_accumulation_changes_nothing(scene, uniform):
    c = Ctx(scene, lens=ON)
    st = copy_settings(scene.settings); st.reset = 1
    for f in range(N):
        c.trace(st, f); st.reset = 0
        for px, py in ((36.5, 28.5), (20.25, 12.0), (1.5, 1.5)):
            c.r.focus_at(st, scene.execute_params(f), px, py)
    for a, b in zip(c.read(), uniform[N - 1]):
        assert same(a, b)
    assert c.r.stats().accumulated_frames == N
    c.close()
