"""Light-probe baking (include/mipt.h pt_set_probes, pt_probe_project) on the MI355X.

The rays come out of the test hook pt_debug_probe_rays, which runs the generate kernel's own ray function, and are held to tests/probe_ref.py
bit for bit (float32 numpy, the direction from the oracle's SquareToSphere).  That pt_trace traces exactly those rays, that an empty cell is
exactly (0, 0, 0, 1), that an escaping ray reads the environment along its direction, and that probes compose with batches, tile shards,
adaptive sampling and checkpoints are bit for bit too.  pt_probe_project is held to the float64 restatement within the derived bound of
probe_ref.projection_bound, and the whole chain -- trace, then project -- to the spherical harmonics of six cube faces the oracle renders
from the probe's position, within the Monte-Carlo error both sides measure on themselves."""
import ctypes as C
import math

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes
from tests import hooks
from gltf_renderer_amd.renderer import MiptError
from tests import lens_ref as lr
from tests import probe_ref as pr
from tests import ray_hook

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
N = 6                                   # frames of the composition tests
# five probes in the lit scene, 16 x 16 each, two to a row: a 32 x 48 atlas whose last cell is empty.  Probe 3 sits inside the occluder box.
POS5 = np.array([(0.5, -0.45, 0.3), (-0.6, 0.5, 0.8), (0.0, 0.0, 0.2), (0.0, 0.0, 0.5), (0.7, 0.7, 1.2)], f32)
N5, C5 = 16, 2
W5, H5 = pr.atlas_size(N5, len(POS5), C5)
MAXD = 50.0


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def base_settings():
    st = abi.PtSettings.app_defaults()
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    st.environment_color[:] = (0.25, 0.5, 0.75)
    st.use_frame_as_seed = 1
    st.max_accumulated_frames = 64
    return st


def lit_scene():
    """The lit scene of the bake tests: a quad in the plane z = 0 over [-1, 1]^2, an occluder box above it, a point light and a constant
    environment."""
    s = scenes.SceneData("probe_lit")
    s.add_mesh(meshgen.Mesh([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], [0, 1, 2, 0, 2, 3], normals=np.repeat([[0.0, 0.0, 1.0]], 4, axis=0),
                            uv0=np.array([(0, 1), (1, 1), (1, 0), (0, 0)], f64)))
    s.add_mesh(meshgen.box((-0.3, -0.35, 0.4), (0.35, 0.3, 0.6)))
    s.add_light(abi.LIGHT_POINT, position=(0.3, 0.2, 1.5), color=(1.0, 0.9, 0.8), intensity=4.0)
    s.settings = base_settings()
    s.world_to_view = np.eye(4)
    return s


class Ctx:
    """A renderer with the scene uploaded, the probes set and, for their atlas, an output and the two AOV targets."""

    def __init__(self, s, probes=(POS5, N5, C5, MAXD), aov=False, mode=None):
        from gltf_renderer_amd.renderer import Renderer
        self.s, self.aov = s, aov
        self.r = Renderer(0)
        self.handles = s.upload(self.r)
        if mode is not None:
            self.r.set_kernel_mode(mode)
        if probes is not None:
            self.use(*self.r.set_probes(*probes))

    def use(self, W, H):
        self.size = (W, H)
        self.out, self.alb, self.nd = (self.r.create_output(W, H) for _ in range(3))
        if self.aov:
            self.r.set_aov(self.alb, self.nd)

    def params(self, frame=0, **kw):
        self.s.width, self.s.height = self.size
        return self.s.execute_params(frame, **kw)

    def trace(self, st, frame, **kw):
        self.r.trace(st, self.params(frame, **kw), self.out)

    def read(self):
        return tuple(self.r.readback(t) for t in ((self.out, self.alb, self.nd) if self.aov else (self.out,)))

    def close(self):
        self.r.close()


def hook_rays(c, st, queries):
    """pt_debug_probe_rays: queries [n, 3] uint32 {px, py, seed} -> [n, 8] float32 (origin, tmin, direction, tmax)."""
    q = np.ascontiguousarray(queries, np.uint32).reshape(-1, 3)
    out = np.zeros((len(q), 8), f32)
    f = hooks.lib().pt_debug_probe_rays
    params = c.params(0)
    rc = f(c.r.h, C.byref(st), C.byref(params), q.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (rc, c.r.L.pt_last_error(c.r.h))
    return out


def texel_queries(W, H, seeds):
    sd, y, x = np.meshgrid(np.asarray(list(seeds), np.uint32), np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), sd.ravel()], axis=1)


def once(st):
    st = copy_settings(st)
    st.flags &= ~abi.FLAG_ACCUMULATE
    return st


def rf_of(st):
    return ray_hook.RF_CULL_BACK if st.flags & abi.FLAG_CULL_BACKFACE else 0


def present_mask(W, H, n, columns, count):
    y, x = np.mgrid[0:H, 0:W]
    return pr.cell(n, columns, x, y)[0] < count


@pytest.fixture(scope="module")
def lit():
    return lit_scene()


@pytest.fixture(scope="module")
def rnd5(oracle_lib):
    """orc_random(px, py, seed, 0) on the 32 x 48 atlas for seeds 0 .. 2 (bit-identical to the product's by tests/test_gpu_parity.py)."""
    return lr.randoms(oracle_lib, W5, H5, range(3))


@pytest.fixture(scope="module")
def rays5(lit):
    """The hook's rays of every texel of the 32 x 48 atlas at seeds 0 .. 2, and the context they came from."""
    c = Ctx(lit)
    q = texel_queries(W5, H5, range(3))
    rays = hook_rays(c, lit.settings, q)
    yield c, q, rays
    c.close()


# ---- 1. the rays are the definition ----------------------------------------------------------------------------------------------------
def test_hook_rays_equal_the_restatement_bit_for_bit(lit, rays5, rnd5, oracle_lib):
    c, q, rays = rays5
    want, (sx, sy) = pr.rays(oracle_lib, POS5, N5, C5, MAXD, q, rnd5[q[:, 2], q[:, 1], q[:, 0]])
    assert same(rays, want), np.nonzero((bits(rays) != bits(want)).any(axis=1))[0][:8]
    absent = ~present_mask(W5, H5, N5, C5, len(POS5))[q[:, 1], q[:, 0]]
    assert absent.sum() == 3 * N5 * N5
    assert (rays[absent, 0:7] == 0).all() and (rays[absent, 7] == -1).all()
    assert len(np.unique(bits(rays[~absent, 4:7]), axis=0)) > 0.99 * (~absent).sum()      # the jitter moves the direction
    assert np.abs(np.linalg.norm(rays[~absent, 4:7].astype(f64), axis=1) - 1).max() < 1e-6
    # the map's +z is world +z: the texels about a map's centre look up, those at its corners down
    k, lx, ly = pr.cell(N5, C5, q[:, 0], q[:, 1])
    centre = ~absent & (np.abs(lx - 7.5) < 1) & (np.abs(ly - 7.5) < 1)
    corner = ~absent & ((lx == 0) | (lx == 15)) & ((ly == 0) | (ly == 15))
    assert (rays[centre, 6] > 0.9).all() and (rays[corner, 6] < -0.9).all()


def test_hook_rays_on_the_seam_diagonals_and_the_draws_end_points(lit, oracle_lib):
    """One 32 x 32 probe.  The texel centres of a map never lie on the diagonals |s.x| + |s.y| = 1 (the equator, where the octahedron folds) nor on
    the axes; the jitter puts samples on both sides of them.  The restatement is evaluated for crafted draws as well -- r = 0, 0.5 and exactly 1
    (quirk q17), which put the square point exactly on the map's border, on texel corners and on the seam."""
    n = 32
    pos = np.array([(0.1, -0.2, 0.3)], f32)
    c = Ctx(lit, probes=(pos, n, 1, 7.5))
    seeds = range(2)
    q = texel_queries(n, n, seeds)
    rays = hook_rays(c, lit.settings, q)
    rnd = lr.randoms(oracle_lib, n, n, seeds)
    want, (sx, sy) = pr.rays(oracle_lib, pos, n, 1, 7.5, q, rnd[q[:, 2], q[:, 1], q[:, 0]])
    assert same(rays, want)
    assert (bits(rays[:, 7]) == bits(f32(7.5))).all() and (rays[:, 3] == 0).all() and same(rays[:, 0:3], np.broadcast_to(pos, (len(q), 3)))
    side = np.abs(sx.astype(f64)) + np.abs(sy.astype(f64)) - 1
    lx, ly = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)
    on_diagonal = (lx + ly == n // 2 - 1) | (lx + ly == 3 * n // 2 - 1) | (lx - ly == n // 2) | (ly - lx == n // 2)   # texels the seam passes through
    assert (side[on_diagonal] > 0).any() and (side[on_diagonal] < 0).any()
    clear = np.abs(side) > 1e-6                                                          # (the float32 sum may round onto the seam)
    assert (np.sign(rays[:, 6]) == -np.sign(side))[clear].all() and clear.mean() > 0.99  # inside the diamond is the upper hemisphere
    # crafted draws through the restatement's float32 steps: the square point of a texel corner on the seam is exactly on it
    crafted = np.array([(0, 0, 0, 0), (1, 1, 0, 0), (0.5, 0.5, 0, 0), (1, 0, 0, 0)], f32)
    u, v = pr.sample_uv32(n, np.array([n - 1, n - 1, 7, 23]), np.array([n - 1, 0, 7, 15]), crafted)
    assert u.tolist() == [(n - 1) / n, 1.0, 7.5 / n, 0.75] and v.tolist() == [(n - 1) / n, 1 / n, 7.5 / n, 15 / n]
    s = pr.uv_to_square32(u, v)
    assert abs(float(s[0][3])) + abs(float(s[1][3])) < 1 and float(s[0][1]) == 1.0
    d = pr.oracle_sphere(oracle_lib, *pr.uv_to_square32(f32([0.75, 1.0]), f32([0.25, 0.5])))
    assert abs(d[0, 2]) < 1e-7 and np.allclose(d[1], [1, 0, 0], atol=1e-6)              # on the seam: the equator
    c.close()


# ---- 2. pt_trace traces exactly the hook's rays ----------------------------------------------------------------------------------------
def test_trace_traces_exactly_the_hooks_rays(lit, rays5):
    hook, q, rays = rays5
    present = present_mask(W5, H5, N5, C5, len(POS5))
    c = Ctx(lit, aov=True)
    st = once(lit.settings)
    c.r.reset_stats()
    black = np.array([0, 0, 0, 1], f32)
    for f in range(3):
        c.trace(st, f)
        out, alb, nd = c.read()
        sel = q[:, 2] == f
        assert np.array_equal(q[sel, 0].reshape(H5, W5)[0], np.arange(W5))                 # the queries of a seed are in image order
        hit = ray_hook.gpu_intersect(hook.r, rays[sel], rf_of(st)).reshape(H5, W5, 8)
        found = (hit[..., 0] > 0) & present
        assert 0.1 < found[present].mean() < 0.99
        assert same(nd[..., 3][found], hit[..., 1][found]), f
        assert np.array_equal(alb[..., 3], found.astype(f32)), f
        assert (bits(nd[present & ~found]) == 0).all()
        assert same(out[~present], np.broadcast_to(black, out[~present].shape)) and (bits(alb[~present]) == 0).all() and (bits(nd[~present]) == 0).all()
        # the probe inside the occluder box sees only the box, from behind or in front as the culling flag has it, never farther than its walls
        box = pr.cell(N5, C5, *np.meshgrid(np.arange(W5), np.arange(H5)))[0] == 3
        if not rf_of(st):
            assert nd[..., 3][box & found].max() < 0.6
    assert c.r.stats().rays_primary == 3 * len(POS5) * N5 * N5
    c.close()


def test_empty_cells_stay_black_and_the_mean_distance_accumulates(lit):
    present = present_mask(W5, H5, N5, C5, len(POS5))
    c = Ctx(lit, aov=True)
    st = copy_settings(lit.settings); st.reset = 1
    c.r.reset_stats()
    black = np.array([0, 0, 0, 1], f32)
    for f in range(5):
        c.trace(st, f); st.reset = 0
        if f in (0, 4):
            out, alb, nd = c.read()
            assert same(out[~present], np.broadcast_to(black, out[~present].shape)), f
            assert (bits(alb[~present]) == 0).all() and (bits(nd[~present]) == 0).all(), f
    assert c.r.stats().rays_primary == 5 * len(POS5) * N5 * N5
    assert ((alb[..., 3] >= 0) & (alb[..., 3] <= 1)).all() and (alb[..., 3][present] > 0).any() and (alb[..., 3][present] < 1).any()   # the fraction of rays that hit
    assert (out[present][:, :3] > 0).any()
    c.close()


# ---- 3. an escaping ray reads the environment along its direction ------------------------------------------------------------------------
def test_no_geometry_in_reach_gives_the_environments_miss_answer_bit_for_bit():
    """One triangle 10^4 units away and a max_distance of 50: every ray escapes.  1 sample, environment map on: the texel is what the MISS
    query (pt_debug_env_query op 3, held to the oracle's by tests/test_gpu_envmap.py) answers along the hook's direction."""
    s = scenes.SceneData("probe_env")
    s.add_mesh(meshgen.Mesh([(9000, 9000, 9000), (9001, 9000, 9000), (9000, 9001, 9000)], [0, 1, 2], normals=np.repeat([[0.0, 0.0, 1.0]], 3, axis=0)))
    s.settings = base_settings()
    s.world_to_view = np.eye(4)
    c = Ctx(s)
    env = c.r.env_create(scenes.sky_image(64, 32, 30.0))
    st = once(s.settings)
    st.flags |= abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS
    st.flags &= ~abi.FLAG_LUMINANCE_CLAMP
    st.environment_intensity = 1.5
    present = present_mask(W5, H5, N5, C5, len(POS5))
    for f in range(2):
        rays = hook_rays(c, st, texel_queries(W5, H5, [f]))
        c.r.trace(st, c.params(f, env_handle=env), c.out)
        out = c.read()[0]
        qin = np.zeros((len(rays), 8), f32)
        qin[:, 0:3] = rays[:, 4:7]
        qin[:, 4] = st.environment_intensity
        res = np.zeros((len(rays), 16), f32)
        fq = hooks.lib().pt_debug_env_query
        assert fq(c.r.h, env, 0, 3, qin.ctypes.data, len(qin), res.ctypes.data) == 0
        want = np.concatenate([res[:, 0:3], np.ones((len(res), 1), f32)], axis=1).reshape(H5, W5, 4)
        assert same(out[present], want[present]), f
        assert (out[present][:, :3] > 0).all() and len(np.unique(bits(out[present][:, :3]), axis=0)) > 100
        assert same(out[~present], np.broadcast_to(np.array([0, 0, 0, 1], f32), out[~present].shape))
    c.close()


# ---- 4. composition --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uniform(lit):
    """The uninterrupted run, traced frame by frame: snapshots [n - 1] = (output, albedo, normal_depth)."""
    c = Ctx(lit, aov=True)
    st = copy_settings(lit.settings); st.reset = 1
    snaps = []
    for f in range(N):
        c.trace(st, f); st.reset = 0
        snaps.append(c.read())
    c.close()
    assert not same(snaps[0][0], snaps[N - 1][0])
    return snaps


def test_a_batch_of_four_equals_four_calls(lit, uniform):
    c = Ctx(lit, aov=True)
    c.r.set_samples_per_trace(4)
    st = copy_settings(lit.settings); st.reset = 1
    c.trace(st, 0)
    for a, b in zip(c.read(), uniform[3]):
        assert same(a, b)
    c.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_tile_shards_unite_to_the_whole_atlas(lit, uniform, ranks):
    root = Ctx(lit)
    dst = [root.r.create_output(W5, H5) for _ in range(3)]
    for k in range(ranks):
        c = Ctx(lit, aov=True)
        st = copy_settings(lit.settings); st.reset = 1
        for f in range(N):
            c.trace(st, f, tile_rank=k, tile_rank_count=ranks); st.reset = 0
        for img, into in zip((c.out, c.alb, c.nd), dst):
            packed = c.r.tiles_pack(img, k, ranks)
            root.r.tiles_unpack(packed.clone(), into, k, ranks)
        c.r.readback(c.out)                                          # the pack has run before the context goes
        c.close()
    for into, want in zip(dst, uniform[N - 1]):
        assert same(root.r.readback(into), want)
    root.close()


def test_an_adaptive_tile_equals_the_uniform_run_at_its_count(lit, uniform):
    """A tile is one probe's: the empty cell's tile retires at min_samples with an error of 0, and every tile holds what the uniform run
    held when it had the tile's count."""
    c = Ctx(lit)
    c.r.set_adaptive(2, N, 1e-3)
    st = copy_settings(lit.settings)
    for f in range(N):
        c.trace(st, f)
    _, samples, error, _ = c.r.adaptive_read(W5, H5)
    out = c.read()[0]
    assert samples.shape == (H5 // 16, W5 // 16) and samples[2, 1] == 2 and error[2, 1] == 0
    assert samples.max() > 2 and (samples >= 2).all()
    for ty in range(H5 // 16):
        for tx in range(W5 // 16):
            sl = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
            assert same(out[sl], uniform[int(samples[ty, tx]) - 1][0][sl]), (ty, tx, samples)
    c.close()


def test_save_destroy_create_set_probes_load_continue_equals_the_uninterrupted_run(lit, uniform):
    a = Ctx(lit, aov=True)
    st = copy_settings(lit.settings); st.reset = 1
    for f in range(3):
        a.trace(st, f); st.reset = 0
    blob = a.r.accum_save(W5, H5, a.out, a.alb, a.nd, next_frame=3)
    a.close()
    b = Ctx(lit, aov=True)                                           # probes are a setting, not part of the blob: set before the load
    info = b.r.accum_load(blob, b.out, b.alb, b.nd)
    assert info.accumulated_frames == 3 and info.next_frame == 3
    for f in range(3, N):
        b.trace(st, f)
        for x, y in zip(b.read(), uniform[f]):
            assert same(x, y), f
    assert b.r.stats().accumulated_frames == N
    b.close()


# ---- 5. probes off, and the refusals ---------------------------------------------------------------------------------------------------
def test_probes_off_after_probes_on_is_the_camera_image_of_a_context_that_never_had_probes(lit):
    cam = lit_scene()
    cam.world_to_view = camera.orbit_world_to_view((0, 0, 0.3), 3.0, 0.4, -0.5)

    def camera_frames(c):
        st = copy_settings(cam.settings); st.reset = 1
        c.r.reset_stats()
        for f in range(4):
            c.trace(st, f); st.reset = 0
        t = c.r.stats()
        return c.read(), (t.rays, t.rays_primary, t.rays_bounce, t.rays_shadow, t.closest_hits)

    never = Ctx(cam, probes=None, aov=True)
    never.use(W5, H5)
    want, rays = camera_frames(never)
    never.close()
    c = Ctx(cam, aov=True)
    probed, _ = camera_frames(c)
    assert not same(probed[0], want[0])
    assert c.r.set_probes(None, 0, enable=False) is None
    got, rays_got = camera_frames(c)
    for a, b in zip(got, want):
        assert same(a, b)
    assert rays_got == rays
    c.close()


def test_set_probes_refusals_and_the_restart(lit):
    c = Ctx(lit, aov=True)
    L, h = c.r.L, c.r.h
    st = copy_settings(lit.settings); st.reset = 1
    for f in range(3):
        c.trace(st, f); st.reset = 0
    assert c.r.stats().accumulated_frames == 3
    good = np.ascontiguousarray(POS5)

    def set_rc(cfg, pos=good):
        rc = L.pt_set_probes(h, C.byref(abi.PtProbeConfig(*cfg)), None if pos is None else pos.ctypes.data_as(C.c_void_p))
        return rc, L.pt_last_error(h).decode()

    nan, inf = float("nan"), float("inf")
    bad = [((1, 0, 5, 2, MAXD), "resolution"), ((1, 24, 5, 2, MAXD), "resolution"), ((1, 1040, 5, 2, MAXD), "resolution"), ((1, -16, 5, 2, MAXD), "resolution"),
           ((1, 16, 0, 2, MAXD), "count"), ((1, 16, -3, 2, MAXD), "count"), ((1, 16, 5, 0, MAXD), "columns"), ((1, 16, 5, 2, 0.0), "max_distance"),
           ((1, 16, 5, 2, -1.0), "max_distance"), ((1, 16, 5, 2, nan), "max_distance"), ((1, 16, 5, 2, inf), "max_distance"),
           ((1, 1024, 5, 1 << 21, MAXD), "columns"), ((1, 1024, (1 << 21), 1, MAXD), "rows")]
    for cfg, field in bad:
        rc, msg = set_rc(cfg)
        assert rc == -1 and field in msg, (cfg, rc, msg)
    assert L.pt_set_probes(h, None, good.ctypes.data_as(C.c_void_p)) == -1 and "config" in L.pt_last_error(h).decode()
    rc, msg = set_rc((1, 16, 5, 2, MAXD), None)
    assert rc == -1 and "positions" in msg
    for value in (nan, inf, -inf):
        p = good.copy(); p[3, 1] = value
        rc, msg = set_rc((1, 16, 5, 2, MAXD), p)
        assert rc == -1 and "probe 3" in msg, msg
    # the old config and positions stay and no restart is pending
    blob = c.r.accum_save(W5, H5, c.out, c.alb, c.nd, next_frame=3)
    c.trace(st, 3)
    assert c.r.stats().accumulated_frames == 4
    ref = c.read()
    # a good config: nothing to save until the next trace, which starts anew with the new positions
    moved = good + f32(0.05)
    assert set_rc((1, 16, 5, 2, MAXD), moved)[0] == 0
    need = C.c_size_t()
    img = abi.PtAccumImages(c.out.data_ptr(), c.alb.data_ptr(), c.nd.data_ptr())
    assert L.pt_accum_save(h, C.byref(img), W5, H5, 0, 1, 0, None, 0, C.byref(need)) == -6
    c.trace(st, 4)
    assert c.r.stats().accumulated_frames == 1
    assert same(hook_rays(c, st, [(0, 0, 0)])[0, 0:3], moved[0])
    # pt_accum_load clears the pending restart
    assert set_rc((1, 16, 5, 2, MAXD), good)[0] == 0
    c.r.accum_load(blob, c.out, c.alb, c.nd)
    c.trace(st, 3)
    assert c.r.stats().accumulated_frames == 4
    assert all(same(a, b) for a, b in zip(c.read(), ref))
    # a config that is not enabled is not checked
    assert set_rc((0, 7, -1, 0, nan), None)[0] == 0
    # the atlas size is the trace's to check, with nothing written
    assert set_rc((1, 16, 5, 2, MAXD), good)[0] == 0
    wrong = c.r.create_output(W5, H5 + 16)
    wrong.fill_(7.0)
    lit.width, lit.height = W5, H5 + 16
    with pytest.raises(MiptError, match="atlas"):
        c.r.trace(st, lit.execute_params(0), wrong)
    assert (c.r.readback(wrong) == 7.0).all()
    # probes and a bake exclude each other, whichever comes second
    with pytest.raises(MiptError, match="probes"):
        c.r.set_bake(0.01)
    c.r.set_probes(None, 0, enable=False)
    c.r.set_bake(0.01)
    rc, msg = set_rc((1, 16, 5, 2, MAXD), good)
    assert rc == -1 and "bake" in msg
    c.r.set_bake(0.01, enable=False)
    assert set_rc((1, 16, 5, 2, MAXD), good)[0] == 0
    c.close()
    # the megakernel refuses probes and writes nothing
    m = Ctx(lit, mode=abi.MODE_MEGAKERNEL)
    m.out.fill_(7.0)
    with pytest.raises(MiptError, match="wavefront"):
        m.trace(st, 0)
    assert (m.read()[0] == 7.0).all()
    m.close()


# ---- 6. the projection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count,columns", [(16, 5, 2), (32, 1, 1), (48, 3, 3)])
def test_projection_is_within_the_derived_bound_of_the_float64_restatement(lit, oracle_lib, n, count, columns):
    """A random atlas over six decades with NaN and Inf texels, garbage in the empty cell and in the w channel."""
    rng = np.random.default_rng(11 + n)
    W, H = pr.atlas_size(n, count, columns)
    pos = rng.uniform(-0.5, 0.5, (count, 3)).astype(f32)
    c = Ctx(lit, probes=(pos, n, columns, MAXD))
    assert c.size == (W, H)
    atlas = (rng.standard_normal((H, W, 4)) * 10.0 ** rng.uniform(-3, 3, (H, W, 1))).astype(f32)
    for value in (np.nan, np.inf, -np.inf):
        ys, xs, ch = rng.integers(0, H, 6), rng.integers(0, W, 6), rng.integers(0, 3, 6)
        atlas[ys, xs, ch] = value
    atlas[..., 3] = np.nan
    atlas[~present_mask(W, H, n, columns, count)] = np.nan
    t = c.r.torch.from_numpy(atlas).to("cuda:0")
    dirs = pr.centre_dirs_oracle(oracle_lib, n).astype(f64)
    want, mag = pr.project_atlas(atlas, dirs, n, count, columns, 0)
    got = c.r.probe_project(t, abi.PROBE_SH_RADIANCE)
    assert got.shape == (count, 9, 3) and np.isfinite(got).all()
    bound = pr.projection_bound(n, mag)[:, None, :]
    err = np.abs(got.astype(f64) - want)
    print("n = %d: largest error / bound %.3f" % (n, (err / bound).max()))
    assert (err <= bound).all(), (err / bound).max()
    assert (np.abs(want) > 10 * bound).mean() > 0.5                                      # the bound is far below the values it guards
    # the irradiance kind: the radiance coefficient times the float32 band factor, one rounding -- the float32 product, bit for bit
    irr = c.r.probe_project(t, abi.PROBE_SH_IRRADIANCE)
    band32 = pr.BAND_FACTOR[pr.SH_BAND].astype(f32)[None, :, None]
    assert same(irr, (got * band32).astype(f32))
    # the refusals
    L, h = c.r.L, c.r.h
    sh = np.full((count, 9, 3), 5.0, f32)
    p = sh.ctypes.data_as(C.c_void_p)
    assert L.pt_probe_project(h, C.c_void_p(t.data_ptr()), W + 16, H, 0, p) == -1
    assert L.pt_probe_project(h, C.c_void_p(t.data_ptr()), W, H, 2, p) == -1
    assert L.pt_probe_project(h, None, W, H, 0, p) == -1 and L.pt_probe_project(h, C.c_void_p(t.data_ptr()), W, H, 0, None) == -1
    c.r.set_probes(None, 0, enable=False)
    assert L.pt_probe_project(h, C.c_void_p(t.data_ptr()), W, H, 0, p) == -6
    assert (sh == 5.0).all()
    c.close()


# ---- 7. end to end against the oracle ----------------------------------------------------------------------------------------------------
def test_probe_sh_equals_the_sh_of_the_oracles_cube_faces(lit, oracle_lib):
    """One 32 x 32 probe in the lit scene, full paths (bounces, the point light, the constant environment), 16 samples a replicate, against the
    SH of six 32 x 32 cube faces the oracle renders from the same point with 16 samples each.  Both sides are Monte-Carlo estimates: R = 4
    replicates with fixed, disjoint seeds on each side give the per-coefficient standard errors, and the means must agree within
    4 * sqrt(se_gpu^2 + se_oracle^2) + q, q = the largest difference between the two quadratures' coefficients of the analytic clamped-cosine
    field about +z (the direction the light comes from), scaled by the probe's mean radiance per channel.
    Measured on an MI355X: se_gpu 3e-4 .. 2.7e-3 and se_oracle 1e-4 .. 1.2e-3 over the 27 values (red smallest, blue largest); the two
    quadratures differ by 3.93e-3 on the lobe, times the mean radiance (0.220, 0.405, 0.590) = q (8.6e-4, 1.6e-3, 2.3e-3), about as much as
    the 4-sigma term; |difference| 3.3e-5 .. 3.0e-3, at most 0.58 of the tolerance (the (2,0) coefficient, red)."""
    n = m = 32
    R, S = 4, 16
    pos = np.array([(0.5, -0.45, 0.3)], f32)
    c = Ctx(lit, probes=(pos, n, 1, 1000.0))
    c.r.set_samples_per_trace(8)
    gpu = []
    for rep in range(R):
        st = copy_settings(lit.settings); st.reset = 1
        for f in range(0, S, 8):
            c.trace(st, rep * S + f); st.reset = 0
        assert c.r.stats().accumulated_frames == S
        gpu.append(c.r.probe_project(c.out).astype(f64)[0])
    c.close()
    o = oracle_lib.Oracle()
    cube = lit_scene()
    cube.upload(o)
    cube.width = cube.height = m
    cube.y_fov, cube.z_near, cube.z_far = math.pi / 2, 0.01, 100.0
    orc = []
    for rep in range(R):
        faces = []
        for face in range(6):
            cube.world_to_view = pr.cube_world_to_view(pos[0], face)
            img = np.zeros((m, m, 4), f32)
            st = copy_settings(lit.settings); st.reset = 1
            for f in range(S):
                o.trace(st, cube.execute_params(1000 + rep * S + f), img); st.reset = 0
            faces.append(img)
        orc.append(pr.cube_sh(faces))
    o.close()
    gpu, orc = np.array(gpu), np.array(orc)
    mean_g, mean_o = gpu.mean(axis=0), orc.mean(axis=0)
    se_g, se_o = gpu.std(axis=0, ddof=1) / math.sqrt(R), orc.std(axis=0, ddof=1) / math.sqrt(R)
    up = np.array([0.0, 0.0, 1.0])
    d = pr.centre_dirs64(n)
    oct_lobe = pr.project_map(np.maximum(d @ up, 0.0)[..., None].repeat(3, -1), d)[:, 0]
    cube_lobe = pr.cube_sh([np.maximum(pr.cube_pixel_dirs(f, m)[0] @ up, 0.0)[..., None].repeat(3, -1) for f in range(6)])[:, 0]
    mean_radiance = mean_g[0] / (2 * math.sqrt(math.pi))
    q = np.abs(oct_lobe - cube_lobe).max() * mean_radiance
    tol = 4 * np.sqrt(se_g ** 2 + se_o ** 2) + q[None, :]
    diff = np.abs(mean_g - mean_o)
    np.set_printoptions(precision=4, linewidth=200)
    print("mean radiance per channel", mean_radiance, "q", q, "quadrature difference", np.abs(oct_lobe - cube_lobe).max())
    print("se gpu\n", se_g, "\nse oracle\n", se_o, "\n|difference|\n", diff, "\ndifference / tolerance\n", diff / tol)
    assert mean_radiance.min() > 0.1 and np.abs(mean_g[1:]).max() > 10 * tol.max()      # a scene with a direction to it: the comparison can fail
    assert (diff <= tol).all(), (diff / tol).max()
