"""Motion vectors and temporal reprojection (include/mipt.h pt_set_motion, pt_motion_snapshot, pt_reproject) on the MI355X.

The scene is the matte test's "confetti" (96 one-quad instances) at 40 x 24 and, for the records and the traced target, also at 17 x 33; the
filter runs on synthetic images of both sizes.  The camera
rays come out of pt_debug_camera_rays, the records out of pt_debug_motion (k_debug_intersect's closest hit, then k_wf_motion's own record
function); tests/motion_ref.py restates the record in float64 from the scene's object-space vertices and transforms, with the bound it derives,
and the filter in float32, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera
from tests import hooks
from tests import adaptive_ref as ar
from tests import aov_ref as av
from tests import motion_ref as mo
from tests.test_gpu_matte import confetti, copy_settings, single

pytestmark = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
W, H = 40, 24                      # 3 x 2 tiles, ragged in both directions
N = 8
POISON = 7.0
MOVED = 4 * 12 + 5                 # an instance in the middle of the picture
SHIFT = camera.translate((0.75, -0.5, 0.25))          # exact in float32, like the identity the quads start with
REWRITTEN = 3 * 12 + 6             # the instance whose vertices are rewritten


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def pan(s):
    """The previous frame's camera: the scene's orbit a little to the side, and its matrices as the config takes them."""
    V = camera.orbit_world_to_view((0.2, 0.0, -0.1), 4.5, 0.06, 0.03)
    P = camera.view_to_clip(s.width / s.height, s.y_fov, s.z_near, s.z_far)
    return camera.cm(V), camera.cm(P)


def same_camera(s):
    p = s.execute_params(0)
    return np.array(p.world_to_view[:], f32), np.array(p.view_to_clip[:], f32)


def camera_rays(r, st, params, queries):
    q = np.ascontiguousarray(queries, u32).reshape(-1, 3)
    out = np.zeros((len(q), 8), f32)
    f = hooks.lib().pt_debug_camera_rays
    rc = f(r.h, C.byref(st), C.byref(params), q.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (rc, r.L.pt_last_error(r.h).decode())
    return out


def hook(r, st, params, rays):
    """pt_debug_motion: rays [n, 8] -> [n, 8] float32 (record.xyzw, instance, primitive, u, v)."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    out = np.zeros((len(rays), 8), f32)
    f = hooks.lib().pt_debug_motion
    rc = f(r.h, C.byref(st), C.byref(params), rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (rc, r.L.pt_last_error(r.h).decode())
    return out


def frame_queries(w, h, frame):
    y, x = np.meshgrid(np.arange(h, dtype=u32), np.arange(w, dtype=u32), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(w * h, frame, u32)], axis=1)


class Pose:
    """Where every instance's triangles are: per instance the object-space positions, the indices and the transform (float32 values)."""

    def __init__(self, s):
        self.pos = [m.positions.copy() for m, _, _ in s.mesh_records]
        self.idx = [np.asarray(m.indices, np.int64).reshape(-1, 3) for m, _, _ in s.mesh_records]
        self.T = [np.asarray(T, f32) for _, T, _ in s.mesh_records]

    def moved(self, k, T):
        p = Pose.__new__(Pose)
        p.pos, p.idx, p.T = list(self.pos), self.idx, list(self.T)
        p.T[k] = np.asarray(T, f32)
        assert np.array_equal(p.T[k].astype(f64), np.asarray(T, f64))
        return p

    def rewritten(self, k, positions):
        p = Pose.__new__(Pose)
        p.pos, p.idx, p.T = list(self.pos), self.idx, list(self.T)
        p.pos[k] = np.ascontiguousarray(positions, f32)
        return p

    def points(self, inst, prim, u, v):
        """float64 world points and packet scales of the hits (inst, prim, u, v), by tests/motion_ref.world_points per instance."""
        P, S = np.zeros((len(inst), 3), f64), np.zeros((len(inst), 3), f64)
        for k in np.unique(inst):
            m = inst == k
            P[m], S[m] = mo.world_points(self.pos[k], self.T[k], self.idx[k][prim[m]], u[m], v[m])
        return P, S


class Ctx:
    def __init__(self, s, prev=None, poison=None, aov=False):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        self.handles = s.upload(self.r)
        self.out = self.r.create_output(s.width, s.height)
        self.mv = self.r.create_output(s.width, s.height)
        self.alb = self.nd = None
        if aov:
            self.alb, self.nd = self.r.create_output(s.width, s.height), self.r.create_output(s.width, s.height)
            self.r.set_aov(self.alb, self.nd)
        if poison is not None:
            self.mv.fill_(poison)
        if prev is not None:
            self.r.set_motion(self.mv, *prev)

    def trace(self, st, frame, **kw):
        self.r.trace(st, self.s.execute_params(frame, **kw), self.out)

    def target(self):
        return self.r.readback(self.mv)

    def records(self, st, frame):
        """The hook's answer for every pixel's camera ray of `frame` (use_frame_as_seed: the seed is the frame): (H, W, 8)."""
        p = self.s.execute_params(frame)
        rays = camera_rays(self.r, st, p, frame_queries(self.s.width, self.s.height, frame))
        return hook(self.r, st, p, rays).reshape(self.s.height, self.s.width, 8)

    def move(self, k, T):
        insts = self.handles["instances"]
        insts[k].gpu.transform[:] = camera.cm(T)
        insts[k].gpu.normal_transform[:] = camera.cm(camera.inverse_transpose(T))
        self.r.set_instances(insts)

    def rewrite(self, k, positions):
        self.r.buffer_update(self.handles["buffers"][self.s.instances[k].gpu.position_descriptor], np.ascontiguousarray(positions, f32))

    def close(self):
        self.r.close()


def check_against_definition(s, rec, cur, prev, prev_cam):
    """Hook records (.., 8) against the float64 restatement from the poses, within tests/motion_ref.record_bound.  Returns the largest
    error / bound."""
    rec = rec.reshape(-1, 8)
    hit = rec[:, 4] >= 0
    assert hit.sum() >= len(rec) // 4 and (~hit).sum() >= 20
    assert np.all(bits(rec[~hit, :4]) == 0) and np.all(rec[~hit, 5] == -1)
    inst, prim = rec[hit, 4].astype(np.int64), rec[hit, 5].astype(np.int64)
    u, v = rec[hit, 6], rec[hit, 7]
    assert np.all(u >= 0) and np.all(v >= 0) and np.all(u.astype(f64) + v.astype(f64) <= 1 + 2.0 ** -22)
    Vc, Pc = same_camera(s)
    Vp, Pp = prev_cam
    Mc, Mp = mo.world_to_clip(Pc, Vc), mo.world_to_clip(Pp, Vp)
    P1, S1 = cur.points(inst, prim, u, v)
    P0, S0 = prev.points(inst, prim, u, v)
    # every tested point in front of both cameras by a clear margin: clip_3 (the view depth here) stays well away from 0
    assert mo.clip_w(Mc, P1).min() > 2.0 and mo.clip_w(Mp, P0).min() > 2.0
    want = mo.record_points(P1, P0, Mc, Mp, Vc, Vp, s.width, s.height)
    bound = mo.record_bound(P1, S1, P0, S0, Mc, Mp, Vc, Vp, s.width, s.height, want)
    assert bound[:, :2].max() < 2e-3 and bound[:, 2:].max() < 2e-5                   # the bound itself says something: well under a pixel
    err = np.abs(rec[hit, :4].astype(f64) - want)
    ratio = (err / bound).max()
    print("hits %d, largest error / bound %.3f, largest |xy| %.2f px" % (hit.sum(), ratio, np.abs(want[:, :2]).max()))
    assert np.all(err <= bound), ratio
    return ratio, want, hit


@pytest.fixture(scope="module")
def scene():
    s = confetti()
    assert s.settings.use_frame_as_seed and (s.width, s.height) == (W, H)
    return s


@pytest.fixture(scope="module")
def tall():
    """The same quads through a 17 x 33 frame: 2 x 3 tiles, ragged in both directions the other way round."""
    s = confetti()
    s.width, s.height = 17, 33
    return s


@pytest.fixture(params=["40x24", "17x33"])
def framed(request, scene, tall):
    return scene if request.param == "40x24" else tall


def accumulate(c, st, frames=N):
    sa = copy_settings(st); sa.reset = 1
    for f in range(frames):
        c.trace(sa, f); sa.reset = 0


def test_static_scene_and_unchanged_camera_give_exact_zeros_and_equal_depths(scene):
    st = scene.settings
    for snapshot in (False, True):
        c = Ctx(scene, prev=same_camera(scene), poison=POISON)
        assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_NONE
        if snapshot:
            c.r.motion_snapshot()
            assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_VALID
        accumulate(c, st)
        t = c.target()
        hit_any = np.stack([c.records(single(st), f)[..., 4] >= 0 for f in range(N)]).any(axis=0)
        assert hit_any.sum() >= 300 and (~hit_any).sum() >= 50
        assert np.all(t[..., 0] == 0) and np.all(t[..., 1] == 0) and np.array_equal(bits(t[..., 2]), bits(t[..., 3]))
        assert np.all(bits(t[~hit_any]) == 0) and np.all(t[hit_any][:, 2] > 0)
        c.close()


def test_records_follow_the_definition_under_a_camera_pan(framed):
    scene = framed
    c = Ctx(scene, prev=pan(scene))
    st = single(scene.settings)
    pose = Pose(scene)
    for f in (0, 5):
        ratio, want, _ = check_against_definition(scene, c.records(st, f), pose, pose, pan(scene))
        assert np.abs(want[:, :2]).max() > 1.0                         # the pan moves things by whole pixels
    c.close()


def test_trace_writes_exactly_the_hooks_records_and_their_running_mean(framed):
    scene = framed
    st = scene.settings
    c = Ctx(scene, prev=pan(scene), poison=POISON)
    c.r.motion_snapshot()
    c.move(MOVED, SHIFT)
    rec = [c.records(single(st), f) for f in range(N)]
    assert any((r[..., 4] == MOVED).sum() >= 4 for r in rec)
    c.trace(single(st), 3)                                              # one sample, no accumulation
    assert np.array_equal(bits(c.target()), bits(rec[3][..., :4]))
    want = av.fold([av.sanitize(r[..., :4]) for r in rec])
    sa = copy_settings(st); sa.reset = 1
    for f in range(N):
        c.trace(sa, f); sa.reset = 0
        assert np.array_equal(bits(c.target()), bits(want[f])), f
    assert c.r.stats().accumulated_frames == N
    c.close()


def test_moved_instances_and_rewritten_vertices_follow_the_definition_and_the_snapshot_outlives_rebuilds(scene):
    st = single(scene.settings)
    c = Ctx(scene, prev=pan(scene))
    pose0 = Pose(scene)
    rng = np.random.default_rng(3)
    new_pos = (pose0.pos[REWRITTEN] + rng.uniform(-0.2, 0.2, pose0.pos[REWRITTEN].shape)).astype(f32)
    pose1 = pose0.moved(MOVED, SHIFT).rewritten(REWRITTEN, new_pos)
    c.r.motion_snapshot()
    c.move(MOVED, SHIFT)                                                # a refit ...
    c.rewrite(REWRITTEN, new_pos)                                       # ... of two instances
    rec = c.records(st, 1)
    assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_VALID
    _, want, hit = check_against_definition(scene, rec, pose1, pose0, pan(scene))
    inst = rec.reshape(-1, 8)[hit, 4]
    for k in (MOVED, REWRITTEN):
        assert (inst == k).sum() >= 4, k
    # the static rows of a run without a snapshot differ from these only at the two instances
    c0 = Ctx(scene, prev=pan(scene))
    c0.move(MOVED, SHIFT); c0.rewrite(REWRITTEN, new_pos)
    rec0 = c0.records(st, 1)
    c0.close()
    differs = (bits(rec[..., :4]) != bits(rec0[..., :4])).any(axis=-1)
    assert differs.any() and np.all(np.isin(rec[..., 4][differs], (MOVED, REWRITTEN)))
    # a rebuild and another builder reorder the packets, not the addresses
    c.r.request_rebuild()
    again = c.records(st, 1)
    assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_VALID and np.array_equal(bits(again), bits(rec))
    c.r.set_accel_builder(abi.BUILDER_LBVH)
    again = c.records(st, 1)
    assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_VALID and np.array_equal(bits(again), bits(rec))
    # another triangle set: the snapshot is stale and the previous geometry is the current geometry
    c.r.set_instances(c.handles["instances"][:-1])
    assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_STALE
    stale = c.records(st, 1)
    c.r.motion_snapshot(False)
    assert c.r.motion_snapshot_state() == abi.MOTION_SNAPSHOT_NONE
    assert np.array_equal(bits(c.records(st, 1)), bits(stale))
    last = len(scene.instances) - 1
    keep = rec0[..., 4] != last
    assert np.array_equal(bits(stale[keep]), bits(rec0[keep]))          # ... which is what a context without a snapshot says
    c.close()


def test_batches_shards_adaptive_tiles_and_debug_outputs_compose_as_the_aovs_do(scene):
    st = scene.settings
    a = Ctx(scene, prev=pan(scene))
    rec = [a.records(single(st), f)[..., :4] for f in range(N)]
    want = av.fold([av.sanitize(r) for r in rec])
    outs = []
    sa = copy_settings(st); sa.reset = 1
    for f in range(N):
        a.trace(sa, f); sa.reset = 0
        outs.append(a.r.readback(a.out))
    a.close()
    # a batch of 4 equals four calls
    c = Ctx(scene, prev=pan(scene), poison=POISON)
    c.r.set_samples_per_trace(4)
    sa = copy_settings(st); sa.reset = 1
    for f in (0, 4):
        c.trace(sa, f); sa.reset = 0
        assert np.array_equal(bits(c.target()), bits(want[f + 3])) and np.array_equal(bits(c.r.readback(c.out)), bits(outs[f + 3])), f
    # a debug-output call leaves the target untouched
    c.mv.fill_(POISON)
    sd = copy_settings(st); sd.debug_output = abi.DEBUG_OUTPUT_COLOR; sd.reset = 1
    c.trace(sd, 0)
    assert np.all(c.target() == POISON)
    c.close()
    # two tile shards: each writes its own tiles and leaves the poison in the other's
    ty, tx = (H + 15) // 16, (W + 15) // 16
    for k in range(2):
        c = Ctx(scene, prev=pan(scene), poison=POISON)
        sa = copy_settings(st); sa.reset = 1
        for f in range(4):
            c.trace(sa, f, tile_rank=k, tile_rank_count=2); sa.reset = 0
        img = c.target()
        for g in range(ty * tx):
            y, x = divmod(g, tx)
            if g % 2 == k:
                assert np.array_equal(bits(ar.tile_view(img, y, x)), bits(ar.tile_view(want[3], y, x))), (k, g)
            else:
                assert np.all(ar.tile_view(img, y, x) == POISON), (k, g)
        c.close()
    # adaptive sampling: a tile holds the uniform target after its own count, so a retired tile was not written again
    raw = []
    c = Ctx(scene, prev=pan(scene), poison=POISON)
    for f in range(N):
        c.trace(single(st), f)
        raw.append(c.r.readback(c.out))
    I, A = ar.fold(raw)
    E4 = ar.tile_errors(I[3], A[3])
    pos = np.sort(E4[E4 > 0].ravel())
    c.r.set_samples_per_trace(2)
    c.r.set_adaptive(2, N, float(pos[len(pos) // 2]))
    frame, active = 0, 1
    while active and frame < N:
        c.trace(st, frame)
        frame += 2
        active, samples, _, _ = c.r.adaptive_read(W, H)
    assert len(set(samples.ravel().tolist())) >= 2, samples
    got = c.target()
    for y, x in np.ndindex(samples.shape):
        n = int(samples[y, x])
        assert np.array_equal(bits(ar.tile_view(got, y, x)), bits(ar.tile_view(want[n - 1], y, x))), (y, x, n)
    c.close()


def test_motion_changes_nothing_else(scene):
    from tests import matte_ref as mr
    st = scene.settings
    runs = {}
    for on in (True, False):
        c = Ctx(scene, prev=pan(scene) if on else None, poison=POISON, aov=True)
        layer = c.r.create_output(W, H)
        c.r.set_matte(mr.INSTANCE, [layer])
        if on:
            c.r.motion_snapshot()
        c.move(MOVED, SHIFT)
        c.r.reset_stats()
        accumulate(c, st)
        runs[on] = ([c.r.readback(t) for t in (c.out, c.alb, c.nd, layer)], c.r.stats(), c.target())
        c.close()
    for a, b in zip(runs[True][0], runs[False][0]):
        assert np.array_equal(bits(a), bits(b))
    for name in ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames"):
        assert getattr(runs[True][1], name) == getattr(runs[False][1], name), name
    assert runs[True][1].accumulated_frames == N and runs[True][1].rays_primary > 0
    assert np.all(runs[False][2] == POISON) and not np.any(runs[True][2] == POISON)


def test_refusals_leave_everything_as_it_was(scene):
    from gltf_renderer_amd.renderer import MiptError
    st = scene.settings
    c = Ctx(scene, prev=pan(scene), poison=POISON)
    r, L = c.r, c.r.L
    sa = copy_settings(st); sa.reset = 1
    c.trace(sa, 0); sa.reset = 0
    good = c.target()

    def cfg(enable=1, target=True, bad=None):
        q = abi.PtMotionConfig()
        q.enable = enable
        q.motion = c.mv.data_ptr() if target else None
        V, P = pan(scene)
        q.prev_world_to_view[:] = [float(x) for x in V]
        q.prev_view_to_clip[:] = [float(x) for x in P]
        if bad == "view":
            q.prev_world_to_view[5] = float("nan")
        if bad == "clip":
            q.prev_view_to_clip[14] = float("inf")
        return q

    for q, word in ((cfg(target=False), "target"), (cfg(bad="view"), "non-finite"), (cfg(bad="clip"), "non-finite")):
        assert L.pt_set_motion(r.h, C.byref(q)) == -1 and word in L.pt_last_error(r.h).decode(), word
    assert L.pt_set_motion(r.h, None) == -1 and "config" in L.pt_last_error(r.h).decode()
    # the old config stays and no restart is pending: the accumulation can be saved and goes on
    r.accum_save(W, H, c.out)
    c.trace(sa, 1)
    assert r.stats().accumulated_frames == 2 and not np.array_equal(bits(c.target()), bits(good))
    # a good config: a restart is pending until the next trace, and pt_accum_save answers PT_ERR_NOT_READY
    assert L.pt_set_motion(r.h, C.byref(cfg())) == 0
    with pytest.raises(MiptError, match="^-6"):
        r.accum_save(W, H, c.out)
    c.trace(sa, 2)
    assert r.stats().accumulated_frames == 1
    # ... unless pt_accum_load comes first: it clears the pending restart (the target is the caller's and stays)
    blob = r.accum_save(W, H, c.out, next_frame=3)
    assert L.pt_set_motion(r.h, C.byref(cfg())) == 0
    assert r.accum_load(blob, c.out).accumulated_frames == 1
    c.trace(sa, 3)
    assert r.stats().accumulated_frames == 2
    # a disabled config is not looked at any further
    assert L.pt_set_motion(r.h, C.byref(cfg(enable=0, target=False, bad="view"))) == 0
    assert L.pt_set_motion(r.h, C.byref(cfg())) == 0
    p = scene.execute_params(0)
    p.output = c.out.data_ptr()

    def refused(word):
        c.out.fill_(POISON); c.mv.fill_(POISON)
        for sx in (sa, single(st)):
            assert L.pt_trace(r.h, C.byref(sx), C.byref(p)) == -1 and word in L.pt_last_error(r.h).decode(), L.pt_last_error(r.h).decode()
        assert np.all(r.readback(c.out) == POISON) and np.all(c.target() == POISON)

    r.set_kernel_mode(abi.MODE_MEGAKERNEL)
    refused("wavefront")
    r.set_kernel_mode(abi.MODE_WAVEFRONT)
    r.set_bake(1.0 / 64)
    refused("motion")
    r.set_bake(1.0 / 64, enable=False)
    aw, ah = r.set_probes([(0.0, -2.0, 0.0), (1.0, -2.0, 0.0)], 16, columns=2)
    atlas, mv = r.create_output(aw, ah), r.create_output(aw, ah)
    atlas.fill_(POISON); mv.fill_(POISON)
    r.set_motion(mv, *pan(scene))
    pp = scene.execute_params(0)
    pp.width, pp.height, pp.output = aw, ah, atlas.data_ptr()
    assert L.pt_trace(r.h, C.byref(sa), C.byref(pp)) == -1 and "motion" in L.pt_last_error(r.h).decode()
    assert np.all(r.readback(atlas) == POISON) and np.all(r.readback(mv) == POISON)
    r.set_probes(None, 16, enable=False)
    # with all of that off again the trace runs
    r.set_motion(c.mv, *pan(scene))
    c.trace(sa, 0)
    assert not np.any(c.target() == POISON)
    c.close()


# ---- pt_reproject ----------------------------------------------------------------------------------------------------------------------
def synthetic(rng, w, h):
    """Random images that hold every case of the definition: integer and fractional vectors, vectors that leave the image, NaN and infinity
    in every input, zero-coverage pixels, depth mismatches on some of the four taps, odd history lengths."""
    color = rng.random((h, w, 4)).astype(f32)
    prev_color = rng.random((h, w, 4)).astype(f32)
    depth = (4.0 + rng.random((h, w))).astype(f32)
    prev_motion = np.zeros((h, w, 4), f32)
    prev_motion[..., :2] = rng.uniform(-2, 2, (h, w, 2))
    prev_motion[..., 2] = depth
    motion = np.zeros((h, w, 4), f32)
    kind = rng.integers(0, 4, (h, w))
    vec = rng.uniform(-3, 3, (h, w, 2)).astype(f32)
    vec[kind == 0] = np.rint(vec[kind == 0])                            # integer vectors
    vec[kind == 1] = 0
    vec[kind == 3] *= f32(8)                                            # many of these leave the image
    motion[..., :2] = vec
    motion[..., 3] = depth
    # the depth the previous frame had where this pixel reads it, so that most taps agree; then break some of them
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    motion[..., 2] = (4.5 + 0.001 * (xs + ys)).astype(f32)
    prev_motion[..., 3] = (4.5 + 0.001 * (xs + ys) + rng.uniform(-0.05, 0.05, (h, w))).astype(f32)
    prev_motion[..., 3][rng.random((h, w)) < 0.15] *= f32(1.2)          # a mismatch on some of the four taps
    prev_motion[..., 3][rng.random((h, w)) < 0.05] = 0                  # zero coverage in the previous frame
    motion[..., 2:][rng.random((h, w)) < 0.05] = 0                      # ... and in this one
    prev_length = rng.choice(np.array([1.0, 1.5, 7.0, 31.5, 40.0, 0.5], f32), (h, w)).astype(f32)
    specials = np.array([np.nan, np.inf, -np.inf], f32)
    for img in (color, motion, prev_color, prev_motion):
        for _ in range(max(4, w * h // 40)):
            img[rng.integers(h), rng.integers(w), rng.integers(4)] = rng.choice(specials)
    for _ in range(max(4, w * h // 40)):
        prev_length[rng.integers(h), rng.integers(w)] = rng.choice(specials)
    return color, motion, prev_color, prev_motion, prev_length


@pytest.mark.parametrize("size", [(40, 24), (17, 33)])
def test_reproject_equals_the_restatement_bit_for_bit(scene, size):
    import torch
    from gltf_renderer_amd.renderer import Renderer
    w, h = size
    rng = np.random.default_rng(w)
    imgs = synthetic(rng, w, h)
    r = Renderer(0)
    dev = [torch.from_numpy(a.copy()).cuda() for a in imgs]
    for cfg, with_length in ((None, True), (abi.PtReprojectConfig(0.3, 6.0, 0.05), True), (None, False)):
        kw = {} if cfg is None else dict(alpha_min=cfg.alpha_min, max_history=cfg.max_history, depth_tolerance=cfg.depth_tolerance)
        want_c, want_l, used = mo.reproject(*imgs[:4], imgs[4] if with_length else None, **kw)
        assert used.sum() >= w * h // 4 and (~used).sum() >= w * h // 8
        out_c, out_l = r.reproject(dev[0], dev[1], dev[2], dev[3], dev[4] if with_length else None, config=cfg)
        got_c, got_l = out_c.cpu().numpy(), out_l.cpu().numpy()
        assert np.array_equal(bits(got_l), bits(want_l)), int((bits(got_l) != bits(want_l)).sum())
        assert np.array_equal(bits(got_c), bits(want_c)), int((bits(got_c) != bits(want_c)).any(axis=-1).sum())
        assert np.array_equal(bits(got_c[~used]), bits(imgs[0][~used])) and np.all(got_l[~used] == 1)     # pass-through: all four channels
        # in place
        col = dev[0].clone()
        r.reproject(col, dev[1], dev[2], dev[3], dev[4] if with_length else None, out_color=col, out_length=out_l, config=cfg)
        assert np.array_equal(bits(col.cpu().numpy()), bits(want_c))
    # every refused argument leaves poisoned outputs intact
    L = r.L
    oc = torch.full((h, w, 4), POISON, dtype=torch.float32, device="cuda")
    ol = torch.full((h, w), POISON, dtype=torch.float32, device="cuda")
    big = torch.zeros((2 * h * w * 4,), dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)

    def call(cfg=None, color=dev[0], motion=dev[1], pc=dev[2], pm=dev[3], pl=dev[4], ww=w, hh=h, out_c=oc, out_l=ol):
        return L.pt_reproject(r.h, C.byref(cfg) if cfg is not None else None, ptr(color), ptr(motion), ptr(pc), ptr(pm), ptr(pl), ww, hh, ptr(out_c), ptr(out_l))

    P = abi.PtReprojectConfig
    nan, inf = float("nan"), float("inf")
    for kw in (dict(color=None), dict(motion=None), dict(pc=None), dict(pm=None), dict(out_c=None), dict(out_l=None), dict(ww=0), dict(hh=0),
               dict(ww=(1 << 30) + 1), dict(hh=(1 << 30) + 1),
               dict(cfg=P(-0.1, 32.0, 0.02)), dict(cfg=P(1.5, 32.0, 0.02)), dict(cfg=P(nan, 32.0, 0.02)), dict(cfg=P(0.1, 0.5, 0.02)),
               dict(cfg=P(0.1, inf, 0.02)), dict(cfg=P(0.1, nan, 0.02)), dict(cfg=P(0.1, 32.0, 0.0)), dict(cfg=P(0.1, 32.0, inf)), dict(cfg=P(0.1, 32.0, nan)),
               dict(out_c=dev[1]), dict(out_c=dev[2]), dict(out_c=dev[3]), dict(out_l=dev[4]),
               dict(color=big.data_ptr(), out_c=big.data_ptr() + 16),                     # overlaps color without being color
               dict(pc=big.data_ptr(), out_l=big.data_ptr() + 4 * (h * w * 4 - 1))):      # the last float of prev_color
        before = [t.clone() for t in dev]
        assert call(**kw) == -1, kw
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, dev)), kw
    assert bool((oc == POISON).all()) and bool((ol == POISON).all()) and bool((big == 0).all())
    assert call() == 0 and call(pl=None) == 0
    r.close()


def test_two_frames_of_a_moved_instance_reproject_onto_each_other(scene):
    """Frame 0: instance MOVED lifted 2.5 towards the camera, to a view depth of about 1.8: the quads behind it lie at 4.0 .. 4.6, and a pixel
    that k of its 8 samples see has a mean depth of k / 8 of that -- at most 1.725 for k = 3, at least 2.0 for k = 4 -- so nothing behind it
    comes within the 2 % tolerance of 1.8.  Frame 1: the same instance 1.5 to the side, about 10 pixels.  Pixels it covered in every sample of
    frame 0 and in none of frame 1 are disoccluded: what shows there now has no history."""
    st = scene.settings
    T0, T1 = camera.translate((0.0, -2.5, 0.0)), camera.translate((1.5, -2.5, 0.0))
    cam = same_camera(scene)
    c = Ctx(scene, prev=cam)
    c.move(MOVED, T0)
    saw0 = np.stack([c.records(single(st), f)[..., 4] == MOVED for f in range(N)])
    accumulate(c, st)
    color0, motion0 = c.out.clone(), c.mv.clone()
    c.r.motion_snapshot()
    c.move(MOVED, T1)
    c.r.set_motion(c.mv, *cam)
    saw1 = np.stack([c.records(single(st), f)[..., 4] == MOVED for f in range(N)])
    accumulate(c, st)
    out_c, out_l = c.r.reproject(c.out, c.mv, color0, motion0)
    got_c, got_l = out_c.cpu().numpy(), out_l.cpu().numpy()
    h_color1, h_motion1 = c.r.readback(c.out), c.target()
    want_c, want_l, used = mo.reproject(h_color1, h_motion1, color0.cpu().numpy(), motion0.cpu().numpy())
    assert used.sum() >= 200
    assert np.array_equal(bits(got_c[used]), bits(want_c[used])) and np.array_equal(bits(got_l[used]), bits(want_l[used]))
    assert np.array_equal(bits(got_c), bits(want_c)) and np.array_equal(bits(got_l), bits(want_l))
    # the moved instance carries its history with it: its pixels read 1.5 world units, several pixels, to the left
    on_it = saw1.all(axis=0)
    assert on_it.sum() >= 4 and np.all(h_motion1[on_it][:, 0] < -3.0) and np.all(np.abs(h_motion1[on_it][:, 2] - 1.8) < 0.4)
    assert (used & on_it).sum() * 2 >= on_it.sum() and np.all(got_l[used & on_it] == 2.0)
    disoccluded = saw0.all(axis=0) & ~saw1.any(axis=0)
    assert disoccluded.sum() >= 4
    assert not used[disoccluded].any() and np.array_equal(bits(got_c[disoccluded]), bits(h_color1[disoccluded])) and np.all(got_l[disoccluded] == 1.0)
    c.close()
