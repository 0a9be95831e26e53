"""Saving and resuming an accumulation (include/mipt.h pt_accum_save / pt_accum_load) on the MI355X.

The yardstick is the run that was never interrupted: trace, save, close the renderer, open a new one, upload the scene again, load into
fresh zero-filled targets and trace on with reset = 0 must give, bit for bit on all four channels, what the same calls give without the
interruption -- the output, the AOV targets and the adaptive tile state alike.  The blobs are parsed with the independent reader
tests/checkpoint_ref.py and their sections compared with its numpy tile pack of the images read back."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes
from tests import adaptive_ref as ar
from tests import checkpoint_ref as cr

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 72, 40                      # 5 x 3 tiles, ragged in both directions
TILES = 15
SENTINEL = 7.0
NOT_READY, INVALID = -6, -1


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def make_scene():
    s = scenes.test_scene(W, 16)
    s.width, s.height = W, H
    return s


class Ctx:
    """A renderer with the scene uploaded, its targets, and the options of a run: samples per trace, AOVs, adaptive config, kernel mode."""

    def __init__(self, s, spt=1, aov=False, adaptive=None, mode=None, fill=0.0):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        self.env = s.upload(self.r).get("env")
        self.st = copy_settings(s.settings)
        self.out = self.r.create_output(W, H)
        self.alb = self.r.create_output(W, H) if aov else None
        self.nd = self.r.create_output(W, H) if aov else None
        self.spt = spt
        self.r.set_samples_per_trace(spt)
        if mode is not None:
            self.r.set_kernel_mode(mode)
        if aov:
            self.r.set_aov(self.alb, self.nd)
        if adaptive is not None:
            self.r.set_adaptive(*adaptive)
        if fill:
            for t in self.targets():
                t.fill_(fill)

    def targets(self):
        return [t for t in (self.out, self.alb, self.nd) if t is not None]

    def trace(self, first, last, **kw):
        """Calls of `spt` samples for frames first .. last - 1."""
        for f in range(first, last, self.spt):
            self.r.trace(self.st, self.s.execute_params(f, env_handle=self.env, **kw), self.out)

    def trace_adaptive(self, first, cap, **kw):
        """The host loop of an adaptive run from frame `first`: until no tile is active or the cap is reached."""
        frame, active = first, 1
        while active and frame < cap:
            self.trace(frame, frame + self.spt, **kw)
            frame += self.spt
            active = self.r.adaptive_read(W, H)[0]
        return frame

    def save(self, next_frame, rank=0, world=1):
        return self.r.accum_save(W, H, self.out, self.alb, self.nd, rank=rank, world=world, next_frame=next_frame)

    def load(self, blob):
        return self.r.accum_load(blob, self.out, self.alb, self.nd)

    def read(self):
        return [self.r.readback(t) for t in self.targets()]

    def frames(self):
        return self.r.stats().accumulated_frames

    def close(self):
        self.r.close()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def data():
    """The scene, the uniform accumulation after 1 .. 4 frames traced one by one, and the adaptive threshold: the median tile error after
    4 samples, from the run's own raw frames through tests/adaptive_ref.py."""
    s = make_scene()
    a = Ctx(s)
    a.st.flags &= ~abi.FLAG_ACCUMULATE
    raw = []
    for f in range(4):
        a.trace(f, f + 1)
        raw.append(a.read()[0])
    a.close()
    b = Ctx(s)
    uni = []
    for f in range(4):
        b.trace(f, f + 1)
        uni.append(b.read()[0])
    b.close()
    I, A = ar.fold(raw)
    for n in range(4):
        assert np.array_equal(I[n], uni[n])
    e = np.sort(ar.tile_errors(I[3], A[3]).ravel())
    return dict(scene=s, uni=uni, threshold=float(e[len(e) // 2]))


def interrupted(s, first, total, **kw):
    """Trace frames 0 .. first - 1, save, close; a new renderer, fresh zero-filled targets, load, trace first .. total - 1.
    Returns the final context (open) and the blob."""
    a = Ctx(s, **kw)
    a.trace(0, first)
    blob = a.save(first)
    a.close()
    b = Ctx(s, **kw)
    info = b.load(blob)
    assert info.next_frame == first and info.accumulated_frames == first
    b.trace(first, total)
    return b, blob


@pytest.mark.parametrize("spt,first,total", [(1, 5, 12), (4, 4, 12)])
def test_a_uniform_accumulation_resumes_bit_for_bit(data, spt, first, total):
    s = data["scene"]
    ref = Ctx(s, spt=spt)
    ref.trace(0, total)
    want = ref.read()
    assert ref.frames() == total
    ref.close()
    b, blob = interrupted(s, first, total, spt=spt)
    assert same(b.read(), want)
    assert b.frames() == total
    b.close()
    assert len(blob) == 160 + TILES * 4096 and cr.parse(blob)["sections"] == cr.OUTPUT
    # the control: the same continuation without the load starts a new accumulation in its zero-filled target
    c = Ctx(s, spt=spt)
    c.trace(first, total)
    assert not same(c.read(), want) and c.frames() == total - first
    c.close()


def test_an_adaptive_accumulation_resumes_with_its_tile_state(data):
    s, thr = data["scene"], data["threshold"]
    cfg = (2, 16, thr)
    ref = Ctx(s, spt=2, adaptive=cfg)
    ref.trace_adaptive(0, 16)
    want_img, want_state = ref.read(), ref.r.adaptive_read(W, H)
    ref.close()
    assert want_state[0] == 0

    a = Ctx(s, spt=2, adaptive=cfg)
    a.trace(0, 4)
    active, samples, error, half = a.r.adaptive_read(W, H)
    assert 0 < active < TILES, active              # the save catches retired and active tiles
    img = a.read()[0]
    blob = a.save(4)
    a.close()
    # the blob, read by the independent parser, holds the numpy pack of what was read back
    d = cr.parse(blob)
    assert d["sections"] == cr.OUTPUT | cr.ADAPTIVE and d["accumulated_frames"] == 4 and d["next_frame"] == 4 and d["tiles"] == TILES
    assert (d["width"], d["height"], d["tile_rank"], d["tile_rank_count"]) == (W, H, 0, 1)
    assert d["adaptive"][:3] == (1, 2, 16) and f32(d["adaptive"][3]).tobytes() == f32(thr).tobytes()
    assert np.array_equal(d["output"].view(np.uint32), cr.pack(img).view(np.uint32))
    assert np.array_equal(d["half"].view(np.uint32), cr.pack(half).view(np.uint32))
    assert np.array_equal(d["records"][:, 1], samples.ravel())
    assert np.array_equal(d["records"][:, 2], error.ravel().view(np.uint32))
    assert int(d["records"][:, 0].sum()) == active and np.all(d["records"][:, 3] == 0)
    assert np.all(samples.ravel()[d["records"][:, 0] == 1] == 4)                  # an active tile holds the context's count
    p = s.execute_params(0)                                                       # the camera pt_trace compares: view_to_clip x world_to_view, column-major
    vc, wv = (np.array(m[:], np.float64).reshape(4, 4).T for m in (p.view_to_clip, p.world_to_view))
    assert np.allclose(d["world_to_clip"].reshape(4, 4).T, vc @ wv, rtol=1e-5, atol=1e-5)

    b = Ctx(s, spt=2, adaptive=cfg)
    info = b.load(blob)
    assert info.sections == 9 and info.adaptive.max_samples == 16
    got0 = b.r.adaptive_read(W, H)                   # the state is there before any trace
    assert got0[0] == active and np.array_equal(got0[1], samples) and np.array_equal(got0[2].view(np.uint32), error.view(np.uint32))
    assert np.array_equal(got0[3], half)
    b.trace_adaptive(4, 16)
    got_img, got_state = b.read(), b.r.adaptive_read(W, H)
    assert same(got_img, want_img)
    assert got_state[0] == want_state[0] == 0
    assert np.array_equal(got_state[1], want_state[1])
    assert np.array_equal(got_state[2].view(np.uint32), want_state[2].view(np.uint32))
    assert np.array_equal(got_state[3], want_state[3])
    assert len(set(want_state[1].ravel().tolist())) >= 2      # tiles stopped at different counts, on both sides of the save
    assert want_state[1].max() > 4 and want_state[1].min() <= 4
    b.close()


def test_the_aov_targets_resume_with_the_output(data):
    s = data["scene"]
    ref = Ctx(s, spt=4, aov=True)
    ref.trace(0, 12)
    want = ref.read()
    ref.close()
    b, blob = interrupted(s, 4, 12, spt=4, aov=True)
    got = b.read()
    assert len(got) == 3 and same(got, want)
    assert b.frames() == 12
    b.close()
    d = cr.parse(blob)
    assert d["sections"] == 7 and len(blob) == 160 + 3 * TILES * 4096
    assert np.any(want[1] != 0) and np.any(want[2] != 0)


def test_a_tile_shard_saves_and_loads_its_own_tiles_only(data):
    s, thr = data["scene"], data["threshold"]
    rank, world = 1, 3
    kw = dict(tile_rank=rank, tile_rank_count=world)
    opts = dict(spt=2, aov=True, adaptive=(2, 16, thr))
    mine = np.zeros((H, W), bool)
    tx = (W + 15) // 16
    for t in cr.rank_tiles(W, H, rank, world):
        mine[(t // tx) * 16:(t // tx + 1) * 16, (t % tx) * 16:(t % tx + 1) * 16] = True
    ref = Ctx(s, **opts)
    ref.trace_adaptive(0, 16, **kw)
    want_img, want_state = ref.read(), ref.r.adaptive_read(W, H)
    ref.close()

    a = Ctx(s, **opts)
    a.trace(0, 4, **kw)
    blob = a.r.accum_save(W, H, a.out, a.alb, a.nd, rank=rank, world=world, next_frame=4)
    a.close()
    P = 5 * 4096                                    # tiles 1, 4, 7, 10, 13
    assert len(blob) == 160 + 3 * P + 5 * 16 + P
    d = cr.parse(blob)
    assert d["tiles"] == 5 and d["sections"] == 15 and (d["tile_rank"], d["tile_rank_count"]) == (rank, world)

    b = Ctx(s, fill=SENTINEL, **opts)
    b.load(blob)
    for img in b.read():                            # only the rank's tiles were written
        assert np.all(img[~mine] == SENTINEL) and not np.any(np.all(img[mine] == SENTINEL, axis=-1))
    b.trace_adaptive(4, 16, **kw)
    got_img, got_state = b.read(), b.r.adaptive_read(W, H)
    for g, w_ in zip(got_img, want_img):
        assert np.array_equal(g[mine], w_[mine])
        assert np.all(g[~mine] == SENTINEL)
    assert got_state[0] == want_state[0]
    assert np.array_equal(got_state[1], want_state[1]) and np.array_equal(got_state[2].view(np.uint32), want_state[2].view(np.uint32))
    assert np.array_equal(got_state[3], want_state[3])
    assert np.all(want_state[1].ravel()[[t for t in range(TILES) if t % world != rank]] == 0)
    b.close()


def test_a_uniform_accumulation_resumes_in_the_megakernel_mode(data):
    s = data["scene"]
    ref = Ctx(s, mode=abi.MODE_MEGAKERNEL)
    ref.trace(0, 6)
    want = ref.read()
    ref.close()
    b, _ = interrupted(s, 3, 6, mode=abi.MODE_MEGAKERNEL)
    assert same(b.read(), want) and b.frames() == 6
    b.close()


def save_rc(ctx, capacity=None, buf=None):
    img = abi.PtAccumImages(ctx.out.data_ptr(), ctx.alb.data_ptr() if ctx.alb is not None else None, ctx.nd.data_ptr() if ctx.nd is not None else None)
    need = C.c_size_t(12345)
    rc = ctx.r.L.pt_accum_save(ctx.r.h, C.byref(img), W, H, 0, 1, 0, buf, capacity or 0, C.byref(need))
    return rc, need.value


def load_rc(ctx, blob, out, alb=None, nd=None):
    img = abi.PtAccumImages(*[t.data_ptr() if t is not None else None for t in (out, alb, nd)])
    return ctx.r.L.pt_accum_load(ctx.r.h, bytes(blob), len(blob), C.byref(img))


def test_saves_that_are_refused_leave_the_run_as_it_was(data):
    s, uni = data["scene"], data["uni"]
    # before any trace
    c = Ctx(s)
    rc, need = save_rc(c)
    assert rc == NOT_READY and need == 12345        # nothing written, not even the size
    c.trace(0, 2)
    assert np.array_equal(c.read()[0], uni[1]) and c.frames() == 2
    # a capacity one byte short: the size is reported, the buffer untouched
    rc, need = save_rc(c)
    assert rc == 0 and need == 160 + TILES * 4096
    buf = (C.c_ubyte * need)(*([0x5a] * need))
    rc, got = save_rc(c, need - 1, buf)
    assert rc == INVALID and got == need and bytes(buf) == b"\x5a" * need
    assert "capacity" in c.r.L.pt_last_error(c.r.h).decode()
    c.trace(2, 4)
    assert np.array_equal(c.read()[0], uni[3]) and c.frames() == 4
    c.close()
    # right after pt_set_aov: the next trace starts anew, there is nothing to save
    c = Ctx(s, aov=True)
    c.trace(0, 3)
    c.r.set_aov(c.alb, c.nd)
    rc, need = save_rc(c)
    assert rc == NOT_READY and need == 12345
    c.trace(0, 1)                                   # ... and it does start anew
    assert np.array_equal(c.read()[0], uni[0]) and c.frames() == 1
    # right after pt_set_adaptive likewise; an adaptive call of 2 samples equals the uniform accumulation of 2
    c.r.set_adaptive(2, 16, data["threshold"])
    assert save_rc(c)[0] == NOT_READY
    c.r.set_samples_per_trace(2); c.spt = 2
    c.trace(0, 2)
    assert np.array_equal(c.read()[0], uni[1]) and c.frames() == 2
    assert save_rc(c)[0] == 0
    c.close()


def test_loads_that_are_refused_leave_the_context_and_the_targets_as_they_were(data):
    s, uni, thr = data["scene"], data["uni"], data["threshold"]
    a = Ctx(s, spt=2, aov=True, adaptive=(2, 16, thr))
    a.trace(0, 4)
    full = a.save(4)                                # output + AOVs + adaptive
    a.close()
    a = Ctx(s)
    a.trace(0, 3)
    plain = a.save(3)                               # output only
    a.close()

    def untouched_and_fresh(c, spt):
        """The targets still hold the sentinel; the next trace is the first of a new accumulation."""
        for img in c.read():
            assert np.all(img == SENTINEL)
        c.trace(0, spt)
        assert np.array_equal(c.read()[0], uni[spt - 1]) and c.frames() == spt

    # another adaptive threshold (one ulp), another max_samples, adaptive sampling off
    for cfg in ((2, 16, float(np.nextafter(f32(thr), f32(np.inf)))), (2, 12, thr), None):
        c = Ctx(s, spt=2, aov=True, adaptive=cfg, fill=SENTINEL)
        assert load_rc(c, full, c.out, c.alb, c.nd) == INVALID
        assert "adaptive" in c.r.L.pt_last_error(c.r.h).decode()
        untouched_and_fresh(c, 2)
        c.close()
    # an albedo section without a target, and a target without a section
    c = Ctx(s, spt=2, aov=True, adaptive=(2, 16, thr), fill=SENTINEL)
    assert load_rc(c, full, c.out, None, c.nd) == INVALID and "albedo" in c.r.L.pt_last_error(c.r.h).decode()
    assert load_rc(c, full, None, c.alb, c.nd) == INVALID
    assert load_rc(c, plain, c.out, c.alb, None) == INVALID and "albedo" in c.r.L.pt_last_error(c.r.h).decode()
    assert load_rc(c, plain, c.out, None, c.nd) == INVALID and "normal_depth" in c.r.L.pt_last_error(c.r.h).decode()
    # one flipped payload byte
    bad = bytearray(full)
    bad[160 + 4096 * 7 + 3] ^= 0x04
    assert load_rc(c, bad, c.out, c.alb, c.nd) == INVALID and "crc32" in c.r.L.pt_last_error(c.r.h).decode()
    assert load_rc(c, full[:-16], c.out, c.alb, c.nd) == INVALID
    with pytest.raises(Exception):
        c.r.accum_inspect(bad)
    untouched_and_fresh(c, 2)
    # ... and the good blob still loads into that context afterwards, over its running accumulation
    assert load_rc(c, full, c.out, c.alb, c.nd) == 0 and c.frames() == 4
    c.close()


def test_after_a_load_a_moved_camera_or_a_reset_starts_anew(data):
    s, uni = data["scene"], data["uni"]
    a = Ctx(s)
    a.trace(0, 3)
    blob = a.save(3)
    a.close()
    moved = camera.cm(camera.orbit_world_to_view((0, 0, 0.6), 3.7, 0.35, -0.45))

    def moved_params(c, frame):
        p = s.execute_params(frame, env_handle=c.env)
        p.world_to_view[:] = moved
        return p

    ref = Ctx(s)
    ref.r.trace(ref.st, moved_params(ref, 3), ref.out)
    want = ref.read()[0]
    ref.close()
    b = Ctx(s)
    b.load(blob)
    assert b.frames() == 3 and np.array_equal(b.read()[0], uni[2])
    b.r.trace(b.st, moved_params(b, 3), b.out)
    assert b.frames() == 1 and np.array_equal(b.read()[0], want)
    # settings.reset
    b.load(blob)
    b.st.reset = 1
    b.trace(0, 1)
    assert b.frames() == 1 and np.array_equal(b.read()[0], uni[0])
    # and with neither, the loaded accumulation goes on
    b.st.reset = 0
    b.load(blob)
    b.trace(3, 4)
    assert b.frames() == 4 and np.array_equal(b.read()[0], uni[3])
    b.close()


# ---- every setter that restarts the accumulation leaves one pending restart -------------------------------------------------------------------
SW = SH = 16
SPT = 2
RESTART_MESSAGE = ("accum_save: pt_set_adaptive / pt_set_aov / pt_set_lens / pt_set_bake / pt_set_probes / pt_set_matte / pt_set_motion since the last trace: "
                   "the next trace starts anew")


class Small:
    """A 16 x 16 context of the scene without a map, with one feature configured; set() calls that feature's setter again: the current config
    for adaptive, AOV, lens, matte and motion, the disabled one for bake and probes."""

    def __init__(self, s, feature):
        from gltf_renderer_amd.renderer import Renderer
        self.s, self.r, self.feature = s, Renderer(0), feature
        s.upload(self.r)
        self.st = copy_settings(s.settings)
        self.r.set_samples_per_trace(SPT)
        self.out = self.r.create_output(SW, SH)
        self.extra = [self.r.create_output(SW, SH) for _ in range(2)]
        self.set()

    def set(self):
        r, p = self.r, self.s.execute_params(0)
        {"adaptive": lambda: r.set_adaptive(2, 64, 0.0),
         "aov": lambda: r.set_aov(*self.extra),
         "lens": lambda: r.set_lens(0.05, 3.0),
         "bake": lambda: r.set_bake(1e-3, enable=False),
         "probes": lambda: r.set_probes(None, 0, enable=False),
         "matte": lambda: r.set_matte(abi.MATTE_INSTANCE, self.extra[:1]),
         "motion": lambda: r.set_motion(self.extra[0], list(p.world_to_view), list(p.view_to_clip))}[self.feature]()

    def trace(self, frame, **change):
        p = self.s.execute_params(frame)
        for k, v in change.items():
            if k == "world_to_view":
                p.world_to_view[:] = v
            else:
                setattr(p, k, v)
        self.r.trace(self.st, p, self.out)

    def save_rc(self, buf=None, capacity=0):
        img = abi.PtAccumImages(self.out.data_ptr(), None, None)
        need = C.c_size_t(0)
        rc = self.r.L.pt_accum_save(self.r.h, C.byref(img), SW, SH, 0, 1, 0, buf, capacity, C.byref(need))
        return rc, need.value, self.r.L.pt_last_error(self.r.h).decode()

    def save(self):
        rc, need, _ = self.save_rc()
        assert rc == 0
        buf = (C.c_ubyte * need)()
        assert self.save_rc(buf, need)[0] == 0
        return bytes(buf)

    def load(self, blob):
        img = abi.PtAccumImages(self.out.data_ptr(), None, None)
        assert self.r.L.pt_accum_load(self.r.h, blob, len(blob), C.byref(img)) == 0, self.r.L.pt_last_error(self.r.h).decode()

    def frames(self):
        return self.r.stats().accumulated_frames

    def close(self):
        self.r.close()


@pytest.mark.parametrize("feature", ["adaptive", "aov", "lens", "bake", "probes", "matte", "motion"])
def test_every_setter_leaves_one_pending_restart(feature):
    from gltf_renderer_amd.renderer import MiptError
    s = scenes.test_scene(SW, 16, with_env=False)
    a = Small(s, feature)
    a.trace(0)
    first = a.r.readback(a.out)
    a.trace(SPT)
    assert a.frames() == 2 * SPT and first[..., :3].std() > 0
    blob = a.save()                                  # two calls accumulated, nothing pending: a save goes through
    a.set()
    rc, _, msg = a.save_rc()
    assert rc == NOT_READY and msg == RESTART_MESSAGE, (rc, msg)
    # a trace refused before the restart is consumed -- the camera is the first thing looked at -- leaves it pending
    with pytest.raises(MiptError, match="singular camera"):
        a.trace(2 * SPT, world_to_view=[0.0] * 16)
    rc, _, msg = a.save_rc()
    assert rc == NOT_READY and msg == RESTART_MESSAGE and a.frames() == 2 * SPT, (rc, msg)
    # a trace refused for an environment handle that does not exist: the save is refused afterwards as well.  (That check sits behind the
    # reset, so the restart has already taken effect -- nothing is accumulated any more -- rather than being lost.)
    with pytest.raises(MiptError, match="environment map handle"):
        a.trace(2 * SPT, environment_map=5)
    assert a.save_rc()[0] == NOT_READY
    # the next good trace is the first of a new accumulation, and can be saved
    a.trace(0)
    assert a.frames() == SPT
    assert np.array_equal(a.r.readback(a.out).view(np.uint32), first.view(np.uint32))
    assert a.save_rc()[0] == 0
    a.close()
    # in a second context a load after the setter clears the pending restart: the next trace continues from the blob's count
    b = Small(s, feature)
    b.set()
    b.load(blob)
    assert b.frames() == 2 * SPT and b.save_rc()[0] == 0
    b.trace(2 * SPT)
    assert b.frames() == 3 * SPT
    b.close()
