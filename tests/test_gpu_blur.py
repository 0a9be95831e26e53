"""pt_motion_blur (include/mipt.h) on the MI355X: the three kernels of csrc/blur.hip against tests/blur_ref.py, which restates the header's
definition in numpy float32 -- bit for bit, all four channels.  The images are synthetic (a context without a scene is enough) except in the
last test, which blurs a traced frame of the matte test's confetti scene with its traced motion target."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera
from tests import blur_ref as br

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
POISON = 7.0
SIZES = [(40, 24), (17, 33), (16, 16), (1, 1), (1, 40)]          # ragged tiles both ways, one whole tile, one pixel, one column over three tiles
CONFIGS = [dict(br.DEFAULTS),
           dict(shutter=1.0, max_radius=12.0, taps=7, jitter=0, depth_softness=0.2),
           dict(shutter=0.25, max_radius=64.0, taps=64, jitter=1, depth_softness=0.05),
           dict(shutter=0.5, max_radius=1.0, taps=2, jitter=1, depth_softness=0.05)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def config(kw):
    return abi.PtMotionBlurConfig(kw["shutter"], kw["max_radius"], kw["taps"], kw["jitter"], kw["depth_softness"])


@pytest.fixture(scope="module")
def r():
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def run(r, color, motion, kw=None):
    """One call on poisoned output: the result on the host.  A pixel the kernels do not write keeps the poison and fails the comparison."""
    import torch
    h, w = color.shape[:2]
    out = torch.full((h, w, 4), POISON, dtype=torch.float32, device="cuda")
    got = r.motion_blur(torch.from_numpy(color.copy()).cuda(), torch.from_numpy(motion.copy()).cuda(), out=out, config=None if kw is None else config(kw))
    assert got is out
    return out.cpu().numpy()


def mismatches(got, want):
    return int((bits(got) != bits(want)).any(axis=-1).sum())


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_equals_the_restatement_bit_for_bit(r, size):
    w, h = size
    color, motion = br.random_field(np.random.default_rng(w), w, h)
    for k, kw in enumerate(CONFIGS):
        want, info = br.blur(color, motion, **kw)
        figures = [int(info[m].sum()) for m in ("clamped", "slow", "uncovered", "bad_centre", "blurred")]
        print(size, kw, "clamped, below half a pixel, uncovered, non-finite centre, blurred:", figures, "of", w * h)
        if k == 0 and w * h > 256:                     # the two larger sizes under the defaults: the input exercises the definition
            assert figures[0] >= 16 and figures[1] >= 16 and figures[2] >= 16 and figures[3] >= max(4, w * h // 80) and 2 * figures[4] >= w * h, figures
        got = run(r, color, motion, None if k == 0 else kw)
        assert mismatches(got, want) == 0, (kw, mismatches(got, want))
        assert np.array_equal(bits(got[~info["blurred"]]), bits(color[~info["blurred"]]))          # a copy: all four channels
    # the defaults spelled out are the defaults
    assert np.array_equal(bits(run(r, color, motion, CONFIGS[0])), bits(br.blur(color, motion)[0]))


@pytest.mark.parametrize("size", SIZES[:2], ids=["%dx%d" % s for s in SIZES[:2]])
def test_the_bright_block_field_bit_for_bit(r, size):
    w, h = size
    color, motion, on_block = br.block_field(np.random.default_rng(w), w, h)
    kw = dict(shutter=1.0, max_radius=16.0, taps=16, jitter=1, depth_softness=0.05)
    want, info = br.blur(color, motion, **kw)
    assert (info["counted"] >= 8).sum() >= 40
    got = run(r, color, motion, kw)
    assert mismatches(got, want) == 0, mismatches(got, want)
    changed = (bits(got[..., :3]) != bits(color[..., :3])).any(axis=-1)
    assert (changed & ~on_block).sum() >= 50 and np.all(got[changed & ~on_block][:, :3] >= color[changed & ~on_block][:, :3])
    assert np.array_equal(bits(got[..., 3]), bits(color[..., 3]))


@pytest.mark.parametrize("size", SIZES[:2], ids=["%dx%d" % s for s in SIZES[:2]])
def test_confined_motion_leaves_the_tiles_beyond_reach_alone(r, size):
    w, h = size
    color, motion = br.random_field(np.random.default_rng(w + 1), w, h, confine=(2, 11))
    kw = dict(br.DEFAULTS, max_radius=16.0)
    want, info = br.blur(color, motion, **kw)
    got = run(r, color, motion, kw)
    assert mismatches(got, want) == 0 and not np.any(got == POISON)
    far = (slice(None), slice(32, None)) if w == 40 else (slice(32, None), slice(None))         # the third tile column / the third tile row
    assert got[far].size > 0 and np.array_equal(bits(got[far]), bits(color[far])) and not info["blurred"][far].any()
    near = info["blurred"]
    assert near.sum() > 200 and mismatches(got[near], color[near]) > 100                        # ... and does blur within reach


def test_a_streak_reaches_four_tiles_at_radius_64(r):
    from tests.test_blur_host import reach_field
    color, motion = reach_field()
    kw = dict(br.DEFAULTS, shutter=2.0, max_radius=64.0)
    want, info = br.blur(color, motion, **kw)
    assert np.all(info["N"][0, :5, 2] == 64.0) and np.all(info["N"][0, 5:, 2] == 0.0)
    got = run(r, color, motion, kw)
    assert mismatches(got, want) == 0
    assert np.array_equal(bits(got[:, 80:]), bits(color[:, 80:])) and mismatches(got[:, :80], color[:, :80]) > 100


def test_scratch_is_regrown_and_reused_across_sizes(r):
    fields = {s: br.random_field(np.random.default_rng(7 * s[0]), *s) for s in SIZES[:2]}
    first = run(r, *fields[(40, 24)])
    second = run(r, *fields[(17, 33)])
    third = run(r, *fields[(40, 24)])
    assert np.array_equal(bits(third), bits(first))
    assert mismatches(first, br.blur(*fields[(40, 24)])[0]) == 0 and mismatches(second, br.blur(*fields[(17, 33)])[0]) == 0


def test_refusals_write_nothing_and_a_valid_call_follows():
    import torch
    from gltf_renderer_amd.renderer import Renderer
    w, h = 40, 24
    color, motion = br.random_field(np.random.default_rng(5), w, h)
    r = Renderer(0)
    L = r.L
    dev = [torch.from_numpy(color.copy()).cuda(), torch.from_numpy(motion.copy()).cuda()]
    out = torch.full((h, w, 4), POISON, dtype=torch.float32, device="cuda")
    big = torch.zeros((2 * h * w * 4,), dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)

    def call(ctx=r.h, cfg=None, c=dev[0], m=dev[1], ww=w, hh=h, o=out):
        return L.pt_motion_blur(ctx, C.byref(cfg) if cfg is not None else None, ptr(c), ptr(m), ww, hh, ptr(o))

    P = abi.PtMotionBlurConfig
    nan, inf = float("nan"), float("inf")
    image_bytes = h * w * 16
    cases = [dict(ctx=None), dict(c=None), dict(m=None), dict(o=None), dict(ww=0), dict(hh=0), dict(ww=(1 << 30) + 1), dict(hh=(1 << 30) + 1),
             dict(ww=1 << 16, hh=1 << 15),                                                 # 2^31 pixels
             dict(cfg=P(0.0, 32.0, 16, 1, 0.05)), dict(cfg=P(-1.0, 32.0, 16, 1, 0.05)), dict(cfg=P(2.5, 32.0, 16, 1, 0.05)),
             dict(cfg=P(nan, 32.0, 16, 1, 0.05)), dict(cfg=P(inf, 32.0, 16, 1, 0.05)),
             dict(cfg=P(0.5, 0.5, 16, 1, 0.05)), dict(cfg=P(0.5, 64.5, 16, 1, 0.05)), dict(cfg=P(0.5, nan, 16, 1, 0.05)), dict(cfg=P(0.5, inf, 16, 1, 0.05)),
             dict(cfg=P(0.5, 32.0, 1, 1, 0.05)), dict(cfg=P(0.5, 32.0, 65, 1, 0.05)), dict(cfg=P(0.5, 32.0, -3, 1, 0.05)),
             dict(cfg=P(0.5, 32.0, 16, 1, 0.0)), dict(cfg=P(0.5, 32.0, 16, 1, -0.05)), dict(cfg=P(0.5, 32.0, 16, 1, inf)), dict(cfg=P(0.5, 32.0, 16, 1, nan)),
             dict(o=dev[0]), dict(o=dev[1]),                                               # in place
             dict(c=big.data_ptr(), o=big.data_ptr() + 16),                                # out one pixel into color
             dict(c=big.data_ptr() + 16, o=big.data_ptr()),                                # color one pixel into out
             dict(m=big.data_ptr() + image_bytes - 16, o=big.data_ptr())]                  # out's last pixel is motion's first
    for kw in cases:
        before = [t.clone() for t in dev]
        assert call(**kw) == -1, kw
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, dev)), kw
    assert bool((out == POISON).all()) and bool((big == 0).all())
    # the boundary values themselves are accepted, and the call after the refusals is the restatement's
    for cfg, kw in ((P(2.0, 1.0, 2, 0, 0.05), dict(shutter=2.0, max_radius=1.0, taps=2, jitter=0, depth_softness=0.05)),
                    (P(0.5, 64.0, 64, 5, 1e-3), dict(shutter=0.5, max_radius=64.0, taps=64, jitter=1, depth_softness=1e-3))):
        assert call(cfg=cfg) == 0
        assert mismatches(out.cpu().numpy(), br.blur(color, motion, **kw)[0]) == 0
    r.close()


def test_a_traced_frame_of_a_moved_instance_blurs_along_its_motion():
    """The confetti scene at 40 x 24 as in test_gpu_motion's last test: instance MOVED lifted 2.5 towards the camera, the snapshot, then 1.5 to
    the side -- about 10 pixels, so a half streak of about 5 at shutter 1."""
    from tests.test_gpu_matte import confetti, single
    from tests.test_gpu_motion import MOVED, N, Ctx, accumulate, same_camera
    scene = confetti()
    st = scene.settings
    T0, T1 = camera.translate((0.0, -2.5, 0.0)), camera.translate((1.5, -2.5, 0.0))
    cam = same_camera(scene)
    c = Ctx(scene, prev=cam)
    c.move(MOVED, T0)
    c.r.motion_snapshot()
    c.move(MOVED, T1)
    c.r.set_motion(c.mv, *cam)
    saw = np.stack([c.records(single(st), f)[..., 4] == MOVED for f in range(N)])
    accumulate(c, st)
    kw = dict(br.DEFAULTS, shutter=1.0, max_radius=16.0)
    out = c.r.motion_blur(c.out, c.mv, config=config(kw))
    got, color, motion = out.cpu().numpy(), c.r.readback(c.out), c.target()
    want, info = br.blur(color, motion, **kw)
    assert mismatches(got, want) == 0, mismatches(got, want)
    on_it = saw.all(axis=0)
    assert on_it.sum() >= 4 and np.all(np.abs(motion[on_it][:, 0]) > 3.0)
    # beside it along x: in a row of the instance, within 4 pixels of a pixel every sample saw on it, and seen on it by no sample
    near = np.zeros_like(on_it)
    for dx in range(1, 5):
        near[:, dx:] |= on_it[:, :-dx]
        near[:, :-dx] |= on_it[:, dx:]
    beside = near & ~saw.any(axis=0)
    changed = (bits(got[..., :3]) != bits(color[..., :3])).any(axis=-1)
    print("on the instance %d, beside it %d, of those changed %d" % (on_it.sum(), beside.sum(), (beside & changed).sum()))
    assert (beside & changed).sum() >= 4
    assert np.array_equal(bits(got[~info["blurred"]]), bits(color[~info["blurred"]]))
    c.close()
