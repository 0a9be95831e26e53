"""pt_bloom (include/mipt.h) on the MI355X: the down and up kernels of csrc/bloom.hip against tests/bloom_ref.py, which restates the header's
definition in numpy float32 -- bit for bit, all four channels, on poisoned output.  The images are synthetic (a context without a scene is
enough) except in the last test, which blooms an accumulated frame of the matte test's confetti scene."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import bloom_ref as bl

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
POISON = 7.0
# 17 x 33: ragged tiles both ways; 40 x 3: the height collapses at level 1, 1 x 1 after 5 levels; 1 x 1: no level; 2 x 1: one level of 1 x 1;
# 67 x 35: 1 x 1 after 6 levels; 130 x 70: several workgroups both ways at levels 0 and 1
SIZES = [(17, 33), (40, 3), (1, 1), (2, 1), (67, 35), (130, 70)]
THRESHOLD = 0.75
CONFIGS = [dict(bl.DEFAULTS),
           dict(iterations=6, strength=0.5, threshold=0.0),
           dict(iterations=8, strength=1.0, threshold=0.0),                # more than any of the sizes has: clamped
           dict(iterations=3, strength=0.25, threshold=THRESHOLD)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def config(kw):
    return abi.PtBloomConfig(kw["iterations"], kw["strength"], kw["threshold"])


@pytest.fixture(scope="module")
def r():
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def fields():
    """One image per size, and the restatement's answer per config: computed once, shared, never written."""
    out = {}
    for (w, h) in SIZES:
        color = bl.random_field(np.random.default_rng(w), w, h)
        out[(w, h)] = (color, [bl.bloom(color, **kw) for kw in CONFIGS])
    return out


def run(r, color, kw=None, in_place=False):
    """One call on poisoned output (or in place): the result on the host.  A pixel the kernels do not write keeps the poison and fails the
    comparison."""
    import torch
    h, w = color.shape[:2]
    src = torch.from_numpy(color.copy()).cuda()
    out = src if in_place else torch.full((h, w, 4), POISON, dtype=torch.float32, device="cuda")
    got = r.bloom(src, out=out, config=None if kw is None else config(kw))
    assert got is out
    if not in_place:
        assert np.array_equal(bits(src.cpu().numpy()), bits(color))        # the input is read only
    return out.cpu().numpy()


def mismatches(got, want):
    return int((bits(got) != bits(want)).any(axis=-1).sum())


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_equals_the_restatement_bit_for_bit(r, fields, size):
    w, h = size
    color, answers = fields[size]
    for k, kw in enumerate(CONFIGS):
        want, info = answers[k]
        finite = ~info["nonfinite"]
        figures = [int(info[m].sum()) for m in ("nonfinite", "negative", "clamped")]
        above = int((finite & ~info["below"]).sum())
        print(size, kw, "levels", info["sizes"], "non-finite, negative, above 65504:", figures, "above the threshold %d of %d finite" % (above, finite.sum()))
        if w * h > 256:                                # a condition on the input, checked before the GPU is asked
            assert min(figures) >= 4, figures
            if kw["threshold"] > 0:
                assert 0.1 * finite.sum() <= above <= 0.9 * finite.sum()
        got = run(r, color, None if k == 0 else kw)
        assert mismatches(got, want) == 0, (kw, mismatches(got, want))
        assert np.array_equal(bits(got[~finite]), bits(color[~finite])) and np.array_equal(bits(got[..., 3]), bits(color[..., 3]))
        if info["sizes"]:
            assert mismatches(got[finite], color[finite]) > 0.9 * finite.sum() or w * h <= 2          # it did something
        else:
            assert np.array_equal(bits(got), bits(color))
    # the defaults spelled out are the defaults
    assert np.array_equal(bits(run(r, color, CONFIGS[0])), bits(answers[0][0]))
    # the clamped run is the run with exactly the levels there are
    n = len(bl.level_sizes(w, h, 8))
    assert np.array_equal(bits(run(r, color, dict(CONFIGS[2], iterations=n))), bits(answers[2][0]))


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_in_place_equals_out_of_place(r, fields, size):
    color, answers = fields[size]
    for k in (0, 3):
        assert np.array_equal(bits(run(r, color, CONFIGS[k], in_place=True)), bits(answers[k][0])), CONFIGS[k]


def test_no_levels_and_no_strength_copy_all_four_channels(r, fields):
    color, _ = fields[(67, 35)]
    for kw in (dict(bl.DEFAULTS, iterations=0), dict(bl.DEFAULTS, strength=0.0), dict(iterations=0, strength=0.0, threshold=3.0)):
        assert np.array_equal(bits(run(r, color, kw)), bits(color)), kw
        assert np.array_equal(bits(run(r, color, kw, in_place=True)), bits(color)), kw


def test_the_chain_is_regrown_and_reused_across_sizes(r, fields):
    a, b = fields[(130, 70)], fields[(17, 33)]
    first = run(r, a[0], CONFIGS[1])
    second = run(r, b[0], CONFIGS[1])                  # a smaller chain
    third = run(r, a[0], CONFIGS[1])                   # ... and a larger one again
    fourth = run(r, a[0], CONFIGS[3])                  # the same size with fewer levels
    assert mismatches(first, a[1][1][0]) == 0 and mismatches(second, b[1][1][0]) == 0
    assert np.array_equal(bits(third), bits(first)) and mismatches(fourth, a[1][3][0]) == 0


def test_refusals_write_nothing_and_a_valid_call_follows(fields):
    import torch
    from gltf_renderer_amd.renderer import Renderer
    w, h = 17, 33
    color, answers = fields[(w, h)]
    r = Renderer(0)
    L = r.L
    dev = torch.from_numpy(color.copy()).cuda()
    out = torch.full((h, w, 4), POISON, dtype=torch.float32, device="cuda")
    big = torch.zeros((2 * h * w * 4,), dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)

    def call(ctx=r.h, cfg=None, c=dev, ww=w, hh=h, o=out):
        return L.pt_bloom(ctx, C.byref(cfg) if cfg is not None else None, ptr(c), ww, hh, ptr(o))

    P = abi.PtBloomConfig
    nan, inf = float("nan"), float("inf")
    image_bytes = h * w * 16
    cases = [dict(ctx=None), dict(c=None), dict(o=None), dict(ww=0), dict(hh=0), dict(ww=(1 << 30) + 1), dict(hh=(1 << 30) + 1),
             dict(ww=1 << 16, hh=1 << 15),                                                 # 2^31 pixels
             dict(cfg=P(9, 0.01, 0.0)), dict(cfg=P(-1, 0.01, 0.0)),
             dict(cfg=P(4, -0.5, 0.0)), dict(cfg=P(4, nan, 0.0)), dict(cfg=P(4, inf, 0.0)),
             dict(cfg=P(4, 0.01, -1.0)), dict(cfg=P(4, 0.01, nan)), dict(cfg=P(4, 0.01, inf)),
             dict(cfg=P(0, 0.01, nan)), dict(cfg=P(9, 0.0, 0.0)),                          # a call that would only copy is checked all the same
             dict(c=big.data_ptr(), o=big.data_ptr() + 16),                                # out one pixel into color
             dict(c=big.data_ptr() + 16, o=big.data_ptr()),                                # color one pixel into out
             dict(c=big.data_ptr() + image_bytes - 16, o=big.data_ptr())]                  # out's last pixel is color's first
    for kw in cases:
        before = dev.clone()
        assert call(**kw) == -1, kw
        assert torch.equal(before.view(torch.int32), dev.view(torch.int32)), kw
    assert bool((out == POISON).all()) and bool((big == 0).all())
    # the boundary values themselves are accepted, and the call after the refusals is the restatement's
    assert call(cfg=P(8, 1.0, 0.0)) == 0
    assert mismatches(out.cpu().numpy(), answers[2][0]) == 0
    assert call(cfg=P(0, 0.0, 0.0)) == 0
    assert np.array_equal(bits(out.cpu().numpy()), bits(color))
    r.close()


def test_a_traced_frame_blooms_as_the_restatement_says():
    """The confetti scene at 40 x 24, 8 accumulated frames: the filter takes pt_trace's own output, out of place and in place."""
    from tests.test_gpu_matte import confetti
    from tests.test_gpu_motion import Ctx, accumulate
    scene = confetti()
    c = Ctx(scene)
    accumulate(c, scene.settings)
    color = c.r.readback(c.out)
    kw = dict(iterations=4, strength=0.5, threshold=0.0)
    want, info = bl.bloom(color, **kw)
    finite = ~info["nonfinite"]
    assert finite.sum() > 0.9 * finite.size and (color[finite][:, :3] > 0).any()
    got = c.r.bloom(c.out, config=config(kw)).cpu().numpy()
    assert mismatches(got, want) == 0, mismatches(got, want)
    assert np.all(got[finite][:, :3] >= color[finite][:, :3]) and (got[finite][:, :3] > color[finite][:, :3]).all(axis=-1).sum() > 0.9 * finite.sum()
    assert c.r.bloom(c.out, out=c.out, config=config(kw)) is c.out
    assert mismatches(c.r.readback(c.out), want) == 0
    c.close()
