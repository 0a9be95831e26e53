"""The wavefront arrangement's ray counts and queue reservations on the MI355X.

The generate and shade stages add their tallies (primary, bounce and shadow rays, closest hits, texture taps) to words of their own
shard's counter line, and the resolve stage folds the 256 shards into pt_stats once a trace; the shade stage reserves its shadow-queue and
bounce-queue entries with one atomic instruction per wave and chunk.  Neither may change a number: the counts are held field by field to the
megakernel's, which books every ray directly, for the same frames -- with fewer tiles than shards, one tile, a tile shard, sample batches,
several traces, pt_reset_stats, pt_enable_counters, a retired tile 0 under adaptive sampling, and the bake and probe generate kernels -- and
the images of the two modes are held bit for bit for every pattern of empty and non-empty pushes the merged reservation can meet.

texture_taps is the one field the two modes never agreed on (the megakernel also books the taps of its shadow rays' alpha tests; measured
before this file was written: 1268 against 1465 for frame 0 of the 48 x 32 view), so it is held to the wavefront arrangement's own counts
instead: a batch, a run of traces and an adaptive trace must count the sum of what their frames and tiles count one by one."""
import numpy as np
import pytest

from gltf_renderer_amd import abi, scenes
from tests.test_gpu_bake import OFFSET, Ctx as BakeCtx, lit_scene as bake_scene
from tests.test_gpu_probe import N5, POS5, Ctx as ProbeCtx, lit_scene as probe_scene

pytestmark = pytest.mark.gpu
FIELDS = ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps")
BOTH = 5                                # the first five are the fields both modes count alike
# (width, height, tile_rank, tile_rank_count): 6 tiles (fewer than the 256 shards), one tile, and rank 1 of 3 of a 5 x 3 tile image (5 tiles)
VIEWS = [(48, 32, 0, 1), (16, 16, 0, 1), (80, 48, 1, 3)]
FRAMES = 3


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def counts(r):
    t = r.stats()
    return tuple(int(getattr(t, f)) for f in FIELDS)


def add(*cs):
    return tuple(sum(v) for v in zip(*cs))


class Ctx:
    def __init__(self, w, h, mode, counters=False):
        from gltf_renderer_amd.renderer import Renderer
        self.s = scenes.test_scene(w, 16)
        self.s.width, self.s.height = w, h
        self.r = Renderer(0)
        self.env = self.s.upload(self.r).get("env")
        self.r.set_kernel_mode(mode)
        if counters:
            self.r.enable_counters(True)
        self.out = self.r.create_output(w, h)

    def trace(self, st, frame, **kw):
        self.r.trace(st, self.s.execute_params(frame, env_handle=self.env, **kw), self.out)

    def close(self):
        self.r.close()


def frame_counts(c, st, frames, spp=1, **kw):
    """The counts of each trace of `frames` (first frames of the sample batches), pt_reset_stats before each."""
    c.r.set_samples_per_trace(spp)
    got = []
    for f in frames:
        c.r.reset_stats()
        c.trace(st, f, **kw)
        got.append(counts(c.r))
    return got


@pytest.fixture(scope="module")
def mega():
    """The megakernel's counts of frames 0 .. 2 * FRAMES - 1 of every view, one trace each: the reference of every count below."""
    ref = {}
    for w, h, rank, ranks in VIEWS:
        c = Ctx(w, h, abi.MODE_MEGAKERNEL)
        st = copy_settings(c.s.settings)
        ref[(w, h, rank, ranks)] = frame_counts(c, st, range(2 * FRAMES), tile_rank=rank, tile_rank_count=ranks)
        c.close()
    return ref


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("view", VIEWS)
def test_wavefront_counts_equal_the_megakernels(mega, view, spp, counters):
    w, h, rank, ranks = view
    ref = mega[view]
    kw = dict(tile_rank=rank, tile_rank_count=ranks)
    c = Ctx(w, h, abi.MODE_WAVEFRONT, counters)
    st = copy_settings(c.s.settings)
    # frame by frame, the stats reset before each
    frames = frame_counts(c, st, range(2 * spp), 1, **kw)
    for f, got in enumerate(frames):
        assert got[:BOTH] == ref[f][:BOTH], (f, dict(zip(FIELDS, got)), dict(zip(FIELDS, ref[f])))
        assert got[0] == got[1] + got[2] + got[3] and got[1] > 0 and got[2] > 0 and got[3] > 0 and got[4] > 0 and got[5] > 0
    # a batch of spp samples counts what its frames count one by one
    single = frame_counts(c, st, [0, spp], spp, **kw)
    for k, got in enumerate(single):
        want = add(*frames[k * spp:(k + 1) * spp])
        assert got == want, (k, dict(zip(FIELDS, got)), dict(zip(FIELDS, want)))
    # two consecutive traces count the sum of the single traces
    c.r.reset_stats()
    c.trace(st, 0, **kw); c.trace(st, spp, **kw)
    assert counts(c.r) == add(*single)
    # and pt_reset_stats zeroes them
    c.r.reset_stats()
    assert counts(c.r) == (0,) * len(FIELDS)
    c.close()


def test_debug_output_mode_counts_one_iteration(mega):
    """A debug output ends the path at its first vertex: one shade launch, the resolve right behind it."""
    w, h = 48, 32
    got = {}
    for mode in (abi.MODE_MEGAKERNEL, abi.MODE_WAVEFRONT):
        c = Ctx(w, h, mode)
        st = copy_settings(c.s.settings); st.debug_output = abi.DEBUG_OUTPUT_SHADING_NORMAL
        got[mode] = frame_counts(c, st, [0, 1])
        c.close()
    assert [g[:BOTH] for g in got[abi.MODE_WAVEFRONT]] == [g[:BOTH] for g in got[abi.MODE_MEGAKERNEL]]
    assert got[abi.MODE_WAVEFRONT][0][1] == mega[(w, h, 0, 1)][0][1]          # the primary rays of the frame


def test_counts_with_tile_zero_retired_under_adaptive_sampling():
    """The resolve's workgroup 0 folds the counts, and under adaptive sampling the workgroup of a retired tile leaves at once.  A threshold
    equal to local tile 0's own error after min_samples retires that tile (and any with less error) at min_samples and leaves the others
    active; every later trace must count exactly what the frame's active tiles count when they are rendered one tile at a time, without adaptive
    sampling: by the megakernel (the fields both modes count alike) and by the wavefront arrangement (all of them)."""
    w, h, spp, min_s, cap = 48, 32, 2, 2, 8
    tiles = 6
    # every tile's error after min_samples, from an adaptive run that retires nothing (threshold 0 retires only an exact zero)
    c = Ctx(w, h, abi.MODE_WAVEFRONT)
    st = copy_settings(c.s.settings)
    c.r.set_samples_per_trace(spp)
    c.r.set_adaptive(min_s, cap, 0.0)
    c.trace(st, 0)
    err = c.r.adaptive_read(w, h)[2].ravel()
    # a shard (rank of ranks) whose local tile 0 does not have the largest error of the shard's tiles
    split = next(((k, n) for k, n in [(0, 1), (1, 2), (2, 3), (0, 2), (0, 3), (1, 3)] if err[k] < err[k::n].max()), None)
    assert split is not None, err
    rank, ranks = split
    kw = dict(tile_rank=rank, tile_rank_count=ranks)
    mine = list(range(tiles))[rank::ranks]
    thr = float(err[rank])
    c.r.set_adaptive(min_s, cap, thr)                                  # (starts a new accumulation)
    got, active = [], []
    for k in range(3):
        c.r.reset_stats()
        c.trace(st, k * spp, **kw)
        got.append(counts(c.r))
        samples = c.r.adaptive_read(w, h)[1].ravel()
        active.append([t for t in mine if samples[t] == (k + 1) * spp])          # the tiles this trace still sampled
    assert active[0] == mine and rank not in active[1] and len(active[1]) > 0, (active, err)
    c.r.reset_stats()
    c.r.set_adaptive(min_s, cap, thr)
    for k in range(3):
        c.trace(st, k * spp, **kw)
    assert counts(c.r) == add(*got)
    c.close()
    # one tile at a time (rank t of `tiles` ranks is tile t alone), frame by frame
    for mode, fields in ((abi.MODE_MEGAKERNEL, BOTH), (abi.MODE_WAVEFRONT, len(FIELDS))):
        m = Ctx(w, h, mode)
        sm = copy_settings(m.s.settings)
        for k in range(3):
            want = add(*[add(*frame_counts(m, sm, range(k * spp, (k + 1) * spp), tile_rank=t, tile_rank_count=tiles)) for t in active[k]])
            assert got[k][:fields] == want[:fields], (mode, k, active[k], dict(zip(FIELDS, got[k])), dict(zip(FIELDS, want)))
        m.close()


def check_sums_and_reset(c, st, frames=(0, 1)):
    """Single traces (reset before each), the same traces in a row, the reset: returns the single traces' counts."""
    single = []
    for f in frames:
        c.r.reset_stats()
        c.trace(st, f)
        single.append(counts(c.r))
    c.r.reset_stats()
    for f in frames:
        c.trace(st, f)
    assert counts(c.r) == add(*single)
    c.r.reset_stats()
    assert counts(c.r) == (0,) * len(FIELDS)
    return single


def test_bake_generate_kernel_counts_its_covered_samples():
    w, h = 48, 32
    c = BakeCtx(bake_scene(chart=0.75), bake=(OFFSET, 0, 0))              # the quad's instance alone: its chart leaves texels uncovered
    c.use(w, h)
    st = copy_settings(c.s.settings)
    single = check_sums_and_reset(c, st)
    covered = int((c.r.bake_coverage(w, h)[0] >= 0).sum())
    assert 0 < covered < w * h
    for got in single:
        assert got[1] == covered and got[0] == got[1] + got[2] + got[3] and got[4] > 0
    c.close()


def test_probe_generate_kernel_counts_its_present_cells():
    c = ProbeCtx(probe_scene())
    st = copy_settings(c.s.settings)
    single = check_sums_and_reset(c, st)
    assert c.size[0] * c.size[1] > len(POS5) * N5 * N5                 # (the atlas has an empty cell)
    for got in single:
        assert got[1] == len(POS5) * N5 * N5 and got[0] == got[1] + got[2] + got[3] and got[4] > 0
    c.close()


def with_flags(st, off=0, max_bounces=None):
    st = copy_settings(st)
    st.flags &= ~off
    if max_bounces is not None:
        st.min_bounces = min(st.min_bounces, max_bounces); st.max_bounces = max_bounces
    return st


# which of the wave's three pushes (environment shadow rays, light shadow rays, bounce rays) a flag set leaves
PUSHES = {
    "default": dict(),                                                  # all three
    "no_point_lights": dict(off=abi.FLAG_POINT_LIGHTS),                 # environment and bounce
    "no_environment_mis": dict(off=abi.FLAG_ENVIRONMENT_MIS),           # light and bounce
    "no_environment_map": dict(off=abi.FLAG_ENVIRONMENT_MAP),           # light and bounce
    "no_shadow_rays": dict(off=abi.FLAG_SHADOW_RAYS),                   # bounce only
    "no_bounces": dict(max_bounces=0),                                  # environment and light, no bounce
}


@pytest.mark.parametrize("name", sorted(PUSHES))
def test_images_of_both_modes_are_bit_identical(name):
    w, h = 48, 32
    img, cnt = {}, {}
    for mode in (abi.MODE_MEGAKERNEL, abi.MODE_WAVEFRONT):
        c = Ctx(w, h, mode)
        st = with_flags(c.s.settings, **PUSHES[name])
        img[mode] = []
        c.r.reset_stats()
        for f in range(FRAMES):
            c.trace(st, f)
            img[mode].append(c.r.readback(c.out).view(np.uint32))
        cnt[mode] = counts(c.r)
        c.close()
    for f in range(FRAMES):
        assert np.array_equal(img[abi.MODE_WAVEFRONT][f], img[abi.MODE_MEGAKERNEL][f]), (name, f)
    assert cnt[abi.MODE_WAVEFRONT][:BOTH] == cnt[abi.MODE_MEGAKERNEL][:BOTH]
    # (rays_shadow is no witness of the shadow pushes: with FLAG_SHADOW_RAYS off the untraced shadow rays are still counted, as the reference does)
    assert (cnt[abi.MODE_WAVEFRONT][2] == 0) == (name == "no_bounces")
