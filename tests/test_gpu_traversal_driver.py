"""The wavefront mode's traversal driver and the any-hit paths, ray for ray (run with -m gpu on an MI355X).

pt_debug_intersect runs traverse(), the megakernel's driver (one ray per lane, the ordered node step).  The default mode -- the one the
benchmark measures -- runs trace_persistent<COUNT, MODE> inside k_wf_trace, k_wf_shadow and the fused k_wf_traverse: lanes refilled from a
shard's queue, the unordered node step for occlusion rays, the DEFAULTS copies, a deep stack indexed by the stage grid.  The test hook
pt_debug_trace_queues (tests/ray_hook.py trace_queues) launches those kernels, through the launch functions a frame uses, on queues filled here:

  a. closest rays: the six flags x bounce rows of launch_wavefront's ray-flag rule, bit for bit against traverse() and the oracle;
  b. occlusion rays through k_wf_shadow and the fused kernel: accept-first, alpha shadows, environment rays under ALPHA_SHADOWS;
  c. both drivers against the float64 restatement of the any-hit rules (tests/traversal_ref.py) on the layered alpha scene, and on
     scenes.test_scene (LINEAR-filtered alpha) against the oracle within the sampler's tolerance;
  d. queue shapes: per-shard counts around the wave, refill and workgroup sizes, at every blocks_per_shard a frame uses;
  e. the deep stack under the stage grid, lanes tracing several rays in a row on one deep-stack column; the deep stacks that
     pt_debug_intersect, pt_debug_motion and pt_lens_focus_at bring for one call.

No test assumes a visiting order.  Only the value the shadow stage WRITES is visible through the hook (the transmission of a committed ray, 1
otherwise); "committed" itself is compared through pt_debug_intersect."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from gltf_renderer_amd import abi, scenes
from tests import hooks
import lens_ref as lr
import traversal_ref as tr
import traversal_scenes as tscenes
from ray_hook import (gpu_intersect, dxr_flags, trace_queues, shadow_rays_of, shadow_counter, TQ_TRACE, TQ_SHADOW, TQ_FUSED, TQ_SENTINEL, CNT_HEAD_CLOSEST,
                      CNT_HEAD_SHADOW, CNT_HEAD_SHADE, RF_CULL_BACK, RF_CULL_FRONT, RF_FORCE_NON_OPAQUE, RF_ACCEPT_FIRST)
from test_traversal_host import check_closest, check_shadow, shadow_value, SHADOW_TMAX, N_RAYS, EPS

pytestmark = pytest.mark.gpu

CULL, IEO, ALPHA = abi.FLAG_CULL_BACKFACE, abi.FLAG_INDIRECT_ENVIRONMENT_ONLY, abi.FLAG_ALPHA_SHADOWS
# flags, bounce, the ray flags launch_wavefront's rule gives the closest rays, their instance mask
CLOSEST_ROWS = [(0, 0, 0, 0xff), (CULL, 0, RF_CULL_BACK, 0xff), (CULL, 1, RF_CULL_FRONT, 0xff), (IEO, 0, 0, 0xff), (IEO, 1, 0, 0), (ALPHA, 0, 0, 0xff)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _geometry_fuzz():
    spec = importlib.util.spec_from_file_location("geometry_fuzz", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "geometry_fuzz.py"))
    gf = importlib.util.module_from_spec(spec); spec.loader.exec_module(gf)
    return gf


class Case:
    """A scene on the product and on the oracle, its rays (tmin = 0: the queue format has none), and the reference answers, computed once."""

    def __init__(self, name, s, rays, oracle_lib, builder=None):
        from gltf_renderer_amd.renderer import Renderer
        self.name, self.s = name, s
        self.r = Renderer(); s.upload(self.r)
        if builder is not None: self.r.set_accel_builder(builder)
        self.o = oracle_lib.Oracle(); s.upload(self.o)
        rays = np.ascontiguousarray(rays, np.float32); rays[:, 3] = 0
        self.rays = rays
        rng = np.random.default_rng(len(rays))
        self.shards = rng.integers(0, 256, len(rays)).astype(np.uint32)
        self._cache = {}

    def reference(self, rf, mode, tmax=None):
        """(traverse() through pt_debug_intersect, the oracle) for the case's rays under ray flags rf."""
        key = (rf, mode, tmax)
        if key not in self._cache:
            rays = self.rays if tmax is None else self.with_tmax(tmax)
            self._cache[key] = (gpu_intersect(self.r, rays, rf, mode), self.o.intersect_many(rays, dxr_flags(rf), mode))
        return self._cache[key]

    def with_tmax(self, tmax):
        rays = self.rays.copy(); rays[:, 7] = tmax
        return rays

    def close(self):
        self.r.close(); self.o.close()


@pytest.fixture(scope="module")
def cases(oracle_lib):
    gf = _geometry_fuzz()
    rng = np.random.default_rng(41)
    out = []
    for builder in range(3):
        s = gf.random_scene(rng)
        o = oracle_lib.Oracle(); s.upload(o)
        rays = gf.random_rays(rng, o, gf.world_triangles(s), 6000); o.close()
        out.append(Case("soup, builder %d" % builder, s, rays, oracle_lib, builder))
    out.append(Case("layered", tscenes.layered_alpha_scene(), tscenes.layered_rays(N_RAYS, 1), oracle_lib))
    yield out
    for c in out: c.close()


@pytest.fixture(scope="module")
def layered_ref(cases):
    c = cases[3]
    return tr.Crossings(tr.Triangles(c.s), c.rays)


def check_counters(cnt, stray, which, bounce, n_closest, n_shadow):
    """After a launch: nothing outside the rays' own records written, the queue counts as they were, each fetch head at least its count, and
    the counters the kernel zeroes for the next shade stage at 0."""
    assert stray[0] == 0 and stray[1] == 0, (which, stray.tolist())
    cur = bounce & 1
    if which in (TQ_TRACE, TQ_FUSED):
        assert np.array_equal(cnt[:, cur], n_closest), which
        assert np.all(cnt[:, CNT_HEAD_CLOSEST] >= n_closest), which
        assert np.all(cnt[:, cur ^ 1] == 0) and np.all(cnt[:, shadow_counter(bounce)] == 0) and np.all(cnt[:, CNT_HEAD_SHADE] == 0), which
    if which in (TQ_SHADOW, TQ_FUSED):
        sb = bounce - 1 if which == TQ_FUSED else bounce
        assert np.array_equal(cnt[:, shadow_counter(sb)], n_shadow), which
        assert np.all(cnt[:, CNT_HEAD_SHADOW] >= n_shadow), which


def per_shard(shards, n):
    return np.bincount(np.broadcast_to(shards, (n,)).astype(np.int64), minlength=256).astype(np.uint32)


def no_sentinel(a):
    return not np.any(bits(a) == TQ_SENTINEL)


# ---- a. closest rays ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which_case", [0, 1, 2, 3], ids=["soup-lbvh", "soup-ploc", "soup-ploc-reinsert", "layered"])
def test_wavefront_driver_finds_what_traverse_and_the_oracle_find_for_every_closest_ray(cases, which_case):
    """Every flags x bounce row through k_wf_trace (and, from bounce 1 on, through the fused k_wf_traverse beside a non-empty shadow queue),
    counters on and off: the seven hit fields bit-identical to pt_debug_intersect with the matching ray flags and to the oracle; under
    INDIRECT_ENVIRONMENT_ONLY at bounce 1 (instance mask 0) every ray misses and every entry is still written; ALPHA_SHADOWS alone (the
    non-DEFAULTS copy) gives the bits of flags 0 (the DEFAULTS copy)."""
    c = cases[which_case]
    n = len(c.rays); counts = per_shard(c.shards, n)
    sh = shadow_rays_of(c.rays[:2000]); sh_shards = c.shards[:2000]
    compared = 0
    results = {}
    for counting in (True, False):
        c.r.enable_counters(counting)
        for flags, bounce, rf, mask in CLOSEST_ROWS:
            g, o = c.reference(rf, 0)
            assert np.array_equal(bits(g[:, :7]), bits(o[:, :7])), (c.name, "traverse() against the oracle", rf)
            expect = g[:, :7].copy()
            if mask == 0: expect[:] = np.float32([0, 0, 0, 0, -1, -1, 0])
            launches = [TQ_TRACE] + ([TQ_FUSED] if bounce >= 1 else [])
            for which in launches:
                h, _, cnt, stray = trace_queues(c.r, c.rays, c.shards, sh if which == TQ_FUSED else None, sh_shards if which == TQ_FUSED else None,
                                                1 if which == TQ_FUSED else None, shadow_tmax=1000.0, flags=flags, bounce=bounce, blocks_per_shard=2, which=which)
                assert no_sentinel(h), (c.name, flags, bounce, which)
                diff = (bits(h[:, :7]) != bits(expect)).any(axis=1)
                assert not diff.any(), (c.name, flags, bounce, which, counting, int(diff.sum()), c.rays[np.nonzero(diff)[0][0]].tolist(), h[np.nonzero(diff)[0][0]].tolist(),
                                        expect[np.nonzero(diff)[0][0]].tolist())
                check_counters(cnt, stray, which, bounce, counts, per_shard(sh_shards, len(sh)))
                results[(counting, flags, bounce, which)] = h
                compared += n
    for key, h in results.items():
        if key[0]: assert np.array_equal(bits(h), bits(results[(False,) + key[1:]])), key                # counters on = counters off
    assert np.array_equal(bits(results[(True, ALPHA, 0, TQ_TRACE)]), bits(results[(True, 0, 0, TQ_TRACE)]))
    hit_share = float(c.reference(0, 0)[0][:, 0].mean())
    assert hit_share > 0.1, hit_share
    print("%s: %d closest-ray queries through the wavefront driver, all bit-identical to traverse() and the oracle (%d rays, %.0f %% hit)" % (c.name, compared, n, 100 * hit_share))


# ---- b. occlusion rays ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which_case", [0, 1, 2, 3], ids=["soup-lbvh", "soup-ploc", "soup-ploc-reinsert", "layered"])
def test_shadow_and_fused_kernels_write_the_oracles_occlusion_for_every_ray(cases, layered_ref, which_case):
    c = cases[which_case]
    n = len(c.rays)
    tmax = float(np.float32(SHADOW_TMAX if c.name == "layered" else np.median(c.rays[:, 7])))
    sh = shadow_rays_of(c.rays)
    rng = np.random.default_rng(7)
    mixed = rng.integers(0, 2, n).astype(np.uint8)
    closest = c.rays[:3000]; cl_shards = c.shards[:3000]

    def run(which, flags, is_light, bounce=0):
        return trace_queues(c.r, closest if which == TQ_FUSED else None, cl_shards if which == TQ_FUSED else None, sh, c.shards, is_light, shadow_tmax=tmax, flags=flags,
                            bounce=bounce + 1 if which == TQ_FUSED else bounce, blocks_per_shard=3, which=which)

    compared = 0
    for which in (TQ_SHADOW, TQ_FUSED):
        # accept-first: 0.0 exactly where the oracle commits a hit, 1.0 exactly where it does not
        for flags, rf in ((0, RF_ACCEPT_FIRST), (CULL, RF_ACCEPT_FIRST | RF_CULL_BACK)):
            g, o = c.reference(rf, 1, tmax)
            assert np.array_equal(g[:, 0], o[:, 0]), (c.name, rf)
            _, v, cnt, stray = run(which, flags, mixed)
            assert np.array_equal(bits(v), bits(np.where(o[:, 0] > 0, np.float32(0), np.float32(1)))), (c.name, which, flags, int((v != np.where(o[:, 0] > 0, 0, 1)).sum()))
            assert stray[0] == 0 and stray[1] == 0
            compared += n
        # alpha shadows, light rays: exactly 0 on exactly the oracle's zero rays, elsewhere within the product-order bound
        for flags, rf in ((ALPHA, RF_FORCE_NON_OPAQUE), (ALPHA | CULL, RF_FORCE_NON_OPAQUE | RF_CULL_BACK)):
            g, o = c.reference(rf, 1, tmax)
            assert np.array_equal(g[:, 0], o[:, 0]), (c.name, rf)                                     # "committed", through traverse()
            ov = shadow_value(o)
            _, v, cnt, stray = run(which, flags, 1)
            assert no_sentinel(v) and stray[0] == 0 and stray[1] == 0
            assert np.array_equal(v == 0, ov == 0), (c.name, which, flags)
            assert np.array_equal(shadow_value(g) == 0, ov == 0), (c.name, flags)
            # both are fp32 products of the same k exact factors in some order: any two orders differ by at most 2 (k - 1) 2^-24 relative.
            # k: the restatement's candidate count; 16 (two triangles of each sheet, a ray along a shared edge) where it is undecided; the
            # soups are opaque (every factor is 0: the values are 0 or 1 exactly)
            if c.name == "layered":
                q = layered_ref.query(rf, 1, tmax=tmax)
                k = np.where(q["undecided"], 16, q["k"])
            else: k = np.ones(n, np.int64)
            bound = 2.0 * np.maximum(k - 1, 0) * EPS * ov.astype(np.float64)
            for name, val in (("wavefront", v), ("traverse()", shadow_value(g))):
                err = np.abs(val.astype(np.float64) - ov)
                assert np.all(err <= bound), (c.name, name, flags, float((err - bound).max()))
            # environment shadow rays never take the alpha path
            _, ve, _, _ = run(which, flags, 0)
            ga, oa = c.reference(RF_ACCEPT_FIRST | (rf & RF_CULL_BACK), 1, tmax)
            assert np.array_equal(bits(ve), bits(np.where(oa[:, 0] > 0, np.float32(0), np.float32(1)))), (c.name, which, flags)
            compared += 2 * n
    # the fused launch = the shadow launch followed by the closest launch, bit for bit
    for flags in (0, CULL | ALPHA):
        _, v1, _, _ = trace_queues(c.r, None, None, sh, c.shards, mixed, shadow_tmax=tmax, flags=flags, bounce=0, blocks_per_shard=3, which=TQ_SHADOW)
        h1, _, _, _ = trace_queues(c.r, closest, cl_shards, None, None, None, shadow_tmax=tmax, flags=flags, bounce=1, blocks_per_shard=3, which=TQ_TRACE)
        h2, v2, cnt, stray = trace_queues(c.r, closest, cl_shards, sh, c.shards, mixed, shadow_tmax=tmax, flags=flags, bounce=1, blocks_per_shard=3, which=TQ_FUSED)
        assert np.array_equal(bits(h1), bits(h2)) and np.array_equal(bits(v1), bits(v2)), (c.name, flags)
        check_counters(cnt, stray, TQ_FUSED, 1, per_shard(cl_shards, len(closest)), per_shard(c.shards, n))
    print("%s: %d occlusion-ray queries through k_wf_shadow and k_wf_traverse compared with the oracle" % (c.name, compared))


def test_mask_sheets_occlude_accept_first_rays_through_their_cut_outs_in_both_drivers(cases, layered_ref):
    c = cases[3]
    closest = layered_ref.query(0, 0); occl = layered_ref.query(RF_ACCEPT_FIRST, 1, tmax=100.0)
    through = ~closest["committed"] & occl["committed"] & ~closest["undecided"]
    assert through.sum() >= 50
    g, o = c.reference(RF_ACCEPT_FIRST, 1, 100.0)
    _, v, _, _ = trace_queues(c.r, None, None, shadow_rays_of(c.rays), c.shards, 1, shadow_tmax=100.0, flags=0, bounce=0, blocks_per_shard=1, which=TQ_SHADOW)
    assert np.all(g[through, 0] > 0) and np.all(o[through, 0] > 0) and np.all(v[through] == 0.0)


# ---- c. the any-hit paths of both drivers against the float64 restatement -------------------------------------------------------------------
def test_any_hit_paths_of_both_drivers_agree_with_the_float64_restatement(cases, layered_ref):
    """Layered scene, decided rays.  Closest hits with and without RF_FORCE_NON_OPAQUE under each culling flag through traverse() (no frame
    gives closest rays the forced any-hit, so the wavefront kernels cannot be asked for it) and, for the flag sets a frame produces, through
    k_wf_trace; accept-first and alpha-shadow rays through traverse() and k_wf_shadow."""
    c = cases[3]; X = layered_ref
    n_cmp = n_und = 0
    for cull in (0, RF_CULL_BACK, RF_CULL_FRONT):
        for fno in (0, RF_FORCE_NON_OPAQUE):
            ref = X.query(cull | fno, 0)
            a, b = check_closest(("traverse()", cull | fno), c.reference(cull | fno, 0)[0], ref); n_cmp += a; n_und = max(n_und, b)
        flags, bounce = {0: (0, 0), RF_CULL_BACK: (CULL, 0), RF_CULL_FRONT: (CULL, 1)}[cull]
        h, _, _, _ = trace_queues(c.r, c.rays, c.shards, flags=flags, bounce=bounce, blocks_per_shard=2, which=TQ_TRACE)
        a, b = check_closest(("k_wf_trace", cull), h, X.query(cull, 0)); n_cmp += a
    sh = shadow_rays_of(c.rays)
    for flags, rf in ((0, RF_ACCEPT_FIRST), (CULL, RF_ACCEPT_FIRST | RF_CULL_BACK), (ALPHA, RF_FORCE_NON_OPAQUE), (ALPHA | CULL, RF_FORCE_NON_OPAQUE | RF_CULL_BACK)):
        ref = X.query(rf, 1, tmax=SHADOW_TMAX)
        g = c.reference(rf, 1, SHADOW_TMAX)[0]
        a, b = check_shadow(("traverse()", rf), g[:, 0] > 0, shadow_value(g), ref); n_cmp += a; n_und = max(n_und, b)
        _, v, _, _ = trace_queues(c.r, None, None, sh, c.shards, 1, shadow_tmax=SHADOW_TMAX, flags=flags, bounce=0, blocks_per_shard=2, which=TQ_SHADOW)
        a, b = check_shadow(("k_wf_shadow", rf), g[:, 0] > 0, v, ref); n_cmp += a
    assert n_und <= 0.02 * len(c.rays)
    print("layered scene: %d ray queries of both drivers compared with the float64 restatement, at most %d of %d rays undecided" % (n_cmp, n_und, len(c.rays)))


def test_alpha_shadows_through_linear_filtered_alpha_agree_with_the_oracle(oracle_lib):
    """scenes.test_scene: a MASK cut-out, a BLEND quad and LINEAR-filtered alpha.  Both drivers and the oracle agree on "committed" and on the
    zeros; the transmission is within 2 k RGBA_TOL + 2 (k - 1) 2^-24 of the oracle's: a product of k factors in [0, 1] moves by at most the sum
    of its factors' errors (the sampler's tolerance, for either side), plus the order of the fp32 products.  k = the float64 crossing count
    of the ray (the scene's layer count for an undecided ray)."""
    from test_gpu_texture import RGBA_TOL
    from ray_hook import surface_rays
    s = scenes.test_scene(64, 32)
    o0 = oracle_lib.Oracle(); s.upload(o0)
    rays = np.concatenate(surface_rays(o0, s, 3000, 5) + (tscenes.alpha_aimed_rays(s, 3000, 6),)); o0.close()
    c = Case("test_scene", s, rays, oracle_lib)
    tmax = 1000.0
    X = tr.Crossings(tr.Triangles(s), c.with_tmax(tmax), with_alpha=False)
    k = np.where(X.fuzzy, 16, X.count(tmax))
    bound = 2.0 * k * RGBA_TOL + 2.0 * np.maximum(k - 1, 0) * EPS
    sh = shadow_rays_of(c.rays)
    for flags, rf in ((ALPHA, RF_FORCE_NON_OPAQUE), (ALPHA | CULL, RF_FORCE_NON_OPAQUE | RF_CULL_BACK)):
        g, o = c.reference(rf, 1, tmax)
        assert np.array_equal(g[:, 0], o[:, 0]), rf
        ov = shadow_value(o)
        _, v, _, stray = trace_queues(c.r, None, None, sh, c.shards, 1, shadow_tmax=tmax, flags=flags, bounce=0, blocks_per_shard=2, which=TQ_SHADOW)
        assert stray[0] == 0 and stray[1] == 0
        for name, val in (("wavefront", v), ("traverse()", shadow_value(g))):
            assert np.array_equal(val == 0, ov == 0), (name, rf)
            err = np.abs(val.astype(np.float64) - ov)
            print("test_scene alpha shadows, %s, ray flags %d: max |transmission - oracle| %.3g (bound %.3g .. %.3g), %d rays strictly between 0 and 1"
                  % (name, rf, err.max(), bound.min(), bound.max(), int(((ov > 0) & (ov < 1)).sum())))
            assert np.all(err <= bound), (name, rf, float(err.max()))
        assert ((ov > 0) & (ov < 1)).sum() >= 100
    c.close()


# ---- d. queue shapes --------------------------------------------------------------------------------------------------------------------------
SHARD_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000]


@pytest.mark.parametrize("bps", [1, 2, 3, 6])
def test_queue_shapes_around_the_wave_refill_and_workgroup_sizes(cases, bps):
    """Counts per shard around the refill threshold (32), the wave (64) and the workgroup (256), alone in one shard, one ray in each of the 256
    shards, the twelve counts dealt over twelve shards, and no ray at all -- through k_wf_trace, k_wf_shadow and the fused kernel at each
    blocks_per_shard a frame uses.  Every entry below a shard's count is written with what pt_debug_intersect finds for that ray, nothing else
    is (guard entries, entries at or above the count, the other words of the pending records), and the counters are left as documented."""
    c = cases[0]
    tmax = float(np.float32(np.median(c.rays[:, 7])))
    g0 = c.reference(0, 0)[0]; g1 = c.reference(RF_ACCEPT_FIRST, 1, tmax)[0]
    occ = np.where(g1[:, 0] > 0, np.float32(0), np.float32(1))
    shapes = [("%d rays in shard 37" % k, np.full(k, 37, np.uint32)) for k in SHARD_COUNTS if k]
    shapes.append(("one ray in each shard", np.arange(256, dtype=np.uint32)))
    shapes.append(("the counts dealt over 12 shards", np.concatenate([np.full(k, 20 * j + 3, np.uint32) for j, k in enumerate(SHARD_COUNTS)])))
    shapes.append(("all shards empty", np.zeros(0, np.uint32)))
    rng = np.random.default_rng(bps)
    for name, shards in shapes:
        m = len(shards)
        pick = rng.permutation(len(c.rays))[:m]
        shards = shards[rng.permutation(m)] if m else shards              # the caller's order within a shard is the queue's; shards interleave
        cl = c.rays[pick]; sh = shadow_rays_of(c.rays[pick]); counts = per_shard(shards, m)
        for which in (TQ_TRACE, TQ_SHADOW, TQ_FUSED):
            bounce = 1 if which == TQ_FUSED else 0
            h, v, cnt, stray = trace_queues(c.r, cl if which != TQ_SHADOW else None, shards if which != TQ_SHADOW else None, sh if which != TQ_TRACE else None,
                                            shards if which != TQ_TRACE else None, 1, shadow_tmax=tmax, flags=0, bounce=bounce, blocks_per_shard=bps, which=which)
            if which != TQ_SHADOW:
                assert no_sentinel(h), (name, which)
                assert np.array_equal(bits(h[:, :7]), bits(g0[pick, :7])), (name, which, bps)
            if which != TQ_TRACE:
                assert no_sentinel(v), (name, which)
                assert np.array_equal(bits(v), bits(occ[pick])), (name, which, bps)
            zero = np.zeros(256, np.uint32)
            check_counters(cnt, stray, which, bounce, counts if which != TQ_SHADOW else zero, counts if which != TQ_TRACE else zero)


# ---- e. the deep stack under the stage grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [1, 6])
def test_deep_stack_columns_serve_several_rays_in_a_row(bps):
    """The deep-chain scene with the LBVH builder (a tree deeper than the on-chip stack): 4096 rays along +x from the scene's orthographic
    frustum, all in one shard and dealt over the 256 shards.  A lane then traces several rays in a row on the deep-stack column of its place
    in the stage grid (sc.deep_lanes = the grid's lanes, not the ray count).  Bit-identical to pt_debug_intersect, deep entries really
    written, no push dropped."""
    from gltf_renderer_amd.renderer import Renderer
    s, n_tris = tscenes._deep_chain_scene()
    r = Renderer(); r.set_accel_builder(abi.BUILDER_LBVH); s.upload(r)
    half = 1.0 / s.ortho[0]
    rng = np.random.default_rng(3)
    n = 4096
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0] = -0.5; rays[:, 1:3] = rng.uniform(-half, half, (n, 2)); rays[:, 4] = 1.0; rays[:, 7] = 1000.0
    g = gpu_intersect(r, rays, 0, 0)
    assert np.all(g[:, 0] > 0)                                           # every ray hits the nearest sheet
    ga = gpu_intersect(r, rays, RF_ACCEPT_FIRST, 1)
    for name, shards in (("one shard", np.zeros(n, np.uint32)), ("256 shards", (np.arange(n) % 256).astype(np.uint32))):
        r.reset_stats()
        h, _, cnt, stray = trace_queues(r, rays, shards, flags=0, bounce=0, blocks_per_shard=bps, which=TQ_TRACE)
        assert np.array_equal(bits(h[:, :7]), bits(g[:, :7])), (name, bps)
        check_counters(cnt, stray, TQ_TRACE, 0, per_shard(shards, n), np.zeros(256, np.uint32))
        q = r.stats()                                                    # raises if a push was dropped
        assert q.bvh_stack_need > 64 and q.deep_stack_pushes > 0, (name, q.bvh_stack_need, q.deep_stack_pushes)
        _, v, _, stray = trace_queues(r, None, None, shadow_rays_of(rays), shards, 1, shadow_tmax=1000.0, flags=0, bounce=0, blocks_per_shard=bps, which=TQ_SHADOW)
        assert np.array_equal(v, np.where(ga[:, 0] > 0, np.float32(0), np.float32(1))) and stray[0] == 0 and stray[1] == 0
        r.stats()
        print("deep chain, %s, %d workgroups per shard: stack need %d, deep pushes %d" % (name, bps, q.bvh_stack_need, q.deep_stack_pushes))
    r.close()


def _params_hook(r, name, st, params, rows, width):
    """pt_debug_camera_rays (rows [n, 3] uint32 {px, py, seed}) or pt_debug_motion (rows [n, 8] float32 rays): -> [n, 8] float32."""
    rows = np.ascontiguousarray(rows).reshape(-1, width)
    out = np.zeros((len(rows), 8), np.float32)
    f = getattr(hooks.lib(), name)
    rc = f(r.h, C.byref(st), C.byref(params), rows.ctypes.data_as(C.c_void_p), len(rows), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (name, rc, r.L.pt_last_error(r.h))
    return out


def test_every_one_call_deep_stack_serves_a_tree_that_needs_it(oracle_lib):
    """pt_debug_intersect, pt_debug_motion and pt_lens_focus_at each bring a deep stack of their own for one call, through one helper
    (pt_ctx.h temp_deep_stack).  The deep-chain scene with the LBVH builder needs one: its stack need is above the 64 entries a lane
    holds on chip.  On the camera rays of 16 pixels (pt_debug_camera_rays, lens off, seed 0):
      a. pt_debug_motion's instance, primitive, u, v (out[4:8]) are pt_debug_intersect's (mode 0), bit for bit;
      b. focus_at at the ray's image position is the view-space depth zo + t * dn of that hook hit (float64, t the hook's), within
         tests/lens_ref.py's bound -- as test_focus_at_is_the_view_space_depth_of_the_hooks_ray (tests/test_gpu_lens.py) computes it."""
    from gltf_renderer_amd.renderer import Renderer
    s, n_tris = tscenes._deep_chain_scene()
    W, H = s.width, s.height
    assert (W, H) == (32, 32)
    r = Renderer(); r.set_accel_builder(abi.BUILDER_LBVH); s.upload(r); r.build_accel()
    q = r.stats()
    deep = q.bvh_stack_capacity - 64                                     # the entries beyond the on-chip ones
    assert deep > 0 and q.bvh_stack_need > q.bvh_stack_capacity - deep, (q.bvh_stack_need, q.bvh_stack_capacity)
    st, params = s.settings, s.execute_params(0)
    rf = RF_CULL_BACK if st.flags & CULL else 0
    picks = [(x, y) for y in (3, 11, 19, 27) for x in (2, 10, 18, 26)]
    r.set_lens(0, 1, enable=False)
    rays = _params_hook(r, "pt_debug_camera_rays", st, params, np.array([(x, y, 0) for x, y in picks], np.uint32), 3)
    g = gpu_intersect(r, rays, rf, 0)
    assert np.all(g[:, 0] > 0) and np.all(g[:, 1] > 0)                   # every ray hits the nearest sheet
    m = _params_hook(r, "pt_debug_motion", st, params, rays, 8)
    assert np.array_equal(bits(m[:, 4:8]), bits(g[:, [4, 5, 2, 3]])), (m[:, 4:8], g[:, [4, 5, 2, 3]])
    cam = lr.Camera(params.world_to_view, params.view_to_clip, W, H)
    sx, sy = lr.jittered(lr.randoms(oracle_lib, W, H, range(1)), W, H)
    for k, (x, y) in enumerate(picks):
        got = r.focus_at(st, params, float(sx[0, y, x]), float(sy[0, y, x]))
        assert got is not None, (x, y)
        od, dd = rays[k, 0:3].astype(np.float64), rays[k, 4:7].astype(np.float64)
        zo, dn = float((od - cam.c) @ cam.F), float(dd @ cam.F)
        want = zo + float(g[k, 1]) * dn
        P = od + dd * float(g[k, 1])
        print("pixel (%d, %d): focus_at %.9g, zo + t dn %.9g" % (x, y, got, want))
        assert abs(got - want) <= float(lr.bound(od[None], cam.c[None], P[None], want)[0]), (x, y, got, want)
    r.stats()                                                            # raises if a push was dropped
    r.close()


# ---- the hook leaves the context alone ---------------------------------------------------------------------------------------------------------
def test_a_hook_call_between_traces_changes_no_bit_of_an_accumulation():
    """Two accumulating frames, pt_set_lens (a pending restart), then two more frames: the same bits with and without a pt_debug_trace_queues
    call (closest and shadow rays, fused) in the middle -- the hook owns its buffers and leaves the accumulation, the workspace and the
    pending restart as they are."""
    from gltf_renderer_amd.renderer import Renderer
    s = scenes.test_scene(32, 16, with_env=False)
    rays = tscenes.alpha_aimed_rays(s, 2000, 9)
    imgs = []
    for with_hook in (False, True):
        r = Renderer(); s.upload(r)
        st = abi.PtSettings.from_buffer_copy(bytes(s.settings)); st.reset = 1
        out = r.create_output(s.width, s.height)
        for f in range(2):
            r.trace(st, s.execute_params(f), out); st.reset = 0
        r.set_lens(0.02, 3.0)
        if with_hook:
            h, v, cnt, stray = trace_queues(r, rays, 5, shadow_rays_of(rays), 9, 1, shadow_tmax=1000.0, flags=ALPHA, bounce=1, blocks_per_shard=2, which=TQ_FUSED)
            assert no_sentinel(h) and no_sentinel(v) and stray[0] == 0 and stray[1] == 0
        mid = r.readback(out).copy()
        for f in range(2, 4):
            r.trace(st, s.execute_params(f), out)
        imgs.append((mid, r.readback(out).copy()))
        r.close()
    assert np.array_equal(bits(imgs[0][0]), bits(imgs[1][0])) and np.array_equal(bits(imgs[0][1]), bits(imgs[1][1]))
    assert not np.array_equal(imgs[0][0], imgs[0][1])
