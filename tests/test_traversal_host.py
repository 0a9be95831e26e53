"""Host-side traversal tests (no GPU): the CPU oracle's any-hit paths against the float64 restatement of the rules (tests/traversal_ref.py) on
the layered alpha scene, the oracle's tree against its own exhaustive search under RAY_FLAG_FORCE_NON_OPAQUE, and the argument checks of the
pt_debug_trace_queues test hook.  The scene and ray recipe checked here are the ones tests/test_gpu_traversal_driver.py sends through the
product's two traversal drivers."""
import numpy as np
import pytest

import traversal_ref as tr
import traversal_scenes as tscenes
from ray_hook import dxr_flags, trace_queues_rc, RF_CULL_BACK, RF_CULL_FRONT, RF_FORCE_NON_OPAQUE, RF_ACCEPT_FIRST

N_RAYS = 12000
SHADOW_TMAX = 3.0          # shorter than the stack is tall: the interval's end lies between sheets for many rays
EPS = 2.0 ** -24

# (ray flags, mode): closest hits with and without the forced any-hit under each culling flag; accept-first occlusion; alpha shadows
CLOSEST_CASES = [(c | f, 0) for f in (0, RF_FORCE_NON_OPAQUE) for c in (0, RF_CULL_BACK, RF_CULL_FRONT)]
SHADOW_CASES = [(RF_ACCEPT_FIRST, 1), (RF_ACCEPT_FIRST | RF_CULL_BACK, 1), (RF_FORCE_NON_OPAQUE, 1), (RF_FORCE_NON_OPAQUE | RF_CULL_BACK, 1)]


@pytest.fixture(scope="module")
def layered():
    s = tscenes.layered_alpha_scene()
    rays = tscenes.layered_rays(N_RAYS, 1)
    return s, rays, tr.Crossings(tr.Triangles(s), rays)


@pytest.fixture(scope="module")
def layered_oracle(oracle_lib, layered):
    o = oracle_lib.Oracle(); layered[0].upload(o)
    yield o
    o.close()


def check_closest(name, got, ref):
    """got [n, 8] (committed, t, u, v, instance, primitive, front, -) against the restatement's closest hit, decided rays only: the same
    triangle and facing; t within MARGIN relative, u and v within MARGIN absolute (the restatement's own margin, not a precision claim)."""
    ok = ~ref["undecided"]
    assert np.array_equal(got[ok, 0] > 0, ref["committed"][ok]), (name, int(((got[:, 0] > 0) != ref["committed"])[ok].sum()))
    for col, key in ((4, "instance"), (5, "primitive")):
        bad = ok & (got[:, col].astype(np.int64) != ref[key])
        assert not bad.any(), (name, key, int(bad.sum()), int(np.nonzero(bad)[0][0]))
    assert np.array_equal(got[ok, 6] > 0, ref["front"][ok]), name
    hit = ok & ref["committed"]
    assert np.all(np.abs(got[hit, 1] - ref["t"][hit]) <= tr.MARGIN * ref["t"][hit]), name
    assert np.all(np.abs(got[hit, 2] - ref["u"][hit]) <= tr.MARGIN) and np.all(np.abs(got[hit, 3] - ref["v"][hit]) <= tr.MARGIN), name
    return int(ok.sum()), int((~ok).sum())


def check_shadow(name, committed, value, ref):
    """committed [n] bool and value [n] (what the shadow stage writes: the transmission of a committed ray, 1 otherwise) against the
    restatement, decided rays only: the same rays commit, exactly the same rays are 0, and elsewhere the value is within
    2 (k - 1) 2^-24 relative of the float64 product of the k exact fp32 factors (each fp32 multiply rounds once)."""
    ok = ~ref["undecided"]
    assert np.array_equal(committed[ok], ref["committed"][ok]), (name, int((committed != ref["committed"])[ok].sum()))
    expect = np.where(ref["committed"], ref["transmission"], 1.0)
    assert np.array_equal(value[ok] == 0.0, expect[ok] == 0.0), (name, int(((value == 0.0) != (expect == 0.0))[ok].sum()))
    bound = 2.0 * np.maximum(ref["k"] - 1, 0) * EPS * expect
    err = np.abs(value.astype(np.float64) - expect)
    assert np.all(err[ok] <= bound[ok]), (name, float((err - bound)[ok].max()), int(np.nonzero(ok & (err > bound))[0][0]))
    return int(ok.sum()), int((~ok).sum())


def shadow_value(h):
    """What the shadow stage stores for an intersect_many / pt_debug_intersect row: ShadowMiss sets the payload to 1."""
    return np.where(h[:, 0] > 0, h[:, 7], np.float32(1.0))


def test_the_layered_scene_and_its_rays_are_what_the_tests_need(layered):
    """At most 2 % of the rays undecided in every mode, at least 20 % cross three or more sheets, at least 5 % of the alpha-shadow rays end at
    exactly 0 -- and a good share of them ends strictly between 0 and 1 with several factors."""
    s, rays, X = layered
    assert s.triangles == 256 and len(s.instances) == 8
    for rf, mode in CLOSEST_CASES + SHADOW_CASES:
        q = X.query(rf, mode, tmax=SHADOW_TMAX if mode else None)
        assert q["undecided"].mean() <= 0.02, (rf, mode, float(q["undecided"].mean()))
    q = X.query(0, 0)
    assert (q["k"] >= 3).mean() >= 0.20, float((q["k"] >= 3).mean())
    a = X.query(RF_FORCE_NON_OPAQUE, 1, tmax=SHADOW_TMAX)
    assert a["zero"].mean() >= 0.05, float(a["zero"].mean())
    partial = (a["transmission"] > 0) & (a["transmission"] < 1)
    assert partial.mean() >= 0.05 and (partial & (a["k"] >= 3)).sum() >= 100, (float(partial.mean()), int((partial & (a["k"] >= 3)).sum()))
    assert a["k"].max() <= 8
    alphas = np.unique(X.alpha)
    assert 0.0 in alphas and 1.0 in alphas and alphas[alphas < 1].max() <= 0.99                # exactly 0, exactly 1, otherwise at most 0.99
    base = np.unique(X.base)
    assert np.float32(127) / np.float32(255) in base and np.float32(128) / np.float32(255) in base      # the texels either side of the 0.5 cutoff


@pytest.mark.parametrize("rf,mode", CLOSEST_CASES + SHADOW_CASES)
def test_oracle_any_hit_paths_agree_with_the_float64_restatement(layered, layered_oracle, rf, mode):
    s, rays, X = layered
    r = rays.copy()
    if mode: r[:, 7] = SHADOW_TMAX
    h = layered_oracle.intersect_many(r, dxr_flags(rf), mode)
    ref = X.query(rf, mode, tmax=SHADOW_TMAX if mode else None)
    if mode == 0: n, und = check_closest((rf, mode), h, ref)
    else: n, und = check_shadow((rf, mode), h[:, 0] > 0, shadow_value(h), ref)
    print("oracle vs float64 restatement, flags %d mode %d: %d rays compared, %d undecided" % (rf, mode, n, und))


def test_mask_sheets_occlude_accept_first_rays_even_through_their_cut_outs(layered, layered_oracle):
    """0 * (1 - a) == 0: an accept-first ray that meets only an ignored-in-closest-mode MASK texel is still occluded."""
    s, rays, X = layered
    closest = X.query(0, 0); occl = X.query(RF_ACCEPT_FIRST, 1, tmax=100.0)
    through = ~closest["committed"] & occl["committed"] & ~closest["undecided"]
    assert through.sum() >= 50, int(through.sum())                         # rays whose every crossing is a cut-out
    h = layered_oracle.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1)
    assert np.all(h[through, 0] > 0) and np.all(shadow_value(h)[through] == 0.0)


@pytest.mark.parametrize("scene", ["layered", "test_scene"])
def test_oracle_tree_equals_its_exhaustive_search_under_force_non_opaque(oracle_lib, layered, scene):
    """RAY_FLAG_FORCE_NON_OPAQUE in both modes: the same rays commit, the same rays are exactly 0, closest hits are bit-identical, and the
    transmission is within the product-order bound 2 (k - 1) 2^-24 relative, k = the most crossings any ray of the set has (+ 1)."""
    if scene == "layered":
        s, rays, X = layered
        kmax = int(X.query(RF_FORCE_NON_OPAQUE, 1)["k"].max()) + 1
    else:
        from gltf_renderer_amd import scenes
        from ray_hook import surface_rays
        s = scenes.test_scene(64, 32)
        o0 = oracle_lib.Oracle(); s.upload(o0)
        rays = np.concatenate(surface_rays(o0, s, 3000, 5) + (tscenes.alpha_aimed_rays(s, 3000, 6),)); o0.close()
        kmax = 16                                                         # floor, wall, 5 spheres x 2, the two quads, the triangle, the box x 2: never all on one line
    o = oracle_lib.Oracle(); s.upload(o)
    for mode in (0, 1):
        a = o.intersect_many(rays, dxr_flags(RF_FORCE_NON_OPAQUE), mode)
        o.set_brute_force(True); b = o.intersect_many(rays, dxr_flags(RF_FORCE_NON_OPAQUE), mode); o.set_brute_force(False)
        assert np.array_equal(a[:, 0], b[:, 0]), (scene, mode)
        if mode == 0: assert np.array_equal(a[:, :7].view(np.uint32), b[:, :7].view(np.uint32)), scene
        else:
            assert np.array_equal(a[:, 7] == 0, b[:, 7] == 0), scene
            assert np.all(np.abs(a[:, 7].astype(np.float64) - b[:, 7]) <= 2.0 * (kmax - 1) * EPS * b[:, 7]), scene
            assert ((a[:, 7] > 0) & (a[:, 7] < 1)).sum() >= 20, scene     # the product path was taken
    o.close()


def test_trace_queues_hook_refuses_bad_arguments_without_a_context():
    """pt_debug_trace_queues answers PT_ERR_INVALID_ARGUMENT -- before it touches a device or dereferences the context -- for a shard above 255,
    a closest ray with tmin != 0, blocks_per_shard < 1, `which` outside 0..2, a fused launch at bounce 0, and for a NULL context."""
    ray = np.array([[0, 0, 1, 0, 0, 0, -1, 10]], np.float32); sh = np.array([[0, 0, 1, 0, 0, -1]], np.float32)
    call = lambda **kw: trace_queues_rc(None, **{**dict(closest=ray, closest_shard=0, shadow=sh, shadow_shard=0, is_light=1, shadow_tmax=10.0, flags=0, bounce=1,
                                                            blocks_per_shard=1, which=0), **kw})[0]
    bad = -1                                                               # PT_ERR_INVALID_ARGUMENT (include/mipt.h)
    tmin = ray.copy(); tmin[0, 3] = 1e-3
    for kw in (dict(closest_shard=256), dict(shadow_shard=256), dict(closest=tmin), dict(blocks_per_shard=0), dict(which=3), dict(which=-1),
               dict(which=2, bounce=0), dict(bounce=-1), dict()):
        assert call(**kw) == bad, kw
