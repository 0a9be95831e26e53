"""The quantised wide node (csrc/pt_types.h Bvh4Node) and its slab test (csrc/pt_traverse.h trav_node_step) at the smallest shapes at which
the node encoding or the choice of near / far planes by the sign of the ray's inverse direction can go wrong: step exponents 2^33 apart in
one tree, small triangles far from the coordinate origin under a wide root, flat and tiny trees, vertices on exact powers of two and on the
root's corners, direction components exactly +0 and -0, rays that start on box planes, and a root that moves from refit to refit.  On each
the product's traversal (pt_debug_intersect) must find the oracle's hit for every ray -- same triangle, bit-identical t, u, v; for
accept-first occlusion rays the same occluded / not occluded -- and the oracle's tree must agree with its own exhaustive search over every
triangle.  (The scenes were written for a 48-byte node payload with a per-tree origin grid and 5-bit step exponents, which was measured and
not kept, profiles/EXPERIMENTS.md; they are the shapes any change of the node format has to survive.)

The scenes have no coplanar overlapping surfaces, so no two triangles are hit at exactly the same distance except along a shared edge, where
both sides apply the same rule (the lower (instance, primitive) wins; tests/test_gpu_round3.py covers that rule on its own).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gltf_renderer_amd import meshgen, scenes  # noqa: E402

f32 = np.float32
N_RAYS = 12_000          # aimed rays per scene; with the rays cast from their hit points, 20-50 k rays per scene
N_BRUTE = 3_000


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def _scene(name, meshes):
    s = scenes.SceneData(name)
    for m in meshes:
        s.add_mesh(m, None, 0)
    tris = np.concatenate([m.positions[m.indices.reshape(-1, 3)] for m in meshes]).astype(np.float64)
    return s, tris


def _unit(rng, k):
    d = rng.standard_normal((k, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _aimed(rng, tris, n, reach):
    """n rays aimed at random points of `tris` from a distance of reach * 10^-2..0 in a random direction."""
    t = tris[rng.integers(0, len(tris), n)]
    w = rng.dirichlet((1, 1, 1), n)
    p = (t * w[:, :, None]).sum(axis=1)
    d = _unit(rng, n)
    dist = reach * 10.0 ** rng.uniform(-2, 0, n)
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3] = p + d * dist[:, None]
    rays[:, 4:7] = -d
    rays[:, 7] = 4 * reach + 1
    return rays


def _from_hits(rng, o, first, reach):
    """Rays as the path tracer casts them from the points `first` hits: random, along a world axis (two direction components exactly zero,
    of either sign, from an origin moved off the surface), grazing; long and short."""
    h = o.intersect_many(first)
    hit = h[:, 0] > 0
    origin = (first[hit, 0:3] + h[hit, 1:2] * first[hit, 4:7]).astype(f32)
    m = len(origin)
    d = _unit(rng, m).astype(f32)
    kind = rng.integers(0, 4, m)
    axis = np.eye(3, dtype=f32)[rng.integers(0, 3, m)] * rng.choice(f32([-1, 1]), m)[:, None]
    axis = np.where(axis == 0, rng.choice(f32([0.0, -0.0]), (m, 3)), axis)
    d[kind == 1] = axis[kind == 1]
    origin[kind == 1] += ((rng.random((int((kind == 1).sum()), 3)) - 0.5) * 2e-3 * reach).astype(f32)
    d[kind == 2] = d[kind == 2] * f32([1, 0.02, 1]); d[kind == 2] /= np.linalg.norm(d[kind == 2], axis=1, keepdims=True)
    second = np.zeros((m, 8), f32); second[:, 0:3] = origin; second[:, 4:7] = d
    second[:, 7] = np.where(rng.random(m) < 0.25, rng.random(m) * 0.5 * reach, 4 * reach + 1).astype(f32)
    return second


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
def _exponent_window():
    """A quad pair of extent 1e5 and 288 triangles of size 1e-5 near the coordinate origin: the root's step is about 2^9, a node over a few
    of the small triangles wants about 2^-25: step exponents 2^33 apart in one tree."""
    big = meshgen.grid(1, 1, (-5e4, -5e4, -1.0), (1e5, 0, 0), (0, 1e5, 0))
    small = meshgen.grid(12, 12, (1e-3, 2e-3, 5e-4), (1.2e-4, 0, 0), (0, 1.2e-4, 3e-5))
    s, tris = _scene("node_format_exponent_window", [big, small])
    return s, [(tris[:2], 1e5), (tris[2:], 1e-3), (tris[2:], 1.0)]


def _origin_slack():
    """2048 triangles of 2e-3 and a small box near (5e3, -7e3, 9e3), and a sphere of radius 300 two thousand units away: the root is ~8e3 wide,
    a float32 ulp there (5e-4 .. 1e-3) is half a small triangle, and the top of the tree is a million times wider than its leaves."""
    c = np.array([5e3, -7e3, 9e3])
    patch = meshgen.grid(32, 32, c, (0.064, 0, 0.008), (0, 0.064, 0.004))
    box = meshgen.box(c + (0.01, 0.012, 0.05), c + (0.03, 0.03, 0.07))
    far = meshgen.uv_sphere(24, 16, 300.0, (3e3, -5e3, 7.5e3))
    s, tris = _scene("node_format_origin_slack", [patch, box, far])
    n0, n1 = patch.num_indices // 3, box.num_indices // 3
    return s, [(tris[:n0 + n1], 0.2), (tris[:n0 + n1], 5.0), (tris[n0 + n1:], 2e3)]


def _single_triangle():
    m = meshgen.Mesh(np.array([[-1, 0.25, -1], [1, 0.5, -1], [0, 0, 1]], f32), np.array([0, 1, 2]), normals=np.array([[0, -1, 0]] * 3, f32))
    s, tris = _scene("node_format_single_triangle", [m])
    return s, [(tris, 3.0)]


def _two_triangles():
    """The root has two children, both leaves."""
    m = meshgen.Mesh(np.array([[-1, 0.25, -1], [1, 0.5, -1], [0, 0, 1], [2, 3, 0.5], [3, 3.5, 0.25], [2.5, 2, 1.5]], f32), np.array([0, 1, 2, 3, 4, 5]),
                     normals=np.array([[0, -1, 0]] * 6, f32))
    s, tris = _scene("node_format_two_triangles", [m])
    return s, [(tris, 3.0)]


def _flat(axis):
    """An axis-aligned plane of zero thickness: the root box, and every box below it, has extent 0 on `axis`."""
    e = np.eye(3)
    u, v = e[(axis + 1) % 3], e[(axis + 2) % 3]
    m = meshgen.grid(9, 7, 0.375 * e[axis] - 2 * u - 1.5 * v, 4 * u, 3 * v)
    s, tris = _scene("node_format_flat_%s" % "xyz"[axis], [m])
    return s, [(tris, 3.0)]


def _grid_edges():
    """Five planes z = 1, 2, 4, 8, 16 over [-16, 16]^2 with vertices on multiples of 4: vertices on exact powers of two, on the root's lower
    corner (-16, -16, 1) and on its upper corner (16, 16, 16), i.e. on the first and the last plane a node can say."""
    planes = [meshgen.grid(8, 8, (-16, -16, z), (32, 0, 0), (0, 32, 0)) for z in (1.0, 2.0, 4.0, 8.0, 16.0)]
    s, tris = _scene("node_format_grid_edges", planes)
    return s, [(tris, 40.0)]


def _grid_edge_rays(rng, n):
    """Rays of the grid-edge scene with direction components exactly +0 and -0, and rays that start ON box planes: on the planes z = 1 .. 16
    themselves (a triangle at distance 0 is not a hit: t > tmin), on the root's side planes x = -16 and y = 16, on its corners' planes."""
    k = n // 4
    rays = np.zeros((4 * k, 8), f32); rays[:, 7] = 100.0
    zero = lambda m: rng.choice(f32([0.0, -0.0]), m)
    xy = lambda m: (rng.random((m, 2)) * 31 - 15.5 + rng.random((m, 2)) * 1e-3).astype(f32)
    a = rays[:k]; a[:, 0:2] = xy(k); a[:, 2] = rng.choice(f32([-3, 0.5, 3, 5, 12, 20]), k); a[:, 4] = zero(k); a[:, 5] = zero(k); a[:, 6] = rng.choice(f32([-1, 1]), k)
    b = rays[k:2 * k]; b[:, 0:2] = xy(k); b[:, 2] = rng.choice(f32([1, 2, 4, 8, 16]), k); b[:, 4:7] = _unit(rng, k); b[: k // 2, 4] = zero(k // 2); b[: k // 2, 5] = zero(k // 2)
    c = rays[2 * k:3 * k]; c[:, 0] = -16.0; c[:, 1] = xy(k)[:, 0]; c[:, 2] = rng.choice(f32([-3, 0.5, 20]), k); c[:, 4] = zero(k); c[:, 5] = zero(k); c[:, 6] = np.where(c[:, 2] > 16, -1, 1)
    d = rays[3 * k:]; d[:, 0] = xy(k)[:, 0]; d[:, 1] = 16.0; d[:, 2] = rng.random(k).astype(f32) * 20 - 2; d[:, 4:7] = _unit(rng, k); d[:, 5] = -np.abs(d[:, 5])
    return rays


SCENES = {"exponent_window": _exponent_window, "origin_slack": _origin_slack, "single_triangle": _single_triangle, "two_triangles": _two_triangles,
          "flat_x": lambda: _flat(0), "flat_y": lambda: _flat(1), "flat_z": lambda: _flat(2), "grid_edges": _grid_edges}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, rays): computed once per scene and shared, unchanged, by the CPU and the GPU test."""
    from oracle import pyoracle
    pyoracle.build()
    s, groups = SCENES[name]()
    rng = np.random.default_rng(sorted(SCENES).index(name) + 11)
    o = pyoracle.Oracle(); s.upload(o)
    small = name in ("single_triangle", "two_triangles") or name.startswith("flat")
    per = (N_RAYS // 3 if small else N_RAYS) // len(groups)
    parts = []
    for tris, reach in groups:
        first = _aimed(rng, tris, per, reach)
        parts += [first, _from_hits(rng, o, first, reach), _from_hits(rng, o, first, reach)]
    if name == "grid_edges":
        parts.append(_grid_edge_rays(rng, 8000))
    o.close()
    rays = np.concatenate(parts)
    rays.setflags(write=False)
    return s, rays


def _identical(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_oracle_tree_agrees_with_its_exhaustive_search_on_every_ray(name):
    """The reference the GPU test compares against, checked on the CPU first: the oracle's binary float tree and its search over every
    triangle give the same answer, bit for bit, for EVERY ray of the scene (closest hit) and the same occluded / not occluded."""
    from oracle import pyoracle
    from ray_hook import dxr_flags, RF_ACCEPT_FIRST
    s, rays = _case(name)
    o = pyoracle.Oracle(); s.upload(o)
    t = o.intersect_many(rays, 0, 0); ts = o.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1)
    o.set_brute_force(True)
    b = o.intersect_many(rays, 0, 0); bs = o.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1)
    o.close()
    print("\n%s: %d rays, %.1f %% hit" % (name, len(rays), 100 * t[:, 0].mean()))
    assert t[:, 0].mean() > 0.2                                   # the rays do meet the scene
    assert _identical(t, b)
    assert np.array_equal(ts[:, 0], bs[:, 0])


def _check_against_oracle(r, o, rays, what):
    from ray_hook import gpu_intersect, dxr_flags, RF_CULL_BACK, RF_ACCEPT_FIRST
    for flags in (0, RF_CULL_BACK):
        g = gpu_intersect(r, rays, flags, 0); c = o.intersect_many(rays, dxr_flags(flags), 0)
        same = (g[:, 0] == c[:, 0]) & (g[:, 4] == c[:, 4]) & (g[:, 5] == c[:, 5])
        for k in (1, 2, 3): same &= g[:, k].view(np.uint32) == c[:, k].view(np.uint32)
        bad = np.nonzero(~same)[0]
        print("\n%s, flags %d: %d rays, %.1f %% hit, different %d" % (what, flags, len(rays), 100 * c[:, 0].mean(), len(bad)))
        for k in bad[:5]: print("   ray", rays[k], "gpu", g[k], "oracle", c[k])
        assert len(bad) == 0, what
    g = gpu_intersect(r, rays, RF_ACCEPT_FIRST, 1); c = o.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1)
    assert np.array_equal(g[:, 0], c[:, 0]), (what, int((g[:, 0] != c[:, 0]).sum()))
    sub = rays[:: max(1, len(rays) // N_BRUTE)][:N_BRUTE]
    g = gpu_intersect(r, sub, 0, 0)
    o.set_brute_force(True); b = o.intersect_many(sub, 0, 0); o.set_brute_force(False)
    assert _identical(g[:, 0:6], b[:, 0:6]), what + ": against the exhaustive search"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_traversal_finds_the_oracles_hit_for_every_ray_at_the_node_formats_edges(R, name):
    from oracle import pyoracle
    s, rays = _case(name)
    r = R(); s.upload(r)
    o = pyoracle.Oracle(); s.upload(o)
    _check_against_oracle(r, o, rays, name)
    r.close(); o.close()


@pytest.mark.gpu
def test_refit_follows_a_root_that_grows_and_shrinks(R):
    """The skinned figure alone (its box IS the root box) posed at six times in a row, the tree refitted each time and never rebuilt: the root
    grows and shrinks with the stride, so every refit requantises every node from the top.  After each refit the hits equal those of a context
    that builds its tree at that pose, and the oracle's."""
    from oracle import pyoracle
    from ray_hook import gpu_intersect
    pyoracle.build()
    s = scenes.SceneData("node_format_refit")
    scenes.add_skinned_figure(s)
    r = R(); hr = s.upload(r); br = scenes.SkinBinding(r, s, hr, 0, use_mfma=0)
    o = pyoracle.Oracle(); ho = s.upload(o); bo = scenes.SkinBinding(o, s, ho, 0, use_mfma=0)
    br.pose(0.0); r.build_accel()
    rng = np.random.default_rng(29)
    for i, t in enumerate((0.25, 0.5, 0.8, 1.1, 1.45, 0.05)):
        br.pose(t); r.build_accel(); bo.pose(t)
        q = r.stats()
        assert (q.accel_builds, q.accel_refits) == (1, i + 1)
        target = rng.uniform((-0.6, -0.6, 0.0), (0.6, 0.6, 1.9), (7000, 3))
        d = _unit(rng, len(target))
        first = np.zeros((len(target), 8), f32); first[:, 0:3] = target + 3 * d; first[:, 4:7] = -d; first[:, 7] = 20
        rays = np.concatenate([first, _from_hits(rng, o, first, 2.0), _from_hits(rng, o, first, 2.0)])
        _check_against_oracle(r, o, rays, "refit to t = %g" % t)
        fresh = R(); hf = s.upload(fresh); scenes.SkinBinding(fresh, s, hf, 0, use_mfma=0).pose(t); fresh.build_accel()
        assert fresh.stats().accel_refits == 0
        assert _identical(gpu_intersect(r, rays, 0, 0), gpu_intersect(fresh, rays, 0, 0)), t
        fresh.close()
    r.close(); o.close()
