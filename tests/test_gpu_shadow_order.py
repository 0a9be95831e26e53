"""The visiting order of accept-first occlusion rays (csrc/pt_traverse.h, trav_node_step<COUNT, false>): the step goes on with the entering
child whose entry distance is greatest, ties to the lowest slot, and pushes the others in slot order; alpha-shadow rays keep the slot order.
An occlusion ray's answer -- some standing candidate exists -- does not depend on the order, so every scene below is held to the oracle's
EXHAUSTIVE search over all triangles, ray for ray, no ray excluded, through the shadow stage alone (k_wf_shadow), the fused launch
(k_wf_traverse) and traverse() (pt_debug_intersect, mode 1).  No test asserts a node count.

  room_closed     a closed box of 6 x 6 quads a side with 28 small boxes standing just above its floor; rays leave the floor and the boxes'
                  faces (1.5e-5 off the surface, as the path tracer's do) in all directions: the occluder is usually the far shell
  room_open       the same room without its +x wall: occluded and free rays mixed
  ... refitted    the closed room after a pt_buffer_update that moves one corner of the shell outwards (a refit, and a new root box)
  root_tie        40 long slivers, the box of each of which contains every ray origin: whatever the tree, a ray starts inside every
                  child of every node it visits, so all entry distances tie at 0 and the slot order decides
  two_triangles   the root is the only node and has two leaves and two empty slots
  five_triangles  five well separated triangles: nodes with empty slots and with one, two or three entering children
  deep_fan        57 slivers that fan out from the origin along +x, +y and +z with the box centres of tests/traversal_scenes.py's deep chain,
                  under the radix-tree builder: one chain of 57 binary levels, a tree that needs more stack entries than a lane holds in
                  LDS.  Every sliver's box contains the small cube at the origin in which the rays start, so a ray enters every child of
                  every node it visits and each step pushes the node's other children: a ray that meets nothing (nine in ten) walks the
                  whole tree
  layered alpha   tests/traversal_scenes.py's eight alpha sheets under SHADOW_CASES, held to check_shadow's rule

Direction classes per scene are stated by the host test below."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gltf_renderer_amd import abi, meshgen, scenes  # noqa: E402
import traversal_ref as tr  # noqa: E402
import traversal_scenes as tscenes  # noqa: E402
from ray_hook import (gpu_intersect, dxr_flags, trace_queues, shadow_rays_of, TQ_SHADOW, TQ_FUSED, RF_FORCE_NON_OPAQUE, RF_ACCEPT_FIRST,  # noqa: E402
                      RF_CULL_BACK)
from test_traversal_host import check_shadow, shadow_value, SHADOW_CASES, SHADOW_TMAX  # noqa: E402

f32 = np.float32
TMAX = 1000.0                      # the application's max_ray_length: a shadow ray runs that far whatever the light's distance
OFFSET = 1.5e-5                    # the path tracer's offset along the normal
ROOM_LO, ROOM_HI = np.array([-4.0, 0.0, -3.0]), np.array([4.0, 5.0, 3.0])
STACK_LDS = 24                     # csrc/pt_traverse.h kStackLds
N_LAYERED = 6000


def _unit(rng, k):
    d = rng.standard_normal((k, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _scene(name, mesh):
    s = scenes.SceneData(name)
    s.add_mesh(mesh, None, 0)
    return s


def _soup(name, tris):
    pos = f32(tris).reshape(-1, 3)
    return _scene(name, meshgen.Mesh(pos, np.arange(len(pos)), normals=np.tile(f32([0, 0, 1]), (len(pos), 1))))


def _rays(origin, direction, tmax=TMAX):
    r = np.zeros((len(origin), 8), f32)
    r[:, 0:3] = origin; r[:, 4:7] = direction; r[:, 7] = tmax
    return r


def _triangles(mesh):
    return mesh.positions.astype(np.float64)[mesh.indices.reshape(-1, 3)]


def _from_surfaces(rng, tris, n, above=False):
    """n rays from random points of `tris`, moved OFFSET along the triangle's normal (either side; above: the side of +y), in directions
    uniform over the hemisphere of that side."""
    t = tris[rng.integers(0, len(tris), n)]
    w = rng.dirichlet((1, 1, 1), n)
    p = (t * w[:, :, None]).sum(axis=1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    side = np.sign(nrm[:, 1]) if above else rng.choice([-1.0, 1.0], n)
    out = nrm * side[:, None]
    d = _unit(rng, n)
    d *= np.where((d * out).sum(axis=1) < 0, -1.0, 1.0)[:, None]              # leaving the surface on the side of the origin
    return p + out * OFFSET, d


# ---- the rooms ------------------------------------------------------------------------------------------------------------------------------
def _room_meshes(with_wall, corner=None):
    lo, hi = ROOM_LO, ROOM_HI
    d = hi - lo
    X, Y, Z = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    g = lambda o, u, v: meshgen.grid(6, 6, o, u, v)
    floor = g(lo, X, Z)
    walls = [g(lo + Y, X, Z), g(lo, X, Y), g(lo + Z, X, Y), g(lo, Z, Y)] + ([g(lo + X, Z, Y)] if with_wall else [])
    rng = np.random.default_rng(7)
    clutter = []
    for k in range(28):                                                     # 4 x 7 cells of the floor, one box in each, 2^-6 above the floor
        cx = lo[0] + (k % 7 + 0.5) * d[0] / 7 + rng.uniform(-0.2, 0.2); cz = lo[2] + (k // 7 + 0.5) * d[2] / 4 + rng.uniform(-0.2, 0.2)
        h = rng.uniform(0.1, 0.3, 3) * [1, 3, 1]
        clutter.append(meshgen.box((cx - h[0], 2.0 ** -6, cz - h[2]), (cx + h[0], 2.0 ** -6 + h[1], cz + h[2])))
    shell = meshgen.merge([floor] + walls)
    if corner is not None:
        pos = shell.positions.copy()
        pos[np.all(pos == f32(ROOM_LO), axis=1)] = f32(corner)             # every copy of the lower corner vertex (floor and two walls)
        shell = meshgen.Mesh(pos, shell.indices, shell.normals, shell.tangents, shell.uv0)
    return floor, shell, meshgen.merge(clutter)


ROOM_CORNER_MOVED = ROOM_LO - [1.5, 0.75, 2.0]


def _room(with_wall, corner=None):
    floor, shell, clutter = _room_meshes(with_wall, corner)
    s = scenes.SceneData("shadow_order_room_%s" % ("closed" if with_wall else "open"))
    s.add_mesh(shell, None, 0); s.add_mesh(clutter, None, 0)
    rng = np.random.default_rng(201 if with_wall else 202)
    n = 2000
    fo, fd = _from_surfaces(rng, _triangles(floor), n, above=True)
    co, cd = _from_surfaces(rng, _triangles(clutter), n)
    kind = np.repeat(np.array(["from the floor", "from the clutter"]), n)
    return s, _rays(np.concatenate([fo, co]), np.concatenate([fd, cd])), kind


def _room_closed(): return _room(True)
def _room_open(): return _room(False)


# ---- every origin inside every box ------------------------------------------------------------------------------------------------------------
TIE_HALF = 0.25
N_TIE = 40


def _root_tie():
    rng = np.random.default_rng(203)
    tris = []
    for _ in range(N_TIE):                                                   # slivers from one octant to the opposite one
        a = rng.uniform(1.0, 3.0, 3) * rng.choice([-1.0, 1.0], 3)
        b = -np.sign(a) * rng.uniform(1.0, 3.0, 3)
        tris.append(np.array([a, b, b + rng.uniform(-0.4, 0.4, 3)]))
    n = 3000
    o = rng.uniform(-TIE_HALF, TIE_HALF, (n, 3))
    return _soup("shadow_order_root_tie", tris), _rays(o, _unit(rng, n)), np.repeat(np.array(["from the common core"]), n)


# ---- the smallest trees -------------------------------------------------------------------------------------------------------------------------
def _aimed(rng, tris, n, reach):
    """n rays aimed at random points of the triangles from afar, n from points near the triangles in random directions."""
    t = tris[rng.integers(0, len(tris), 2 * n)]
    p = (t * rng.dirichlet((1, 1, 1), 2 * n)[:, :, None]).sum(axis=1)
    d = _unit(rng, 2 * n)
    o = p - d * (reach * 10.0 ** rng.uniform(-2, 0, 2 * n))[:, None]
    o[n:] = p[n:] + _unit(rng, n) * 0.05 * reach                            # beside the surface: most of these pass the triangles by
    return _rays(o, d), np.repeat(np.array(["aimed", "nearby"]), n)


def _two_triangles():
    tris = np.array([[[-1, 0.25, -1], [1, 0.5, -1], [0, 0, 1]], [[2, 3, 0.5], [3, 3.5, 0.25], [2.5, 2, 1.5]]], np.float64)
    rays, kind = _aimed(np.random.default_rng(204), tris, 1500, 3.0)
    return _soup("shadow_order_two_triangles", tris), rays, kind


def _five_triangles():
    rng = np.random.default_rng(205)
    centres = np.array([[0, 0, 0], [3, 0.5, 0], [0.5, 3, 0.2], [0.2, 0.4, 3], [3, 3, 3]], np.float64)
    tris = centres[:, None, :] + rng.uniform(-0.8, 0.8, (5, 3, 3))
    rays, kind = _aimed(rng, tris, 1500, 4.0)
    return _soup("shadow_order_five_triangles", tris), rays, kind


# ---- the deep fan -----------------------------------------------------------------------------------------------------------------------------
FAN_DELTA = 2.0 ** -12


def _deep_fan():
    """57 slivers from the origin out along +x, +y or +z whose bounding-box centres are tests/traversal_scenes.py's deep chain's --
    (C, d/2, d/2), (d/2, C, d/2), (d/2, d/2, C) with C = (2^j + 1/4) 2^-10, j = 0..18, d = 2^-12: every Morton code has a different highest
    bit, so the radix tree is one chain of 57 binary levels -- and whose boxes all contain the cube [0, d]^3 the rays start in."""
    d = FAN_DELTA
    tris = []
    for j in range(19):
        C2 = 2.0 * (2.0 ** j + 0.25) * 2.0 ** -10
        tris += [[(0, 0, 0), (C2, d, 0), (C2, 0, d)], [(0, 0, 0), (0, C2, d), (d, C2, 0)], [(0, 0, 0), (d, 0, C2), (0, d, C2)]]
    rng = np.random.default_rng(206)
    n = 1500
    o = rng.uniform(0.2 * d, 0.8 * d, (2 * n, 3))
    dirs = _unit(rng, 2 * n)
    dirs[:n] = -np.abs(dirs[:n])                                             # out of the octant the slivers lie in
    kind = np.repeat(np.array(["leaving the fan", "any direction"]), n)
    return _soup("shadow_order_deep_fan", np.array(tris, np.float64)), _rays(o, dirs), kind


SCENES = {"room_closed": _room_closed, "room_open": _room_open, "root_tie": _root_tie, "two_triangles": _two_triangles, "five_triangles": _five_triangles,
          "deep_fan": _deep_fan}
# share of occluded rays each scene must show, so that it is the scene its name says
OCCLUDED_SHARE = {"room_closed": (0.99, 1.0), "room_open": (0.5, 0.97), "root_tie": (0.1, 0.9), "two_triangles": (0.1, 0.9), "five_triangles": (0.1, 0.9),
                  "deep_fan": (0.02, 0.2)}


@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import pyoracle
    pyoracle.build()
    s, rays, kind = SCENES[name]()
    rays.setflags(write=False)
    return s, rays, kind


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _brute_force_occluded(o, rays):
    """Occluded or not by the oracle's exhaustive search over every triangle; the oracle's tree must say the same."""
    o.set_brute_force(True)
    brute = o.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1)[:, 0] > 0
    o.set_brute_force(False)
    tree = o.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1)[:, 0] > 0
    assert np.array_equal(tree, brute), ("the oracle's tree against its exhaustive search", int((tree != brute).sum()))
    return brute


def _state_classes(name, kind, occluded):
    for c in np.unique(kind):
        k = kind == c
        print("%s, %s: %d rays, %.1f %% occluded" % (name, c, int(k.sum()), 100 * occluded[k].mean()))
        assert k.sum() >= 1000
    lo, hi = OCCLUDED_SHARE[name]
    assert lo <= occluded.mean() <= hi, (name, float(occluded.mean()))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_are_what_their_names_say_and_the_oracles_tree_agrees_with_its_exhaustive_search(name):
    from oracle import pyoracle
    s, rays, kind = _case(name)
    o = pyoracle.Oracle(); s.upload(o)
    occluded = _brute_force_occluded(o, rays)
    _state_classes(name, kind, occluded)
    if name == "room_closed":
        # "usually the far shell": the nearest thing a ray meets is the shell (instance 0) for most rays
        h = o.intersect_many(rays, 0, 0)
        shell = (h[:, 0] > 0) & (h[:, 4] == 0)
        print("room_closed: the nearest surface is the shell for %.1f %% of the rays, at a median distance of %.2f" % (100 * shell.mean(), float(np.median(h[shell, 1]))))
        assert shell.mean() > 0.5 and np.median(h[shell, 1]) > 1.0
    if name == "root_tie":
        T = tr.Triangles(s).P
        assert np.all(T.min(axis=1).max(axis=0) < -TIE_HALF) and np.all(T.max(axis=1).min(axis=0) > TIE_HALF)      # every triangle's box holds every origin
        assert np.all(np.abs(rays[:, 0:3]) <= TIE_HALF) and len(T) == N_TIE
    if name == "deep_fan":
        T = tr.Triangles(s).P
        assert np.all(T.min(axis=1) == 0) and np.all(T.max(axis=1) >= FAN_DELTA)                                    # every triangle's box holds [0, d]^3 ...
        assert np.all(rays[:, 0:3] > 0) and np.all(rays[:, 0:3] < f32(FAN_DELTA))                                   # ... and with it every origin
        assert occluded.mean() < 0.2                                                                                 # most rays meet nothing: they walk the whole tree
    o.close()


def _check_occlusion(r, rays, occluded, what):
    """Counters on and off: the shadow stage alone, the fused launch (beside a closest queue) and traverse() give the exhaustive search's
    answer for every ray."""
    n = len(rays)
    shards = np.random.default_rng(n).integers(0, 256, n).astype(np.uint32)
    sh = shadow_rays_of(rays)
    want = np.where(occluded, f32(0), f32(1))
    closest = np.array(rays[:500]); closest[:, 3] = 0
    for counting in (True, False):
        r.enable_counters(counting)
        r.reset_stats()
        g = gpu_intersect(r, rays, RF_ACCEPT_FIRST, 1)
        bad = np.nonzero((g[:, 0] > 0) != occluded)[0]
        for k in bad[:5]: print("   traverse()", rays[k].tolist(), "gpu", g[k].tolist())
        assert len(bad) == 0, (what, "traverse()", counting, len(bad))
        for which, bounce in ((TQ_SHADOW, 0), (TQ_FUSED, 1)):
            _, v, _, stray = trace_queues(r, closest if which == TQ_FUSED else None, shards[:500] if which == TQ_FUSED else None, sh, shards,
                                          np.arange(n) % 2, shadow_tmax=TMAX, flags=0, bounce=bounce, blocks_per_shard=2, which=which)
            bad = np.nonzero(bits(v) != bits(want))[0]
            for k in bad[:5]: print("   wavefront", which, rays[k].tolist(), "gpu", float(v[k]), "exhaustive search", bool(occluded[k]))
            assert len(bad) == 0 and stray[0] == 0 and stray[1] == 0, (what, which, counting, len(bad))
        q = r.stats()                                                       # raises if a push was dropped
        if counting: print("%s: %d shadow-stage node visits and %d triangle tests for 2 x %d rays" % (what, q.nodes_visited_shadow, q.tris_tested_shadow, n))
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_occlusion_ray_gets_the_exhaustive_searchs_answer(name):
    from gltf_renderer_amd.renderer import Renderer
    from oracle import pyoracle
    s, rays, kind = _case(name)
    o = pyoracle.Oracle(); s.upload(o)
    occluded = _brute_force_occluded(o, rays)
    o.close()
    r = Renderer()
    if name == "deep_fan": r.set_accel_builder(abi.BUILDER_LBVH)
    s.upload(r)
    r.enable_counters(False); r.reset_stats()
    q = _check_occlusion(r, rays, occluded, name)
    if name == "deep_fan":
        # the premise: the tree needs more stack entries than a step may still push into the LDS part.  A ray that meets nothing (nine in ten)
        # starts inside every box, so it visits every node and every step pushes all the node's other children
        print("deep_fan: stack need %d, deep pushes %d" % (q.bvh_stack_need, q.deep_stack_pushes))
        assert q.bvh_stack_need > STACK_LDS - 3, q.bvh_stack_need
    r.close()


@pytest.mark.gpu
def test_every_occlusion_ray_gets_the_exhaustive_searchs_answer_after_a_refit_that_moves_the_root():
    """The closed room, then the shell's lower corner moves outwards by (1.5, 0.75, 2) (a pt_buffer_update: refitted, never rebuilt): the root's
    origin changes on every axis and every node on the corner's path is requantised."""
    from gltf_renderer_amd.renderer import Renderer
    from oracle import pyoracle
    s, rays, kind = _case("room_closed")
    _, moved, _ = _room_meshes(True, ROOM_CORNER_MOVED)
    assert np.array_equal(moved.positions.min(axis=0), f32(ROOM_CORNER_MOVED))
    r = Renderer(); hr = s.upload(r); r.build_accel()
    o = pyoracle.Oracle(); ho = s.upload(o); o.build_accel()
    which = s.instances[0].gpu.position_descriptor
    r.buffer_update(hr["buffers"][which], moved.positions); r.build_accel()
    o.buffer_update(ho["buffers"][which], moved.positions); o.build_accel()
    q = r.stats()
    assert (q.accel_builds, q.accel_refits) == (1, 1)
    occluded = _brute_force_occluded(o, rays)
    o.close()
    _state_classes("room_closed", kind, occluded)
    _check_occlusion(r, rays, occluded, "room_closed, refitted")
    r.close()


@pytest.mark.gpu
def test_a_frame_of_the_room_counts_the_shadow_rays_it_sent():
    """rays_shadow is tallied where the shade stage queues a shadow ray (the traversal hook queues none itself), so the count is taken over a
    frame: the open room, a point light inside and a constant environment beyond the missing wall, 48 x 32 pixels, counters on -- as many
    shadow, bounce and primary rays and closest hits as the oracle counts."""
    from gltf_renderer_amd import camera
    from gltf_renderer_amd.renderer import Renderer
    from oracle import pyoracle
    s, _, _ = _room_open()
    s.width, s.height = 48, 32
    s.world_to_view = camera.free_world_to_view((0.0, 2.0, 0.5), yaw=0.0)
    s.add_light(abi.LIGHT_POINT, position=(1.0, 4.0, 0.5), color=(1, 1, 1), intensity=30.0)
    st = abi.PtSettings.app_defaults()
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    st.environment_color[:] = (1.0, 1.0, 1.0)
    s.settings = st
    r = Renderer(); s.upload(r); r.enable_counters(True)
    o = pyoracle.Oracle(); s.upload(o)
    out = r.create_output(s.width, s.height)
    b = np.zeros((s.height, s.width, 4), f32)
    r.reset_stats(); o.counters()
    for f in range(2):
        r.trace(st, s.execute_params(f), out); o.trace(st, s.execute_params(f), b)
    q = r.stats(); c = o.counters()
    print("room frame: %d shadow rays (oracle %d), %d bounce rays" % (q.rays_shadow, c["shadow"], q.rays_bounce))
    assert q.rays_shadow == c["shadow"] and q.rays_shadow > s.width * s.height
    assert (q.rays_primary, q.rays_bounce, q.closest_hits) == (c["primary"], c["bounce"], c["closest_hits"])
    assert (b[..., :3].sum(axis=2) > 0).mean() > 0.5                        # the oracle's frame is lit: the paths above carried light
    r.close(); o.close()


# ---- alpha shadows keep their order -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layered():
    s = tscenes.layered_alpha_scene()
    rays = tscenes.layered_rays(N_LAYERED, 21)
    rays[:, 7] = SHADOW_TMAX
    return s, rays, tr.Crossings(tr.Triangles(s), rays)


def _oracle_alone(oracle_lib, s, rays, X):
    """What the host test does (tests/test_traversal_host.py): the oracle against the restatement; the undecided rays per case."""
    o = oracle_lib.Oracle(); s.upload(o)
    und = {}
    for rf, mode in SHADOW_CASES:
        h = o.intersect_many(rays, dxr_flags(rf), mode)
        und[rf] = check_shadow(("oracle", rf), h[:, 0] > 0, shadow_value(h), X.query(rf, mode, tmax=SHADOW_TMAX))[1]
    o.close()
    return und


def test_layered_rays_of_this_file_are_what_the_alpha_test_needs(oracle_lib):
    s, rays, X = _layered()
    und = _oracle_alone(oracle_lib, s, rays, X)
    a = X.query(RF_FORCE_NON_OPAQUE, 1, tmax=SHADOW_TMAX)
    partial = (a["transmission"] > 0) & (a["transmission"] < 1)
    print("layered alpha, %d rays: undecided per case %s, %.1f %% partial transmissions" % (len(rays), und, 100 * partial.mean()))
    assert max(und.values()) <= 0.02 * len(rays) and partial.mean() >= 0.05 and (partial & (a["k"] >= 3)).sum() >= 50


@pytest.mark.gpu
def test_alpha_shadow_and_accept_first_rays_of_the_layered_scene_keep_check_shadows_rule(oracle_lib):
    from gltf_renderer_amd.renderer import Renderer
    s, rays, X = _layered()
    und = _oracle_alone(oracle_lib, s, rays, X)
    n = len(rays)
    shards = np.random.default_rng(n).integers(0, 256, n).astype(np.uint32)
    sh = shadow_rays_of(rays)
    closest = np.array(rays[:500]); closest[:, 3] = 0; closest[:, 7] = 100.0
    r = Renderer(); s.upload(r)
    for rf, mode in SHADOW_CASES:
        flags = (abi.FLAG_ALPHA_SHADOWS if rf & RF_FORCE_NON_OPAQUE else 0) | (abi.FLAG_CULL_BACKFACE if rf & RF_CULL_BACK else 0)
        ref = X.query(rf, mode, tmax=SHADOW_TMAX)
        g = gpu_intersect(r, rays, rf, mode)
        _, u = check_shadow(("traverse()", rf), g[:, 0] > 0, shadow_value(g), ref)
        assert u <= und[rf], (rf, u, und[rf])
        for which, bounce in ((TQ_SHADOW, 0), (TQ_FUSED, 1)):
            _, v, _, stray = trace_queues(r, closest if which == TQ_FUSED else None, shards[:500] if which == TQ_FUSED else None, sh, shards, 1,
                                          shadow_tmax=SHADOW_TMAX, flags=flags, bounce=bounce, blocks_per_shard=2, which=which)
            assert stray[0] == 0 and stray[1] == 0
            # "committed" is not visible through the hook (a committed ray's transmission, 1 otherwise): traverse()'s, checked above
            _, u = check_shadow(("wavefront", which, rf), g[:, 0] > 0, v, ref)
            assert u <= und[rf], (rf, which, u, und[rf])
    r.close()
