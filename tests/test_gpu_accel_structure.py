"""The acceleration structure the device builds, read back (pt_debug_accel_read, tests/accel_hook.py) and checked node by node by
tests/accel_ref.py check_tree (its docstring lists every invariant and where each bound comes from; tests/test_accel_check_host.py shows that
each can fail).  Run with -m gpu on an MI355X.  No ray is traced here: a case is a build (or a refit) plus a host check.
This file asks whether the device built A correct tree; WHICH tree -- the one the builder is meant to build -- is tests/test_gpu_builder_topology.py.

For all three builders (PT_BUILDER_LBVH, _PLOC, _PLOC_REINSERT), in a fresh context each:
  sizes      seeded random soups in three instances (non-indexed; 16- or 32-bit indices under a rotation and an uneven scale; mirrored) of
             1, 2, 3, 4, 5, 7, 13 triangles (the collapse filling its slots, kLeafMax), 255, 256, 257 (the block edge of every
             one-lane-per-triangle kernel and of a segment-tree pass), 171 and 172 (the scratch's segment tree, sized n + n / 8 + 64, grows from
             256 to 512 leaves), 32769 and 32770 (32768 binary nodes: k_collapse_small or the level launches), 58198 and 58199 (65536 or
             131072 segment-tree leaves: two passes or three).  The clustering must not have fallen back to the radix tree on these.
  stale      one context builds 58199 triangles, then 257, then 5: the segment tree's upper levels, the recorded ranges and the collapse's
             counters of the larger build are still in the scratch.
  geometry   at 2, 3, 4, 5 and 257 triangles (the smallest counts that have a node, and one past a block): coincident triangles (equal Morton
             codes; also 300 of them), zero-area and point triangles, a flat axis-aligned sheet on each axis, tiny triangles at an offset of 1e4
             (the step is close to an ulp of the origin: the exact plane check decides), extents mixed from 1e-6 to 1e6; and 2 and 64
             instances sharing one mesh, one scaled by 1e-3, one mirrored.  These may fall back; the test prints what built them.
  refit      257 and 32770 triangles in three instances: one instance's transform moves, another's vertex buffer is rewritten, the third
             is left alone; pt_build_accel must refit.  Child references, ranges and triangle order stay bit-identical, every node whose ranges
             hold no touched triangle stays bit-identical in all 64 bytes, and the new tree checks clean -- with one invariant read as the
             refit means it: children are in decreasing area in the pose of the BUILD (a refit keeps every child in its slot), so the order
             is demanded of the nodes no triangle of which has moved since, and of all of them again in the last step.  Then the moved instance is scaled to
             zero (boxes of zero extent), moved 1e4 away (the root grows), moved back (the root shrinks: byte for byte the tree of the first
             refit), and everything is put back (byte for byte the first build)."""
import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes
from tests import accel_ref as ar
from tests.accel_hook import accel_read

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
BUILDERS = [abi.BUILDER_LBVH, abi.BUILDER_PLOC, abi.BUILDER_PLOC_REINSERT]
BUILDER_NAMES = {abi.BUILDER_LBVH: "lbvh", abi.BUILDER_PLOC: "ploc", abi.BUILDER_PLOC_REINSERT: "reinsert"}
builders = pytest.mark.parametrize("builder", BUILDERS, ids=[BUILDER_NAMES[b] for b in BUILDERS])
SIZES = (1, 2, 3, 4, 5, 7, 13, 171, 172, 255, 256, 257, 32769, 32770, 58198, 58199)
GEOMETRY_COUNTS = (2, 3, 4, 5, 257)


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def add(s, tris, T=None, indexed=False, seed=0):
    """One instance of the triangles [n, 3, 3]; indexed: the vertices stored in a shuffled order behind an index stream."""
    pos = np.ascontiguousarray(tris, f32).reshape(-1, 3)
    if not indexed: return s.add_mesh(meshgen.Mesh(pos, None), T, 0)
    perm = np.random.default_rng(seed).permutation(len(pos))
    back = np.empty(len(pos), np.int64); back[perm] = np.arange(len(pos))
    return s.add_mesh(meshgen.Mesh(pos[perm], back), T, 0)


def share(s, i, T):
    """Another instance of instance i's streams under the transform T."""
    d = abi.PtInstanceDesc.from_buffer_copy(bytes(s.instances[i]))
    d.gpu.transform[:] = camera.cm(T); d.gpu.normal_transform[:] = camera.cm(camera.inverse_transpose(T))
    s.instances.append(d); s.mesh_records.append((s.mesh_records[i][0], np.asarray(T, np.float64), 0)); s.triangles += d.num_of_indices // 3


def random_tris(n, seed, spread=10.0, size=0.4):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-spread, spread, (n, 1, 3)) + rng.normal(0, size, (n, 3, 3)) * rng.uniform(0.2, 1.5, (n, 1, 1))).astype(f32)


TURNED = camera.trs((0.5, -0.25, 0.125), (0.0, 0.0, np.sin(0.35), np.cos(0.35)), (1.5, 0.75, 1.25))
MIRRORED = camera.trs((-0.75, 0.5, 0.25), scale=(-1.0, 1.0, 1.0))


def soup_scene(n, seed, centres=((0, 0, 0), (0, 0, 0), (0, 0, 0))):
    """n random triangles in up to three instances; centres moves the three apart."""
    s = scenes.SceneData("soup_%d" % n)
    t = random_tris(n, seed)
    a = n // 6 if n >= 1000 else n // 3                                  # (large: the third instance has more than 65535 vertices, so 32-bit indices)
    cuts = [t[:1], t[1:]] if n == 2 else [t[:a], t[a:2 * a], t[2 * a:]]
    kinds = [(None, False), (TURNED, True), (MIRRORED, True)]
    for k, (part, (T, indexed)) in enumerate(zip(cuts, kinds)):
        if len(part) == 0: continue
        part = (part + f32(centres[k])).astype(f32)
        add(s, part, T, indexed, seed + k)
    assert s.triangles == n
    return s


def coincident(n, seed):
    s = scenes.SceneData("coincident")
    one = random_tris(1, seed)[0]
    s.add_mesh(meshgen.Mesh(one, np.tile(np.arange(3), n)), None, 0)
    return s


def degenerate(n, seed):
    """Points, collinear triples, triangles with two equal vertices, and ordinary ones, in turn."""
    rng = np.random.default_rng(seed)
    t = random_tris(n, seed, spread=3.0)
    d = rng.normal(0, 0.3, (n, 3)).astype(f32)
    for i in range(n):
        if i % 4 == 0: t[i, 1] = t[i, 0]; t[i, 2] = t[i, 0]
        elif i % 4 == 1: t[i, 1] = t[i, 0] + d[i]; t[i, 2] = t[i, 0] + f32(2) * d[i]
        elif i % 4 == 2: t[i, 2] = t[i, 1]
    s = scenes.SceneData("degenerate"); add(s, t, None, True, seed)
    return s


def sheet(axis):
    def make(n, seed):
        t = random_tris(n, seed, spread=4.0)
        t[:, :, axis] = f32(0.75)
        s = scenes.SceneData("sheet_%d" % axis); add(s, t)
        return s
    return make


def tiny_far(n, seed):
    """Vertices on the float32 grid around 1e4 (an ulp is 2^-10): triangles a few ulps across, clusters a few dozen ulps apart."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 48, (n, 1, 3)) + rng.integers(0, 7, (n, 3, 3))
    t = (1.0e4 + k * 2.0 ** -10).astype(f32)
    assert np.array_equal(t.astype(np.float64), 1.0e4 + k * 2.0 ** -10)
    s = scenes.SceneData("tiny_far"); add(s, t, None, True, seed)
    return s


def mixed_extents(n, seed):
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-6, 6, (n, 1, 1))
    t = ((rng.normal(0, 3, (n, 1, 3)) + rng.normal(0, 1, (n, 3, 3))) * size).astype(f32)
    s = scenes.SceneData("mixed_extents"); add(s, t)
    return s


def shared_mesh(instances, mesh_tris, seed):
    rng = np.random.default_rng(seed)
    s = scenes.SceneData("shared_mesh")
    add(s, random_tris(mesh_tris, seed, spread=1.0, size=0.3), camera.trs((2.0, -1.0, 0.5), scale=(1e-3, 1e-3, 1e-3)), True, seed)
    for i in range(1, instances):
        q = rng.normal(0, 1, 4); q /= np.linalg.norm(q)
        sc = rng.uniform(0.5, 2.0, 3) * ((-1.0, 1.0, 1.0) if i == 1 else (1.0, 1.0, 1.0))
        share(s, 0, camera.trs(rng.uniform(-5, 5, 3), q, sc))
    assert ar.scene_rows(s)[1]["mask_flags"] & ar.TF_MIRRORED and not ar.scene_rows(s)[0]["mask_flags"] & ar.TF_MIRRORED
    return s


GEOMETRY = {"coincident": coincident, "degenerate": degenerate, "sheet_x": sheet(0), "sheet_y": sheet(1), "sheet_z": sheet(2), "tiny_far": tiny_far,
            "mixed_extents": mixed_extents}


# ---- the check ------------------------------------------------------------------------------------------------------------------------------
def read_and_check(r, rows, label, ordered=None):
    tree = accel_read(r)
    info = tree[0]
    stats = {}
    found = ar.check_tree(*tree, rows, stats, ordered)
    print("%s: %d triangles, %d nodes, nodes with 0..4 children %s, %d levels, stack_need %d, builder in force %s, fallbacks %d" %
          (label, info[ar.INFO_N_TRIS], stats["node_count"], stats["children"], stats["levels"], info[ar.INFO_STACK_NEED],
           BUILDER_NAMES[int(info[ar.INFO_BUILDER])], info[ar.INFO_FALLBACKS]))
    assert found == [], found[:10]
    assert (tree[2] is not None) == bool(info[ar.INFO_HAVE_RANGES]) and (info[ar.INFO_HAVE_RANGES] or info[ar.INFO_N_TRIS] < 2)
    return tree


def build_and_check(R, builder, s, label):
    r = R()
    try:
        r.set_accel_builder(builder)
        s.upload(r); r.build_accel()
        tree = read_and_check(r, ar.scene_rows(s), "%s %s" % (BUILDER_NAMES[builder], label))
        assert tree[0][ar.INFO_N_TRIS] == s.triangles and tree[0][ar.INFO_BUILDER] == builder
        return tree, r.stats()
    finally:
        r.close()


def seg_leaves_of(n):
    cap, p = n + n // 8 + 64, 256
    while p < cap: p *= 2
    return p


@builders
@pytest.mark.parametrize("n", SIZES)
def test_a_random_soup_builds_a_correct_tree(R, builder, n):
    tree, q = build_and_check(R, builder, soup_scene(n, 1000 + n), "soup")
    assert q.accel_builder_fallbacks == 0 and tree[0][ar.INFO_FALLBACKS] == 0          # the clustering path is what was checked
    assert tree[0][ar.INFO_SEG_LEAVES] == seg_leaves_of(n)                             # 171 | 172 and 58198 | 58199 straddle a size of the segment tree
    assert (q.accel_builds, q.accel_refits) == (1, 0)


def test_the_sizes_straddle_what_they_are_meant_to():
    assert (seg_leaves_of(171), seg_leaves_of(172), seg_leaves_of(58198), seg_leaves_of(58199)) == (256, 512, 65536, 131072)
    assert 32769 - 1 == 32768 and 32770 - 1 > 32768                                    # binary nodes against kSmallCollapseNodes


@builders
def test_a_smaller_build_in_a_used_scratch_is_correct(R, builder):
    r = R()
    try:
        r.set_accel_builder(builder)
        for k, n in enumerate((58199, 257, 5)):
            s = soup_scene(n, 2000 + n)
            s.upload(r); r.build_accel()
            tree = read_and_check(r, ar.scene_rows(s), "%s after %d builds, soup" % (BUILDER_NAMES[builder], k))
            q = r.stats()
            assert tree[0][ar.INFO_N_TRIS] == n and tree[0][ar.INFO_SEG_LEAVES] == 131072 and (q.accel_builds, q.accel_builder_fallbacks) == (k + 1, 0)
    finally:
        r.close()


@builders
@pytest.mark.parametrize("kind,n", [(kind, n) for kind in sorted(GEOMETRY) for n in GEOMETRY_COUNTS] + [("coincident", 300)])
def test_degenerate_geometry_builds_a_correct_tree(R, builder, kind, n):
    build_and_check(R, builder, GEOMETRY[kind](n, 3000 + n), "%s" % kind)


@builders
@pytest.mark.parametrize("instances,mesh_tris", [(2, 1), (2, 2), (2, 129), (64, 1), (64, 4), (64, 5)])
def test_instances_of_one_mesh_build_a_correct_tree(R, builder, instances, mesh_tris):
    build_and_check(R, builder, shared_mesh(instances, mesh_tris, 4000 + instances + mesh_tris), "%d instances of %d triangles" % (instances, mesh_tris))


# ---- refit ----------------------------------------------------------------------------------------------------------------------------------
def same_bytes(a, b, what):
    a, b = ar.as_bytes(a, 1), ar.as_bytes(b, 1)
    assert a.shape == b.shape and np.array_equal(a, b), (what, int((a != b).sum()), "bytes differ")


@builders
@pytest.mark.parametrize("n", (257, 32770))
def test_a_refit_is_a_fresh_quantisation_of_the_same_topology(R, builder, n):
    s = soup_scene(n, 5000 + n, centres=((0, 0, -30), (0, 0, 0), (0, 0, 30)))       # apart along z, which all three transforms keep: most nodes hold one instance
    name = BUILDER_NAMES[builder]
    r = R()
    try:
        r.set_accel_builder(builder)
        h = s.upload(r); r.build_accel()
        first = read_and_check(r, ar.scene_rows(s), name + " build")
        buffer1 = h["buffers"][s.instances[1].gpu.position_descriptor]
        pos1 = s.buffers[s.instances[1].gpu.position_descriptor][0]
        T0 = np.array(list(s.instances[0].gpu.transform), f32)
        rng = np.random.default_rng(n)
        jittered = (pos1 + rng.normal(0, 0.2, pos1.shape)).astype(f32)
        col = lambda T: np.array(camera.cm(T), f32)
        moved = col(camera.trs((0.37, -0.21, 0.11), (0.0, np.sin(0.1), 0.0, np.cos(0.1))))
        to_point = col(camera.translate((0.5, 0.25, -0.125)) @ np.diag([0.0, 0.0, 0.0, 1.0]))
        far = col(camera.trs((1.0e4, 0.37, -0.21)))
        now = {"pos": pos1}                                               # instance 1's vertices as the device has them

        ids = lambda t: ar.as_bytes(t[3], 64).view(u32).reshape(-1, 16)[:, [3, 7]]
        # a refit keeps every child in its slot: decreasing area is claimed where no triangle has moved since the build (accel_ref `order`)
        in_build_pose = ~ar.touched_nodes(first[2], n, np.isin(ids(first)[:, 0], [0, 1]))

        def refit(prev, T, pos, touched, label, ordered=in_build_pose):
            """Instance 0 under the transform T, instance 1's vertices pos (None: as they are); touched: the instances this changes."""
            q0 = r.stats()
            table = [abi.PtInstanceDesc.from_buffer_copy(bytes(d)) for d in h["instances"]]
            table[0].gpu.transform[:] = [float(x) for x in T]
            r.set_instances(table)
            if pos is not None: r.buffer_update(buffer1, pos); now["pos"] = pos
            r.build_accel()
            q1 = r.stats()
            assert (q1.accel_builds, q1.accel_refits) == (q0.accel_builds, q0.accel_refits + 1), label
            tree = read_and_check(r, ar.scene_rows(s, {0: T}, {1: now["pos"]}), "%s refit, %s" % (name, label), ordered)
            same_bytes(tree[1][:, 16:32], prev[1][:, 16:32], label + ": child references")
            same_bytes(tree[2], prev[2], label + ": ranges")
            assert np.array_equal(ids(tree), ids(prev)), label + ": triangle order"
            hit = ar.touched_nodes(tree[2], n, np.isin(ids(tree)[:, 0], touched))
            assert hit[0] and (~hit).sum() * 8 >= len(hit), (label, int(hit.sum()), len(hit))      # the root is touched, an eighth of the nodes at least is not
            same_bytes(tree[1][~hit], prev[1][~hit], label + ": nodes without a touched triangle")
            assert tree[0][ar.INFO_STACK_NEED] == prev[0][ar.INFO_STACK_NEED] and tree[0][ar.INFO_WIDE_NODES] == prev[0][ar.INFO_WIDE_NODES]
            return tree

        second = refit(first, moved, jittered, [0, 1], "moved and rewritten")
        assert not np.array_equal(second[1], first[1])
        t = refit(second, to_point, None, [0], "scaled to zero")
        t = refit(t, far, None, [0], "1e4 away")
        assert t[1][0, 0:12].tobytes() != second[1][0, 0:12].tobytes() or t[1][0, 12:15].tobytes() != second[1][0, 12:15].tobytes()      # the root's grid changed
        t = refit(t, moved, None, [0], "moved back")
        for k, what in ((1, "nodes"), (3, "packets"), (4, "shading packets")): same_bytes(t[k], second[k], "moved back: " + what)
        t = refit(t, T0, pos1, [0, 1], "everything put back", None)
        for k, what in ((1, "nodes"), (3, "packets"), (4, "shading packets")): same_bytes(t[k], first[k], "put back: " + what)
    finally:
        r.close()
