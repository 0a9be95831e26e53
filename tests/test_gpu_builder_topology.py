"""WHICH tree the device builds: the acceleration structure read back (pt_debug_accel_read, tests/accel_hook.py) and compared node for node
with tests/builder_ref.py, the three builders of csrc/accel.hip restated on the host (tests/test_builder_ref_host.py shows that the restatement
means something: that a wrong Morton code, search radius, pair key, lock round count, pass count, gain threshold, collapse order or sorting
network gives another tree on these very scenes).  tests/test_gpu_accel_structure.py asks whether it is A correct tree; every case here runs
its check_tree on the same read too.  Run with -m gpu on an MI355X.  No ray is traced: a case is a build plus host work.  No tolerance anywhere:
every comparison is of integers or of float32 bits.

  keys       pt_debug_accel_keys, the sorted Morton keys of the build, against sorted(morton_keys): soups of 2, 255, 257, 2049, a sheet on each
             axis (zero extent: the 1e-30 floor decides), tiny_far, mixed_extents
  lbvh       soups of 2 .. 13, 255 .. 257, 2047 .. 2049 (a tile of the sort), 32769 | 32770 (k_collapse_small | level launches), 58199; 5 and 300
             coincident triangles (equal keys: the index builds the tree); the three sheets
  ploc       the same soups and 240, 241, 272, 273, 511, 513 (the +-16 window of k_ploc_nearest at and across the edge of a 256-thread block);
             16 x 16 quads and 1 x 128 quads on exactly representable coordinates (areas tie everywhere: the integer key decides every pair);
             300 coincident triangles; 64 instances of one 5-triangle mesh; block_or_strip (the extent-sum term of the pair key decides)
  reinsert   4 .. 1025 triangles with MIPT_REINSERT_PASSES 0 (the PLOC tree), 1, 2, 8; the quad grid and mixed_extents at 8
  scratch    one context builds 58199 triangles (clustering, no pass), then 257 and 5 (8 passes): the temporary tree, boxes and counters of the
             larger build are still in the scratch
  fallback   the monotone strip of tests/test_gpu_round3.py (12 001 triangles), on which the clustering gives up: the radix tree"""
import os
import time

import numpy as np
import pytest

from gltf_renderer_amd import abi, meshgen, scenes
from tests import accel_ref as ar
from tests import builder_ref as br
from tests.accel_hook import accel_read, accel_keys
from tests.test_gpu_accel_structure import soup_scene, coincident, sheet, tiny_far, mixed_extents, shared_mesh, add, BUILDER_NAMES

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


# ---- scenes (tests/test_builder_ref_host.py uses them by these names) -------------------------------------------------------------------------
def quad_grid(nx, ny):
    """nx x ny unit quads in the plane z = 0.5, two triangles each, on integer coordinates: every box, union and area is exact and ties abound."""
    t = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (i, j, 0.5), (i + 1, j, 0.5), (i + 1, j + 1, 0.5), (i, j + 1, 0.5)
            t.append((a, b, c)); t.append((a, c, d))
    s = scenes.SceneData("quads_%dx%d" % (nx, ny)); add(s, np.array(t, f32))
    return s


def block_or_strip():
    """Three flat boxes in Morton order B, A, C: B with its neighbour A is a 1 x 4 strip, B with C, one slot further, a 2 x 2 block of the same
    area.  Only the extent-sum term of the pair key prefers the block; the index distance alone would take the strip."""
    B, A, C = [(0, 0), (1, 0), (0, 2)], [(0, 2), (1, 2), (0, 4)], [(1, 0), (2, 0), (1, 2)]
    s = scenes.SceneData("block_or_strip"); add(s, np.array([[(x, y, 0.5) for x, y in t] for t in (B, A, C)], f32))
    return s


def monotone_strip(n=12000):
    """tests/test_gpu_round3.py test_clustering_builder_that_gives_up_falls_back_to_the_radix_tree: points on a line with geometrically growing
    gaps, one degenerate triangle each, plus one real triangle.  Cluster i prefers i - 1, which prefers i - 2: one merge a round."""
    x = np.cumsum(1e-4 * 1.0008 ** np.arange(n)).astype(f32)
    pos = np.zeros((3 * n, 3), f32); pos[:, 0] = np.repeat(x, 3); pos[:, 2] = 5.0
    pos = np.concatenate([np.array([[-1, 0, -1], [1, 0, -1], [0, 0, 1]], f32), pos])
    s = scenes.SceneData("monotone_strip"); s.add_mesh(meshgen.Mesh(pos, np.arange(len(pos))), None, 0)
    return s


SCENES = {
    "soup": lambda n: soup_scene(n, 1000 + n),
    "coincident": lambda n: coincident(n, 3000 + n),
    "sheet_x": lambda n: sheet(0)(n, 3000 + n), "sheet_y": lambda n: sheet(1)(n, 3000 + n), "sheet_z": lambda n: sheet(2)(n, 3000 + n),
    "tiny_far": lambda n: tiny_far(n, 3000 + n),
    "mixed_extents": lambda n: mixed_extents(n, 3000 + n),
    "shared_mesh_64x": lambda n: shared_mesh(64, n, 4000 + 64 + n),
    "quads_16x": lambda n: quad_grid(16, n),
    "quads_1x": lambda n: quad_grid(1, n),
    "block_or_strip": lambda n: block_or_strip(),
}
SMALL = (2, 3, 4, 5, 7, 13, 255, 256, 257, 2047, 2048, 2049, 32769, 32770, 58199)
LBVH_CASES = [("soup", n) for n in SMALL] + [("coincident", 5), ("coincident", 300), ("sheet_x", 257), ("sheet_y", 257), ("sheet_z", 257)]
PLOC_CASES = [("soup", n) for n in SMALL + (240, 241, 272, 273, 511, 513)] + [("quads_16x", 16), ("quads_1x", 128), ("coincident", 300), ("shared_mesh_64x", 5), ("block_or_strip", 3)]
REINSERT_CASES = [("soup", n, p) for n in (4, 5, 7, 13, 64, 65, 257, 1025) for p in (0, 1, 2, 8)] + [("quads_16x", 16, 8), ("mixed_extents", 257, 8)]
KEY_CASES = [("soup", 2), ("soup", 255), ("soup", 257), ("soup", 2049), ("sheet_x", 257), ("sheet_y", 257), ("sheet_z", 257), ("tiny_far", 257), ("mixed_extents", 257)]
case_id = lambda c: "-".join(str(x) for x in c)


class reinsert_passes:
    """MIPT_REINSERT_PASSES is read when a context is created."""
    def __init__(self, passes): self.passes = passes

    def __enter__(self):
        self.before = os.environ.get("MIPT_REINSERT_PASSES")
        os.environ["MIPT_REINSERT_PASSES"] = str(self.passes)

    def __exit__(self, *exc):
        if self.before is None: os.environ.pop("MIPT_REINSERT_PASSES", None)
        else: os.environ["MIPT_REINSERT_PASSES"] = self.before


def read_and_compare(r, s, predicted, label, fallbacks=0):
    tree = accel_read(r)
    info = tree[0]
    found = br.compare(tree, predicted)
    print("%s: %d triangles, %d wide nodes (predicted %d), stack_need %d, fallbacks %d: %d findings" %
          (label, info[ar.INFO_N_TRIS], info[ar.INFO_WIDE_NODES], len(predicted["cnt"]), info[ar.INFO_STACK_NEED], info[ar.INFO_FALLBACKS], len(found)))
    for line in found[:10]: print("   ", line)
    assert found == [], found[:10]
    assert ar.check_tree(*tree, ar.scene_rows(s)) == []
    assert info[ar.INFO_FALLBACKS] == fallbacks and r.stats().accel_builder_fallbacks == fallbacks
    return tree


def build_and_compare(R, builder, s, label, passes=8, fallbacks=0, predicted=None):
    t0 = time.perf_counter()
    if predicted is None: predicted = br.predict(ar.scene_rows(s), builder, passes=passes)
    t1 = time.perf_counter()
    with reinsert_passes(passes):
        r = R()
    try:
        r.set_accel_builder(builder)
        s.upload(r); r.build_accel()
        tree = read_and_compare(r, s, predicted, "%s %s" % (BUILDER_NAMES[builder], label), fallbacks)
        assert tree[0][ar.INFO_BUILDER] == builder
        print("    host prediction %.2f s, build, read and checks %.2f s" % (t1 - t0, time.perf_counter() - t1))
        return tree
    finally:
        r.close()


# ---- the stages -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", KEY_CASES, ids=[case_id(c) for c in KEY_CASES])
def test_the_sorted_morton_keys_are_the_restated_ones(R, kind, n):
    s = SCENES[kind](n)
    lo, hi, _ = br.world_boxes(ar.scene_rows(s))
    want = np.sort(br.morton_keys(lo, hi))
    r = R()
    try:
        r.set_accel_builder(abi.BUILDER_LBVH)
        s.upload(r); r.build_accel()
        got = accel_keys(r)
    finally:
        r.close()
    bad = np.nonzero(got != want)[0]
    print("%s %d: %d of %d keys differ%s" % (kind, n, len(bad), len(want), "" if not len(bad) else ", first: key %d is %#x, restated %#x" % (bad[0], got[bad[0]], want[bad[0]])))
    assert got.shape == want.shape and len(bad) == 0
    if kind.startswith("sheet"): assert len(np.unique(want)) > n // 2                   # the flat axis took nothing from the other two


def test_the_keys_are_refused_after_a_refit_and_given_again_by_a_rebuild(R):
    s = soup_scene(257, 1257)
    r = R()
    try:
        r.set_accel_builder(abi.BUILDER_LBVH)
        h = s.upload(r); r.build_accel()
        first = accel_keys(r)
        table = [abi.PtInstanceDesc.from_buffer_copy(bytes(d)) for d in h["instances"]]
        table[0].gpu.transform[12] += 0.25
        r.set_instances(table); r.build_accel()
        assert r.stats().accel_refits == 1
        with pytest.raises(RuntimeError, match="refit"): accel_keys(r)
        r.request_rebuild(); r.build_accel()
        again = accel_keys(r)
        assert again.shape == first.shape and not np.array_equal(again, first)
    finally:
        r.close()


@pytest.mark.parametrize("kind,n", LBVH_CASES, ids=[case_id(c) for c in LBVH_CASES])
def test_the_radix_tree_is_the_restated_one(R, kind, n):
    build_and_compare(R, abi.BUILDER_LBVH, SCENES[kind](n), "%s %d" % (kind, n))


@pytest.mark.parametrize("kind,n", PLOC_CASES, ids=[case_id(c) for c in PLOC_CASES])
def test_the_clustered_tree_is_the_restated_one(R, kind, n):
    build_and_compare(R, abi.BUILDER_PLOC, SCENES[kind](n), "%s %d" % (kind, n))


@pytest.mark.parametrize("kind,n,passes", REINSERT_CASES, ids=[case_id(c) for c in REINSERT_CASES])
def test_the_reinserted_tree_is_the_restated_one(R, kind, n, passes):
    s = SCENES[kind](n)
    rows = ar.scene_rows(s)
    predicted = br.predict(rows, abi.BUILDER_PLOC_REINSERT, passes=passes)
    if passes == 0:                                                                    # no pass: the clustered tree
        assert br.compare(br.as_device_tree(br.predict(rows, abi.BUILDER_PLOC)), predicted) == []
    build_and_compare(R, abi.BUILDER_PLOC_REINSERT, s, "%s %d, %d passes" % (kind, n, passes), passes=passes, predicted=predicted)


def test_a_smaller_build_in_a_used_scratch_is_the_restated_tree(R):
    """58199 triangles without a pass (the restated reinsertion is per node in Python), then 257 and 5 with 8: reinsert_passes is read at context
    creation, so the passes are switched by the builder -- PLOC for the large build, PLOC + reinsertion for the small ones, one scratch."""
    with reinsert_passes(8):
        r = R()
    try:
        for k, (n, builder) in enumerate(((58199, abi.BUILDER_PLOC), (257, abi.BUILDER_PLOC_REINSERT), (5, abi.BUILDER_PLOC_REINSERT))):
            s = soup_scene(n, 2000 + n)
            r.set_accel_builder(builder)
            s.upload(r); r.build_accel()
            tree = read_and_compare(r, s, br.predict(ar.scene_rows(s), builder, passes=8), "%s after %d builds, soup %d" % (BUILDER_NAMES[builder], k, n))
            assert tree[0][ar.INFO_SEG_LEAVES] == 131072 and r.stats().accel_builds == k + 1
    finally:
        r.close()


def test_a_clustering_that_gives_up_builds_the_radix_tree(R):
    s = monotone_strip()
    assert s.triangles == 12001
    build_and_compare(R, abi.BUILDER_PLOC, s, "monotone strip", fallbacks=1, predicted=br.predict_fallback(ar.scene_rows(s)))
