"""tests/builder_ref.py means something: no GPU, nothing compiled.

  validity     the restated tree of every builder is a valid wide tree at 2 .. 2049 triangles
  definitions  radix_tree (recursive: split at the highest differing bit of the augmented keys) is the tree of Karras's formula (direction, upper
               bound by doubling, binary search, split), transcribed here from the paper
  sensitivity  each deliberately wrong builder gives a tree that compare() tells from the right one on a scene of tests/test_gpu_builder_topology.py
               -- so a device bug of that kind could not pass there.  SENSITIVITY names the scene that catches each
  reinsertion  moves something on every soup where something can be gained, and never ends with more inner-node area than the clustering
  compare      reports under the right name

The whole file takes a few seconds: the reinsertion search is vectorised over the nodes, so the sizes of the GPU test (up to 1025) are kept.

Inner-node area in root areas (sum of the inner boxes' area keys over the root's; the reinsertion test prints them), radix tree / clustered /
reinserted (moves): soup 4: 1.8223 / 1.4979 / 1.4979 (0); 5: 1.9863 / 1.6911 / 1.6911 (0); 7: 2.2066 / 1.7212 / 1.7212 (0); 13: 3.4954 / 2.6614 /
2.5989 (2); 64: 6.0965 / 5.7936 / 5.2734 (9); 65: 5.9413 / 5.3988 / 5.2388 (14); 257: 10.8699 / 10.4462 / 9.5648 (74); 1025: 18.9678 / 18.4702 /
16.9472 (249).  At 4, 5 and 7 triangles nothing moves because nothing is to be gained: an exhaustive search over every single reinsertion finds
no tree of lower area, which the test checks instead of demanding a move there."""
import numpy as np
import pytest

from tests import accel_ref as ar
from tests import builder_ref as br
from tests.test_gpu_builder_topology import SCENES, LBVH_CASES, PLOC_CASES, REINSERT_CASES

LBVH, PLOC, REINSERT = br.BUILDER_LBVH, br.BUILDER_PLOC, br.BUILDER_PLOC_REINSERT
NAMES = {LBVH: "lbvh", PLOC: "ploc", REINSERT: "reinsert"}
_rows, _right = {}, {}


def rows_of(kind, n):
    if (kind, n) not in _rows: _rows[kind, n] = ar.scene_rows(SCENES[kind](n))
    return _rows[kind, n]


def right_tree(kind, n, builder):
    """The prediction and its stages, computed once and left unchanged."""
    if (kind, n, builder) not in _right:
        stages = {}
        _right[kind, n, builder] = (br.predict(rows_of(kind, n), builder, stages=stages), stages)
    return _right[kind, n, builder]


# ---- validity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", (LBVH, PLOC, REINSERT), ids=lambda b: NAMES[b])
@pytest.mark.parametrize("n", (2, 3, 4, 5, 7, 13, 257, 2049))
def test_the_restated_tree_is_a_valid_tree(builder, n):
    w, stages = right_tree("soup", n, builder)
    W = len(w["cnt"])
    used = np.arange(4)[None, :] < w["cnt"][:, None]
    assert ((w["cnt"] >= 2) & (w["cnt"] <= 4)).all()
    assert not (used & ~w["leaf"] & (w["cnt"] < 4)[:, None]).any()                     # fewer than four children: only leaves
    assert ((w["count"][used & w["leaf"]] >= 1) & (w["count"][used & w["leaf"]] <= br.K_LEAF_MAX)).all() and (w["count"][used & ~w["leaf"]] > br.K_LEAF_MAX).all()
    cover = np.zeros(n + 1, np.int64)                                                 # the leaf ranges tile [0, n)
    np.add.at(cover, w["first"][used & w["leaf"]], 1); np.add.at(cover, (w["first"] + w["count"])[used & w["leaf"]], -1)
    assert (np.cumsum(cover)[:n] == 1).all()
    kids = w["child"][used & ~w["leaf"]]                                               # every node but the root is the child of exactly one slot
    assert sorted(kids.tolist()) == list(range(1, W)) and (w["child"][~(used & ~w["leaf"])] == -1).all()
    for v in range(W):                                                                # an inner child's node covers the child's range
        for k in range(4):
            c = w["child"][v, k]
            if c >= 0:
                u = np.arange(4) < w["cnt"][c]
                assert w["first"][c][u].min() == w["first"][v, k] and w["count"][c][u].sum() == w["count"][v, k]
    assert sorted(map(tuple, w["ids"].tolist())) == sorted(map(tuple, stages["ids"].tolist()))
    assert br.compare(br.as_device_tree(w), w) == []


# ---- the radix tree, two definitions ------------------------------------------------------------------------------------------------------------
def karras_tree(keys):
    """Karras 2012, section 4, for sorted keys with ties broken by the index: delta(i, j) is the length of the common prefix of keys i and j, of
    the indices' too when the keys are equal, -1 outside the array.  Inner node i: direction d = sign(delta(i, i + 1) - delta(i, i - 1)); the
    other end j by doubling an upper bound on the length and a binary search for the last k with delta(i, k) > delta(i, i - d); the split by
    a binary search for the last position that shares more than delta(i, j) with i.  Children: leaves where the split meets an end."""
    n = len(keys); keys = [int(k) for k in keys]

    def delta(i, j):
        if j < 0 or j >= n: return -1
        x = keys[i] ^ keys[j]
        return 64 - x.bit_length() if x else 64 + 32 - (i ^ j).bit_length()

    left, right = [0] * (n - 1), [0] * (n - 1)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin: lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin: l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while t > 1:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode: s += t
        gamma = i + s * d + min(d, 0)
        left[i] = gamma if min(i, j) == gamma else n + gamma
        right[i] = gamma + 1 if max(i, j) == gamma + 1 else n + gamma + 1
    return br.Tree(n, left, right, n)


def shape_of(tree):
    """{(first, count, count of the left child)} over the inner nodes: the tree, whatever its nodes are called."""
    lay = br.layout(tree)
    assert np.array_equal(lay["perm"], np.arange(tree.n))                             # a radix tree keeps the sorted order
    n = tree.n
    return {(int(lay["first"][n + t]), int(lay["count"][n + t]), int(lay["count"][tree.left[t]])) for t in range(n - 1)}


def duplicate_keys(n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(0, 1 << 63, max(n // 40, 2), dtype=np.uint64)[rng.integers(0, max(n // 40, 2), n)])


@pytest.mark.parametrize("n", (2, 3, 257, 2049))
@pytest.mark.parametrize("kind", ("soup", "duplicates", "all_equal"))
def test_the_recursive_radix_tree_is_karrass(kind, n):
    if kind == "soup": keys = np.sort(right_tree("soup", n, LBVH)[1]["keys"])
    elif kind == "duplicates": keys = duplicate_keys(n, n)
    else: keys = np.full(n, 0x123456789abcdef, np.uint64)
    if kind == "duplicates" and n > 100: assert len(np.unique(keys)) * 10 < n
    a, b = shape_of(br.radix_tree(keys)), shape_of(karras_tree(keys))
    assert a == b and len(a) == n - 1


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------------------------
# what is wrong -> (builder, the wrong builder's options, the scene of the GPU test that catches it)
SENSITIVITY = {
    "morton axes x and y swapped": (LBVH, dict(axes=(1, 0, 2)), ("soup", 257)),
    "morton axes y and z swapped": (LBVH, dict(axes=(0, 2, 1)), ("soup", 257)),
    "morton axes x and z swapped": (LBVH, dict(axes=(2, 1, 0)), ("sheet_y", 257)),
    "search radius 15": (PLOC, dict(radius=15), ("soup", 241)),
    "search radius 15 to the left, 16 to the right": (PLOC, dict(radius_left=15), ("soup", 273)),
    "search radius 16 to the left, 15 to the right": (PLOC, dict(radius=15, radius_left=16), ("soup", 272)),
    "pair key without the extent sum": (PLOC, dict(use_extent=False), ("block_or_strip", 3)),
    "pair key with the lower index before the index distance": (PLOC, dict(index_before_distance=True), ("coincident", 300)),
    "two lock rounds": (REINSERT, dict(lock_rounds=2), ("soup", 257)),
    "seven passes": (REINSERT, dict(passes=7), ("soup", 257)),
    "no minimum gain": (REINSERT, dict(min_gain=0.0), ("soup", 1025)),
    "a round's temporary nodes numbered from the last pair to the first": (REINSERT, dict(number_descending=True), ("soup", 257)),
    "collapse opens the smallest child (radix tree)": (LBVH, dict(open_largest=False), ("soup", 13)),
    "collapse opens the smallest child (clustered tree)": (PLOC, dict(open_largest=False), ("quads_16x", 16)),
    "sorting network swaps equal keys (radix tree)": (LBVH, dict(strict_network=False), ("coincident", 5)),
    "sorting network swaps equal keys (clustered tree)": (PLOC, dict(strict_network=False), ("quads_1x", 128)),
}
GPU_CASES = {LBVH: LBVH_CASES, PLOC: PLOC_CASES, REINSERT: [c[:2] for c in REINSERT_CASES if c[2] == 8]}


@pytest.mark.parametrize("what", sorted(SENSITIVITY))
def test_a_wrong_builder_is_told_apart_on_a_scene_of_the_gpu_test(what):
    builder, options, scene = SENSITIVITY[what]
    assert scene in GPU_CASES[builder], "the scene is not one the GPU test builds with this builder"
    right, _ = right_tree(scene[0], scene[1], builder)
    wrong = br.predict(rows_of(*scene), builder, **options)
    found = br.compare(br.as_device_tree(wrong), right)
    print("%s: %s %d triangles with %s reports %s" % (what, scene[0], scene[1], NAMES[builder], ar.names(found)))
    assert found != []
    assert br.compare(br.as_device_tree(right), right) == []


# ---- reinsertion ------------------------------------------------------------------------------------------------------------------------------------
def subtree(t, v):
    out, todo = set(), [v]
    while todo:
        v = todo.pop(); out.add(v)
        if v >= t.n: todo += [int(t.left[v - t.n]), int(t.right[v - t.n])]
    return out


def best_single_move(t):
    """Exhaustive: the lowest inner area (float64) any one reinsertion of a movable node can reach, over the tree's own."""
    par = br._parents(t)
    base = br.inner_area(t); best = base
    for u in range(2 * t.n - 1):
        if par[u] < 0 or par[par[u]] < 0: continue
        for o in set(range(2 * t.n - 1)) - subtree(t, u) - {int(par[u]), t.root}:
            m = t.copy(); q = par.copy()
            br.apply_moves(m, q, [u], {u: o}, {u: -1})
            best = min(best, br.inner_area(m))
    return base, best


@pytest.mark.parametrize("n", sorted({c[1] for c in REINSERT_CASES if c[0] == "soup"}))
def test_reinsertion_moves_something_and_does_not_raise_the_area(n):
    area = {}
    for b in (LBVH, PLOC, REINSERT):
        _, st = right_tree("soup", n, b)
        area[b] = br.inner_area(st["tree"], st["layout"])
    ploc, after = right_tree("soup", n, PLOC)[1]["tree"], right_tree("soup", n, REINSERT)[1]["tree"]
    print("soup %d: inner area in root areas: radix tree %.4f, clustered %.4f, reinserted %.4f (%d moves)" % (n, area[LBVH], area[PLOC], area[REINSERT], after.moves))
    assert area[REINSERT] <= area[PLOC]
    if after.moves == 0:
        # nothing moved: then nothing is to be gained -- no single reinsertion lowers the clustered tree's area (exhaustive; feasible because such trees are tiny)
        assert n <= 7
        base, best = best_single_move(ploc)
        print("    the best single move of all reaches %.6f of %.6f" % (best, base))
        assert best >= base * (1 - 1e-3)
    else:
        assert area[REINSERT] < area[PLOC]
    assert br.compare(br.as_device_tree(br.predict(rows_of("soup", n), REINSERT, passes=0)), right_tree("soup", n, PLOC)[0]) == []


def test_the_exhaustive_search_can_find_a_move():
    """... so that finding none above means something: on the 13-triangle soup, where the restated reinsertion moves, it finds a better tree too."""
    base, best = best_single_move(right_tree("soup", 13, PLOC)[1]["tree"])
    assert best < base * (1 - 1e-3)


# ---- compare ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", (LBVH, REINSERT), ids=lambda b: NAMES[b])
def test_compare_reports_under_the_right_name(builder):
    right, _ = right_tree("soup", 257, builder)
    info, nodes, ranges, tris, shade = br.as_device_tree(right)
    assert br.compare((info, nodes, ranges, tris, shade), right) == []
    t = tris.copy(); t[[10, 11]] = t[[11, 10]]                                        # two adjacent triangles swapped
    assert ar.names(br.compare((info, nodes, ranges, t, shade), right)) == ["order.triangles"]
    v = int(np.nonzero(right["cnt"] == 4)[0][0])                                      # two child slots of one node swapped: references and ranges
    nd = nodes.copy().view(np.int32).reshape(-1, 16); rg = ranges.copy().view(np.uint32).reshape(-1, 8)
    nd[v, [4, 5]] = nd[v, [5, 4]]; rg[v, [0, 1]] = rg[v, [1, 0]]; rg[v, [4, 5]] = rg[v, [5, 4]]
    assert ar.names(br.compare((info, nd.view(np.uint8).reshape(-1, 64), rg.view(np.uint8).reshape(-1, 32), tris, shade), right)) == ["topology.slot"]
    nd = nodes.copy().view(np.int32).reshape(-1, 16)                                  # a child dropped
    nd[v, 7] = br.K_EMPTY
    assert "topology.children" in ar.names(br.compare((info, nd.view(np.uint8).reshape(-1, 64), ranges, tris, shade), right))
    rg = ranges.copy().view(np.uint32).reshape(-1, 8)                                 # a boundary between two children moved
    rg[v, 4] += 1
    assert "topology.range" in ar.names(br.compare((info, nodes, rg.view(np.uint8).reshape(-1, 32), tris, shade), right))
    nd = nodes.copy().view(np.int32).reshape(-1, 16)                                  # a leaf reference with another count
    w, k = [int(x) for x in np.argwhere(right["leaf"])[0]]
    nd[w, 4 + k] ^= 1 << 28
    assert ar.names(br.compare((info, nd.view(np.uint8).reshape(-1, 64), ranges, tris, shade), right)) == ["topology.leaf"]
    i2 = info.copy(); i2[3] += 1
    assert ar.names(br.compare((i2, nodes, ranges, tris, shade), right)) == ["stack_need"]
