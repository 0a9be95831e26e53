"""tests/accel_ref.py can fail: no GPU, nothing compiled.

A small host builder -- median split of the centroids, the greedy collapse (open the inner child with the largest box until four children or
only leaves; a subtree of at most kLeafMax triangles is one leaf), children in decreasing area, accel_ref.quantise for the bytes -- writes
the arrays pt_debug_accel_read returns for soups of 2, 5, 40 and 300 triangles in two instances; check_tree finds nothing in them.  Then one
mutation at a time, each of which check_tree must report under its own name (accel_ref's docstring lists the names and where each bound
comes from).  The containment and tightness checks are separate expressions from quantise(), so the builder's trees also check the
restated quantiser against them.  Last, the worked example of tests/host/slab_check.cpp: origin 2^-10 + 2^-33, step 2^-8, a bound at
2^-10 + 200 * 2^-8 -- the float plane of byte 200 equals the bound, the exact plane is 2^-33 past it: only the float64 check may see it."""
import numpy as np
import pytest

from tests import accel_ref as ar

f32, u32, u8 = np.float32, np.uint32, np.uint8
SIZES = (2, 5, 40, 300)


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-4, 4, (n, 1, 3))
    return (c + rng.normal(0, 0.3, (n, 3, 3))).astype(f32)


def host_build(P):
    """P [n, 3, 3] float32 -> (info, nodes, ranges, tris, shade, scene rows): two instances with identity transforms, the first n // 2 triangles and the rest."""
    n = len(P); half = n // 2
    cen = (P.min(axis=1).astype(np.float64) + P.max(axis=1)) / 2
    order = []

    def split(ids):                                                      # -> (first, count, left, right) over the order being written
        if len(ids) == 1: order.append(int(ids[0])); return (len(order) - 1, 1, None, None)
        a = int(np.argmax(cen[ids].max(axis=0) - cen[ids].min(axis=0)))
        ids = ids[np.argsort(cen[ids, a], kind="stable")]
        first = len(order); l = split(ids[:len(ids) // 2]); r = split(ids[len(ids) // 2:])
        return (first, len(ids), l, r)

    top = split(np.arange(n))
    order = np.array(order)
    tris = np.zeros((n, 16), u32); shade = np.zeros((n, 32), u32)
    V = P[order]
    tris[:, 0:3] = V[:, 0].view(u32); tris[:, 4:7] = (V[:, 1] - V[:, 0]).astype(f32).view(u32); tris[:, 8:11] = (V[:, 2] - V[:, 0]).astype(f32).view(u32)
    tris[:, 3] = order >= half; tris[:, 7] = np.where(order >= half, order - half, order); tris[:, 11] = 1
    for k in range(3): shade[:, 4 * k:4 * k + 3] = V[:, k].view(u32)
    shade[:, 18] = tris[:, 3]
    # the second instance has all four optional streams (non-zero words, one value per vertex and field), the first has none: zeros
    nv = 3 * (n - half)
    rng = np.random.default_rng(n)
    streams = {"tangent": rng.integers(1, 2 ** 32, nv, dtype=np.uint64).astype(u32), "uv0": rng.uniform(0.1, 1, (nv, 2)).astype(f32),
               "uv1": rng.uniform(1.1, 2, (nv, 2)).astype(f32), "color": rng.integers(1, 2 ** 32, (nv, 2), dtype=np.uint64).astype(u32)}
    second = np.nonzero(order >= half)[0]
    corner = 3 * (order[second] - half)[:, None] + np.arange(3)[None, :]                       # [packets of the second instance, 3] vertex
    shade[second[:, None], np.array(ar.SHADE_TANGENT)[None, :]] = streams["tangent"][corner]
    for name, at in (("uv0", ar.SHADE_UV0), ("uv1", ar.SHADE_UV1), ("color", ar.SHADE_COLOR)):
        shade[second, at:at + 6] = streams[name].view(u32)[corner].reshape(-1, 6)
    lo_t, hi_t = ar.tri_boxes(tris)
    box = lambda b: (lo_t[b[0]:b[0] + b[1]].min(axis=0), hi_t[b[0]:b[0] + b[1]].max(axis=0))
    key = lambda b: float(ar.area_key(*box(b)))
    inner = lambda b: b[1] > ar.K_LEAF_MAX
    rows, queue, need_max = [], [(top, 0)], 0                             # breadth first: a node's index is its place in the queue
    while len(rows) < len(queue):
        b, need_in = queue[len(rows)]
        kids = [b[2], b[3]]
        while len(kids) < 4 and any(inner(k) for k in kids):
            pick = max((k for k in kids if inner(k)), key=key)
            at = kids.index(pick); kids[at] = pick[2]; kids.append(pick[3])
        kids.sort(key=key, reverse=True)
        need = need_in + len(kids) - 1; need_max = max(need_max, need)
        refs = []
        for k in kids:
            if inner(k): refs.append(len(queue)); queue.append((k, need))
            else: refs.append(~(k[0] | (k[1] - 1) << 28))
        rows.append((kids, refs))
    W = len(rows)
    lo = np.zeros((W, 4, 3), f32); hi = np.zeros((W, 4, 3), f32); child = np.full((W, 4), ar.K_EMPTY, np.int64); ranges = np.zeros((W, 8), u32)
    for w, (kids, refs) in enumerate(rows):
        for k, (b, ref) in enumerate(zip(kids, refs)):
            lo[w, k], hi[w, k] = box(b); child[w, k] = ref; ranges[w, k] = b[0]; ranges[w, 4 + k] = b[1]
    cnt = np.array([len(kids) for kids, _ in rows])
    o, e, ql, qh = ar.quantise(lo, hi, cnt)
    nodes = ar.node_bytes(o, e, child, ql, qh)
    ident = np.eye(4, dtype=f32).reshape(-1)
    scene = [{"positions": P[:half].reshape(-1, 3), "indices": None, "transform": ident, "mask_flags": 1, "triangles": half},
             dict({"positions": P[half:].reshape(-1, 3), "indices": None, "transform": ident, "mask_flags": 1, "triangles": n - half}, **streams)]
    info = np.array([n, W, 0, need_max, 256, 0, 0, 1], u32)
    return info, nodes, ranges, tris, shade, scene


@pytest.fixture(scope="module")
def trees():
    return {n: host_build(soup(n, 100 + n)) for n in SIZES}


def parts(tree):
    """The tree decoded, with the children's boxes and the exact planes."""
    info, nodes, ranges, tris, shade, scene = tree
    origin, exps, child, qlo, qhi = ar.decode_nodes(nodes)
    used = child != ar.K_EMPTY
    r = ranges.astype(np.int64)
    lo = np.zeros(qlo.shape, f32); hi = np.zeros(qlo.shape, f32)
    lo_t, hi_t = ar.tri_boxes(tris)
    lo[used], hi[used] = ar.range_boxes(lo_t, hi_t, r[:, 0:4][used], r[:, 4:8][used])
    step = ar.step_of(exps)[:, None, :]
    p_lo = origin.astype(np.float64)[:, None, :] + qlo * step; p_hi = origin.astype(np.float64)[:, None, :] + qhi * step
    return dict(origin=origin, exps=exps, child=child, qlo=qlo, qhi=qhi, used=used, lo=lo, hi=hi, step=np.broadcast_to(step, lo.shape), p_lo=p_lo, p_hi=p_hi)


def q_byte(w, k, a, hi):
    return ar.Q_OFFSET + 8 * a + (4 if hi else 0) + k


def first_of(mask, what):
    at = np.argwhere(mask)
    assert len(at), "no place for the mutation: " + what
    return tuple(int(x) for x in at[0])


def copy_of(tree):
    return tuple(x.copy() if isinstance(x, np.ndarray) else x for x in tree)


@pytest.mark.parametrize("n", SIZES)
def test_the_host_builders_trees_check_clean(trees, n):
    info, nodes, ranges, tris, shade, scene = trees[n]
    stats = {}
    assert ar.check_tree(info, nodes, ranges, tris, shade, scene, stats) == []
    assert stats["node_count"] == info[1] and sum(stats["children"]) == info[1]
    print(n, "triangles:", stats)


# ---- one mutation each --------------------------------------------------------------------------------------------------------------------
def m_qhi_lowered(t, p):
    w, k, a = first_of(p["used"][:, :, None] & (p["qhi"] > 0) & (p["p_hi"] - p["step"] < p["hi"]), "a tight hi plane")
    t[1][w, q_byte(w, k, a, True)] -= 1


def m_qlo_raised(t, p):
    w, k, a = first_of(p["used"][:, :, None] & (p["qlo"] < 255) & (p["p_lo"] + p["step"] > p["lo"]), "a tight lo plane")
    t[1][w, q_byte(w, k, a, False)] += 1


def m_qlo_loose(t, p):
    w, k, a = first_of(p["used"][:, :, None] & (p["qlo"] >= 2), "a lo byte of at least 2")
    t[1][w, q_byte(w, k, a, False)] -= 2


def m_exponent(t, p):
    w, a = first_of((p["exps"] > 1) & (p["exps"] < 250), "an axis with extent")
    t[1][w, 12 + a] += 2


def m_range_shifted(t, p):
    t[2][len(t[2]) - 1, 1] += 1


def m_leaf_duplicated(t, p):
    leaf = p["used"] & (p["child"] < 0)
    w, = first_of(leaf.sum(axis=1) >= 2, "a node with two leaves")
    k0, k1 = np.nonzero(leaf[w])[0][:2]
    t[1][w, 16 + 4 * k1:20 + 4 * k1] = t[1][w, 16 + 4 * k0:20 + 4 * k0]


def m_triangle_dropped(t, p):
    t[3][0] = t[3][1]; t[4][0] = t[4][1]


def m_children_swapped(t, p):
    key = ar.area_key(p["lo"], p["hi"])
    w, k = first_of(p["used"][:, 1:] & (key[:, :-1] > key[:, 1:]), "two children of different area")
    b = t[1][w]
    c0, c1 = 16 + 4 * k, 20 + 4 * k
    b[c0:c0 + 4], b[c1:c1 + 4] = b[c1:c1 + 4].copy(), b[c0:c0 + 4].copy()
    for off in range(ar.Q_OFFSET, ar.Q_OFFSET + 24, 4): b[off + k], b[off + k + 1] = b[off + k + 1], b[off + k]
    r = t[2][w]
    for base in (0, 4): r[base + k], r[base + k + 1] = r[base + k + 1], r[base + k]


def m_stack_need(t, p):
    t[0][ar.INFO_STACK_NEED] -= 1


def m_shade_inst(t, p):
    t[4][len(t[4]) // 2, 18] ^= 1


def of_second_instance(t):
    """A packet of the second instance (the one with the optional streams), and one of the first."""
    inst = t[3][:, 3]
    return int(np.nonzero(inst == 1)[0][-1]), int(np.nonzero(inst == 0)[0][0])


def m_shade_tangent(t, p):
    t[4][of_second_instance(t)[0], ar.SHADE_TANGENT[1]] ^= 1 << 20                    # the second vertex's packed word


def m_shade_uv0(t, p):
    t[4][of_second_instance(t)[0], ar.SHADE_UV0 + 5] ^= 1                              # the last ulp of the third vertex's v


def m_shade_uv1(t, p):
    t[4][of_second_instance(t)[0], ar.SHADE_UV1] ^= 1


def m_shade_color(t, p):
    t[4][of_second_instance(t)[0], ar.SHADE_COLOR + 3] ^= 1 << 31


def m_shade_stale_uv(t, p):
    """The words of another vertex of the same stream: what a refit that skipped the packet after an index rewrite would leave."""
    at = of_second_instance(t)[0]
    t[4][at, ar.SHADE_UV0:ar.SHADE_UV0 + 2], t[4][at, ar.SHADE_UV0 + 2:ar.SHADE_UV0 + 4] = t[4][at, ar.SHADE_UV0 + 2:ar.SHADE_UV0 + 4].copy(), t[4][at, ar.SHADE_UV0:ar.SHADE_UV0 + 2].copy()


MUTATIONS = [(m_shade_tangent, "tri.shade_tangent"), (m_shade_uv0, "tri.shade_uv0"), (m_shade_uv1, "tri.shade_uv1"), (m_shade_color, "tri.shade_color"),
             (m_shade_stale_uv, "tri.shade_uv0"), (m_qhi_lowered, "contain.exact_hi"), (m_qlo_raised, "contain.exact_lo"), (m_qlo_loose, "tight.lo"), (m_exponent, "tight.exp"),
             (m_range_shifted, "ranges"), (m_leaf_duplicated, "shape.leaf_tiling"), (m_triangle_dropped, "tri.multiset"),
             (m_children_swapped, "order"), (m_stack_need, "stack_need"), (m_shade_inst, "tri.shade_inst")]
# what else a mutation may set off: a changed byte is also not what the restated quantiser writes, a lowered hi or raised lo plane may also
# fail in float, a larger step lifts the hi planes off their boxes, a leaf named twice leaves its recorded range and its box wrong
ALSO = {"contain.exact_hi": {"quantise", "contain.float_hi"}, "contain.exact_lo": {"quantise", "contain.float_lo"}, "tight.lo": {"quantise"},
        "tight.exp": {"quantise", "tight.hi", "tight.lo", "contain.exact_lo", "contain.float_lo"}}
BOXES = {"quantise", "contain.exact_lo", "contain.exact_hi", "contain.float_lo", "contain.float_hi", "tight.lo", "tight.hi", "origin", "order", "tight.exp", "tight.flat"}
ALSO["tri.multiset"] = BOXES                     # (the packet that took the dropped one's place has another box)
ALSO["shape.leaf_tiling"] = BOXES | {"ranges"}


@pytest.mark.parametrize("n", (5, 40, 300))
@pytest.mark.parametrize("mutate,name", MUTATIONS, ids=[name + ("-stale" if m is m_shade_stale_uv else "") for m, name in MUTATIONS])
def test_each_mutation_is_reported_under_its_own_name(trees, n, mutate, name):
    t = copy_of(trees[n])
    mutate(t, parts(trees[n]))
    found = ar.check_tree(*t)
    got = set(ar.names(found))
    assert name in got, (name, found)
    assert got <= {name} | ALSO.get(name, set()), (name, found)


def test_the_order_is_demanded_only_of_the_nodes_named(trees):
    """After a refit the slots keep the build's order: check_tree(ordered=) leaves the other nodes' order alone, and nothing else."""
    t = copy_of(trees[40])
    m_children_swapped(t, parts(trees[40]))
    swapped = np.array([(a != b).any() for a, b in zip(t[1], trees[40][1])])
    assert swapped.sum() == 1 and ar.names(ar.check_tree(*t)) == ["order"]
    assert ar.check_tree(*t, None, ~swapped) == []
    assert ar.names(ar.check_tree(*t, None, swapped)) == ["order"]


def test_the_two_triangle_tree_reports_what_it_can(trees):
    """Two leaves under one node: the mutations that need no inner structure."""
    for mutate, name in ((m_stack_need, "stack_need"), (m_shade_inst, "tri.shade_inst"), (m_triangle_dropped, "tri.multiset"), (m_range_shifted, "ranges"),
                         (m_shade_tangent, "tri.shade_tangent"), (m_shade_uv0, "tri.shade_uv0"), (m_shade_uv1, "tri.shade_uv1"), (m_shade_color, "tri.shade_color")):
        t = copy_of(trees[2])
        mutate(t, parts(trees[2]))
        assert name in ar.names(ar.check_tree(*t)), name


@pytest.mark.parametrize("word,name", [(ar.SHADE_TANGENT[0], "tri.shade_tangent"), (ar.SHADE_UV0 + 1, "tri.shade_uv0"), (ar.SHADE_UV1 + 4, "tri.shade_uv1"),
                                       (ar.SHADE_COLOR + 5, "tri.shade_color")])
def test_a_word_of_a_stream_the_instance_lacks_must_be_zero(trees, word, name):
    """The first instance has none of the four streams: its packets hold zeros there, and one set bit is reported under the field's name."""
    t = copy_of(trees[40])
    t[4][of_second_instance(t)[1], word] = 1
    assert ar.names(ar.check_tree(*t)) == [name]


def test_an_indexed_row_is_checked_at_the_vertex_its_index_names(trees):
    """The same arrays against a scene row that reaches the same vertices through an index stream: clean; with two indices of one triangle
    exchanged (a rewritten index stream that the packets did not follow): the positions and every stream of that packet are reported."""
    info, nodes, ranges, tris, shade, scene = copy_of(trees[40])
    row = dict(scene[1]); nv = len(row["positions"])
    perm = np.random.default_rng(7).permutation(nv)
    back = np.empty(nv, np.int64); back[perm] = np.arange(nv)
    for key in ("positions",) + ar.STREAMS: row[key] = row[key][perm]
    row["indices"] = back
    assert ar.check_tree(info, nodes, ranges, tris, shade, [scene[0], row]) == []
    row["indices"] = back.copy(); row["indices"][[0, 1]] = row["indices"][[1, 0]]
    got = set(ar.names(ar.check_tree(info, nodes, ranges, tris, shade, [scene[0], row])))
    assert {"tri.shade_pos", "tri.shade_tangent", "tri.shade_uv0", "tri.shade_uv1", "tri.shade_color", "tri.transform"} <= got, got


def test_the_worked_example_is_seen_by_the_float64_check_alone():
    p, L = f32(2.0 ** -10 + 2.0 ** -33), f32(2.0 ** -10 + 200 * 2.0 ** -8)
    assert float(p) == 2.0 ** -10 + 2.0 ** -33 and float(L) == 2.0 ** -10 + 200 * 2.0 ** -8
    P = np.array([[(p, 0.0, 0.0), (p + f32(0.0625), 0.25, 0.0), (p, 0.0, 0.5)],
                  [(L, 1.0, 1.0), (L + f32(0.125), 1.5, 1.0), (L, 1.0, 1.25)]], f32)
    tree = host_build(P)
    assert ar.check_tree(*tree) == []
    q = parts(tree)
    w, k = first_of(q["used"] & (q["lo"][:, :, 0] == L), "the child whose box starts at the bound")
    assert q["origin"][w, 0] == p and q["exps"][w, 0] == 127 - 8 and q["qlo"][w, k, 0] == 199          # the exact check took the byte down from 200
    t = copy_of(tree)
    t[1][w, q_byte(w, k, 0, False)] = 200
    exact = 2.0 ** -10 + 2.0 ** -33 + 200 * 2.0 ** -8
    assert f32(exact) == L and exact > float(L)                                                     # the float plane equals the bound, the exact plane is past it
    got = set(ar.names(ar.check_tree(*t)))
    assert "contain.exact_lo" in got and not got & {"contain.float_lo", "contain.float_hi", "contain.exact_hi"}, got
    assert got <= {"contain.exact_lo", "quantise"}, got


def test_a_single_triangle_has_no_node():
    P = soup(1, 5)
    tris = np.zeros((1, 16), u32); shade = np.zeros((1, 32), u32)
    tris[0, 0:3] = P[0, 0].view(u32); tris[0, 4:7] = (P[0, 1] - P[0, 0]).view(u32); tris[0, 8:11] = (P[0, 2] - P[0, 0]).view(u32); tris[0, 11] = 1
    for k in range(3): shade[0, 4 * k:4 * k + 3] = P[0, k].view(u32)
    scene = [{"positions": P.reshape(-1, 3), "indices": None, "transform": np.eye(4, dtype=f32).reshape(-1), "mask_flags": 1, "triangles": 1}]
    empty = np.zeros((0, 64), u8)
    assert ar.check_tree([1, 0, 0xffffffff, 0, 256, 0, 0, 1], empty, np.zeros((0, 32), u8), tris, shade, scene) == []
    assert ar.names(ar.check_tree([1, 0, 0, 0, 256, 0, 0, 1], empty, np.zeros((0, 32), u8), tris, shade, scene)) == ["shape.root"]
    assert ar.names(ar.check_tree([1, 1, 0, 0, 256, 0, 0, 1], np.zeros((1, 64), u8), np.zeros((1, 32), u8), tris, shade, scene)) == ["shape.root"]
