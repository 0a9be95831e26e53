"""The three BVH builders of csrc/accel.hip restated on the host, stage by stage, and compare(): is the tree the device built THE tree the builder
is meant to build?  (tests/accel_ref.py check_tree asks whether it is A correct tree; the two together pin every byte but the node numbering.)
Plain numpy and Python; it shares no code with csrc/.  Written from the algorithm descriptions in accel.hip's comments, DESIGN.md, Karras 2012
("Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees") and Meister & Bittner 2018 ("Parallel Locally-Ordered Clustering
for Bounding Volume Hierarchy Construction", "Parallel Reinsertion for Bounding Volume Hierarchy Optimization").

The whole build is a deterministic function of the scene: Morton codes are float32 arithmetic in a file compiled without contraction, the sort is
stable, the radix tree breaks ties by index, a clustering round ranks pairs by an integer key made of explicitly rounded float32 areas, a
reinsertion pass resolves conflicts by the maximum of (gain bits, node), the layout is depth first, the collapse greedy by a float32 key with a
fixed sorting network.  The temporary nodes of the clustering are numbered by round and slot (select_moves ranks equal gains by the slot).  Only
the NUMBERING of the wide nodes comes out of atomics, so the wide tree is compared up to that numbering.

A binary tree is a Tree: n leaves in slots [0, n) (leaf i = triangle i of the Morton order) and n - 1 inner nodes in slots [n, 2 n - 1), in any
order; left / right [n - 1] hold the child SLOTS of inner node t = slot n + t; root is a slot; lo / hi [2 n - 1, 3] float32 are the slots' boxes.

Stages (each returns something a test can look at):
  world_boxes(rows)    -> lo, hi [n, 3], ids [n, 2] (inst, prim) in the scene's order: the packets' v0, e1, e2 and their box
  morton_keys(lo, hi)  -> [n] uint64
  sorted_order(keys)   -> [n] the stable order
  radix_tree(keys)     -> Tree over sorted keys, defined recursively
  ploc_tree(lo, hi)    -> Tree by rounds of locally-ordered clustering
  reinsert(tree)       -> Tree after passes of parallel reinsertion; tree.moves counts the moves applied
  layout(tree)         -> the depth-first leaf order and every slot's (first, count)
  collapse(tree)       -> the 4-wide tree ("predicted": what compare() takes)
  predict(rows, builder, **variant) runs them in the product's order
  compare(device_tree, predicted) -> list of "<name>: <detail>", empty when the two are the same tree
"""
from bisect import bisect_left

import numpy as np

from tests.accel_ref import scene_rows, row_vertices, mul_point, tri_boxes, area_key, leaf_first_count  # noqa: F401  (scene_rows: for the callers)

f32, u32, u64, i64 = np.float32, np.uint32, np.uint64, np.int64
K_WIDTH, K_LEAF_MAX, K_EMPTY = 4, 3, 0x7fffffff
BUILDER_LBVH, BUILDER_PLOC, BUILDER_PLOC_REINSERT = 0, 1, 2
AREA_CLAMP = f32(3.0e38)
NETWORK = ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2))


class Tree:
    def __init__(self, n, left, right, root, lo=None, hi=None):
        self.n, self.left, self.right, self.root = n, np.asarray(left, i64), np.asarray(right, i64), int(root)
        self.lo, self.hi, self.moves, self.rounds = lo, hi, 0, 0

    def copy(self):
        t = Tree(self.n, self.left.copy(), self.right.copy(), self.root, None if self.lo is None else self.lo.copy(), None if self.hi is None else self.hi.copy())
        t.moves, t.rounds = self.moves, self.rounds
        return t


# ---- the triangles ------------------------------------------------------------------------------------------------------------------------
def world_boxes(rows):
    """rows: accel_ref.scene_rows().  The packet of a triangle is v0 = mul_point(M, p0), e1 = w1 - w0, e2 = w2 - w0 in float32; its box is the
    min / max of v0, v0 + e1, v0 + e2 (NOT of the three world vertices: v0 + e1 is w1 rounded once more)."""
    lo, hi, ids = [], [], []
    for i, r in enumerate(rows):
        if r["triangles"] == 0: continue
        w = mul_point(r["transform"], row_vertices(r))
        with np.errstate(over="ignore", invalid="ignore"):
            v0, e1, e2 = w[:, 0], (w[:, 1] - w[:, 0]).astype(f32), (w[:, 2] - w[:, 0]).astype(f32)
            a, b = (v0 + e1).astype(f32), (v0 + e2).astype(f32)
        lo.append(np.minimum(np.minimum(v0, a), b)); hi.append(np.maximum(np.maximum(v0, a), b))
        ids.append(np.stack([np.full(r["triangles"], i, i64), np.arange(r["triangles"], dtype=i64)], axis=1))
    return np.concatenate(lo).astype(f32), np.concatenate(hi).astype(f32), np.concatenate(ids)


def _spread21(v):
    """Bit k of v to bit 3 k."""
    out = np.zeros(v.shape, u64)
    for k in range(21): out |= ((v >> u64(k)) & u64(1)) << u64(3 * k)
    return out


def morton_keys(lo, hi, axes=(0, 1, 2)):
    """63-bit Morton code of every box's centroid, bit for bit k_morton's: centroid (lo + hi) * 0.5, scene bounds the min / max of the centroids,
    ext = max(bounds_hi - bounds_lo, 1e-30), q = (c - bounds_lo) / ext, cell = clamp(q * 2^21, 0, 2^21 - 1) truncated, bits interleaved x, y, z
    with x highest.  All float32.  The kernel divides with pt_math.h fdiv, which is the rounded quotient whenever divisor, dividend and quotient
    are normal numbers or the dividend is zero: ext >= 1e-30 is normal, and a quotient too small to be normal lands in cell 0 either way.
    axes: which coordinate goes to the high, middle and low bit (a wrong builder for the sensitivity test)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = ((lo + hi).astype(f32) * f32(0.5)).astype(f32)
        blo, bhi = c.min(axis=0), c.max(axis=0)
        ext = np.maximum((bhi - blo).astype(f32), f32(1e-30))
        q = ((c - blo).astype(f32) / ext).astype(f32)
        cell = np.minimum(np.maximum((q * f32(2097152.0)).astype(f32), f32(0.0)), f32(2097151.0))
        cell = np.where(np.isnan(cell), f32(0.0), cell).astype(u64)
    return (_spread21(cell[:, axes[0]]) << u64(2)) | (_spread21(cell[:, axes[1]]) << u64(1)) | _spread21(cell[:, axes[2]])


def sorted_order(keys):
    return np.argsort(keys, kind="stable")


# ---- the radix tree -----------------------------------------------------------------------------------------------------------------------
def radix_tree(keys):
    """keys: sorted.  The tree over the augmented keys (key << 32 | index), which are distinct: a range [a, b] of the sorted array is one node; it
    splits after the last element that has a 0 at the highest bit in which its first and last augmented key differ (every element before has a 0
    there, every one after a 1: the array is sorted and the bits above are common to the range).  Iterative: coincident triangles chain."""
    n = len(keys)
    aug = [(int(k) << 32) | i for i, k in enumerate(keys)]
    assert all(aug[i] < aug[i + 1] for i in range(n - 1)), "the keys are not sorted"
    left, right, root, made = [0] * (n - 1), [0] * (n - 1), 0, 0
    todo = [(0, n - 1, -1, 0)]
    while todo:
        a, b, parent, side = todo.pop()
        if a == b: slot = a
        else:
            slot = n + made
            bit = (aug[a] ^ aug[b]).bit_length() - 1
            split = bisect_left(aug, (aug[b] >> bit) << bit, a, b + 1) - 1
            todo.append((split + 1, b, made, 1)); todo.append((a, split, made, 0))
            made += 1
        if parent < 0: root = slot
        elif side == 0: left[parent] = slot
        else: right[parent] = slot
    return Tree(n, left, right, root)


# ---- PLOC -------------------------------------------------------------------------------------------------------------------------------
def _clamped_bits(x):
    """Negative, NaN or overflowing values rank last: 3.0e38; then the float's bits (non-negative floats order like their bits)."""
    with np.errstate(invalid="ignore"):
        x = np.where(x >= 0, np.minimum(x, AREA_CLAMP), AREA_CLAMP).astype(f32)
    return x.view(u32).astype(u64)


def _nearest(clo, chi, radius_left, radius_right, use_extent, index_before_distance):
    m = len(clo)
    i = np.arange(m, dtype=i64)
    best_hi = np.full(m, ~u64(0)); best_lo = np.full(m, ~u64(0)); best = i.copy()
    for d in list(range(-radius_left, 0)) + list(range(1, radius_right + 1)):
        g = i + d
        ok = (g >= 0) & (g < m)
        if not ok.any(): continue
        gc = np.clip(g, 0, m - 1)
        with np.errstate(over="ignore", invalid="ignore"):
            e = (np.maximum(chi, chi[gc]) - np.minimum(clo, clo[gc])).astype(f32)
            area = ((e[:, 0] * e[:, 1]).astype(f32) + (e[:, 1] * e[:, 2]).astype(f32)).astype(f32) + (e[:, 2] * e[:, 0]).astype(f32)
            ext = ((e[:, 0] + e[:, 1]).astype(f32) + e[:, 2]).astype(f32)
        key_hi = _clamped_bits(area) << u64(32) | (_clamped_bits(ext) if use_extent else u64(0))
        low = np.minimum(i, gc).astype(u64); dist = u64(abs(d))
        key_lo = (low << u64(8) | dist << u64(1) | (low & u64(1))) if index_before_distance else (dist << u64(33) | (low & u64(1)) << u64(32) | low)
        better = ok & ((key_hi < best_hi) | ((key_hi == best_hi) & (key_lo < best_lo)))
        best_hi = np.where(better, key_hi, best_hi); best_lo = np.where(better, key_lo, best_lo); best = np.where(better, g, best)
    return best


def ploc_tree(lo, hi, radius=16, radius_left=None, use_extent=True, index_before_distance=False, max_rounds=4100, number_descending=False):
    """lo, hi: the triangles' boxes in Morton order.  Rounds over the cluster array: every cluster picks, among the `radius` slots either side, the
    partner whose pair has the smallest key (float32 bits of the union's dx dy + dy dz + dz dx, float32 bits of dx + dy + dz, index distance,
    parity of the lower index, lower index) -- the same key from both ends, a strict total order on pairs; the pairs that picked each other merge
    into the lower slot, whose cluster becomes the left child; the survivors close up in order.  Until one cluster is left.
    The new nodes are numbered round by round, within a round by the pair's upper slot (k_ploc_compact): the reinsertion breaks ties of
    bit-equal gains by the node's slot, so the numbering of the temporary nodes is part of the tree's definition.
    max_rounds: the product looks at the count every four rounds and gives up past 4096 (then the radix tree is built instead): raises GaveUp.
    radius_left, use_extent, index_before_distance, number_descending (a round's new nodes numbered from the last pair to the first): wrong
    builders for the sensitivity test."""
    n = len(lo)
    rl = radius if radius_left is None else radius_left
    clo, chi, slot = np.asarray(lo, f32).copy(), np.asarray(hi, f32).copy(), np.arange(n, dtype=i64)
    left, right, blo, bhi = [], [], [clo.copy()], [chi.copy()]
    rounds = 0
    while len(slot) > 1:
        if rounds >= max_rounds: raise GaveUp("%d clusters after %d rounds" % (len(slot), rounds))
        m = len(slot)
        nn = _nearest(clo, chi, rl, radius, use_extent, index_before_distance)
        i = np.arange(m, dtype=i64)
        mutual = (nn != i) & (nn[nn] == i)
        b = np.nonzero(mutual & (i > nn))[0]; a = nn[b]               # in the order of the upper slots: the numbering of the new nodes
        if number_descending: a, b = a[::-1], b[::-1]
        if len(a) == 0:                                                  # (cannot happen with one radius: the best pair of all picks each other)
            assert rl != radius, "a round merged nothing: the key is not a total order"
            raise GaveUp("no pair merged at %d clusters" % m)
        made = n + len(left) + np.arange(len(a), dtype=i64)
        left.extend(slot[a].tolist()); right.extend(slot[b].tolist())
        clo[a] = np.minimum(clo[a], clo[b]); chi[a] = np.maximum(chi[a], chi[b]); slot[a] = made
        blo.append(clo[a].copy()); bhi.append(chi[a].copy())
        keep = ~(mutual & (i > nn))
        clo, chi, slot = clo[keep], chi[keep], slot[keep]
        rounds += 1
    t = Tree(n, left, right, slot[0], np.concatenate(blo), np.concatenate(bhi))
    t.rounds = rounds
    return t


class GaveUp(Exception):
    pass


# ---- reinsertion ------------------------------------------------------------------------------------------------------------------------
def _area(lo, hi):
    return area_key(lo, hi)


def _parents(t):
    par = np.full(2 * t.n - 1, -1, i64)
    inner = t.n + np.arange(t.n - 1, dtype=i64)
    par[t.left] = inner; par[t.right] = inner
    assert par[t.root] == -1 and (par >= 0).sum() == 2 * t.n - 2
    return par


def find_moves(t, par, min_gain, max_steps=8192):
    """Every node's best place, by the stackless branch-and-bound walk of accel.hip 4c.  THIS is the one place where the restatement follows the
    kernel's order of operations: the running sums d (the gain if `in` went next to the node under the cursor), d_path (the gain from taking it
    out, summed up the path) and best are float32 and rounded at every step, so the order of the additions and the sequence of nodes visited are
    part of the result.  All searches advance in lock step here, one loop iteration of each per step, at most max_steps of them.
    -> gain [S] float32 (0: no move), out [S], top [S] (slots; -1: no move)."""
    n, S = t.n, 2 * t.n - 1
    lo, hi, left, right = t.lo, t.hi, t.left, t.right
    with np.errstate(over="ignore", invalid="ignore"):
        area = _area(lo, hi)
        gp_all = np.where(par >= 0, par[np.maximum(par, 0)], -1)
        U = np.nonzero((par >= 0) & (gp_all >= 0))[0]                   # neither the root nor a child of the root moves
        gain_all, out_all, top_all = np.zeros(S, f32), np.zeros(S, i64), np.full(S, -1, i64)
        if len(U) == 0: return gain_all, out_all, top_all
        p, gp = par[U], gp_all[U]
        ilo, ihi, area_in = lo[U], hi[U], area[U]
        d_path = area[p].copy(); d = d_path.copy()                       # the parent goes away
        best = (f32(min_gain) * d_path).astype(f32)
        best = np.where(best >= 0, best, f32(0)).astype(f32)
        pivot = p.copy(); plo, phi = ilo.copy(), ihi.copy()
        out = np.where(left[p - n] == U, right[p - n], left[p - n])
        down = np.ones(len(U), bool); alive = np.ones(len(U), bool)
        b_out, b_top = np.zeros(len(U), i64), np.full(len(U), -1, i64)
        for _ in range(max_steps):
            A = np.nonzero(alive)[0]
            if len(A) == 0: break
            D, C = A[down[A]], A[~down[A]]
            if len(D):                                                  # down: try `out`, descend into its left child while it can still pay
                o = out[D]
                merged = _area(np.minimum(lo[o], ilo[D]), np.maximum(hi[o], ihi[D]))
                here = (d[D] - merged).astype(f32)
                w = here > best[D]; W = D[w]
                best[W] = here[w]; b_out[W] = o[w]; b_top[W] = np.where(pivot[W] == p[W], gp[W], pivot[W])
                grow = (merged - area[o]).astype(f32)
                rest = (d[D] - grow).astype(f32)
                go = (o >= n) & ((rest - area_in[D]).astype(f32) > best[D])
                G = D[go]
                d[G] = rest[go]; out[G] = left[o[go] - n]
                down[D[~go]] = False
            if len(C):                                                  # up: to the right sibling, or one level up
                o = out[C]; po = par[o]
                done = po == pivot[C]
                from_left = ~done & (left[po - n] == o)
                back = ~done & ~from_left
                X = C[back]; px = po[back]                              # from a right child: undo the growth charged on the way down
                d[X] = (d[X] + (_area(np.minimum(lo[px], ilo[X]), np.maximum(hi[px], ihi[X])) - area[px]).astype(f32)).astype(f32)
                out[X] = px
                X = C[from_left]
                out[X] = right[po[from_left] - n]; down[X] = True
                X = C[done]; ox = o[done]                               # the subtree hanging off `pivot` is done: one ancestor up
                first = pivot[X] == p[X]
                plo[X] = np.where(first[:, None], lo[ox], np.minimum(plo[X], lo[ox])); phi[X] = np.where(first[:, None], hi[ox], np.maximum(phi[X], hi[ox]))
                up = par[pivot[X]]
                alive[X[up < 0]] = False
                Y = X[(up >= 0) & ~first]; upy = par[pivot[Y]]         # this ancestor shrinks; `in` as the sibling of the shrunk ancestor itself
                a_pivot = area[pivot[Y]]
                d_path[Y] = (d_path[Y] + (a_pivot - _area(plo[Y], phi[Y])).astype(f32)).astype(f32)
                here = (d_path[Y] - a_pivot).astype(f32)
                w = here > best[Y]; W = Y[w]
                best[W] = here[w]; b_out[W] = pivot[W]; b_top[W] = upy[w]
                Z = X[up >= 0]; upz = up[up >= 0]
                l = left[upz - n]
                out[Z] = np.where(l == pivot[Z], right[upz - n], l)
                pivot[Z] = upz; d[Z] = d_path[Z]; down[Z] = True
        gain_all[U] = np.where(b_top >= 0, best, f32(0)); out_all[U] = b_out; top_all[U] = b_top
    return gain_all, out_all, top_all


def _path(par, u, o, top, max_links=256):
    """in -> top <- out, top last; None if a side does not reach top within max_links links."""
    nodes = []
    for v in (u, o):
        k = 0
        while k < max_links and v != top:
            nodes.append(v); v = par[v]; k += 1
            if v < 0: return None
        if v != top: return None
    nodes.append(top)
    return nodes


def select_moves(par, gain, out, top, lock_rounds=3):
    """The moves that are carried out.  A move owns the path in -> top <- out.  A lock round: every candidate still in the race drops out for good
    if its path touches a path already won (or is longer than 256 links a side); the others stamp the maximum of (gain bits << 32 | node) on
    every node of their paths; those who then hold their whole path have won and own it.  -> the winners (slots)."""
    par = par.tolist()
    bits = gain.view(u32)
    cands = [int(u) for u in np.nonzero(gain > 0)[0]]
    key = {u: (int(bits[u]) << 32) | u for u in cands}
    owned, winners = set(), []
    for _ in range(lock_rounds):
        lock, live = {}, []
        for u in cands:
            nodes = _path(par, u, int(out[u]), int(top[u]))
            if nodes is None or any(v in owned for v in nodes): continue
            live.append((u, nodes))
            for v in nodes:
                if lock.get(v, 0) < key[u]: lock[v] = key[u]
        cands = []
        for u, nodes in live:
            if all(lock[v] == key[u] for v in nodes): winners.append(u); owned.update(nodes)
            else: cands.append(u)
    return winners


def apply_moves(t, par, winners, out, top, max_links=256):
    """The winners' paths are disjoint, so the order does not matter.  Taking `in` out: its sibling takes the parent's place under the
    grandparent.  Putting it in: the freed parent goes between `out` and out's parent, with `out` left and `in` right.  Then the boxes on the
    two sides of the path, up to but not including top."""
    n, left, right, lo, hi = t.n, t.left, t.right, t.lo, t.hi
    for u in winners:
        p = par[u]; g = par[p]; o = out[u]
        s = right[p - n] if left[p - n] == u else left[p - n]
        if left[g - n] == p: left[g - n] = s
        else: right[g - n] = s
        par[s] = g
        po = par[o]
        if left[po - n] == o: left[po - n] = p
        else: right[po - n] = p
        par[p] = po; left[p - n] = o; right[p - n] = u; par[o] = p
        for v in (g, p):
            k = 0
            while k < max_links and v >= 0 and v != top[u]:
                a, b = left[v - n], right[v - n]
                lo[v] = np.minimum(lo[a], lo[b]); hi[v] = np.maximum(hi[a], hi[b])
                v = par[v]; k += 1


def reinsert(tree, passes=8, min_gain=1e-3, lock_rounds=3):
    """Meister & Bittner's parallel reinsertion as accel.hip 4c describes it: `passes` times find_moves (whose docstring says where it follows the
    kernel's order of operations), select_moves, apply_moves.  Trees of fewer than four leaves are left alone, as the product leaves them."""
    t = tree.copy()
    if t.n < 4: return t
    par = _parents(t)
    for _ in range(passes):
        gain, out, top = find_moves(t, par, min_gain)
        winners = select_moves(par, gain, out, top, lock_rounds)
        apply_moves(t, par, winners, out, top)
        t.moves += len(winners)
    return t


# ---- layout and collapse ------------------------------------------------------------------------------------------------------------------
def layout(tree):
    """Depth first, left before right -> {"perm": [n] the Morton index at every final position, "first", "count": [2 n - 1] of every slot}."""
    n, left, right = tree.n, tree.left.tolist(), tree.right.tolist()
    first, count = [0] * (2 * n - 1), [1] * (2 * n - 1)
    perm, pre, todo = [], [], [tree.root]
    while todo:
        v = todo.pop()
        first[v] = len(perm)
        if v < n: perm.append(v)
        else: pre.append(v); todo.append(right[v - n]); todo.append(left[v - n])
    for v in reversed(pre): count[v] = count[left[v - n]] + count[right[v - n]]
    assert len(perm) == n and sorted(perm) == list(range(n)) and len(pre) == n - 1, "the links do not form a tree over the leaves"
    return {"perm": np.array(perm, i64), "first": np.array(first, i64), "count": np.array(count, i64)}


def range_boxes(lo_t, hi_t, first, count):
    """min lo / max hi over [first, first + count) of the ordered triangles' boxes, for every entry."""
    order = np.lexsort((-count, first))
    idx = np.empty(2 * len(first), i64)
    idx[0::2] = first[order]; idx[1::2] = (first + count)[order]
    pad = np.zeros((1, 3), f32)
    lo = np.minimum.reduceat(np.concatenate([lo_t, pad]), idx, axis=0)[0::2]; hi = np.maximum.reduceat(np.concatenate([hi_t, pad]), idx, axis=0)[0::2]
    out_lo, out_hi = np.empty_like(lo), np.empty_like(hi)
    out_lo[order] = lo; out_hi[order] = hi
    return out_lo, out_hi


def inner_area(tree, lay=None):
    """Sum of the inner nodes' area keys over the root's, from the leaves' boxes (float64 sum of float32 keys): the expected node visits of a ray."""
    lay = lay or layout(tree)
    n = tree.n
    lo, hi = range_boxes(tree.lo[:n][lay["perm"]], tree.hi[:n][lay["perm"]], lay["first"][n:], lay["count"][n:])
    a = area_key(lo, hi).astype(np.float64)
    return float(a.sum() / a[tree.root - n])


def collapse(tree, lay=None, open_largest=True, strict_network=True):
    """The 4-wide collapse, top down: a wide node starts with a binary node's two children and keeps opening the inner child with the largest
    float32 key dx dy + dy dz + dz dx (strictly larger: the lowest slot wins ties; the opened child's left takes its slot, its right the next free
    one) until it holds four children or only leaves, a subtree of at most kLeafMax triangles being one leaf; then the children are ordered by the
    network (0,1)(2,3)(0,2)(1,3)(1,2), swapping when key[A] < key[B].  Needs tree.lo / tree.hi of the leaves only.
    -> {"perm", "cnt" [W], "first", "count" [W, 4], "leaf" [W, 4] bool, "child" [W, 4] (a node of THIS numbering, breadth first; -1), "stack_need"}
    open_largest, strict_network: wrong builders for the sensitivity test."""
    n = tree.n
    lay = lay or layout(tree)
    first, count = lay["first"], lay["count"]
    lo, hi = range_boxes(tree.lo[:n][lay["perm"]], tree.hi[:n][lay["perm"]], first, count)
    key = area_key(lo, hi).astype(np.float64).tolist()
    inner = (count > K_LEAF_MAX).tolist()
    left, right = tree.left.tolist(), tree.right.tolist()
    rows, queue, need_max = [], [(tree.root, 0)], 0
    at = 0
    while at < len(queue):
        b, need_in = queue[at]; at += 1
        kids = [left[b - n], right[b - n]]
        while len(kids) < K_WIDTH:
            pick, best = -1, (-1.0 if open_largest else np.inf)
            for k, s in enumerate(kids):
                if inner[s] and (key[s] > best if open_largest else key[s] < best): best, pick = key[s], k
            if pick < 0: break
            s = kids[pick]
            kids[pick] = left[s - n]; kids.append(right[s - n])
        ks = [key[s] for s in kids] + [-1.0] * (K_WIDTH - len(kids))
        kids = kids + [-1] * (K_WIDTH - len(kids))
        for a, b2 in NETWORK:
            if ks[a] < ks[b2] or (not strict_network and ks[a] == ks[b2]):
                ks[a], ks[b2] = ks[b2], ks[a]; kids[a], kids[b2] = kids[b2], kids[a]
        cnt = sum(1 for s in kids if s >= 0)
        assert all(s >= 0 for s in kids[:cnt])
        need = need_in + cnt - 1; need_max = max(need_max, need)
        child = []
        for s in kids:
            if s >= 0 and inner[s]: child.append(len(queue)); queue.append((s, need))
            else: child.append(-1)
        rows.append((kids, child, cnt))
    W = len(rows)
    slots = np.array([r[0] for r in rows], i64).reshape(W, K_WIDTH)
    used = slots >= 0
    s0 = np.maximum(slots, 0)
    return {"perm": lay["perm"], "cnt": np.array([r[2] for r in rows], i64), "first": np.where(used, first[s0], 0), "count": np.where(used, count[s0], 0),
            "leaf": used & (count[s0] <= K_LEAF_MAX), "child": np.array([r[1] for r in rows], i64).reshape(W, K_WIDTH), "stack_need": need_max}


# ---- the whole build ------------------------------------------------------------------------------------------------------------------------
def predict(rows, builder, passes=8, min_gain=1e-3, lock_rounds=3, axes=(0, 1, 2), radius=16, radius_left=None, use_extent=True,
            index_before_distance=False, open_largest=True, strict_network=True, number_descending=False, stages=None):
    """The tree the product is meant to build for the scene rows (accel_ref.scene_rows) with the builder: collapse()'s dict plus "ids" [n, 2], the
    (inst, prim) of the triangle at every final position.  stages (a dict, optional) receives keys, order, the binary tree, the layout."""
    lo, hi, ids = world_boxes(rows)
    keys = morton_keys(lo, hi, axes)
    order = sorted_order(keys)
    mlo, mhi = lo[order], hi[order]
    if builder == BUILDER_LBVH:
        tree = radix_tree(keys[order]); tree.lo, tree.hi = mlo, mhi
    else:
        tree = ploc_tree(mlo, mhi, radius, radius_left, use_extent, index_before_distance, number_descending=number_descending)
        if builder == BUILDER_PLOC_REINSERT: tree = reinsert(tree, passes, min_gain, lock_rounds)
    lay = layout(tree)
    wide = collapse(tree, lay, open_largest, strict_network)
    wide["ids"] = ids[order][lay["perm"]]
    if stages is not None: stages.update(keys=keys, order=order, tree=tree, layout=lay, lo=lo, hi=hi, ids=ids)
    return wide


def predict_fallback(rows):
    """A clustering build that gave up: the radix tree over the same Morton order."""
    return predict(rows, BUILDER_LBVH)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def compare(device_tree, predicted, limit=4):
    """device_tree: what accel_hook.accel_read returns (info, nodes, ranges, tris, shade); predicted: predict() / collapse() with "ids".
    Walks the two trees from their roots together with an explicit frontier of (device node, predicted node) pairs and compares, slot by slot in
    slot order, the number of children, each child's (first, count) from WideRanges, whether it is a leaf and the leaf reference's bits, and
    descends into the inner children; wide node indices are not compared.  Names:
      order.triangles    the (inst, prim) of the packets, position by position
      topology.children  the number of children of a node
      topology.slot      a node has the predicted children, in other slots (the walk goes on below them, matched by range)
      topology.range     a node has a child the predicted node has not
      topology.leaf      a child is a leaf on one side only, or its reference is not ~(first | (count - 1) << 28)
      stack_need         info's stack_need
    One line per name: how many, and the first `limit` of them."""
    info, nodes, ranges, tris = device_tree[0], device_tree[1], device_tree[2], device_tree[3]
    found = {}

    def add(name, detail):
        found.setdefault(name, []).append(detail)

    n = int(info[0]); W = int(info[1])
    tw = np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 64).view(u32).reshape(-1, 16)
    got_ids = np.stack([tw[:, 3], tw[:, 7]], axis=1).astype(i64)
    want_ids = predicted["ids"]
    if len(got_ids) != len(want_ids) or n != len(want_ids): add("order.triangles", "%d packets, info says %d, predicted %d" % (len(got_ids), n, len(want_ids)))
    else:
        for at in np.nonzero((got_ids != want_ids).any(axis=1))[0]:
            add("order.triangles", "position %d holds (inst %d, prim %d), predicted (%d, %d)" % (at, got_ids[at, 0], got_ids[at, 1], want_ids[at, 0], want_ids[at, 1]))
    if int(info[3]) != predicted["stack_need"]: add("stack_need", "info says %d, predicted %d" % (int(info[3]), predicted["stack_need"]))
    if ranges is None or W < 1 or int(info[2]) != 0: add("topology.range", "no tree to walk: %d wide nodes, root %#x, ranges %s" % (W, int(info[2]), "absent" if ranges is None else "present"))
    else:
        child = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 64)[:, 16:32].copy().view(np.int32).reshape(-1, 4).astype(i64)
        rw = np.ascontiguousarray(ranges).view(np.uint8).reshape(-1, 32).view(u32).reshape(-1, 8).astype(i64)
        frontier, seen = [(0, 0)], 0
        while frontier and seen <= W:
            nxt = []
            for dv, pv in frontier:
                seen += 1
                if dv >= W: add("topology.range", "device node %d of %d" % (dv, W)); continue
                dc = int((child[dv] != K_EMPTY).sum()); pc = int(predicted["cnt"][pv])
                if dc != pc: add("topology.children", "device node %d has %d children, predicted node %d has %d" % (dv, dc, pv, pc))
                want = {(int(predicted["first"][pv, k]), int(predicted["count"][pv, k])): k for k in range(pc)}
                for k in range(K_WIDTH):
                    ref = int(child[dv, k])
                    if ref == K_EMPTY: continue
                    r = (int(rw[dv, k]), int(rw[dv, 4 + k]))
                    if r not in want: add("topology.range", "device node %d slot %d covers [%d, +%d), predicted node %d has %s" % (dv, k, r[0], r[1], pv, sorted(want))); continue
                    pk = want[r]
                    if pk != k: add("topology.slot", "device node %d holds [%d, +%d) in slot %d, predicted node %d in slot %d" % (dv, r[0], r[1], k, pv, pk))
                    p_leaf = bool(predicted["leaf"][pv, pk])
                    if (ref < 0) != p_leaf: add("topology.leaf", "device node %d slot %d [%d, +%d) is %s, predicted %s" % (dv, k, r[0], r[1], "a leaf" if ref < 0 else "inner", "a leaf" if p_leaf else "inner"))
                    elif ref < 0:
                        if ref != ~(r[0] | (r[1] - 1) << 28): add("topology.leaf", "device node %d slot %d: reference %#x for [%d, +%d)" % (dv, k, ref & 0xffffffff, r[0], r[1]))
                    else: nxt.append((ref, int(predicted["child"][pv, pk])))
            frontier = nxt
    return ["%s: %d, first: %s" % (name, len(v), "; ".join(v[:limit])) for name, v in sorted(found.items())]


def as_device_tree(predicted):
    """A predicted tree in the form accel_read returns (only what compare() reads: the child words, the ranges, inst / prim of the packets), so
    that two predictions can be compared and a host test can mutate a correct tree."""
    W, n = len(predicted["cnt"]), len(predicted["ids"])
    nodes = np.zeros((W, 16), np.int32); ranges = np.zeros((W, 8), u32); tris = np.zeros((n, 16), u32)
    used = np.arange(K_WIDTH)[None, :] < predicted["cnt"][:, None]
    leaf_ref = ~(predicted["first"] | (predicted["count"] - 1) << 28)
    nodes[:, 4:8] = np.where(used, np.where(predicted["leaf"], leaf_ref, predicted["child"]), K_EMPTY)
    ranges[:, 0:4] = predicted["first"]; ranges[:, 4:8] = predicted["count"]
    tris[:, 3] = predicted["ids"][:, 0]; tris[:, 7] = predicted["ids"][:, 1]
    info = np.array([n, W, 0, predicted["stack_need"], 0, 0, 0, 1], u32)
    return info, nodes.view(np.uint8).reshape(W, 64), ranges.view(np.uint8).reshape(W, 32), tris.view(np.uint8).reshape(n, 64), None
