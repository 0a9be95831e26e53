"""The acceleration structure checked node by node: check_tree() takes the arrays the device built (tests/accel_hook.py reads them back) or
a host builder wrote (tests/test_accel_check_host.py) and returns a list of named violations, empty for a correct tree.  Plain numpy; it shares
no code with csrc/accel.hip.  It decodes the structures of csrc/pt_types.h (Bvh4Node 64 B, WideRanges 32 B, TriPacket 64 B, ShadePacket 128 B),
walks the tree from the root level by level, vectorised over the frontier (a chain of coincident centroids is thousands of levels deep),
and compares with what the scene's triangles say.  accel.o is compiled without floating-point contraction, so numpy float32 reproduces its
products and sums bit for bit; a triangle's box is the kernel's own expression: min and max of v0, v0 + e1, v0 + e2 in float32.

Every violation is "<name>: <detail>"; the names and what each demands:

  shape.root          root == 0 and wide_nodes >= 1, or root == ~0 and wide_nodes == 0, the latter exactly when n_tris == 1
  shape.reach         every wide node index in [0, wide_nodes) is reached exactly once from the root; no child index is out of range
  shape.leaf_ref      a leaf reference ~(first | (count - 1) << 28) has count in 1..kLeafMax and first + count <= n_tris
  shape.leaf_tiling   the leaf ranges cover every triangle of [0, n_tris) exactly once; the ranges under a node's children are adjacent
  shape.empty_slots   kEmptyChild comes only after the used slots, and a reached node has at least two children
  shape.narrow_inner  a node with fewer than four children has only leaf children (the collapse keeps opening inner children)
  shape.pad           a node's last 8 bytes and the exponent word's fourth byte are zero (wide_write writes them)
  tri.multiset        the (inst, prim) pairs of the packets are the scene's triangles, each once
  tri.flags           TriPacket::flags is the instance row's mask_flags (mipt_api.hip pt_scene_set_instances, restated in scene_rows)
  tri.shade_inst      ShadePacket::inst == TriPacket::inst
  tri.shade_pos       the ShadePacket's three positions are the primitive's object-space vertices, bit for bit
  tri.shade_tangent   ShadePacket::v[k].tangent_space is the instance's packed tangent-space word at the de-indexed vertex; 0 without the stream
  tri.shade_uv0       ShadePacket::uv0[k] is the instance's first texcoord pair at the de-indexed vertex, bit for bit; zeros without the stream
  tri.shade_uv1       ShadePacket::uv1[k] likewise for the second set
  tri.shade_color     ShadePacket::color[k] is the two words of the instance's R16G16B16A16 colour at the de-indexed vertex; zeros without the
                      stream (k_shade_packets at a build and k_refit_packets at a refit write all four; offsets from pt_types.h ShadePacket)
  tri.transform       v0, e1, e2 are mul_point's float32 expression M0 x + M4 y + M8 z + M12 (left to right) and w1 - w0, w2 - w0, bit for bit
  ranges              WideRanges first / count of child k is the leaf range found by walking below it; count 0 for an empty slot
  contain.exact_lo    origin + qlo * step <= min lo of the triangles below the child, in float64, where the sum is exact (pt_slab.h
  contain.exact_hi    bvh_plane_exceeds: the product has 8 bits, |origin| / step < 2^45); origin + qhi * step >= max hi likewise
  contain.float_lo    the same two inequalities through bvh_dequant, fmaf(q, step, origin) in float32 (the exact sum rounded once)
  contain.float_hi
  origin              the node's origin has the bits of the minimum of its children's lo
  tight.lo            min lo - (origin + qlo * step) < 2 * step, and (origin + qhi * step) - max hi < 2 * step.  From wide_write, not measured:
  tight.hi            with x = (lo - origin) / step exact, the start value floor(fl(lo - origin) / step) is >= floor(x) - 1 (one float32 rounding
                      of a number below 2^9 moves it by less than 2^-14), the loop stops at the first plane that is <= lo exactly and in float,
                      every q <= floor(x) is such a plane, so q >= floor(x) - 1 and x - q < 2; the mirror image for hi, x <= 255 by the exponent
  tight.exp           the step exponent is >= 1 and at most one above the smallest exponent (>= 1) whose 255th plane reaches the far side
                      exactly (wide_write starts at the exponent of fl(extent / 255), which cannot reach with a factor two to spare, and
                      raises it only while the 255th plane falls short)
  tight.flat          on an axis of zero extent every byte of the node is 0
  quantise            quantise(), wide_write restated operation for operation, applied to the children's boxes taken from their ranges,
                      reproduces the node's 56 payload bytes: this is what makes "a refit equals a fresh wide_write of the same topology" checkable
  order               the float32 key dx * dy + dy * dz + dz * dx, evaluated left to right, is non-increasing over the used slots.  This is a
                      promise of the BUILD: a refit keeps every child in the slot the build gave it (bit-identical references and ranges) and
                      only requantises, so after a refit the order is that of the build's pose.  check_tree(ordered=) names the nodes for which
                      the claim is made: all of them for a built tree; after refits, those with no triangle touched since the build
  stack_need          info's stack_need is the maximum over the nodes of need(parent) + children - 1, need(parent) = 0 at the root
"""
import numpy as np

f32, f64, u32, i32, u8 = np.float32, np.float64, np.uint32, np.int32, np.uint8

K_WIDTH, K_LEAF_MAX, K_EMPTY, K_FIRST_MASK = 4, 3, 0x7fffffff, 0x0fffffff                      # pt_types.h
NODE_BYTES, RANGE_BYTES, TRI_BYTES, SHADE_BYTES = 64, 32, 64, 128
TF_CULL_DISABLE, TF_FORCE_NON_OPAQUE, TF_MIRRORED = 1 << 8, 1 << 9, 1 << 10
INFO_N_TRIS, INFO_WIDE_NODES, INFO_ROOT, INFO_STACK_NEED, INFO_SEG_LEAVES, INFO_BUILDER, INFO_FALLBACKS, INFO_HAVE_RANGES = range(8)
Q_OFFSET = 32                                                                                  # byte of qlox[0]: qlo[a][k] at 32 + 8 a + k, qhi 4 further
# ShadePacket in 32-bit words (pt_types.h): v[k] = {pos[3], tangent_space} at 4 k, uv0[3][2] at 12, inst at 18, uv1[3][2] at 20, color[3][2] at 26
SHADE_TANGENT, SHADE_UV0, SHADE_INST, SHADE_UV1, SHADE_COLOR = (3, 7, 11), 12, 18, 20, 26
STREAMS = ("tangent", "uv0", "uv1", "color")                                                   # scene_rows keys; words per vertex 1, 2, 2, 2


# ---- the scene's side -------------------------------------------------------------------------------------------------------------------
def scene_rows(scene, transforms=None, positions=None):
    """What check_tree needs of a scenes.SceneData: per instance its float32 positions, its indices (or None), the 16 floats of its transform,
    the packets' flags word and the four optional vertex streams as 32-bit words ("tangent" [vertices], "uv0" / "uv1" / "color" [vertices, 2];
    None where the instance has no such stream).  transforms / positions override the scene's own for a moved or rewritten instance:
    {instance: 16 floats, column-major} and {instance: [vertices, 3]}."""
    rows = []
    for i, d in enumerate(scene.instances):
        g = d.gpu
        take = lambda h: scene.buffers[h][0]
        M = np.array(list(g.transform) if transforms is None or i not in transforms else transforms[i], f32).reshape(16)
        m = M.astype(f64)
        det = m[0] * (m[5] * m[10] - m[9] * m[6]) - m[4] * (m[1] * m[10] - m[9] * m[2]) + m[8] * (m[1] * m[6] - m[5] * m[2])
        flags = (d.instance_mask & 0xff) | (TF_CULL_DISABLE if d.instance_flags & 0x1 else 0) | (TF_FORCE_NON_OPAQUE if d.instance_flags & 0x8 else 0) | \
                (TF_MIRRORED if det < 0 else 0)
        idx = None if g.index_descriptor == -1 else np.asarray(take(g.index_descriptor)).astype(np.int64)[:d.num_of_indices]
        pos = take(g.position_descriptor) if positions is None or i not in positions else positions[i]
        words = lambda h, per: None if h == -1 else np.ascontiguousarray(take(h)).reshape(-1).view(u32).reshape(-1, per)
        rows.append({"positions": np.asarray(pos, f32).reshape(-1, 3), "indices": idx, "transform": M,
                     "mask_flags": flags, "triangles": d.num_of_indices // 3,
                     "tangent": None if g.tangent_space_descriptor == -1 else words(g.tangent_space_descriptor, 1).reshape(-1),
                     "uv0": words(g.texcoord_descriptors[0], 2), "uv1": words(g.texcoord_descriptors[1], 2), "color": words(g.color_descriptor, 2)})
    return rows


def row_corners(row):
    """[triangles, 3] the vertex each corner of each primitive reads (the index stream's entry, or 3 prim + k without one)."""
    n = row["triangles"]
    return (np.arange(3 * n) if row["indices"] is None else row["indices"][:3 * n]).reshape(n, 3)


def row_vertices(row):
    """[triangles, 3, 3] float32 object-space vertices of an instance row."""
    n = row["triangles"]
    idx = np.arange(3 * n) if row["indices"] is None else row["indices"][:3 * n]
    return row["positions"][idx].reshape(n, 3, 3)


def mul_point(M, v):
    """pt_math.h mul_point in float32, products and sums in the order written."""
    M = M.astype(f32); v = v.astype(f32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([((M[0] * x + M[4] * y) + M[8] * z) + M[12], ((M[1] * x + M[5] * y) + M[9] * z) + M[13], ((M[2] * x + M[6] * y) + M[10] * z) + M[14]], axis=-1)


# ---- decoding -------------------------------------------------------------------------------------------------------------------------
def as_bytes(a, row):
    a = np.ascontiguousarray(a)
    return a.view(u8).reshape(-1, row)


def tri_boxes(tris):
    """(lo, hi) [n, 3] float32 of the packets: the kernel's own expression."""
    w = as_bytes(tris, TRI_BYTES).view(f32).reshape(-1, 16)
    p, q, r = w[:, 0:3], w[:, 0:3] + w[:, 4:7], w[:, 0:3] + w[:, 8:11]
    return np.minimum(np.minimum(p, q), r), np.maximum(np.maximum(p, q), r)


def decode_nodes(nodes):
    b = as_bytes(nodes, NODE_BYTES)
    W = len(b)
    origin = b[:, 0:12].copy().view(f32).reshape(W, 3)
    exps = b[:, 12:15].astype(np.int64)
    child = b[:, 16:32].copy().view(i32).reshape(W, 4).astype(np.int64)
    q = b[:, Q_OFFSET:Q_OFFSET + 24].reshape(W, 3, 2, 4)                  # [node, axis, lo / hi, child]
    qlo = q[:, :, 0, :].transpose(0, 2, 1).astype(np.int64)              # [node, child, axis]
    qhi = q[:, :, 1, :].transpose(0, 2, 1).astype(np.int64)
    return origin, exps, child, qlo, qhi


def leaf_first_count(ref):
    x = ~ref
    return x & K_FIRST_MASK, ((x >> 28) & 0xf) + 1


def step_of(e, dtype=f64):
    """bvh_step: 2^(e - 127) from the biased exponent."""
    return (np.asarray(e).astype(u32) << u32(23)).view(f32).astype(dtype)


def range_boxes(lo_t, hi_t, first, count):
    """min lo / max hi over the triangles [first, first + count) of every entry (count >= 1), float32."""
    n = len(lo_t)
    idx = np.empty(2 * len(first), np.int64)
    idx[0::2] = first; idx[1::2] = first + count                         # (a pair whose second index is not larger yields one row: not used here)
    lo_p = np.concatenate([lo_t, np.zeros((1, 3), f32)]); hi_p = np.concatenate([hi_t, np.zeros((1, 3), f32)])
    assert (idx >= 0).all() and (idx <= n).all() and (count >= 1).all()
    return np.minimum.reduceat(lo_p, idx, axis=0)[0::2], np.maximum.reduceat(hi_p, idx, axis=0)[0::2]


# ---- wide_write restated ----------------------------------------------------------------------------------------------------------------
def _plane64(q, step64, p):
    return p.astype(f64) + q.astype(f64) * step64                        # exact (pt_slab.h)


def _dequant(q, step64, p):
    return _plane64(q, step64, p).astype(f32)                            # fmaf(q, step, origin): the exact sum rounded once


def quantise(lo, hi, cnt):
    """wide_write (accel.hip) for many nodes at once.  lo, hi: [N, 4, 3] float32 boxes of the children, cnt: [N] how many are used (they are
    packed from slot 0).  Returns (origin [N, 3] float32, exps [N, 3], qlo [N, 4, 3], qhi [N, 4, 3]); bytes of unused slots are 0."""
    lo = np.asarray(lo, f32); hi = np.asarray(hi, f32); cnt = np.asarray(cnt)
    N = len(lo)
    used = np.arange(K_WIDTH)[None, :] < cnt[:, None]
    p = lo[:, 0, :].copy(); top = hi[:, 0, :].copy()
    for k in range(1, K_WIDTH):
        m = used[:, k, None]
        p = np.where(m, np.minimum(p, lo[:, k, :]), p); top = np.where(m, np.maximum(top, hi[:, k, :]), top)
    with np.errstate(over="ignore", invalid="ignore"):
        e = (((top - p) * (f32(1.0) / f32(255.0))).astype(f32).view(u32) >> u32(23)).astype(np.int64) & 0xff
        e = np.clip(e, 1, 254)
        q255 = np.full(e.shape, 255, np.int64)
        while True:                                                     # smallest power-of-two step whose 255th plane reaches the far side
            s = step_of(e)
            grow = (e < 254) & (~(_dequant(q255, s, p) >= top) | (_plane64(q255, s, p) < top.astype(f64)))
            if not grow.any(): break
            e = e + grow
        s = step_of(e)[:, None, :]; inv = step_of(254 - e, f32)[:, None, :]
        pk = np.broadcast_to(p[:, None, :], lo.shape)
        ql = np.clip(np.floor(((lo - pk).astype(f32) * inv).astype(f32)), 0, 255)
        qh = np.clip(np.ceil(((hi - pk).astype(f32) * inv).astype(f32)), 0, 255)
        ql = np.where(np.isnan(ql), 0, ql).astype(np.int64); qh = np.where(np.isnan(qh), 0, qh).astype(np.int64)
        while True:
            down = (ql > 0) & ((_dequant(ql, s, pk) > lo) | (_plane64(ql, s, pk) > lo.astype(f64)))
            if not down.any(): break
            ql = ql - down
        while True:
            up = (qh < 255) & ((_dequant(qh, s, pk) < hi) | (_plane64(qh, s, pk) < hi.astype(f64)))
            if not up.any(): break
            qh = qh + up
    ql = np.where(used[:, :, None], ql, 0); qh = np.where(used[:, :, None], qh, 0)
    return p, e, ql, qh


def node_bytes(origin, exps, child, qlo, qhi):
    """The 64 bytes of Bvh4Node from its decoded parts (child: [N, 4] references, kEmptyChild in unused slots)."""
    N = len(origin)
    b = np.zeros((N, NODE_BYTES), u8)
    b[:, 0:12] = np.ascontiguousarray(origin, f32).view(u8).reshape(N, 12)
    b[:, 12:15] = exps.astype(u8)
    b[:, 16:32] = np.ascontiguousarray(child.astype(i32)).view(u8).reshape(N, 16)
    q = np.stack([qlo.transpose(0, 2, 1), qhi.transpose(0, 2, 1)], axis=2)     # [node, axis, lo / hi, child]
    b[:, Q_OFFSET:Q_OFFSET + 24] = q.reshape(N, 24).astype(u8)
    return b


def area_key(lo, hi):
    """The collapse's ordering key in float32, left to right."""
    d = (hi - lo).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((d[..., 0] * d[..., 1]).astype(f32) + (d[..., 1] * d[..., 2]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 0]).astype(f32)


# ---- the check ----------------------------------------------------------------------------------------------------------------------------
class _Report:
    def __init__(self): self.items = []

    def add(self, name, mask_or_flag, detail):
        """One line per name: how many entries fail and the first of them."""
        if isinstance(mask_or_flag, (bool, np.bool_)):
            if mask_or_flag: self.items.append("%s: %s" % (name, detail() if callable(detail) else detail))
            return
        bad = np.argwhere(np.asarray(mask_or_flag))
        if len(bad): self.items.append("%s: %d, first at %s: %s" % (name, len(bad), tuple(int(x) for x in bad[0]), detail(tuple(bad[0])) if callable(detail) else detail))


def names(violations):
    return sorted({v.split(":")[0] for v in violations})


def check_triangles(rep, n, tris, shade, scene):
    tw = as_bytes(tris, TRI_BYTES).view(u32).reshape(-1, 16)[:n]
    sw = as_bytes(shade, SHADE_BYTES).view(u32).reshape(-1, 32)[:n]
    counts = np.array([r["triangles"] for r in scene], np.int64)
    total = int(counts.sum())
    rep.add("tri.multiset", total != n or len(tw) != n or len(sw) != n, "the scene has %d triangles, info says %d, %d packets, %d shading packets" % (total, n, len(tw), len(sw)))
    if total != n or len(tw) != n or len(sw) != n: return
    inst, prim = tw[:, 3].astype(np.int64), tw[:, 7].astype(np.int64)
    want = np.concatenate([np.full(c, i, np.int64) << 32 | np.arange(c, dtype=np.int64) for i, c in enumerate(counts)]) if n else np.zeros(0, np.int64)
    got = np.sort(inst << 32 | prim)
    rep.add("tri.multiset", got != want, lambda at: "sorted (inst, prim) %d / %d, expected %d / %d" % (got[at] >> 32, got[at] & 0xffffffff, want[at] >> 32, want[at] & 0xffffffff))
    rep.add("tri.shade_inst", sw[:, SHADE_INST] != tw[:, 3], lambda at: "shade.inst %d, tris.inst %d" % (sw[at][SHADE_INST], tw[at][3]))
    ok = (inst < len(scene)) & (prim < counts[np.minimum(inst, len(scene) - 1)])
    if not ok.all(): return                                            # (already a tri.multiset violation)
    pos = np.zeros((n, 3, 3), f32); world = np.zeros((n, 3, 3), f32); flags = np.zeros(n, u32)
    stream = {"tangent": np.zeros((n, 3, 1), u32), "uv0": np.zeros((n, 3, 2), u32), "uv1": np.zeros((n, 3, 2), u32), "color": np.zeros((n, 3, 2), u32)}
    for i, r in enumerate(scene):
        m = inst == i
        if not m.any(): continue
        v = row_vertices(r)[prim[m]]
        pos[m] = v; world[m] = mul_point(r["transform"], v); flags[m] = r["mask_flags"]
        corners = row_corners(r)[prim[m]]
        for name in STREAMS:
            if r.get(name) is not None: stream[name][m] = np.asarray(r[name]).view(u32).reshape(len(r[name]), -1)[corners]       # (absent: zeros)
    rep.add("tri.flags", tw[:, 11] != flags, lambda at: "flags %#x, the instance row's %#x" % (tw[at][11], flags[at]))
    spos = np.stack([sw[:, 0:3], sw[:, 4:7], sw[:, 8:11]], axis=1)
    rep.add("tri.shade_pos", (spos != pos.view(u32)).any(axis=(1, 2)), "shading packet positions differ from the primitive's vertices")
    got_s = {"tangent": sw[:, list(SHADE_TANGENT)].reshape(n, 3, 1), "uv0": sw[:, SHADE_UV0:SHADE_UV0 + 6].reshape(n, 3, 2),
             "uv1": sw[:, SHADE_UV1:SHADE_UV1 + 6].reshape(n, 3, 2), "color": sw[:, SHADE_COLOR:SHADE_COLOR + 6].reshape(n, 3, 2)}
    for name in STREAMS:
        g, w = got_s[name], stream[name]
        rep.add("tri.shade_" + name, (g != w).any(axis=(1, 2)), lambda at, g=g, w=w: "packet %d (instance %d primitive %d) holds %s, the stream says %s" %
                (at[0], inst[at[0]], prim[at[0]], [hex(int(x)) for x in g[at[0]].reshape(-1)], [hex(int(x)) for x in w[at[0]].reshape(-1)]))
    with np.errstate(over="ignore", invalid="ignore"):
        want_t = np.stack([world[:, 0], (world[:, 1] - world[:, 0]).astype(f32), (world[:, 2] - world[:, 0]).astype(f32)], axis=1)
    got_t = np.stack([tw[:, 0:3], tw[:, 4:7], tw[:, 8:11]], axis=1)
    rep.add("tri.transform", (got_t != want_t.view(u32)).any(axis=(1, 2)), lambda at: "packet %s, expected %s" % (got_t[at[0]].view(f32).tolist(), want_t[at[0]].tolist()))


def check_tree(info, nodes, ranges, tris, shade, scene, stats=None, ordered=None):
    """info: the 8 words of pt_debug_accel_read; nodes / ranges / tris / shade: its arrays (any dtype, the right number of bytes; ranges None if
    absent); scene: scene_rows().  Returns the list of violations.  stats (a dict, optional) receives node_count, children histogram, levels.
    ordered: [wide_nodes] bool, the nodes whose children must be in decreasing area (None: all; see `order` above)."""
    rep = _Report()
    info = [int(x) for x in info]
    n, W, root, need_said = info[INFO_N_TRIS], info[INFO_WIDE_NODES], info[INFO_ROOT], info[INFO_STACK_NEED]
    check_triangles(rep, n, tris, shade, scene)
    single = root == 0xffffffff and W == 0
    rep.add("shape.root", not ((single and n == 1) or (root == 0 and W >= 1 and n >= 2)), "root %#x, %d wide nodes, %d triangles" % (root, W, n))
    if stats is not None: stats.update(node_count=W, children=[0] * 5, levels=0, stack_need=need_said)
    if n < 2 or W < 1 or root != 0:
        if single and n == 1: rep.add("stack_need", need_said != 0, "stack_need %d for a single triangle" % need_said)
        return rep.items
    nb = as_bytes(nodes, NODE_BYTES)
    rep.add("shape.reach", len(nb) != W, "%d nodes given, info says %d" % (len(nb), W))
    if len(nb) != W or len(as_bytes(tris, TRI_BYTES)) != n: return rep.items
    origin, exps, child, qlo, qhi = decode_nodes(nodes)
    used = child != K_EMPTY
    cnt = used.sum(axis=1)
    is_leaf = used & (child < 0)
    is_inner = used & (child >= 0)
    lf, lc = leaf_first_count(child)

    # -- the walk, top down: who is reached, with what stack need
    reached = np.zeros(W, np.int64)
    need_in = np.zeros(W, np.int64)
    levels = []
    frontier = np.array([0], np.int64); reached[0] = 1
    bad_child = 0
    while len(frontier) and len(levels) <= W:
        levels.append(frontier)
        kids = child[frontier]; inner = is_inner[frontier]
        bad = inner & (kids >= W)
        bad_child += int(bad.sum())
        go = inner & ~bad
        nxt = kids[go]
        nneed = np.repeat(need_in[frontier] + cnt[frontier] - 1, go.sum(axis=1))
        first_time = reached[nxt] == 0                                   # a node referenced twice (in this level or an earlier one) is walked once
        np.add.at(reached, nxt, 1)
        if (reached[nxt] != 1).any():
            _, where = np.unique(nxt, return_index=True)
            keep = np.zeros(len(nxt), bool); keep[where] = True
            first_time &= keep
        nxt, nneed = nxt[first_time], nneed[first_time]
        need_in[nxt] = nneed
        frontier = nxt
    rep.add("shape.reach", bad_child > 0, "%d child references beyond the %d nodes" % (bad_child, W))
    rep.add("shape.reach", reached != 1, lambda at: "node %d is reached %d times" % (at[0], reached[at]))
    live = reached >= 1
    need = need_in + cnt - 1
    need_max = int(need[live].max())
    rep.add("stack_need", need_said != need_max, "info says %d, the tree needs %d" % (need_said, need_max))
    if stats is not None: stats.update(children=np.bincount(cnt[live], minlength=5).tolist(), levels=len(levels))

    # -- shape of the reached nodes
    rep.add("shape.empty_slots", live[:, None] & (used[:, 1:] & ~used[:, :-1]), "a used slot follows an empty one")
    rep.add("shape.empty_slots", live & (cnt < 2), lambda at: "node %d has %d children" % (at[0], cnt[at]))
    rep.add("shape.narrow_inner", live & (cnt < K_WIDTH) & is_inner.any(axis=1), lambda at: "node %d has %d children, one of them an inner node" % (at[0], cnt[at]))
    rep.add("shape.pad", live & ((nb[:, 56:64] != 0).any(axis=1) | (nb[:, 15] != 0)), "non-zero padding")
    leaf_bad = live[:, None] & is_leaf & ((lc > K_LEAF_MAX) | (lf + lc > n))
    rep.add("shape.leaf_ref", leaf_bad, lambda at: "node %d slot %d: first %d count %d of %d triangles" % (at[0], at[1], lf[at], lc[at], n))
    m = live[:, None] & is_leaf & ~leaf_bad
    cover = np.zeros(n + 1, np.int64)
    np.add.at(cover, lf[m], 1); np.add.at(cover, lf[m] + lc[m], -1)
    cover = np.cumsum(cover)[:n]
    rep.add("shape.leaf_tiling", cover != 1, lambda at: "triangle %d is under %d leaf references" % (at[0], cover[at]))

    # -- the range under every child, bottom up
    cf = np.where(is_leaf, lf, 0); cc = np.where(is_leaf, lc, 0)                                 # [W, 4] first / count; inner slots are filled level by level
    nf = np.zeros(W, np.int64); nc = np.zeros(W, np.int64)
    gap = np.zeros(W, bool)
    for frontier in reversed(levels):
        inner = is_inner[frontier] & (child[frontier] < W)
        kid = np.where(inner, child[frontier], 0)
        f = np.where(inner, nf[kid], cf[frontier]); c = np.where(inner, nc[kid], cc[frontier])
        cf[frontier] = f; cc[frontier] = c
        u = c > 0
        order = np.argsort(np.where(u, f, np.int64(1) << 40), axis=1, kind="stable")
        fs = np.take_along_axis(f, order, axis=1); cs = np.take_along_axis(c, order, axis=1); us = np.take_along_axis(u, order, axis=1)
        gap[frontier] = (us[:, 1:] & (fs[:, 1:] != fs[:, :-1] + cs[:, :-1])).any(axis=1)
        nf[frontier] = fs[:, 0]; nc[frontier] = c.sum(axis=1)
    rep.add("shape.leaf_tiling", live & gap, lambda at: "node %d: the ranges under its children %s + %s are not adjacent" % (at[0], cf[at[0]].tolist(), cc[at[0]].tolist()))
    rep.add("shape.leaf_tiling", bool(nf[0] != 0 or nc[0] != n), "the root covers [%d, %d + %d) of %d triangles" % (nf[0], nf[0], nc[0], n))
    if ranges is None:
        rep.add("ranges", bool(info[INFO_HAVE_RANGES]), "info says the ranges are present, none were given")
    else:
        rw = as_bytes(ranges, RANGE_BYTES).view(u32).reshape(-1, 8).astype(np.int64)
        rep.add("ranges", len(rw) != W, "%d range records for %d nodes" % (len(rw), W))
        if len(rw) == W:
            wrong = live[:, None] & ((rw[:, 4:8] != cc) | ((cc > 0) & (rw[:, 0:4] != cf)))
            rep.add("ranges", wrong, lambda at: "node %d slot %d: recorded [%d, +%d), walked [%d, +%d)" % (at[0], at[1], rw[at[0], at[1]], rw[at[0], 4 + at[1]], cf[at], cc[at]))

    # -- the boxes: every used child of every reached node whose walked range lies inside the triangles
    lo_t, hi_t = tri_boxes(tris)
    lo_t, hi_t = lo_t[:n], hi_t[:n]
    boxed = live[:, None] & used & (cc > 0) & (cf + cc <= n)
    full = live & (boxed == used).all(axis=1)                             # nodes all of whose children have a box
    lo = np.zeros((W, 4, 3), f32); hi = np.zeros((W, 4, 3), f32)
    if boxed.any(): lo[boxed], hi[boxed] = range_boxes(lo_t, hi_t, cf[boxed], cc[boxed])
    B = boxed[:, :, None]
    step = step_of(exps)[:, None, :]                                      # [W, 1, 3] float64
    o64 = origin.astype(f64)[:, None, :]
    p_lo = o64 + qlo.astype(f64) * step; p_hi = o64 + qhi.astype(f64) * step
    where = lambda at: "node %d slot %d axis %d" % at
    rep.add("contain.exact_lo", B & (p_lo > lo.astype(f64)), lambda at: "%s: plane %r > lo %r" % (where(at), p_lo[at], float(lo[at])))
    rep.add("contain.exact_hi", B & (p_hi < hi.astype(f64)), lambda at: "%s: plane %r < hi %r" % (where(at), p_hi[at], float(hi[at])))
    rep.add("contain.float_lo", B & ~(p_lo.astype(f32) <= lo), lambda at: "%s: plane %r > lo %r" % (where(at), float(p_lo.astype(f32)[at]), float(lo[at])))
    rep.add("contain.float_hi", B & ~(p_hi.astype(f32) >= hi), lambda at: "%s: plane %r < hi %r" % (where(at), float(p_hi.astype(f32)[at]), float(hi[at])))
    rep.add("tight.lo", B & ~(lo.astype(f64) - p_lo < 2.0 * step), lambda at: "%s: lo %r is %g steps above its plane" % (where(at), float(lo[at]), (lo[at] - p_lo[at]) / step[at[0], 0, at[2]]))
    rep.add("tight.hi", B & ~(p_hi - hi.astype(f64) < 2.0 * step), lambda at: "%s: hi %r is %g steps below its plane" % (where(at), float(hi[at]), (p_hi[at] - hi[at]) / step[at[0], 0, at[2]]))
    # per node and axis: origin, extent, exponent
    big = f32(np.inf)
    node_lo = np.where(B, lo, big).min(axis=1); node_hi = np.where(B, hi, -big).max(axis=1)      # [W, 3]
    F = full[:, None]
    rep.add("origin", F & (origin.view(u32) != node_lo.view(u32)), lambda at: "node %d axis %d: origin %r, the children's lowest lo %r" % (at[0], at[1], float(origin[at]), float(node_lo[at])))
    with np.errstate(invalid="ignore", over="ignore"):
        flat = F & (node_hi == node_lo)
        rep.add("tight.flat", flat[:, None, :] & ((qlo != 0) | (qhi != 0)), lambda at: "%s has a non-zero byte on an axis of zero extent" % where(at))
        reaches = lambda e: node_lo.astype(f64) + 255.0 * step_of(e) >= node_hi.astype(f64)
        # smallest exponent >= 1 whose 255th plane reaches the far side, exactly: searched down, then up, from the exponent of extent / 255
        ext = np.where(F, node_hi.astype(f64) - node_lo.astype(f64), 0.0)
        e_min = np.where(ext > 0, np.clip(np.frexp(ext / 255.0)[1] + 125, 1, 254), 1).astype(np.int64)
        for _ in range(254):
            spare = F & (e_min > 1) & reaches(np.maximum(e_min - 1, 1))
            if not spare.any(): break
            e_min = e_min - spare
        for _ in range(254):
            short = F & (e_min < 254) & ~reaches(e_min)
            if not short.any(): break
            e_min = e_min + short
    rep.add("tight.exp", F & ((exps < 1) | (exps > e_min + 1)), lambda at: "node %d axis %d: exponent %d, the smallest that reaches is %d" % (at[0], at[1], exps[at], e_min[at]))
    # the quantiser restated, on the boxes taken from the ranges
    idx = np.nonzero(full & (cnt >= 1))[0]
    if len(idx):
        qo, qe, ql, qh = quantise(lo[idx], hi[idx], cnt[idx])
        want = node_bytes(qo, qe, child[idx], ql, qh)
        diff = (want[:, :56] != nb[idx, :56]).any(axis=1)
        rep.add("quantise", diff, lambda at: "node %d: bytes %s, wide_write restated gives %s" % (idx[at[0]], nb[idx[at[0]], :56].tobytes().hex(), want[at[0], :56].tobytes().hex()))
    key = area_key(lo, hi)
    with np.errstate(invalid="ignore"):
        claimed = full if ordered is None else full & np.asarray(ordered, bool)
        rep.add("order", claimed[:, None] & used[:, 1:] & used[:, :-1] & ~(key[:, :-1] >= key[:, 1:]), lambda at: "node %d: keys %s" % (at[0], key[at[0]].tolist()))
    return rep.items


def touched_nodes(ranges, n_tris, touched_tris):
    """[wide_nodes] bool: the node has a touched triangle (touched_tris: [n_tris] bool) in one of its recorded ranges."""
    rw = as_bytes(ranges, RANGE_BYTES).view(u32).reshape(-1, 8).astype(np.int64)
    acc = np.concatenate([[0], np.cumsum(touched_tris[:n_tris].astype(np.int64))])
    f, c = rw[:, 0:4], rw[:, 4:8]
    return ((acc[np.minimum(f + c, n_tris)] - acc[np.minimum(f, n_tris)]) * (c > 0)).sum(axis=1) > 0
