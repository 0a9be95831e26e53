"""Closed meshes, rays aimed at their shared edges and vertices, and what such a ray must find: the inputs and the ground truth of
tests/test_watertight_host.py and tests/test_gpu_watertight.py.  CPU only, plain numpy.

Why.  The float32 Moeller-Trumbore test of csrc/pt_traverse.h and oracle.cpp takes every triangle by its own (v0, e1, e2): nothing in it makes
the two triangles of an edge agree on which side of the edge a ray passes, so a ray within rounding of a shared edge or vertex can be refused
by every triangle around it and go through a closed surface.  Kernel and oracle state the test the same way: their parity says nothing about it.

The rule that closes the gap (restated here as `decide`): where min(u, v, 1 - (u + v)) lies inside a band of BAND_UNITS * 2^-24 * scale around zero
the float test no longer decides; each edge is evaluated from its two exact world-space end points in a canonical order (of their bit patterns),
in float64, so the two triangles of an edge compute the SAME number, and zero counts as inside for both.

Meshes (gltf_renderer_amd/meshgen.py): icosphere(1), icosphere(2) (closed, convex, indexed), box with seg = (2, 2, 2) (vertices duplicated per face
with equal bits, axis-aligned edges) and a displaced grid (interior edges, open rim: only its interior edges and vertices are aimed at).  Each is
one scene with five instances: identity; scale 0.01 near (100, -57, 31); near (1e4, 1e4, -1e4); rotated and non-uniformly scaled; mirrored.

Ray classes, each a deterministic function of (mesh, placement, class, side, seed), targets in float64 from the world-space float32 vertices:
interior (all barycentrics >= 0.05), edge (a point at s in [0.02, 0.98] of a shared edge), vertex (a shared vertex), near (an edge or vertex target
moved 1..8 float32 ulps across the edge).  Origins 0.5-20 mesh radii from the target on the outside, or (closed meshes) inside looking out; the
cosine to every face incident to the target is >= 0.2; directions normalised in float64, then rounded.

The expected answer needs no search: the closed meshes are convex (and the grid's rays are checked in float64 to meet nothing before their
target), so the ray must commit a hit at |t - |target - o|| <= 1e-4 |target - o| on a primitive incident to the target: `expected`."""
import numpy as np

from gltf_renderer_amd import meshgen, scenes

f32, f64, u32 = np.float32, np.float64, np.uint32
BAND_UNITS = f32(16.0)
BAND = f32(BAND_UNITS * f32(2.0 ** -24))    # csrc/pt_traverse.h kEdgeBand
GATE_PAD = f32(1.000004)                    # csrc/pt_slab.h kExitPadWatertight
GATE_PAD_BEFORE = f32(1.0000004)            # kExitPad, the float test's: with it the gate refuses about 1e-4 of the vertex-aimed rays the edge rule accepts
T_TOL = 1e-4
MIN_COS = 0.2
MESHES = ("ico1", "ico2", "box", "grid")
CLOSED = ("ico1", "ico2", "box")
PLACEMENTS = ("identity", "small_far", "far", "rotated", "mirrored")
CLASSES = ("interior", "edge", "vertex", "near")


# ---- meshes and placements ----------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    a = np.asarray(axis, f64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def placement_transform(name):
    T = np.eye(4)
    if name == "small_far": T[:3, :3] *= 0.01; T[:3, 3] = (100.0, -57.0, 31.0)
    elif name == "far": T[:3, 3] = (10000.37, 9999.79, -10000.11)
    elif name == "rotated": T[:3, :3] = _rotation((1, 2, -0.5), 0.83) @ np.diag([0.7, 1.3, 2.1]); T[:3, 3] = (-300.0, 200.0, 150.0)
    elif name == "mirrored": T[:3, :3] = _rotation((-0.3, 1, 0.4), 2.1) @ np.diag([1.0, -1.2, 0.9]); T[:3, 3] = (250.0, 300.0, -200.0)
    else: assert name == "identity", name
    return T


def moved_transform(name):
    """Another transform for the same placement: what the refit case moves the instance to."""
    T = placement_transform(name)
    T[:3, :3] = _rotation((0.2, -1, 0.7), 0.41) @ T[:3, :3] * 1.37
    T[:3, 3] += (3.25, -1.5, 0.75)
    return T


def make_mesh(name):
    if name in ("ico1", "ico2"):
        v, f = meshgen.icosphere(1 if name == "ico1" else 2)
        return meshgen.Mesh(v, f.reshape(-1))
    if name == "box": return meshgen.box((-1.0, -0.7, -0.5), (1.0, 0.7, 0.5), seg=(2, 2, 2))
    assert name == "grid", name
    return meshgen.grid(6, 6, (-1, -1, 0), (2, 0, 0), (0, 2, 0), displace=lambda s, t: 0.08 * np.sin(5 * s + 1) * np.cos(4 * t))


def world_vertices(positions, T):
    """float32 [n, 3]: mul_point of csrc/pt_math.h (and the oracle's mul) on the float32 transform, product by product and sum by sum."""
    M = np.asarray(T, f64).astype(f32); p = np.asarray(positions, f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)], axis=1).astype(f32)


def make_scene(name, transforms=None):
    """One scene per mesh: an instance per placement, in PLACEMENTS' order (instance id = placement index)."""
    s = scenes.SceneData("watertight_" + name)
    mesh = make_mesh(name)
    for k, p in enumerate(PLACEMENTS):
        s.add_mesh(mesh, placement_transform(p) if transforms is None else transforms[k], 0)
    return s


class Topology:
    """Which triangles share an edge or a vertex, by the BITS of the positions (the box's faces duplicate their vertices)."""

    def __init__(self, mesh):
        self.mesh = mesh
        self.idx = mesh.indices.reshape(-1, 3).astype(np.int64)
        bits = np.ascontiguousarray(mesh.positions + f32(0.0)).view(u32)             # (+ 0.0: -0.0 and 0.0 are the same point)
        _, vid = np.unique(bits, axis=0, return_inverse=True)
        self.tri_vid = vid.reshape(-1)[self.idx]
        nt = len(self.idx)
        pairs = np.concatenate([self.tri_vid[:, [0, 1]], self.tri_vid[:, [1, 2]], self.tri_vid[:, [2, 0]]])
        corner = np.concatenate([np.stack([np.arange(nt), np.full(nt, k)], 1) for k in range(3)])     # (triangle, corner the edge starts at)
        key = np.sort(pairs, axis=1)
        uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        assert cnt.max() <= 2
        order = np.argsort(inv, kind="stable")
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        shared = np.nonzero(cnt == 2)[0]
        self.edge_tris = np.stack([corner[order[start[shared]], 0], corner[order[start[shared] + 1], 0]], 1)           # [ne, 2] triangles
        first = corner[order[start[shared]]]                                                                          # the edge in the first of them
        self.edge_ends = np.stack([self.idx[first[:, 0], first[:, 1]], self.idx[first[:, 0], (first[:, 1] + 1) % 3]], 1)   # [ne, 2] vertex indices
        rim = np.unique(uniq[cnt == 1])
        inc = [[] for _ in range(int(self.tri_vid.max()) + 1)]
        for t in range(nt):
            for k in range(3): inc[self.tri_vid[t, k]].append(t)
        ok = [v for v in range(len(inc)) if v not in set(rim.tolist()) and len(inc[v]) >= 3]
        self.K = max(len(inc[v]) for v in ok)
        self.vert_tris = np.array([inc[v] + [-1] * (self.K - len(inc[v])) for v in ok], np.int64)                     # [nv, K], -1 padded
        rep = {}
        for t in range(nt):
            for k in range(3): rep.setdefault(int(self.tri_vid[t, k]), int(self.idx[t, k]))
        self.vert_index = np.array([rep[v] for v in ok], np.int64)                                                    # a vertex index of each


class Placed:
    """A mesh under one placement: its world-space float32 vertices and, in float64, what aiming needs."""

    def __init__(self, topo, T, closed):
        self.topo = topo; self.T = np.asarray(T, f64)
        self.W = world_vertices(topo.mesh.positions, T)
        self.tri = self.W[topo.idx]                                   # [nt, 3, 3] float32
        t64 = self.tri.astype(f64)
        n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        self.centre = self.W.astype(f64).mean(0)
        if np.linalg.det(self.T[:3, :3]) < 0: n = -n                  # the object-space front side (a mirrored instance flips the world winding)
        self.normal = n
        c = t64.mean(1) - self.centre
        self.radius = float(np.linalg.norm(self.W.astype(f64) - self.centre, axis=1).max())
        if closed:
            assert ((c * n).sum(1) > 0).all(), "front faces look outwards"
            self.inradius = float((c * n).sum(1).min())


_TOPO = {}


def topology(name):
    if name not in _TOPO: _TOPO[name] = Topology(make_mesh(name))
    return _TOPO[name]


# ---- rays -------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _blocked(pl, o, d, dist, incident):
    """float64, every triangle: does the ray meet a triangle that is NOT incident to its target before the target?  (The grid is not convex.)"""
    t = pl.tri.astype(f64)
    v0, e1, e2 = t[None, :, 0], (t[:, 1] - t[:, 0])[None], (t[:, 2] - t[:, 0])[None]
    p = np.cross(d[:, None], e2); det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        tv = o[:, None] - v0; u = (tv * p).sum(-1) / det
        q = np.cross(tv, e1); v = (d[:, None] * q).sum(-1) / det; tt = (e2 * q).sum(-1) / det
    hit = (u > -1e-6) & (v > -1e-6) & (u + v < 1 + 1e-6) & (tt > 0) & (tt < dist[:, None] * (1 + 1e-3))
    own = (np.arange(t.shape[0])[None, None, :] == incident[:, :, None]).any(1)
    return (hit & ~own).any(1)


def make_rays(name, placement, cls, inside, n, seed):
    """-> dict(rays [n, 8] float32 (origin, tmin 0, direction, tmax), dist [n] float64 = |target - origin|, incident [n, K] primitives of the
    placement's instance the target lies on (-1 padded), instance).  A deterministic function of its arguments."""
    topo = topology(name); closed = name in CLOSED
    assert closed or not inside
    pl = Placed(topo, placement_transform(placement) if isinstance(placement, str) else placement, closed)
    tag = PLACEMENTS.index(placement) if isinstance(placement, str) else 9
    rng = np.random.default_rng([seed, MESHES.index(name), tag, CLASSES.index(cls), int(inside)])
    K = max(topo.K, 2)
    out_r, out_d, out_i = [], [], []
    have = 0
    for attempt in range(60):
        m = 2 * n
        t64 = pl.tri.astype(f64)
        inc = np.full((m, K), -1, np.int64)
        kind = cls
        edge_pick = rng.integers(0, len(topo.edge_tris), m); vert_pick = rng.integers(0, len(topo.vert_tris), m); s = rng.uniform(0.02, 0.98, m)
        a, b = pl.W[topo.edge_ends[edge_pick, 0]].astype(f64), pl.W[topo.edge_ends[edge_pick, 1]].astype(f64)
        on_edge = a + s[:, None] * (b - a)
        on_vert = pl.W[topo.vert_index[vert_pick]].astype(f64)
        if cls == "interior":
            k = rng.integers(0, len(t64), m)
            w = 0.05 + 0.85 * rng.dirichlet((1, 1, 1), m)
            target = (t64[k] * w[:, :, None]).sum(1); inc[:, 0] = k
        elif cls == "edge":
            target = on_edge; inc[:, :2] = topo.edge_tris[edge_pick]
        elif cls == "vertex":
            target = on_vert; inc[:, :topo.K] = topo.vert_tris[vert_pick]
        else:
            use_edge = rng.random(m) < 0.5
            inc[use_edge, :2] = topo.edge_tris[edge_pick[use_edge]]
            inc[~use_edge, :topo.K] = topo.vert_tris[vert_pick[~use_edge]]
            target = np.where(use_edge[:, None], on_edge, on_vert)
            # across the edge, staying ON the surface: into the first or the second triangle of the edge, in that triangle's plane; from a
            # vertex into its first triangle
            side = np.where(use_edge, rng.integers(0, 2, m), 0)
            into = t64[inc[np.arange(m), side]]
            third = into.sum(1) - a - b
            along = _unit(b - a)
            perp = (third - a) - ((third - a) * along).sum(1, keepdims=True) * along
            w = 0.1 + 0.7 * rng.dirichlet((1, 1, 1), m)
            across = _unit(np.where(use_edge[:, None], perp, (into * w[:, :, None]).sum(1) - on_vert))
            ulp = np.spacing(np.abs(target).max(1).astype(f32)).astype(f64)
            target = target + across * (rng.integers(1, 9, m) * ulp)[:, None]
        valid = inc >= 0
        nrm = pl.normal[np.where(valid, inc, 0)]                                       # [m, K, 3]
        if inside:
            o = pl.centre + _unit(rng.standard_normal((m, 3))) * (0.3 * pl.inradius * rng.random(m) ** (1 / 3))[:, None]
        else:
            base = -_unit((nrm * valid[:, :, None]).sum(1))
            d0 = _unit(base + 0.8 * rng.standard_normal((m, 3)))
            dist = pl.radius * 10.0 ** rng.uniform(np.log10(0.5), np.log10(20.0), m)
            o = target - d0 * dist[:, None]
        o = o.astype(f32)
        d = _unit(target - o.astype(f64))
        dist = np.linalg.norm(target - o.astype(f64), axis=1)
        d32 = d.astype(f32)
        cos = (nrm * d32.astype(f64)[:, None, :]).sum(-1) * (1.0 if inside else -1.0)
        good = np.where(valid, cos >= MIN_COS, True).all(1) & (dist > 0.05 * pl.radius)
        if not closed: good &= ~_blocked(pl, o.astype(f64), d32.astype(f64), dist, inc)
        rays = np.zeros((m, 8), f32); rays[:, 0:3] = o; rays[:, 4:7] = d32; rays[:, 7] = (4.0 * dist).astype(f32)
        out_r.append(rays[good]); out_d.append(dist[good]); out_i.append(inc[good]); have += int(good.sum())
        if have >= n: break
    assert have >= n, (name, placement, cls, inside, have)
    return {"rays": np.concatenate(out_r)[:n], "dist": np.concatenate(out_d)[:n], "incident": np.concatenate(out_i)[:n], "instance": tag, "placed": pl}


def expected(case, out):
    """float64: [n] bool, the ray committed a hit at the target's distance on a primitive incident to the target.  out: [n, 8] as intersect_many's."""
    o = np.asarray(out)
    t = o[:, 1].astype(f64)
    return (o[:, 0] > 0) & (np.abs(t - case["dist"]) <= T_TOL * case["dist"]) & (o[:, 4] == case["instance"]) & (o[:, 5].astype(np.int64)[:, None] == case["incident"]).any(1)


# ---- the triangle test restated: numpy float32, every product and sum rounded on its own (no contraction) ------------------------------------
def _c(a):
    return a[..., 0], a[..., 1], a[..., 2]


def _cross(a, b):
    ax, ay, az = _c(a); bx, by, bz = _c(b)
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], axis=-1)


def float_test(o, d, v0, e1, e2):
    """The leaf test of pt_traverse.h / oracle.cpp Tracer::intersect up to its `inside` decision, as it stood before the edge rule and as the part
    of it that still decides outside the band.  float32 arrays broadcast against each other; -> dict of det, u, v, t, inside, m, band."""
    o, d, v0, e1, e2 = (np.asarray(a, f32) for a in (o, d, v0, e1, e2))
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        a = e1 * p; det = (a[..., 0] + a[..., 1]) + a[..., 2]
        invd = f32(1.0) / det
        tv = o - v0
        pu = tv * p; u = ((pu[..., 0] + pu[..., 1]) + pu[..., 2]) * invd
        q = _cross(tv, e1)
        pv = d * q; v = ((pv[..., 0] + pv[..., 1]) + pv[..., 2]) * invd
        pt = e2 * q; t = ((pt[..., 0] + pt[..., 1]) + pt[..., 2]) * invd
        inside = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1)
        m = np.fmin(np.fmin(u, v), f32(1.0) - (u + v))
        su = (np.abs(pu[..., 0]) + np.abs(pu[..., 1])) + np.abs(pu[..., 2]); sv = (np.abs(pv[..., 0]) + np.abs(pv[..., 1])) + np.abs(pv[..., 2])
        band = (BAND * np.fmax(su, sv)) * np.abs(invd)
    return {"det": det, "u": u, "v": v, "t": t, "inside": inside, "m": m, "band": band}


def today_accepts(o, d, w0, w1, w2):
    """The known-bad statement, fixed here for good: the float test alone decides.  w0, w1, w2: the triangle's world-space float32 vertices."""
    return float_test(o, d, w0, w1 - w0, w2 - w0)["inside"]


def own_box_gate(o, d, v0, e1, e2, t, tmin=f32(0.0), pad=None):
    """candidate_stands' box gate: the ray passes the triangle's own box, in the node test's arithmetic, at a distance consistent with t."""
    pad = GATE_PAD if pad is None else f32(pad)
    o, d, v0, e1, e2, t = (np.asarray(a, f32) for a in (o, d, v0, e1, e2, t))
    with np.errstate(all="ignore"):
        inv = np.clip(f32(1.0) / d, f32(-1.0e30), f32(1.0e30))
        v1, v2 = v0 + e1, v0 + e2
        lo, hi = np.minimum(np.minimum(v0, v1), v2), np.maximum(np.maximum(v0, v1), v2)
        a, b = (lo - o) * inv, (hi - o) * inv
        near, far = np.fmin(a, b), np.fmax(a, b)
        tn = np.fmax(np.fmax(near[..., 0], near[..., 1]), np.fmax(near[..., 2], tmin))
        tx = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2])
        return (tn <= tx * pad) & (tn <= t * pad)


def _bits_less(p, q):
    """Lexicographic order of the bit patterns of two float32 points (x, then y, then z)."""
    a, b = np.ascontiguousarray(p, f32).view(u32), np.ascontiguousarray(q, f32).view(u32)
    return (a[..., 0] < b[..., 0]) | ((a[..., 0] == b[..., 0]) & ((a[..., 1] < b[..., 1]) | ((a[..., 1] == b[..., 1]) & (a[..., 2] < b[..., 2]))))


def edge_value(o, d, p, q):
    """E = d . ((P - o) x (Q - o)) in float64 without contraction, P and Q taken in the order of their bit patterns and the sign flipped back:
    the two triangles of an edge compute the same number."""
    shape = np.broadcast_shapes(np.shape(o), np.shape(p), np.shape(q))
    p, q = np.broadcast_to(np.asarray(p, f32), shape), np.broadcast_to(np.asarray(q, f32), shape)
    swap = _bits_less(q, p)
    a = np.where(swap[..., None], q, p).astype(f64) - np.asarray(o, f32).astype(f64)
    b = np.where(swap[..., None], p, q).astype(f64) - np.asarray(o, f32).astype(f64)
    c = _cross(a, b)
    e = np.asarray(d, f32).astype(f64) * c
    e = (e[..., 0] + e[..., 1]) + e[..., 2]
    return np.where(swap, -e, e)


def edge_rule(o, d, w0, w1, w2, det):
    """Inside iff the three edge values have the sign the float determinant says (zero counts as inside): det = -(E01 + E12 + E20) exactly in
    real arithmetic."""
    s = np.where(np.asarray(det) > 0, -1.0, 1.0)
    return (edge_value(o, d, w0, w1) * s >= 0) & (edge_value(o, d, w1, w2) * s >= 0) & (edge_value(o, d, w2, w0) * s >= 0)


def decide(o, d, w0, w1, w2):
    """The new rule.  -> (inside, u, v, t, in_band, float_test's dict): outside the band the float test's decision and bits; inside it the edge
    rule decides, t is the float test's and (u, v) are the float test's clamped to u, v >= 0 and u + v <= 1."""
    w0, w1, w2 = (np.asarray(a, f32) for a in (w0, w1, w2))
    f = float_test(o, d, w0, w1 - w0, w2 - w0)
    with np.errstate(all="ignore"):
        in_band = (f["det"] != 0) & (np.abs(f["m"]) < f["band"])
        inside = np.where(in_band, edge_rule(o, d, w0, w1, w2, f["det"]), f["inside"])
        uc = np.fmin(np.fmax(f["u"], f32(0.0)), f32(1.0))
        vc = np.fmin(np.fmax(f["v"], f32(0.0)), f32(1.0) - uc)
    return inside, np.where(in_band, uc, f["u"]), np.where(in_band, vc, f["v"]), f["t"], in_band, f


def incident_vertices(case):
    """The world-space float32 vertices of a case's incident triangles: three [n, K, 3] arrays and the [n, K] mask of real entries."""
    inc = case["incident"]; valid = inc >= 0
    t = case["placed"].tri[np.where(valid, inc, 0)]
    return t[:, :, 0], t[:, :, 1], t[:, :, 2], valid


def mesh_cases(name, n, seed=1, transforms=None):
    """Every (placement, side, class) case of a mesh, each with its `placement`, `inside`, `cls` and `instance`.  transforms: the five
    instances' transforms where they are not the placements' own (the refit case)."""
    out = []
    for k, p in enumerate(PLACEMENTS):
        for inside in ((False, True) if name in CLOSED else (False,)):
            for cls in CLASSES:
                c = make_rays(name, p if transforms is None else transforms[k], cls, inside, n, seed)
                c.update(placement=p, inside=inside, cls=cls, instance=k)
                out.append(c)
    return out


def gate_refused(case, pad=None):
    """[n] bool, by the restatements above: the new rule accepts the ray on triangles incident to its target, and the own-box gate refuses
    every one of them.  Such a ray is a refusal of the gate, not a crack."""
    w0, w1, w2, valid = incident_vertices(case)
    r = case["rays"]; o, d = r[:, None, 0:3], r[:, None, 4:7]
    inside, u, v, t, in_band, f = decide(o, d, w0, w1, w2)
    with np.errstate(all="ignore"):
        cand = inside & valid & (t > r[:, None, 3]) & (t <= r[:, None, 7])
    gate = own_box_gate(o, d, w0, w1 - w0, w2 - w0, t, r[:, None, 3], pad)
    return cand.any(1) & ~(cand & gate).any(1)
