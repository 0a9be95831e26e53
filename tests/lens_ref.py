"""float64 restatement of the thin lens (include/mipt.h pt_set_lens), used by tests/test_gpu_lens.py and checked on its own by
tests/test_lens_host.py.  Everything takes the random numbers as input and works on arrays of queries: vectors are [n, 3], scalars [n].

The inputs are the float32 data the product starts from -- the caller's matrices, the host's float32 camera vectors and polygon vertices
(each an fp64 value rounded once) -- and every operation on them is float64, so the restatement carries none of the product's float32
roundings: the product must agree with it within the bound that counts those roundings (BOUND_ROUNDINGS below).  One value is taken in
float32 on purpose: the polygon's s = r.z * n.  The mapping is discontinuous where s crosses an integer (the outer edge of triangle k, then
the centre of triangle k + 1), so which triangle a sample falls in is part of the definition and is decided by the float32 product."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
PI_F32 = float(f32(3.14159265359))          # the kernels' kPi (Common.hlsli:8), a float32 constant
# The bound of the GPU tests: 64 * 2^-24 * M, M = the largest magnitude among o, c, P and focus_distance of the query.  Count of the float32
# roundings between the inputs and a component of the lens ray's origin (the longest chain; each at most 2^-24 of the largest operand):
#   pinhole ray: clip coordinate 4, matrix row 4, divide by w 1, difference 1, length 6 (3 products, 2 sums, sqrt), normalise 1      = 17
#   zo 6 (difference, 3 products, 2 sums), dn 5, (focus - zo) / dn 2, P 2, zo / dn 1, A 2                                             = 18
#   lens sample: mapping <= 8 (disc: square 2, radius and angle 4, sine / cosine 1, product 1; polygon: s 1, a 2, weights 1, blend 3,
#   scale 1), times the radius 1, A' 4 (two products, two sums)                                                                      = 13
#   d' = normalize(P - A') 1 + 6 + 1, dot(d', F) 5, zo / dot 1, o' 2                                                                 = 16
# 64 in all.  They do not all lie on one chain, so the figure is an upper bound of the chain's length, not an estimate of the error.
BOUND_ROUNDINGS = 64


def bound(*magnitudes):
    """64 * 2^-24 * M for arrays of vectors [n, 3] or scalars [n] (or plain numbers)."""
    m = 0.0
    for a in magnitudes:
        a = np.abs(np.asarray(a, f64))
        m = np.maximum(m, a.max(axis=-1) if a.ndim >= 2 else a)
    return BOUND_ROUNDINGS * 2.0 ** -24 * m


def from_cm(flat):
    """glm column-major float[16] -> 4x4 float64 (row, column)."""
    return np.asarray(flat, f64).reshape(4, 4).T


class Camera:
    """What the host derives from pt_execute_params: clip_to_world (the float32 product view_to_clip * world_to_view, inverted in fp64 and
    rounded once) and c, R, U, F from view_to_world (fp64, normalised, rounded once).  Held as float64 arrays of float32 values."""

    def __init__(self, world_to_view, view_to_clip, width, height):
        w2v, v2c = np.asarray(world_to_view, f32).reshape(16), np.asarray(view_to_clip, f32).reshape(16)
        w2c = np.zeros(16, f32)
        for c in range(4):
            for r in range(4):
                s = f32(0)
                for k in range(4):
                    s = f32(s + f32(v2c[k * 4 + r] * w2v[c * 4 + k]))
                w2c[c * 4 + r] = s
        self.clip_to_world = np.linalg.inv(from_cm(w2c)).astype(f32).astype(f64)
        v2w = np.linalg.inv(from_cm(w2v))
        unit = lambda v: v / math.sqrt(float(v @ v))
        r32 = lambda v: np.asarray(v, f64).astype(f32).astype(f64)
        self.c, self.R, self.U, self.F = r32(v2w[:3, 3]), r32(unit(v2w[:3, 0])), r32(unit(v2w[:3, 1])), r32(-unit(v2w[:3, 2]))
        self.width, self.height = int(width), int(height)


def dot(a, b):
    return (np.asarray(a, f64) * np.asarray(b, f64)).sum(axis=-1)


def pinhole_ray(cam, sx, sy):
    """The pinhole ray through image position (sx, sy), pixel units with centres at + 0.5 (pt_trace: sx = px + 0.5 + (r.x - 0.5)).
    Returns o [n, 3], d [n, 3] (unit), tmax [n]."""
    sx, sy = np.atleast_1d(np.asarray(sx, f64)), np.atleast_1d(np.asarray(sy, f64))
    cx = sx / cam.width * 2 - 1
    cy = -(sy / cam.height * 2 - 1)
    one = np.ones_like(cx)
    near = np.stack([cx, cy, one, one], axis=-1) @ cam.clip_to_world.T
    far = np.stack([cx, cy, 0 * one, one], axis=-1) @ cam.clip_to_world.T
    o = near[:, :3] / near[:, 3:4]
    d = far[:, :3] / far[:, 3:4] - o
    length = np.sqrt(dot(d, d))
    return o, d / length[:, None], length


def disk_sample(u, v):
    """square_to_disk(uv_to_square({u, v})) (Transforms.hlsli:52-55, 83-90): the concentric mapping onto the unit disc, [n, 2]."""
    u, v = np.atleast_1d(np.asarray(u, f64)), np.atleast_1d(np.asarray(v, f64))
    sx, sy = u * 2 - 1, v * -2 + 1
    r = np.maximum(np.abs(sx), np.abs(sy))
    phi = np.where(r == 0, 0.0, PI_F32 * (r + (np.abs(sy) - np.abs(sx))) / np.where(r == 0, 1.0, 4 * r))
    return np.stack([np.sign(sx) * r * np.cos(phi), np.sign(sy) * r * np.sin(phi)], axis=-1)


def polygon_vertices(blades, rotation):
    """v_0 .. v_n (v_n = v_0) of the host: fp64 cos / sin of float32(rotation) + 2 pi k / n, rounded once to float32.  [n + 1, 2]."""
    rot = float(f32(rotation))
    ang = np.array([rot + 2.0 * math.pi * (k % blades) / blades for k in range(blades + 1)], f64)
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(f32).astype(f64)


def polygon_sample(blades, rotation, u, v):
    """Uniform over the regular polygon inscribed in the unit circle: triangle k = min((int)s, n - 1) of the fan about the centre, s = u * n
    in float32 (see the module docstring), a = sqrt(s - k), L = a * ((1 - v) * v_k + v * v_{k+1}).  [n, 2]."""
    u, v = np.atleast_1d(np.asarray(u, f32)), np.atleast_1d(np.asarray(v, f64))
    verts = polygon_vertices(blades, rotation)
    s = (u * f32(blades)).astype(f32).astype(f64)
    k = np.minimum(s.astype(np.int64), blades - 1)
    a = np.sqrt(s - k)
    return a[:, None] * ((1 - v)[:, None] * verts[k] + v[:, None] * verts[k + 1])


def lens_sample(blades, rotation, u, v):
    return disk_sample(u, v) if blades == 0 else polygon_sample(blades, rotation, u, v)


def focus_point(cam, o, d, focus_distance):
    """P = o + d * ((focus_distance - zo) / dn), with zo and dn."""
    zo, dn = dot(o - cam.c, cam.F), dot(d, cam.F)
    return o + d * ((focus_distance - zo) / dn)[:, None], zo, dn


def lens_ray(cam, o, d, tmax, L, aperture_radius, focus_distance):
    """The lens ray of the pinhole ray (o, d, tmax) for the unit lens samples L [n, 2].  A zero radius returns the pinhole ray itself (the
    product runs none of the arithmetic then).  Returns o', d', tmax', and P, the lens point A' and zo for the checks."""
    P, zo, dn = focus_point(cam, o, d, focus_distance)
    A = o - d * (zo / dn)[:, None]
    if aperture_radius == 0:
        return o, d, tmax, P, A, zo
    l = float(f32(aperture_radius)) * np.asarray(L, f64)
    A2 = (A + l[:, 0:1] * cam.R) + l[:, 1:2] * cam.U
    d2 = P - A2
    d2 = d2 / np.sqrt(dot(d2, d2))[:, None]
    o2 = A2 + d2 * (zo / dot(d2, cam.F))[:, None]
    return o2, d2, tmax, P, A2, zo


def lens_point_of(cam, o, d, centre=None):
    """The lens sample a ray (o, d) came from: the ray taken back to view-space depth 0, projected on R and U (world units) about `centre`
    (default c; the pinhole ray's own crossing A differs from c by the float32 roundings of the two matrices they come from), and the point."""
    t = -dot(o - cam.c, cam.F) / dot(d, cam.F)
    A = o + d * t[:, None]
    rel = A - (cam.c if centre is None else centre)
    return np.stack([dot(rel, cam.R), dot(rel, cam.U)], axis=-1), A


def distance_to_line(p, o, d):
    """Distance of the points p from the lines o + t d (d unit)."""
    w = np.asarray(p, f64) - o
    w = w - dot(w, d)[:, None] * d
    return np.sqrt(dot(w, w))


def inside_polygon(verts, p, slack=0.0):
    """p [n, 2] inside the convex counter-clockwise polygon verts [m + 1, 2] (closed), widened by `slack` (scalar or [n])."""
    p = np.asarray(p, f64)
    ok = np.ones(len(p), bool)
    for k in range(len(verts) - 1):
        e = verts[k + 1] - verts[k]
        nrm = np.array([e[1], -e[0]]) / math.hypot(e[0], e[1])          # outward for a counter-clockwise polygon
        ok &= ((p - verts[k]) @ nrm) <= slack
    return ok


def polygon_moments(verts):
    """Mean [2] and second moment E[x x^T] [2, 2] of the uniform distribution over the fan of triangles (0, v_k, v_{k+1})."""
    n = len(verts) - 1
    area = np.array([0.5 * (verts[k][0] * verts[k + 1][1] - verts[k][1] * verts[k + 1][0]) for k in range(n)])
    mean, second = np.zeros(2), np.zeros((2, 2))
    for k in range(n):
        a, b = verts[k], verts[k + 1]
        mean += area[k] * (a + b) / 3.0
        second += area[k] * (np.outer(a, a) + np.outer(b, b) + np.outer(a + b, a + b)) / 12.0
    return mean / area.sum(), second / area.sum()


# ---- the oracle's random numbers and disc mapping (bit-identical to the product's by tests/test_gpu_parity.py and tests/test_oracle_kat.py)
def randoms(oracle, width, height, seeds):
    """orc_random(px, py, seed, 0) for every pixel and seed: float32 [len(seeds), height, width, 4]."""
    import ctypes as C
    L = oracle.lib()
    out = np.zeros((len(seeds), height, width, 4), f32)
    row = np.zeros(4, f32)
    p = row.ctypes.data_as(C.c_void_p)
    for i, seed in enumerate(seeds):
        for y in range(height):
            for x in range(width):
                L.orc_random(x, y, int(seed), 0, p)
                out[i, y, x] = row
    return out


def oracle_disk(oracle, u, v):
    """orc_square_to_disk(orc_uv_to_square({u, v})) per query: float64 [n, 2] of float32 values."""
    import ctypes as C
    L = oracle.lib()
    u, v = np.asarray(u, f32).ravel(), np.asarray(v, f32).ravel()
    out = np.zeros((len(u), 2), f32)
    a, b = np.zeros(2, f32), np.zeros(2, f32)
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    for i in range(len(u)):
        a[0], a[1] = u[i], v[i]
        L.orc_uv_to_square(pa, pb)
        L.orc_square_to_disk(pb, pa)
        out[i] = a
    return out.astype(f64)


def jittered(rnd, width, height):
    """Image positions of pt_trace's samples from their random numbers [..., height, width, 4], in float32 as the kernel adds them:
    sx = (px + 0.5) + (r.x - 0.5)."""
    px = np.arange(width, dtype=f32)[None, :] + f32(0.5)
    py = np.arange(height, dtype=f32)[:, None] + f32(0.5)
    return (px + (rnd[..., 0] - f32(0.5))).astype(f32), (py + (rnd[..., 1] - f32(0.5))).astype(f32)


# ---- the single-quad case (tests/test_gpu_lens.py item 4; its excluded share is computed in tests/test_lens_host.py) ------------------
# One quad in the plane y = QUAD_Y facing a camera at (0, -QUAD_CAMERA, 0) that looks along + y: view-space depth QUAD_Y + QUAD_CAMERA = 4,
# twice the focus distance, so a point of it blurs over a disc of 2 * aperture * (4 - 2) / 2 = 1 world unit = 5 pixels of the 72 x 40 frame
# (a pixel is 2 * 4 / 40 = 0.2 units there).  The quad covers about 30 x 20 pixels: its four edges and the diagonal cross many pixels.
QUAD_Y, QUAD_CAMERA, QUAD_HALF_X, QUAD_HALF_Z = 1.0, 3.0, 3.0, 2.0
QUAD_APERTURE, QUAD_FOCUS = 0.5, 2.0


def quad_coverage(o, d, tmax, slack):
    """Where the rays (float64) meet the quad's plane: hit [n] and near_edge [n] -- within `slack` [n] of one of the four edges or of the
    diagonal the two triangles share (a ray through it belongs to either triangle, and to neither only by rounding)."""
    t = (QUAD_Y - o[:, 1]) / d[:, 1]
    x, z = o[:, 0] + t * d[:, 0], o[:, 2] + t * d[:, 2]
    ok = (t > 0) & (t < tmax)
    hit = ok & (np.abs(x) <= QUAD_HALF_X) & (np.abs(z) <= QUAD_HALF_Z)
    edge = np.minimum(np.abs(np.abs(x) - QUAD_HALF_X), np.abs(np.abs(z) - QUAD_HALF_Z))
    inside_wide = (np.abs(x) <= QUAD_HALF_X + slack) & (np.abs(z) <= QUAD_HALF_Z + slack)
    diag = np.abs((x + QUAD_HALF_X) * QUAD_HALF_Z - (z + QUAD_HALF_Z) * QUAD_HALF_X) / math.hypot(QUAD_HALF_X, QUAD_HALF_Z)
    near = ok & inside_wide & ((edge <= slack) | (diag <= slack))
    return hit, near
