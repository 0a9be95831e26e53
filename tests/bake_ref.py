"""Restatement of texture-space baking (include/mipt.h pt_set_bake, pt_bake_coverage, pt_bake_dilate) in numpy.

coverage(): the coverage map in float32.  numpy rounds every float32 product, sum and difference on its own, in the order written, which is what
the kernels do (csrc/bake.hip and csrc/pt_bake.h are compiled without contraction): the comparison with the GPU is exact, texel for texel.

ray(): the sample's ray in float64 from the float32 inputs (the UVs, the world-space packet, the random draw, the offset).  The kernel's float32
result is held to
    |o - o_ref| <= RAY_ROUNDINGS * 2^-24 * K * (max|v0| + max|e1| + max|e2| + surface_offset)          per component
    |d - d_ref| <= NORMAL_ROUNDINGS * 2^-24 * Kn
The roundings on the longest chain from an input to a component of o, counted along the header's lines:
    p = px + 0.5 + (r - 0.5)                                 2      (the subtraction, the sum; px + 0.5 is exact)
    E(C, A, p): a difference, a product, the subtraction     3      (the UV vertex u * W is one rounding too, but on the shorter branch)
    b = E / area2                                            1
    b0 = max((1 - b1) - b2, 0)                               2
    s = (b0 + b1) + b2                                       2
    b = b / s                                                1
    b = b * (1 - 2^-10) + c                                  2
    P = (v0 + b1 * e1) + b2 * e2                             3      (product, sum, sum)
    o = P + Ng * offset                                      2      (product, sum; Ng's own chain below is shorter)
                                                            --
                                                 RAY_ROUNDINGS = 18
and to a component of d = -Ng:  cross 2 (product, difference), dot(n, n) 3, sqrt 1, n / len 1:  NORMAL_ROUNDINGS = 7.
Each rounding is at most 2^-24 of its result.  Two of the steps subtract nearly equal numbers, which is where a relative error grows, and the
bound carries their condition numbers: K = max(1, the largest |product| inside the three edge functions / |area2|) -- what an error of a product
becomes in a barycentric coordinate -- and Kn = max(1, the largest |product| inside cross(e1, e2) / |n|).  Both are 1..4 for the charts of
tests/test_gpu_bake.py; a sliver chart has a large K and the bound says so.

dilate(): pt_bake_dilate in float32, sums in the header's order.
"""
import numpy as np

f32, f64 = np.float32, np.float64
NONE = 0xFFFFFFFF
RAY_ROUNDINGS = 18
NORMAL_ROUNDINGS = 7
KEEP = f32(1.0) - f32(2.0 ** -10)
THIRD = f32(2.0 ** -10 / 3.0)


class Tri:
    """One triangle as the tree holds it: instance row, triangle within the instance, the three UVs of each set (None: the instance has no such
    stream), the world-space packet v0, e1 = v1 - v0, e2 = v2 - v0 (float32) and whether the instance is mirrored."""

    def __init__(self, inst, prim, uv, v0, e1, e2, mirrored):
        self.inst, self.prim, self.uv, self.mirrored = int(inst), int(prim), uv, bool(mirrored)
        self.v0, self.e1, self.e2 = (np.asarray(a, f32) for a in (v0, e1, e2))


def scene_triangles(scene, uv_override=None):
    """The triangles of a gltf_renderer_amd.scenes.SceneData whose instance transforms are exact in float32 (asserted): the world-space vertices
    are then the float32 values the builder computes, and e1, e2 one float32 subtraction each.  uv_override: {(instance, set): [n, 2] array}
    replaces a UV stream (a pt_buffer_update)."""
    out = []
    for inst, (mesh, T, _) in enumerate(scene.mesh_records):
        T = np.asarray(T, f64)
        w64 = mesh.positions.astype(f64) @ T[:3, :3].T + T[:3, 3]
        w = w64.astype(f32)
        assert np.array_equal(w.astype(f64), w64), "instance %d: the transform is not exact in float32" % inst
        idx = mesh.indices if mesh.indices is not None else np.arange(len(mesh.positions))
        idx = np.asarray(idx, np.int64).reshape(-1, 3)
        sets = []
        for k, uv in enumerate((mesh.uv0, mesh.uv1)):
            if uv_override and (inst, k) in uv_override:
                uv = np.asarray(uv_override[(inst, k)], f32)
            sets.append(uv)
        mirrored = np.linalg.det(T[:3, :3]) < 0
        for prim, (a, b, c) in enumerate(idx):
            uv = [None if s is None else np.asarray(s, f32)[[a, b, c]] for s in sets]
            out.append(Tri(inst, prim, uv, w[a], w[b] - w[a], w[c] - w[a], mirrored))
    return out


def edge(P, Q, p):
    """E(P, Q, p) = (Q.x - P.x)(p.y - P.y) - (Q.y - P.y)(p.x - P.x); the dtype of the operands (float32: every operation rounded)."""
    return (Q[..., 0] - P[..., 0]) * (p[..., 1] - P[..., 1]) - (Q[..., 1] - P[..., 1]) * (p[..., 0] - P[..., 0])


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def texel_uv(t, tex_coord, W, H):
    """A, B, C in texel units and area2 (float32), or None for skip test 1 / no stream."""
    uv = t.uv[tex_coord]
    if uv is None:
        return None
    with np.errstate(all="ignore"):
        A, B, C = (uv[k] * np.array([W, H], f32) for k in range(3))
        area2 = edge(A, B, C)
    if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()) or area2 == 0:
        return None
    return A, B, C, area2


def world_normal(t):
    """n = cross(e1, e2) and its length (float32), or None for skip test 2."""
    with np.errstate(all="ignore"):
        n = cross(t.e1, t.e2)
        ln = np.sqrt(dot(n, n))
    if not (ln > 0 and np.isfinite(ln)):
        return None
    return n, ln


def participates(t, tex_coord, instance, W, H):
    if instance >= 0 and t.inst != instance:
        return None
    uvs = texel_uv(t, tex_coord, W, H)
    if uvs is None or world_normal(t) is None:
        return None
    return uvs


def covers(A, B, C, area2, p):
    positive = area2 > 0
    with np.errstate(all="ignore"):
        e0, e1, e2 = edge(B, C, p), edge(C, A, p), edge(A, B, p)
    inside = lambda e: (e == 0) | ((e > 0) == positive)
    return inside(e0) & inside(e1) & inside(e2)


def coverage(tris, W, H, tex_coord=0, instance=-1):
    """(instance [H, W] int32, -1 where none; primitive [H, W] uint32, NONE where none; index into `tris` [H, W] int64, -1 where none)."""
    ys, xs = np.mgrid[0:H, 0:W]
    p = np.stack([xs.astype(f32) + f32(0.5), ys.astype(f32) + f32(0.5)], axis=-1)
    inst = np.full((H, W), -1, np.int32)
    prim = np.full((H, W), NONE, np.uint32)
    which = np.full((H, W), -1, np.int64)
    for k in sorted(range(len(tris)), key=lambda k: (tris[k].inst, tris[k].prim)):          # ascending: the first to cover a texel owns it
        t = tris[k]
        uvs = participates(t, tex_coord, instance, W, H)
        if uvs is None:
            continue
        new = covers(*uvs, p) & (which < 0)
        inst[new], prim[new], which[new] = t.inst, t.prim, k
    return inst, prim, which


def ray(t, tex_coord, W, H, px, py, r, offset):
    """The sample's ray in float64: (o [3], d [3], tmax, bound_o, bound_d).  r = the draw's (x, y), float32; t = the texel's owner."""
    A, B, C, _ = texel_uv(t, tex_coord, W, H)
    A, B, C = A.astype(f64), B.astype(f64), C.astype(f64)
    area2 = edge(A, B, C)
    p = np.array([px + 0.5 + (f64(r[0]) - 0.5), py + 0.5 + (f64(r[1]) - 0.5)])
    b1, b2 = edge(C, A, p) / area2, edge(A, B, p) / area2
    b1, b2 = max(b1, 0.0), max(b2, 0.0)
    b0 = max((1.0 - b1) - b2, 0.0)
    s = (b0 + b1) + b2
    b1, b2 = b1 / s, b2 / s
    b1, b2 = b1 * f64(KEEP) + f64(THIRD), b2 * f64(KEEP) + f64(THIRD)
    v0, e1, e2 = t.v0.astype(f64), t.e1.astype(f64), t.e2.astype(f64)
    P = (v0 + b1 * e1) + b2 * e2
    n = cross(e1, e2)
    if t.mirrored:
        n = -n
    ln = np.sqrt(dot(n, n))
    Ng = n / ln
    off = f64(f32(offset))
    # the condition numbers of the two cancelling steps (module docstring)
    prods = [abs((Q[0] - P_[0]) * (q[1] - P_[1])) for P_, Q, q in ((B, C, p), (C, A, p), (A, B, p), (A, B, C))] + \
            [abs((Q[1] - P_[1]) * (q[0] - P_[0])) for P_, Q, q in ((B, C, p), (C, A, p), (A, B, p), (A, B, C))]
    K = max(1.0, max(prods) / abs(area2))
    cp = [abs(e1[i] * e2[j]) for i in range(3) for j in range(3) if i != j]
    Kn = max(1.0, max(cp) / ln)
    M = np.abs(v0).max() + np.abs(e1).max() + np.abs(e2).max() + off
    return P + Ng * off, -Ng, 2.0 * off, RAY_ROUNDINGS * 2.0 ** -24 * K * M, NORMAL_ROUNDINGS * 2.0 ** -24 * Kn


def sample_uv(t, tex_coord, W, H, px, py, r):
    """The sample's own atlas position as a UV (float64): its jittered position p / (W, H), clamped onto the owner like the ray's start, before
    the shrink; and the largest extent |u| or |v| of an edge of the owner's UV triangle (what the shrink's 2^-10 scales with)."""
    A, B, C, _ = texel_uv(t, tex_coord, W, H)
    A, B, C = A.astype(f64), B.astype(f64), C.astype(f64)
    area2 = edge(A, B, C)
    p = np.array([px + 0.5 + (f64(r[0]) - 0.5), py + 0.5 + (f64(r[1]) - 0.5)])
    b1, b2 = max(edge(C, A, p) / area2, 0.0), max(edge(A, B, p) / area2, 0.0)
    b0 = max((1.0 - b1) - b2, 0.0)
    s = (b0 + b1) + b2
    b0, b1, b2 = b0 / s, b1 / s, b2 / s
    uv = t.uv[tex_coord].astype(f64)
    extent = max(np.abs(uv[i] - uv[j]).max() for i, j in ((0, 1), (1, 2), (2, 0)))
    return b0 * uv[0] + b1 * uv[1] + b2 * uv[2], extent


def clamped_barycentrics(A, B, C, p):
    """(b0, b1, b2) of the header's clamp, before the shrink, in float32 (for the hand-worked cases)."""
    A, B, C, p = (np.asarray(a, f32) for a in (A, B, C, p))
    area2 = edge(A, B, C)
    b1, b2 = edge(C, A, p) / area2, edge(A, B, p) / area2
    b1, b2 = max(b1, f32(0)), max(b2, f32(0))
    b0 = max((f32(1) - b1) - b2, f32(0))
    s = (b0 + b1) + b2
    b1, b2 = b1 / s, b2 / s
    return f32(1) - b1 - b2, b1, b2


def dilate(image, filled, passes):
    """pt_bake_dilate: image [H, W, 4] float32, filled [H, W] bool (the coverage) -> (image, filled) after `passes` passes."""
    img = np.array(image, f32)
    fill = np.array(filled, bool)
    H, W = fill.shape
    for _ in range(passes):
        out, nfill = img.copy(), fill.copy()
        for y, x in zip(*np.nonzero(~fill)):
            s = np.zeros(4, f32)
            count = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qx, qy = x + dx, y + dy
                    if (dx == 0 and dy == 0) or qx < 0 or qy < 0 or qx >= W or qy >= H or not fill[qy, qx]:
                        continue
                    with np.errstate(all="ignore"):
                        s = s + img[qy, qx]
                    count += 1
            if count > 0:
                with np.errstate(all="ignore"):
                    out[y, x] = s / f32(count)
                nfill[y, x] = True
        img, fill = out, nfill
    return img, fill
