"""Restatement of motion vectors and temporal reprojection (include/mipt.h pt_set_motion, pt_reproject) in numpy.

record(): one sample's record, in the dtype of its inputs.  In float32 numpy rounds every product, sum, difference and quotient on its own,
in the order written -- what the kernels do (csrc/pt_motion.h is compiled without contraction, fdiv is the rounded quotient): a restatement
rounding for rounding.  In float64 it is the reference the GPU's float32 records are held to.

The float64 reference of tests/test_gpu_motion.py does not start from the tree's packets: world_points() forms the hit point from the scene's
object-space vertices and the instance transform, all float32 values taken as exact, with the hit's (u, v):
    w_k = T p_k,   P = w_0 + u (w_1 - w_0) + v (w_2 - w_0)                                     (float64)
The matrices Mc, Mp, Vc, Vp are float32 inputs of the definition (world_to_clip() forms Mc and Mp as the library does), taken as exact too.
record_bound() then bounds |record_f32 - record_f64| per component.  eps = 2^-24, every rounding at most eps of its result.
  The packet (the build's mul_point, then k_setup's differences):
    w_k,i = ((T_i0 x + T_i1 y) + T_i2 z) + T_i3      three products, three sums: |err| <= 4 eps Sw_i,  Sw_i = sum_j |T_ij| |p_j| + |T_i3|
                                                     (the four-term dot-product bound; max over the triangle's three vertices)
    e = w_k - w_0                                    both vertices' errors and one rounding of |e| <= 2 Sw:  |err| <= (4 + 4 + 2) eps Sw = 10 eps Sw
  The point (the header's line):
    P = (v0 + u e1) + v e2                           inherited: 4 + 10 (u + v) <= 14 (u, v >= 0, u + v <= 1, asserted by the test);
                                                     three roundings (product, sum, sum) of magnitudes <= 3 Sw: 9
                                                     |P_f32 - P_f64| <= P_ROUNDINGS eps Sw,  P_ROUNDINGS = 23
  The projection, for a row r of M (k = 0, 1, 3) or of V (k = 2):
    c = ((r0 Px + r1 Py) + r2 Pz) + r3               |err| <= sum_j |r_j| dP_j + DOT_ROUNDINGS eps Sc,  Sc = sum_j |r_j| |P_j| + |r3|,  DOT_ROUNDINGS = 4
    q = fdiv(c_k, c_3)                               |err| <= (dc_k + |q| dc_3) / (|c_3| - dc_3) + eps |q|       -- the condition of the projection
    s = ((q + 1) * 0.5) * W   (1 - q for y)          |err| <= (W / 2) (dq + eps |q + 1|) + eps |s|               (* 0.5 is exact)
    x = s_prev - s_cur                               |err| <= ds_prev + ds_cur + eps |x|
    z = -c_2                                         |err| <= dc_2
The bound is derived from these counts alone; nothing in it was fitted to what a GPU produced.  It needs |c_3| well above dc_3: the tests choose
cameras that keep every tested point in front of both cameras by a clear margin and assert it.

reproject(): pt_reproject in float32, sums in the header's order.
"""
import numpy as np

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24
P_ROUNDINGS = 23
DOT_ROUNDINGS = 4


def world_to_clip(view_to_clip, world_to_view):
    """The library's mat4_mul in float32 on glm column-major 16-vectors: out[4c + r] = sum over k ascending, from 0.0f, of a[4k + r] * b[4c + k]."""
    a, b = np.asarray(view_to_clip, f32).reshape(16), np.asarray(world_to_view, f32).reshape(16)
    out = np.zeros(16, f32)
    for c in range(4):
        for r in range(4):
            s = f32(0)
            for k in range(4):
                s = f32(s + f32(a[4 * k + r] * b[4 * c + k]))
            out[4 * c + r] = s
    return out


def point(v0, e1, e2, u, v):
    """P = (v0 + u * e1) + v * e2, componentwise; arrays (..., 3) and (...,) of one dtype."""
    return (v0 + u[..., None] * e1) + v[..., None] * e2


def row(M, k, P):
    """((M[k] P.x + M[4+k] P.y) + M[8+k] P.z) + M[12+k] for a column-major 16-vector M of P's dtype."""
    return ((M[k] * P[..., 0] + M[4 + k] * P[..., 1]) + M[8 + k] * P[..., 2]) + M[12 + k]


def screen(M, P, W, H):
    dt = P.dtype.type
    with np.errstate(all="ignore"):
        c0, c1, c3 = row(M, 0, P), row(M, 1, P), row(M, 3, P)
        sx = ((c0 / c3 + dt(1)) * dt(0.5)) * dt(W)
        sy = ((dt(1) - c1 / c3) * dt(0.5)) * dt(H)
    return sx, sy


def record_points(Pc, Pp, Mc, Mp, Vc, Vp, W, H):
    """The record of current / previous world points (..., 3), in their dtype; a non-finite record gives zeros."""
    dt = Pc.dtype
    Mc, Mp, Vc, Vp = (np.asarray(m).astype(dt).reshape(16) for m in (Mc, Mp, Vc, Vp))
    sxc, syc = screen(Mc, Pc, W, H)
    sxp, syp = screen(Mp, Pp, W, H)
    with np.errstate(all="ignore"):
        rec = np.stack([sxp - sxc, syp - syc, -row(Vp, 2, Pp), -row(Vc, 2, Pc)], axis=-1)
    rec[~np.isfinite(rec).all(axis=-1)] = 0
    return rec


def record(cur, prev, u, v, Mc, Mp, Vc, Vp, W, H, dtype=f32):
    """cur, prev: (v0, e1, e2) triples of (..., 3) arrays -- the hit packet and its snapshot entry (prev = cur without a valid snapshot)."""
    u, v = np.asarray(u).astype(dtype), np.asarray(v).astype(dtype)
    Pc = point(*(np.asarray(a).astype(dtype) for a in cur), u, v)
    Pp = point(*(np.asarray(a).astype(dtype) for a in prev), u, v)
    return record_points(Pc, Pp, Mc, Mp, Vc, Vp, W, H)


def world_points(positions, T, tri, u, v):
    """float64, from the object-space vertices: positions (n, 3) float32, T a 4x4 (row, column) matrix of float32 values, tri (q, 3) vertex
    indices of each query's triangle, (u, v) the hit's barycentrics.  Returns (P (q, 3), Sw (q, 3)): the point and the packet's scale."""
    T = np.asarray(T, f32).astype(f64)
    p = np.asarray(positions, f32).astype(f64)[np.asarray(tri, np.int64)]                 # (q, 3 vertices, 3)
    w = p @ T[:3, :3].T + T[:3, 3]
    Sw = (np.abs(p) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max(axis=1)
    u, v = np.asarray(u, f64)[:, None], np.asarray(v, f64)[:, None]
    return w[:, 0] + u * (w[:, 1] - w[:, 0]) + v * (w[:, 2] - w[:, 0]), Sw


def _row_err(M, k, P, dP):
    r = np.abs(np.asarray(M, f64).reshape(16)[[k, 4 + k, 8 + k, 12 + k]])
    return (r[:3] * dP).sum(axis=-1) + DOT_ROUNDINGS * EPS * ((r[:3] * np.abs(P)).sum(axis=-1) + r[3])


def _screen_err(M, P, dP, size, axis):
    M = np.asarray(M, f64).reshape(16)
    c, c3 = row(M, axis, P), row(M, 3, P)
    dc, dc3 = _row_err(M, axis, P, dP), _row_err(M, 3, P, dP)
    q = c / c3
    room = np.abs(c3) - dc3
    assert np.all(room > 0), "a tested point is too close to a camera plane for the bound"
    dq = (dc + np.abs(q) * dc3) / room + EPS * np.abs(q)
    lin = q + 1 if axis == 0 else 1 - q
    return (size / 2.0) * (dq + EPS * np.abs(lin)) + EPS * np.abs(lin * 0.5 * size)


def record_bound(Pc, Swc, Pp, Swp, Mc, Mp, Vc, Vp, W, H, rec):
    """Per query and component, the bound on |record_f32 - record_f64| derived in the module's docstring.  Pc, Pp: the float64 points;
    Swc, Swp: their packets' scales (world_points); rec: the float64 record."""
    dPc, dPp = P_ROUNDINGS * EPS * Swc, P_ROUNDINGS * EPS * Swp
    out = np.zeros(rec.shape, f64)
    out[..., 0] = _screen_err(Mp, Pp, dPp, W, 0) + _screen_err(Mc, Pc, dPc, W, 0) + EPS * np.abs(rec[..., 0])
    out[..., 1] = _screen_err(Mp, Pp, dPp, H, 1) + _screen_err(Mc, Pc, dPc, H, 1) + EPS * np.abs(rec[..., 1])
    out[..., 2] = _row_err(Vp, 2, Pp, dPp)
    out[..., 3] = _row_err(Vc, 2, Pc, dPc)
    return out


def clip_w(M, P):
    return row(np.asarray(M, f64).reshape(16), 3, np.asarray(P, f64))


# ---- pt_reproject ----------------------------------------------------------------------------------------------------------------------
def reproject(color, motion, prev_color, prev_motion, prev_length=None, alpha_min=0.1, max_history=32.0, depth_tolerance=0.02):
    """-> (out_color (H, W, 4), out_length (H, W), usable (H, W) bool: the pixels that blended), float32 throughout."""
    c, m, pc, pm = (np.ascontiguousarray(a, f32) for a in (color, motion, prev_color, prev_motion))
    H, W = c.shape[:2]
    pl = np.ones((H, W), f32) if prev_length is None else np.ascontiguousarray(prev_length, f32)
    alpha_min, max_history, tol = f32(alpha_min), f32(max_history), f32(depth_tolerance)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        sx = xs.astype(f32) + m[..., 0]
        sy = ys.astype(f32) + m[..., 1]
        usable = np.isfinite(m).all(axis=-1) & (m[..., 3] > 0) & (m[..., 2] > 0) & (sx > -1) & (sx < f32(W)) & (sy > -1) & (sy < f32(H))
        sxs, sys_ = np.where(usable, sx, f32(0)), np.where(usable, sy, f32(0))
        x0, y0 = np.floor(sxs), np.floor(sys_)
        fx, fy = (sxs - x0).astype(f32), (sys_ - y0).astype(f32)
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        ws = np.zeros((H, W), f32); hist = np.zeros((H, W, 3), f32); hl = np.zeros((H, W), f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                inside = usable & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                tm, tc, tl = pm[cy, cx], pc[cy, cx], pl[cy, cx]
                b = ((fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)).astype(f32)
                counts = inside & np.isfinite(tm).all(axis=-1) & (tm[..., 3] > 0) & (np.abs(tm[..., 3] - m[..., 2]) <= tol * m[..., 2]) & \
                    np.isfinite(tc[..., :3]).all(axis=-1) & np.isfinite(tl) & (tl >= 1)
                ws = np.where(counts, ws + b, ws)
                hist = np.where(counts[..., None], hist + b[..., None] * tc[..., :3], hist)
                hl = np.where(counts, hl + b * tl, hl)
        blended = usable & (ws > 0)
        safe = np.where(blended, ws, f32(1))
        hist = (hist / safe[..., None]).astype(f32)
        hl = (hl / safe).astype(f32)
        n = np.minimum(hl + f32(1), max_history).astype(f32)
        a = np.maximum(f32(1) / n, alpha_min).astype(f32)
        rgb = (hist + a[..., None] * (c[..., :3] - hist)).astype(f32)
    out = c.copy()
    out[..., :3] = np.where(blended[..., None], rgb, c[..., :3])
    length = np.where(blended, n, f32(1)).astype(f32)
    return out, length, blended
