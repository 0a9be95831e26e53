"""pt_motion_blur (include/mipt.h) restated in numpy float32, rounding for rounding: every product, sum, quotient and square root below is
one float32 operation in the header's order, so a device result is held to it bit for bit.  Vectorised over pixels, a loop over taps.

blur(color, motion, ...) -> (out, info).  info holds the intermediates and the masks the tests assert their inputs with:
    V (H, W, 4), T and N (tiles_y, tiles_x, 3)
    blurred    (H, W) bool   the pixels that went through the gather (ln >= 0.5 in their tile and a finite centre colour)
    counted    (H, W) int    per pixel, the taps that were not skipped (inside the image, finite colour); 0 where not blurred
    clamped    (H, W) bool   moving pixels whose streak was cut to max_radius
    slow       (H, W) bool   moving pixels with 0 < l < 0.5
    uncovered  (H, W) bool   pixels without a positive finite depth
    bad_centre (H, W) bool   pixels with a non-finite colour component
"""
import numpy as np

f32 = np.float32
TILE = 16
DEFAULTS = dict(shutter=0.5, max_radius=32.0, taps=16, jitter=1, depth_softness=0.05)


def _fract(a):
    return (a - np.floor(a)).astype(f32)


def _clamp01(a):
    return np.fmin(np.fmax(a, f32(0)), f32(1)).astype(f32)         # fminf(fmaxf(a, 0), 1): a NaN gives 0


def prepare(motion, shutter, max_radius):
    """-> V (H, W, 4) float32 and the masks (moving, clamped, covered)."""
    m = np.ascontiguousarray(motion, f32)
    h = f32(0.5) * f32(shutter)
    R = f32(max_radius)
    with np.errstate(all="ignore"):
        covered = np.isfinite(m[..., 3]) & (m[..., 3] > 0)
        z = np.where(covered, m[..., 3], f32(np.inf)).astype(f32)
        vx = ((-m[..., 0]) * h).astype(f32)
        vy = ((-m[..., 1]) * h).astype(f32)
        l = np.sqrt((vx * vx + vy * vy).astype(f32)).astype(f32)
        moving = covered & np.isfinite(m[..., 0]) & np.isfinite(m[..., 1]) & np.isfinite(m[..., 2]) & (m[..., 2] > 0) & np.isfinite(l)
        over = l > R
        k = (R / np.where(over, l, f32(1))).astype(f32)
        vx = np.where(over, (vx * k).astype(f32), vx)
        vy = np.where(over, (vy * k).astype(f32), vy)
        l = np.where(over, R, l)
    zero = f32(0)
    vx, vy, l = np.where(moving, vx, zero), np.where(moving, vy, zero), np.where(moving, l, zero)
    V = np.stack([vx, vy, l, z], axis=-1).astype(f32)
    assert not np.isnan(V).any()
    return V, moving, moving & over, covered


def tile_max(V):
    H, W = V.shape[:2]
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    T = np.zeros((ty, tx, 3), f32)
    for j in range(ty):
        for i in range(tx):
            blk = V[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE]
            y, x = np.unravel_index(np.argmax(blk[..., 2]), blk.shape[:2])      # the first of the largest in row-major order: the least (y, x)
            T[j, i] = blk[y, x, :3]
    return T


def neighbour_max(T, max_radius):
    ty, tx = T.shape[:2]
    r = int(np.ceil(f32(max_radius) / f32(16.0)))
    N = np.zeros_like(T)
    for j in range(ty):
        for i in range(tx):
            best, best_l = None, f32(-1)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    y, x = j + dy, i + dx
                    if 0 <= y < ty and 0 <= x < tx and T[y, x, 2] > best_l:
                        best, best_l = T[y, x], T[y, x, 2]
            N[j, i] = best
    return N


def blur(color, motion, shutter=0.5, max_radius=32.0, taps=16, jitter=1, depth_softness=0.05):
    c = np.ascontiguousarray(color, f32)
    H, W = c.shape[:2]
    V, moving, clamped, covered = prepare(motion, shutter, max_radius)
    T = tile_max(V)
    N = neighbour_max(T, max_radius)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Np = N[ys // TILE, xs // TILE]
    nx, ny, ln = Np[..., 0], Np[..., 1], Np[..., 2]
    finite_c = np.isfinite(c[..., :3]).all(axis=-1)
    blurred = (ln >= f32(0.5)) & finite_c
    xf, yf = xs.astype(f32), ys.astype(f32)
    soft = f32(depth_softness)
    one, zero = f32(1), f32(0)
    with np.errstate(all="ignore"):
        if jitter:
            u = ((f32(0.06711056) * xf).astype(f32) + (f32(0.00583715) * yf).astype(f32)).astype(f32)
            g = _fract((f32(52.9829189) * _fract(u)).astype(f32))
        else:
            g = np.full((H, W), 0.5, f32)
        lp, zp = V[..., 2], V[..., 3]
        wc = (one / np.fmax(lp, f32(0.5))).astype(f32)
        sw = wc.copy()
        s = (wc[..., None] * np.where(finite_c[..., None], c[..., :3], zero)).astype(f32)
        cx, cy = (xf + f32(0.5)).astype(f32), (yf + f32(0.5)).astype(f32)
        counted = np.zeros((H, W), np.int32)

        def cone(d, l):
            return np.where(l > d, (one - (d / np.where(l > d, l, one)).astype(f32)).astype(f32), zero)

        def cyl(d, l):
            return np.where(l >= d, one, zero)

        for i in range(int(taps)):
            tau = ((((f32(i) + g).astype(f32) / f32(taps)).astype(f32) * f32(2.0)).astype(f32) - one).astype(f32)
            qx = np.floor((cx + (tau * nx).astype(f32)).astype(f32)).astype(np.int64)
            qy = np.floor((cy + (tau * ny).astype(f32)).astype(f32)).astype(np.int64)
            inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            d = (np.abs(tau) * ln).astype(f32)
            Vq, cq = V[qyc, qxc], c[qyc, qxc]
            lq, zq = Vq[..., 2], Vq[..., 3]
            ok = inside & np.isfinite(cq[..., :3]).all(axis=-1)
            same = zp == zq
            e = (soft * np.fmin(zp, zq)).astype(f32)
            fg = np.where(same, one, _clamp01((one - ((zq - zp).astype(f32) / e).astype(f32)).astype(f32)))
            bg = np.where(same, one, _clamp01((one - ((zp - zq).astype(f32) / e).astype(f32)).astype(f32)))
            w = (((fg * cone(d, lq)).astype(f32) + (bg * cone(d, lp)).astype(f32)).astype(f32) +
                 (f32(2.0) * (cyl(d, lq) * cyl(d, lp)).astype(f32)).astype(f32)).astype(f32)
            sw = np.where(ok, (sw + w).astype(f32), sw)
            s = np.where(ok[..., None], (s + (w[..., None] * np.where(ok[..., None], cq[..., :3], zero)).astype(f32)).astype(f32), s)
            counted += (ok & blurred).astype(np.int32)
        rgb = (s / sw[..., None]).astype(f32)
    out = c.copy()
    out[..., :3] = np.where(blurred[..., None], rgb, c[..., :3])
    info = dict(V=V, T=T, N=N, blurred=blurred, counted=counted, clamped=clamped, slow=moving & (V[..., 2] > 0) & (V[..., 2] < f32(0.5)),
                uncovered=~covered, bad_centre=~finite_c, moving=moving)
    return out, info


# ---- the fields the tests run on --------------------------------------------------------------------------------------------------------
def random_field(rng, w, h, confine=None):
    """-> (color, motion): colour uniform in [0, 1) with a tenth of the pixels fifty times as bright; depths from {2, 2.05, 4, 8}; per pixel
    one of four kinds of motion (none, a twentieth of uniform(-20, 20), that, eight times that); the previous depth zeroed on 5 % and the
    current depth on 10 % of the pixels; max(4, w * h / 40) NaN or infinite entries in each image.  confine = (lo, hi): motion only where both
    x and y lie in lo..hi."""
    color = rng.random((h, w, 4)).astype(f32)
    color[rng.random((h, w)) < 0.1] *= f32(50)
    depth = rng.choice(np.array([2.0, 2.05, 4.0, 8.0], f32), (h, w)).astype(f32)
    kind = rng.integers(0, 4, (h, w))
    vec = rng.uniform(-20, 20, (h, w, 2)).astype(f32)
    vec[kind == 0] = 0
    vec[kind == 1] *= f32(0.05)
    vec[kind == 3] *= f32(8)
    if confine is not None:
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        lo, hi = confine
        vec[~((xs >= lo) & (xs <= hi) & (ys >= lo) & (ys <= hi))] = 0
    motion = np.zeros((h, w, 4), f32)
    motion[..., :2] = vec
    motion[..., 2] = depth
    motion[..., 3] = depth
    motion[..., 2][rng.random((h, w)) < 0.05] = 0
    motion[..., 3][rng.random((h, w)) < 0.10] = 0
    specials = np.array([np.nan, np.inf, -np.inf], f32)
    for img in (color, motion):
        for _ in range(max(4, w * h // 40)):
            img[rng.integers(h), rng.integers(w), rng.integers(4)] = rng.choice(specials)
    return color, motion


BLOCK = (slice(4, 11), slice(5, 11))                       # rows 4..10, columns 5..10: 7 high, 6 wide, inside 17 x 33 and 40 x 24


def block_field(rng, w, h):
    """-> (color, motion, on_block): a bright 6 x 7 block at depth 2 with motion (-12, 5) over static ground at depth 8, three rows of misses
    on top.  The ground and the sky are darker than every block pixel."""
    color = np.zeros((h, w, 4), f32)
    color[..., :3] = (0.1 + 0.2 * rng.random((h, w, 3))).astype(f32)
    color[..., 3] = rng.random((h, w)).astype(f32)
    motion = np.zeros((h, w, 4), f32)
    motion[..., 2] = motion[..., 3] = 8.0
    motion[:3] = 0                                         # misses: no depth, no record
    color[BLOCK][..., :3] = (4.0 + rng.random((7, 6, 3))).astype(f32)
    motion[BLOCK] = np.array([-12.0, 5.0, 2.0, 2.0], f32)
    on_block = np.zeros((h, w), bool)
    on_block[BLOCK] = True
    return color, motion, on_block
