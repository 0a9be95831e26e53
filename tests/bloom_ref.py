"""pt_bloom (include/mipt.h) restated in numpy, rounding for rounding: every product, sum and quotient below is one operation of `dtype` in the
header's order, so with dtype = float32 (the default) a device result is held to it bit for bit, and with dtype = float64 the same text gives
the figure the float32 chain is measured against.  Vectorised over a level's pixels; a tap's x and y parts are formed once per column and row.

bloom(color, iterations, strength, threshold, dtype) -> (out, info).  info holds
    sizes        [(w_k, h_k)] for k = 1 .. n                    the levels the run has (n = len(sizes))
    down         [M_k as the down steps left it]                (h_k, w_k, 3) each
    levels       [M_k after the pyramid walk]                   M_n is its down[n - 1]
    glow         (H, W, 3)                                      U = up(M_1) at full size; zeros when the call is a copy
    nonfinite    (H, W) bool   a component of c.rgb is NaN or infinite: the pixel is copied
    negative     (H, W) bool   a finite pixel with a component below 0
    clamped      (H, W) bool   a pixel with a component above 65504 (+inf included)
    below        (H, W) bool   threshold > 0 and the prefiltered pixel's largest component is not above it: it feeds nothing
"""
import numpy as np

f32, f64 = np.float32, np.float64
DEFAULTS = dict(iterations=4, strength=0.01, threshold=0.0)
HALF_MAX = 65504.0


def level_sizes(w, h, iterations):
    """The reference's NextMipSize, level by level, stopping after the first level that is 1 x 1."""
    sizes = []
    for _ in range(int(iterations)):
        if (w, h) == (1, 1):
            break
        w, h = max(w // 2, 1), max(h // 2, 1)
        sizes.append((w, h))
    return sizes


def prefilter(color, threshold, dt):
    """-> (B (H, W, 3), below): the texel the first down step fetches."""
    c = np.ascontiguousarray(color)[..., :3]
    with np.errstate(all="ignore"):
        b = np.where(c > 0, np.fmin(c, f32(HALF_MAX)), f32(0)).astype(dt)        # a select: NaN, negatives and -0 give +0, +inf gives 65504
        below = np.zeros(b.shape[:2], bool)
        thr = dt(f32(threshold))
        if thr > 0:
            L = np.fmax(np.fmax(b[..., 0], b[..., 1]), b[..., 2])
            over = L > thr
            k = np.where(over, ((L - thr).astype(dt) / np.where(over, L, dt(1))).astype(dt), dt(0)).astype(dt)
            b = (b * k[..., None]).astype(dt)
            below = ~over
    return b, below


def _axis(u, n, dt):
    """One axis of the bilinear tap at coordinates u of a level n texels long: (i0, i1, f)."""
    s = ((u * dt(n)).astype(dt) - dt(0.5)).astype(dt)
    i0f = np.floor(s).astype(dt)
    f = (s - i0f).astype(dt)
    i = i0f.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), f


def _tap(T, X, Y, dt):
    """S(T, u, v) over the grid of the column coordinates behind X and the row coordinates behind Y."""
    x0, x1, fx = X
    y0, y1, fy = Y
    fx, fy = fx[None, :, None], fy[:, None, None]
    r0, r1 = T[y0], T[y1]
    a = (r0[:, x0] + (fx * (r0[:, x1] - r0[:, x0]).astype(dt)).astype(dt)).astype(dt)
    b = (r1[:, x0] + (fx * (r1[:, x1] - r1[:, x0]).astype(dt)).astype(dt)).astype(dt)
    return (a + (fy * (b - a).astype(dt)).astype(dt)).astype(dt)


def _coords(wo, ho, dt):
    u = ((np.arange(wo).astype(dt) + dt(0.5)).astype(dt) / dt(wo)).astype(dt)
    v = ((np.arange(ho).astype(dt) + dt(0.5)).astype(dt) / dt(ho)).astype(dt)
    return u, v


def down(T, wo, ho, dt):
    hi, wi = T.shape[:2]
    u, v = _coords(wo, ho, dt)
    ox, oy = (dt(0.5) / dt(wo)).astype(dt), (dt(0.5) / dt(ho)).astype(dt)
    X = {s: _axis((u + dt(s) * ox).astype(dt), wi, dt) for s in (-1, 0, 1)}          # (+-1) * ox is exact
    Y = {s: _axis((v + dt(s) * oy).astype(dt), hi, dt) for s in (-1, 0, 1)}
    r = (dt(4.0) * _tap(T, X[0], Y[0], dt)).astype(dt)
    for sx, sy in ((1, 1), (-1, -1), (-1, 1), (1, -1)):
        r = (r + _tap(T, X[sx], Y[sy], dt)).astype(dt)
    return (r / dt(8.0)).astype(dt)


def up(T, wo, ho, dt):
    hi, wi = T.shape[:2]
    u, v = _coords(wo, ho, dt)
    ox, oy = (dt(1.0) / dt(wo)).astype(dt), (dt(1.0) / dt(ho)).astype(dt)
    X = {s: _axis((u + dt(s) * ox).astype(dt), wi, dt) for s in (-1, 0, 1)}
    Y = {s: _axis((v + dt(s) * oy).astype(dt), hi, dt) for s in (-1, 0, 1)}
    r = _tap(T, X[1], Y[0], dt)
    for sx, sy in ((-1, 0), (0, 1), (0, -1)):
        r = (r + _tap(T, X[sx], Y[sy], dt)).astype(dt)
    r = (r * dt(2.0)).astype(dt)
    for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        r = (r + _tap(T, X[sx], Y[sy], dt)).astype(dt)
    return (r / dt(12.0)).astype(dt)


def bloom(color, iterations=4, strength=0.01, threshold=0.0, dtype=f32):
    dt = dtype
    c = np.ascontiguousarray(color, f32)
    H, W = c.shape[:2]
    sizes = level_sizes(W, H, iterations)
    with np.errstate(all="ignore"):
        nonfinite = ~np.isfinite(c[..., :3]).all(axis=-1)
        negative = ~nonfinite & (c[..., :3] < 0).any(axis=-1)
        clamped = (c[..., :3] > f32(HALF_MAX)).any(axis=-1)
    B, below = prefilter(c, threshold, dt)
    info = dict(sizes=sizes, down=[], levels=[], glow=np.zeros((H, W, 3), dt), nonfinite=nonfinite, negative=negative, clamped=clamped, below=below)
    s = dt(f32(strength))
    if not sizes or s == 0:
        return c.copy() if dt is f32 else c.astype(dt), info
    M = []
    src = B
    for (w, h) in sizes:
        src = down(src, w, h, dt)
        M.append(src)
    info["down"] = list(M)
    for i in range(len(sizes) - 1, 0, -1):                      # M_i = up(M_{i+1}): replaces, as upstream with output_scale = 0
        M[i - 1] = up(M[i], sizes[i - 1][0], sizes[i - 1][1], dt)
    U = up(M[0], W, H, dt)
    info["levels"], info["glow"] = M, U
    out = c.astype(dt)
    with np.errstate(all="ignore"):
        rgb = (c[..., :3].astype(dt) + (s * U).astype(dt)).astype(dt)
    out[..., :3] = np.where(nonfinite[..., None], out[..., :3], rgb)
    return out, info


# ---- the field the tests run on ---------------------------------------------------------------------------------------------------------
def random_field(rng, w, h):
    """-> color (h, w, 4): uniform in [0, 1) with a tenth of the pixels up to fifty times as bright (an emissive surface), then, each on
    max(4, w * h / 50) pixels drawn afresh: a NaN or an infinity of either sign in one of the four channels, a negative component, a
    component above 65504."""
    color = rng.random((h, w, 4)).astype(f32)
    bright = rng.random((h, w)) < 0.1
    color[bright] *= rng.uniform(2.0, 50.0, (int(bright.sum()), 1)).astype(f32)
    n = max(4, w * h // 50)
    specials = np.array([np.nan, np.inf, -np.inf], f32)
    for _ in range(n):
        color[rng.integers(h), rng.integers(w), rng.integers(4)] = rng.choice(specials)
    for _ in range(n):
        color[rng.integers(h), rng.integers(w), rng.integers(3)] = f32(-rng.uniform(0.1, 3.0))
    for _ in range(n):
        color[rng.integers(h), rng.integers(w), rng.integers(3)] = f32(rng.uniform(7.0e4, 1.0e6))
    return color
