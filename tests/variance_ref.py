"""The variance AOV and the noise report (include/mipt.h pt_set_variance / pt_noise_estimate) restated in numpy float32, operation by
operation from the header: every product and sum below is one float32 operation on float32 arrays, in the header's order."""
import numpy as np

f32 = np.float32
TILE = 16


def fold_step(m, V, x, n):
    """One sample x (..., 3) into a pixel with n samples: m (..., 3) is the output's rgb before it, V (..., 4) the target.  Returns (m', V')."""
    x = np.ascontiguousarray(x, f32)
    if n == 0:
        return x.copy(), np.zeros(x.shape[:-1] + (4,), f32)
    with np.errstate(all="ignore"):
        b = f32(1.0) / (f32(n) + f32(1.0))
        d0 = x - m
        m1 = m + b * d0
        d1 = x - m1
        q = d0 * d1
        q = np.where(np.isfinite(q), q, f32(0.0)).astype(f32)
        rgb = V[..., :3] + b * (q - V[..., :3])
        s0 = (d0[..., 0] + d0[..., 1]) + d0[..., 2]
        s1 = (d1[..., 0] + d1[..., 1]) + d1[..., 2]
        qs = s0 * s1
        qs = np.where(np.isfinite(qs), qs, f32(0.0)).astype(f32)
        w = V[..., 3] + b * (qs - V[..., 3])
    out = np.concatenate([rgb, w[..., None]], axis=-1).astype(f32)
    return m1.astype(f32), out


def fold(samples, first=0, m=None, V=None):
    """The targets after each of `samples` (a list of (..., 3) or (..., 4) arrays, rgb taken) folded into a pixel that holds `first` samples
    with mean m and target V (None for first == 0).  Returns (means, targets), one entry per sample."""
    means, targets = [], []
    for k, x in enumerate(samples):
        x = np.ascontiguousarray(x, f32)[..., :3]
        m, V = fold_step(m, V, x, first + k)
        means.append(m)
        targets.append(V)
    return means, targets


def tile_grid(w, h):
    return (h + TILE - 1) // TILE, (w + TILE - 1) // TILE


def pixel_error(image, variance, n):
    """e per pixel for the count n (a scalar or an array broadcast over the pixels), n >= 2."""
    image, variance = np.ascontiguousarray(image, f32), np.ascontiguousarray(variance, f32)
    with np.errstate(all="ignore"):
        s = (image[..., 0] + image[..., 1]) + image[..., 2]
        den = f32(1e-4) + np.sqrt(np.fmax(s, f32(0.0)))              # fmaxf: a NaN s counts as 0
        e = np.sqrt(variance[..., 3] / (np.asarray(n) - 1).astype(f32)) / den
    e = np.where(np.isnan(e), f32(np.inf), e).astype(f32)
    return e


def noise_tiles(image, variance, tile_samples):
    """(tile_mean as float64 -- the exact sum of the float32 errors over the count --, tile_max float32, in-image pixel counts), -1 where
    a tile's count is below 2.  tile_samples: (tiles_y, tiles_x)."""
    h, w = image.shape[:2]
    ty, tx = tile_grid(w, h)
    ts = np.asarray(tile_samples, np.uint32).reshape(ty, tx)
    mean, mx, px = np.full((ty, tx), -1.0, np.float64), np.full((ty, tx), -1.0, f32), np.zeros((ty, tx), np.int64)
    for y in range(ty):
        for x in range(tx):
            sl = (slice(y * TILE, min((y + 1) * TILE, h)), slice(x * TILE, min((x + 1) * TILE, w)))
            px[y, x] = image[sl].shape[0] * image[sl].shape[1]
            n = int(ts[y, x])
            if n < 2:
                continue
            e = pixel_error(image[sl], variance[sl], n)
            mx[y, x] = e.max()
            with np.errstate(all="ignore"):
                mean[y, x] = e.astype(np.float64).sum() / px[y, x]
    return mean, mx, px


def summary(tile_mean, tile_max, px, tile_samples, threshold):
    """The host formula over the returned float32 tile arrays: (tiles, tiles_estimated, tiles_above, mean, max)."""
    ts = np.asarray(tile_samples).reshape(tile_mean.shape)
    est = ts >= 2
    if not est.any():
        return ts.size, 0, 0, f32(-1.0), f32(-1.0)
    weighted, pixels, top = 0.0, 0.0, -1.0                             # Python floats are doubles; tile order, as the library sums
    for t in np.ndindex(ts.shape):
        if est[t]:
            weighted += float(tile_mean[t]) * float(px[t])
            pixels += float(px[t])
            top = max(top, float(tile_max[t]))
    return ts.size, int(est.sum()), int((tile_max[est] > f32(threshold)).sum()), f32(weighted / pixels), f32(top)
