"""numpy float32 restatement of tile-level adaptive sampling (include/mipt.h pt_set_adaptive), used by tests/test_gpu_adaptive.py and
checked on its own by tests/test_adaptive_host.py.

  blend          pt_vertex.h blend_sample: h + (1 / (n + 1)) * (L - h), alpha towards 1 (the division is IEEE on these operands)
  fold           the uniform accumulation I_n and the half buffer A_n (mean of the samples with an even index) after n raw samples
  pixel_error    e = ((|I.r-A.r| + |I.g-A.g|) + |I.b-A.b|) / (1e-4 + sqrt(max((I.r + I.g) + I.b, 0))), NaN -> +inf
  tile_errors    E = max of e over a 16x16 tile's in-image pixels
  predict        which call boundary retires each tile, given E_t(n)
"""
import numpy as np

f32 = np.float32
TILE = 16


def blend(h, n, L):
    b = f32(1.0) / f32(n + 1)
    out = np.empty_like(h)
    out[..., :3] = h[..., :3] + b * (L - h[..., :3])
    out[..., 3] = h[..., 3] + b * (f32(1.0) - h[..., 3])
    return out


def fold(raw):
    """raw[k] = the (H, W, 4) output of frame k traced without accumulation, i.e. (L, 1).  Returns I, A with I[n - 1], A[n - 1] the
    accumulated image and the half buffer after n samples."""
    I, A = [], []
    cur = half = None
    for n, s in enumerate(raw):
        s = np.asarray(s, f32)
        L = s[..., :3]
        cur = s.copy() if n == 0 else blend(cur, n, L)
        if n % 2 == 0:
            half = s.copy() if n == 0 else blend(half, n // 2, L)
        I.append(cur.copy())
        A.append(half.copy())
    return I, A


def pixel_error(I, A, dtype=f32):
    I = np.asarray(I, dtype)
    A = np.asarray(A, dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = (np.abs(I[..., 0] - A[..., 0]) + np.abs(I[..., 1] - A[..., 1])) + np.abs(I[..., 2] - A[..., 2])
        s = (I[..., 0] + I[..., 1]) + I[..., 2]
        e = d / (dtype(1e-4) + np.sqrt(np.fmax(s, dtype(0))))
    return np.where(np.isnan(e), dtype(np.inf), e).astype(dtype)


def tile_errors(I, A, dtype=f32):
    """(tiles_y, tiles_x) max of pixel_error over each tile's in-image pixels."""
    e = pixel_error(I, A, dtype)
    H, W = e.shape
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    pad = np.full((ty * TILE, tx * TILE), -np.inf, dtype)
    pad[:H, :W] = e
    return pad.reshape(ty, TILE, tx, TILE).max(axis=(1, 3))


def tile_pixels(W, H):
    """(tiles_y, tiles_x) count of in-image pixels per tile."""
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    m = np.zeros((ty * TILE, tx * TILE), np.int64)
    m[:H, :W] = 1
    return m.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3))


def predict(E_of_n, spp, min_samples, cap, threshold, shape):
    """E_of_n(n) -> (tiles_y, tiles_x) tile errors after n samples.  Replays the host loop (calls of `spp` samples, clamped to the cap,
    until no tile is active): returns the count and last error of each tile, and the boundaries called."""
    samples = np.zeros(shape, np.int64)
    err = np.zeros(shape, f32)
    active = np.ones(shape, bool)
    acc, calls = 0, []
    while acc < cap and active.any():
        n = acc + min(spp, cap - acc)
        E = E_of_n(n)
        samples[active] = n
        err[active] = E[active]
        retire = active & ((n >= cap) | ((n >= min_samples) & (E <= f32(threshold))))
        active &= ~retire
        calls.append(n)
        acc = n
    return samples, err, calls


def tile_view(img, t_y, t_x):
    return img[t_y * TILE:(t_y + 1) * TILE, t_x * TILE:(t_x + 1) * TILE]
