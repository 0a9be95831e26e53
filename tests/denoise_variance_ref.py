"""numpy restatement of pt_denoise_variance (include/mipt.h): the a-trous filter steered by the variance AOV, operation by operation in the
order the header states, in the dtype asked for -- float32 is what the kernels compute, float64 of the same float32 inputs is the yardstick
tests/test_gpu_denoise_variance.py measures them against.  Prepare, the tap order, h, wn and ez are pt_denoise's and come from
tests/denoise_ref.py.  Also the synthetic scene of the two test files: denoise_ref.scene's geometry, with a colour that is the mean of real
per-sample draws and a variance target from those same draws."""
import numpy as np

from tests import denoise_ref as dr
from tests.denoise_ref import H5, f32, prepare, rel_error, shifted

TILE = 16
K3 = (1.0 / 4, 1.0 / 2, 1.0 / 4)                            # exact in binary, and so is every product of two of them


class Config:
    """pt_denoise_variance_config with its defaults."""

    def __init__(self, iterations=5, demodulate=1, normal_power_log2=7, sigma_depth=0.02, sigma_variance=4.0):
        self.iterations, self.demodulate, self.normal_power_log2 = int(iterations), int(demodulate), int(normal_power_log2)
        self.sigma_depth, self.sigma_variance = float(f32(sigma_depth)), float(f32(sigma_variance))     # the config holds float32


def pixel_counts(tile_samples, w, h):
    """The (h, w) count map of a (tiles_y, tiles_x) array of 16 x 16 tiles' counts, or of one count for every tile."""
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    ts = np.broadcast_to(np.asarray(tile_samples, np.int64).reshape((ty, tx) if np.ndim(tile_samples) else ()), (ty, tx))
    return np.repeat(np.repeat(ts, TILE, axis=0), TILE, axis=1)[:h, :w]


def prepare_variance(color, albedo, normal_depth, variance, counts, cfg, dtype):
    """(S, a', n, z, v, valid): pt_denoise's prepare, the variance v of the demodulated signal's mean, and the valid mask."""
    T = dtype
    S, a, n, z, valid = prepare(color, albedo, normal_depth, cfg, T)
    V = np.asarray(variance, f32).astype(T)
    N = np.asarray(counts, np.int64)
    with np.errstate(all="ignore"):
        k = (N - 1).astype(T)[..., None]                     # (float)(N - 1); a count below 2 is invalid whatever this gives
        u = (V[..., :3] / k) / (a * a)
        v = (u[..., 0] + u[..., 1]) + u[..., 2]
        valid = valid & (N >= 2) & np.isfinite(v) & (v >= 0)
    return S, a, n, z, v, valid


def prefilter(v, valid, dtype):
    """vt: the 3 x 3 binomial mean of v over the valid taps at unit spacing, dy outer, dx inner, sequential sums."""
    T = dtype
    sg = np.zeros(v.shape, T)
    sv = np.zeros(v.shape, T)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                ok = shifted(valid, dy, dx, False) & valid
                g = T(K3[dy + 1] * K3[dx + 1])
                sg = sg + np.where(ok, g, T(0))
                sv = sv + np.where(ok, g * shifted(v, dy, dx, 0), T(0))
        vt = sv / sg
    return np.where(valid, vt, T(0))


def one_pass(S, v, n, z, valid, i, cfg, dtype):
    """Pass i on (S, v): the prefilter, then the 25 taps at spacing 2^i.  Returns (S', v'); invalid pixels keep their (unused) values."""
    T = dtype
    s = 1 << i
    vt = prefilter(v, valid, T)
    sv2 = T(cfg.sigma_variance) * T(cfg.sigma_variance)
    zden = (T(cfg.sigma_depth) * T(s)) * z + T(1e-6)
    sw = np.zeros(z.shape, T)
    sc = np.zeros(S.shape, T)
    sv = np.zeros(z.shape, T)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                ok = shifted(valid, oy, ox, False) & valid
                Sq, nq, zq = shifted(S, oy, ox, 0), shifted(n, oy, ox, 0), shifted(z, oy, ox, 0)
                vq, vtq = shifted(v, oy, ox, 0), shifted(vt, oy, ox, 0)
                wn = np.clip((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2], T(0), T(1))
                for _ in range(cfg.normal_power_log2):
                    wn = wn * wn
                ez = np.abs(z - zq) / zden
                if cfg.sigma_variance != 0:
                    d = S - Sq
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    ec = d2 / (sv2 * (vt + vtq) + T(1e-8))
                else:
                    ec = np.zeros_like(ez)
                w = (T(H5[dy + 2] * H5[dx + 2]) * wn) * np.exp(-(ez + ec))
                sw = sw + np.where(ok, w, T(0))                                  # a select, not a product: a NaN never leaks
                sc = sc + np.where(ok[..., None], w[..., None] * Sq, T(0))
                sv = sv + np.where(ok, (w * w) * vq, T(0))
        S1 = sc / sw[..., None]
        v1 = sv / (sw * sw)
    return np.where(valid[..., None], S1, S), np.where(valid, v1, v)


def denoise_variance(color, albedo, normal_depth, variance, counts, cfg=None, dtype=f32, return_variance=False):
    """The whole call; counts: the (H, W) count map (pixel_counts).  Returns (out, valid) like denoise_ref.denoise: out is float32 (H, W, 4)
    for dtype float32 -- invalid pixels and every alpha are the input's bits -- and float64 for dtype float64, where only the valid pixels'
    rgb mean anything beyond a copy of the input.  return_variance: (out, valid, v) with the propagated variance of the last pass."""
    cfg = cfg or Config()
    color = np.asarray(color, f32)
    S, a, n, z, v, valid = prepare_variance(color, albedo, normal_depth, variance, counts, cfg, dtype)
    out = color.astype(dtype).copy()
    if cfg.iterations > 0:
        for i in range(cfg.iterations):
            S, v = one_pass(S, v, n, z, valid, i, cfg, dtype)
        with np.errstate(all="ignore"):
            rgb = S * a
        out[..., :3] = np.where(valid[..., None], rgb, out[..., :3])
    return (out, valid, v) if return_variance else (out, valid)


# ---- the synthetic scene -----------------------------------------------------------------------------------------------------------
def scene(w=72, h=40, counts=8, seed=3, specials=True):
    """denoise_ref.scene's geometry (two planes, depth ramps, the albedo checker, the background wedge behind a half-covered diagonal, the
    shadow column no guide shows), rendered from real draws: pixel p holds the mean of counts[p] samples, each gamma(0.5, 2) * light * albedo
    (mean 1, variance 2: denoise_ref's noise, sample by sample) composited over ENV by the coverage, and the variance target holds the
    population variance of those same samples per channel and of their channel sum, from a float64 two-pass fold cast to float32.  counts:
    one count or an (h, w) map; every pixel uses the first counts[p] of one stream of draws, so a map changes no draw.  specials: one NaN
    pixel, one +inf pixel and a block of cov == 0 (an unrendered shard tile).  denoise_ref's black drop-out is left out on purpose: a pixel
    whose samples are all black has variance 0, and a filter steered by the variance rightly believes it.  Returns a dict of float32 images
    color, albedo, normal_depth, variance, clean, the int64 map counts, and the masks rendered and band."""
    base = dr.scene(w, h, spp=0, seed=seed, specials=False)              # spp = 0: the geometry and the clean image, no draw taken
    rng = np.random.default_rng(seed)
    N = np.broadcast_to(np.asarray(counts, np.int64), (h, w)).copy()
    nmax = int(max(N.max(), 1))
    g = rng.gamma(0.5, 2.0, size=(nmax, h, w))
    use = np.arange(nmax)[:, None, None] < N[None]
    A = base["albedo"].astype(np.float64)
    cov = A[..., 3]
    y, x = np.mgrid[0:h, 0:w]
    light = np.where((x >= dr.SHADOW[0]) & (x < dr.SHADOW[1]), 0.3, 1.0)
    color = np.ones((h, w, 4))
    variance = np.zeros((h, w, 4))
    den = np.maximum(N, 1)
    total = np.zeros((nmax, h, w))
    for c in range(3):
        xs = (A[..., c] * light)[None] * g + ((1.0 - cov) * dr.ENV[c])[None]          # albedo holds cov * alb
        mean = np.where(use, xs, 0.0).sum(axis=0) / den
        color[..., c] = mean
        variance[..., c] = np.where(use, (xs - mean[None]) ** 2, 0.0).sum(axis=0) / den
        total += xs
    tmean = np.where(use, total, 0.0).sum(axis=0) / den
    variance[..., 3] = np.where(use, (total - tmean[None]) ** 2, 0.0).sum(axis=0) / den
    sc = dict(color=color, albedo=base["albedo"].copy(), normal_depth=base["normal_depth"].copy(), variance=variance, clean=base["clean"].copy())
    rendered = (cov > 0) & (N >= 2)
    if specials and w >= 48 and h >= 36:
        sc["color"][5, 7, 1] = np.nan
        sc["color"][9, 50, 0] = np.inf
        for img in sc.values():
            img[28:35, 3:11] = 0.0                   # a tile this rank did not render
        rendered = rendered & np.all(np.isfinite(sc["color"]), axis=-1)
        rendered[28:35, 3:11] = False
    band = ((np.abs(x - dr.SHADOW[0] + 0.5) <= 6) | (np.abs(x - dr.SHADOW[1] + 0.5) <= 6)) & rendered
    sc = {k: np.ascontiguousarray(v, f32) for k, v in sc.items()}
    sc.update(counts=N, rendered=rendered, band=band)
    return sc
