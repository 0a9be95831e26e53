"""numpy restatement of pt_denoise (include/mipt.h): the edge-avoiding a-trous filter over the first-hit AOVs, operation by operation in the
order the header states, in the dtype asked for -- float32 is what the kernels compute, float64 of the same float32 inputs is the yardstick
tests/test_gpu_denoise.py measures them against.  Also the synthetic scene of tests/test_denoise_host.py and tests/test_gpu_denoise.py."""
import numpy as np

f32 = np.float32
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)        # exact in binary, and so is every product of two of them


class Config:
    """pt_denoise_config with its defaults."""

    def __init__(self, iterations=5, demodulate=1, normal_power_log2=7, sigma_depth=0.02, sigma_color=1.0):
        self.iterations, self.demodulate, self.normal_power_log2 = int(iterations), int(demodulate), int(normal_power_log2)
        self.sigma_depth, self.sigma_color = float(f32(sigma_depth)), float(f32(sigma_color))     # the config holds float32


def luminance(S):
    return (S[..., 0] + S[..., 1]) + S[..., 2]


def prepare(color, albedo, normal_depth, cfg, dtype):
    """(S, a', n, z, valid): the demodulated signal, the albedo it was divided by, the unit normal, the depth, and the valid mask."""
    T = dtype
    C, A, N = (np.asarray(x, f32).astype(T) for x in (color, albedo, normal_depth))
    cov = A[..., 3]
    with np.errstate(all="ignore"):
        if cfg.demodulate:
            a = np.maximum(A[..., :3] + (T(1) - cov)[..., None], T(1e-3))
        else:
            a = np.ones_like(A[..., :3])
        S = C[..., :3] / a
        length = np.sqrt((N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2])
        n = N[..., :3] / length[..., None]
        z = N[..., 3] / cov
        valid = (cov > 0) & (length > 0) & np.isfinite(z) & (z > 0) & np.all(np.isfinite(S), axis=-1) & np.all(np.isfinite(n), axis=-1)
    return S, a, n, z, valid


def shifted(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox], `fill` outside the image."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return b


def one_pass(S, n, z, valid, i, cfg, dtype):
    """Pass i: taps at spacing 2^i, dy outer, dx inner, sequential sums.  Invalid pixels keep their (unused) S."""
    T = dtype
    s = 1 << i
    L = luminance(S)
    sig = T(cfg.sigma_color) * T(2.0 ** -i)
    sig2 = sig * sig
    zden = (T(cfg.sigma_depth) * T(s)) * z + T(1e-6)
    sw = np.zeros(z.shape, T)
    ss = np.zeros(S.shape, T)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                ok = shifted(valid, oy, ox, False) & valid
                Sq, nq, zq, Lq = shifted(S, oy, ox, 0), shifted(n, oy, ox, 0), shifted(z, oy, ox, 0), shifted(L, oy, ox, 0)
                wn = np.clip((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2], T(0), T(1))
                for _ in range(cfg.normal_power_log2):
                    wn = wn * wn
                ez = np.abs(z - zq) / zden
                if cfg.sigma_color != 0:
                    d = S - Sq
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    ls = L + Lq
                    ec = d2 / (sig2 * (ls * ls) + T(1e-8))
                else:
                    ec = np.zeros_like(ez)
                w = (T(H5[dy + 2] * H5[dx + 2]) * wn) * np.exp(-(ez + ec))
                sw = sw + np.where(ok, w, T(0))                                  # a select, not a product: a NaN never leaks
                ss = ss + np.where(ok[..., None], w[..., None] * Sq, T(0))
        out = ss / sw[..., None]
    return np.where(valid[..., None], out, S)


def denoise(color, albedo, normal_depth, cfg=None, dtype=f32):
    """The whole call.  Returns (out, valid): out is float32 (H, W, 4) for dtype float32 -- invalid pixels and every alpha are the input's
    bits -- and float64 for dtype float64, where only the valid pixels' rgb mean anything beyond a copy of the input."""
    cfg = cfg or Config()
    color = np.asarray(color, f32)
    S, a, n, z, valid = prepare(color, albedo, normal_depth, cfg, dtype)
    out = color.astype(dtype).copy()
    if cfg.iterations == 0:
        return out, valid
    for i in range(cfg.iterations):
        S = one_pass(S, n, z, valid, i, cfg, dtype)
    with np.errstate(all="ignore"):
        rgb = S * a
    out[..., :3] = np.where(valid[..., None], rgb, out[..., :3])
    return out, valid


def rel_error(got, ref64, valid):
    """max over valid pixels and channels of |got - ref64| / (|ref64| + 1e-3), in float64."""
    if not valid.any():
        return 0.0
    g, r = np.asarray(got, np.float64)[..., :3][valid], np.asarray(ref64, np.float64)[..., :3][valid]
    return float(np.max(np.abs(g - r) / (np.abs(r) + 1e-3)))


# ---- the synthetic scene -----------------------------------------------------------------------------------------------------------
SHADOW = (20, 26)                 # columns [20, 26) receive 0.3 of the light; no guide shows it
ENV = (0.25, 0.5, 0.75)


def scene(w=72, h=40, spp=8, seed=3, specials=True):
    """Two planes with normals (-+0.6, 0, 0.8) meeting at the middle column, depth ramps, a 6-pixel albedo checker, a background wedge in
    the lower right corner behind a half-coverage diagonal, a shadow column, and gamma-distributed noise of the mean of `spp` samples
    (each sample's shape is 1/2: relative variance 2).  specials: one NaN pixel, one +inf pixel, one black drop-out and a block of
    cov == 0 (an unrendered shard tile).  Returns a dict of float32 images color, albedo, normal_depth, clean, and the masks
    rendered (cov > 0 and finite) and band (the 6 pixels either side of the shadow column's two edges)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    left = x < w // 2
    nrm = np.where(left[..., None], np.array([-0.6, 0.0, 0.8]), np.array([0.6, 0.0, 0.8]))
    depth = np.where(left, 2.0 + 0.03 * x + 0.01 * y, 2.0 + 0.03 * (w // 2) - 0.02 * (x - w // 2) + 0.01 * y)
    alb = np.where((((x // 6) + (y // 6)) % 2 == 0)[..., None], np.array([0.8, 0.7, 0.6]), np.array([0.2, 0.3, 0.4]))
    light = np.where((x >= SHADOW[0]) & (x < SHADOW[1]), 0.3, 1.0)
    t = (x - w) + (y - h) + min(17, (w + h) // 4)    # > 0: background; == 0: the diagonal, half covered
    cov = np.where(t > 0, 0.0, np.where(t == 0, 0.5, 1.0))
    noise = rng.gamma(0.5 * spp, 1.0 / (0.5 * spp), size=(h, w)) if spp else np.ones((h, w))

    def compose(irradiance):
        surf = alb * irradiance[..., None]
        return cov[..., None] * surf + (1.0 - cov)[..., None] * np.array(ENV)

    clean = np.concatenate([compose(light), np.ones((h, w, 1))], axis=-1)
    color = np.concatenate([compose(light * noise), np.ones((h, w, 1))], axis=-1)
    albedo = np.concatenate([cov[..., None] * alb, cov[..., None]], axis=-1)
    nd = np.concatenate([cov[..., None] * nrm, (cov * depth)[..., None]], axis=-1)
    rendered = cov > 0
    if specials and w >= 48 and h >= 36:
        color[5, 7, 1] = np.nan
        color[9, 50, 0] = np.inf
        color[12, 40, :3] = 0.0                      # a black drop-out: the guides say surface, the sample says nothing
        for img in (color, albedo, nd, clean):
            img[28:35, 3:11] = 0.0                   # a tile this rank did not render
        rendered = rendered & np.all(np.isfinite(color), axis=-1)
        rendered[28:35, 3:11] = False
    band = ((np.abs(x - SHADOW[0] + 0.5) <= 6) | (np.abs(x - SHADOW[1] + 0.5) <= 6)) & rendered
    return dict(color=color.astype(f32), albedo=albedo.astype(f32), normal_depth=nd.astype(f32), clean=clean.astype(f32),
                rendered=rendered, band=band)


def half_planes(w=24, h=12, right_scale=1.0, seed=11):
    """Left half: normal (1, 0, 0); right half: normal (0, 0, 1); same depth.  The colours of the right half are scaled by right_scale:
    the normal weight across the middle is exactly zero, so the left half of the result does not depend on it in any bit."""
    rng = np.random.default_rng(seed)
    color = np.concatenate([rng.random((h, w, 3)) + 0.1, np.ones((h, w, 1))], axis=-1)
    color[:, w // 2:, :3] *= right_scale
    albedo = np.concatenate([rng.random((h, w, 3)) * 0.8 + 0.1, np.ones((h, w, 1))], axis=-1)
    nd = np.zeros((h, w, 4))
    nd[:, :w // 2, 0] = 1.0
    nd[:, w // 2:, 2] = 1.0
    nd[..., 3] = 3.0
    return color.astype(f32), albedo.astype(f32), nd.astype(f32)


def rmse(a, b, mask):
    d = np.asarray(a, np.float64)[..., :3][mask] - np.asarray(b, np.float64)[..., :3][mask]
    return float(np.sqrt(np.mean(d * d)))
