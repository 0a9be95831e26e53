"""pt_env_filter (include/mipt.h) restated in numpy from the header's text and the reference's FilterEnvironmentCubeMap.cs.hlsl, in two forms:

  dtype = float32: rounding for rounding -- every product, sum, quotient and root below is one operation of float32 in the header's order;
      sin and cos go through float64 and are rounded once, log2 is the header's defined log2 (log2_defined), as on the device;
  dtype = float64: the same text in float64 with numpy's sin, cos and log2, starting from the SAME float32 sample points u (the rounding of
      (float)i * c is part of the definition, not error), the same float32 roughness and bias, and the same RGBA16F texels.

Both take an explicit list of texels, so a large level can be checked on a subset.  Shares no code with csrc/.  The cube's mip chain is
restated too (chain_from_mip0: GenerateMipLevelArray.cs.hlsl as k_cube_mip computes it), so a test needs only the cube's mip 0.
"""
import numpy as np

f16, f32, f64 = np.float16, np.float32, np.float64
DEFAULTS = dict(ggx_samples=256, ggx_mip_bias=2.0, ggx_mips=0, diffuse_samples=512, diffuse_mip_bias=3.0, diffuse_resolution=256)
GGX, DIFFUSE = 0, 1

# CubemapToDirection's faces (Transforms.hlsli:10-50): forward, u axis, v axis
_FD = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f64)
_UD = np.array([(0, 0, -1), (0, 0, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (-1, 0, 0)], f64)
_VD = np.array([(0, -1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0), (0, -1, 0)], f64)


def _quiet():
    return np.errstate(all="ignore")


# ---- the cube chain ---------------------------------------------------------------------------------------------------------------------
def half_rgb(texels_u16):
    """(..., 4) uint16 RGBA16F -> (..., 3) float32."""
    return np.ascontiguousarray(texels_u16, np.uint16).view(f16)[..., :3].astype(f32)


def chain_from_mip0(mip0_u16):
    """The cube's mips as (6, n, n, 3) float32 arrays of half values, n = N, N >> 1 .. 1: each the float32 sum of the four texels below it
    in the order (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1), times 0.25, rounded to half."""
    chain = [half_rgb(mip0_u16)]
    while chain[-1].shape[1] > 1:
        p = chain[-1]
        n = p.shape[1] >> 1
        q = p[:, :2 * n, :2 * n]
        with _quiet():
            r = ((q[:, 0::2, 0::2] + q[:, 0::2, 1::2]) + q[:, 1::2, 0::2]) + q[:, 1::2, 1::2]
            chain.append((r * f32(0.25)).astype(f16).astype(f32))
    return chain


def ggx_level_sizes(N, mips):
    out, n = [], N
    for _ in range(mips):
        out.append(n)
        n //= 2
    return out


def reference_ggx_mips(N):
    """EnvironmentMap.cpp:106-107."""
    return max(int(np.floor(np.log2(f32(N)))) + 1 - 4, 1)


def mip_to_roughness(i, mips):
    """MipToRoughness (EnvironmentMap.cpp:17-22) in float32; a chain of one level has roughness 0 where upstream divides 0 by 0 (quirk q30)."""
    if mips == 1:
        return f32(0.0)
    r = f32(i) / (f32(mips) - f32(1.0))
    return f32(r * r)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    with _quiet():
        return v / np.sqrt(_dot(v, v))[..., None]


def cubemap_to_direction(face, u, v, dt):
    one, two = dt(1), dt(2)
    u2, v2 = u * two - one, v * two - one
    fd, ud, vd = _FD.astype(dt)[face], _UD.astype(dt)[face], _VD.astype(dt)[face]
    return _normalize(fd + u2[..., None] * ud + v2[..., None] * vd)


def dir_to_face(d, dt):
    """D3D's major-axis table: (face, u, v)."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    fx = (ax >= ay) & (ax >= az)
    fy = ~fx & (ay >= az)
    face = np.where(fx, np.where(x >= 0, 0, 1), np.where(fy, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
    ma = np.where(fx, ax, np.where(fy, ay, az))
    sc = np.choose(face, [-z, z, x, x, x, -x])
    tc = np.choose(face, [-y, -y, z, -z, -y, -y])
    half, one = dt(0.5), dt(1)
    with _quiet():
        return face, half * (sc / ma + one), half * (tc / ma + one)


def _tap(mip, n, face, i, j, dt):
    """One bilinear tap with seamless edges: a tap outside the face is re-projected through its direction onto the neighbouring face and
    fetched point-wise there.  Which texel that is, is a map from integers (face, i, j, n) to integers: an addressing rule, not arithmetic
    on the signal, and it is DEFINED by its float32 evaluation in both forms -- a corner tap's direction has two components of equal
    size, and which face wins that tie hangs on the last bit of (i + 0.5) / n * 2 - 1."""
    outside = ~((i >= 0) & (i < n) & (j >= 0) & (j < n))
    if outside.any():
        fo, io, jo = face[outside], i[outside], j[outside]
        d = cubemap_to_direction(fo, (io.astype(f32) + f32(0.5)) / f32(n), (jo.astype(f32) + f32(0.5)) / f32(n), f32)
        f2, u, v = dir_to_face(d, f32)
        i2 = np.clip(np.floor(u * f32(n)).astype(np.int64), 0, n - 1)
        j2 = np.clip(np.floor(v * f32(n)).astype(np.int64), 0, n - 1)
        face, i, j = face.copy(), i.copy(), j.copy()
        face[outside], i[outside], j[outside] = f2, i2, j2
    return mip[face, j, i].astype(dt)


def sample_mip(mip, d, dt):
    """TextureCube.SampleLevel(linear, d, 0) of one mip (6, n, n, 3): (rgb, the largest |tap component| fetched).  A direction without a face
    (a NaN coordinate) gives 0."""
    n = mip.shape[1]
    face, u, v = dir_to_face(d, dt)
    bad = np.isnan(u) | np.isnan(v)
    u, v = np.where(bad, dt(0.5), u), np.where(bad, dt(0.5), v)
    x, y = u * dt(n) - dt(0.5), v * dt(n) - dt(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    one = dt(1)
    w00, w10, w01, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    t00, t10 = _tap(mip, n, face, i0, j0, dt), _tap(mip, n, face, i0 + 1, j0, dt)
    t01, t11 = _tap(mip, n, face, i0, j0 + 1, dt), _tap(mip, n, face, i0 + 1, j0 + 1, dt)
    with _quiet():
        c = ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11
        big = np.maximum(np.maximum(np.abs(t00), np.abs(t10)), np.maximum(np.abs(t01), np.abs(t11))).max(axis=-1)
    c[bad] = 0
    big = np.where(bad, 0, big)
    return c, big


def sample_level(chain, d, level, dt):
    """The trilinear lookup (the oracle's SampleCubeLevel) at an already clamped level, element by element: (rgb, largest |tap|)."""
    M = len(chain)
    flat_d, flat_l = d.reshape(-1, 3), level.reshape(-1)
    l0 = np.floor(flat_l).astype(np.int64)
    f = flat_l - l0.astype(dt)
    out = np.zeros(flat_d.shape, dt)
    big = np.zeros(flat_l.shape, dt)
    for m in np.unique(l0):
        at = np.nonzero(l0 == m)[0]
        a, ba = sample_mip(chain[m], flat_d[at], dt)
        out[at], big[at] = a, ba
        both = (f[at] != 0) & (m + 1 < M)
        two = at[both]
        if two.size:
            b, bb = sample_mip(chain[m + 1], flat_d[two], dt)
            ff = f[two][:, None]
            with _quiet():
                out[two] = a[both] * (dt(1) - ff) + b * ff
            big[two] = np.maximum(big[two], bb)
    return out.reshape(d.shape), big.reshape(level.shape)


# ---- the samples ------------------------------------------------------------------------------------------------------------------------
def r2(samples):
    """R2(0.5, i) (Random.hlsli:80-85) in float32, i = 0 .. samples - 1: (u.x, u.y)."""
    g = f32(1.324717957244746)
    gg = f32(g * g)
    c0, c1 = f32(1.0) / g, f32(1.0) / gg
    i = np.arange(samples).astype(f32)
    s0, s1 = f32(0.5) + i * c0, f32(0.5) + i * c1
    return (s0 - np.floor(s0)).astype(f32), (s1 - np.floor(s1)).astype(f32)


_H = float.fromhex


def log2_defined(x):
    """The device's defined log2 (csrc/pt_math.h co_log2), float32 operation by operation."""
    x = np.asarray(x, f32)
    with _quiet():
        m, e = np.frexp(x)
        m = m.astype(f32)
        small = m < f32(0.707106769)
        m = np.where(small, m * f32(2), m)
        e = e - small
        t = (m - f32(1)) / (m + f32(1))
        s = t * t
        q = np.full(x.shape, f32(_H("0x1.ba1838p-2")), f32)
        q = q * s + f32(_H("0x1.274720p-1"))
        q = q * s + f32(_H("0x1.ec70e6p-1"))
        q = q * s + f32(_H("0x1.715476p+1"))
        r = e.astype(f32) + t * q
    r = np.where(x == np.inf, f32(np.inf), r)
    r = np.where(x > 0, r, np.where(x == 0, f32(-np.inf), f32(np.nan)))
    return r.astype(f32)


def _sincos(angle, dt):
    a = angle.astype(f64)
    return np.cos(a).astype(dt), np.sin(a).astype(dt)


def mip_level(pdf, samples, N, M, bias, dt):
    """The clamped level of samples of density pdf: D3D's clamp, NaN -> 0, +inf -> M - 1."""
    PI = dt(f32(3.14159265359))
    with _quiet():
        omega_s = dt(1) / (dt(samples) * pdf)
        omega_p = (dt(4) * PI) / ((dt(6) * dt(N)) * dt(N))
        ratio = omega_s / omega_p
        lg = log2_defined(ratio) if dt is f32 else np.log2(ratio)
        level = dt(0.5) * lg + dt(f32(bias))
    return np.fmin(np.fmax(level, dt(0)), dt(M - 1)).astype(dt)


def filter_texels(chain, kind, n, texels, samples, roughness, bias, dtype=f32, chunk=64):
    """The unrounded filter result, (T, 3) of dtype, at the texels (face, x, y) -- three int arrays of length T -- of a level of resolution
    n, and per texel the largest |tap component| any of its samples fetched.  chain: chain_from_mip0's."""
    dt = dtype
    N, M = chain[0].shape[1], len(chain)
    PI = dt(f32(3.14159265359))
    TAU = dt(f32(2.0) * f32(3.14159265359))
    face, x, y = (np.asarray(a, np.int64) for a in texels)
    normal = cubemap_to_direction(face, (x.astype(dt) + dt(0.5)) / dt(n), (y.astype(dt) + dt(0.5)) / dt(n), dt)
    zero = np.zeros_like(normal[:, 0])
    first = np.abs(normal[:, 0]) > np.abs(normal[:, 2])                       # CreateBasis
    b = np.where(first[:, None], np.stack([-normal[:, 1], normal[:, 0], zero], 1), np.stack([zero, -normal[:, 2], normal[:, 1]], 1))
    b = _normalize(b)
    t = np.stack([b[:, 1] * normal[:, 2] - b[:, 2] * normal[:, 1], b[:, 2] * normal[:, 0] - b[:, 0] * normal[:, 2],
                  b[:, 0] * normal[:, 1] - b[:, 1] * normal[:, 0]], 1)
    u0, u1 = (u.astype(dt) for u in r2(samples))
    a = dt(f32(roughness))
    cs, sn = _sincos(TAU * u0, dt)
    with _quiet():
        if kind == GGX:
            ct = np.sqrt((dt(1) - u1) / (dt(1) + (a * a - dt(1)) * u1))
            st = np.sqrt(dt(1) - ct * ct)
            h = np.stack([st * cs, st * sn, ct], 1)
            e = h[:, 2] * h[:, 2] * (a * a - dt(1)) + dt(1)
            e = e * (PI * e)
            D = (a * a) * np.where(h[:, 2] > 0, dt(1), dt(0)) / e
            table_level = mip_level(D / dt(4), samples, N, M, bias, dt)
        else:
            yy = dt(2) * u1 - dt(1)
            rr = np.sqrt(dt(1) - yy * yy)
            point = np.stack([rr * cs, rr * sn, yy], 1)
    total = np.zeros((len(face), 3), dt)
    total_weight = np.zeros(len(face), dt)
    big = np.zeros(len(face), dt)
    nn = normal[:, None, :]
    for s0 in range(0, samples, chunk):
        k = slice(s0, min(s0 + chunk, samples))
        with _quiet():
            if kind == GGX:
                hk = h[None, k, :]
                hw = t[:, None, :] * hk[..., 0:1] + b[:, None, :] * hk[..., 1:2] + nn * hk[..., 2:3]
                v = -nn
                l = v - (dt(2) * _dot(hw, v))[..., None] * hw
                weight = np.fmin(np.fmax(_dot(nn, l), dt(0)), dt(1))
                level = np.broadcast_to(table_level[None, k], weight.shape)
            else:
                l = _normalize(nn + point[None, k, :])
                pdf = np.fmin(np.fmax(_dot(l, nn) / PI, dt(0)), dt(1))
                weight = np.ones(pdf.shape, dt)
                level = mip_level(pdf, samples, N, M, bias, dt)
            c, bg = sample_level(chain, np.ascontiguousarray(l), np.ascontiguousarray(level), dt)
            c = weight[..., None] * c
            for j in range(c.shape[1]):                                   # the sum is sequential in i
                total = total + c[:, j]
                total_weight = total_weight + weight[:, j]
        big = np.maximum(big, bg.max(axis=1))
    with _quiet():
        return (total / total_weight[:, None]).astype(dt), big


def all_texels(n):
    face, y, x = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
    return face.reshape(-1), x.reshape(-1), y.reshape(-1)


def to_half(v):
    """The stored texel: rgb rounded to nearest-even half (as float32 values)."""
    with _quiet():
        return np.asarray(v).astype(f16).astype(f32)


def half_rounding(v):
    """One RGBA16F rounding of the value v: half the spacing of halfs at |v| (the subnormal spacing below 2^-14)."""
    with _quiet():
        h = np.abs(np.asarray(v, f64)).astype(f16)
        h = np.where(np.isfinite(h), h, f16(65504))
        return np.spacing(h).astype(f64) * 0.5


def e32(chain, kind, n, texels, samples, roughness, bias):
    """E32 of one level: the float32 restatement's largest distance from float64, as a share of the largest tap the texel fetched; and the
    two results with the taps, for whoever compares a third computation with them."""
    v32, big = filter_texels(chain, kind, n, texels, samples, roughness, bias, f32)
    v64, big64 = filter_texels(chain, kind, n, texels, samples, roughness, bias, f64)
    big = np.maximum(big.astype(f64), big64)
    with _quiet():
        share = np.abs(v32.astype(f64) - v64).max(axis=1) / big
    share = np.where(big > 0, share, 0.0)
    return float(np.nanmax(share)), v32, v64, big
