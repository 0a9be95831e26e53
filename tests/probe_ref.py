"""Restatement of light-probe baking (include/mipt.h pt_set_probes, pt_probe_project), used by tests/test_gpu_probe.py and checked on its own
by tests/test_probe_host.py.

The atlas layout and the ray are float32 numpy, operation for operation; the direction of a square point is the oracle's orc_square_to_sphere
on that same float32 point (bit-identical to the product's square_to_sphere by tests/test_oracle_kat.py and tests/test_gpu_envmap.py).  The
spherical-harmonic basis and the projection are float64 -- with the header's float32 constants -- and so carry none of the product's
roundings.  A float64 statement of the mapping itself (square_to_sphere64) serves the properties that need no oracle: the Gram matrix of the
texel-centre quadrature and the projection of analytic fields."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
PI_F32 = float(f32(3.14159265359))          # the kernels' kPi (Common.hlsli:8), a float32 constant

# Y_lm in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2): the header's constants, each rounded once to float
SH_CONST = [float(f32(c)) for c in (0.282094792, 0.488602512, 0.488602512, 0.488602512, 1.092548431, 1.092548431, 0.315391565, 1.092548431, 0.546274215)]
SH_BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
# the clamped-cosine kernel's band factors pi, 2 pi / 3, pi / 4 (Ramamoorthi & Hanrahan 2001)
BAND_FACTOR = np.array([math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0])


# ---- layout -----------------------------------------------------------------------------------------------------------------------------
def atlas_size(n, count, columns):
    """(W, H) of the atlas of `count` n x n maps, `columns` to a row."""
    rows = -(-count // columns)
    return columns * n, rows * n


def cell(n, columns, px, py):
    """Atlas pixel -> (probe index k, lx, ly); k may be >= count (an empty cell)."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    cx, cy = px // n, py // n
    return cy * columns + cx, px - cx * n, py - cy * n


# ---- the mapping ------------------------------------------------------------------------------------------------------------------------
def uv_to_square32(u, v):
    """UvToSquare (Transforms.hlsli:52-55) in float32: (u * 2 + -1, v * -2 + 1), products and sums not fused."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    return ((u * f32(2)).astype(f32) + f32(-1)).astype(f32), ((v * f32(-2)).astype(f32) + f32(1)).astype(f32)


def oracle_sphere(oracle, sx, sy):
    """orc_square_to_sphere per float32 square point: float32 [n, 3]."""
    import ctypes as C
    L = oracle.lib()
    sx, sy = np.asarray(sx, f32).ravel(), np.asarray(sy, f32).ravel()
    out = np.zeros((len(sx), 3), f32)
    a, b = np.zeros(2, f32), np.zeros(3, f32)
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    for i in range(len(sx)):
        a[0], a[1] = sx[i], sy[i]
        L.orc_square_to_sphere(pa, pb)
        out[i] = b
    return out


def square_to_sphere64(sx, sy):
    """SquareToSphere (Transforms.hlsli:124-136) in float64, with the kernels' float32 pi: [..., 3]."""
    sx, sy = np.asarray(sx, f64), np.asarray(sy, f64)
    d = 1 - (np.abs(sx) + np.abs(sy))
    r = 1 - np.abs(d)
    phi = np.where(r == 0, 0.0, (PI_F32 / 4) * ((np.abs(sy) - np.abs(sx)) / np.where(r == 0, 1.0, r) + 1))
    f = r * np.sqrt(2 - r * r)
    return np.stack([f * np.sign(sx) * np.cos(phi), f * np.sign(sy) * np.sin(phi), np.sign(d) * (1 - r * r)], axis=-1)


def centre_uv32(n):
    """The texel centres of an n x n map as the product divides them: u[i] = (i + 0.5) / n in float32 (a correctly rounded division)."""
    return ((np.arange(n, dtype=f32) + f32(0.5)) / f32(n)).astype(f32)


def centre_dirs64(n):
    """w(i, j) in float64 from the float32 centres: [n (j), n (i), 3]."""
    c = centre_uv32(n)
    sx, sy = uv_to_square32(c[None, :].repeat(n, 0), c[:, None].repeat(n, 1))
    return square_to_sphere64(sx, sy)


def centre_dirs_oracle(oracle, n):
    """w(i, j) as the product computes it (float32, the oracle's mapping): [n, n, 3] float32."""
    c = centre_uv32(n)
    sx, sy = uv_to_square32(c[None, :].repeat(n, 0), c[:, None].repeat(n, 1))
    return oracle_sphere(oracle, sx, sy).reshape(n, n, 3)


# ---- the ray ----------------------------------------------------------------------------------------------------------------------------
def sample_uv32(n, lx, ly, rnd):
    """u = (((float)lx + 0.5) + (r.x - 0.5)) / (float)n, v likewise: float32, in that order.  rnd [..., 4] float32."""
    rnd = np.asarray(rnd, f32)
    u = ((np.asarray(lx, f32) + f32(0.5)).astype(f32) + (rnd[..., 0] - f32(0.5)).astype(f32)).astype(f32) / f32(n)
    v = ((np.asarray(ly, f32) + f32(0.5)).astype(f32) + (rnd[..., 1] - f32(0.5)).astype(f32)).astype(f32) / f32(n)
    return u.astype(f32), v.astype(f32)


def rays(oracle, positions, n, columns, max_distance, queries, rnd):
    """The rays of the queries [m, 3] {px, py, seed} whose draws are rnd [m, 4] (orc_random(px, py, seed, 0)): float32 [m, 8] (origin, tmin,
    direction, tmax); zeros with tmax = -1 for a cell without a probe."""
    positions = np.asarray(positions, f32).reshape(-1, 3)
    q = np.asarray(queries, np.int64).reshape(-1, 3)
    k, lx, ly = cell(n, columns, q[:, 0], q[:, 1])
    present = k < len(positions)
    u, v = sample_uv32(n, lx, ly, rnd)
    sx, sy = uv_to_square32(u, v)
    out = np.zeros((len(q), 8), f32)
    out[:, 7] = -1
    out[present, 0:3] = positions[k[present]]
    out[present, 3] = 0
    out[present, 4:7] = oracle_sphere(oracle, sx[present], sy[present])
    out[present, 7] = f32(max_distance)
    return out, (sx, sy)


# ---- spherical harmonics ----------------------------------------------------------------------------------------------------------------
def sh_basis(w):
    """Y [..., 9] float64 at directions w [..., 3]."""
    w = np.asarray(w, f64)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    c = SH_CONST
    return np.stack([c[0] * np.ones_like(x), c[1] * y, c[2] * z, c[3] * x, c[4] * (x * y), c[5] * (y * z), c[6] * (3 * z * z - 1), c[7] * (x * z),
                     c[8] * (x * x - y * y)], axis=-1)


def project_map(L, dirs):
    """c[9, 3] = 4 pi / n^2 * sum L(i, j) Y(w(i, j)) in float64 for one n x n x 3 map; a texel with a non-finite channel counts as 0."""
    L = np.asarray(L, f64)[..., :3]
    n = L.shape[0]
    L = np.where(np.isfinite(L).all(axis=-1, keepdims=True), L, 0.0)
    Y = sh_basis(dirs)
    return (4.0 * math.pi / (n * n)) * np.einsum("jic,jil->lc", L, Y)


def project_atlas(atlas, dirs, n, count, columns, kind=0):
    """pt_probe_project in float64: [count, 9, 3], and per probe the sum of |L| over its (finite) texels [count, 3] for the bound."""
    out, mag = np.zeros((count, 9, 3)), np.zeros((count, 3))
    for k in range(count):
        cy, cx = divmod(k, columns)
        m = np.asarray(atlas, f64)[cy * n:(cy + 1) * n, cx * n:(cx + 1) * n, :3]
        out[k] = project_map(m, dirs)
        mag[k] = np.abs(np.where(np.isfinite(m).all(axis=-1, keepdims=True), m, 0.0)).sum(axis=(0, 1))
    if kind == 1:
        out = out * BAND_FACTOR[SH_BAND][None, :, None]
    return out, mag


def projection_bound(n, mag):
    """(n^2 + 8) * 2^-24 * (4 pi / n^2) * sum |L|: the product's float32 sum against the float64 one, whatever its order.  Every term L * Y
    has |Y| < 1; a sum of n^2 float32 terms carries at most n^2 - 1 roundings of partial sums no larger than sum |L|, each product one more
    (counted with its term), and the 8 cover the evaluation of Y (at most 4 roundings of values below 1), the scale and the band factor."""
    return (n * n + 8) * 2.0 ** -24 * (4.0 * math.pi / (n * n)) * np.asarray(mag, f64)


def gram_deviation(n):
    """max |G - I| of G = 4 pi / n^2 * sum Y Y' over the texel centres, float64."""
    Y = sh_basis(centre_dirs64(n)).reshape(-1, 9)
    G = (4.0 * math.pi / (n * n)) * (Y.T @ Y)
    return float(np.abs(G - np.eye(9)).max())


def clamped_cosine_sh(axis):
    """The exact coefficients of L(w) = max(dot(w, axis), 0): A_l * Y_lm(axis) [9], A = pi, 2 pi / 3, pi / 4, with the exact basis constants
    (the header's float32 ones differ from them by < 2^-24 relative)."""
    axis = np.asarray(axis, f64)
    return BAND_FACTOR[SH_BAND] * sh_basis(axis / np.linalg.norm(axis))


# ---- six 90-degree cube faces -----------------------------------------------------------------------------------------------------------
# forward and up of the six cameras (any consistent choice serves: the directions of the pixels are taken from the matrices)
CUBE_FACES = [((1, 0, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))]


def cube_world_to_view(position, face):
    """world_to_view of the camera at `position` looking along the face's forward axis (a right-handed view space that looks along -z)."""
    fwd, up = (np.asarray(v, f64) for v in CUBE_FACES[face])
    right = np.cross(fwd, up)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = right, up, -fwd
    m[:3, 3] = -m[:3, :3] @ np.asarray(position, f64)
    return m


def cube_pixel_dirs(face, m):
    """Unit directions [m (row), m (column), 3] and solid angles [m, m] of the pixel centres of a 90-degree m x m view of the face: pixel
    (i, j) has the image-plane position x = (i + 0.5) / m * 2 - 1, y = -((j + 0.5) / m * 2 - 1) at distance 1 and subtends
    (4 / m^2) / (1 + x^2 + y^2)^1.5."""
    fwd, up = (np.asarray(v, f64) for v in CUBE_FACES[face])
    right = np.cross(fwd, up)
    c = (np.arange(m) + 0.5) / m * 2 - 1
    x, y = c[None, :], -c[:, None]
    d = fwd[None, None, :] + x[..., None] * right[None, None, :] + y[..., None] * up[None, None, :]
    r2 = 1 + x * x + y * y
    return d / np.sqrt(r2)[..., None], (4.0 / (m * m)) / r2 ** 1.5


def cube_sh(faces):
    """SH radiance coefficients [9, 3] of six m x m x (3 or 4) face images (CUBE_FACES order): sum L Y dOmega over the pixels, float64."""
    out = np.zeros((9, 3))
    for f, img in enumerate(faces):
        img = np.asarray(img, f64)[..., :3]
        d, dw = cube_pixel_dirs(f, img.shape[0])
        out += np.einsum("jic,jil,ji->lc", img, sh_basis(d), dw)
    return out
