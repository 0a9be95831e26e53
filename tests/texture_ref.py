"""A float64 statement of D3D Texture2D.SampleLevel(s, uv, 0) on an RGBA8 texture behind a KHR_texture_transform,
written from the D3D rules and sharing no code with the oracle.  tests/test_gpu_texture.py holds the product's sampler and the oracle's to it
query by query; tests/surface_ref.py samples its material slots through it."""
import math

import numpy as np

from gltf_renderer_amd import abi

f32 = np.float32
WRAP, MIRROR, CLAMP = abi.ADDRESS_WRAP, abi.ADDRESS_MIRROR, abi.ADDRESS_CLAMP
POINT, LINEAR = abi.FILTER_POINT, abi.FILTER_LINEAR


def srgb_to_linear(c):
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def address(i, n, mode):
    """D3D texture address modes on integer texel indices (Python integer modulo: non-negative)."""
    i = [int(k) for k in i]
    if mode == WRAP:
        r = [k % n for k in i]
    elif mode == MIRROR:
        r = [(k % (2 * n)) if (k % (2 * n)) < n else 2 * n - 1 - (k % (2 * n)) for k in i]
    else:
        r = [min(max(k, 0), n - 1) for k in i]
    return np.array(r, np.int64)


def transform_rows(rotation, offset, scale):
    """The UV transform T * R * S as the host forms it in fp32: sin / cos correctly rounded from the fp32 angle."""
    rot = float(f32(rotation))
    sn, cs = (f32(math.sin(rot)), f32(math.cos(rot))) if rot != 0.0 else (f32(0), f32(1))
    sx, sy = f32(scale[0]), f32(scale[1])
    return (cs * sx, sn * sy, f32(offset[0]), -sn * sx, cs * sy, f32(offset[1]))


def sample_level0(data, srgb, sampler, rows, uv):
    """Float64 SampleLevel(..., 0) of the texture `data` (H, W, 4) uint8 at the n UVs `uv` (n, 2).  sampler: (address u, address v,
    filter); rows: transform_rows(...).  The fp32 steps up to the texel coordinate are the product's (transform without FMA, * size,
    non-finite -> 0, clamp to +-1e9 texels, - 0.5, floor); everything after them is float64.  Returns rgba (n, 4) float64, taps (n, 4) =
    i0, i1, j0, j1, and per-query flags (with texel_xy: the fp32 texel coordinates the floor was taken of)."""
    n = len(uv)
    H, W = data.shape[:2]
    au, av, flt = sampler
    m00, m01, ox, m10, m11, oy = rows
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = uv[:, 0].astype(f32), uv[:, 1].astype(f32)
        tu = (m00 * u + m01 * v) + ox                 # numpy float32: every operation rounded, no contraction
        tv = (m10 * u + m11 * v) + oy
        x, y = tu * f32(W), tv * f32(H)
        nf = ~np.isfinite(x) | ~np.isfinite(y)
        x = np.where(np.isfinite(x), x, f32(0)); y = np.where(np.isfinite(y), y, f32(0))
        cl = (np.abs(x) > f32(1e9)) | (np.abs(y) > f32(1e9))
        x = np.clip(x, f32(-1e9), f32(1e9)); y = np.clip(y, f32(-1e9), f32(1e9))
        unit_w = np.zeros(n, bool)
        if flt == POINT:
            i0 = i1 = address(np.floor(x), W, au); j0 = j1 = address(np.floor(y), H, av)
            w = [np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n)]
        else:
            x = x - f32(0.5); y = y - f32(0.5)
            fx0, fy0 = np.floor(x), np.floor(y)
            fx = x.astype(np.float64) - fx0.astype(np.float64); fy = y.astype(np.float64) - fy0.astype(np.float64)
            i0 = address(fx0, W, au); i1 = address(fx0.astype(np.int64) + 1, W, au)
            j0 = address(fy0, H, av); j1 = address(fy0.astype(np.int64) + 1, H, av)
            w = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
            unit_w = (fx == 0) & (fy == 0)

        def val(j, i):
            c = data[j, i].astype(np.float64) / 255.0
            if srgb:
                c[:, :3] = srgb_to_linear(c[:, :3])                   # sRGB decoded before filtering; alpha linear
            return c
        rgba = val(j0, i0) * w[0][:, None] + val(j0, i1) * w[1][:, None] + val(j1, i0) * w[2][:, None] + val(j1, i1) * w[3][:, None]
    taps = np.stack([i0, i1, j0, j1], 1)
    return rgba, taps, dict(nonfinite=nf, clamped=cl, unit_weights=unit_w, linear=np.full(n, flt != POINT), texel_xy=np.stack([x, y], 1))
