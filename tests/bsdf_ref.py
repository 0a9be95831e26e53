"""The material model and the punctual lights restated in numpy float64, directly from the reference's shader text and with a different
structure from oracle/ and the kernels (vectorised over the inputs, no shared helpers with either):

  * GltfBsdf, both overloads                     Source/Shaders/Bsdf.hlsli:241-325 (and the helpers it calls, :26-228)
  * LayerProbabilities, BsdfPdf                  Source/Shaders/PathTracer.lib.hlsl:535-565 (and the lobe pdfs :337-500)
  * GetLightRay                                  Source/Shaders/Lights.hlsli:26-61

with the random surfaces and directions they are compared on, the 36-float SurfaceProperties packing, the 48-float query layout of
pt_debug_bsdf_query / orc_bsdf_query_many, and the comparison `_check` with the project's thresholds.  Shared by
tests/test_oracle_independent.py (oracle against float64, CPU) and tests/test_gpu_bsdf.py (kernels against the oracle and float64)."""
import math
import os

import numpy as np

PI = math.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = np.load(os.path.join(ROOT, "tests", "golden", "sheen_e_16x16.npy")).astype(np.float64).reshape(16, 16)      # rows = alpha, columns = cos(theta)


# ---- the second restatement (numpy, float64, arrays of N inputs) ---------------------------------------------------------------
def dot(a, b):
    return (a * b).sum(axis=-1)


def nrm(a):
    return a / np.sqrt(dot(a, a))[..., None]


def hclamp(x, lo, hi):                          # HLSL clamp = min(max(x, lo), hi), and min / max return the non-NaN operand
    return np.fmin(np.fmax(x, lo), hi)


def sat(x):                                      # saturate(NaN) = 0
    return hclamp(x, 0.0, 1.0)


def step(x):                                     # Heavyside, Bsdf.hlsli:29-32
    return (x > 0).astype(np.float64)


def hpow(x, y):                                  # HLSL pow = exp2(y * log2(x)): NaN for x < 0, pow(0, y > 0) = 0
    with np.errstate(all="ignore"):
        return np.exp2(y * np.log2(x))


def schlick(f0, c):                              # :39-47
    return f0 + (1 - f0) * hpow(1 - np.abs(c), 5.0)


def ggx_d(a, ndh):                               # :50-57
    a2 = a * a
    den = ndh * ndh * (a2 - 1) + 1
    return a2 * step(ndh) / (PI * den * den)


def ggx_corr_v(a, ndl, ndv, hdl, hdv):           # :77-84
    a2 = a * a
    den = np.abs(ndv) * np.sqrt(a2 + (1 - a2) * ndl * ndl) + np.abs(ndl) * np.sqrt(a2 + (1 - a2) * ndv * ndv)
    return 0.5 * step(hdl) * step(hdv) / den


def specular_brdf(a, ndl, ndv, ndh, hdl, hdv):   # :86-89
    return ggx_corr_v(a, ndl, ndv, hdl, hdv) * ggx_d(a, ndh)


def ggx_aniso_d(ax, ay, h):                      # :92-98
    a2 = ax * ay
    f = np.stack([ay * h[..., 0], ax * h[..., 1], a2 * h[..., 2]], axis=-1)
    w2 = a2 / dot(f, f)
    return step(h[..., 2]) * a2 * w2 * w2 / PI


def aniso_len(ax, ay, w):
    return np.sqrt((ax * w[..., 0]) ** 2 + (ay * w[..., 1]) ** 2 + w[..., 2] ** 2)


def aniso_specular(ax, ay, v, h, l):             # :116-129
    hdv, hdl = dot(h, v), dot(h, l)
    vv = np.abs(l[..., 2]) * aniso_len(ax, ay, v)
    ll = np.abs(v[..., 2]) * aniso_len(ax, ay, l)
    return 0.5 * step(hdv) * step(hdl) / (vv + ll) * ggx_aniso_d(ax, ay, h)


def fresnel_mix(f0_color, ior, weight, base, layer, hdv):            # :136-143
    f0 = ((1 - ior) / (1 + ior))[..., None] * np.ones(3)
    f0 = f0 * (f0 * f0_color)                    # `f0 *= f0 * f0_color`
    f0 = np.fmin(f0, 1.0)
    fr = schlick(f0, hdv[..., None])
    return (1 - weight[..., None] * fr.max(axis=-1)[..., None]) * base + weight[..., None] * fr * layer


def fresnel_coat(ior, weight, base, layer, ndv):                     # :156-162
    f0 = ((1 - ior) / (1 + ior)) ** 2
    fr = schlick(f0, ndv)
    t = (weight * fr)[..., None]
    return base + t * (layer - base)


def sheen_l(alpha, x):                           # :174-183
    t = (1 - alpha) ** 2
    lerp = lambda p, q: p + t * (q - p)
    a, b, c, d, e = lerp(21.5473, 25.3245), lerp(3.82987, 3.32435), lerp(0.19823, 0.16801), lerp(-1.97760, -1.27393), lerp(-4.32054, -4.85967)
    return a / (1 + b * hpow(x, c)) + d * x + e


def sheen_shadowing(alpha, c):                   # :185-192
    with np.errstate(all="ignore"):
        return np.where(c < 0.5, np.exp(sheen_l(alpha, c)), np.exp(2 * sheen_l(alpha, np.full_like(c, 0.5)) - sheen_l(alpha, 1 - c)))


def sheen_brdf(alpha, ndl, ndv, ndh):            # :164-202 (SheenBrdf hands (n_dot_v, n_dot_l) to SheenVisibility: symmetric)
    inv_r = 1 / alpha
    d = (2 + inv_r) * hpow(1 - ndh * ndh, inv_r * 0.5) / (2 * PI)
    with np.errstate(all="ignore"):
        vis = hclamp(1 / ((1 + sheen_shadowing(alpha, ndv) + sheen_shadowing(alpha, ndl)) * 4 * ndv * ndl), 0, 1)
    return d * vis


def sheen_e(alpha, c):
    """Texture2D<float>.SampleLevel(linear_clamp, (cos_theta, alpha), 0) on the 16x16 table: D3D bilinear, texel centres at +0.5."""
    x, y = c * 16 - 0.5, alpha * 16 - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix = lambda i: np.clip(i, 0, 15).astype(int)
    t = lambda i, j: LUT[ix(j), ix(i)]
    return (t(x0, y0) * (1 - fx) + t(x0 + 1, y0) * fx) * (1 - fy) + (t(x0, y0 + 1) * (1 - fx) + t(x0 + 1, y0 + 1) * fx) * fy


def modulate_roughness(a, ior):                  # :216-220
    return hclamp(a * sat(2 * (ior - 1)), 0.001, 1.0)


def thin_btdf(color, a, ior, n, v, l):           # :222-228
    a = modulate_roughness(a, ior)
    l = l - 2 * dot(n, l)[..., None] * n
    h = nrm(v + l)
    return color * specular_brdf(a, dot(n, l), dot(n, v), dot(n, h), dot(h, l), dot(h, v))[..., None]


def gltf_bsdf(sp, v, l, is_transmission=None):
    """Bsdf.hlsli:241-282 (is_transmission None) and :284-325 (a bool array)."""
    n = sp["shading_normal"]
    ax, ay = sp["roughness_squared"][..., 0], sp["roughness_squared"][..., 1]
    h = nrm(v + l)
    loc = lambda w: np.stack([dot(sp["anisotropy_tangent"], w), dot(sp["anisotropy_bitangent"], w), dot(n, w)], axis=-1)
    vl, hl, ll = loc(v), loc(h), loc(l)
    hdl, hdv = dot(h, l), dot(h, v)
    la = ll.copy(); la[..., 2] = np.abs(la[..., 2])
    h_dot_abs_l = dot(nrm(la + vl), vl)
    if is_transmission is None:
        refl = trans = np.ones(len(v))
    else:
        refl, trans = (~is_transmission).astype(np.float64), is_transmission.astype(np.float64)
    zeros = lambda x, keep: np.where(keep[..., None] > 0, x, 0.0)
    specular = zeros((sat(ll[..., 2]) * aniso_specular(ax, ay, vl, hl, ll))[..., None] * np.ones(3), refl)
    diffuse = zeros(sat(ll[..., 2])[..., None] * sp["albedo"] / PI, refl)
    transmission = zeros(sat(-ll[..., 2])[..., None] * thin_btdf(sp["albedo"], ay, sp["ior"], n, v, l), trans)
    diffuse = diffuse + sp["transmissive"][..., None] * (transmission - diffuse)
    dielectric = fresnel_mix(sp["specular_color"], sp["ior"], sp["specular_factor"], diffuse, specular, h_dot_abs_l)
    metal = zeros(specular * schlick(sp["albedo"], hdv[..., None]), refl)
    material = dielectric + sp["metalness"][..., None] * (metal - dielectric)
    sa = hclamp(sp["sheen_roughness_squared"], 0.000001, 1)
    sheen = zeros((sat(ll[..., 2]) * sheen_brdf(sa, ll[..., 2], vl[..., 2], hl[..., 2]))[..., None] * np.ones(3), refl)
    mx = sp["sheen_color"].max(axis=-1)
    scaling = np.fmin(1 - mx * sheen_e(sa, vl[..., 2]), 1 - mx * sheen_e(sa, ll[..., 2]))
    material = sp["sheen_color"] * sheen + material * scaling[..., None]
    cndv, cndh, cndl = dot(n, v), dot(n, h), dot(n, l)           # clearcoat lobe evaluated about the SHADING normal (:273-277)
    cc = np.where(refl > 0, sat(cndl) * specular_brdf(sp["clearcoat_roughness"], cndl, cndv, cndh, hdl, hdv), 0.0)
    return fresnel_coat(1.5, sp["clearcoat"], material, cc[..., None] * np.ones(3), cndv)


def layer_probabilities(sp, v):                  # PathTracer.lib.hlsl:535-553
    rem = np.ones(len(v))
    p = {}
    p["alpha"] = 1.0 - sp["alpha"]; rem = rem - p["alpha"]
    p["clearcoat"] = fresnel_coat(1.5, sp["clearcoat"], np.zeros((len(v), 3)), np.ones((len(v), 3)), dot(sp["clearcoat_normal"], v))[..., 0] * rem
    rem = rem - p["clearcoat"]
    p["sheen"] = np.where((sp["sheen_color"] > 0).any(axis=-1), 0.5, 0.0) * rem; rem = rem - p["sheen"]
    p["specular"] = 0.5 * rem; rem = rem - p["specular"]
    p["transmission"] = sp["transmissive"] * rem; rem = rem - p["transmission"]
    p["diffuse"] = rem
    return p


def bsdf_pdf(sp, v, l, is_transmission, p):      # :555-565 with the lobe pdfs :337-347, :355-358, :378-394, :401-404, :424-435
    n = sp["shading_normal"]
    ggx_normal_pdf = lambda a, nn, hh: ggx_d(a, dot(nn, hh)) * dot(nn, hh)                       # Sampling.hlsli:55-59
    # transmission: mirror l about the shading normal, isotropic GGX of the modulated roughness
    lt = l - 2 * dot(n, l)[..., None] * n
    ht = nrm(v + lt)
    with np.errstate(all="ignore"):
        t_pdf = ggx_normal_pdf(modulate_roughness(sp["roughness_squared"][..., 1], sp["ior"]), n, ht) / (4 * dot(v, ht))
        h = nrm(v + l)
        cc = ggx_normal_pdf(sp["clearcoat_roughness"], sp["clearcoat_normal"], h) / (4 * dot(v, h))
        cosine = sat(dot(l, n) / PI)
        hl = np.stack([dot(sp["anisotropy_tangent"], h), dot(sp["anisotropy_bitangent"], h), dot(n, h)], axis=-1)
        spec = ggx_aniso_d(sp["roughness_squared"][..., 0], sp["roughness_squared"][..., 1], hl) * hl[..., 2] / (4 * dot(v, h))
        refl = p["clearcoat"] * cc + p["sheen"] * cosine + p["specular"] * spec + p["diffuse"] * cosine
    return np.where(is_transmission, p["transmission"] * t_pdf, refl)


# ---- random inputs ------------------------------------------------------------------------------------------------------------------
ORDER = [("albedo", 3), ("alpha", 1), ("metalness", 1), ("roughness_squared", 2), ("shading_normal", 3), ("anisotropy_tangent", 3),
         ("anisotropy_bitangent", 3), ("ior", 1), ("specular_color", 3), ("specular_factor", 1), ("clearcoat", 1), ("clearcoat_roughness", 1),
         ("clearcoat_normal", 3), ("sheen_color", 3), ("sheen_roughness_squared", 1), ("transmissive", 1), ("thickness", 1),
         ("attenuation_distance", 1), ("attenuation_color", 3)]


def random_surfaces(rng, n):
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)          # inputs representable in float32: both sides see the same numbers
    unit = lambda k: nrm(rng.normal(size=(k, 3)))
    sp = {}
    nn = unit(n)
    t = nrm(np.cross(nn, unit(n)))
    sp["shading_normal"], sp["anisotropy_tangent"], sp["anisotropy_bitangent"] = f32(nn), f32(t), f32(nrm(np.cross(t, nn)))
    sp["albedo"] = f32(rng.uniform(0.02, 1, (n, 3)))
    sp["alpha"] = f32(np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.1, 1, n)))
    sp["metalness"] = f32(np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0, 1, n)))
    ry = np.maximum(rng.uniform(0.03, 1, n) ** 2, 0.001)
    sp["roughness_squared"] = f32(np.stack([np.maximum(ry + rng.uniform(0, 1, n) ** 2 * (1 - ry), 0.001), ry], axis=1))
    sp["ior"] = f32(rng.uniform(1.0, 2.0, n))
    sp["specular_color"] = f32(rng.uniform(0, 1, (n, 3)))
    sp["specular_factor"] = f32(rng.uniform(0, 1, n))
    sp["clearcoat"] = f32(np.where(rng.random(n) < 0.4, 0.0, rng.uniform(0, 1, n)))
    sp["clearcoat_roughness"] = f32(rng.uniform(0.03, 1, n))
    sp["clearcoat_normal"] = f32(nrm(nn + 0.2 * rng.normal(size=(n, 3))))
    sp["sheen_color"] = f32(np.where(rng.random((n, 1)) < 0.5, 0.0, rng.uniform(0, 1, (n, 3))))
    sp["sheen_roughness_squared"] = f32(np.maximum(rng.uniform(0.05, 1, n) ** 2, 0.001))
    sp["transmissive"] = f32(np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0, 1, n)))
    sp["thickness"], sp["attenuation_distance"] = np.zeros(n), np.zeros(n)
    sp["attenuation_color"] = np.ones((n, 3))
    return sp


def pack36(sp, i):
    flat = []
    for k, w in ORDER:
        flat += [float(sp[k][i])] if w == 1 else [float(x) for x in sp[k][i]]
    assert len(flat) == 36
    return np.array(flat, np.float32)


def pack36_all(sp):
    """pack36 of every surface at once: (n, 36) float32."""
    n = len(sp["alpha"])
    out = np.concatenate([np.asarray(sp[k], np.float64).reshape(n, w) for k, w in ORDER], axis=1).astype(np.float32)
    assert out.shape == (n, 36)
    return out


def unpack36(s36):
    """The surfaces of (n, 36) float32 rows as the dict of float64 arrays the restatement takes."""
    s36 = np.asarray(s36, np.float32).astype(np.float64)
    sp, at = {}, 0
    for k, w in ORDER:
        sp[k] = s36[:, at] if w == 1 else s36[:, at:at + w]
        at += w
    return sp


def pack48(s36, ng, v, a):
    """The 48-float queries of pt_debug_bsdf_query / orc_bsdf_query_many: surface, geometric normal, view, and l (EVALUATE) or u (SAMPLE)."""
    s36 = np.asarray(s36, np.float32)
    q = np.zeros((len(s36), 48), np.float32)
    q[:, :36] = s36; q[:, 36:39] = ng; q[:, 39:42] = v; q[:, 42:45] = a
    return q


def directions(rng, sp, n, transmit_fraction):
    """v on the shading normal's side, l on the same side or (a fraction) through the surface; both float32-representable."""
    nn = sp["shading_normal"]
    def hemi(sign):
        d = nrm(rng.normal(size=(n, 3)))
        c = dot(d, nn)
        d = d - nn * (c - sign * np.abs(c))[..., None]              # reflect into the wanted hemisphere
        return nrm(d + sign * 0.05 * nn)                            # keep away from grazing, where Heavyside steps amplify rounding
    v = hemi(1.0)
    through = rng.random(n) < transmit_fraction
    l = np.where(through[:, None], hemi(-1.0), hemi(1.0))
    v32, l32 = v.astype(np.float32), l.astype(np.float32)
    v32 /= np.linalg.norm(v32, axis=1, keepdims=True); l32 /= np.linalg.norm(l32, axis=1, keepdims=True)
    return v32.astype(np.float64), l32.astype(np.float64), through


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(np.abs(want), 1e-4 * max(1.0, float(np.abs(want).max())) if want.size else 1.0)


def _check(name, got, want, tol_typical=2e-5, tol_max=2e-2, tol_median=1e-6):
    ok = np.isfinite(want) & np.isfinite(got)
    assert (np.isfinite(want) == np.isfinite(got)).mean() > 0.999, name
    e = rel_err(got[ok], want[ok])
    print("%s: median rel %.1e, 99%% %.1e, max %.1e over %d values" % (name, float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max()), e.size))
    assert np.median(e) <= tol_median, (name, float(np.median(e)))
    assert np.quantile(e, 0.99) <= tol_typical, (name, float(np.quantile(e, 0.99)))
    assert e.max() <= tol_max, (name, float(e.max()))


def sample_masks(sp, p, ux):
    """For SampleBsdf queries with first random number ux: the cumulative lobe edges in float64, `margin` (ux away from every edge: the
    float32 subtraction chain upstream may pick the neighbouring lobe within it) and `smooth` (every lobe's alpha >= 0.05: a sampled direction
    sits ON its lobe's peak, where D(h) of a near-mirror lobe amplifies the float32 rounding of h = normalize(v + l) by ~1 / alpha^2)."""
    edges = np.cumsum(np.stack([p["alpha"], p["clearcoat"], p["sheen"], p["specular"], p["transmission"]], axis=1), axis=1)
    margin = np.abs(edges - ux[:, None]).min(axis=1) > 1e-5
    smooth = np.minimum(sp["roughness_squared"].min(axis=1), np.minimum(sp["clearcoat_roughness"], modulate_roughness(sp["roughness_squared"][:, 1], sp["ior"]))) >= 0.05
    return edges, margin, smooth


# ---- punctual lights (Lights.hlsli:26-61) ---------------------------------------------------------------------------------------------
LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 0, 1, 2
U32 = 2.0 ** -24                                 # float32 unit roundoff


def lights_array(n):
    """n zeroed Light records as (n, 16) float32 rows: [0] type (int32 bits) [1:4] position [4] cutoff [5:8] direction [8] intensity
    [9:12] colour [12] inner angle [13] outer angle [14:16] padding."""
    return np.zeros((n, 16), np.float32)


def light_types(lights):
    """The types of the records, as a copy."""
    return np.ascontiguousarray(lights[:, 0]).view(np.int32)


def set_light_types(lights, types):
    lights[:, 0] = np.asarray(types, np.int32).view(np.float32)


def light_ray(lights, index, p):
    """GetLightRay(lights[index[q]], p[q]) in float64: (direction (n, 3), colour (n, 3)).  Non-finite where the shader's is (a point at the
    light's position, a zero light direction)."""
    L = np.asarray(lights, np.float32)[index]
    t = light_types(np.asarray(lights, np.float32))[index]
    L = L.astype(np.float64)
    p = np.asarray(p, np.float32).astype(np.float64)
    local = (t == LIGHT_POINT) | (t == LIGHT_SPOT)
    with np.errstate(all="ignore"):
        d = np.where(local[:, None], L[:, 1:4] - p, -L[:, 5:8])
        color = L[:, 9:12] * L[:, 8:9]
        dist = np.sqrt(dot(d, d))
        cutoff = L[:, 4]
        window = np.where(cutoff > 0, np.fmax(np.fmin(1.0 - (dist / np.where(cutoff > 0, cutoff, 1.0)) ** 4, 1.0), 0.0), 1.0)
        color = np.where(local[:, None], color * (window / (dist * dist))[:, None], color)
        d = d / dist[:, None]
        scale = 1.0 / np.maximum(0.001, np.cos(L[:, 12]) - np.cos(L[:, 13]))
        offset = -np.cos(L[:, 13]) * scale
        cd = -dot(nrm(L[:, 5:8]), d)
        att = sat(cd * scale + offset)
        color = np.where((t == LIGHT_SPOT)[:, None], color * (att * att)[:, None], color)
    return d, color


def light_ray_bound(lights, index, p):
    """Bounds on |float32 GetLightRay - light_ray| per query, to first order in u = 2^-24 with 1 % for the higher orders, from the float32
    operation count of the shader text under the project's defined math (correctly rounded +, -, *, /, sqrt and cos; x^4 as two products):

      direction  position - p is ONE rounding of exact inputs: u per component.  |d|^2: 2u (components) + u (product) + 2u (two sums of
                 non-negative terms) = 5u, the root halves it and rounds: distance 3.5u.  component / distance: u + 3.5u + u = 5.5u of a
                 component that is at most 1: 6u absolute.  (Directional: exact components, 3.5u.)
      window     distance / cutoff 4.5u; squared twice: 2 (2 * 4.5u + u) + u = 21u of a value <= 1 where the window is not 0; 1 - that and its
                 rounding: 22u absolute on a window in [0, 1].  distance^2 8u, the quotient's rounding u: (22u + 9u) / distance^2.
      colour     colour * intensity u, times the falloff u: C0 / distance^2 * 33u with C0 = |colour * intensity|.
      cone       cos(inner) - cos(outer): u + u + u absolute; m = max(0.001, .); scale = 1 / m: es = 3u / m + u relative; offset: es + 2u
                 relative, |offset| <= scale.  cd: normalised light direction 3.5u, ray direction 5.5u, product u, two sums 2u: <= 13u
                 absolute for unit vectors.  cd * scale + offset: scale * (13u + es + u) + scale * (es + 2u) + u inside [0, 1]:
                 Ea = scale * (16u + 2 es) + u.  Squared: 2 Ea + Ea^2 + u; times the colour: u.

    Returns (bound on a direction component, bound on a colour component (n,), Ea (n,))."""
    L = np.asarray(lights, np.float32)[index].astype(np.float64)
    t = light_types(np.asarray(lights, np.float32))[index]
    u = U32
    d, _ = light_ray(lights, index, p)
    with np.errstate(all="ignore"):
        dist2 = dot(L[:, 1:4] - np.asarray(p, np.float32).astype(np.float64), L[:, 1:4] - np.asarray(p, np.float32).astype(np.float64))
        c0 = np.abs(L[:, 9:12] * L[:, 8:9]).max(axis=1)
        local = (t == LIGHT_POINT) | (t == LIGHT_SPOT)
        base = np.where(local, c0 / dist2, c0)
        m = np.maximum(0.001, np.cos(L[:, 12]) - np.cos(L[:, 13]))
        es = 3 * u / m + u
        ea = np.where(t == LIGHT_SPOT, (16 * u + 2 * es) / m + u, 0.0)
        cone = np.where(t == LIGHT_SPOT, 2 * ea + ea * ea + 2 * u, 0.0)
        color_bound = 1.01 * base * (np.where(local, 33 * u, 2 * u) + cone)
    return 1.01 * 6 * u, color_bound, ea
