"""The shade stage's software texture unit (pt_shading.h: wrap_addr, finite_coord, texture_taps, tap_row / tap_quad, resolve_taps,
sample_slot, and get_surface's batched / interleaved fetch), query by query, through the test hook pt_debug_sample_texture.

Every query is checked four ways:
  * the texel columns and rows the footprint used equal those of a float64 statement of D3D Texture2D.SampleLevel(s, uv, 0)
    (SURVEY.md section 10), written here from the D3D rules and sharing no code with the oracle -- exactly -- and the texel pair
    each row is loaded from starts at clamp(i0, 0, width - 2);
  * the filtered RGBA is within RGBA_TOL of that statement;
  * the RGBA is bit-identical to the CPU oracle's SampleTexture (orc_sample_material_slot);
  * the RGBA is bit-identical across the two kernel builds (wavefront stages: tables in LDS; megakernel: tables in global memory)
    and with the interleaved texel copy on and off (MIPT_TEXTURE_INTERLEAVE=0).
Image tests only reach the UVs that rays happen to hit; the coordinates here are placed on texel centres, exact texel borders and the
ulps either side, wrap / mirror periods up to 1e6, both sides of the +-1e9-texel clamp, signed zeros, subnormals, infinities and NaN,
on power-of-two and other sizes, and the waves are shaped for the WRAP seam reload and for the interleaved / general branch split."""
import ctypes as C
import math
import time

import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import hooks

from texture_ref import sample_level0, transform_rows

f32 = np.float32
WRAP, MIRROR, CLAMP = abi.ADDRESS_WRAP, abi.ADDRESS_MIRROR, abi.ADDRESS_CLAMP
POINT, LINEAR = abi.FILTER_POINT, abi.FILTER_LINEAR

# Absolute bound on |kernel - float64 reference| per component.  The kernel forms the four bilinear weights as fp32 products of
# fp32 differences (each within 3 roundings of the exact weight, relative 2^-24 each), multiplies each by a texel value in [0, 1]
# and sums four terms in fp32 (4 more roundings of a value <= 1); an sRGB texel value is one fp32 rounding (2^-25 relative) of the
# exact decode.  That totals below 1e-6; 2e-6 leaves room without hiding a wrong texel (the smallest texel step is 1/255, and a
# wrong neighbour at a weight near zero is caught by the exact tap check).
RGBA_TOL = 2e-6

# (width, height)
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (2, 3), (3, 5), (5, 3), (64, 64), (127, 129), (256, 1), (1, 256), (1000, 3), (4096, 4096)]
SAMPLERS = [(au, av, flt) for au in (WRAP, MIRROR, CLAMP) for av in (WRAP, MIRROR, CLAMP) for flt in (POINT, LINEAR)]
# (rotation, offset, scale) of KHR_texture_transform
TRANSFORMS = [
    (0.0, (0.0, 0.0), (1.0, 1.0)),                       # identity
    (0.0, (0.25, -0.375), (1.0, 1.0)),                   # offsets, one negative
    (0.0, (-3.5, 7.25), (1.0, 1.0)),
    (0.0, (0.5, 0.25), (0.0, 0.0)),                      # scale 0: one texel coordinate whatever the UV
    (0.0, (0.0, 0.0), (-1.0, -2.5)),                     # negative scales
    (0.0, (0.125, 0.0), (1.0e4, 1.0e4)),                 # 1e4
    (0.7, (0.1, 0.2), (1.5, 0.75)),                      # rotation
    (4 * math.pi + 0.3, (0.0, 0.0), (1.0, 1.0)),         # two full turns and a bit
    (6 * math.pi, (-0.5, 0.5), (2.0, 1.0)),              # three full turns
    (-2 * math.pi - 1.1, (0.0, -1.0), (1.0, -1.0)),
]
TRIO_SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 3), (64, 64), (127, 129), (256, 1)]
SEAM_SIZES = [(7, 1), (5, 3), (3, 5), (127, 129), (1000, 3)]      # WRAP seam reload needs width >= 3
TRIO_SLOT = {16: 1, 17: 0, 18: 2, 19: 4}                          # hook slot 16..19 -> the material slot it filters
WAVE = 64


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def _hook(L):
    f = hooks.lib().pt_debug_sample_texture
    return f


def gpu_sample(r, unit, mat_slot, tc):
    n = len(tc)
    out = np.zeros((n, 4), f32)
    taps = np.zeros((n, 5), np.int32)
    ms = np.ascontiguousarray(mat_slot, np.uint32)
    tc = np.ascontiguousarray(tc, f32)
    rc = _hook(r.L)(r.h, unit, ms.ctypes.data, tc.ctypes.data, n, out.ctypes.data, taps.ctypes.data)
    assert rc == 0, rc
    return out, taps


# ---------------------------------------------------------------- float64 statement of SampleLevel(s, uv, 0): tests/texture_ref.py
class Binding:
    """One bound material slot: texture + sampler + UV transform + UV set."""
    def __init__(self, tex, smp, xf, tex_coord):
        self.tex, self.smp, self.xf, self.tex_coord = tex, smp, xf, tex_coord


def reference(textures, bindings, bidx, tc):
    """Float64 SampleLevel(..., 0) for each query (binding index bidx[q], UVs tc[q]), through texture_ref.sample_level0.  Returns rgba
    (n, 4) float64, taps (n, 4) = i0, i1, j0, j1, and per-query flags."""
    n = len(bidx)
    rgba = np.zeros((n, 4), np.float64)
    taps = np.zeros((n, 4), np.int64)
    flags = dict(nonfinite=np.zeros(n, bool), clamped=np.zeros(n, bool), unit_weights=np.zeros(n, bool), linear=np.zeros(n, bool))
    for b in np.unique(bidx):
        q = np.nonzero(bidx == b)[0]
        B = bindings[b]
        data, srgb = textures[B.tex]
        uv = tc[q][:, 2:4] if B.tex_coord else tc[q][:, 0:2]
        rgba[q], taps[q], fl = sample_level0(data, srgb, SAMPLERS[B.smp], transform_rows(*TRANSFORMS[B.xf]), uv)
        for k in flags:
            flags[k][q] = fl[k]
    return rgba, taps, flags


# ---------------------------------------------------------------- coordinates
def axis_values(N, rng):
    """Texel-space classes of one axis of an N-texel texture, as fp32 normalised coordinates."""
    N32 = f32(N)
    ks = sorted({0, 1, N - 1, N, max(N - 2, 0)} | set(rng.integers(0, N + 1, 3).tolist()))
    vals = []
    for k in ks:
        c = f32(k) / N32                                                  # exact texel border k / N ...
        vals += [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]    # ... and the ulps either side
        vals.append((f32(k) + f32(0.5)) / N32)                            # texel centre
        vals.append((f32(k) + f32(0.25)) / N32)
    for p in (1.0, 2.0, 1e3, 1e6):                                        # wrap / mirror periods, both signs
        for s in (1, -1):
            c = f32(s * p)
            vals += [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf)), c + f32(0.5) / N32, c - f32(0.75) / N32]
    lim = f32(1e9) / N32                                                  # the +-1e9-texel clamp
    for s in (1, -1):
        vals += [f32(s) * lim, f32(s) * lim * f32(1 - 2 ** -20), f32(s) * lim * f32(1 + 2 ** -20), f32(s) * lim * f32(3)]
    vals += [f32(0.0), f32(-0.0), f32(1e-40), f32(-1e-45), f32(np.inf), f32(-np.inf), f32(np.nan)]
    vals += list(rng.uniform(-3, 3, 6).astype(f32))
    return np.array(vals, f32)


def binding_queries(B, size, rng):
    """UV pairs for one binding: each class of u against random v and vice versa, plus every special value in each component."""
    W, H = size
    us, vs = axis_values(W, rng), axis_values(H, rng)
    uv = np.concatenate([np.stack([us, rng.choice(vs, len(us))], 1), np.stack([rng.choice(us, len(vs)), vs], 1)])
    sp = np.array([0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan], f32)
    uv = np.concatenate([uv, np.stack([sp, np.full(len(sp), f32(0.3))], 1), np.stack([np.full(len(sp), f32(0.6)), sp], 1)])
    return place_uv(B, uv, rng)


def place_uv(B, uv, rng):
    """(n, 4) tc0.xy, tc1.xy with the designed UVs in the binding's set and different values in the other."""
    other = rng.uniform(-2, 2, uv.shape).astype(f32) + f32(0.37)
    return np.concatenate([other, uv], 1) if B.tex_coord else np.concatenate([uv, other], 1)


def seam_waves(B, size, rng):
    """64-lane waves over one WRAP-u linear binding: no lane, exactly lane 0 / 31 / 63, or every lane on the seam i0 = width - 1."""
    W, H = size
    def lanes(seam):
        r = rng.uniform(0.01, 0.99, WAVE)
        col = np.where(seam, (W - 1) + 0.5 + r, rng.integers(0, W - 1, WAVE) + 0.5 + r)     # x - 0.5 = column + fraction
        u = (col / W).astype(f32) + f32(rng.integers(-2, 3))
        v = rng.uniform(0, 1, WAVE).astype(f32)
        return np.stack([u, v], 1)
    waves = []
    for pick in ([], [0], [31], [63], list(range(WAVE))):
        seam = np.zeros(WAVE, bool); seam[pick] = True
        waves.append(place_uv(B, lanes(seam), rng))
    return waves


# ---------------------------------------------------------------- the scene: textures, samplers, material tables
class Bench:
    def __init__(self, r, o, rng):
        self.r, self.o = r, o
        self.textures = []                  # (rgba8 array (H, W, 4), srgb)
        self.gpu_tex, self.orc_tex = [], []
        self.gpu_smp = [r.sampler_create(au, av, flt, flt) for au, av, flt in SAMPLERS]
        self.orc_smp = [o.sampler_create(au, av, flt, flt) for au, av, flt in SAMPLERS]
        self.bindings = []

    def texture(self, data, srgb):
        self.textures.append((data, srgb))
        self.gpu_tex.append(self.r.texture_create(data, srgb))
        self.orc_tex.append(self.o.texture_create(data, srgb))
        return len(self.textures) - 1

    def bind(self, tex, smp, xf, tex_coord):
        self.bindings.append(Binding(tex, smp, xf, tex_coord))
        return len(self.bindings) - 1

    def materials(self, table, handles_of):
        """PtMaterial records for the renderer (handles_of = gpu) or the oracle; table: list of {slot: binding index}."""
        tex_h, smp_h = handles_of
        out = []
        names = ["normal", "albedo", "metallic_roughness", "occlusion", "emissive", "specular", "specular_color", "clearcoat",
                 "clearcoat_roughness", "clearcoat_normal", "anisotropy", "sheen_color", "sheen_roughness", "transmission", "thickness"]
        for slots in table:
            m = abi.PtMaterial.default()
            for k, name in enumerate(names):
                ts = getattr(m, name)
                if k in slots:
                    B = self.bindings[slots[k]]
                    rot, off, sc = TRANSFORMS[B.xf]
                    ts.descriptor, ts.sampler, ts.tex_coord, ts.rotation = tex_h[B.tex], smp_h[B.smp], B.tex_coord, rot
                    ts.offset[:] = off; ts.scale[:] = sc
                else:
                    ts.descriptor = -1
            out.append(m)
        return out


def random_texture(rng, size):
    W, H = size
    return rng.integers(0, 256, (H, W, 4), dtype=np.uint8)


def run_table(bench, table, mat_slot, tc, monkeypatch, expect_counts=None):
    """Every query on both kernel builds with the interleaved copy on and off; returns the RGBA / taps of the first run and checks
    that the other three are bit-identical to it, and the wall time of the hook calls."""
    r = bench.r
    runs, seconds = [], 0.0
    for env in (None, "0"):
        if env is None: monkeypatch.delenv("MIPT_TEXTURE_INTERLEAVE", raising=False)
        else: monkeypatch.setenv("MIPT_TEXTURE_INTERLEAVE", env)
        r.set_materials(bench.materials(table, (bench.gpu_tex, bench.gpu_smp)))
        counts = (hooks.lib().pt_debug_interleaved_materials(r.h), hooks.lib().pt_debug_interleaved_emissive(r.h))
        if expect_counts is not None:
            assert counts == (expect_counts if env is None else (0, 0)), (env, counts, expect_counts)
        for unit in (0, 1):
            t0 = time.perf_counter()
            runs.append(gpu_sample(r, unit, mat_slot, tc))
            seconds += time.perf_counter() - t0
    monkeypatch.delenv("MIPT_TEXTURE_INTERLEAVE", raising=False)
    rgba, taps = runs[0]
    for k, (o, t) in enumerate(runs[1:], 1):
        bad = np.nonzero((o.view(np.uint32) != rgba.view(np.uint32)).any(1))[0]
        assert len(bad) == 0, "run %d (interleave %s, unit %d) differs from run 0 in %d queries, first %s: %s vs %s" % (
            k, "off" if k >= 2 else "on", k % 2, len(bad), mat_slot[bad[0]], o[bad[0]], rgba[bad[0]])
        assert np.array_equal(t, taps), "run %d: taps differ" % k
    return rgba, taps, seconds


def check(bench, table, mat_slot, tc, rgba, taps, what):
    """Taps exact, RGBA within RGBA_TOL of the float64 statement and bit-identical to the oracle.  Returns the coverage flags."""
    ref_slot = np.array([TRIO_SLOT.get(int(s), int(s)) for s in mat_slot[:, 1]])
    bidx = np.array([table[m][s] for m, s in zip(mat_slot[:, 0].tolist(), ref_slot.tolist())])
    ref, ref_taps, flags = reference(bench.textures, bench.bindings, bidx, tc)
    bad = np.nonzero((taps[:, :4] != ref_taps).any(1))[0]
    assert len(bad) == 0, "%s: %d queries use other texels than SampleLevel, first: query %d %s binding %s tc %s -> %s, expected %s" % (
        what, len(bad), bad[0], mat_slot[bad[0]], vars(bench.bindings[bidx[bad[0]]]), tc[bad[0]], taps[bad[0]], ref_taps[bad[0]])
    err = np.abs(rgba.astype(np.float64) - ref).max(1)
    bad = np.nonzero(~(err <= RGBA_TOL))[0]
    assert len(bad) == 0, "%s: %d queries off the float64 sampler by > %g, worst %g at query %d %s tc %s: %s vs %s" % (
        what, len(bad), RGBA_TOL, err.max(), bad[0], mat_slot[bad[0]], tc[bad[0]], rgba[bad[0]], ref[bad[0]])
    bench.o.set_materials(bench.materials(table, (bench.orc_tex, bench.orc_smp)))
    orc = bench.o.sample_material_slot(mat_slot[:, 0], ref_slot, tc)
    bad = np.nonzero((orc.view(np.uint32) != rgba.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, "%s: %d queries not bit-identical to the oracle, first query %d %s tc %s: %r vs %r" % (
        what, len(bad), bad[0], mat_slot[bad[0]], tc[bad[0]], rgba[bad[0]].tolist(), orc[bad[0]].tolist())
    # Both texels of a row come from one 8-byte load at column ia.  It must hold i0 and stay inside the row (ia + 1 < width; a
    # width-1 texture reads its one texel and the allocation's 4-byte pad): ia = clamp(i0, 0, width - 2), exactly.
    W = np.array([bench.textures[bench.bindings[b].tex][0].shape[1] for b in bidx])
    ia = np.clip(ref_taps[:, 0], 0, np.maximum(W - 2, 0))
    bad = np.nonzero(taps[:, 4] != ia)[0]
    assert len(bad) == 0, "%s: %d queries load their texel pair at another column than clamp(i0, 0, width - 2), first query %d %s width %d: %s" % (
        what, len(bad), bad[0], mat_slot[bad[0]], W[bad[0]], taps[bad[0]])
    flags["seam_reload"] = flags["linear"] & (taps[:, 1] != ia) & (taps[:, 1] != ia + 1)
    return flags


def pad_waves(ms, tc):
    """Pad a query list to whole waves with copies of its first query, so that wave-shaped blocks appended after it stay aligned."""
    k = (-len(ms)) % WAVE
    return np.concatenate([ms, np.repeat(ms[:1], k, 0)]), np.concatenate([tc, np.repeat(tc[:1], k, 0)])


# ---------------------------------------------------------------- tests
@pytest.mark.gpu
def test_sampler_matches_float64_sampleLevel_and_oracle_query_by_query(R, oracle_lib, monkeypatch):
    """All sizes x sRGB / linear x the nine address-mode pairs x point / linear x ten UV transforms x both UV sets, each material slot
    0..14 through sample_slot, plus WRAP-seam waves; then the interleaved-footprint table through get_surface's fetch (slots 16..19)."""
    rng = np.random.default_rng(20261015)
    r = R()
    o = oracle_lib.Oracle()
    bench = Bench(r, o, rng)
    try:
        tex_of = {}
        for size in SIZES:
            for srgb in (False, True):
                tex_of[size, srgb] = bench.texture(random_texture(rng, size), srgb)
        totals = {}
        queries = 0
        gpu_seconds = 0.0

        def account(flags, n):
            nonlocal queries
            queries += n
            for k, v in flags.items():
                totals[k] = totals.get(k, 0) + int(v.sum())

        # --- table 1: every (texture, sampler) pair under the identity and one other transform, 15 bindings a material
        slots = []
        k = 0
        for (size, srgb), t in tex_of.items():
            for s in range(len(SAMPLERS)):
                for xf in (0, 1 + k % (len(TRANSFORMS) - 1)):
                    slots.append((bench.bind(t, s, xf, (k + xf) % 2), size))
                k += 1
        table = [dict() for _ in range((len(slots) + 14) // 15)]
        where = []
        for n, (b, size) in enumerate(slots):
            table[n // 15][n % 15] = b
            where.append((n // 15, n % 15, size))
        ms_list, tc_list = [], []
        for (m, s, size), (b, _) in zip(where, slots):
            tc = binding_queries(bench.bindings[b], size, rng)
            ms_list.append(np.tile([m, s], (len(tc), 1))); tc_list.append(tc)
        ms, tc = np.concatenate(ms_list).astype(np.uint32), np.concatenate(tc_list)
        perm = rng.permutation(len(ms))                          # waves mixing materials, slots, sizes and samplers
        ms, tc = pad_waves(ms[perm], tc[perm])
        # seam waves: WRAP-u linear samplers, identity transform
        for (m, s, size), (b, _) in zip(where, slots):
            B = bench.bindings[b]
            if size in SEAM_SIZES and SAMPLERS[B.smp][0] == WRAP and SAMPLERS[B.smp][2] == LINEAR and B.xf == 0:
                for w in seam_waves(B, size, rng):
                    ms = np.concatenate([ms, np.tile(np.array([m, s], np.uint32), (WAVE, 1))]); tc = np.concatenate([tc, w])
        assert len(table) <= 96                                  # the wavefront build keeps the whole table in LDS
        rgba, taps, sec = run_table(bench, table, ms, tc, monkeypatch)
        gpu_seconds += sec
        account(check(bench, table, ms, tc, rgba, taps, "slots 0..14"), len(ms))

        # --- table 2: interleaved footprints (RM_TRIO) next to general-path twins, read as get_surface reads them
        roles = {}
        for size in TRIO_SIZES:
            for role in "ANME":
                for srgb in (False, True):
                    roles[size, role, srgb] = bench.texture(random_texture(rng, size), srgb)
        variants = []                                            # (normal bound, mr bound, emissive: None / "same" / "moved", sN, sM, sE)
        for bn, bm in ((True, False), (False, True), (True, True)):
            for em in (None, "same", "same_srgb"):
                for sn in ((False, True) if bn else (False,)):
                    for sm in ((False, True) if bm else (False,)):
                        variants.append((bn, bm, em, sn, sm))
        variants.append((True, True, "moved", True, False))      # emissive differs only in its transform: fetched on its own
        trio_table, trio_expect, twins = [], [0, 0], []
        seam_mats = []

        def trio_material(v, size, smp, xf, tc_set, albedo_srgb):
            bn, bm, em, sn, sm = v
            d = {1: bench.bind(roles[size, "A", albedo_srgb], smp, xf, tc_set)}
            if bn: d[0] = bench.bind(roles[size, "N", sn], smp, xf, tc_set)
            if bm: d[2] = bench.bind(roles[size, "M", sm], smp, xf, tc_set)
            if em == "moved": d[4] = bench.bind(roles[size, "E", True], smp, (xf + 1) % len(TRANSFORMS), tc_set)
            elif em: d[4] = bench.bind(roles[size, "E", em == "same_srgb"], smp, xf, tc_set)
            return d

        for i, v in enumerate(variants):
            size = TRIO_SIZES[i % len(TRIO_SIZES)]
            smp, xf = (7 * i + 3) % len(SAMPLERS), i % len(TRANSFORMS)
            d = trio_material(v, size, smp, xf, i % 2, i % 3 == 0)
            trio_table.append(d)
            trio_expect[0] += 1; trio_expect[1] += 1 if v[2] in ("same", "same_srgb") else 0
            twin = dict(d)                                       # the same textures, the normal / metal-rough footprint moved
            moved = 0 if 0 in d else 2
            B = bench.bindings[d[moved]]
            twin[moved] = bench.bind(B.tex, B.smp, (B.xf + 3) % len(TRANSFORMS), B.tex_coord)
            twins.append(twin)
        for size in [z for z in TRIO_SIZES if z[0] >= 3]:        # WRAP / linear footprints for the interleaved seam reload
            smp = SAMPLERS.index((WRAP, WRAP, LINEAR))
            d = trio_material((True, True, "same", True, False), size, smp, 0, 0, True)
            seam_mats.append((len(trio_table), size)); trio_table.append(d)
            trio_expect[0] += 1; trio_expect[1] += 1
        table2 = trio_table + twins
        n_trio = len(trio_table)
        assert len(table2) <= 96

        def mat_queries(m, slot_set):
            d = table2[m]
            size = bench.textures[bench.bindings[d[1]].tex][0].shape[1::-1]
            out_ms, out_tc = [], []
            for s in slot_set:
                if TRIO_SLOT.get(s, s) not in d: continue
                tcq = binding_queries(bench.bindings[d[TRIO_SLOT.get(s, s)]], tuple(size), rng)
                out_ms.append(np.tile([m, s], (len(tcq), 1))); out_tc.append(tcq)
            return np.concatenate(out_ms), np.concatenate(out_tc)

        # lane by lane: interleaved material, general twin, interleaved, ...
        ms_a, tc_a, ms_b, tc_b = [], [], [], []
        for i in range(len(variants)):
            a = mat_queries(i, (16, 17, 18, 19)); b = mat_queries(n_trio + i, (16, 17, 18, 19))
            ms_a.append(a[0]); tc_a.append(a[1]); ms_b.append(b[0]); tc_b.append(b[1])
        ms_a, tc_a, ms_b, tc_b = map(np.concatenate, (ms_a, tc_a, ms_b, tc_b))
        n = min(len(ms_a), len(ms_b))
        ms2 = np.empty((2 * n, 2), np.uint32); tc2 = np.empty((2 * n, 4), f32)
        ms2[0::2], ms2[1::2], tc2[0::2], tc2[1::2] = ms_a[:n], ms_b[:n], tc_a[:n], tc_b[:n]
        # every material and slot, 0..14 and 16..19, shuffled: waves mixing slots, paths and footprints
        mix = [mat_queries(m, (0, 1, 2, 4, 16, 17, 18, 19)) for m in range(len(table2))]
        ms_m, tc_m = np.concatenate([a for a, _ in mix]), np.concatenate([b for _, b in mix])
        perm = rng.permutation(len(ms_m))
        ms2, tc2 = pad_waves(np.concatenate([ms2, ms_m[perm].astype(np.uint32)]), np.concatenate([tc2, tc_m[perm]]))
        for m, size in seam_mats:
            for s in (16, 17, 18, 19):
                for w in seam_waves(bench.bindings[table2[m][1]], size, rng):
                    ms2 = np.concatenate([ms2, np.tile(np.array([m, s], np.uint32), (WAVE, 1))]); tc2 = np.concatenate([tc2, w])
        rgba, taps, sec = run_table(bench, table2, ms2, tc2, monkeypatch, expect_counts=tuple(trio_expect))
        gpu_seconds += sec
        account(check(bench, table2, ms2, tc2, rgba, taps, "interleaved table"), len(ms2))

        print("\ntexture sampler: %d queries x 4 runs, hook wall time %.2f s; coverage %s" % (queries, gpu_seconds, totals))
        for k in ("seam_reload", "unit_weights", "nonfinite", "clamped"):
            assert totals[k] > 0, (k, totals)
        assert queries >= 100000, queries
    finally:
        r.close()


@pytest.mark.gpu
def test_sample_texture_hook_rejects_bad_arguments(R):
    """Argument errors come back as error codes; no query reaches the device."""
    r = R()
    try:
        t = r.texture_create(np.full((2, 2, 4), 200, np.uint8), False)
        smp = r.sampler_create(WRAP, WRAP, LINEAR, LINEAR)
        m = abi.PtMaterial.default()
        for name in ("normal", "albedo", "metallic_roughness", "occlusion", "emissive", "specular", "specular_color", "clearcoat",
                     "clearcoat_roughness", "clearcoat_normal", "anisotropy", "sheen_color", "sheen_roughness", "transmission", "thickness"):
            getattr(m, name).descriptor = -1
        m.albedo.descriptor, m.albedo.sampler = t, smp
        r.set_materials([m])
        f = _hook(r.L)
        tc = np.zeros((1, 4), f32); out = np.zeros((1, 4), f32)
        for ms in ([1, 1], [0, 15], [0, 20], [0, 0xffffffff]):
            a = np.array(ms, np.uint32)
            assert f(r.h, 0, a.ctypes.data, tc.ctypes.data, 1, out.ctypes.data, None) != 0, ms
        a = np.array([0, 1], np.uint32)
        assert f(None, 0, a.ctypes.data, tc.ctypes.data, 1, out.ctypes.data, None) != 0
        assert f(r.h, 2, a.ctypes.data, tc.ctypes.data, 1, out.ctypes.data, None) != 0
        assert f(r.h, 0, None, tc.ctypes.data, 1, out.ctypes.data, None) != 0
        assert f(r.h, 1, a.ctypes.data, tc.ctypes.data, 1, out.ctypes.data, None) == 0       # taps may be null
        assert np.allclose(out[0], 200 / 255, atol=1e-6), out
    finally:
        r.close()


def test_oracle_material_slot_export_gives_the_sampling_rules_values(oracle_lib):
    """orc_sample_material_slot = SampleTexture of a material slot: through an identity transform it gives what orc_sample_texture
    gives (test_oracle_kat.py::test_texture_sampling_rules' values), on both UV sets, and white for an unbound slot."""
    o = oracle_lib.Oracle()
    ramp = np.zeros((2, 4, 4), np.uint8)
    ramp[..., 0] = np.array([0, 85, 170, 255])[None, :]
    ramp[1, :, 1] = 255
    ramp[..., 3] = 255
    t_lin, t_srgb = o.texture_create(ramp, False), o.texture_create(ramp, True)
    s_clamp = o.sampler_create(CLAMP, CLAMP, LINEAR, LINEAR)
    s_mirror = o.sampler_create(MIRROR, MIRROR, LINEAR, LINEAR)
    s_point = o.sampler_create(WRAP, WRAP, POINT, POINT)
    s_wrap = o.sampler_create(WRAP, WRAP, LINEAR, LINEAR)
    m = abi.PtMaterial.default()
    names = ["normal", "albedo", "metallic_roughness", "occlusion", "emissive", "specular", "specular_color", "clearcoat",
             "clearcoat_roughness", "clearcoat_normal", "anisotropy", "sheen_color", "sheen_roughness", "transmission", "thickness"]
    combos = [(t_lin, s_wrap), (t_lin, s_clamp), (t_lin, s_mirror), (t_lin, s_point), (t_srgb, s_wrap)]
    for k, name in enumerate(names):
        ts = getattr(m, name)
        ts.descriptor = -1
        if k < 2 * len(combos):
            ts.descriptor, ts.sampler = combos[k % len(combos)]; ts.tex_coord = k // len(combos)
            ts.rotation = 0.0; ts.offset[:] = (0, 0); ts.scale[:] = (1, 1)
    o.set_materials([m])
    L = oracle_lib.lib()

    def tap(tex, smp, u, v):
        uv = np.array([u, v], f32); out = np.zeros(4, f32)
        L.orc_sample_texture(o.h, tex, smp, uv.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out
    for u, v in [(0.125, 0.25), (0.5, 0.25), (0.0, 0.25), (1.125, 0.25), (7.0, 0.25), (0.49, 0.25), (1.3, 0.25), (0.125, 0.5), (0.625, 0.25)]:
        for k in range(2 * len(combos)):
            tex, smp = combos[k % len(combos)]
            tc = [u, v, 9.0, -9.0] if k < len(combos) else [-9.0, 9.0, u, v]
            got = o.sample_material_slot(0, k, tc)
            assert np.array_equal(got, tap(tex, smp, u, v)), (k, u, v, got)
    assert abs(o.sample_material_slot(0, 0, [0.5, 0.25, 0, 0])[0] - 0.5 * (85 + 170) / 255) < 1e-6
    assert abs(o.sample_material_slot(0, 1, [7.0, 0.25, 0, 0])[0] - 1.0) < 1e-6
    assert abs(o.sample_material_slot(0, 3, [1.3, 0.25, 0, 0])[0] - 85 / 255) < 1e-6
    assert np.array_equal(o.sample_material_slot(0, 14, [0.5, 0.5, 0.5, 0.5]), np.ones(4, f32))
