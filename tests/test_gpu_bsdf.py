"""The material model and the punctual lights (pt_shading.h: gltf_bsdf, lobe_probabilities, bsdf_pdf, evaluate_bsdf, sample_bsdf, the
sheen helpers, stage_lights / load_light / light_ray), query by query, through the test hooks pt_debug_bsdf_query and pt_debug_light_query
on both kernel builds:
  unit 0  the wavefront build: the sheen table and the first 32 lights staged into LDS as the shade stage stages them (the spot cone terms
          precomputed into the staged copy);
  unit 1  the megakernel build: tables in global memory, cone terms computed in place.

Every query is checked
  A  against the CPU oracle's EvaluateBsdf / SampleBsdf / LayerProbabilities / GetLightRay (orc_bsdf_query_many, orc_light_query_many):
     every output float bit-identical, NaN positions included (payloads are not compared); no tolerance;
  B  unit 0 against unit 1: bit-identical;
  C  where a test says so, against the float64 restatement of tests/bsdf_ref.py, with the thresholds of its _check (the ones
     tests/test_oracle_independent.py holds the oracle to) and, for the lights, a bound derived from the float32 operation count
     (bsdf_ref.light_ray_bound).

Query i of a BSDF call runs in lane i % 64 of wave i / 64 (the hook's contract), so the tests compose waves by ordering the queries: the
sheen lobe of gltf_bsdf is run or skipped by a vote of the wave's active lanes.

What this does NOT show: the hooks compile the same source functions in the same translation units with the same flags as the shade
kernels, but they are not the machine code of the specialised k_wf_shade copies or of pt_megakernel.  The image-parity tests and the
kernel-copy-selection tests (test_gpu_tables.py) remain the check on those copies.

The tests at the end that carry no gpu mark run the same query sets on the oracle alone: the _many exports against the single-query
exports, the float64 light_ray against orc_light_ray, and the non-vacuity conditions of every query set (so the seeds are proven without
a GPU)."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import hooks

import bsdf_ref as B

f32 = np.float32
u32 = np.uint32
EVALUATE, SAMPLE = 0, 1
MIS, WHITE = abi.FLAG_MATERIAL_MIS, abi.FLAG_MATERIAL_DIFFUSE_WHITE
MODES = [("non-MIS", 0), ("MIS", MIS), ("white", WHITE)]
LAYERS = ["alpha", "clearcoat", "sheen", "specular", "diffuse", "transmission"]          # the order of the hook's outputs [9, 15)
ONE_BELOW = np.nextafter(f32(1), f32(0))                                                 # 1 - 2^-24

# Non-vacuity, stated once and asserted on the ORACLE's outputs (so that the CPU tests at the end prove the seeds):
MIN_REFLECTIVE_SHARE = 0.6        # of the reflective EVALUATE queries have a value above 1e-3
MIN_TRANSMISSION = 100            # transmission EVALUATE queries with a value above 1e-4
MIN_PER_LAYER = 100               # SAMPLE queries that chose each of the six layers
MAX_NON_FINITE = 0.001            # share of non-finite output floats


# ---------------------------------------------------------------- hooks
@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


@pytest.fixture(scope="module")
def gpu(R, oracle_lib):
    r = R()
    o = oracle_lib.Oracle()
    yield r, o
    r.close(); o.close()


def gpu_bsdf(r, unit, op, flags, q):
    q = np.ascontiguousarray(q, f32)
    assert q.ndim == 2 and q.shape[1] == 48
    out = np.full((len(q), 16), 7.0, f32)                                  # the hook writes all 16
    rc = hooks.lib().pt_debug_bsdf_query(r.h, unit, op, flags, q.ctypes.data, len(q), out.ctypes.data)
    assert rc == 0, rc
    return out


def gpu_lights(r, unit, small, n_lights, index, p):
    index = np.ascontiguousarray(index, u32); p = np.ascontiguousarray(p, f32)
    out = np.full((len(index), 8), 7.0, f32)
    rc = hooks.lib().pt_debug_light_query(r.h, unit, small, n_lights, index.ctypes.data, p.ctypes.data, len(index), out.ctypes.data)
    assert rc == 0, rc
    return out


def same_bits(a, b):
    """Bit-identical, except that any NaN equals any NaN."""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    return (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))


def check_ab(name, r, o, op, flags, q):
    """A and B on the queries q; returns the oracle's outputs."""
    want = o.bsdf_query_many(op, flags, q)
    g0 = gpu_bsdf(r, 0, op, flags, q)
    g1 = gpu_bsdf(r, 1, op, flags, q)
    bad_a = ~same_bits(g0, want).all(axis=1)
    bad_b = ~same_bits(g0, g1).all(axis=1)
    print("%s: %d queries, %d differ from the oracle, %d between the units, %d non-finite floats" %
          (name, len(q), int(bad_a.sum()), int(bad_b.sum()), int((~np.isfinite(want)).sum())))
    if bad_a.any():
        i = int(np.flatnonzero(bad_a)[0])
        raise AssertionError("%s: query %d of %d differs from the oracle\n in   %r\n gpu  %r\n want %r" % (name, i, int(bad_a.sum()), q[i], g0[i], want[i]))
    if bad_b.any():
        i = int(np.flatnonzero(bad_b)[0])
        raise AssertionError("%s: query %d: unit 0 %r, unit 1 %r" % (name, i, g0[i], g1[i]))
    return want


class OracleOnly:
    """check_ab's stand-in for the CPU tests: the oracle's outputs, nothing to compare."""
    def __init__(self, o): self.o = o
    def __call__(self, name, op, flags, q): return self.o.bsdf_query_many(op, flags, q)


class OnGpu:
    def __init__(self, r, o): self.r, self.o = r, o
    def __call__(self, name, op, flags, q): return check_ab(name, self.r, self.o, op, flags, q)


# ---------------------------------------------------------------- float32 helpers
def select_layer(ux, probs):
    """SelectBsdf in float32 (the subtraction chain of sample_bsdf): index into LAYERS for each query."""
    x = np.asarray(ux, f32).copy()
    p = np.asarray(probs, f32)
    layer = np.full(len(x), -1)
    for k, col in [(0, 0), (1, 1), (2, 2), (3, 3), (5, 5)]:                # alpha, clearcoat, sheen, specular, transmission; else diffuse
        hit = (layer < 0) & (x <= p[:, col])
        layer[hit] = k
        x = (x - p[:, col]).astype(f32)
    layer[layer < 0] = 4
    return layer


def lobe_edges(probs):
    """The five cumulative edges, accumulated in float32 in the order sample_bsdf subtracts them: alpha, + clearcoat, + sheen, + specular,
    + transmission."""
    p = np.asarray(probs, f32)
    e, acc = [], np.zeros(len(p), f32)
    for col in (0, 1, 2, 3, 5):
        acc = (acc + p[:, col]).astype(f32)
        e.append(acc.copy())
    return np.stack(e, axis=1)


def u_inside_layers(rng, probs, target):
    """u.x inside the interval of layer target[i] (an index into LAYERS) where that layer has one, else uniform."""
    p = np.asarray(probs, np.float64)
    order = [0, 1, 2, 3, 5, 4]                                              # the intervals' order along u.x
    lo = np.zeros(len(p)); ux = rng.random(len(p))
    for k in order:
        hi = lo + p[:, k]
        pick = (target == k) & (p[:, k] > 1e-3)
        ux[pick] = (lo + (0.2 + 0.6 * rng.random(len(p))) * (hi - lo))[pick]
        lo = hi
    return ux.astype(f32)


def tilted(rng, n, lo_deg, hi_deg):
    """Unit vectors lo..hi degrees away from the unit vectors n, float32."""
    k = len(n)
    t = B.nrm(np.cross(n, B.nrm(rng.normal(size=(k, 3)))))
    a = np.radians(rng.uniform(lo_deg, hi_deg, k))[:, None]
    return B.nrm(np.cos(a) * n + np.sin(a) * t).astype(f32)


def ulps(x, k):
    """x moved k float32 ulps (k an int array or scalar)."""
    x = np.asarray(x, f32)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i) + k                           # a monotone integer line through +-0
    i = np.where(i < 0, (-i) | 0x80000000, i)
    return i.astype(np.uint32).view(f32)


# ---------------------------------------------------------------- query set 1: random surfaces
N_RANDOM = 3000
SEED_RANDOM = 211


def random_set():
    rng = np.random.default_rng(SEED_RANDOM)
    sp = B.random_surfaces(rng, N_RANDOM)
    v, l, through = B.directions(rng, sp, N_RANDOM, 0.4)
    ng_tilt = tilted(rng, sp["shading_normal"], 20, 80)
    u = rng.random((N_RANDOM, 3)).astype(f32)
    return sp, v, l, through, ng_tilt, u


def run_random_set(run):
    sp, v, l, through, ng_tilt, u = random_set()
    s36 = B.pack36_all(sp)
    n = sp["shading_normal"]
    q_same, q_tilt, q_sample = B.pack48(s36, n, v, l), B.pack48(s36, ng_tilt, v, l), B.pack48(s36, n, v, u)
    out = {}
    for mode, flags in MODES:
        out["same", mode] = run("random EVALUATE ng = n, " + mode, EVALUATE, flags, q_same)
        out["tilt", mode] = run("random EVALUATE ng tilted, " + mode, EVALUATE, flags, q_tilt)
        out["sample", mode] = run("random SAMPLE, " + mode, SAMPLE, flags, q_sample)
    # ---- non-vacuity, on these (the oracle's) outputs
    is_t = B.dot(n, l) * B.dot(n, v) < 0
    assert np.array_equal(is_t, through)
    val = out["same", "MIS"][:, :3].max(axis=1)
    refl_share = float((val[~is_t] > 1e-3).mean()); n_trans = int((val[is_t] > 1e-4).sum())
    is_t_tilt = B.dot(ng_tilt.astype(np.float64), l) * B.dot(ng_tilt.astype(np.float64), v) < 0
    disagree = int((is_t_tilt != is_t).sum())
    layer = select_layer(u[:, 0], out["sample", "MIS"][:, 9:15])
    per_layer = np.bincount(layer, minlength=6)
    nonfinite = float(np.mean([(~np.isfinite(x)).mean() for x in out.values()]))
    print("random set non-vacuity: %.1f %% of %d reflective queries above 1e-3, %d transmission queries above 1e-4, ng decides otherwise than n for %d, "
          "layers chosen %s, %.4f %% non-finite" % (100 * refl_share, int((~is_t).sum()), n_trans, disagree, dict(zip(LAYERS, per_layer.tolist())), 100 * nonfinite))
    assert refl_share >= MIN_REFLECTIVE_SHARE and n_trans >= MIN_TRANSMISSION
    assert disagree >= 300 and (val[is_t_tilt != is_t] > 1e-4).sum() >= 100          # `is_transmission` is decided by ng, and it shows
    assert per_layer.min() >= MIN_PER_LAYER, per_layer
    assert nonfinite <= MAX_NON_FINITE
    # ---- C, for the ng = n EVALUATE queries and the SAMPLE queries
    alpha = sp["alpha"]
    g = out["same", "non-MIS"].astype(np.float64)
    B._check("EVALUATE non-MIS value", g[:, :3], alpha[:, None] * B.gltf_bsdf(sp, v, l))
    B._check("EVALUATE non-MIS pdf", g[:, 3], B.sat(B.dot(n, l)) / B.PI * alpha, 2e-6)
    g = out["same", "MIS"].astype(np.float64)
    p = B.layer_probabilities(sp, v)
    B._check("EVALUATE MIS value", g[:, :3], alpha[:, None] * B.gltf_bsdf(sp, v, l, is_t))
    B._check("EVALUATE MIS pdf", g[:, 3], B.bsdf_pdf(sp, v, l, is_t, p))
    B._check("lobe probabilities", g[:, 9:15], np.stack([p[k] for k in LAYERS], axis=1))
    g = out["same", "white"].astype(np.float64)
    B._check("EVALUATE white value and pdf", g[:, :4], (B.sat(B.dot(n, l)) / B.PI)[:, None] * np.ones(4))
    g = out["sample", "MIS"].astype(np.float64)
    ux = u[:, 0].astype(np.float64)
    edges, margin, smooth = B.sample_masks(sp, p, ux)
    alpha_lobe = ux <= edges[:, 0]
    trans_lobe = (ux > edges[:, 3]) & (ux <= edges[:, 4])
    s_t = g[:, 7] == 1
    assert np.array_equal(s_t[margin], (alpha_lobe | trans_lobe)[margin])
    assert np.array_equal((g[:, 8] == 0)[margin], alpha_lobe[margin])                              # use_mis off only for the alpha lobe
    a = margin & alpha_lobe
    assert a.sum() > 100
    assert np.allclose(g[a, 4:7], -v[a], atol=1e-6) and np.allclose(g[a, 3], p["alpha"][a], atol=1e-6) and np.allclose(g[a, 0], 1 - alpha[a], atol=1e-6)
    b = margin & ~alpha_lobe & np.isfinite(g).all(axis=1) & smooth
    assert b.sum() > 500
    sub = {k: x[b] for k, x in sp.items()}
    pb = {k: x[b] for k, x in p.items()}
    ls = g[b, 4:7]
    B._check("SAMPLE MIS value", g[b, :3], sub["alpha"][:, None] * B.gltf_bsdf(sub, v[b], ls, s_t[b]), 1e-4)
    B._check("SAMPLE MIS pdf", g[b, 3], B.bsdf_pdf(sub, v[b], ls, s_t[b], pb), 1e-4)
    g = out["sample", "non-MIS"].astype(np.float64)
    c = (g[:, 8] == 1) & np.isfinite(g).all(axis=1)                                                # the cosine-sampled ones (u.x <= alpha)
    assert np.array_equal(g[:, 8] == 1, ux <= alpha) and c.sum() > 1500
    sub = {k: x[c] for k, x in sp.items()}
    B._check("SAMPLE non-MIS value", g[c, :3], sub["alpha"][:, None] * B.gltf_bsdf(sub, v[c], g[c, 4:7]), 1e-4)
    B._check("SAMPLE non-MIS pdf", g[c, 3], B.sat(B.dot(n[c], g[c, 4:7])) / B.PI * alpha[c], 1e-4)
    g = out["sample", "white"].astype(np.float64)
    B._check("SAMPLE white value and pdf", g[:, [0, 3]], (B.sat(B.dot(n, g[:, 4:7])) / B.PI)[:, None] * np.ones(2), 1e-4)
    return out


@pytest.mark.gpu
def test_random_surfaces_against_the_oracle_the_other_unit_and_float64(gpu):
    run_random_set(OnGpu(*gpu))


# ---------------------------------------------------------------- query set 2: independence from wave neighbours
def neighbour_set(o):
    """577 = 64 * 9 + 1 queries: first 256 surfaces WITHOUT sheen (in order, four waves -- a whole workgroup -- that skip the sheen lobe),
    then surfaces with and without; u.x placed inside each of the six layers in turn."""
    rng = np.random.default_rng(223)
    n = 64 * 9 + 1
    sp = B.random_surfaces(rng, n)
    sp["sheen_color"][:256] = 0.0
    sp["alpha"][::3] = np.asarray(rng.uniform(0.2, 0.8, len(sp["alpha"][::3])), f32)              # an alpha lobe to choose
    v, l, _ = B.directions(rng, sp, n, 0.4)
    s36 = B.pack36_all(sp)
    nn = sp["shading_normal"]
    probs = o.bsdf_query_many(EVALUATE, MIS, B.pack48(s36, nn, v, l))[:, 9:15]
    u = rng.random((n, 3)).astype(f32)
    u[:, 0] = u_inside_layers(rng, probs, np.arange(n) % 6)
    has_sheen = (sp["sheen_color"] != 0).any(axis=1)
    layer = select_layer(u[:, 0], probs)
    return B.pack48(s36, nn, v, l), B.pack48(s36, nn, v, u), has_sheen, layer


def check_neighbour_set_covers(has_sheen, layer):
    counts = np.bincount(layer, minlength=6)
    print("neighbour set: %d sheen and %d no-sheen surfaces, layers chosen %s; among the first 256 (no sheen) %s" %
          (int(has_sheen.sum()), int((~has_sheen).sum()), dict(zip(LAYERS, counts.tolist())), np.bincount(layer[:256], minlength=6).tolist()))
    assert not has_sheen[:256].any() and has_sheen[256:].sum() >= 100 and (~has_sheen[256:]).sum() >= 100
    assert counts.min() >= 20, counts
    assert (np.bincount(layer[:256], minlength=6)[[0, 1, 3, 4, 5]] >= 10).all()                    # (no sheen layer without a sheen colour)


@pytest.mark.gpu
def test_a_query_does_not_depend_on_its_wave_neighbours(gpu):
    r, o = gpu
    q_eval, q_sample, has_sheen, layer = neighbour_set(o)
    check_neighbour_set_covers(has_sheen, layer)
    n = len(q_eval)
    perm = np.random.default_rng(5).permutation(n)
    moved = 0
    for name, op, flags, q in [("EVALUATE MIS", EVALUATE, MIS, q_eval), ("EVALUATE non-MIS", EVALUATE, 0, q_eval), ("SAMPLE MIS", SAMPLE, MIS, q_sample),
                               ("SAMPLE non-MIS", SAMPLE, 0, q_sample)]:
        want = check_ab("neighbours, in order, " + name, r, o, op, flags, q)
        for unit in (0, 1):
            base = gpu_bsdf(r, unit, op, flags, q)
            shuffled = gpu_bsdf(r, unit, op, flags, q[perm])
            back = np.empty_like(shuffled); back[perm] = shuffled
            assert same_bits(back, base).all(), (name, unit, "permuted", int((~same_bits(back, base).all(axis=1)).sum()))
            for m in (257, 64 * 3 + 1, 63, 1):                             # a partial last wave; 257: one lane past a workgroup
                part = gpu_bsdf(r, unit, op, flags, q[:m])
                assert same_bits(part, base[:m]).all(), (name, unit, m)
                tail = gpu_bsdf(r, unit, op, flags, q[n - m:])            # ... and the same queries in other lanes
                assert same_bits(tail, base[n - m:]).all(), (name, unit, m, "tail")
            moved += 1
        assert same_bits(want, base).all()
    print("neighbours: %d queries x %d (op, mode, unit) runs: in order, permuted, and prefixes / suffixes of 257, 193, 63 and 1 queries: 0 differ" % (n, moved))


# ---------------------------------------------------------------- query set 3: the sheen shortcut
def sheen_shortcut_set():
    """W0: 64 queries on surfaces WITHOUT sheen; W1: the same with lane 63's surface given a sheen colour.  Returns (s36 of W0, s36 of W1,
    v, l, u), 64 each.  Cases: v = l = n exactly (lanes 0-7), v and l within a few ulp of n (8-31), l = -v (32-35), l below the horizon
    (36-47), the rest ordinary; sheen_roughness_squared 1e-6, 0 and 1 cycle through all of them."""
    rng = np.random.default_rng(227)
    sp = B.random_surfaces(rng, 64)
    sp["sheen_color"][:] = 0.0
    sp["sheen_roughness_squared"] = np.asarray(np.resize([1e-6, 0.0, 1.0, 0.3], 64), f32).astype(np.float64)
    v, l, _ = B.directions(rng, sp, 64, 0.0)
    v = v.astype(f32); l = l.astype(f32)
    n = sp["shading_normal"].astype(f32)
    v[:32] = n[:32]; l[:32] = n[:32]
    k = rng.integers(-3, 4, (24, 3))
    v[8:32] = ulps(n[8:32], k); l[8:32] = ulps(n[8:32], rng.integers(-3, 4, (24, 3)))
    l[32:36] = -v[32:36]
    l[36:48] = (l[36:48] - 2 * B.dot(n[36:48].astype(np.float64), l[36:48].astype(np.float64))[:, None] * n[36:48]).astype(f32)   # mirrored below
    u = rng.random((64, 3)).astype(f32)
    s0 = B.pack36_all(sp)
    s1 = s0.copy()
    s1[63, 26:29] = (0.5, 0.3, 0.2)
    return s0, s1, n, v, l, u


def sheen_shortcut_runs():
    """(name, op, flags, 128 queries: W0 then W1)"""
    s0, s1, n, v, l, u = sheen_shortcut_set()
    with np.errstate(all="ignore"):
        ng_through = (v - l) / np.linalg.norm(v - l, axis=1, keepdims=True)          # dot(ng, v) > 0 > dot(ng, l): is_transmission (NaN where v = l)
    ng_through = np.where(np.isfinite(ng_through), ng_through, n).astype(f32)
    runs = []
    for name, op, flags, ng, a in [("EVALUATE MIS, ng = n", EVALUATE, MIS, n, l), ("EVALUATE MIS, ng makes it transmission", EVALUATE, MIS, ng_through, l),
                                   ("EVALUATE non-MIS", EVALUATE, 0, n, l), ("SAMPLE MIS", SAMPLE, MIS, n, u), ("SAMPLE non-MIS", SAMPLE, 0, n, u)]:
        runs.append((name, op, flags, np.concatenate([B.pack48(s0, ng, v, a), B.pack48(s1, ng, v, a)])))
    return runs


def check_sheen_shortcut_outputs(name, want):
    """Non-vacuity on the oracle's outputs: the no-sheen wave holds NaN values (the shortcut's hand-built NaN case) and finite ones."""
    nan = np.isnan(want[:64, :3]).any(axis=1)
    print("sheen shortcut, %s: %d of the 64 no-sheen queries have a NaN value (lanes %s)" % (name, int(nan.sum()), np.flatnonzero(nan).tolist()))
    assert np.isfinite(want[:64, :3]).all(axis=1).sum() >= 20
    return nan


@pytest.mark.gpu
def test_the_sheen_shortcut_gives_the_bits_of_the_sheen_lobe(gpu):
    r, o = gpu
    nan_from_the_lobe = 0
    for name, op, flags, q in sheen_shortcut_runs():
        want = check_ab("sheen shortcut, " + name, r, o, op, flags, q)
        nan = check_sheen_shortcut_outputs(name, want)
        if name == "EVALUATE MIS, ng = n":
            nan_from_the_lobe = int(nan[:32].sum())
        for unit in (0, 1):
            g = gpu_bsdf(r, unit, op, flags, q)
            assert same_bits(g[64:127], g[:63]).all(), (name, unit)                  # lanes 0..62: with the sheen lobe run = with it skipped
            alone = gpu_bsdf(r, unit, op, flags, q[:64])                              # W0 as the launch's only wave
            assert same_bits(alone, g[:64]).all(), (name, unit)
    assert nan_from_the_lobe >= 3                                                    # h.n rounds above 1 for some of v, l = n +- ulps: pow of a negative base


SHEEN_COLOURS = [(0.3, 0.0, 0.0), (0.0, 0.0, 0.7), (-0.0, -0.0, -0.0), (-0.0, 0.0, 0.0), (-0.5, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -0.25),
                 (-0.5, 0.25, 0.0)]


def sheen_colour_set():
    """One wave of 64 queries per colour of SHEEN_COLOURS (so the wave's vote is that colour's alone), then all of them shuffled.  A colour
    with no positive channel has no sheen LOBE to sample (lobe_probabilities) yet is not "no sheen" for gltf_bsdf unless all are +-0."""
    rng = np.random.default_rng(229)
    k = len(SHEEN_COLOURS)
    sp = B.random_surfaces(rng, 64 * k)
    sp["sheen_color"] = np.repeat(np.asarray(SHEEN_COLOURS, f32), 64, axis=0)
    v, l, _ = B.directions(rng, sp, 64 * k, 0.3)
    s36 = B.pack36_all(sp)
    s36[:, 26:29] = np.repeat(np.asarray(SHEEN_COLOURS, f32), 64, axis=0)                    # (keeps the sign of -0.0)
    u = rng.random((64 * k, 3)).astype(f32)
    n = sp["shading_normal"]
    perm = rng.permutation(64 * k)
    qe, qs = B.pack48(s36, n, v, l), B.pack48(s36, n, v, u)
    return np.concatenate([qe, qe[perm]]), np.concatenate([qs, qs[perm]])


def check_sheen_colour_outputs(want_eval):
    k = len(SHEEN_COLOURS)
    p_sheen = want_eval[:64 * k, 11].reshape(k, 64)
    has_lobe = np.array([max(c) > 0 for c in SHEEN_COLOURS])
    assert (p_sheen[has_lobe] > 0).all() and (p_sheen[~has_lobe] == 0).all()
    print("sheen colours: a sheen lobe for %s, none for %s" % ([SHEEN_COLOURS[i] for i in np.flatnonzero(has_lobe)], [SHEEN_COLOURS[i] for i in np.flatnonzero(~has_lobe)]))


@pytest.mark.gpu
def test_sheen_colours_for_which_no_sheen_and_no_sheen_lobe_disagree(gpu):
    r, o = gpu
    qe, qs = sheen_colour_set()
    for mode, flags in MODES[:2]:
        want = check_ab("sheen colours EVALUATE " + mode, r, o, EVALUATE, flags, qe)
        check_ab("sheen colours SAMPLE " + mode, r, o, SAMPLE, flags, qs)
    check_sheen_colour_outputs(want)


# ---------------------------------------------------------------- query set 4: surface edges
def surface_edge_set():
    """Each edge value on 6 base surfaces (3 with the frame on the coordinate axes, so that n.v = 0 holds exactly; 3 of them with sheen)
    crossed with 5 direction pairs.  Returns the EVALUATE and SAMPLE queries and the edge's name per query."""
    rng = np.random.default_rng(233)
    nb = 6
    base = B.random_surfaces(rng, nb)
    base["shading_normal"][:3] = (0, 0, 1); base["anisotropy_tangent"][:3] = (1, 0, 0); base["anisotropy_bitangent"][:3] = (0, 1, 0)
    base["clearcoat_normal"][:3] = (0, 0, 1)
    base["sheen_color"][0::2] = 0.0
    base["sheen_color"][1::2] = np.asarray(rng.uniform(0.1, 1, (3, 3)), f32)
    base["ior"][:] = 1.5
    n0 = base["shading_normal"]
    cc60 = tilted(rng, n0, 60, 60).astype(np.float64)
    edges = [("alpha 0", {"alpha": 0.0}), ("alpha 1", {"alpha": 1.0}), ("metalness 0", {"metalness": 0.0}), ("metalness 1", {"metalness": 1.0}),
             ("roughness at the clamp", {"roughness_squared": (0.001, 0.001)}), ("ax / ay 10", {"roughness_squared": (0.01, 0.001)}),
             ("ax / ay 1000", {"roughness_squared": (1.0, 0.001)}), ("ax = ay = 1", {"roughness_squared": (1.0, 1.0)}),
             ("ior 1.0", {"ior": 1.0}), ("ior 0.9", {"ior": 0.9}), ("ior 2.5", {"ior": 2.5}),
             ("clearcoat 0", {"clearcoat": 0.0, "clearcoat_normal": n0}), ("clearcoat 1", {"clearcoat": 1.0, "clearcoat_normal": n0}),
             ("clearcoat 0, normal 60 degrees off", {"clearcoat": 0.0, "clearcoat_normal": cc60}), ("clearcoat 1, normal 60 degrees off", {"clearcoat": 1.0, "clearcoat_normal": cc60}),
             ("transmissive 0", {"transmissive": 0.0}), ("transmissive 1", {"transmissive": 1.0}), ("ior 1.0, transmissive 1", {"ior": 1.0, "transmissive": 1.0}),
             ("specular_factor 0", {"specular_factor": 0.0}), ("specular_color 1e4 (f0 clamps at 1)", {"specular_color": (1.0e4, 1.0e4, 1.0e4), "specular_factor": 1.0})]
    n32, t32 = n0.astype(f32), base["anisotropy_tangent"].astype(f32)
    rnd = lambda sign: B.directions(rng, base, nb, 1.0 if sign < 0 else 0.0)[1].astype(f32)
    grazing = B.nrm(t32.astype(np.float64) + 1e-4 * n32).astype(f32)
    pairs = [("normal incidence", n32, n32), ("n.v = 0", t32, rnd(1)), ("n.v < 0", rnd(-1), rnd(1)), ("grazing l", rnd(1), grazing), ("l through the surface", rnd(1), rnd(-1))]
    assert (B.dot(n32[:3].astype(np.float64), t32[:3].astype(np.float64)) == 0).all()
    s36, vs, ls, names = [], [], [], []
    for ename, over in edges:
        sp = {k: x.copy() for k, x in base.items()}
        for k, val in over.items():
            sp[k][...] = np.asarray(val, f32).astype(np.float64)
        rows = B.pack36_all(sp)
        for pname, v, l in pairs:
            s36.append(rows); vs.append(v); ls.append(l); names += [ename + ", " + pname] * nb
    s36, vs, ls = np.concatenate(s36), np.concatenate(vs), np.concatenate(ls)
    u = rng.random((len(s36), 3)).astype(f32)
    ng = s36[:, 7:10]
    return B.pack48(s36, ng, vs, ls), B.pack48(s36, ng, vs, u), names


@pytest.mark.gpu
def test_surface_edges(gpu):
    r, o = gpu
    qe, qs, names = surface_edge_set()
    for mode, flags in MODES:
        try:
            want = check_ab("surface edges EVALUATE " + mode, r, o, EVALUATE, flags, qe)
            check_ab("surface edges SAMPLE " + mode, r, o, SAMPLE, flags, qs)
        except AssertionError as e:
            m = re.search(r"query (\d+)", str(e))
            raise AssertionError("%s\n(%s)" % (e, names[int(m.group(1))] if m else "?"))
    print("surface edges: %d edge x direction cases on 6 surfaces; %d of the MIS EVALUATE values are non-finite" % (len(names) // 6, int((~np.isfinite(want[:, :3])).any(axis=1).sum())))


# ---------------------------------------------------------------- query set 5: lobe boundaries in SAMPLE
N_BOUNDARY = 200
UYZ = [0.0, 0.5, float(ONE_BELOW), 1.0]


def boundary_surfaces():
    rng = np.random.default_rng(239)
    sp = B.random_surfaces(rng, N_BOUNDARY)
    sp["alpha"][::2] = np.asarray(rng.uniform(0.2, 0.9, N_BOUNDARY // 2), f32)
    v, l, _ = B.directions(rng, sp, N_BOUNDARY, 0.0)
    return rng, B.pack36_all(sp), sp["shading_normal"], v, l


def boundary_set(probs_of):
    """probs_of(queries) -> the six probabilities per query, read from the hook under test.  17 values of u.x per surface: each of the
    five cumulative float32 edges, one ulp either side, 0 and 1; u.y, u.z from the corners {0, 0.5, 1 - 2^-24, 1}^2 in turn and, for every
    fifth query, random."""
    rng, s36, n, v, l = boundary_surfaces()
    probs = probs_of(B.pack48(s36, n, v, l))
    e = lobe_edges(probs)                                                                     # (200, 5)
    ux = np.concatenate([e, ulps(e, -1), ulps(e, 1), np.zeros((N_BOUNDARY, 1), f32), np.ones((N_BOUNDARY, 1), f32)], axis=1)   # (200, 17)
    m = ux.size
    k = np.arange(m)
    uy = np.where(k % 5 == 4, rng.random(m), np.take(UYZ, (k // 5) % 4)).astype(f32)
    uz = np.where(k % 5 == 4, rng.random(m), np.take(UYZ, (k // 20) % 4)).astype(f32)
    u = np.stack([ux.ravel(), uy, uz], axis=1)
    rep = lambda x: np.repeat(np.asarray(x, f32), 17, axis=0)
    return B.pack48(rep(s36), rep(n), rep(v), u), np.repeat(probs, 17, axis=0), e


def check_boundary_set(q, probs, e):
    """Non-vacuity: the edges ARE the selector's boundaries -- u.x on an edge and one ulp above choose different layers."""
    ux = q[:, 42].reshape(N_BOUNDARY, 17)
    p = probs.reshape(N_BOUNDARY, 17, 6)[:, 0]
    on = np.stack([select_layer(ux[:, j], p) for j in range(5)], axis=1)
    above = np.stack([select_layer(ux[:, 10 + j], p) for j in range(5)], axis=1)
    below = np.stack([select_layer(ux[:, 5 + j], p) for j in range(5)], axis=1)
    real = (e > 0) & (np.diff(np.concatenate([np.zeros((N_BOUNDARY, 1), f32), e], axis=1), axis=1) > 0)   # a lobe of positive width ends here
    flips = (on != above) & real
    print("lobe boundaries: %d queries; of %d edges that end a lobe, u.x on the edge and one ulp above choose different layers at %d (per edge %s); "
          "on the edge = one ulp below at %d" % (len(q), int(real.sum()), int(flips.sum()), flips.sum(axis=0).tolist(), int(((on == below) & real).sum())))
    assert (flips.sum(axis=0)[[0, 1, 3]] >= 50).all() and flips.sum() >= 300
    return flips


@pytest.mark.gpu
def test_lobe_boundaries_in_sample(gpu):
    r, o = gpu
    for unit in (0, 1):
        q, probs, e = boundary_set(lambda qq: gpu_bsdf(r, unit, EVALUATE, MIS, qq)[:, 9:15])
        check_boundary_set(q, probs, e)
        want = check_ab("lobe boundaries (edges from unit %d)" % unit, r, o, SAMPLE, MIS, q)
        layer = select_layer(q[:, 42], want[:, 9:15])
        # the selector's answer is visible in the outputs: the alpha lobe alone clears use_mis, alpha and transmission set is_transmission
        assert np.array_equal(want[:, 8] == 0, layer == 0) and np.array_equal(want[:, 7] == 1, (layer == 0) | (layer == 5))
        nan = np.isnan(want[:, :7]).any(axis=1)
        print("lobe boundaries: layers chosen %s, %d queries with a NaN (the oracle decides where)" % (np.bincount(layer, minlength=6).tolist(), int(nan.sum())))
    check_ab("lobe boundaries, non-MIS", r, o, SAMPLE, 0, q)
    check_ab("lobe boundaries, white", r, o, SAMPLE, WHITE, q)


# ---------------------------------------------------------------- query set 6: lights
def crafted_lights(rng):
    """40 light records (bsdf_ref.lights_array rows) mixing the three types; [35] repeats [5].  Every spot has a unit or deliberately odd
    direction; the padding holds garbage (the staged copy overwrites it with the cone terms, the others must not read it)."""
    L = B.lights_array(40)
    B.set_light_types(L, np.resize([B.LIGHT_POINT, B.LIGHT_SPOT, B.LIGHT_DIRECTIONAL, B.LIGHT_SPOT], 40))
    T = B.light_types(L)
    L[:, 1:4] = rng.uniform(-3, 3, (40, 3)).round(2)
    L[:, 4] = np.resize([0.0, 4.0, 0.0, 8.0, 2.0], 40)
    L[:, 5:8] = B.nrm(rng.normal(size=(40, 3)))
    L[:, 8] = rng.uniform(0.5, 20, 40)
    L[:, 9:12] = rng.uniform(0.05, 1, (40, 3))
    L[:, 12] = rng.uniform(0.05, 0.6, 40)
    L[:, 13] = L[:, 12] + rng.uniform(0.06, 0.7, 40)
    L[:, 14:16] = rng.uniform(-1e3, 1e3, (40, 2))                              # garbage in the padding
    L[1, 12] = L[1, 13] = 0.4                                                # inner == outer
    L[3, 12], L[3, 13] = 0.7, 0.3                                            # inner > outer
    L[5, 13] = f32(math.pi / 2)                                              # outer angle at pi / 2
    L[7, 5:8] *= 3.5                                                         # a non-unit direction
    L[9, 5:8] = 0.0                                                          # a zero direction (spot)
    L[10, 5:8] = 0.0                                                         # ... and directional
    L[11, 8] = 0.0                                                           # intensity 0
    L[12, 1:4] = (1.0e4, -1.0e4, 1.0e4); L[12, 4] = 16.0                     # 1e4 from the origin (point)
    L[13, 1:4] = (-1.0e4, 1.0e4, 250.0); L[13, 4] = 0.0                      # ... (spot)
    L[14, 5:8] *= 0.25                                                       # a short directional direction
    L[17, 12], L[17, 13] = 0.0, 0.02                                         # a cone narrower than the 0.001 floor of the scale
    L[33, 12], L[33, 13] = 0.2, 0.9                                          # spots past the LDS copy
    L[35] = L[5]
    L[37, 4] = 4.0
    assert T[5] == T[33] == T[37] == T[35] == T[1] == T[3] == T[7] == T[9] == T[13] == T[17] == B.LIGHT_SPOT and T[10] == T[14] == B.LIGHT_DIRECTIONAL
    return L


POINTS_PER_LIGHT = 50


def light_points(rng, L):
    """50 points per light: at the light (distance 0), along +x at half the range, exactly at it, one ulp either side and beyond; on the spot's
    axis; on the inner and the outer cone's edge and a few ulp either side; the rest random around the light."""
    n = len(L)
    pos = L[:, 1:4].astype(np.float64)
    P = pos[:, None, :] + rng.normal(size=(n, POINTS_PER_LIGHT, 3)) * rng.choice([0.3, 2.0, 6.0], (n, POINTS_PER_LIGHT, 1))
    P = P.astype(f32)
    c = np.where(L[:, 4] > 0, L[:, 4], 4.0).astype(f32)
    x = L[:, 1]
    P[:, 0] = L[:, 1:4]
    for k, dx in enumerate([c * f32(0.5), c, c * f32(1.5)]):
        P[:, 1 + k] = L[:, 1:4]; P[:, 1 + k, 0] = x + dx
    P[:, 4] = P[:, 2]; P[:, 4, 0] = ulps(P[:, 2, 0], 1)
    P[:, 5] = P[:, 2]; P[:, 5, 0] = ulps(P[:, 2, 0], -1)
    with np.errstate(all="ignore"):
        axis = B.nrm(L[:, 5:8].astype(np.float64))
    axis = np.where(np.isfinite(axis), axis, [0.0, 0.0, 1.0])
    perp = B.nrm(np.cross(axis, B.nrm(rng.normal(size=(n, 3)))))
    P[:, 6] = (pos + 1.7 * axis).astype(f32)                                  # on the axis
    P[:, 7] = (pos - 1.7 * axis).astype(f32)                                  # ... behind the light
    for k, ang in enumerate([L[:, 12], L[:, 13]]):
        a = ang.astype(np.float64)[:, None]
        edge = (pos + 2.3 * (np.cos(a) * axis + np.sin(a) * perp)).astype(f32)
        for j, d in enumerate([0, 2, -2, 5, -5]):
            P[:, 8 + 5 * k + j] = ulps(edge, d)
    return P


def light_cases(rng):
    """(name, table, query indices, query points) for tables of 1, 32, 33 and 40 lights."""
    full = crafted_lights(rng)
    cases = []
    for n in (1, 32, 33, 40):
        table = full[1:2].copy() if n == 1 else full[:n].copy()              # the table of one light: a spot
        if n == 1: table[0, 12], table[0, 13] = 0.3, 0.6
        P = light_points(rng, table)
        index = np.repeat(np.arange(n, dtype=u32), POINTS_PER_LIGHT)
        cases.append(("%d lights" % n, table, index, P.reshape(-1, 3)))
    return cases


def as_pt_lights(table):
    table = np.ascontiguousarray(table, f32)
    return (abi.PtLight * len(table)).from_buffer_copy(table.tobytes())


def check_lights_against_float64(name, table, index, p, got):
    """C for the lights: wherever float64 is finite the output is, and within bsdf_ref.light_ray_bound of it."""
    d64, c64 = B.light_ray(table, index, p)
    bd, bc, ea = B.light_ray_bound(table, index, p)
    ok = np.isfinite(d64).all(axis=1) & np.isfinite(c64).all(axis=1) & np.isfinite(bc)
    g = got.astype(np.float64)
    assert np.isfinite(g[ok, :6]).all(), name
    ed = np.abs(g[ok, :3] - d64[ok]).max(axis=1)
    ec = np.abs(g[ok, 3:6] - c64[ok]).max(axis=1)
    tight = ok & (ea <= 1e-3)
    ratio = ec / np.maximum(bc[ok], 1e-300)
    print("%s against float64: %d of %d queries finite (%d with a cone bound below 1e-3): direction error max %.2e (bound %.2e), colour error / bound max %.3f, median %.3f" %
          (name, int(ok.sum()), len(ok), int(tight.sum()), float(ed.max()), bd, float(ratio.max()), float(np.median(ratio))))
    assert (ed <= bd).all(), (name, float(ed.max()))
    assert (ec <= bc[ok]).all(), (name, int(np.flatnonzero(ec > bc[ok])[0]))
    assert ok.mean() > 0.8 and tight.sum() > 0.5 * ok.sum()
    return ok


def check_light_case_covers(name, table, index, p, want):
    """Non-vacuity on the oracle's outputs of the 40-light table: the cases of the issue are there."""
    T = B.light_types(table)[index]
    col = want[:, 3:6]
    lit = (col > 0).any(axis=1)
    nan = np.isnan(want[:, :6]).any(axis=1)
    cut = table[index, 4] > 0
    local = T != B.LIGHT_DIRECTIONAL
    with np.errstate(all="ignore"):
        dist = np.linalg.norm(table[index, 1:4].astype(np.float64) - p.astype(np.float64), axis=1)
    beyond = local & cut & (dist > table[index, 4]) & ~nan
    print("%s: %d lit, %d dark, %d with a NaN; %d beyond their range (all dark: %s); %d at distance 0" %
          (name, int(lit.sum()), int((~lit & ~nan).sum()), int(nan.sum()), int(beyond.sum()), bool((~lit[beyond]).all()), int((local & (dist == 0)).sum())))
    assert lit.sum() > 300 and (~lit & ~nan).sum() > 100 and nan.sum() >= 40 and beyond.sum() > 50 and (local & (dist == 0)).sum() >= 20
    spot = T == B.LIGHT_SPOT
    part = spot & lit & ~nan
    assert part.sum() > 100


@pytest.mark.gpu
def test_punctual_lights_staged_and_unstaged(gpu):
    r, o = gpu
    from oracle import pyoracle
    rng = np.random.default_rng(241)
    for name, table, index, p in light_cases(rng):
        n = len(table)
        r.set_lights(list(as_pt_lights(table)))
        want = pyoracle.light_query_many(as_pt_lights(table), index, p)
        if n == 40:
            check_light_case_covers(name, table, index, p, want)
        runs = [("unit 0", 0, 0), ("unit 1", 1, 0)] + ([("unit 0, small tables", 0, 1)] if n <= 32 else [])
        got = {}
        for rname, unit, small in runs:
            g = gpu_lights(r, unit, small, n, index, p)
            got[rname] = g
            bad = ~same_bits(g[:, :6], want[:, :6]).all(axis=1)
            print("%s, %s: %d queries, %d differ from the oracle" % (name, rname, len(g), int(bad.sum())))
            if bad.any():
                i = int(np.flatnonzero(bad)[0])
                raise AssertionError("%s, %s: query %d (light %d, %r at %r): gpu %r, oracle %r" % (name, rname, i, index[i], table[index[i]], p[i], g[i], want[i]))
            staged = np.ones(len(g), f32) if (unit == 0 and small) else (index < 32).astype(f32) if unit == 0 else np.zeros(len(g), f32)
            assert np.array_equal(g[:, 6], staged) and (g[:, 7] == 0).all(), (name, rname)
        assert same_bits(got["unit 0"][:, :6], got["unit 1"][:, :6]).all()
        check_lights_against_float64(name, table, index, p, got["unit 0"])
        if n == 40:
            # the same record in the LDS copy (index 5, cone terms staged) and outside it (index 35, computed in place), from the same points
            pts = p[index == 5]
            i5, i35 = np.full(len(pts), 5, u32), np.full(len(pts), 35, u32)
            a, b = gpu_lights(r, 0, 0, n, i5, pts), gpu_lights(r, 0, 0, n, i35, pts)
            assert (a[:, 6] == 1).all() and (b[:, 6] == 0).all() and same_bits(a[:, :6], b[:, :6]).all()
            assert (a[:, 3:6] > 0).any(axis=1).sum() >= 10 and (a[:, 3:6] == 0).all(axis=1).sum() >= 5        # inside and outside the cone
            # a prefix of the table: num_of_lights below the table's size stages only that many
            g = gpu_lights(r, 0, 1, 20, index[index < 20], p[index < 20])
            assert same_bits(g[:, :6], want[index < 20, :6]).all() and (g[:, 6] == 1).all()
    r.set_lights([])


# ---------------------------------------------------------------- query set 7: argument checking
@pytest.mark.gpu
def test_bsdf_and_light_hooks_reject_bad_arguments(gpu):
    r, o = gpu
    INVALID = -1                                                            # PT_ERR_INVALID_ARGUMENT
    q = np.zeros((70, 48), f32); out = np.full((70, 16), 7.0, f32)
    fb = hooks.lib().pt_debug_bsdf_query
    for unit, op in [(2, 0), (-1, 0), (0, 2), (1, -1)]:
        assert fb(r.h, unit, op, MIS, q.ctypes.data, 70, out.ctypes.data) == INVALID, (unit, op)
    assert fb(r.h, 0, 0, MIS, None, 70, out.ctypes.data) == INVALID
    assert fb(r.h, 0, 0, MIS, q.ctypes.data, 70, None) == INVALID
    assert fb(None, 0, 0, MIS, q.ctypes.data, 70, out.ctypes.data) == INVALID
    assert fb(r.h, 0, 0, MIS, None, 0, None) == 0
    assert (out == 7.0).all()                                               # nothing was launched
    table = crafted_lights(np.random.default_rng(1))[:33]
    r.set_lights(list(as_pt_lights(table)))
    fl = hooks.lib().pt_debug_light_query
    idx = np.zeros(70, u32); p = np.ones((70, 3), f32); lo = np.full((70, 8), 7.0, f32)
    call = lambda unit, small, n_lights, i=idx, pp=p, oo=lo, h=r.h: fl(h, unit, small, n_lights, None if i is None else i.ctypes.data, None if pp is None else pp.ctypes.data, 70,
                                                                      None if oo is None else oo.ctypes.data)
    assert call(2, 0, 33) == INVALID and call(-1, 0, 33) == INVALID
    assert call(0, 1, 33) == INVALID                                        # small_tables with 33 lights
    assert call(0, 0, 34) == INVALID and call(1, 0, 34) == INVALID and call(0, 0, -1) == INVALID      # more lights than the table holds
    assert call(0, 0, 33, i=None) == INVALID and call(0, 0, 33, pp=None) == INVALID and call(0, 0, 33, oo=None) == INVALID and call(0, 0, 33, h=None) == INVALID
    bad = idx.copy(); bad[69] = 33
    assert call(0, 0, 33, i=bad) == INVALID and call(1, 0, 33, i=bad) == INVALID
    bad[69] = 20
    assert call(0, 1, 20, i=bad) == INVALID                                 # an index past num_of_lights, inside the table
    assert call(0, 0, 0) == INVALID                                         # no light to index
    assert (lo == 7.0).all()
    assert call(0, 1, 32) == 0 and (lo[:, 7] == 0).all()                    # ... and the legal neighbour of the refused calls works
    r.set_lights([])


# ---------------------------------------------------------------- the same query sets on the oracle alone (no GPU)
def test_oracle_many_exports_equal_the_single_query_exports(oracle_lib):
    L = oracle_lib.lib()
    o = oracle_lib.Oracle()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    sp, v, l, through, ng_tilt, u = random_set()
    k = 300
    s36 = B.pack36_all(sp)[:k]
    for i in range(3):
        assert np.array_equal(s36[i], B.pack36(sp, i))
    unp = B.unpack36(s36)
    assert all(np.array_equal(unp[key], np.asarray(sp[key][:k], f32).astype(np.float64)) for key, _ in B.ORDER)
    qe, qs = B.pack48(s36, ng_tilt[:k], v[:k], l[:k]), B.pack48(s36, ng_tilt[:k], v[:k], u[:k])
    for mode, flags in MODES:
        many_e, many_s = o.bsdf_query_many(EVALUATE, flags, qe), o.bsdf_query_many(SAMPLE, flags, qs)
        for i in range(k):
            one4, one9 = np.zeros(4, f32), np.zeros(9, f32)
            row = np.ascontiguousarray(qe[i]); rows = np.ascontiguousarray(qs[i])
            L.orc_evaluate_bsdf(o.h, flags, vp(row[:36]), vp(row[36:39]), vp(row[39:42]), vp(row[42:45]), vp(one4))
            L.orc_sample_bsdf(o.h, flags, vp(rows[:36]), vp(rows[42:45]), vp(rows[39:42]), vp(one9))
            assert same_bits(one4, many_e[i, :4]).all() and same_bits(many_e[i, 4:7], qe[i, 42:45]).all() and (many_e[i, 7:9] == 0).all(), (mode, i)
            assert same_bits(one9, many_s[i, :9]).all(), (mode, i)
        assert same_bits(many_e[:, 9:15], many_s[:, 9:15]).all() and (many_e[:, 15] == 0).all()
    rng = np.random.default_rng(241)
    name, table, index, p = light_cases(rng)[3]
    lights = as_pt_lights(table)
    many = oracle_lib.light_query_many(lights, index, p)
    for i in range(0, len(index), 7):
        one = np.zeros(6, f32)
        L.orc_light_ray(C.byref(lights[int(index[i])]), vp(np.ascontiguousarray(p[i])), vp(one))
        assert same_bits(one, many[i, :6]).all() and (many[i, 6:] == 0).all(), i
    o.close()


def test_float64_light_ray_against_the_oracle_within_the_derived_bound(oracle_lib):
    rng = np.random.default_rng(241)
    for name, table, index, p in light_cases(rng):
        want = oracle_lib.light_query_many(as_pt_lights(table), index, p)
        check_lights_against_float64("oracle, " + name, table, index, p, want)
        d64, c64 = B.light_ray(table, index, p)
        assert np.array_equal(np.isnan(d64).any(axis=1) | np.isnan(c64).any(axis=1), np.isnan(want[:, :6]).any(axis=1))      # NaN where the shader's is
        if len(table) == 40:
            check_light_case_covers(name, table, index, p, want)


def test_query_sets_are_not_vacuous_on_the_oracle(oracle_lib):
    """The conditions every GPU test above asserts on the oracle's outputs, with the same seeds, without a GPU."""
    o = oracle_lib.Oracle()
    run = OracleOnly(o)
    run_random_set(run)
    q_eval, q_sample, has_sheen, layer = neighbour_set(o)
    check_neighbour_set_covers(has_sheen, layer)
    nan_from_the_lobe = 0
    for name, op, flags, q in sheen_shortcut_runs():
        nan = check_sheen_shortcut_outputs(name, run(name, op, flags, q))
        if name == "EVALUATE MIS, ng = n":
            nan_from_the_lobe = int(nan[:32].sum())
    assert nan_from_the_lobe >= 3
    qe, qs = sheen_colour_set()
    check_sheen_colour_outputs(run("sheen colours", EVALUATE, MIS, qe))
    qe, qs, names = surface_edge_set()
    assert len(names) == len(qe) == 20 * 5 * 6
    q, probs, e = boundary_set(lambda qq: o.bsdf_query_many(EVALUATE, MIS, qq)[:, 9:15])
    check_boundary_set(q, probs, e)
    o.close()
