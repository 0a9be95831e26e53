"""The per-vertex BSDF terms (pt_shading.h: BsdfView / prepare_bsdf, BsdfHalf / half_vectors) leave every result what it was.

The shade stage forms a vertex's light-independent BSDF terms once (prepare_bsdf<true>) and hands them to the up-to-three evaluations of the
hit; the megakernel keeps forming them in each evaluation (prepare_bsdf<false>, view_of); both hand one half-vector record to an evaluation's
pdf and value.  Every moved expression is the one that stood in place, so:

  (a) ~2 000 BSDF queries through pt_debug_bsdf_query, EVALUATE and SAMPLE, MIS and not, on both kernel builds (unit 0: the wavefront text,
      terms once per vertex; unit 1: the megakernel text, terms per evaluation), give the bits recorded in tests/golden/bsdf_hoist_queries.npz.
      That fixture was recorded ONCE from the library of the commit BEFORE this change, on an MI355X (tools/record_bsdf_hoist_fixture.py);
      it holds the inputs and that library's outputs, nothing else.  The comparison is test_gpu_bsdf.py's: bit-identical, any NaN equal to
      any NaN (payloads are not compared).  The same queries are compared with the CPU oracle in the same way.
      The queries put every moved term at its edges, in dedicated waves and mixed at random (hoist_queries).
  (b) small renders (24 x 20 and 40 x 24, 1 and 3 samples per trace) of a scene whose material table mixes those cases inside single waves,
      with the punctual lights on and off and with a flag set no specialised copy serves -- the two specialised k_wf_shade copies and the
      general one: wavefront == megakernel bit for bit, both against the oracle sample for sample (test_gpu_shade_parking.py's run_cases).
  (c) one query in which every hoisted term is live -- the oracle's answer moves when the term's own input moves -- answered by the hook,
      which prepares its vertex through the function the product calls (prepare_bsdf), with the oracle's bits, alone in a wave and among
      neighbours.

The tests without a gpu mark check the fixture itself: the generator reproduces its inputs, the inputs hold the edge cases they claim, and
the recorded outputs are the oracle's bits."""
import os

import numpy as np
import pytest

from gltf_renderer_amd import abi, scenes

import bsdf_ref as B
from test_gpu_bsdf import EVALUATE, MIS, SAMPLE, check_ab, gpu_bsdf, same_bits, tilted

f32 = np.float32
u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bsdf_hoist_queries.npz")
N_QUERIES = 2048                                     # 32 waves
SEED = 307
RUNS = [("eval_mis", EVALUATE, MIS), ("eval_plain", EVALUATE, 0), ("sample_mis", SAMPLE, MIS), ("sample_plain", SAMPLE, 0)]
ONE_ABOVE = np.nextafter(f32(1), f32(2))             # 1 + 2^-23

# columns of the 48-float query (tests/bsdf_ref.py ORDER)
ALBEDO, ALPHA, METAL, AX, AY, NORMAL, TANGENT, BITANGENT, IOR = slice(0, 3), 3, 4, 5, 6, slice(7, 10), slice(10, 13), slice(13, 16), 16
CLEARCOAT, CC_ROUGH, CC_NORMAL, SHEEN, SHEEN_ROUGH, TRANSMISSIVE = 21, 22, slice(23, 26), slice(26, 29), 29, 30
NG, VIEW, ARG = slice(36, 39), slice(39, 42), slice(42, 45)


# ---------------------------------------------------------------- the queries
def _axis_frame(q, i):
    q[i, NORMAL] = (0, 0, 1); q[i, TANGENT] = (1, 0, 0); q[i, BITANGENT] = (0, 1, 0); q[i, CC_NORMAL] = (0, 0, 1); q[i, NG] = (0, 0, 1)
    q[i, 44] = np.abs(q[i, 44])                      # l on the normal's side (still a unit vector)


def case_view_along_a_tangent_axis(rng, q, i):
    """ax != ay, the view exactly along the tangent (even positions) or the bitangent (odd): n.v = 0 exactly."""
    _axis_frame(q, i)
    q[i, AX], q[i, AY] = 0.3, 0.01
    q[i[0::2], VIEW] = (1, 0, 0); q[i[1::2], VIEW] = (0, 1, 0)


def case_view_along_the_normal(rng, q, i):
    """|n.v| = 1 exactly: v = n and v = -n."""
    _axis_frame(q, i)
    q[i[0::2], VIEW] = (0, 0, 1); q[i[1::2], VIEW] = (0, 0, -1)


def case_view_one_ulp_past_the_normal(rng, q, i):
    """|n.v| one ulp above 1."""
    _axis_frame(q, i)
    q[i[0::2], VIEW] = (0, 0, ONE_ABOVE); q[i[1::2], VIEW] = (0, 0, -ONE_ABOVE)


def case_nan_normal(rng, q, i):
    """A NaN in one component of the shading normal, in all three at every fourth position; the geometric normal stays."""
    for k in range(3):
        q[i[k::4], 7 + k] = np.nan
    q[i[3::4], NORMAL] = np.nan


def case_ior(rng, q, i):
    q[i, IOR] = np.resize(np.asarray([1.0, 0.0, -1.0, 1e30], f32), len(i))


def case_clearcoat(rng, q, i):
    """clearcoat 0, 0.5 and 1 with a clearcoat normal 40 degrees off the shading normal."""
    q[i, CLEARCOAT] = np.resize(np.asarray([0.0, 0.5, 1.0], f32), len(i))
    n = np.where(np.isfinite(q[i, NORMAL]), q[i, NORMAL], q[i, NG]).astype(np.float64)
    q[i, CC_NORMAL] = tilted(rng, B.nrm(n), 40, 40)


def case_both_modes(rng, q, i):
    """transmissive 0, 0, 1, 1 in turn; l through the surface at odd positions, on the view's side at even ones (ng = n decides)."""
    q[i, TRANSMISSIVE] = np.resize(np.asarray([0.0, 0.0, 1.0, 1.0], f32), len(i))
    n = q[i, NG].astype(np.float64); l = q[i, ARG].astype(np.float64); v = q[i, VIEW].astype(np.float64)
    side = np.sign(B.dot(n, v)) * np.where(np.arange(len(i)) % 2 == 1, -1.0, 1.0)          # the side l is wanted on
    flip = np.sign(B.dot(n, l)) != side
    l = np.where(flip[:, None], l - 2 * B.dot(n, l)[:, None] * n, l)
    q[i, ARG] = l.astype(f32)


def case_sheen_in_some_lanes(rng, q, i):
    q[i[0::2], SHEEN] = 0.0
    q[i[1::2], SHEEN] = rng.uniform(0.1, 1, (len(i[1::2]), 3)).astype(f32)


def case_no_sheen(rng, q, i):
    q[i, SHEEN] = 0.0


def case_sheen_everywhere(rng, q, i):
    q[i, SHEEN] = rng.uniform(0.1, 1, (len(i), 3)).astype(f32)


def case_albedo_zero_and_infinity(rng, q, i):
    q[i[0::4], ALBEDO] = (0.0, 0.5, np.inf); q[i[1::4], ALBEDO] = np.inf; q[i[2::4], ALBEDO] = 0.0


def case_alpha_below_one(rng, q, i):
    q[i, ALPHA] = rng.uniform(0.2, 0.8, len(i)).astype(f32)


# (case, waves it has to itself, sheen colour cleared in the first of them: the wave's vote for the sheen terms then says no)
DEDICATED = [(case_view_along_a_tangent_axis, 2, True), (case_view_along_the_normal, 2, True), (case_view_one_ulp_past_the_normal, 2, True),
             (case_nan_normal, 1, False), (case_ior, 2, True), (case_clearcoat, 2, True), (case_both_modes, 2, True),
             (case_sheen_in_some_lanes, 1, False), (case_no_sheen, 1, False), (case_sheen_everywhere, 1, False),
             (case_albedo_zero_and_infinity, 1, False), (case_alpha_below_one, 2, True)]
MIXED = [case_ior, case_clearcoat, case_both_modes, case_albedo_zero_and_infinity, case_alpha_below_one, case_nan_normal]
AXIS = [case_view_along_a_tangent_axis, case_view_along_the_normal, case_view_one_ulp_past_the_normal]


def hoist_queries():
    """(q_eval, u, wave_of): N_QUERIES EVALUATE queries, the SAMPLE queries' u, and the first wave of each dedicated case by name.  Waves
    [0, 19): the dedicated cases; the rest: every lane takes each MIXED case with probability 0.2, one AXIS case with probability 0.15, and
    loses its sheen colour with probability 0.5, so that the cases meet each other and both outcomes of the votes."""
    rng = np.random.default_rng(SEED)
    n = N_QUERIES
    sp = B.random_surfaces(rng, n)
    v, l, _ = B.directions(rng, sp, n, 0.35)
    q = B.pack48(B.pack36_all(sp), sp["shading_normal"], v, l)
    wave_of, w = {}, 0
    for case, waves, clear_first in DEDICATED:
        wave_of[case.__name__] = w
        i = np.arange(64 * w, 64 * (w + waves))
        case(rng, q, i)
        if clear_first:
            q[i[:64], SHEEN] = 0.0
        w += waves
    rest = np.arange(64 * w, n)
    q[rest[rng.random(len(rest)) < 0.5], SHEEN] = 0.0
    for case in MIXED:
        case(rng, q, rest[rng.random(len(rest)) < 0.2])
    pick = rng.integers(0, len(AXIS), len(rest)); take = rng.random(len(rest)) < 0.15
    for k, case in enumerate(AXIS):
        case(rng, q, rest[take & (pick == k)])
    u = rng.random((n, 3)).astype(f32)
    return np.ascontiguousarray(q, f32), u, wave_of


def sample_queries(q_eval, u):
    q = q_eval.copy()
    q[:, ARG] = u
    return q


def expand(fx, name, q):
    """The hook's 16 output floats per query from what the fixture keeps of run `name`: value and pdf (EVALUATE: l echoed, two zeros) or value,
    pdf, l, is_transmission, use_mis (SAMPLE); the six lobe probabilities are the vertex's, the same in every run; a last zero."""
    rec = fx["out_" + name]
    out = np.zeros((len(q), 16), f32)
    out[:, :rec.shape[1]] = rec
    if rec.shape[1] == 4:
        out[:, 4:7] = q[:, ARG]
    out[:, 9:15] = fx["lobes"]
    return out


def compact(name, out):
    return np.ascontiguousarray(out[:, :4] if name.startswith("eval") else out[:, :9])


@pytest.fixture(scope="module")
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------- (a) on the GPU
@pytest.fixture(scope="module")
def gpu(oracle_lib):
    from gltf_renderer_amd.renderer import Renderer
    r = Renderer()
    o = oracle_lib.Oracle()
    yield r, o
    r.close(); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,op,flags", RUNS, ids=[r[0] for r in RUNS])
def test_both_builds_give_the_bits_recorded_before_the_change(gpu, fixture, name, op, flags):
    r, o = gpu
    q = fixture["q_eval"] if op == EVALUATE else sample_queries(fixture["q_eval"], fixture["u"])
    want = expand(fixture, name, q)
    for unit in (0, 1):
        got = gpu_bsdf(r, unit, op, flags, q)
        bad = ~same_bits(got, want).all(axis=1)
        print("%s, unit %d: %d queries, %d differ from the recording" % (name, unit, len(q), int(bad.sum())))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError("%s, unit %d: query %d of %d (wave %d) differs from the recording\n in   %r\n got  %r\n want %r" % (name, unit, i, int(bad.sum()), i // 64, q[i], got[i], want[i]))
    check_ab("hoist queries, " + name, r, o, op, flags, q)                  # ... and the oracle's, by test_gpu_bsdf.py's comparison


# ---------------------------------------------------------------- (b) small renders
SIZES = [(24, 20), (40, 24)]
SPP = [1, 3]


def hoist_scene(width, height):
    """scenes.test_scene (16^2 textures: textured, anisotropic metal, clearcoat with its own normal map, sheen, glass, MASK and BLEND quads) with
    the two large surfaces behind and under the spheres changed, so that every 8 x 8 block of the image mixes the cases of (a): the floor
    gets a half clearcoat, a sheen colour with a zero channel and anisotropy; the default material (the back wall, the lone triangle) an ior
    of 1 -- f0 = 0 -- and a partly transmissive base; the BLEND quad, alpha 0.5, becomes a metal."""
    s = scenes.test_scene(32, 16)
    floor = s.materials[-1]
    floor.clearcoat_factor = 0.5; floor.clearcoat_roughness_factor = 0.3; floor.sheen_color_factor[:] = (0.4, 0.0, 0.2); floor.sheen_roughness_factor = 0.4
    floor.anisotropy_strength = 0.6
    s.materials[0].ior = 1.0; s.materials[0].transmission_factor = 0.3
    s.materials[-2].metalness_factor = 1.0
    s.width, s.height = width, height
    s.name = "hoist_%dx%d" % (width, height)
    return s


def hoist_cases(s):
    from test_gpu_shade_parking import copy_settings
    base = copy_settings(s.settings); base.reset = 1
    assert base.flags == abi.APP_DEFAULT_FLAGS
    no_lights = copy_settings(base); no_lights.flags &= ~abi.FLAG_POINT_LIGHTS
    general = copy_settings(base); general.flags &= ~abi.FLAG_SHADING_NORMAL_ADAPTATION          # no specialised copy for these flags
    plain = copy_settings(base); plain.flags &= ~abi.FLAG_MATERIAL_MIS                           # gltf_bsdf's mode 0: every term in one evaluation
    return [("defaults", base), ("no_point_lights", no_lights), ("general_copy", general), ("no_material_mis", plain)]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPP)
@pytest.mark.parametrize("size", SIZES, ids=lambda z: "%dx%d" % z)
def test_small_renders_wavefront_equals_megakernel_and_the_oracle(oracle_lib, size, spp):
    from gltf_renderer_amd.renderer import Renderer
    from test_gpu_shade_parking import run_cases
    s = hoist_scene(*size)
    img = run_cases(Renderer, oracle_lib, s, hoist_cases(s), spp)
    bits = lambda a: a.view(u32)
    # the cases are what they are named after where an image can show it (normal adaptation, the flag the general copy is picked by, acts on
    # few hits: its image may equal the defaults')
    assert not np.array_equal(bits(img["defaults"]), bits(img["no_point_lights"])) and not np.array_equal(bits(img["defaults"]), bits(img["no_material_mis"]))


# ---------------------------------------------------------------- (c) one query in which every hoisted term is live
def live_query():
    """A clearcoated, anisotropic, half-metallic sheen surface seen and lit at 50 and 35 degrees."""
    s36 = np.zeros((1, 36), f32)
    s36[0, ALBEDO] = (0.8, 0.5, 0.3); s36[0, ALPHA] = 1.0; s36[0, METAL] = 0.5; s36[0, AX], s36[0, AY] = 0.4, 0.1
    s36[0, NORMAL] = (0, 0, 1); s36[0, TANGENT] = (1, 0, 0); s36[0, BITANGENT] = (0, 1, 0); s36[0, IOR] = 1.5
    s36[0, 17:20] = (1.0, 0.9, 0.8); s36[0, 20] = 1.0; s36[0, CLEARCOAT] = 0.6; s36[0, CC_ROUGH] = 0.5
    s36[0, CC_NORMAL] = B.nrm(np.asarray([0.1, 0.05, 1.0])).astype(f32); s36[0, SHEEN] = (0.6, 0.3, 0.5); s36[0, SHEEN_ROUGH] = 0.3
    v = B.nrm(np.asarray([np.sin(np.radians(50)), 0.2, np.cos(np.radians(50))])).astype(f32)
    l = B.nrm(np.asarray([-np.sin(np.radians(35)), 0.3, np.cos(np.radians(35))])).astype(f32)
    return B.pack48(s36, s36[:, NORMAL], v[None], l[None])


# the input each hoisted term is formed from, and a second value for it
LIVE_TERMS = [("coat weight", CLEARCOAT, 0.0), ("f0", IOR, 1.0), ("albedo / pi", 0, 0.1), ("view half of the anisotropic visibility; ax * ay", AX, 0.05),
              ("view half of the clearcoat's visibility; a^2, 1 - a^2", CC_ROUGH, 0.9), ("sheen shadowing, E and max of the colour", 26, 0.0),
              ("sheen alpha", SHEEN_ROUGH, 0.9), ("local view, n.v", 41, 0.2)]


def live_term_moves(o):
    """Relative change of the oracle's MIS value when each term's input moves."""
    q = live_query()
    base = o.bsdf_query_many(EVALUATE, MIS, q)[0, :3].astype(np.float64)
    moves = []
    for name, col, val in LIVE_TERMS:
        p = q.copy(); p[0, col] = val
        moves.append((name, float(np.abs(o.bsdf_query_many(EVALUATE, MIS, p)[0, :3] - base).max() / np.abs(base).max())))
    return base, moves


@pytest.mark.gpu
def test_the_hook_prepares_its_vertex_as_the_product_does(gpu):
    r, o = gpu
    base, moves = live_term_moves(o)
    assert np.isfinite(base).all() and all(m > 1e-3 for _, m in moves), moves
    q, u, _ = hoist_queries()
    one = live_query()
    among = np.concatenate([q[:37], one, q[37:100]])                        # lane 37 of a wave of other surfaces, with and without sheen
    for op, arg in ((EVALUATE, one[0, ARG]), (SAMPLE, (0.9, 0.3, 0.6))):
        a = one.copy(); a[0, ARG] = arg
        b = among.copy(); b[37, ARG] = arg
        want = check_ab("live query alone, op %d" % op, r, o, op, MIS, a)
        check_ab("live query among neighbours, op %d" % op, r, o, op, MIS, b)
        for unit in (0, 1):
            assert same_bits(gpu_bsdf(r, unit, op, MIS, b)[37], want[0]).all(), (op, unit)


# ---------------------------------------------------------------- the fixture itself (no GPU)
def test_the_generator_reproduces_the_fixtures_inputs(fixture):
    q, u, _ = hoist_queries()
    assert q.shape == (N_QUERIES, 48) and same_bits(q, fixture["q_eval"]).all() and same_bits(u, fixture["u"]).all()
    assert set(fixture) == {"q_eval", "u", "lobes"} | {"out_" + r[0] for r in RUNS}
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_the_queries_hold_the_edges_of_every_moved_term():
    q, u, wave_of = hoist_queries()
    W = lambda name, k=0: q[64 * (wave_of[name] + k):64 * (wave_of[name] + k + 1)]
    ndv = lambda w: (w[:, NORMAL] * w[:, VIEW]).sum(axis=1, dtype=f32)
    sheen = lambda w: (w[:, SHEEN] != 0).any(axis=1)
    w = W("case_view_along_a_tangent_axis")
    assert (w[:, AX] != w[:, AY]).all() and (ndv(w) == 0).all() and (w[0::2, 39] == 1).all() and (w[1::2, 40] == 1).all()
    assert not sheen(w).any() and sheen(W("case_view_along_a_tangent_axis", 1)).any()              # the vote both ways
    assert set(ndv(W("case_view_along_the_normal")).tolist()) == {1.0, -1.0}
    assert set(np.abs(ndv(W("case_view_one_ulp_past_the_normal"))).tolist()) == {float(ONE_ABOVE)}
    w = W("case_nan_normal")
    assert np.isnan(w[:, NORMAL]).any(axis=1).all() and np.isnan(w[3::4, NORMAL]).all() and np.isfinite(w[:, NG]).all()
    assert set(W("case_ior")[:, IOR].tolist()) == {1.0, 0.0, -1.0, float(f32(1e30))}
    w = W("case_clearcoat")
    assert set(w[:, CLEARCOAT].tolist()) == {0.0, 0.5, 1.0}
    c = (w[:, NORMAL] * w[:, CC_NORMAL]).sum(axis=1)
    assert np.allclose(c, np.cos(np.radians(40)), atol=1e-5)
    for k in (0, 1):                                                                               # modes 1 and 2 in one wave, transmissive 0 and 1 in each
        w = W("case_both_modes", k)
        through = (w[:, NG] * w[:, ARG]).sum(axis=1) * (w[:, NG] * w[:, VIEW]).sum(axis=1) < 0
        assert np.array_equal(through, np.arange(64) % 2 == 1)
        for t in (0.0, 1.0):
            assert (through & (w[:, TRANSMISSIVE] == t)).sum() >= 8 and (~through & (w[:, TRANSMISSIVE] == t)).sum() >= 8
    w = W("case_sheen_in_some_lanes")
    assert np.array_equal(sheen(w), np.arange(64) % 2 == 1)
    assert not sheen(W("case_no_sheen")).any() and sheen(W("case_sheen_everywhere")).all()
    w = W("case_albedo_zero_and_infinity")
    assert np.isinf(w[:, ALBEDO]).any() and (w[:, ALBEDO] == 0).any() and (np.isinf(w[0::4, 2]) & (w[0::4, 0] == 0)).all()
    w = W("case_alpha_below_one", 1)
    assert (w[:, ALPHA] < 1).all() and (u[64 * (wave_of["case_alpha_below_one"] + 1):][:64, 0] <= 1 - w[:, ALPHA]).sum() >= 10      # the alpha layer is sampled
    rest = q[64 * 19:]
    mixed_waves = sum(int(0 < sheen(rest[k:k + 64]).sum() < 64) for k in range(0, len(rest), 64))
    assert len(rest) == 64 * 13 and mixed_waves == 13
    assert np.isnan(rest[:, NORMAL]).any() and np.isinf(rest[:, ALBEDO]).any() and (rest[:, IOR] == -1).any() and (np.abs(ndv(rest)) == ONE_ABOVE).any()


def test_the_recording_is_the_oracles_bits(oracle_lib, fixture):
    """What the library before the change gave on the MI355X is what the CPU oracle gives: the fixture is no snapshot of a private quirk."""
    o = oracle_lib.Oracle()
    lobes = None
    for name, op, flags in RUNS:
        q = fixture["q_eval"] if op == EVALUATE else sample_queries(fixture["q_eval"], fixture["u"])
        want = o.bsdf_query_many(op, flags, q)
        bad = ~same_bits(expand(fixture, name, q), want).all(axis=1)
        assert not bad.any(), (name, int(bad.sum()), int(np.flatnonzero(bad)[0]))
        assert (want[:, 15] == 0).all() and (op == SAMPLE or (want[:, 7:9] == 0).all())
        lobes = want[:, 9:15] if lobes is None else lobes
        assert same_bits(lobes, want[:, 9:15]).all()                                              # the vertex's, whatever the run
        nonfinite = ~np.isfinite(want[:, :4]).all(axis=1)
        print("%s: %d of %d queries with a non-finite value or pdf" % (name, int(nonfinite.sum()), len(q)))
        assert 50 <= nonfinite.sum() <= len(q) // 2                                               # the edges bite, and most queries are ordinary
    base, moves = live_term_moves(o)
    print("live query: value %r, relative moves %r" % (base, moves))
    assert np.isfinite(base).all() and all(m > 1e-3 for _, m in moves), moves
    o.close()
