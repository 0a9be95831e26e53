"""Closed meshes do not leak: rays aimed at shared edges and vertices through the CPU oracle's traversal (its LBVH and its exhaustive search),
ray by ray against the float64 expectation of tests/watertight_cases.py -- plus the conditions that keep these tests from passing vacuously:
the rays do meet the cracks of the float test, the band the product uses holds every disagreement, and refusals of the own-box gate are
counted apart.  The oracle states the triangle test as csrc/pt_traverse.h does; tests/test_gpu_watertight.py holds the kernels to it bit by bit."""
import os

import numpy as np
import pytest

import watertight_cases as wc
from gltf_renderer_amd import scenes
from ray_hook import dxr_flags, surface_rays, RF_CULL_BACK, RF_ACCEPT_FIRST

N = 2000                      # rays per (mesh, placement, side, class)
GATE_CAP = 1e-5               # share of a case's rays the gate may refuse
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "watertight_ordinary_hits.npy")
N_GOLDEN, N_SURFACE = 300, 4000
_CASES = {}


def cases_of(name):
    if name not in _CASES: _CASES[name] = wc.mesh_cases(name, N)
    return _CASES[name]


def label(c):
    return "%s/%s/%s" % (c["placement"], "inside" if c["inside"] else "outside", c["cls"])


@pytest.mark.parametrize("name", wc.MESHES)
def test_the_rays_meet_the_cracks_of_the_float_test(name):
    """A condition on the INPUTS: the float test alone, as it stood, refuses at least 1 % of the edge rays and 1 % of the vertex rays of every
    placement and side on every triangle around the target -- rays that went through the surface."""
    print()
    for c in cases_of(name):
        if c["cls"] not in ("edge", "vertex"): continue
        w0, w1, w2, valid = wc.incident_vertices(c)
        r = c["rays"]
        refused = ~(wc.today_accepts(r[:, None, 0:3], r[:, None, 4:7], w0, w1, w2) & valid).any(1)
        print("%s %s: the float test refuses %.2f %% on every incident triangle" % (name, label(c), 100 * refused.mean()))
        assert refused.mean() >= 0.01, (name, label(c), float(refused.mean()))


@pytest.mark.parametrize("name", wc.MESHES)
def test_no_disagreement_of_float_test_and_edge_rule_lies_outside_the_band(name):
    """On every ray and every triangle incident to its target: where the float test and the edge values disagree, the candidate is in the band
    (so the edge values decide it).  Interior rays never are.  Prints how much of the band the disagreements use."""
    worst = 0.0
    for c in cases_of(name):
        w0, w1, w2, valid = wc.incident_vertices(c)
        r = c["rays"]; o, d = r[:, None, 0:3], r[:, None, 4:7]
        inside, u, v, t, in_band, f = wc.decide(o, d, w0, w1, w2)
        differ = (wc.edge_rule(o, d, w0, w1, w2, f["det"]) != f["inside"]) & valid
        with np.errstate(all="ignore"):
            units = np.where(differ, np.abs(f["m"]) / (f["band"] / wc.BAND_UNITS), 0.0)
        worst = max(worst, float(units.max()))
        assert int((differ & ~in_band).sum()) == 0, (name, label(c), float(units.max()))
        if c["cls"] == "interior": assert not (in_band & valid).any() and not differ.any(), (name, label(c))
    print("\n%s: disagreements reach %.2f of the band's %.0f units" % (name, worst, float(wc.BAND_UNITS)))
    assert worst < float(wc.BAND_UNITS) / 2


@pytest.fixture(scope="module")
def oracles(oracle_lib):
    made = {}
    def get(name):
        if name not in made:
            s = wc.make_scene(name); o = oracle_lib.Oracle(); s.upload(o); o.build_accel(); o.set_watertight(True)
            made[name] = o
        return made[name]
    yield get
    for o in made.values(): o.close()


def leaks(c, out, excused):
    leak = ~wc.expected(c, out)
    return leak & ~excused, leak & excused


@pytest.mark.parametrize("search", ["lbvh", "brute_force"])
@pytest.mark.parametrize("name", wc.MESHES)
def test_no_ray_leaks_through_a_shared_edge_or_vertex(oracles, name, search):
    """Every ray of every class commits the expected hit: closest-hit without flags, with back-face culling from the outside (front faces are
    aimed at; the mirrored placement included), and as an occlusion ray that accepts the first hit.  A ray leaves the assertion only as a
    refusal of the own-box gate that the numpy restatement of the gate confirms; at most 1e-5 of a case's rays may (counts printed)."""
    o = oracles(name); o.set_brute_force(search == "brute_force")
    try:
        n_gate = n_rays = 0
        for c in cases_of(name):
            r = c["rays"]
            excused = wc.gate_refused(c)
            assert excused.sum() <= GATE_CAP * len(r), (name, label(c), int(excused.sum()))
            out = o.intersect_many(r, 0, 0)
            bad, gone = leaks(c, out, excused)
            assert not bad.any(), (name, label(c), "closest hit", int(bad.sum()), r[bad][:3], out[bad][:3])
            n_gate += int(gone.sum()); n_rays += len(r)
            if search == "lbvh":           # the restatement IS the oracle's arithmetic: t, u, v of the hit, to the bit
                w0, w1, w2, valid = wc.incident_vertices(c)
                inside, u, v, t, in_band, f = wc.decide(r[:, None, 0:3], r[:, None, 4:7], w0, w1, w2)
                k = np.argmax(c["incident"] == out[:, 5].astype(np.int64)[:, None], axis=1); i = np.arange(len(r))
                mine = np.stack([t[i, k], u[i, k], v[i, k]], 1).astype(np.float32)
                assert np.array_equal(mine[~gone].view(np.uint32), out[~gone, 1:4].view(np.uint32)), (name, label(c))
            if not c["inside"]:
                out = o.intersect_many(r, dxr_flags(RF_CULL_BACK), 0)
                bad, gone = leaks(c, out, excused)
                assert not bad.any() and (out[~gone, 6] == 1).all(), (name, label(c), "culling back faces", int(bad.sum()))
            out = o.intersect_many(r, dxr_flags(RF_ACCEPT_FIRST), 1)
            bad = (out[:, 0] == 0) & ~excused
            assert not bad.any(), (name, label(c), "occlusion", int(bad.sum()))
        print("\n%s, %s: %d rays, %d refused by the own-box gate" % (name, search, n_rays, n_gate))
    finally:
        o.set_brute_force(False)


def test_the_former_gate_pad_refused_aimed_rays_and_the_present_one_refuses_none():
    """Why the watertight test brings a wider exit pad (csrc/pt_slab.h exit_pad): with the pad 1.0000004 of the float test the restated gate
    refuses more than 1e-5 of the rays the edge rule accepts (all of them aimed at vertices or edges), with 1.000004 none.  Prints both counts."""
    before = now = total = 0
    for name in wc.MESHES:
        for c in cases_of(name):
            if c["cls"] == "interior": continue
            before += int(wc.gate_refused(c, wc.GATE_PAD_BEFORE).sum()); now += int(wc.gate_refused(c).sum()); total += len(c["rays"])
    print("\nown-box gate refusals among %d edge, vertex and near rays: %d with pad %.7f, %d with pad %.6f" % (total, before, wc.GATE_PAD_BEFORE, now, wc.GATE_PAD))
    assert before > GATE_CAP * total and now == 0


def ordinary_rays(oracle_lib):
    """The rays whose hits the edge rule must leave alone: the interior class of every case, and rays as the path tracer casts them in an
    existing scene (ray_hook.surface_rays)."""
    rays = [c["rays"][:N_GOLDEN] for name in wc.MESHES for c in cases_of(name) if c["cls"] == "interior"]
    scene_of = [name for name in wc.MESHES for c in cases_of(name) if c["cls"] == "interior"]
    s = scenes.material_grid(64, 8)
    o = oracle_lib.Oracle(); s.upload(o); o.build_accel()
    first, second = surface_rays(o, s, N_SURFACE, 5)
    return rays, scene_of, o, [first, second]


def ordinary_hits(oracle_lib, oracle_of, watertight):
    rays, scene_of, o, surface = ordinary_rays(oracle_lib)
    switch = lambda x, on: x.set_watertight(on) if hasattr(x, "set_watertight") else None      # (an oracle from before the switch: the float test alone)
    switch(o, watertight)
    out = []
    for r, name in zip(rays, scene_of):
        x = oracle_of(name)
        switch(x, watertight); out.append(x.intersect_many(r, 0, 0)[:, :7]); switch(x, True)
    out += [o.intersect_many(r, 0, 0)[:, :7] for r in surface]
    o.close()
    return np.ascontiguousarray(np.concatenate(out), np.float32)


@pytest.mark.parametrize("watertight", [False, True])
def test_ordinary_hits_keep_their_bits(oracle_lib, oracles, watertight):
    """(committed, t, u, v, instance, primitive, front) of the interior class and of surface rays in the material grid, against what the oracle
    gave before the edge rule and the wider pad existed (recorded once into tests/golden/): identical to the bit, with the watertight test
    switched on and, as it is by default, off."""
    got = ordinary_hits(oracle_lib, oracles, watertight)
    want = np.load(GOLDEN)
    assert got.shape == want.shape and (want[:, 0] > 0).mean() > 0.5
    differ = (got.view(np.uint32) != want.view(np.uint32)).any(1)
    assert not differ.any(), (int(differ.sum()), got[differ][:3], want[differ][:3])

