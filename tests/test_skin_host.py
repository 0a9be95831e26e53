"""tests/skin_ref.py on its own, CPU only: the oracle's GpuSkin against the float64 restatement on every case that tests/test_gpu_skin.py
runs on the GPU, the properties those cases are chosen for, and the loader contract behind the non-finite cases.

The position criterion is derived, not tuned (tests/skin_ref.py): |p - p'| <= 10 * 2^-24 * S per vertex and component, exactly 0 where
S == 0.  The worst ratio err / (2^-24 * S) of every case is printed."""
import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import skin_ref as sr

f32, f64 = np.float32, np.float64
ANGLE_BOUND = 1.01 * 18 ** 0.5 / 1023


@pytest.fixture(scope="module")
def oracle_run(oracle_lib):
    """The oracle's outputs of a case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            o = oracle_lib.Oracle()
            cache[name] = sr.run(o, sr.case(name), 0)
            o.close()
        return cache[name]
    return get


@pytest.mark.parametrize("name", sr.ALL_CASES)
def test_the_oracle_meets_the_position_criterion_on_every_case(oracle_lib, oracle_run, name):
    c = sr.case(name)
    assert c.n <= 4000
    ref = sr.reference(oracle_lib, c)
    pos, ts = oracle_run(name)
    if not c.out_flags & abi.DYNAMIC_MESH_FLAG_POSITION:
        assert (sr.bits(pos) == sr.POSITION_FILL).all()
        return
    rows = np.isfinite(ref.p).all(axis=1) & np.isfinite(ref.S).all(axis=1)
    ratio = sr.position_ratio(pos, ref, rows)
    print("%-28s worst err / (2^-24 S) = %.3f over %d of %d vertices; S == 0 in %d components" %
          (name, float(ratio.max()), int(rows.sum()), c.n, int((ref.S[rows] == 0).sum())))
    assert (ratio <= sr.POSITION_ROUNDINGS).all(), float(ratio.max())
    # where the restatement is not finite the oracle has a NaN in exactly the components where it has one
    assert np.array_equal(np.isnan(pos), np.isnan(ref.p))
    if c.bad is None:
        assert rows.all()
    else:
        assert rows[~c.lists(c.bad)].all()


@pytest.mark.parametrize("name", sr.TS_SHARE_CASES)
def test_nine_tenths_of_a_tangent_space_case_are_well_conditioned(oracle_lib, name):
    """The packed-field rule of tests/test_gpu_skin.py applies where max(k_n, k_t) <= 64: the cases made for it (positive weights, scales
    within 10^[-1, 1]) must leave it at least 90 % of their vertices."""
    c = sr.case(name)
    ref = sr.reference(oracle_lib, c)
    share = float(ref.conditioned.mean())
    print("%-28s conditioned %.4f; median k_n %.2f, k_t %.2f" % (name, share, float(np.median(ref.k_n)), float(np.median(ref.k_t))))
    assert share >= 0.9
    w = c.jw[:, 4:]
    assert (w > 0).all() and np.abs(np.log10(np.linalg.svd(c.T[:, :3, :3].astype(f64), compute_uv=False))).max() <= 1 + 1e-6


@pytest.mark.parametrize("name", ["shape_1000_257", "gentle_4000", "rigid", "nonuniform"])
def test_the_oracles_normals_are_the_restatements(oracle_lib, oracle_run, name):
    """The decoded output normal of a well-conditioned vertex against n' / |n'|.  Each 10-bit octahedral field is rounded to the nearest
    step of 2 / 1023, so a coordinate (x, y) of the octahedron point v = (x, y, 1 - |x| - |y|) is off by at most h = 1 / 1023:
    |dv|^2 = dx^2 + dy^2 + (dx +- dy)^2 <= 6 h^2, and |v| >= 1 / sqrt(3) (a face centre), so the angle is at most sqrt(6) h * sqrt(3) =
    sqrt(18) / 1023 rad to first order; 1 % is added for the second order (h^2).  The computed direction's own error, at most
    10 * 2^-24 * 64, is two orders below that."""
    c = sr.case(name)
    ref = sr.reference(oracle_lib, c)
    _, ts = oracle_run(name)
    n, _, wind = sr.decode(oracle_lib, ts)
    m = ref.conditioned
    want = ref.n[m] / np.sqrt((ref.n[m] ** 2).sum(axis=1))[:, None]
    got = n[m].astype(f64)
    got /= np.sqrt((got ** 2).sum(axis=1))[:, None]
    ang = np.arccos(np.clip((got * want).sum(axis=1), -1, 1))
    print("%-28s worst angle %.5f rad of %.5f over %d vertices" % (name, float(ang.max()), ANGLE_BOUND, int(m.sum())))
    assert m.sum() > 0.5 * c.n and ang.max() <= ANGLE_BOUND


def test_the_cases_are_what_they_are_chosen_for():
    ns, js = {sr.case(n).n for n in sr.SHAPE_CASES}, {sr.case(n).bone_count for n in sr.SHAPE_CASES}
    assert ns == {1, 15, 16, 17, 63, 64, 65, 1000} and js == {1, 3, 4, 5, 19, 64, 257}
    assert {(1, 1), (17, 5), (1000, 257)} <= set(sr.SHAPES)
    # duplicated joints, joints beyond the bone array, zero weights and all-zero vertices are all there
    c = sr.case("nonuniform")
    ids, w = c.ids(), c.jw[:, 4:]
    assert (ids[:, 0] == ids[:, 1]).mean() > 0.2 and (ids >= c.bone_count).any() and (ids == 65535).any()
    assert (w == 0).mean() > 0.15 and (w == 0).all(axis=1).sum() >= 10 and (np.abs(w.astype(f64).sum(axis=1) / 65535 - 1) > 0.1).mean() > 0.8
    assert (sr.case("extreme").T[:, :3, 3].__abs__().max() > 5e3)
    # the non-finite cases: the bad bone is non-finite, every other bone finite; some vertices list it, some with weight zero, some do not
    for name in sr.NONFINITE:
        c = sr.case(name)
        raw = np.concatenate([c.T.reshape(len(c.T), -1), c.IT.reshape(len(c.IT), -1)], axis=1)
        finite = np.isfinite(raw).all(axis=1)
        assert not finite[c.bad] and finite[np.arange(len(finite)) != c.bad].all(), name
        lists = c.lists(c.bad)
        if name.startswith("e_"):
            assert not lists.any()
            continue
        zero = ((c.ids() == c.bad) & (c.jw[:, 4:] == 0)).any(axis=1)
        assert 0.1 < lists.mean() < 0.9 and zero.sum() >= 5 and (~lists).sum() >= 50, (name, float(lists.mean()), int(zero.sum()))
    assert sr.case("c_first_slab").bad < 4 and sr.case("d_last_partial_slab").bad == 18 and sr.case("d_last_partial_slab").bone_count % 4 == 3
    assert sr.case("arena_%d" % sr.ARENA_BIG).bone_count == 3000 and sr.case("arena_0").bone_count == 300


def test_the_loader_gives_a_zero_scaled_joint_a_finite_transform_and_a_nan_inverse_transpose(tmp_path):
    """The input that case (a) stands for: glm_lite.h inverse_transpose returns NaN for a singular matrix, and gather_bones calls it for
    every joint.  The other two joints' bones are finite."""
    from gltf_renderer_amd import gltf as G
    path, node = sr.zero_scaled_strip(str(tmp_path / "strip.glb"))
    sc = G.GltfScene(path)
    sc.calculate_global_transforms(0)
    bones = sc.gather_bones(node)
    assert len(bones) == 3
    t = np.array([list(b.transform) for b in bones], f32)
    it = np.array([list(b.inverse_transpose) for b in bones], f32)
    assert np.isfinite(t).all()
    assert np.isfinite(it[0]).all() and np.isfinite(it[2]).all()
    assert not np.isfinite(it[1]).all()
    assert (t[1].reshape(4, 4)[:3, :3] == 0).all()                        # the zero scale, finite
    # the other two are what they should be: inverse_transpose * transpose(transform) = 1 on the 3x3
    for k in (0, 2):
        m, n = t[k].reshape(4, 4).T[:3, :3].astype(f64), it[k].reshape(4, 4).T[:3, :3].astype(f64)
        assert np.allclose(n.T @ m, np.eye(3), atol=1e-5)
    # and these are the bones that case (a) feeds to the kernels
    a = sr.case("a_loader_zero_scale")
    assert np.array_equal(sr.bits(a.T.transpose(0, 2, 1).reshape(3, 16)), sr.bits(t))
    assert np.array_equal(np.isnan(a.IT.transpose(0, 2, 1).reshape(3, 16)), np.isnan(it))
