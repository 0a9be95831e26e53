"""GpuSkin::Run (include/mipt.h pt_skin_run; k_skin and k_skin_mfma of csrc/skin_tonemap.hip) on the MI355X, case by case against
tests/skin_ref.py -- a float64 restatement of Skin.cs.hlsl -- and the oracle.  The buffers are built directly; no scene is involved.

  positions      both kernels: |p - p'| <= 10 * 2^-24 * S per vertex and component, exactly 0 where S == 0 (the count of the roundings is in
                 tests/skin_ref.py; tests/test_skin_host.py holds the oracle to the same bound on the same cases).  The worst ratio is printed.
  k_skin         follows the shader's order of operations: the oracle's bits, positions and packed words, on every case.
  k_skin_mfma    packed tangent spaces against the oracle's by the suite's rule (both octahedral fields within 1 step, the angle within 2
                 cyclically, winding equal) on the vertices with max(k_n, k_t) <= 64: there the computed direction is off by about
                 10 * 2^-24 * k, far below a quantisation step.  The share of identical words is printed, not asserted.
  non-finite     a bone with a NaN or an infinity damages the vertices that list it and no others (GpuSkin::Run keeps such a call away
                 from the dense matrix-core product, where 0 * NaN would reach every vertex)."""
import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import skin_ref as sr

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
KERNELS = {"k_skin": 0, "k_skin_mfma": 1}
kernels = pytest.mark.parametrize("kernel", list(KERNELS))


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


@pytest.fixture(scope="module")
def expected(oracle_lib):
    """The restatement and the oracle's outputs of a case, computed once and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            o = oracle_lib.Oracle()
            cache[name] = (sr.reference(oracle_lib, sr.case(name)),) + sr.run(o, sr.case(name), 0)
            o.close()
        return cache[name]
    return get


def gpu_run(R, name, kernel):
    r = R()
    out = sr.run(r, sr.case(name), KERNELS[kernel])
    r.close()
    return out


def check(name, kernel, got, want, rows=None):
    """The criteria of the module docstring over the vertices `rows` (default: all) of a case; prints the figures."""
    c = sr.case(name)
    ref, pos_o, ts_o = want
    pos, ts = got
    rows = np.ones(c.n, bool) if rows is None else rows
    line = "%-30s %-11s" % (name, kernel)
    if c.out_flags & abi.DYNAMIC_MESH_FLAG_POSITION:
        ratio = sr.position_ratio(pos, ref, rows)
        line += " worst err / (2^-24 S) = %.3f" % float(ratio.max())
    else:
        ratio = np.zeros(1)
        assert (sr.bits(pos) == sr.POSITION_FILL).all(), "the position buffer is no output of this call and was written"
    if c.out_flags & abi.DYNAMIC_MESH_FLAG_TANGENT_SPACE:
        m = rows & ref.conditioned if c.in_flags & abi.MESH_FLAG_TANGENT_SPACE else np.zeros(c.n, bool)
        close = sr.packed_fields(ts[m], ts_o[m])
        line += "; packed words equal %.4f of %d conditioned (%.4f of all %d)" % (float(np.mean(ts[m] == ts_o[m])) if m.any() else 1.0, int(m.sum()),
                                                                                 float(np.mean(ts[rows] == ts_o[rows])), int(rows.sum()))
    else:
        close = np.ones(1, bool)
        assert (ts == sr.TANGENT_SPACE_FILL).all(), "the tangent-space buffer is no output of this call and was written"
    print(line)
    assert (ratio <= sr.POSITION_ROUNDINGS).all(), (name, kernel, float(ratio.max()), int((ratio > sr.POSITION_ROUNDINGS).sum()))
    assert close.all(), (name, kernel, int((~close).sum()), "vertices part from the oracle's packed fields")
    if not c.in_flags & abi.MESH_FLAG_TANGENT_SPACE and c.out_flags & abi.DYNAMIC_MESH_FLAG_TANGENT_SPACE:
        assert np.array_equal(ts, ts_o)                  # normal and tangent stay zero: normalize gives NaN, and its encoding is one function
    if kernel == "k_skin":
        assert sr.same_floats(pos, pos_o), (name, int((sr.bits(pos) != sr.bits(pos_o)).sum()), "position components are not the oracle's bits")
        assert np.array_equal(ts, ts_o), (name, int((ts != ts_o).sum()), "packed words are not the oracle's")


# ---- tile and slab shapes; bone kinds ----------------------------------------------------------------------------------------------------
@kernels
@pytest.mark.parametrize("name", sr.SHAPE_CASES + ["gentle_4000"])
def test_tile_and_slab_shapes(R, expected, name, kernel):
    """Vertex counts around the 16-vertex tile and the 64-lane group, bone counts around the 4-bone slab, in one, several and many blocks."""
    check(name, kernel, gpu_run(R, name, kernel), expected(name))


@kernels
@pytest.mark.parametrize("name", sr.KINDS)
def test_bone_kinds(R, expected, name, kernel):
    """Rigid; non-uniform and mirrored over 10^[-2, 2] with translations to 1e3; extreme over 10^[-3, 3] with translations to 1e4.  Zero
    weights, all-zero vertices, duplicated joints and joints beyond the bone array are in every one of them."""
    check(name, kernel, gpu_run(R, name, kernel), expected(name))


# ---- flag subsets ----------------------------------------------------------------------------------------------------------------------
@kernels
@pytest.mark.parametrize("name", sr.FLAG_SUBSETS)
def test_flag_subsets(R, expected, name, kernel):
    """Joint weights without an input tangent space; position the only output; tangent space the only output.  The buffer that is no output
    is pre-filled and must come back untouched (checked in check())."""
    c = sr.case(name)
    got = gpu_run(R, name, kernel)
    check(name, kernel, got, expected(name))
    if c.out_flags == abi.DYNAMIC_MESH_FLAG_POSITION:
        assert (got[1] == sr.TANGENT_SPACE_FILL).all() and not (sr.bits(got[0]) == sr.POSITION_FILL).any()
    if c.out_flags == abi.DYNAMIC_MESH_FLAG_TANGENT_SPACE:
        assert (sr.bits(got[0]) == sr.POSITION_FILL).all() and not (got[1] == sr.TANGENT_SPACE_FILL).any()


@kernels
def test_zero_to_four_morph_targets_with_scaled_bones(R, expected, kernel):
    """0 .. 4 targets (position + tangent space, position only, tangent space only, both) under non-uniform, mirrored bones."""
    moved = []
    for k in range(5):
        name = "morph_%d" % k
        got = gpu_run(R, name, kernel)
        check(name, kernel, got, expected(name))
        moved.append(got)
    for k in range(1, 5):                               # every added target changes something
        assert not (np.array_equal(sr.bits(moved[k][0]), sr.bits(moved[k - 1][0])) and np.array_equal(moved[k][1], moved[k - 1][1])), k


# ---- non-finite bones ------------------------------------------------------------------------------------------------------------------
@kernels
@pytest.mark.parametrize("name", sr.NONFINITE)
def test_a_non_finite_bone_damages_only_the_vertices_that_list_it(R, expected, name, kernel):
    """(a) the loader's bones of a zero-scaled joint: finite transform, all-NaN inverse_transpose; (b) one +inf in a transform; (c) the bad
    bone in slab 0; (d) in the last, partial slab; (e) listed by no vertex.  Vertices that do not list the bad bone, whatever their weights,
    meet every criterion as if the bone were finite; those that do have NaN in exactly the position components where the oracle has NaN
    (listing it with weight 0 counts: 0 * NaN)."""
    c = sr.case(name)
    want = expected(name)
    ref, pos_o, ts_o = want
    got = gpu_run(R, name, kernel)
    lists = c.lists(c.bad)
    assert np.isfinite(ref.p[~lists]).all() and np.isfinite(ref.n[~lists]).all() and np.isfinite(ref.t[~lists]).all()
    check(name, kernel, got, want, rows=~lists)
    print("%-30s %-11s lists the bad bone: %d of %d vertices; NaN position components: %d (oracle %d); words unlike the oracle's: %d there, %d elsewhere" %
          (name, kernel, int(lists.sum()), c.n, int(np.isnan(got[0]).sum()), int(np.isnan(pos_o).sum()), int((got[1] != ts_o)[lists].sum()),
           int((got[1] != ts_o)[~lists].sum())))
    assert np.array_equal(np.isnan(got[0]), np.isnan(pos_o)), (int(np.isnan(got[0]).sum()), int(np.isnan(pos_o).sum()))
    assert not np.isnan(got[0][~lists]).any()
    # the position components that are finite on both sides of a listing vertex still meet the bound
    fin = lists[:, None] & np.isfinite(ref.p) & np.isfinite(ref.S) & np.isfinite(pos_o)
    if fin.any():
        ratio = sr.position_ratio(got[0], ref)[fin]
        assert (ratio <= sr.POSITION_ROUNDINGS).all(), float(ratio.max())


# ---- the bone arena ----------------------------------------------------------------------------------------------------------------------
@kernels
def test_back_to_back_calls_keep_their_own_bones(R, expected, kernel):
    """One context, 24 calls of 300 bones with no read between them (the arena of GpuSkin::Run wraps behind its fence), one of 3000 (it
    regrows), two more of 300; only then everything is read.  Every output is, bit for bit, what the same call gives alone in a fresh
    context, and for k_skin the oracle's."""
    names = ["arena_%d" % k for k in range(sr.ARENA_CALLS)]
    r = R()
    calls = [sr.Call(r, sr.case(n), KERNELS[kernel]) for n in names]
    for call in calls:
        call.run()
    together = [call.read() for call in calls]
    r.close()
    for n, (pos, ts) in zip(names, together):
        alone_pos, alone_ts = gpu_run(R, n, kernel)
        assert np.array_equal(sr.bits(pos), sr.bits(alone_pos)) and np.array_equal(ts, alone_ts), n
        if kernel == "k_skin":
            _, pos_o, ts_o = expected(n)
            assert sr.same_floats(pos, pos_o) and np.array_equal(ts, ts_o), n
    # the calls differ: nobody's bones would do for somebody else
    assert not np.array_equal(sr.bits(together[0][0]), sr.bits(together[1][0]))
