"""Random sequences of scene edits against a freshly built context.  Run with -m gpu on an MI355X.

Every kernel is pinned in isolation elsewhere; this file pins the bookkeeping that decides WHICH of them runs after the host edits a scene
(csrc/mipt_api.hip: pt_scene_set_instances' three-way choice, mark_buffer_users, pt_accel_request_rebuild, pt_set_accel_builder, what
Pathtracer::BuildAccel consumes, and every call that builds implicitly).  tests/scene_edit_model.py holds the model of include/mipt.h's rules, the
starting scene (7 rows, 578 triangles), the edit kinds a-o and the generator; tests/test_scene_edit_model_host.py proves on the CPU what the
12 cases here (three builders x scene_edit_model.SEEDS, STEPS steps each) cover.  A step is 0-4 edits and one realisation (pt_build_accel, a
1-sample pt_trace, pt_lens_focus_at, pt_motion_snapshot, pt_debug_intersect or pt_debug_accel_read).  After every realisation:

  decision   the deltas of stats().accel_builds / accel_refits are the model's; a pt_build_accel straight after changes neither; no builder
             fell back.  A refused call returned the code the model names and moved neither count nor the snapshot's state.
  tree       pt_debug_accel_read through accel_ref.check_tree against the model's rows -- every invariant of its docstring, the whole shading
             packet included -- with the children's order demanded of the nodes no triangle of which was touched since the last full build;
             unless the step built, child references, WideRanges and the packets' (instance, primitive) order are those of the last full build.
  hits       >= 4000 fixed rays per sequence (half aimed from outside at the starting scene's triangles, half ray_hook.surface_rays) with flags 0
             and RF_CULL_BACK: the six words committed, t, u, v, instance, primitive bit-identical to a fresh Renderer loaded from the model's
             state with the same builder and to a fresh oracle; occlusion rays (RF_ACCEPT_FIRST): column 0.  No tolerance: DESIGN.md section 2
             rule (viii) makes the hit independent of the tree.
  picture    one 40 x 24 frame, 1 sample, FLAG_ACCUMULATE and FLAG_ALPHA_SHADOWS off (alpha-shadow transmittances multiply in slot order,
             which follows the tree): the float bits and the ray counts of the fresh context's frame.  Every fifth step also the first-vertex
             debug outputs TEXCOORD_0, TEXCOORD_1, VERTEX_COLOR, VERTEX_TANGENT and VERTEX_NORMAL: the ones that read the shading packet
             (and in the last step of a sequence, so that the suite's short ones have them too).
  snapshot   pt_motion_snapshot_state answers as include/mipt.h says: VALID iff the table has the row count and per-row triangle counts of
             the last take.

A failure's message carries the seed, the builder, the step and its edits: scene_edit_model.sequence(seed, STEPS, builder)[step] is the step.

Time per case on an MI355X, one session: 0.09-0.12 s at 8 steps (the first case of a process 1.8 s: it loads the library's kernels), against
0.17-0.26 s of the yardstick tests/test_gpu_accel_structure.py::test_a_refit_is_a_fresh_quantisation_of_the_same_topology[32770-*], which a case
here may not exceed.  A step takes about 13 ms, so 20 steps would take 0.27 s: hence 8; the conditions of tests/test_scene_edit_model_host.py hold for the 96 steps."""
import time

import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import accel_ref as ar
from tests import scene_edit_model as sem
from tests.accel_hook import accel_read
from tests.ray_hook import gpu_intersect, dxr_flags, RF_CULL_BACK, RF_ACCEPT_FIRST

pytestmark = pytest.mark.gpu
u32 = np.uint32
BUILDER_NAMES = {abi.BUILDER_LBVH: "lbvh", abi.BUILDER_PLOC: "ploc", abi.BUILDER_PLOC_REINSERT: "reinsert"}
PACKET_OUTPUTS = (abi.DEBUG_OUTPUT_TEXCOORD_0, abi.DEBUG_OUTPUT_TEXCOORD_1, abi.DEBUG_OUTPUT_VERTEX_COLOR, abi.DEBUG_OUTPUT_VERTEX_TANGENT, abi.DEBUG_OUTPUT_VERTEX_NORMAL)


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def counts(r):
    q = r.stats()
    return q.accel_builds, q.accel_refits


def frame(r, s, frame_index, debug_output=abi.DEBUG_OUTPUT_NONE):
    """-> (the frame's float bits [H, W, 4] uint32, the rays it took): one sample, nothing accumulated."""
    st = abi.PtSettings.from_buffer_copy(bytes(s.settings)); st.debug_output = debug_output
    assert not st.flags & (abi.FLAG_ACCUMULATE | abi.FLAG_ALPHA_SHADOWS)
    out = r.create_output(s.width, s.height)
    r.reset_stats()
    r.trace(st, s.execute_params(frame_index), out)
    q = r.stats()
    return r.readback(out).view(u32), (q.rays, q.rays_primary, q.rays_bounce, q.rays_shadow)


def realise(r, s, how, rays, k):
    if how == "build_accel": r.build_accel()
    elif how == "trace": r.trace(s.settings, s.execute_params(1000 + k), r.create_output(s.width, s.height))
    elif how == "focus_at": r.focus_at(s.settings, s.execute_params(0), s.width / 2, s.height / 2)
    elif how == "motion_snapshot": r.motion_snapshot(True)
    elif how == "debug_intersect": gpu_intersect(r, rays[:64], 0, 0)
    elif how == "accel_read": accel_read(r)
    else: raise KeyError(how)


def packet_ids(tree):
    return ar.as_bytes(tree[3], 64).view(u32).reshape(-1, 16)[:, [3, 7]]


def same_hits(a, b):
    return np.array_equal(a[:, :6].view(u32), b[:, :6].view(u32))


def first_difference(rays, a, b):
    k = int(np.nonzero((a[:, :6].view(u32) != b[:, :6].view(u32)).any(axis=1))[0][0])
    return "ray %d %s: %s against %s" % (k, rays[k].tolist(), a[k].tolist(), b[k].tolist())


_RAYS = {}
ORACLE_THREADS = 8


def run_sequence(R, oracle_lib, builder, seed, steps, say=print):
    """Plays scene_edit_model.sequence(seed, steps, builder) into a context and makes every check of the module docstring after every
    realisation.  -> the number of realisations checked.  Raises AssertionError with the reproducer on the first mismatch."""
    seq = sem.sequence(seed, steps, builder)
    model = sem.Model(builder)
    s = model.scene
    if seed not in _RAYS:                                                 # computed once per seed, shared by the builders, never written
        o0 = oracle_lib.Oracle(); s.upload(o0)
        _RAYS[seed] = sem.make_rays(seed, o0, s); _RAYS[seed].setflags(write=False)
        o0.close()
    rays = _RAYS[seed]
    assert len(rays) >= 4000
    r = R()
    try:
        live = sem.Live(r, model)
        base = None                                                       # the tree as the last full build left it
        for k, step in enumerate(seq):
            where = sem.describe(seed, builder, k, step)
            for e in step.edits:
                before = counts(r), r.motion_snapshot_state()
                live.send(model.apply(e))
                if e[0] == "m": assert (counts(r), r.motion_snapshot_state()) == before, where + ": a refused call changed something"
            assert r.motion_snapshot_state() == model.snapshot_state(), where + ": snapshot state after the edits"
            # 1. the decision
            c0 = counts(r)
            realise(r, s, step.realise, rays, k)
            c1 = counts(r)
            predict = model.realise(step.realise)
            assert predict == step.predict
            want = (c0[0] + (predict == "build"), c0[1] + (predict == "refit"))
            assert c1 == want, "%s: accel_builds, accel_refits went from %s to %s, the model says %s" % (where, c0, c1, want)
            r.build_accel()
            assert counts(r) == c1, where + ": a second pt_build_accel did something"
            assert counts(r) == (model.builds, model.refits) and r.stats().accel_builder_fallbacks == 0, where
            # 5. the snapshot rule
            assert r.motion_snapshot_state() == model.snapshot_state(), where + ": snapshot state"
            # 2. the tree
            tree = accel_read(r)
            n = int(tree[0][ar.INFO_N_TRIS])
            assert tree[2] is not None and int(tree[0][ar.INFO_BUILDER]) == model.builder and int(tree[0][ar.INFO_FALLBACKS]) == 0, where
            ids = packet_ids(tree)
            ordered = ~ar.touched_nodes(tree[2], n, model.touched_triangles(ids[:, 0])) if model.touched else None
            found = ar.check_tree(*tree, ar.scene_rows(model.scene), None, ordered)
            assert found == [], "%s: %s" % (where, found[:6])
            if predict == "build": base = tree
            else:
                assert np.array_equal(tree[1][:, 16:32], base[1][:, 16:32]), where + ": child references differ from the last full build's"
                assert np.array_equal(tree[2], base[2]), where + ": WideRanges differ from the last full build's"
                assert np.array_equal(ids, packet_ids(base)), where + ": the packets' (instance, primitive) order differs from the last full build's"
            # 3. the hits
            fresh = R(); o = oracle_lib.Oracle()
            try:
                sem.load_fresh(fresh, model); fresh.build_accel()
                assert counts(fresh) == (1, 0)
                sem.load_fresh(o, model, False)
                for flags in (0, RF_CULL_BACK):
                    g = gpu_intersect(r, rays, flags, 0)
                    f = gpu_intersect(fresh, rays, flags, 0)
                    c = o.intersect_many(rays, dxr_flags(flags), 0, ORACLE_THREADS)
                    assert same_hits(g, f), "%s: flags %d, against a fresh context: %s" % (where, flags, first_difference(rays, g, f))
                    assert same_hits(g, c), "%s: flags %d, against the oracle: %s" % (where, flags, first_difference(rays, g, c))
                g = gpu_intersect(r, rays, RF_ACCEPT_FIRST, 1)[:, 0]
                assert np.array_equal(g, gpu_intersect(fresh, rays, RF_ACCEPT_FIRST, 1)[:, 0]), where + ": occlusion rays, against a fresh context"
                assert np.array_equal(g, o.intersect_many(rays, dxr_flags(RF_ACCEPT_FIRST), 1, ORACLE_THREADS)[:, 0]), where + ": occlusion rays, against the oracle"
                # 4. the picture
                for d in (abi.DEBUG_OUTPUT_NONE,) + (PACKET_OUTPUTS if k % 5 == 4 or k == len(seq) - 1 else ()):
                    a, ra = frame(r, s, k, d); b, rb = frame(fresh, s, k, d)
                    assert np.array_equal(a, b), "%s: debug output %s: %d of %d words differ from the fresh context's frame" % (where, abi.DEBUG_OUTPUT_NAMES[d], int((a != b).sum()), a.size)
                    assert ra == rb, "%s: debug output %s: rays %s, the fresh context's %s" % (where, abi.DEBUG_OUTPUT_NAMES[d], ra, rb)
                assert counts(r) == c1, where + ": the checks themselves built or refitted"
            finally:
                fresh.close(); o.close()
        say("seed %d %s: %d steps, %d builds, %d refits, %d rows and %d triangles at the end" %
            (seed, BUILDER_NAMES[builder], len(seq), model.builds, model.refits, len(model.scene.instances), sum(model.counts())))
        return len(seq)
    finally:
        r.close()


@pytest.mark.parametrize("seed", sem.SEEDS)
@pytest.mark.parametrize("builder", sem.BUILDERS, ids=[BUILDER_NAMES[b] for b in sem.BUILDERS])
def test_a_random_sequence_of_edits_leaves_what_a_fresh_context_builds(R, oracle_lib, builder, seed):
    t0 = time.perf_counter()
    assert run_sequence(R, oracle_lib, builder, seed, sem.STEPS) == sem.STEPS
    print("%.2f s" % (time.perf_counter() - t0))
