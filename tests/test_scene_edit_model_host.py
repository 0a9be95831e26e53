"""tests/scene_edit_model.py without a GPU: the sequences tests/test_gpu_scene_edits.py runs cover what they are meant to, their rays hit
something in every state, the model is deterministic and a refused edit leaves it alone, and a state loaded at once equals the same state
reached edit by edit (both into the oracle, which has no tree to keep and so nothing to get wrong there)."""
import collections

import numpy as np
import pytest

from gltf_renderer_amd import abi
from tests import scene_edit_model as sem

CASES = [(b, s) for b in sem.BUILDERS for s in sem.SEEDS]


@pytest.fixture(scope="module")
def sequences():
    return {(b, s): sem.sequence(s, sem.STEPS, b) for b, s in CASES}


def test_the_sequences_cover_every_edit_prediction_realisation_and_order(sequences):
    kinds, predictions, realisations, tags = (collections.Counter() for _ in range(4))
    steps = many = 0
    for seq in sequences.values():
        assert len(seq) == sem.STEPS
        for st in seq:
            steps += 1; many += len(st.edits) >= 2
            kinds.update(e[0] for e in st.edits); predictions[st.predict] += 1; realisations[st.realise] += 1; tags.update(st.tags)
            assert len(st.edits) <= 4
    print(dict(kinds), dict(predictions), dict(realisations), dict(tags), many, steps)
    assert all(kinds[k] >= 3 for k in sem.KINDS), kinds
    assert all(predictions[p] >= 10 for p in sem.PREDICTIONS), predictions
    assert 3 * many >= steps, (many, steps)
    assert all(realisations[r] >= 4 for r in sem.REALISATIONS), realisations
    for t in ("refit pending, then builder change", "rebuild pending, then same-shape edit", "edit moved and moved back"): assert tags[t] >= 1, (t, tags)
    # the variants inside a kind the suite names: both index widths, all four vertex streams, every refusal, both builder cases, a mirroring move
    edits = [e for seq in sequences.values() for st in seq for e in st.edits]
    start = sem.start_scene()                                            # (rows 0-4 are never dropped: row 1 has 16-bit indices, row 2 32-bit ones)
    assert start.buffers[start.instances[1].gpu.index_descriptor][1] == abi.FORMAT_R16_UINT and start.buffers[start.instances[2].gpu.index_descriptor][1] == abi.FORMAT_R32_UINT
    assert {1, 2} <= {e[1] for e in edits if e[0] == "f"}
    assert {e[2] for e in edits if e[0] == "g"} == {"tangent", "uv0", "uv1", "color"}
    assert {e[1] for e in edits if e[0] == "m"} == {"dead", "range", "material", "materials_short"}
    assert {e[3] for e in edits if e[0] == "b"} == {"move", "mirror", "there_and_back"}
    assert {e[1] for e in edits if e[0] == "j"} == {"drop", "add", "count"}
    assert {e[2] for e in edits if e[0] == "d"} == {"mask", "flags"} and {e[2] for e in edits if e[0] == "h"} == {"position", "uv0"}


def test_an_index_rewrite_permutes_triangles_and_corners_and_stays_in_range():
    idx = np.arange(30) % 17
    new = sem._permuted_indices(idx, 3)
    as_sets = lambda a: sorted(tuple(sorted(t)) for t in a.reshape(-1, 3).tolist())
    assert as_sets(new) == as_sets(idx) and not np.array_equal(new, idx) and new.max() <= idx.max()
    assert any(tuple(t) not in {tuple(np.roll(u, k)) for u in idx.reshape(-1, 3) for k in range(3)} for t in new.reshape(-1, 3))      # a winding flips


def test_a_buffer_two_rows_read_touches_both_and_one_nobody_reads_touches_none():
    m = sem.Model(abi.BUILDER_LBVH)
    assert m.realise("build_accel") == "build" and m.realise("build_accel") == "nothing"
    m.apply(("e", 3, 5))
    assert m.touched == {3, 4} and m.realise("trace") == "refit" and m.touched == {3, 4}
    m.apply(("n", 9)); m.apply(("c", 2, 1)); m.apply(("a",)); m.apply(("l", abi.BUILDER_LBVH))
    assert m.realise("accel_read") == "nothing"
    m.apply(("b", (1,), 4, "there_and_back"))
    assert m.touched == {1, 3, 4} and m.realise("focus_at") == "refit"
    m.apply(("d", 0, "flags", abi.INSTANCE_FLAG_FORCE_NON_OPAQUE)); m.apply(("l", abi.BUILDER_PLOC))
    assert m.realise("motion_snapshot") == "build" and m.touched == set() and m.snapshot_state() == abi.MOTION_SNAPSHOT_VALID
    m.apply(("j", "drop")); m.apply(("o", sem.POSE_TIMES[2]))
    assert m.snapshot_state() == abi.MOTION_SNAPSHOT_STALE and m.touched == set()          # the skinned row is gone: its outputs have no reader
    assert m.realise("build_accel") == "build" and (m.builds, m.refits) == (3, 2)
    m.apply(("o", sem.POSE_TIMES[3]))
    assert m.realise("build_accel") == "nothing"


@pytest.mark.parametrize("builder,seed", CASES[:4])
def test_replaying_a_sequence_gives_the_same_states(sequences, builder, seed):
    seq = sequences[(builder, seed)]
    assert seq == sem.sequence(seed, sem.STEPS, builder)
    a, b = sem.Model(builder), sem.Model(builder)
    for st in seq:
        for e in st.edits: a.apply(e); b.apply(e)
        assert a.realise(st.realise) == b.realise(st.realise) == st.predict
        assert a.state_bytes() == b.state_bytes()
    assert a.state_bytes() == sem.replay(builder, seq).state_bytes()


def test_a_refused_edit_leaves_every_table_and_buffer_unchanged(sequences):
    seen = 0
    for (builder, seed), seq in sequences.items():
        m = sem.Model(builder)
        for st in seq:
            for e in st.edits:
                before = m.state_bytes()
                ops = m.apply(e)
                if e[0] == "m":
                    seen += 1
                    assert m.state_bytes() == before and all(op[-1] == sem.ERR_BAD_HANDLE for op in ops) and len(ops) == 1
            m.realise(st.realise)
    assert seen >= 3


@pytest.fixture(scope="module")
def start(oracle_lib):
    s = sem.start_scene()
    o = oracle_lib.Oracle(); s.upload(o)
    yield s, o
    o.close()


@pytest.mark.parametrize("seed", sem.SEEDS)
def test_the_rays_hit_something_in_every_state(oracle_lib, start, sequences, seed):
    s, o0 = start
    rays = sem.make_rays(seed, o0, s)
    assert len(rays) >= 4000
    h = o0.intersect_many(rays)
    share = float((h[:, 0] > 0).mean())
    per_row = np.bincount(h[h[:, 0] > 0, 4].astype(np.int64), minlength=len(s.instances))
    print("seed", seed, "start: %.3f hit, per row" % share, per_row.tolist())
    assert share >= 0.5 and (per_row >= 10).all()
    worst = 1.0
    for builder in sem.BUILDERS:
        m = sem.Model(builder)
        for k, st in enumerate(sequences[(builder, seed)]):
            for e in st.edits: m.apply(e)
            m.realise(st.realise)
            o = oracle_lib.Oracle(); sem.load_fresh(o, m, False)
            share = float((o.intersect_many(rays)[:, 0] > 0).mean()); worst = min(worst, share)
            o.close()
            assert share >= 0.25, sem.describe(seed, builder, k, st)
    print("seed", seed, "worst later state: %.3f hit" % worst)


@pytest.mark.parametrize("builder,seed", [CASES[1], CASES[6], CASES[11]])
def test_a_state_loaded_at_once_renders_what_the_edited_oracle_renders(oracle_lib, sequences, builder, seed):
    """Model -> scenes.SceneData.upload -> oracle against the oracle that received the edits one by one through Live: the same frame, bit for bit,
    and the same streams.  The oracle rebuilds its tree for every trace, so this checks the model's bookkeeping of the DATA and the driver."""
    seq = sequences[(builder, seed)]
    m = sem.Model(builder)
    edited = oracle_lib.Oracle(); live = sem.Live(edited, m, False)
    s = m.scene
    for k, st in enumerate(seq):
        for e in st.edits: live.send(m.apply(e))
        m.realise(st.realise)
        if k % 5 != 4 and k != len(seq) - 1: continue
        fresh = oracle_lib.Oracle(); sem.load_fresh(fresh, m, False)
        a = np.zeros((s.height, s.width, 4), np.float32); b = np.zeros_like(a)
        edited.trace(s.settings, s.execute_params(k), a); fresh.trace(s.settings, s.execute_params(k), b)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), sem.describe(seed, builder, k, st)
        assert a[..., :3].std() > 0.01
        for local, (arr, _) in enumerate(m.scene.buffers):
            got = edited.buffer_read(live.bmap[local], arr.dtype, arr.size)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(arr).reshape(-1).view(np.uint8)), (local, sem.describe(seed, builder, k, st))
        fresh.close()
    edited.close()
