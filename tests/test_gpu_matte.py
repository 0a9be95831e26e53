"""ID mattes (include/mipt.h pt_set_matte, pt_matte_extract) on the MI355X, sample for sample against the oracle.

The scene is "confetti": 12 x 8 small quads, each its own instance with its own untextured material whose base colour k / 64 names it, no
environment map and an environment colour no quad has.  The oracle's HIT_KIND and COLOR debug frames, traced without accumulation, then give
every pixel-sample's material exactly and -- the mapping being 1:1 -- its instance; for a variant in which two instances share a material
the instance comes from the oracle's ray log.  tests/matte_ref.py restates the fold; everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes
from tests import adaptive_ref as ar
from tests import aov_ref as av
from tests import matte_ref as mr

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
W, H = 40, 24                      # 3 x 2 tiles, ragged in both directions
N = 8                              # frames
GX, GY = 12, 8                     # quads
ENV = (0.25, 0.5, 0.75)
POISON = 7.0
# Settled on the CPU oracle: at this distance a quad of side 1.2 is about 3.3 pixels wide and, over the 8 frames, 62 pixels see more than two
# ids, 499 exactly one, 194 a miss and a hit, and none more than four.
DISTANCE, SIDE, JITTER = 4.3, 1.2, 0.3
SHARED = (17, 18)                  # the variant: these two neighbouring instances share instance 17's material


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def color_of(m):
    return ((m % 8 + 1) / 64.0, (m // 8 % 8 + 1) / 64.0, (m // 64 + 1) / 64.0)


def confetti(shared=False):
    """Instance k = j * GX + i has material k + 1 (material 0 is the default material, which no instance uses)."""
    rng = np.random.default_rng(1)
    s = scenes.SceneData("confetti")
    for k in range(GX * GY):
        j, i = divmod(k, GX)
        mat = s.add_material(scenes.material(base_color_factor=color_of(k + 1) + (1.0,), flags=abi.MATERIAL_FLAG_DOUBLE_SIDED))
        c = np.array([i - GX / 2 + 0.5 + rng.uniform(-JITTER, JITTER), rng.uniform(-0.3, 0.3), j - GY / 2 + 0.5 + rng.uniform(-JITTER, JITTER)])
        a = rng.uniform(0, np.pi)
        du = SIDE * np.array([np.cos(a), 0, np.sin(a)]); dv = SIDE * np.array([-np.sin(a), 0, np.cos(a)])
        s.add_mesh(meshgen.grid(1, 1, c - 0.5 * du - 0.5 * dv, du, dv), None, SHARED[0] + 1 if shared and k == SHARED[1] else mat)
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0), DISTANCE, 0.0, 0.0)
    s.width, s.height = W, H
    st = copy_settings(s.settings)
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    st.min_bounces, st.max_bounces = 1, 2
    st.environment_color[:] = ENV
    st.max_accumulated_frames = 64
    s.settings = st
    return s


def single(st):
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE
    return s1


def oracle_rows(oracle_lib, s):
    """Per frame (H, W) int: the material-table row each pixel's sample sees, -1 for a miss (HIT_KIND and COLOR frames, no accumulation)."""
    o = oracle_lib.Oracle()
    s.upload(o)
    rows = []
    for f in range(N):
        img = {}
        for key, dbg in (("hk", abi.DEBUG_OUTPUT_HIT_KIND), ("col", abi.DEBUG_OUTPUT_COLOR)):
            sd = single(s.settings); sd.debug_output = dbg
            img[key] = np.zeros((H, W, 4), f32)
            o.trace(sd, s.execute_params(f), img[key])
        m = av.hit_mask(img["hk"], ENV)
        c = img["col"][..., :3] * f32(64)
        ci = np.rint(c).astype(np.int64)
        assert np.all(c[m] == ci[m]) and np.all(ci[m] >= 1) and np.all(ci[m] <= 8)       # a base colour exactly
        rows.append(np.where(m, (ci[..., 0] - 1) + (ci[..., 1] - 1) * 8 + (ci[..., 2] - 1) * 64, -1))
    o.close()
    return rows


def oracle_logged_instances(oracle_lib, s, picks):
    """{(y, x): [instance row or -1 per frame]} from the oracle's ray log: the camera ray's committed instance."""
    o = oracle_lib.Oracle()
    s.upload(o)
    s1 = single(s.settings)
    b = np.zeros((H, W, 4), f32)
    out = {}
    for (y, x) in picks:
        seq = []
        for f in range(N):
            o.set_window(x, y, x + 1, y + 1)
            o.ray_log(x, y)
            o.trace(s1, s.execute_params(f), b)
            log = o.read_ray_log()
            assert len(log) >= 1 and log[0, 8] == 0                     # the first logged ray is the camera ray, a closest-hit search
            seq.append(int(log[0, 11]) if log[0, 9] != 0 else -1)
        out[(y, x)] = seq
    o.ray_log(-1, 0); o.set_window()
    o.close()
    return out


def records(rows, table):
    """Rows (-1 = miss) -> uint32 records through a table of ids."""
    return [np.where(r >= 0, table[np.maximum(r, 0)], u32(0)).astype(u32) for r in rows]


class Ctx:
    def __init__(self, s, kind=None, K=6, ids=None, aov=False, poison=None, size=None):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        s.upload(self.r)
        w, h = size or (s.width, s.height)
        self.out = self.r.create_output(w, h)
        self.alb = self.nd = None
        if aov:
            self.alb, self.nd = self.r.create_output(w, h), self.r.create_output(w, h)
            self.r.set_aov(self.alb, self.nd)
        self.layers = [self.r.create_output(w, h) for _ in range(K // 2)]
        if poison is not None:
            for l in self.layers:
                l.fill_(poison)
        if kind is not None:
            self.r.set_matte(kind, self.layers, ids)

    def trace(self, st, frame, **kw):
        self.r.trace(st, self.s.execute_params(frame, **kw), self.out)

    def state(self):
        return mr.unpack([self.r.readback(l) for l in self.layers])

    def raw(self):
        return [self.r.readback(l) for l in self.layers]

    def close(self):
        self.r.close()


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(u32), b[1].view(u32))


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


@pytest.fixture(scope="module")
def data(oracle_lib):
    s = confetti()
    mat_rows = oracle_rows(oracle_lib, s)
    inst_rows = [np.where(r >= 0, r - 1, -1) for r in mat_rows]         # material k + 1 <-> instance k
    R = np.stack(inst_rows)
    distinct = np.array([[len(set(R[:, y, x].tolist()) - {-1}) for x in range(W)] for y in range(H)])
    mixed = (R < 0).any(axis=0) & (R >= 0).any(axis=0)
    print("pixels seeing > 2 ids: %d, exactly 1: %d, a miss and a hit: %d, most ids in a pixel: %d" % ((distinct > 2).sum(), (distinct == 1).sum(), mixed.sum(), distinct.max()))
    # the conditions on the inputs, on the oracle's data
    assert (distinct > 2).sum() >= 20 and (distinct == 1).sum() >= 20 and mixed.sum() >= 20 and distinct.max() <= 6
    tables = {mr.INSTANCE: mr.id_table(mr.INSTANCE, GX * GY), mr.MATERIAL: mr.id_table(mr.MATERIAL, GX * GY + 1)}
    rec = {mr.INSTANCE: records(inst_rows, tables[mr.INSTANCE]), mr.MATERIAL: records(mat_rows, tables[mr.MATERIAL])}
    d = dict(scene=s, st=copy_settings(s.settings), inst_rows=inst_rows, mat_rows=mat_rows, distinct=distinct, tables=tables, rec=rec, want={}, got={})

    def want(kind, K):
        if (kind, K) not in d["want"]:
            d["want"][(kind, K)] = mr.fold(rec[kind], K)
        return d["want"][(kind, K)]

    def got(kind, K):
        """The product's accumulation traced frame by frame: the state after every frame, the outputs and the stats."""
        if (kind, K) not in d["got"]:
            c = Ctx(s, kind, K)
            sa = copy_settings(d["st"]); sa.reset = 1
            c.r.reset_stats()
            states, outs = [], []
            for f in range(N):
                c.trace(sa, f); sa.reset = 0
                states.append(c.state()); outs.append(c.r.readback(c.out))
            d["got"][(kind, K)] = dict(states=states, outs=outs, stats=c.r.stats())
            c.close()
        return d["got"][(kind, K)]

    d["want_of"], d["got_of"] = want, got
    return d


@pytest.mark.parametrize("K", [6, 2])
@pytest.mark.parametrize("kind", [mr.INSTANCE, mr.MATERIAL], ids=["instance", "material"])
def test_layers_equal_the_fold_of_the_oracles_records_after_every_frame(data, kind, K):
    want, got = data["want_of"](kind, K), data["got_of"](kind, K)["states"]
    for n in range(N):
        assert same_state(got[n], want[n]), (n, int((got[n][0] != want[n][0]).sum()), int((got[n][1].view(u32) != want[n][1].view(u32)).sum()))
    ids, cov = got[N - 1]
    if K == 2:                                                           # the pixels with more than two ids dropped samples
        hit = np.stack([r >= 0 for r in data["inst_rows"]]).mean(axis=0)
        lost = cov.astype(np.float64).sum(axis=-1) < hit - 1e-3
        assert lost.sum() >= 20 and not np.any(lost & (data["distinct"] <= 2))
    else:
        assert np.array_equal((ids != 0).sum(axis=-1), data["distinct"])


def test_two_instances_with_one_material_are_told_apart_by_the_instance_kind(data, oracle_lib):
    s = confetti(shared=True)
    # at least 64 pixels over all six tiles, by position, and the pixels at which the 1:1 scene sees either of the two instances
    picks = {(y, x) for y in range(1, H, 3) for x in range(2, W, 4)}
    R = np.stack(data["inst_rows"])
    ys, xs = np.nonzero(np.isin(R, SHARED).any(axis=0))
    picks |= set(zip(ys.tolist(), xs.tolist()))
    picks = sorted(picks)
    tiles = {(y // 16, x // 16) for y, x in picks}
    assert len(picks) >= 64 and len(tiles) == 6
    truth = oracle_logged_instances(oracle_lib, s, picks)
    saw = set(v for seq in truth.values() for v in seq)
    assert SHARED[0] in saw and SHARED[1] in saw
    py, px = np.array([p[0] for p in picks]), np.array([p[1] for p in picks])
    seqs = np.array([truth[p] for p in picks]).T                        # (N, picks)
    c = {kind: Ctx(s, kind, 6) for kind in (mr.INSTANCE, mr.MATERIAL)}
    want_i = mr.fold(records(list(seqs), data["tables"][mr.INSTANCE]), 6)
    mat_of = np.arange(GX * GY) + 1
    mat_of[SHARED[1]] = SHARED[0] + 1
    want_m = mr.fold(records([np.where(q >= 0, mat_of[np.maximum(q, 0)], -1) for q in seqs], data["tables"][mr.MATERIAL]), 6)
    sa = copy_settings(data["st"]); sa.reset = 1
    for f in range(N):
        for kind, want in ((mr.INSTANCE, want_i), (mr.MATERIAL, want_m)):
            c[kind].trace(sa, f)
            ids, cov = c[kind].state()
            assert same_state((ids[py, px], cov[py, px]), want[f]), (kind, f)
        sa.reset = 0
    # a pixel that saw both instances holds two instance ids and one material id
    both = np.array([SHARED[0] in truth[p] and SHARED[1] in truth[p] for p in picks])
    assert both.any()
    ti, tm = data["tables"][mr.INSTANCE], data["tables"][mr.MATERIAL]
    ids_i, ids_m = c[mr.INSTANCE].state()[0][py, px], c[mr.MATERIAL].state()[0][py, px]
    assert np.all((ids_i[both] == ti[SHARED[0]]).any(axis=-1) & (ids_i[both] == ti[SHARED[1]]).any(axis=-1))
    assert np.all((ids_m[both] == tm[SHARED[0] + 1]).any(axis=-1)) and not np.any(ids_m == tm[SHARED[1] + 1])
    for x in c.values():
        x.close()


def test_two_batches_of_four_equal_the_eight_frames_and_a_call_without_accumulation_holds_one_sample(data):
    s, kind, K = data["scene"], mr.INSTANCE, 6
    want = data["got_of"](kind, K)
    c = Ctx(s, kind, K)
    c.r.set_samples_per_trace(4)
    sa = copy_settings(data["st"]); sa.reset = 1
    for f in (0, 4):
        c.trace(sa, f); sa.reset = 0
        assert same_state(c.state(), want["states"][f + 3]), f
        assert np.array_equal(bits(c.r.readback(c.out)), bits(want["outs"][f + 3]))
    c.r.set_samples_per_trace(1)
    c.trace(single(data["st"]), 5)
    ids, cov = c.state()
    h = data["rec"][kind][5]
    assert np.array_equal(ids[..., 0], h) and np.array_equal(cov[..., 0], (h != 0).astype(f32))
    assert np.all(ids[..., 1:] == 0) and np.all(cov[..., 1:].view(u32) == 0)
    c.close()


def test_mattes_change_nothing_else_and_nothing_is_written_when_they_are_off_or_the_call_has_a_debug_output(data):
    s, st = data["scene"], data["st"]
    runs = {}
    for on in (True, False):
        c = Ctx(s, mr.INSTANCE if on else None, 6, aov=True, poison=POISON)
        sa = copy_settings(st); sa.reset = 1
        c.r.reset_stats()
        snaps = []
        for f in range(N):
            c.trace(sa, f); sa.reset = 0
            snaps.append([c.r.readback(t) for t in (c.out, c.alb, c.nd)])
        runs[on] = (snaps, c.r.stats(), c.raw())
        if on:                                                            # a debug-output call leaves poisoned layers untouched
            for l in c.layers:
                l.fill_(POISON)
            sd = copy_settings(st); sd.debug_output = abi.DEBUG_OUTPUT_COLOR; sd.reset = 1
            c.trace(sd, 0)
            assert all(np.all(x == POISON) for x in c.raw())
        c.close()
    for f in range(N):
        for a, b in zip(runs[True][0][f], runs[False][0][f]):
            assert np.array_equal(bits(a), bits(b)), f
    for name in ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames"):
        assert getattr(runs[True][1], name) == getattr(runs[False][1], name), name
    assert runs[True][1].accumulated_frames == N
    assert all(np.all(x == POISON) for x in runs[False][2])              # mattes off: the poison stays
    assert same_state(mr.unpack(runs[True][2]), data["want_of"](mr.INSTANCE, 6)[N - 1])


def test_two_tile_shards_write_their_own_tiles_and_pack_to_the_one_rank_layers(data):
    s, kind, K, ranks, frames = data["scene"], mr.MATERIAL, 6, 2, 4
    want = mr.pack(*data["want_of"](kind, K)[frames - 1])
    ty, tx = (H + 15) // 16, (W + 15) // 16
    root = Ctx(s)
    whole = [root.r.create_output(W, H) for _ in range(K // 2)]
    for k in range(ranks):
        c = Ctx(s, kind, K, poison=POISON)
        sa = copy_settings(data["st"]); sa.reset = 1
        for f in range(frames):
            c.trace(sa, f, tile_rank=k, tile_rank_count=ranks); sa.reset = 0
        for j, img in enumerate(c.raw()):
            for g in range(ty * tx):
                y, x = divmod(g, tx)
                if g % ranks == k:
                    assert np.array_equal(bits(ar.tile_view(img, y, x)), bits(ar.tile_view(want[j], y, x))), (k, j, g)
                else:
                    assert np.all(ar.tile_view(img, y, x) == POISON), (k, j, g)
        for l, into in zip(c.layers, whole):                              # a layer travels as any float4 image: the bits survive
            packed = c.r.tiles_pack(l, k, ranks)
            root.r.tiles_unpack(packed.clone(), into, k, ranks)
        c.r.readback(c.out)                                              # the pack has run before the context goes
        c.close()
    for into, w in zip(whole, want):
        assert np.array_equal(bits(root.r.readback(into)), bits(w))
    root.close()


def test_adaptive_tiles_hold_the_uniform_mattes_at_their_own_count(data):
    s, st, kind, K = data["scene"], data["st"], mr.INSTANCE, 6
    want = data["want_of"](kind, K)
    c = Ctx(s, kind, K, poison=POISON)
    raw = []
    for f in range(N):                                                    # the threshold: the median tile error after four uniform samples
        c.trace(single(st), f)
        raw.append(c.r.readback(c.out))
    I, A = ar.fold(raw)
    E4 = ar.tile_errors(I[3], A[3])
    pos = np.sort(E4[E4 > 0].ravel())
    thr = float(pos[len(pos) // 2])
    spp = 2
    c.r.set_samples_per_trace(spp)
    c.r.set_adaptive(2, N, thr)
    frame, active = 0, 1
    while active and frame < N:
        c.trace(st, frame)
        frame += spp
        active, samples, _, _ = c.r.adaptive_read(W, H)
    assert len(set(samples.ravel().tolist())) >= 2, samples              # some tiles retired early, some did not
    got = c.raw()
    for y, x in np.ndindex(samples.shape):
        n = int(samples[y, x])
        for j, w in enumerate(mr.pack(*want[n - 1])):
            assert np.array_equal(bits(ar.tile_view(got[j], y, x)), bits(ar.tile_view(w, y, x))), (y, x, n, j)
    c.close()


def test_save_destroy_create_set_matte_load_continue_equals_the_uninterrupted_run(data):
    import torch
    from gltf_renderer_amd.renderer import MiptError
    s, st, kind, K = data["scene"], data["st"], mr.MATERIAL, 6
    want = data["got_of"](kind, K)
    a = Ctx(s, kind, K)
    sa = copy_settings(st); sa.reset = 1
    for f in range(4):
        a.trace(sa, f); sa.reset = 0
    blob = a.r.accum_save(W, H, a.out, next_frame=4)
    saved = a.raw()
    a.r.set_matte(kind, a.layers)                                        # a good config: a restart is pending until the next trace ...
    with pytest.raises(MiptError, match="^-6"):                           # ... and pt_accum_save answers PT_ERR_NOT_READY
        a.r.accum_save(W, H, a.out, next_frame=4)
    a.close()
    b = Ctx(s)                                                            # the layers are the caller's: restored bits, set before the load
    b.layers = [torch.from_numpy(x.copy()).to(b.out.device) for x in saved]
    b.r.set_matte(kind, b.layers)
    info = b.r.accum_load(blob, b.out)
    assert info.accumulated_frames == 4 and info.next_frame == 4
    for f in range(4, N):
        b.trace(sa, f)
        assert same_state(b.state(), want["states"][f]), f
        assert np.array_equal(bits(b.r.readback(b.out)), bits(want["outs"][f])), f
    assert b.r.stats().accumulated_frames == N
    b.close()


def test_a_bake_holds_the_covering_instance_at_full_coverage_and_zeros_where_nothing_covers():
    A = 32
    s = scenes.SceneData("matte_bake")
    up = np.repeat([[0.0, 0.0, 1.0]], 4, axis=0)
    for x0, u0 in ((-2.0, 0.06), (0.5, 0.56)):                          # two quads side by side, charts in the left and the right half
        uv = np.array([(u0, 0.9), (u0 + 0.38, 0.9), (u0 + 0.38, 0.1), (u0, 0.1)], np.float64)
        s.add_mesh(meshgen.Mesh([(x0, -1, 0), (x0 + 1.5, -1, 0), (x0 + 1.5, 1, 0), (x0, 1, 0)], [0, 1, 2, 0, 2, 3], normals=up, uv0=uv))
    st = abi.PtSettings.app_defaults()
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    st.environment_color[:] = ENV
    st.max_accumulated_frames = 64
    s.settings = st
    s.world_to_view = np.eye(4)
    s.width = s.height = A
    table = mr.id_table(mr.INSTANCE, 2)
    for spp in (1, 4):
        c = Ctx(s, mr.INSTANCE, 4, poison=POISON)
        c.r.set_bake(1.0 / 64)
        c.r.set_samples_per_trace(spp)
        sa = copy_settings(st); sa.reset = 1
        c.trace(sa, 0)
        inst, _ = c.r.bake_coverage(A, A)
        covered = inst >= 0
        assert set(np.unique(inst).tolist()) == {-1, 0, 1} and covered.sum() > A * A // 4 and (~covered).sum() > A * A // 8
        ids, cov = c.state()
        assert np.array_equal(ids[..., 0][covered], table[inst[covered]]) and np.all(cov[..., 0][covered] == f32(1))
        assert np.all(ids[..., 1:][covered] == 0) and np.all(cov[..., 1:][covered].view(u32) == 0)
        assert all(np.all(bits(l)[~covered] == 0) for l in c.raw()), spp
        c.close()


def test_user_ids_name_the_first_rows_and_the_rest_keep_their_default_names(data):
    s, K, frames = data["scene"], 6, 3
    half = GX * GY // 2
    user = [5, 0x7f800000, 0xffffffff, 0x3f800000] + [0x40000000 + 977 * i for i in range(4, half)]    # the first three need the fix
    table = mr.id_table(mr.INSTANCE, GX * GY, user)
    assert table[0] == 5 ^ (1 << 23) and table[3] == 0x3f800000 and table[half] == mr.default_id(mr.INSTANCE, half) and len(set(table.tolist())) == GX * GY
    want = mr.fold(records(data["inst_rows"][:frames], table), K)
    c = Ctx(s, mr.INSTANCE, K, ids=user)
    sa = copy_settings(data["st"]); sa.reset = 1
    for f in range(frames):
        c.trace(sa, f); sa.reset = 0
        assert same_state(c.state(), want[f]), f
    seen = set(c.state()[0].ravel().tolist())
    assert len(seen & set(table[:half].tolist())) >= 10 and len(seen & set(table[half:].tolist())) >= 10
    c.close()


def test_extract_is_the_sequential_sum_of_the_matching_ranks(data):
    s, kind, K = data["scene"], mr.INSTANCE, 6
    table = data["tables"][kind]
    c = Ctx(s, kind, K)
    sa = copy_settings(data["st"]); sa.reset = 1
    for f in range(N):
        c.trace(sa, f); sa.reset = 0
    ids, cov = c.state()
    # three neighbouring quads in the middle of the picture
    pick = [int(table[k]) for k in (4 * GX + 5, 4 * GX + 6, 3 * GX + 5)]
    got = c.r.matte_extract(c.layers, pick).cpu().numpy()
    want = mr.extract(ids, cov, pick)
    assert np.array_equal(got.view(u32), want.view(u32)) and (want > 0).sum() >= 20 and (want == 0).sum() >= 20
    # the set goes through the fix: an unfixed id selects the fixed one
    got5 = c.r.matte_extract(c.layers, [5]).cpu().numpy()
    assert np.array_equal(got5.view(u32), mr.extract(ids, cov, [5]).view(u32))
    # all ids, 64 at a time: nothing was dropped at K = 6, so a pixel's masks are both 0 exactly where every frame missed
    m0 = c.r.matte_extract(c.layers, table[:64]).cpu().numpy()
    m1 = c.r.matte_extract(c.layers, table[64:]).cpu().numpy()
    all_missed = np.stack([r < 0 for r in data["inst_rows"]]).all(axis=0)
    assert np.array_equal((m0 == 0) & (m1 == 0), all_missed) and all_missed.sum() >= 20
    assert np.array_equal(m0.view(u32), mr.extract(ids, cov, table[:64]).view(u32))
    # a K = 2 view of the same layers reads the first layer only
    g2 = c.r.matte_extract(c.layers[:1], pick).cpu().numpy()
    assert np.array_equal(g2.view(u32), mr.extract(ids[..., :2], cov[..., :2], pick).view(u32))
    c.close()


def test_refusals_name_the_field_and_leave_everything_as_it_was(data):
    s, st = data["scene"], data["st"]
    c = Ctx(s, mr.INSTANCE, 4, poison=POISON)
    r, L = c.r, c.r.L
    sa = copy_settings(st); sa.reset = 1
    c.trace(sa, 0); sa.reset = 0                                          # the good config is in use; no restart is pending
    good = c.state()

    def cfg(enable=1, kind=0, ranks=4, id_count=0, layers=(0, 1)):
        q = abi.PtMatteConfig(enable, kind, ranks, id_count)
        for j in layers:
            q.layers[j] = c.layers[j % 2].data_ptr()
        return q

    some = np.array([1, 2], u32)
    for q, ids, word in ((cfg(kind=2), None, "kind"), (cfg(kind=-1), None, "kind"), (cfg(ranks=3), None, "ranks"), (cfg(ranks=10), None, "ranks"),
                         (cfg(ranks=0), None, "ranks"), (cfg(layers=(0,)), None, "layers[1]"), (cfg(ranks=8, layers=(0, 1, 3)), None, "layers[2]"),
                         (cfg(id_count=-1), some, "id_count"), (cfg(id_count=2), None, "ids")):
        rc = L.pt_set_matte(r.h, C.byref(q), ids.ctypes.data_as(C.c_void_p) if ids is not None else None)
        assert rc == -1 and word in L.pt_last_error(r.h).decode(), (word, rc, L.pt_last_error(r.h).decode())
    assert L.pt_set_matte(r.h, None, None) == -1 and "config" in L.pt_last_error(r.h).decode()
    # the old config stays and no restart is pending: the accumulation can be saved and goes on
    r.accum_save(W, H, c.out)
    c.trace(sa, 1)
    assert r.stats().accumulated_frames == 2 and not same_state(c.state(), good)
    assert same_state(c.state(), data["want_of"](mr.INSTANCE, 4)[1])
    # a disabled config is not looked at any further
    assert L.pt_set_matte(r.h, C.byref(cfg(enable=0, kind=9, ranks=9, id_count=-4, layers=())), None) == 0
    assert L.pt_set_matte(r.h, C.byref(cfg()), None) == 0
    # the megakernel: refused, the output and the layers untouched
    r.set_kernel_mode(abi.MODE_MEGAKERNEL)
    c.out.fill_(POISON)
    for l in c.layers:
        l.fill_(POISON)
    p = s.execute_params(0)
    p.output = c.out.data_ptr()
    for sx in (sa, single(st)):
        assert L.pt_trace(r.h, C.byref(sx), C.byref(p)) == -1 and "wavefront" in L.pt_last_error(r.h).decode()
    assert np.all(r.readback(c.out) == POISON) and all(np.all(x == POISON) for x in c.raw())
    r.set_kernel_mode(abi.MODE_WAVEFRONT)
    # pt_matte_extract
    mask = r.torch.full((H, W), POISON, dtype=r.torch.float32, device=c.out.device)
    ptrs = (C.c_void_p * 2)(*[l.data_ptr() for l in c.layers])
    ids = np.arange(1, 66, dtype=u32)

    def extract(layers=ptrs, ranks=4, w=W, h=H, idp=ids.ctypes.data_as(C.c_void_p), n=3, m=C.c_void_p(mask.data_ptr())):
        return L.pt_matte_extract(r.h, layers, ranks, w, h, idp, n, m)

    assert extract() == 0
    mask.fill_(POISON)
    for kw in (dict(ranks=3), dict(ranks=0), dict(ranks=10), dict(n=0), dict(n=65), dict(n=-1), dict(w=0), dict(h=0), dict(layers=None), dict(idp=None), dict(m=None),
               dict(layers=(C.c_void_p * 2)(c.layers[0].data_ptr(), None))):
        assert extract(**kw) == -1, kw
    assert bool((mask == POISON).all())
    c.close()
