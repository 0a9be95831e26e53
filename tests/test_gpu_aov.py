"""First-hit AOVs (include/mipt.h pt_set_aov) on the MI355X, sample for sample against the oracle.

The oracle renders the same first-vertex values as debug outputs: HIT_KIND tells hits from misses (the scenes have no environment map
and an environment colour no debug colour takes), COLOR is the albedo, SHADING_NORMAL the encoded normal (n + 1) / 2, and its ray log
holds the primary ray's t.  tests/aov_ref.py restates the per-sample rules and the fold; nothing here is compared with a tolerance except
the decoded normal, whose bound 2^-23 is the two roundings of the oracle's encoding (tests/test_aov_host.py derives it)."""
import ctypes as C

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes
from tests import adaptive_ref as ar
from tests import aov_ref as av

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H = 72, 40                      # 5 x 3 tiles, ragged in both directions
N = 8                              # frames of the accumulations below
ENV = (0.25, 0.5, 0.75)            # no debug output shows this colour at a hit of these scenes
POISON = 7.0
DEBUGS = dict(hk=abi.DEBUG_OUTPUT_HIT_KIND, col=abi.DEBUG_OUTPUT_COLOR, nrm=abi.DEBUG_OUTPUT_SHADING_NORMAL)


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def small_scene():
    """test_scene without an environment map from a distance at which about a quarter of the picture is geometry: tiles of sky only,
    a tile nearly full of hits, silhouettes in between."""
    s = scenes.test_scene(W, 16, with_env=False)
    s.width, s.height = W, H
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.6), 5.0, 0.35, -0.45)
    s.settings.environment_color[:] = ENV
    s.settings.max_accumulated_frames = 64
    return s


class Ctx:
    def __init__(self, s, aov=True, albedo=True, normal_depth=True):
        from gltf_renderer_amd.renderer import Renderer
        self.s = s
        self.r = Renderer(0)
        s.upload(self.r)
        self.out = self.r.create_output(s.width, s.height)
        self.alb = self.r.create_output(s.width, s.height) if aov and albedo else None
        self.nd = self.r.create_output(s.width, s.height) if aov and normal_depth else None
        if aov:
            self.r.set_aov(self.alb, self.nd)

    def trace(self, st, frame, **kw):
        self.r.trace(st, self.s.execute_params(frame, **kw), self.out)

    def read(self):
        return tuple(self.r.readback(t) if t is not None else None for t in (self.out, self.alb, self.nd))

    def close(self):
        self.r.close()


def oracle_frames(oracle_lib, s, st, frames):
    """The oracle's HIT_KIND, COLOR and SHADING_NORMAL frames 0 .. frames - 1, traced without accumulation, and the hit masks."""
    o = oracle_lib.Oracle()
    s.upload(o)
    d = dict(hk=[], col=[], nrm=[])
    for f in range(frames):
        for key, dbg in DEBUGS.items():
            sd = copy_settings(st); sd.flags &= ~abi.FLAG_ACCUMULATE; sd.debug_output = dbg
            b = np.zeros((s.height, s.width, 4), f32)
            o.trace(sd, s.execute_params(f), b)
            d[key].append(b)
    d["mask"] = [av.hit_mask(b, ENV) for b in d["hk"]]
    o.close()
    return d


def product_runs(s, st, frames):
    """The product's single-sample targets (accumulation off, frame by frame) and the snapshots of an accumulation traced frame by frame;
    entry [k] of each list is (output, albedo, normal_depth) as numpy arrays.  Also the stats after the accumulation."""
    a = Ctx(s)
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE
    single = []
    for f in range(frames):
        a.trace(s1, f)
        single.append(a.read())
    a.close()
    b = Ctx(s)
    sa = copy_settings(st); sa.reset = 1
    acc = []
    b.r.reset_stats()
    for f in range(frames):
        b.trace(sa, f); sa.reset = 0
        acc.append(b.read())
    stats = b.r.stats()
    b.close()
    return single, acc, stats


def check_albedo(acc, orc, frames):
    """Item 1: the accumulated albedo target, all four channels, against the fold of the oracle's COLOR frames and hit masks."""
    want = av.fold([av.albedo_record(orc["col"][f], orc["mask"][f]) for f in range(frames)])
    for n in range(frames):
        got = acc[n][1]
        assert same(got, want[n]), (n, int((bits(got) != bits(want[n])).sum()))
    # the coverage channel is the running mean of the hit mask (the fold of 1 where hit, 0 where miss)
    cov = av.fold([np.repeat(m[..., None].astype(f32), 4, axis=-1) for m in orc["mask"][:frames]])
    assert same(acc[frames - 1][1][..., 3], cov[frames - 1][..., 3])


def check_normals(single, orc, frames):
    """Item 2: every single-sample normal against the oracle's encoded frame -- decoded within 2^-23, re-encoded bit-equal; zeros at a miss."""
    for f in range(frames):
        nd, c, m = single[f][2], orc["nrm"][f][..., :3], orc["mask"][f]
        xyz = nd[..., :3]
        err = np.abs(xyz.astype(np.float64) - av.decode_normal(c).astype(np.float64))
        assert np.all(err[m] <= 2.0 ** -23), (f, float(err[m].max()))
        assert same(av.encode_normal(xyz)[m], c[m]), (f, int((bits(av.encode_normal(xyz)[m]) != bits(c[m])).any(axis=-1).sum()))
        assert np.all(bits(nd[~m]) == 0), f                        # a miss: all four components +0
        assert np.all(nd[m][:, 3] > 0), f                          # a hit has a positive distance


def hit_and_miss_shares(orc, frames):
    m = np.stack(orc["mask"][:frames])
    return float(m.mean()), float((~m).mean())


@pytest.fixture(scope="module")
def data(oracle_lib):
    s = small_scene()
    st = copy_settings(s.settings)
    orc = oracle_frames(oracle_lib, s, st, N)
    single, acc, stats = product_runs(s, st, N)
    return dict(scene=s, st=st, orc=orc, single=single, acc=acc, stats=stats)


def test_hits_and_misses_each_make_up_a_tenth_of_the_samples(data):
    hit, miss = hit_and_miss_shares(data["orc"], N)
    print("hit share %.3f, miss share %.3f" % (hit, miss))
    assert hit >= 0.10 and miss >= 0.10, (hit, miss)


def test_albedo_equals_the_fold_of_the_oracles_color_frames_bit_for_bit(data):
    check_albedo(data["acc"], data["orc"], N)
    # a single sample is the record itself
    for f in range(N):
        assert same(data["single"][f][1], av.albedo_record(data["orc"]["col"][f], data["orc"]["mask"][f])), f


def test_single_sample_normals_against_the_oracles_encoded_frames(data):
    check_normals(data["single"], data["orc"], N)


def test_accumulated_normal_depth_is_the_fold_of_the_single_samples(data):
    want = av.fold([data["single"][f][2] for f in range(N)])
    for n in range(N):
        assert same(data["acc"][n][2], want[n]), n


def depth_pixels(mask):
    """At least 24 pixels: eight from a tile without a hit, eight from the tile with the most hits, eight from silhouette tiles (hits and
    misses both), chosen by position only."""
    ty, tx = (H + 15) // 16, (W + 15) // 16
    pad = np.zeros((ty * 16, tx * 16), bool)
    pad[:H, :W] = mask
    count = pad.reshape(ty, 16, tx, 16).sum(axis=(1, 3))
    inside = ar.tile_pixels(W, H)
    tiles = [(y, x) for y in range(ty) for x in range(tx)]
    empty = [t for t in tiles if count[t] == 0 and inside[t] == 256]
    full = max(tiles, key=lambda t: count[t])
    sil = [t for t in tiles if 16 <= count[t] <= inside[t] - 16 and t != full]
    assert empty and sil and count[full] >= 128, count
    picks = []
    for cls in ([empty[0]], [full], sil):
        cand = [(y * 16 + j, x * 16 + i) for (y, x) in cls for j in range(1, 16, 3) for i in range(2, 16, 3) if y * 16 + j < H and x * 16 + i < W]
        step = max(len(cand) // 8, 1)
        picks += cand[::step][:8]
    # silhouette pixels proper: hit pixels with a miss beside them, and the other way round
    edge = mask[:, 1:] != mask[:, :-1]
    ys, xs = np.nonzero(edge)
    for k in range(0, len(ys), max(len(ys) // 8, 1)):
        picks += [(int(ys[k]), int(xs[k])), (int(ys[k]), int(xs[k]) + 1)]
    return sorted(set(picks))


def test_depth_equals_the_oracles_logged_primary_ray_bit_for_bit(data, oracle_lib):
    s, st, frames = data["scene"], data["st"], 4
    picks = depth_pixels(data["orc"]["mask"][0])
    assert len(picks) >= 24
    o = oracle_lib.Oracle()
    s.upload(o)
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE
    b = np.zeros((H, W, 4), f32)
    n_hit = n_miss = 0
    for (y, x) in picks:
        ts = []
        for f in range(frames):
            o.set_window(x, y, x + 1, y + 1)
            o.ray_log(x, y)
            o.trace(s1, s.execute_params(f), b)
            log = o.read_ray_log()
            assert len(log) >= 1 and log[0, 8] == 0                  # the first logged ray is the camera ray, a closest-hit search
            committed = log[0, 9] != 0
            assert committed == bool(data["orc"]["mask"][f][y, x]), (x, y, f)
            t = f32(log[0, 10]) if committed else f32(0)
            n_hit += int(committed); n_miss += int(not committed)
            got = data["single"][f][2][y, x, 3]
            assert bits(got) == bits(t), (x, y, f, float(got), float(t))
            ts.append(np.array([0, 0, 0, t], f32))
        want = av.fold(ts)[frames - 1][3]
        got = data["acc"][frames - 1][2][y, x, 3]
        assert bits(got) == bits(want), (x, y, float(got), float(want))
    o.ray_log(-1, 0); o.set_window()
    o.close()
    assert n_hit >= 16 and n_miss >= 16, (n_hit, n_miss)


def test_the_output_ray_counts_and_frame_count_are_those_of_a_context_without_aovs(data):
    s, st = data["scene"], data["st"]
    c = Ctx(s, aov=False)
    sa = copy_settings(st); sa.reset = 1
    c.r.reset_stats()
    for f in range(N):
        c.trace(sa, f); sa.reset = 0
        assert same(c.read()[0], data["acc"][f][0]), f
    q, p = c.r.stats(), data["stats"]
    for name in ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "texture_taps", "accumulated_frames"):
        assert getattr(q, name) == getattr(p, name), (name, getattr(q, name), getattr(p, name))
    assert q.accumulated_frames == N
    # and the single samples without accumulation
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE
    for f in (0, 5):
        c.trace(s1, f)
        assert same(c.read()[0], data["single"][f][0]), f
    c.close()


@pytest.mark.parametrize("spp", [1, 3, 8])
def test_sample_batches_give_the_aovs_of_the_calls_one_by_one(data, spp):
    s = data["scene"]
    st = copy_settings(data["st"]); st.max_accumulated_frames = N      # 3 + 3 + 2: the last batch is clamped
    c = Ctx(s)
    c.r.set_samples_per_trace(spp)
    frame = 0
    while frame < N:
        c.trace(st, frame)
        frame = min(frame + spp, N)
        out, alb, nd = c.read()
        assert same(out, data["acc"][frame - 1][0]) and same(alb, data["acc"][frame - 1][1]) and same(nd, data["acc"][frame - 1][2]), (spp, frame)
    assert c.r.stats().accumulated_frames == N
    before = c.read()
    c.trace(st, frame)                                                  # past max_accumulated_frames: a no-op for the targets too
    assert all(same(x, y) for x, y in zip(c.read(), before))
    c.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_tile_shards_assemble_to_the_one_rank_aovs(data, ranks):
    import torch
    s, st = data["scene"], data["st"]
    frames = 4
    ctxs = []
    for k in range(ranks):
        c = Ctx(s)
        c.r.exchange_create_loopback(k, ranks, 7000 + ranks)
        c.alb.fill_(POISON); c.nd.fill_(POISON)
        ctxs.append(c)
    sa = copy_settings(st); sa.reset = 1
    for f in range(frames):
        for k, c in enumerate(ctxs):
            c.trace(sa, f, tile_rank=k, tile_rank_count=ranks)
        sa.reset = 0
    ty, tx = (H + 15) // 16, (W + 15) // 16
    for k, c in enumerate(ctxs):                                         # a rank writes its own tiles only
        _, alb, nd = c.read()
        for g in range(ty * tx):
            y, x = divmod(g, tx)
            for img, want in ((alb, data["acc"][frames - 1][1]), (nd, data["acc"][frames - 1][2])):
                if g % ranks == k:
                    assert same(ar.tile_view(img, y, x), ar.tile_view(want, y, x)), (k, g)
                else:
                    assert np.all(ar.tile_view(img, y, x) == POISON), (k, g)
    dst = ranks - 1
    order = [k for k in range(ranks) if k != dst] + [dst]                # posted transfers: the root is called last
    frames_alb = [c.r.create_output(W, H) for c in ctxs]
    frames_nd = [c.r.create_output(W, H) for c in ctxs]
    for k in order:                                                      # one exchange per target
        ctxs[k].r.exchange_frame(ctxs[k].alb, frames_alb[k], mode=abi.EXCHANGE_GATHER, dst=dst)
    for k in order:
        ctxs[k].r.exchange_frame(ctxs[k].nd, frames_nd[k], mode=abi.EXCHANGE_GATHER, dst=dst)
    torch.cuda.synchronize()
    root = ctxs[dst].r
    assert same(root.readback(frames_alb[dst]), data["acc"][frames - 1][1])
    assert same(root.readback(frames_nd[dst]), data["acc"][frames - 1][2])
    for c in ctxs:
        c.r.exchange_destroy(); c.close()


def test_adaptive_tiles_hold_the_uniform_aovs_at_their_own_count_and_retired_tiles_are_not_written(data):
    s, st = data["scene"], data["st"]
    raw = [x[0] for x in data["single"]]
    I, A = ar.fold(raw)
    E4 = ar.tile_errors(I[3], A[3])
    pos = np.sort(E4[E4 > 0].ravel())
    thr = float(pos[len(pos) // 2])                                       # retires some of the varying tiles early, the sky tiles at once
    spp, min_s = 2, 2

    def run(c, poison_at=None):
        c.r.set_samples_per_trace(spp)
        c.r.set_adaptive(min_s, N, thr)
        frame, active, poisoned = 0, 1, None
        while active and frame < N:
            c.trace(st, frame)
            frame += spp
            active, samples, _, _ = c.r.adaptive_read(W, H)
            if poison_at == frame:
                retired = samples < frame
                assert retired.any() and not retired.all(), samples
                for y, x in zip(*np.nonzero(retired)):
                    for t in (c.alb, c.nd):
                        t[y * 16:(y + 1) * 16, x * 16:(x + 1) * 16] = POISON
                poisoned = retired
        return c.r.adaptive_read(W, H)[1], poisoned

    c = Ctx(s)
    samples, _ = run(c)
    _, alb, nd = c.read()
    assert len(set(samples.ravel().tolist())) >= 2, samples
    for y, x in np.ndindex(samples.shape):
        n = int(samples[y, x])
        assert same(ar.tile_view(alb, y, x), ar.tile_view(data["acc"][n - 1][1], y, x)), (y, x, n)
        assert same(ar.tile_view(nd, y, x), ar.tile_view(data["acc"][n - 1][2], y, x)), (y, x, n)
    # the same run again (pt_set_adaptive restarts it), the tiles retired after the second call poisoned
    samples2, poisoned = run(c, poison_at=2 * spp)
    assert np.array_equal(samples2, samples) and poisoned is not None
    _, alb, nd = c.read()
    for y, x in np.ndindex(samples.shape):
        n = int(samples[y, x])
        for img, k in ((alb, 1), (nd, 2)):
            if poisoned[y, x]:
                assert np.all(ar.tile_view(img, y, x) == POISON), (y, x)
            else:
                assert same(ar.tile_view(img, y, x), ar.tile_view(data["acc"][n - 1][k], y, x)), (y, x, n)
    c.close()


def test_resets_restart_the_output_and_the_aovs_together(data):
    s, st = data["scene"], data["st"]
    acc, single = data["acc"], data["single"]
    c = Ctx(s)

    def expect(n):
        got = c.read()
        assert all(same(g, w) for g, w in zip(got, acc[n - 1])), n

    sa = copy_settings(st)
    for f in range(3):
        c.trace(sa, f)
    expect(3)
    # settings.reset
    sa.reset = 1
    c.trace(sa, 0); sa.reset = 0
    expect(1)
    c.trace(sa, 1)
    expect(2)
    # a camera change, and back: each starts a new accumulation in all three images
    p = s.execute_params(0)
    p.world_to_view[:] = camera.cm(camera.orbit_world_to_view((0, 0, 0.6), 4.2, 0.35, -0.45))
    c.r.trace(sa, p, c.out)
    moved = c.read()
    assert not same(moved[1], acc[0][1]) and c.r.stats().accumulated_frames == 1
    c.trace(sa, 0)
    expect(1)
    c.trace(sa, 1)
    expect(2)
    # pt_set_aov: new targets start from scratch, the output with them
    alb2, nd2 = c.r.create_output(W, H), c.r.create_output(W, H)
    alb2.fill_(POISON); nd2.fill_(POISON)
    old = c.read()
    c.r.set_aov(alb2, nd2)
    c.trace(sa, 0)
    assert same(c.r.readback(c.out), acc[0][0]) and same(c.r.readback(alb2), acc[0][1]) and same(c.r.readback(nd2), acc[0][2])
    assert same(c.r.readback(c.alb), old[1]) and same(c.r.readback(c.nd), old[2])       # the former targets are no longer written
    c.alb, c.nd = alb2, nd2
    c.trace(sa, 1)
    expect(2)
    # a debug-output call leaves the targets untouched
    sd = copy_settings(st); sd.debug_output = abi.DEBUG_OUTPUT_COLOR; sd.reset = 1
    before = c.read()
    c.trace(sd, 0)
    after = c.read()
    assert same(after[1], before[1]) and same(after[2], before[2]) and not same(after[0], before[0])
    # without FLAG_ACCUMULATE a target holds the one sample
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE
    c.trace(s1, 5)
    assert all(same(g, w) for g, w in zip(c.read(), single[5]))
    # AOVs off: the targets stay as they are, the output restarts
    c.r.set_aov(None, None)
    before = c.read()
    c.trace(sa, 0)
    after = c.read()
    assert same(after[0], acc[0][0]) and same(after[1], before[1]) and same(after[2], before[2])
    c.close()


@pytest.mark.parametrize("which", ["albedo", "normal_depth"])
def test_one_target_alone(data, which):
    s, st = data["scene"], data["st"]
    c = Ctx(s, albedo=which == "albedo", normal_depth=which == "normal_depth")
    sa = copy_settings(st); sa.reset = 1
    for f in range(3):
        c.trace(sa, f); sa.reset = 0
    out, alb, nd = c.read()
    assert same(out, data["acc"][2][0])
    if which == "albedo":
        assert nd is None and same(alb, data["acc"][2][1])
    else:
        assert alb is None and same(nd, data["acc"][2][2])
    c.close()


def test_argument_errors_and_the_megakernel_refusal(data):
    s, st = data["scene"], data["st"]
    c = Ctx(s)
    r, L = c.r, c.r.L

    def set_rc(enable, a, n):
        cfg = abi.PtAovConfig(enable, a.data_ptr() if a is not None else None, n.data_ptr() if n is not None else None)
        return L.pt_set_aov(r.h, C.byref(cfg))

    assert set_rc(1, None, None) == -1                                   # enabled without a target
    assert L.pt_set_aov(r.h, None) == -1
    assert set_rc(0, None, None) == 0                                    # off needs none
    assert set_rc(1, c.alb, c.nd) == 0
    # megakernel: refused, nothing written
    r.set_kernel_mode(abi.MODE_MEGAKERNEL)
    for t in (c.out, c.alb, c.nd):
        t.fill_(POISON)
    p = s.execute_params(0)
    p.output = c.out.data_ptr()
    sa = copy_settings(st)
    assert L.pt_trace(r.h, C.byref(sa), C.byref(p)) == -1
    assert all(np.all(x == POISON) for x in c.read())
    s1 = copy_settings(st); s1.flags &= ~abi.FLAG_ACCUMULATE              # AOV calls need not accumulate: refused all the same
    assert L.pt_trace(r.h, C.byref(s1), C.byref(p)) == -1
    # ... but a debug-output call is no AOV call, and with AOVs off the megakernel runs as always
    sd = copy_settings(st); sd.debug_output = abi.DEBUG_OUTPUT_COLOR
    c.trace(sd, 0)
    out, alb, nd = c.read()
    assert not np.all(out == POISON) and np.all(alb == POISON) and np.all(nd == POISON)
    assert set_rc(0, None, None) == 0
    c.trace(sa, 0)
    assert np.all(c.read()[1] == POISON)
    # back in wavefront mode the refused configuration works
    r.set_kernel_mode(abi.MODE_WAVEFRONT)
    assert set_rc(1, c.alb, c.nd) == 0
    sa.reset = 1
    c.trace(sa, 0)
    assert all(same(g, w) for g, w in zip(c.read(), data["acc"][0]))
    c.close()


@pytest.mark.parametrize("white", [0, 1], ids=["materials", "diffuse_white"])
@pytest.mark.parametrize("geometric", [0, 1], ids=["shading_normals", "geometric_normals"])
def test_material_heavy_scene_albedo_and_normals(oracle_lib, white, geometric):
    """Items 1 and 2 on test_scene at 128x128: textures, a normal map, texture transforms, vertex colours, double-sided, MASK and BLEND
    materials, a mirrored instance, meshes without tangents."""
    frames = 4
    s = scenes.test_scene(128, 64, with_env=False)
    s.settings.environment_color[:] = ENV
    st = copy_settings(s.settings)
    st.flags |= (abi.FLAG_MATERIAL_DIFFUSE_WHITE if white else 0) | (abi.FLAG_MATERIAL_USE_GEOMETRIC_NORMALS if geometric else 0)
    orc = oracle_frames(oracle_lib, s, st, frames)
    hit, miss = hit_and_miss_shares(orc, frames)
    print("hit share %.3f, miss share %.3f" % (hit, miss))
    assert hit >= 0.10 and miss >= 0.10, (hit, miss)
    single, acc, _ = product_runs(s, st, frames)
    check_albedo(acc, orc, frames)
    check_normals(single, orc, frames)
    want = av.fold([single[f][2] for f in range(frames)])
    assert same(acc[frames - 1][2], want[frames - 1])
