"""The API on a non-blocking side stream (include/mipt.h: "asynchronous on the context's stream" / "synchronises the stream").

Every other GPU file of the suite runs its contexts on the legacy null stream, which orders itself against everything in the process:
there a missing hipStreamSynchronize in front of a blocking null-stream copy, a null-stream fill that lands late, an upload ring slot
reused too early or a loopback exchange that does not wait for its peer cannot show.  Here every context sits on a stream of
torch.cuda.Stream() -- non-blocking, checked by stream_ballast.side_stream() -- and every race is made deterministic with ballast
(stream_ballast.py): a spin kernel of known length in front of the work a call must wait for, or must not.

Each test asserts its premise -- the ballast is still running where the race is decided (`Env.open`), and the two versions a stale
read could confuse really differ -- so a mis-sized ballast fails loudly.  Every expectation is bit-equality with `serial()`: the same
call sequence on the null stream with a device synchronise after every call, the configuration the rest of the suite pins to the oracle.

Ballast: torch.cuda._sleep, calibrated once per session against the event clock -- 2.40e6 cycles per millisecond on the MI355X (64e6
cycles took 26.6 ms) -- and 100 ms (stream_ballast.NOMINAL_MS) in front of every group of calls; no premise needed more.  The most in
one test is 1.0 s (trace_reads_flow: a ballast in front of each of its ten producers).
"""
import functools
import math

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes

import stream_ballast as sb

pytestmark = pytest.mark.gpu

W, H = 40, 24                  # ragged: 3 x 2 tiles, the last column and the last row partly outside
POISON = 7.0
SPP = 2


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


@pytest.fixture(scope="module")
def side():
    """Three side streams for the whole module (with the null stream: the four hardware queues a process gets)."""
    import torch
    streams = [sb.side_stream() for _ in range(3)]
    sb.cycles_per_ms()
    yield streams
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def small_scene(with_env=False):
    """The all-feature test scene on the ragged frame, seen from above through a 60 degree lens: geometry in nearly every pixel, so
    that two versions of the scene differ in most of them."""
    s = scenes.test_scene(size=48, tex=16, with_env=with_env)
    s.width, s.height = W, H
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.4), 2.4, 0.35, -1.1)
    s.y_fov = math.pi / 3
    return s


@functools.lru_cache(maxsize=None)
def chart_scene():
    """The test scene with the floor's UV chart shrunk into the middle of its atlas: a bake of the floor leaves texels to dilate."""
    s = scenes.test_scene(size=48, tex=16, with_env=False)
    k = s.instances[0].gpu.texcoord_descriptors[0]
    uv, fmt = s.buffers[k]
    s.buffers[k] = (np.ascontiguousarray(uv * 0.5 + 0.2, dtype=np.float32), fmt)
    return s


@functools.lru_cache(maxsize=None)
def figure_scene():
    """The skinned figure on its floor, small frame, constant sky (no environment map to preprocess)."""
    s = scenes.skinned_figure(W, H)
    s.env_image = None
    st = copy_settings(s.settings)
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)
    st.environment_color[:] = (0.6, 0.7, 0.9)
    s.settings = st
    return s


def settings_of(s, reset=1):
    st = copy_settings(s.settings)
    st.reset = reset
    return st


def params(s, frame, size=None, env=None, **kw):
    p = s.execute_params(frame, env_handle=env, **kw)
    if size is not None:
        p.width, p.height = size
    return p


def poisoned(w=W, h=H, c=4):
    import torch
    shape = (h, w, c) if c else (h, w)
    return torch.full(shape, POISON, dtype=torch.float32, device="cuda:0")


def plane(r, t):
    """pt_readback of an (H, W) float32 plane (W a multiple of 4: the call counts float4)."""
    import ctypes as C
    h, w = t.shape
    assert w % 4 == 0
    out = np.full((h, w), -1.0, np.float32)
    r._check(r.L.pt_readback(r.h, C.c_void_p(t.data_ptr()), w // 4, h, out.ctypes.data_as(C.c_void_p)))
    return out


def struct_bytes(x):
    return np.frombuffer(bytes(x), np.uint8).copy()


RAY_COUNTS = ("rays", "rays_primary", "rays_bounce", "rays_shadow", "closest_hits", "accumulated_frames")


def ray_counts(r):
    q = r.stats()
    return np.array([int(getattr(q, n)) for n in RAY_COUNTS], np.int64)


def warm_ring(r):
    """Steady state of the upload ring: every pinned slot already holds room for anything these tests upload."""
    big = np.zeros(1 << 16, np.uint8)
    hb = r.buffer_create(big, abi.FORMAT_R32_UINT)
    for _ in range(8):
        r.buffer_update(hb, big)
    return hb


def materials_of(s, h, edit=None):
    """The scene's material table with the context's handles (scenes.SceneData.upload), optionally edited."""
    mats = []
    for m in s.materials:
        c = abi.PtMaterial.from_buffer_copy(bytes(m))
        for slot in abi.PtMaterial.TEXTURE_SLOTS:
            ts = getattr(c, slot)
            if ts.descriptor != -1:
                ts.descriptor = h["textures"][ts.descriptor]
            ts.sampler = h["samplers"][ts.sampler]
        if edit is not None:
            edit(c)
        mats.append(c)
    return mats


def assert_same(got, want, where=""):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    bad = []
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if not sb.same(a, b):
            n = int((sb.bits(a) != sb.bits(b)).sum()) if a.shape == b.shape else -1
            bad.append("%s: %d of %d words differ" % (k, n, sb.bits(b).size))
    assert not bad, "%s differs from the serial null-stream run: %s" % (where, "; ".join(bad))


def assert_versions_differ(res, a, b, least=0.5):
    d = sb.differing_pixels(res[a], res[b])
    print("pixels that differ between %s and %s: %.0f %%" % (a, b, 100 * d))
    assert d >= least, "premise on the inputs failed: %s and %s differ in only %.0f %% of the pixels" % (a, b, 100 * d)


# ---- 1. the whole flow ----------------------------------------------------------------------------------------------------------------
def whole_flow(env, mode):
    s = small_scene(True)
    wf = mode == abi.MODE_WAVEFRONT
    r = env.R()
    out, alb, nd, var, layer, mv = (poisoned() for _ in range(6))
    ev = env.ballast(); env.open(ev, "the upload began")
    h = s.upload(r)
    r.set_kernel_mode(mode)
    ev = env.ballast(); env.open(ev, "build_accel began")
    r.build_accel()
    if wf:
        r.set_aov(alb, nd); r.set_variance(var); r.set_matte(abi.MATTE_INSTANCE, [layer])
        p0 = params(s, 0)
        r.set_motion(mv, list(p0.world_to_view), list(p0.view_to_clip))
    st = settings_of(s)
    for f in range(3):
        ev = env.ballast(); env.open(ev, "trace %d began" % f)
        r.trace(st, params(s, f, env=h["env"]), out)
        st.reset = 0
    res = {}
    ev = env.ballast(); env.open(ev, "the filters began")
    dev = {"bloom": r.bloom(out)}
    if wf:
        dev["denoise"] = r.denoise(out, alb, nd)
        dev["denoise_variance"] = r.denoise_variance(out, alb, nd, var, samples=3)
        dev["motion_blur"] = r.motion_blur(out, mv)
        dev["reproject"], length = r.reproject(out, mv, dev["denoise"], mv)
        dev.update(albedo=alb, normal_depth=nd, variance=var, matte=layer, motion=mv)
    ev = env.ballast(); env.open(ev, "the reads began")
    res["tonemap"], res["rgba8"] = r.tonemap(out, want_rgba8=True)
    res["output"] = r.readback(out)
    for k, t in dev.items():
        res[k] = r.readback(t)
    if wf:
        res["history"] = plane(r, length)
    return res


@pytest.mark.parametrize("mode", [abi.MODE_WAVEFRONT, abi.MODE_MEGAKERNEL], ids=["wavefront", "megakernel"])
def test_whole_flow_on_a_side_stream_equals_the_null_stream_flow(side, mode):
    """Upload, build, three accumulated traces with every optional target, every post filter, tone map and readback, with ballast in
    front of each group of calls (the megakernel without the passes it refuses): every image bit-equal to the serial run."""
    want = sb.serial(whole_flow, mode)
    got = sb.on_streams(whole_flow, side[:1], mode)
    assert not np.any(want["output"] == POISON) and np.isfinite(want["tonemap"]).all()
    assert_same(got, want, "whole flow")


# ---- 2. synchronising calls -----------------------------------------------------------------------------------------------------------
def trace_reads_flow(env):
    """One more accumulated frame behind ballast before each read: a read that does not wait returns the previous frame count's answer
    (or, for the first, the poison)."""
    s = small_scene(False)
    r = env.R()
    h = s.upload(r)
    out, alb, nd, var, layer, mv = (poisoned() for _ in range(6))
    r.set_aov(alb, nd); r.set_variance(var); r.set_matte(abi.MATTE_INSTANCE, [layer])
    p0 = params(s, 0)
    r.set_motion(mv, list(p0.world_to_view), list(p0.view_to_clip))
    r.build_accel(); r.motion_snapshot()
    r.trace(settings_of(s), p0, out)                   # the steady state: the workspace and the passes' scratch exist
    r.reset_stats()
    mask = poisoned(c=0)
    env.sync()
    for t in (out, alb, nd, var, layer, mv):
        t.fill_(POISON)
    env.sync()
    frame = [0]
    res = {}

    def produce(what):
        ev = env.ballast()
        r.trace(settings_of(s, 1 if frame[0] == 0 else 0), params(s, frame[0]), out)
        frame[0] += 1
        env.open(ev, "pt_trace before " + what)

    produce("pt_readback"); res["readback@1"] = r.readback(out)
    produce("pt_readback"); res["readback@2"] = r.readback(out)
    produce("pt_tonemap"); res["tonemap"], res["rgba8"] = r.tonemap(out, want_rgba8=True)
    produce("pt_get_stats"); res["ray_counts"] = ray_counts(r)
    produce("pt_accum_save"); res["blob"] = np.frombuffer(r.accum_save(W, H, out, alb, nd), np.uint8)
    produce("pt_noise_estimate")
    mean, mx, summary = r.noise_estimate(out, var, samples=frame[0], threshold=0.05)
    res["noise_mean"], res["noise_max"], res["noise_summary"] = mean, mx, struct_bytes(summary)
    produce("pt_motion_snapshot_state"); res["snapshot_state"] = np.array([r.motion_snapshot_state()], np.int32)
    produce("pt_matte_extract")
    ev = env.ballast()
    r.matte_extract([layer], [r.matte_id("instance_%d" % i) for i in (0, 2, 3)], out=mask)
    env.open(ev, "pt_matte_extract")
    res["mask"] = plane(r, mask)
    res["layer"] = r.readback(layer)
    # pt_lens_focus_at: the floor moves away behind ballast; the ray must meet the refitted tree
    floor = h["buffers"][s.instances[0].gpu.position_descriptor]
    P = s.buffers[s.instances[0].gpu.position_descriptor][0]
    st, p = settings_of(s), params(s, 0)
    px, py = W / 2 + 0.5, H - 1.5
    before = r.focus_at(st, p, px, py)
    ev = env.ballast()
    r.buffer_update(floor, (P - np.array([0, 0, 0.35], np.float32)).astype(np.float32))
    env.open(ev, "pt_buffer_update before pt_lens_focus_at")
    after = r.focus_at(st, p, px, py)
    assert before is not None and after is not None
    res["focus"] = np.array([before, after], np.float32)
    return res


def adaptive_reads_flow(env):
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    out = poisoned()
    r.set_adaptive(2, 16, 0.02); r.set_samples_per_trace(2)
    r.trace(settings_of(s), params(s, 0), out)          # the steady state: the tile state and the half buffer exist
    env.sync()
    res = {}
    for k, what in enumerate(("pt_adaptive_read", "pt_accum_save")):
        ev = env.ballast()
        r.trace(settings_of(s, 1 if k == 0 else 0), params(s, 2 * k), out)
        env.open(ev, "the adaptive pt_trace before " + what)
        if k == 0:
            active, samples, error, half = r.adaptive_read(W, H)
            res.update(active=np.array([active], np.int32), samples=samples, error=error, half=half)
        else:
            res["blob"] = np.frombuffer(r.accum_save(W, H, out), np.uint8)
    return res


def skin_read_flow(env):
    s = figure_scene()
    r = env.R()
    h = s.upload(r)
    b = scenes.SkinBinding(r, s, h, 0, 1)
    warm_ring(r)
    b.pose(0.0)
    env.sync()
    nv = b.params.num_of_vertices
    res = {"position@0": r.buffer_read(b.out_position, np.float32, nv * 3)}
    ev = env.ballast()
    b.pose(0.55)
    env.open(ev, "pt_skin_run before pt_buffer_read")
    res["position"] = r.buffer_read(b.out_position, np.float32, nv * 3)
    res["tangent_space"] = r.buffer_read(b.out_tangent_space, np.uint32, nv)
    return res


def atlas_reads_flow(env):
    """The calls whose producing work drains the stream itself at some point (pt_env_create, the first bake trace after the tree
    changed): the window is open when the producer is called; what the read returns must still be the serial answer."""
    s = small_scene(False)
    r = env.R()
    h = s.upload(r)
    r.build_accel()
    res = {}
    rng = np.random.default_rng(5)
    sky = (rng.random((32, 64, 3)) * 4).astype(np.float32)
    ev = env.ballast(); env.open(ev, "pt_env_create began")
    e = r.env_create(sky)
    n, cube, pyr = r.env_read(e)
    res.update(env_n=np.array([n], np.int32), env_cube=cube.view(np.uint8), env_pyramid=pyr)
    # bake: the floor's atlas
    A = 32
    atlas = poisoned(A, A)
    r.set_bake(1.0 / 64, 0, 0)
    r.trace(settings_of(s), params(s, 0, size=(A, A)), atlas)
    ev = env.ballast()
    r.trace(settings_of(s, 0), params(s, 1, size=(A, A)), atlas)
    env.open(ev, "the bake pt_trace before pt_bake_coverage")
    inst, prim = r.bake_coverage(A, A)
    res.update(bake_instance=inst, bake_primitive=prim, bake=r.readback(atlas))
    r.set_bake(1.0 / 64, enable=False)
    # probes
    aw, ah = r.set_probes([(0.0, -0.5, 1.2), (0.8, 0.2, 1.0)], 16, columns=2)
    patlas = poisoned(aw, ah)
    r.trace(settings_of(s), params(s, 0, size=(aw, ah)), patlas)
    env.sync()
    ev = env.ballast()
    r.trace(settings_of(s, 0), params(s, 1, size=(aw, ah)), patlas)
    env.open(ev, "the probe pt_trace before pt_probe_project")
    res["sh"] = r.probe_project(patlas, abi.PROBE_SH_IRRADIANCE)
    res["probes"] = r.readback(patlas)
    return res


@pytest.mark.parametrize("flow", [trace_reads_flow, adaptive_reads_flow, skin_read_flow, atlas_reads_flow], ids=lambda f: f.__name__)
def test_every_synchronising_call_returns_what_the_stream_has_produced(side, flow):
    """Ballast, the producing work, and at once a call the header says synchronises the stream: pt_readback, pt_tonemap (both host
    outputs), pt_get_stats, pt_accum_save, pt_noise_estimate, pt_motion_snapshot_state, pt_matte_extract + readback, pt_lens_focus_at,
    pt_adaptive_read, pt_buffer_read of a skin output, pt_env_read, pt_bake_coverage, pt_probe_project.  The device memory starts
    poisoned or holds a visibly different earlier version; the answers equal the serial run's."""
    want = sb.serial(flow)
    if flow is trace_reads_flow:
        assert not sb.same(want["readback@1"], want["readback@2"]) and sb.differing_pixels(want["readback@1"], want["readback@2"]) >= 0.5
        assert want["focus"][0] != want["focus"][1], want["focus"]
        assert not np.any(want["mask"] == POISON)
    if flow is skin_read_flow:
        assert (want["position@0"] != want["position"]).mean() > 0.5
    got = sb.on_streams(flow, side[:1])
    assert_same(got, want, flow.__name__)


# ---- 3. asynchronous calls ------------------------------------------------------------------------------------------------------------
def nowait(env, what, fn):
    """The call returns while the ballast in front of it is still running: it did not wait for the stream."""
    ev = env.ballast()
    out = fn()
    env.open(ev, what + " (documented asynchronous)")
    return out


def async_trace_flow(env):
    s = figure_scene()
    r = env.R()
    h = s.upload(r)
    b = scenes.SkinBinding(r, s, h, 0, 1)
    warm_ring(r)
    r.set_samples_per_trace(SPP)
    out = [poisoned() for _ in range(4)]
    floor = h["buffers"][s.instances[1].gpu.position_descriptor]
    P = s.buffers[s.instances[1].gpu.position_descriptor][0]
    st, p = settings_of(s), params(s, 0)
    # the steady state: tree built, a refit done, scratch and workspace at their sizes
    b.pose(0.0); r.trace(st, p, out[0]); b.pose(0.1); r.trace(st, p, out[0])
    env.sync()
    nowait(env, "pt_trace on an unchanged scene", lambda: r.trace(st, p, out[1]))
    nowait(env, "pt_skin_run", lambda: b.pose(0.55))
    nowait(env, "pt_trace after pt_skin_run (the refit)", lambda: r.trace(st, p, out[2]))
    nowait(env, "five pt_buffer_update", lambda: [r.buffer_update(floor, (P + np.array([0, 0, 0.04 * k], np.float32)).astype(np.float32)) for k in range(1, 6)])
    nowait(env, "pt_trace after pt_buffer_update (the refit)", lambda: r.trace(st, p, out[3]))
    env.sync()
    nv = b.params.num_of_vertices
    res = {"out%d" % k: r.readback(t) for k, t in enumerate(out)}
    res["position"] = r.buffer_read(b.out_position, np.float32, nv * 3)
    return res


def async_filters_flow(env):
    import torch
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    out, alb, nd, var, mv = (poisoned() for _ in range(5))
    r.set_aov(alb, nd); r.set_variance(var)
    p0 = params(s, 0)
    r.set_motion(mv, list(p0.world_to_view), list(p0.view_to_clip))
    st = settings_of(s)
    for f in range(3):
        r.trace(st, params(s, f), out); st.reset = 0
    r.exchange_create(0, 1, None)
    dst = {k: poisoned() for k in ("denoise", "denoise_variance", "bloom", "motion_blur", "reproject", "unpacked", "frame")}
    length = poisoned(c=0)
    packed = torch.full((max(r.tiles_packed_bytes(W, H, 1, 2) // 16, 1), 4), POISON, dtype=torch.float32, device="cuda:0")
    import ctypes as C

    def pack():
        r._check(r.L.pt_tiles_pack(r.h, C.c_void_p(out.data_ptr()), W, H, 1, 2, C.c_void_p(packed.data_ptr())))

    calls = [("pt_denoise", lambda: r.denoise(out, alb, nd, out=dst["denoise"])),
             ("pt_denoise_variance", lambda: r.denoise_variance(out, alb, nd, var, samples=3, out=dst["denoise_variance"])),
             ("pt_bloom", lambda: r.bloom(out, out=dst["bloom"])),
             ("pt_motion_blur", lambda: r.motion_blur(out, mv, out=dst["motion_blur"])),
             ("pt_reproject", lambda: r.reproject(out, mv, alb, mv, out_color=dst["reproject"], out_length=length)),
             ("pt_tiles_pack", pack),
             ("pt_tiles_unpack", lambda: r.tiles_unpack(packed, dst["unpacked"], 1, 2)),
             ("pt_exchange_frame with world 1", lambda: r.exchange_frame(out, dst["frame"]))]
    for _, fn in calls:            # the steady state: every filter's scratch at its size
        fn()
    env.sync()
    for t in dst.values():
        t.fill_(POISON)
    packed.fill_(POISON); length.fill_(POISON)
    env.sync()
    for what, fn in calls:
        nowait(env, what, fn)
    env.sync()
    res = {k: r.readback(t) for k, t in dst.items()}
    res["history"] = plane(r, length)
    res["packed"] = packed.cpu().numpy()
    # pt_bake_dilate, after a bake trace of its size
    A = 32
    s = chart_scene()
    r = env.R()
    s.upload(r)
    atlas = poisoned(A, A)
    r.set_bake(1.0 / 64, 0, 0)
    r.trace(settings_of(s), params(s, 0, size=(A, A)), atlas)
    filled = atlas.clone()
    r.bake_dilate(filled, 3)
    env.sync()
    filled.copy_(atlas)
    env.sync()
    nowait(env, "pt_bake_dilate", lambda: r.bake_dilate(filled, 3))
    env.sync()
    res["bake"], res["dilated"] = r.readback(atlas), r.readback(filled)
    return res


@pytest.mark.parametrize("flow", [async_trace_flow, async_filters_flow], ids=lambda f: f.__name__)
def test_calls_documented_asynchronous_do_not_wait_and_are_right(side, flow):
    """The steady-state calls include/mipt.h calls asynchronous, each with ballast ahead of it on the stream: the ballast is still
    running when the call returns, and after the stream has drained the result equals the serial run's."""
    want = sb.serial(flow)
    for k, v in want.items():
        assert not np.all(np.asarray(v) == POISON), k
    if flow is async_filters_flow:
        assert not sb.same(want["bake"], want["dilated"])
    got = sb.on_streams(flow, side[:1])
    assert_same(got, want, flow.__name__)


# ---- 4. tables between frames ---------------------------------------------------------------------------------------------------------
def tables_flow(env):
    s = small_scene(False)
    r = env.R()
    h = s.upload(r)
    warm_ring(r)
    r.set_samples_per_trace(SPP)
    st, p = settings_of(s), params(s, 3)
    L1 = list(s.lights)
    L2 = []
    for l in s.lights:
        c = abi.PtLight.from_buffer_copy(bytes(l))
        c.intensity = l.intensity * 2.5
        c.color[:] = (l.color[2] * 0.5 + 0.2, l.color[0], l.color[1] * 0.6)
        L2.append(c)
    M1 = materials_of(s, h)

    def edit(m):
        b = list(m.base_color_factor)
        m.base_color_factor[:] = (b[2] * 0.5 + 0.1, b[0] * 0.5 + 0.1, b[1] * 0.5 + 0.1, b[3])
        m.roughness_factor = min(1.0, m.roughness_factor * 0.5 + 0.3)
    M2 = materials_of(s, h, edit)
    I1 = h["instances"]
    I2 = [abi.PtInstanceDesc.from_buffer_copy(bytes(d)) for d in I1]
    T = camera.trs((0.45, 0.35, -0.2))
    I2[0].gpu.transform[:] = camera.cm(T)
    I2[0].gpu.normal_transform[:] = camera.cm(camera.inverse_transpose(T))
    floor = h["buffers"][s.instances[0].gpu.position_descriptor]             # (the floor's positions)
    P1 = s.buffers[s.instances[0].gpu.position_descriptor][0]
    P2 = (P1 + np.stack([0.3 * np.sin(2 * P1[:, 1]), 0.3 * np.cos(2 * P1[:, 0]), 0.15 * np.sin(3 * P1[:, 0]) * np.cos(2 * P1[:, 1])], axis=1)).astype(np.float32)

    def run(outs):
        r.trace(st, p, outs[0])
        r.set_lights(L2); r.trace(st, p, outs[1])
        r.set_materials(M2); r.trace(st, p, outs[2])
        r.set_instances(I2); r.trace(st, p, outs[3])
        r.buffer_update(floor, P2); r.trace(st, p, outs[4])

    scratch = [poisoned() for _ in range(5)]
    outs = [poisoned() for _ in range(5)]
    run(scratch)                   # the steady state: every table, the refit's scratch and the ring at their sizes
    r.set_lights(L1); r.set_materials(M1); r.set_instances(I1); r.buffer_update(floor, P1)
    r.trace(st, p, scratch[0])
    env.sync()
    ev = env.ballast()
    run(outs)
    env.open(ev, "five traces and the four table changes between them were enqueued")
    env.sync()
    return {"out%d" % (k + 1): r.readback(t) for k, t in enumerate(outs)}


def test_an_enqueued_frame_reads_the_table_it_was_enqueued_with(side):
    """trace, set_lights, trace, set_materials, trace, set_instances (a moved instance: a refit), trace, buffer_update of a vertex
    stream, trace -- all behind one ballast, no wait in between: each image is the serial run's for its own version of the tables."""
    want = sb.serial(tables_flow)
    for k in range(1, 5):
        assert_versions_differ(want, "out%d" % k, "out%d" % (k + 1))
    got = sb.on_streams(tables_flow, side[:1])
    assert_same(got, want, "tables")


def ring_wrap_flow(env):
    s = small_scene(False)
    r = env.R()
    h = s.upload(r)
    warm_ring(r)
    r.set_samples_per_trace(SPP)
    st, p = settings_of(s), params(s, 3)
    floor = h["buffers"][s.instances[0].gpu.position_descriptor]             # (the floor's positions)
    P1 = s.buffers[s.instances[0].gpu.position_descriptor][0]
    outs = [poisoned() for _ in range(10)]
    r.buffer_update(floor, P1); r.trace(st, p, outs[0])
    env.sync()
    ev = env.ballast()
    env.open(ev, "the first pt_buffer_update")
    for k in range(10):            # two ring slots a pair (the stream, the refit's touched rows): the 8-slot ring wraps
        Pk = (P1 + np.array([0.05 * (k + 1), -0.08 * (k + 1), 0], np.float32) * (1 + np.sin(3 * P1[:, :1] + k))).astype(np.float32)
        r.buffer_update(floor, Pk)
        r.trace(st, p, outs[k])
    env.sync()
    return {"out%d" % k: r.readback(t) for k, t in enumerate(outs)}


def bone_wrap_flow(env):
    s = figure_scene()
    r = env.R()
    h = s.upload(r)
    b = scenes.SkinBinding(r, s, h, 0, 1)
    warm_ring(r)
    st, p = settings_of(s), params(s, 0)
    n = 12                         # 19 bones: the arena of bytes * 8 + 4096 holds nine slices, the tenth call wraps it
    outs = [poisoned() for _ in range(n)]
    b.pose(0.0); r.trace(st, p, outs[0])
    env.sync()
    ev = env.ballast()
    env.open(ev, "the first pt_skin_run")
    for k in range(n):
        b.pose(0.15 * (k + 1))
        r.trace(st, p, outs[k])
    env.sync()
    return {"out%02d" % k: r.readback(t) for k, t in enumerate(outs)}


@pytest.mark.parametrize("flow", [ring_wrap_flow, bone_wrap_flow], ids=lambda f: f.__name__)
def test_upload_ring_and_bone_arena_wrap_under_enqueued_frames(side, flow):
    """Ten buffer_update + trace pairs (the pinned ring's eight slots wrap) and twelve skin_run + trace pairs (the bone arena wraps)
    into as many outputs, behind one ballast.  The host may block at the wrap, so only the start of the window is asserted; every
    output is the serial run's."""
    want = sb.serial(flow)
    keys = sorted(want)
    differ = [sb.differing_pixels(want[a], want[b]) for a, b in zip(keys, keys[1:])]
    print("pixels that differ between consecutive outputs: " + " ".join("%.0f%%" % (100 * d) for d in differ))
    assert min(differ) > 0, differ             # every version is its own (a moving floor or figure covers a part of the frame)
    got = sb.on_streams(flow, side[:1])
    assert_same(got, want, flow.__name__)


# ---- 5. null-stream fills -------------------------------------------------------------------------------------------------------------
def null_fill_flow(env):
    import torch
    s = figure_scene()
    null = torch.cuda.default_stream()
    out = poisoned()
    env.sync()
    ev = env.ballast(stream=null)
    env.open(ev, "pt_create")
    r = env.R()
    h = s.upload(r)                # (its blocking copies run on the null stream: they outlast the ballast)
    env.sync()
    ev = env.ballast(stream=null)
    b = scenes.SkinBinding(r, s, h, 0, 1)          # pt_buffer_create(NULL) for the two skin outputs
    b.pose(0.55)
    env.open(ev, "pt_buffer_create(NULL) and pt_skin_run")
    r.enable_counters(1); r.reset_stats()
    r.trace(settings_of(s), params(s, 0), out)
    env.sync()                     # the context's stream only: the null stream is not waited for
    nv = b.params.num_of_vertices
    res = {"output": r.readback(out), "position": r.buffer_read(b.out_position, np.float32, nv * 3),
           "tangent_space": r.buffer_read(b.out_tangent_space, np.uint32, nv), "ray_counts": ray_counts(r)}
    q = r.stats()
    res["counters"] = np.array([q.nodes_visited, q.tris_tested, q.texture_taps], np.int64)
    return res


def test_null_stream_fills_cannot_land_late(side):
    """The context on a side stream, the ballast on the null stream: pt_create's fills (the white texel, the counters) and the zero
    fill of pt_buffer_create(NULL) are ordered with the kernels that read and overwrite that memory, because they run on the context's
    stream too.  A fill left on the null stream would land behind the ballast, over what the skin kernel wrote."""
    want = sb.serial(null_fill_flow)
    assert np.abs(want["position"]).max() > 0 and want["counters"].min() > 0
    got = sb.on_streams(null_fill_flow, side[:1])
    assert_same(got, want, "null-stream fills")


# ---- 6. loopback exchange, a stream per rank ------------------------------------------------------------------------------------------
def one_rank_flow(env):
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    acc = poisoned()
    st = settings_of(s)
    res = {}
    for f in range(3):
        r.trace(st, params(s, f), acc); st.reset = 0
        res["frame%d" % f] = r.readback(acc)
    return res


def exchange_flow(env, mode, dst):
    import torch
    s = small_scene(False)
    world = 3
    group = 7000 + mode * 10 + dst
    ranks = []
    for k in range(world):
        r = env.R(k)
        s.upload(r)
        r.exchange_create_loopback(k, world, group)
        ranks.append((r, poisoned()))
    frames = [poisoned() for _ in range(3)]
    warm = poisoned()
    senders = [k for k in range(world) if k != dst]
    env.sync()                     # (the images were filled on the first stream)

    def rank_frame(k, f, st, frame):
        """Returns an event behind the rank's trace (its exchange may have to wait for the root: its trace never does)."""
        r, acc = ranks[k]
        traced = None
        with env.stream(k):
            r.trace(st, params(s, f, tile_rank=k, tile_rank_count=world), acc)
            if not env.serial:
                traced = torch.cuda.Event()
                traced.record(env.streams[k])
            r.exchange_frame(acc, frame, mode=mode, dst=dst)
        return traced

    for k in senders + [dst]:      # the steady state: every send and receive buffer at its size
        rank_frame(k, 0, settings_of(s), warm)
    env.sync()
    evb = None
    for f in range(3):
        st = settings_of(s, 1 if f == 0 else 0)
        eva = env.ballast(k=senders[0])                    # (a) a sender's post is late: the root must wait for it
        idle = [rank_frame(k, f, st, None) for k in senders][1]
        # (b) the root's receive of frame f - 1 is still behind its ballast while the senders have enqueued the pack of frame f
        env.open(evb, "the senders enqueued their next frame")
        evb = env.ballast(k=dst)
        rank_frame(dst, f, st, frames[f])
        if not env.serial:         # the rank without ballast gets on with its trace while the two ballasts have not run out
            idle.synchronize()
            assert not eva.query() and not evb.query(), \
                "premise failed: the idle rank's trace finished only after another stream's ballast -- queue sharing has serialised the streams"
    env.sync()
    root = ranks[dst][0]
    res = {"frame%d" % f: root.readback(t) for f, t in enumerate(frames)}
    for r, _ in ranks:
        r.exchange_destroy()
    return res


@pytest.fixture(scope="module")
def one_rank():
    return sb.serial(one_rank_flow)


@pytest.mark.parametrize("dst", [0, 2])
@pytest.mark.parametrize("mode", [abi.EXCHANGE_GATHER, abi.EXCHANGE_REDUCE], ids=["gather", "reduce"])
def test_loopback_exchange_with_every_rank_on_its_own_stream(side, one_rank, mode, dst):
    """World 3, a side stream per rank, three accumulated frames.  (a) Ballast in front of a sender's trace: the root's receive waits
    for the post.  (b) Ballast in front of the root's frame while the senders already enqueue the next frame's pack: their pack waits
    for `consumed`.  The root's frame after every exchange is the one-rank running mean, bit for bit."""
    assert sb.differing_pixels(one_rank["frame0"], one_rank["frame1"]) >= 0.5 and sb.differing_pixels(one_rank["frame1"], one_rank["frame2"]) >= 0.5
    got = sb.on_streams(exchange_flow, side, mode, dst)
    assert_same(got, one_rank, "root's frames")


# ---- 7. two contexts at once ----------------------------------------------------------------------------------------------------------
def contexts_flow(env, which):
    """which: the contexts that run, of (0: the test scene, 1: the skinned figure) -- each on its own stream."""
    ctx = {}
    for k in which:
        s = small_scene(False) if k == 0 else figure_scene()
        r = env.R(k)
        h = s.upload(r)
        if k == 1:
            scenes.SkinBinding(r, s, h, 0, 1).pose(0.55)
        ctx[k] = (s, r, poisoned(), [poisoned() for _ in range(4)], settings_of(s))
        env.sync()                 # (the images were filled on the first stream)
        r.trace(ctx[k][4], params(s, 0), ctx[k][2]); r.bloom(ctx[k][2], out=ctx[k][3][0])     # the steady state
    env.sync()
    evs = {k: env.ballast(k=k) for k in which}
    for f in range(4):
        for k in which:
            s, r, acc, blooms, st = ctx[k]
            with env.stream(k):
                r.trace(st, params(s, f), acc); st.reset = 0
                r.bloom(acc, out=blooms[f])
    for k in which:
        env.open(evs[k], "four frames of each context were enqueued")
    env.sync()
    res = {}
    for k in which:
        s, r, acc, blooms, st = ctx[k]
        res["acc%d" % k] = r.readback(acc)
        for f in range(4):
            res["bloom%d_%d" % (k, f)] = r.readback(blooms[f])
    return res


def test_two_contexts_on_two_streams_interleaved(side):
    """Two scenes, a context and a stream each, four accumulated frames each with a bloom after every frame, enqueued alternately with
    no wait: each context's results are those of its solo serial run."""
    want = dict(sb.serial(contexts_flow, (0,)))
    want.update(sb.serial(contexts_flow, (1,)))
    assert not sb.same(want["bloom0_0"], want["bloom0_3"]) and not sb.same(want["bloom1_0"], want["bloom1_3"])
    got = sb.on_streams(contexts_flow, side[:2], (0, 1))
    assert_same(got, want, "two contexts")
