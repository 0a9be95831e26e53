"""One caller thread per context (include/mipt.h: "One caller thread per context"; INTEGRATION.md, "Threads").

Every other GPU file of the suite calls its contexts in turn from one thread.  Here three Python threads -- the library is loaded with
ctypes.CDLL, so its calls drop the GIL -- each drive contexts of their own on a non-blocking side stream of their own
(stream_ballast.side_stream(); with the null stream: the four hardware queues a process gets), released together by a barrier.  What
could go wrong is state that two contexts share without saying so: a process-wide scratch buffer, a static table built on first use,
an error text or a staging slot that is not the context's own, the loopback registry, a pt_destroy whose implicit device
synchronise lands in the middle of another context's frame, a null-stream test hook beside side-stream work.

Every expectation is bit equality with stream_ballast.serial() of the same call sequence: one thread, the null stream, a device
synchronise after every call -- the configuration the rest of the suite pins to the oracle.  (The exchange is compared with the
one-rank running mean, as in test_gpu_round3.py.)  Each test asserts its premise: the threads' wall-clock intervals have a common
part of at least half the shortest of them; otherwise nothing ran side by side and the test proved nothing.

These tests detect races; they do not prove their absence: a run in which the threads happened not to collide passes.  There are no
retries and nothing is repeated until it fails.

Shape for trouble: a worker checks the shared stop event before every call and sets it on any exception; the main thread joins with
a cap and re-raises the first error; after a HIP error or a join that timed out, BROKEN makes the remaining tests of this file fail
at once without touching the GPU.  The cap is 20 x the serial script's wall time, at least 60 s -- a cap, not a measurement.  Serial
wall times measured on the MI355X, in seconds (SERIAL_S below; the frames are 40 x 24, so a script is tens of milliseconds): features
0.050, figure 0.182 (the first skin and refit of the process), atlases 0.028, render 0.010 (six frames; 0.069 for the 128 of the churn
test), errors 0.008, churn 0.069, hooks 0.006, one_rank 0.008.  Every cap is therefore the floor of 60 s.
"""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from gltf_renderer_amd import abi, scenes

import stream_ballast as sb
from test_gpu_streams import (H, SPP, W, assert_same, chart_scene, figure_scene, params, poisoned, settings_of, side, small_scene,  # noqa: F401
                              warm_ring)

pytestmark = pytest.mark.gpu

# serial wall time of each script on the MI355X, seconds (printed by every test: "serial <name>: ... s")
SERIAL_S = {"features": 0.050, "figure": 0.182, "atlases": 0.028, "render": 0.010, "render128": 0.069, "errors": 0.008, "churn": 0.069, "hooks": 0.006,
            "one_rank": 0.008}

THREADS = 3
BROKEN = []                    # why the file gave up: a HIP error in a worker, or a join that ran into its cap


class Stopped(Exception):
    """Another worker failed: this one stops before its next call."""


def cap_s(*names):
    return max(60.0, 20.0 * sum(SERIAL_S[n] for n in names))


class Run:
    """What the workers of one threaded run share."""

    def __init__(self, cap):
        self.stop = threading.Event()
        self.cap = cap
        self.start = threading.Barrier(THREADS)
        self.barriers = {}
        self.lock = threading.Lock()
        self.errors = []

    def check(self):
        if self.stop.is_set():
            raise Stopped()

    def wait(self, name):
        """A barrier of all workers inside a script (the exchange's "root last")."""
        self.check()
        with self.lock:                                # (fail() sets the stop event under this lock: a barrier made after it is never waited on)
            self.check()
            b = self.barriers.setdefault(name, threading.Barrier(THREADS))
        b.wait(self.cap)

    def fail(self, k, e):
        with self.lock:
            self.errors.append((k, e))
            self.stop.set()
            for b in [self.start] + list(self.barriers.values()):
                b.abort()


class Guarded:
    """A Renderer whose every call first checks the run's stop event."""

    def __init__(self, r, run):
        self.__dict__["_r"] = r
        self.__dict__["_run"] = run

    def __getattr__(self, name):
        v = getattr(self._r, name)
        if not callable(v):
            return v

        def call(*a, **kw):
            self._run.check()
            return v(*a, **kw)
        return call

    def __setattr__(self, name, value):
        setattr(self._r, name, value)


class ThreadEnv(sb.Env):
    """stream_ballast.Env for one worker: one side stream, guarded contexts."""

    def __init__(self, stream, run):
        super().__init__([stream])
        self.run = run

    def R(self, k=0):
        self.run.check()
        return Guarded(super().R(k), self.run)

    def abandon(self):
        """After trouble: nothing more goes to the GPU, not even pt_destroy."""
        for r in self.renderers:
            r.h = None
        self.renderers = []


def check(env):
    """Before a raw library call of a script (the guarded Renderer methods check by themselves)."""
    run = getattr(env, "run", None)
    if run is not None:
        run.check()


def wait(env, name):
    run = getattr(env, "run", None)
    if run is not None:
        run.wait(name)


def is_hip_error(e):
    from gltf_renderer_amd.renderer import MiptError
    text = str(e)
    return (isinstance(e, MiptError) and text.startswith("-3")) or (isinstance(e, RuntimeError) and not isinstance(e, MiptError) and ("HIP" in text or "hip" in text))


def not_broken():
    assert not BROKEN, "an earlier test of this file met GPU trouble; not touching the GPU again: %s" % BROKEN[0]


def serial(name, fn, *args):
    t0 = time.perf_counter()
    out = sb.serial(fn, *args)
    print("serial %s: %.3f s" % (name, time.perf_counter() - t0))
    return out


def run_threads(streams, jobs, cap):
    """jobs[k] = (script, args): thread k runs script(env, *args) with its contexts on streams[k].  Returns (results, intervals)."""
    import torch
    not_broken()
    torch.cuda.synchronize()
    run = Run(cap)
    results, intervals = [None] * THREADS, [None] * THREADS

    def worker(k):
        env = ThreadEnv(streams[k], run)
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[k]):
                fn, args = jobs[k]
                run.start.wait(cap)
                t0 = time.perf_counter()
                results[k] = fn(env, *args)
                intervals[k] = (t0, time.perf_counter())
                env.close()
        except BaseException as e:                     # noqa: B036  (the first error is re-raised by the main thread)
            if is_hip_error(e):
                BROKEN.append("thread %d: %r" % (k, e))
            run.fail(k, e)
            env.abandon()

    threads = [threading.Thread(target=worker, args=(k,), daemon=True, name="ctx-%d" % k) for k in range(THREADS)]
    deadline = time.monotonic() + cap
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        run.stop.set()
        BROKEN.append("threads %s did not finish within the cap of %.0f s" % ([t.name for t in threads if t.is_alive()], cap))
        raise AssertionError(BROKEN[-1])
    if run.errors:
        first = [e for _, e in run.errors if not isinstance(e, (Stopped, threading.BrokenBarrierError))] or [run.errors[0][1]]
        raise first[0]
    return results, intervals


def assert_overlap(intervals):
    """The premise: the threads ran side by side."""
    shortest = min(b - a for a, b in intervals)
    common = min(b for _, b in intervals) - max(a for a, _ in intervals)
    print("intervals: %s s, common part %.3f s" % (" ".join("%.3f" % (b - a) for a, b in intervals), common))
    assert common >= 0.5 * shortest, "premise failed: the threads' intervals have %.3f s in common, the shortest is %.3f s" % (common, shortest)


def error_text(r):
    return np.frombuffer(r.L.pt_last_error(r.h), np.uint8).copy()


# ---- the scripts -----------------------------------------------------------------------------------------------------------------------
def features_script(env):
    """Upload, a build with each of the three builders, an accumulation with every optional target, every post filter, tone map, readback."""
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    out, alb, nd, var, layer, mv = (poisoned() for _ in range(6))
    res = {}
    for b in (abi.BUILDER_LBVH, abi.BUILDER_PLOC, abi.BUILDER_PLOC_REINSERT):
        r.set_accel_builder(b); r.request_rebuild(); r.build_accel()
        r.trace(settings_of(s), params(s, 0), out)
        res["builder%d" % b] = r.readback(out)
    r.set_aov(alb, nd); r.set_variance(var); r.set_matte(abi.MATTE_INSTANCE, [layer])
    p0 = params(s, 0)
    r.set_motion(mv, list(p0.world_to_view), list(p0.view_to_clip))
    st = settings_of(s)
    for f in range(3):
        r.trace(st, params(s, f), out)
        st.reset = 0
    dev = {"denoise": r.denoise(out, alb, nd), "denoise_variance": r.denoise_variance(out, alb, nd, var, samples=3), "bloom": r.bloom(out),
           "motion_blur": r.motion_blur(out, mv), "albedo": alb, "normal_depth": nd, "variance": var, "matte": layer, "motion": mv}
    res["tonemap"], res["rgba8"] = r.tonemap(out, want_rgba8=True)
    res["output"] = r.readback(out)
    for k, t in dev.items():
        res[k] = r.readback(t)
    res["last_error"] = error_text(r)
    return res


def figure_script(env):
    """The skinned figure through skin, refit and trace for four frames (the bone arena, the upload ring)."""
    s = figure_scene()
    r = env.R()
    h = s.upload(r)
    b = scenes.SkinBinding(r, s, h, 0, 1)
    warm_ring(r)
    st, p = settings_of(s), params(s, 0)
    outs = [poisoned() for _ in range(4)]
    for k in range(4):
        b.pose(0.15 * (k + 1))
        r.trace(st, p, outs[k])
    nv = b.params.num_of_vertices
    res = {"out%d" % k: r.readback(t) for k, t in enumerate(outs)}
    res["position"] = r.buffer_read(b.out_position, np.float32, nv * 3)
    res["tangent_space"] = r.buffer_read(b.out_tangent_space, np.uint32, nv)
    res["last_error"] = error_text(r)
    return res


def atlases_script(env):
    """A bake with dilation, a probe atlas, and an adaptive accumulation saved and loaded into a fresh context half way."""
    res = {}
    A = 32
    s = chart_scene()
    r = env.R()
    s.upload(r)
    atlas = poisoned(A, A)
    r.set_bake(1.0 / 64, 0, 0)
    for f in range(2):
        r.trace(settings_of(s, 1 if f == 0 else 0), params(s, f, size=(A, A)), atlas)
    filled = atlas.clone()
    r.bake_dilate(filled, 3)
    res["bake_instance"], res["bake_primitive"] = r.bake_coverage(A, A)
    res["bake"], res["dilated"] = r.readback(atlas), r.readback(filled)
    r.set_bake(1.0 / 64, enable=False)
    aw, ah = r.set_probes([(0.0, -0.5, 1.2), (0.8, 0.2, 1.0)], 16, columns=2)
    patlas = poisoned(aw, ah)
    for f in range(2):
        r.trace(settings_of(s, 1 if f == 0 else 0), params(s, f, size=(aw, ah)), patlas)
    res["sh"] = r.probe_project(patlas, abi.PROBE_SH_IRRADIANCE)
    res["probes"] = r.readback(patlas)
    res["last_error"] = error_text(r)
    # adaptive, two batches, then save; a fresh context loads and goes on
    s = small_scene(False)
    a = env.R()
    s.upload(a)
    out = poisoned()
    a.set_adaptive(2, 16, 0.02); a.set_samples_per_trace(2)
    for k in range(2):
        a.trace(settings_of(s, 1 if k == 0 else 0), params(s, 2 * k), out)
    blob = a.accum_save(W, H, out, next_frame=4)
    res["blob"] = np.frombuffer(blob, np.uint8)
    b = env.R()
    s.upload(b)
    out2 = poisoned()
    b.set_adaptive(2, 16, 0.02); b.set_samples_per_trace(2)
    b.accum_load(blob, out2)
    for k in range(2, 4):
        b.trace(settings_of(s, 0), params(s, 2 * k), out2)
    active, samples, error, half = b.adaptive_read(W, H)
    res.update(active=np.array([active], np.int32), samples=samples, error=error, half=half, adaptive=b.readback(out2))
    return res


def render_script(env, frames=6):
    """What the bystanders of the last three tests do: an accumulation with a bloom after every frame."""
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    acc = poisoned()
    blooms = [poisoned() for _ in range(frames)]
    st = settings_of(s)
    for f in range(frames):
        r.trace(st, params(s, f), acc)
        st.reset = 0
        r.bloom(acc, out=blooms[f])
    res = {"bloom%d" % f: r.readback(t) for f, t in enumerate(blooms)}
    res["acc"] = r.readback(acc)
    res["last_error"] = error_text(r)
    return res


SCRIPTS = {"features": features_script, "figure": figure_script, "atlases": atlases_script}


@pytest.fixture(scope="module")
def serial_results():
    """The serial reference of every script, computed once and left unchanged."""
    not_broken()
    out = {name: serial(name, fn) for name, fn in SCRIPTS.items()}
    out["render"] = serial("render", render_script)
    for name, res in out.items():
        assert len(res["last_error"]) == 0, (name, bytes(res["last_error"]))
    assert not sb.same(out["features"]["builder0"], out["features"]["output"]) and not sb.same(out["figure"]["out0"], out["figure"]["out3"])
    assert not sb.same(out["atlases"]["bake"], out["atlases"]["dilated"]) and not sb.same(out["render"]["bloom0"], out["render"]["bloom5"])
    return out


# ---- 1, 2. whole pipelines side by side ------------------------------------------------------------------------------------------------
def test_three_pipelines_overlap_and_each_equals_its_serial_run(side, serial_results):
    """Thread k runs script (k + rotation) % 3 of (features, figure, atlases), for the three rotations: every thread runs every script
    beside the two others.  Each result is the serial run's, bit for bit."""
    names = list(SCRIPTS)
    for rotation in range(3):
        mine = [names[(k + rotation) % 3] for k in range(THREADS)]
        got, intervals = run_threads(side, [(SCRIPTS[n], ()) for n in mine], cap_s(*names))
        assert_overlap(intervals)
        for k, n in enumerate(mine):
            assert_same(got[k], serial_results[n], "rotation %d, thread %d, %s" % (rotation, k, n))


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_the_same_script_on_all_three_threads(side, serial_results, name):
    """State shared between contexts would have to differ per thread to be harmless: identical work collides on it the most."""
    got, intervals = run_threads(side, [(SCRIPTS[name], ())] * THREADS, cap_s(name, name, name))
    assert_overlap(intervals)
    for k in range(THREADS):
        assert_same(got[k], serial_results[name], "thread %d, %s" % (k, name))


# ---- 3. loopback exchange, a thread per rank -------------------------------------------------------------------------------------------
XW, XH = 56, 24                # 4 x 2 tiles, the last column and the last row ragged: 8 tiles, 3 / 3 / 2 over a world of 3
SECOND = 10                    # the second group renders frames 10, 11, 12: another image, so that a mixed-up post shows


def one_rank_script(env, first):
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    acc = poisoned(XW, XH)
    st = settings_of(s)
    res = {}
    for f in range(3):
        r.trace(st, params(s, first + f, size=(XW, XH)), acc)
        st.reset = 0
        res["frame%d" % f] = r.readback(acc)
    return res


def rank_script(env, rank, groups):
    """Rank `rank` of every group of `groups` = [(group id, mode, dst, first frame)], one context a group.  Per frame: every rank traces,
    the ranks that are not a group's root post; a barrier; the roots receive; a barrier (the root's call of frame f comes before any
    sender's of frame f + 1: the documented "root last, every frame")."""
    s = small_scene(False)
    ctx = []
    for group, mode, dst, first in groups:
        r = env.R()
        s.upload(r)
        r.exchange_create_loopback(rank, THREADS, group)
        ctx.append((r, poisoned(XW, XH), [poisoned(XW, XH) for _ in range(3)]))
    wait(env, "created")
    res = {}
    for f in range(3):
        st = settings_of(s, 1 if f == 0 else 0)
        for (group, mode, dst, first), (r, acc, frames) in zip(groups, ctx):
            r.trace(st, params(s, first + f, size=(XW, XH), tile_rank=rank, tile_rank_count=THREADS), acc)
            if rank != dst:
                r.exchange_frame(acc, None, mode=mode, dst=dst)
        wait(env, "posted %d" % f)
        for (group, mode, dst, first), (r, acc, frames) in zip(groups, ctx):
            if rank == dst:
                r.exchange_frame(acc, frames[f], mode=mode, dst=dst)
        wait(env, "received %d" % f)
    for (group, mode, dst, first), (r, acc, frames) in zip(groups, ctx):
        if rank == dst:
            for f in range(3):
                res["%d/frame%d" % (group, f)] = r.readback(frames[f])
    wait(env, "read")              # a rank's send buffers go away with its context: not before the roots have read
    for r, _, _ in ctx:
        r.exchange_destroy()
    return res


@pytest.fixture(scope="module")
def one_rank():
    not_broken()
    out = {first: serial("one_rank", one_rank_script, first) for first in (0, SECOND)}
    for first, res in out.items():
        assert sb.differing_pixels(res["frame0"], res["frame1"]) >= 0.5 and sb.differing_pixels(res["frame1"], res["frame2"]) >= 0.5
    assert sb.differing_pixels(out[0]["frame2"], out[SECOND]["frame2"]) >= 0.5          # the two groups' images differ
    return out


@pytest.mark.parametrize("dst", [0, 2])
@pytest.mark.parametrize("mode", [abi.EXCHANGE_GATHER, abi.EXCHANGE_REDUCE], ids=["gather", "reduce"])
def test_loopback_exchange_with_a_thread_per_rank(side, one_rank, mode, dst):
    """World 3, a thread, a stream and a context per rank, three accumulated frames.  A second group (the other mode, the other root,
    other frames) runs on the same threads' second contexts at the same time.  Each root's frame after every exchange is the one-rank
    running mean of its own group's frames, bit for bit."""
    other_mode = abi.EXCHANGE_REDUCE if mode == abi.EXCHANGE_GATHER else abi.EXCHANGE_GATHER
    ga, gb = 8100 + mode * 10 + dst, 8200 + mode * 10 + dst
    groups = [(ga, mode, dst, 0), (gb, other_mode, 2 - dst, SECOND)]
    got, intervals = run_threads(side, [(rank_script, (k, groups)) for k in range(THREADS)], cap_s("one_rank", "one_rank", "one_rank", "one_rank"))
    assert_overlap(intervals)
    assert sorted(got[dst]) == ["%d/frame%d" % (ga, f) for f in range(3)] and sorted(got[2 - dst]) == ["%d/frame%d" % (gb, f) for f in range(3)] and not got[1]
    assert_same({k.split("/")[1]: v for k, v in got[dst].items()}, one_rank[0], "group %d, root %d" % (ga, dst))
    assert_same({k.split("/")[1]: v for k, v in got[2 - dst].items()}, one_rank[SECOND], "group %d, root %d" % (gb, 2 - dst))


# ---- 4. errors stay with their context -------------------------------------------------------------------------------------------------
REFUSALS = 200


def errors_script(env):
    """One good frame, then 200 refused calls: a bad buffer handle, a null readback target (refused without a text: the last one stays),
    a probe trace at a size that is not the atlas's (another size every time), a bad texture handle.  After each, the code and the
    context's error text; at the end the frame again: nothing was written."""
    s = small_scene(False)
    r = env.R()
    s.upload(r)
    out = poisoned()
    r.trace(settings_of(s), params(s, 0), out)
    res = {"before": r.readback(out)}
    aw, ah = r.set_probes([(0.0, -0.5, 1.2), (0.8, 0.2, 1.0)], 16, columns=2)
    L, h = r.L, r.h
    host = np.zeros(16, np.uint8)
    st = settings_of(s)
    codes, texts = [], []
    for i in range(REFUSALS):
        check(env)
        kind = i % 4
        if kind == 0:
            rc = L.pt_buffer_update(h, 100000 + i, host.ctypes.data_as(C.c_void_p), 16)
        elif kind == 1:
            rc = L.pt_readback(h, C.c_void_p(out.data_ptr()), W, H, None)
        elif kind == 2:
            p = params(s, 0, size=(aw + 1 + i, ah))
            p.output = out.data_ptr()
            rc = L.pt_trace(h, C.byref(st), C.byref(p))
        else:
            rc = L.pt_texture_destroy(h, 100000 + i)
        codes.append(rc)
        texts.append(L.pt_last_error(h))
    assert all(c != 0 for c in codes), codes
    assert all((b"%d x %d" % (aw + 1 + i, ah)) in texts[i] for i in range(2, REFUSALS, 4)), texts[:8]
    res["codes"] = np.array(codes, np.int32)
    res["texts"] = np.frombuffer(b"\n".join(texts), np.uint8).copy()
    res["after"] = r.readback(out)
    return res


def test_errors_stay_with_their_context(side, serial_results):
    """One thread is refused 200 times while two render: its codes and texts are the serial run's, call for call, each text its own
    context's; the renderers' contexts never hold an error text and their images are unchanged."""
    want = serial("errors", errors_script)
    assert sb.same(want["before"], want["after"])
    got, intervals = run_threads(side, [(errors_script, ()), (render_script, ()), (render_script, ())], cap_s("errors", "render", "render"))
    assert_overlap(intervals)
    assert_same(got[0], want, "the refused thread")
    for k in (1, 2):
        assert_same(got[k], serial_results["render"], "renderer on thread %d" % k)


# ---- 5. create / destroy churn ---------------------------------------------------------------------------------------------------------
def churn_script(env):
    """Ten contexts created, uploaded to, traced once and destroyed (pt_destroy's frees synchronise the device implicitly)."""
    s = small_scene(False)
    res = {}
    for i in range(10):
        r = env.R()
        s.upload(r)
        out = poisoned()
        r.trace(settings_of(s), params(s, i), out)
        res["out%d" % i] = r.readback(out)
        r.close()
    return res


CHURN_FRAMES = 128             # the bystanders render about as long as the ten contexts take (0.07 s and 0.07 s serially on the MI355X)


def test_create_destroy_churn_beside_two_renderers(side):
    """One thread creates, uploads to, traces in and destroys ten contexts while two render 128 accumulated frames each: every destroy
    lands in the middle of the others' frames, which must not change."""
    want = serial("churn", churn_script)
    want_render = serial("render128", render_script, CHURN_FRAMES)
    assert len(want_render["last_error"]) == 0 and not sb.same(want_render["bloom0"], want_render["bloom%d" % (CHURN_FRAMES - 1)])
    got, intervals = run_threads(side, [(churn_script, ()), (render_script, (CHURN_FRAMES,)), (render_script, (CHURN_FRAMES,))], cap_s("churn", "render128", "render128"))
    assert_overlap(intervals)
    assert_same(got[0], want, "the churning thread")
    for k in (1, 2):
        assert_same(got[k], want_render, "renderer on thread %d" % k)


# ---- 6. null-stream hooks beside side-stream work --------------------------------------------------------------------------------------
def hooks_script(env, rounds=3):
    """pt_debug_math, pt_debug_sort_pairs and pt_debug_exclusive_scan: test hooks without a context, on the null stream, ending in a
    device synchronise."""
    import ray_hook
    from tests import hooks
    L = hooks.lib()
    inputs = ray_hook.math_inputs(seed=3, n=2000)
    n = 2049                       # one full tile of 2048 and a second block
    rng = np.random.default_rng(n)
    res = {}
    for i in range(rounds):
        for op, (a, b) in inputs.items():
            check(env)
            res["%s@%d" % (op, i)] = ray_hook.gpu_math(op, a, b)
        keys, vals = rng.integers(0, 1 << 63, n, dtype=np.uint64), np.arange(n, dtype=np.uint32)
        check(env)
        assert L.pt_debug_sort_pairs(keys.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), n) == 0
        res["keys@%d" % i], res["vals@%d" % i] = keys.view(np.uint32), vals
        data = rng.integers(0, 400, n, dtype=np.uint32)
        check(env)
        assert L.pt_debug_exclusive_scan(data.ctypes.data_as(C.c_void_p), n) == 0
        res["scan@%d" % i] = data
    return res


def test_null_stream_hooks_beside_side_stream_renderers(side, serial_results):
    """One thread runs the three context-free hooks, whose kernels go to the null stream and end in a device synchronise, while two render
    on their side streams: both sides equal their serial results."""
    want = serial("hooks", hooks_script)
    assert np.array_equal(want["keys@0"].view(np.uint64), np.sort(want["keys@0"].view(np.uint64)))
    got, intervals = run_threads(side, [(hooks_script, ()), (render_script, ()), (render_script, ())], cap_s("hooks", "render", "render"))
    assert_overlap(intervals)
    assert_same(got[0], want, "the hooks")
    for k in (1, 2):
        assert_same(got[k], serial_results["render"], "renderer on thread %d" % k)
