"""Closed meshes do not leak on the GPU: the rays of tests/watertight_cases.py (aimed at shared edges and vertices, a few ulps beside them, and
at triangle interiors) through both arrangements of the traversal -- traverse() behind pt_debug_intersect, and the wavefront stages' k_wf_trace,
k_wf_shadow and k_wf_traverse behind pt_debug_trace_queues -- for every builder and once more after a refit that moves every instance.
Zero leaks against the float64 expectation, and every output the oracle's to the bit (tests/test_watertight_host.py holds the oracle to the
expectation, and proves that these rays meet the cracks of the plain float test).  Of an occlusion ray that accepts the first hit only
"blocked or not" is defined, so that is what is compared there."""
import numpy as np
import pytest

import watertight_cases as wc
from gltf_renderer_amd import camera
from ray_hook import gpu_intersect, dxr_flags, trace_queues, shadow_rays_of, TQ_TRACE, TQ_SHADOW, TQ_FUSED, RF_CULL_BACK, RF_ACCEPT_FIRST

pytestmark = pytest.mark.gpu

N = 500                       # rays per (placement, side, class): 20 000 per closed mesh
SHADOW_TMAX = 1000.0          # the shadow queue has one tmax for all its rays
CULL = 0x1                    # abi.FLAG_CULL_BACKFACE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Reference:
    """The rays of one mesh under one set of transforms, and what the oracle finds for them."""

    def __init__(self, oracle_lib, name, transforms=None):
        self.cases = wc.mesh_cases(name, N, seed=2, transforms=transforms)
        self.rays = np.concatenate([c["rays"] for c in self.cases])
        self.outside = np.concatenate([np.full(N, not c["inside"]) for c in self.cases])
        self.excused = np.concatenate([wc.gate_refused(c) for c in self.cases])
        assert self.excused.sum() <= 1e-5 * len(self.rays)
        self.shards = np.random.default_rng(7).integers(0, 256, len(self.rays)).astype(np.uint32)
        o = oracle_lib.Oracle(); wc.make_scene(name, transforms).upload(o); o.build_accel()
        self.by_default = o.intersect_many(self.rays, 0, 0)                             # whatever a fresh oracle and a fresh context do
        o.set_watertight(True)
        self.closest = o.intersect_many(self.rays, 0, 0)
        self.culled = o.intersect_many(self.rays[self.outside], dxr_flags(RF_CULL_BACK), 0)
        self.blocked = o.intersect_many(self.rays, dxr_flags(RF_ACCEPT_FIRST), 1)[:, 0] > 0
        far = self.rays.copy(); far[:, 7] = SHADOW_TMAX
        self.blocked_far = o.intersect_many(far, dxr_flags(RF_ACCEPT_FIRST), 1)[:, 0] > 0
        o.close()
        assert not self.leaks(self.closest).any() and self.blocked[~self.excused].all() and self.blocked_far[~self.excused].all()

    def leaks(self, out, only_outside=False):
        """[n] bool: the rays that did not commit the expected hit (and are no refusal of the gate).  only_outside: out holds the outside rays alone."""
        if only_outside:
            full = np.zeros((len(self.rays), 8), np.float32); full[self.outside] = out; out = full
        leak = np.concatenate([~wc.expected(c, out[k * N:(k + 1) * N]) for k, c in enumerate(self.cases)])
        if only_outside: leak &= self.outside
        return leak & ~self.excused


def check_all(r, ref, what):
    """Both arrangements on one built (or refitted) tree."""
    rays, sh = ref.rays, ref.shards
    g = gpu_intersect(r, rays, 0, 0)
    assert not ref.leaks(g).any(), (what, "traverse()", int(ref.leaks(g).sum()))
    assert np.array_equal(bits(g[:, :7]), bits(ref.closest[:, :7])), (what, "traverse()", int((bits(g[:, :7]) != bits(ref.closest[:, :7])).any(1).sum()))
    g = gpu_intersect(r, rays[ref.outside], RF_CULL_BACK, 0)
    assert not ref.leaks(g, True).any() and np.array_equal(bits(g[:, :7]), bits(ref.culled[:, :7])), (what, "traverse(), culling")
    g = gpu_intersect(r, rays, RF_ACCEPT_FIRST, 1)
    assert np.array_equal(g[:, 0] > 0, ref.blocked) and (g[~ref.excused, 0] > 0).all(), (what, "traverse(), occlusion")
    h, _, _, stray = trace_queues(r, rays, sh, flags=0, bounce=0, blocks_per_shard=2, which=TQ_TRACE)
    assert stray[0] == 0 and stray[1] == 0
    assert not ref.leaks(h).any() and np.array_equal(bits(h[:, :7]), bits(ref.closest[:, :7])), (what, "k_wf_trace")
    h, _, _, _ = trace_queues(r, rays[ref.outside], sh[ref.outside], flags=CULL, bounce=0, blocks_per_shard=2, which=TQ_TRACE)
    assert np.array_equal(bits(h[:, :7]), bits(ref.culled[:, :7])), (what, "k_wf_trace, culling")
    want = np.where(ref.blocked_far, np.float32(0.0), np.float32(1.0))
    _, v, _, _ = trace_queues(r, None, None, shadow_rays_of(rays), sh, 1, shadow_tmax=SHADOW_TMAX, flags=0, bounce=0, blocks_per_shard=2, which=TQ_SHADOW)
    assert np.array_equal(v, want) and (v[~ref.excused] == 0).all(), (what, "k_wf_shadow")
    h, v, _, _ = trace_queues(r, rays, sh, shadow_rays_of(rays), sh, 1, shadow_tmax=SHADOW_TMAX, flags=0, bounce=1, blocks_per_shard=2, which=TQ_FUSED)
    assert not ref.leaks(h).any() and np.array_equal(bits(h[:, :7]), bits(ref.closest[:, :7])) and np.array_equal(v, want), (what, "k_wf_traverse")


@pytest.mark.parametrize("name", wc.MESHES)
def test_closed_meshes_do_not_leak_on_either_arrangement_for_any_builder_or_after_a_refit(oracle_lib, name):
    from gltf_renderer_amd.renderer import Renderer
    ref = Reference(oracle_lib, name)
    s = wc.make_scene(name)
    r = Renderer()
    try:
        handles = s.upload(r)
        # a fresh context and a fresh oracle agree, whatever their default is
        g = gpu_intersect(r, ref.rays, 0, 0)
        assert np.array_equal(bits(g[:, :7]), bits(ref.by_default[:, :7])), (name, "default")
        r.set_watertight(True)
        for builder in (0, 1, 2):
            r.set_accel_builder(builder); r.build_accel()
            check_all(r, ref, (name, "builder %d" % builder))
        # every instance moves (rotated, scaled, shifted): a refit, which has to keep the exact vertices of the edge rule current
        moved = [wc.moved_transform(p) for p in wc.PLACEMENTS]
        rows = []
        for d, T in zip(handles["instances"], moved):
            c = type(d).from_buffer_copy(bytes(d))
            c.gpu.transform[:] = camera.cm(T); c.gpu.normal_transform[:] = camera.cm(camera.inverse_transpose(T))
            rows.append(c)
        before = r.stats()
        r.set_instances(rows); r.build_accel()
        after = r.stats()
        assert after.accel_refits == before.accel_refits + 1 and after.accel_builds == before.accel_builds
        check_all(r, Reference(oracle_lib, name, moved), (name, "refitted"))
    finally:
        r.close()


def test_a_frame_traced_with_the_watertight_test_matches_the_oracles(oracle_lib):
    """pt_trace against the oracle's trace with the setting on on both sides: the all-feature scene, eight samples at matched seeds, tone-mapped
    relative L2 within the 1e-3 of every frame parity test here and equal ray counts -- and switching the setting restarts the accumulation."""
    from gltf_renderer_amd import scenes
    from gltf_renderer_amd.renderer import Renderer
    s = scenes.test_scene(64, 32)
    r = Renderer()
    try:
        hg = s.upload(r); r.set_watertight(True)
        o = oracle_lib.Oracle(); ho = s.upload(o, env_raw=r.env_read(hg["env"])); o.set_watertight(True)
        og = r.create_output(s.width, s.height); b = np.zeros((s.height, s.width, 4), np.float32)
        r.reset_stats(); o.counters()                            # (both count from here)
        for f in range(8):
            r.trace(s.settings, s.execute_params(f, env_handle=hg["env"]), og)
            o.trace(s.settings, s.execute_params(f, env_handle=ho["env"]), b)
        ta, tb = r.tonemap(og), oracle_lib.tonemap(b)
        rel = float(np.sqrt(((ta - tb) ** 2).sum() / (tb ** 2).sum()))
        print("\nwatertight frame: rel L2 %.3e" % rel)
        assert rel < 1e-3, rel
        assert r.stats().accumulated_frames == 8 and r.stats().rays == o.counters()["rays"]
        r.set_watertight(False)                                  # another intersection rule: the image starts anew
        r.trace(s.settings, s.execute_params(8, env_handle=hg["env"]), og)
        assert r.stats().accumulated_frames == 1
        o.close()
    finally:
        r.close()
