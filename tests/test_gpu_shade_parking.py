"""GPU tests of the shade stage's LDS parking (run with -m gpu on an MI355X).

k_wf_shade (csrc/pt_wavefront.hip) parks the two UV sets of the hit a lane is shading in the workgroup's LDS (ParkLds, csrc/pt_vertex.h)
and every texture of the vertex reads the set it samples from there; the megakernel keeps them in HitGeom (ParkRegisters).  Parking moves
values and changes no operation, so the two pipelines must leave the same accumulation buffer bit for bit, and both must match the CPU
oracle within the suite's bar for single samples (tests/test_gpu_tables.py: equal finiteness, no pixel beyond 1e-3 relative, equal ray
counts).

The scenes are 24 x 20 and 40 x 24 pixels: one and a half and two and a half tiles across, so queues are a few waves long, waves are partly
filled and a chunk's last wave has idle lanes.  Each is traced with 1 and with 3 samples per pt_trace.  The cases walk every path the
values a vertex carries from its start to its end can take -- the ones the parking experiment moved to LDS (profiles/EXPERIMENTS.md): an
environment sample only, a punctual light only, both, neither; a transmissive material (the bounce leaves from o_below); a material that
samples the second UV set, and both sets in one material, next to materials on the first set in the same wave; the debug outputs that
overwrite the colour after the follow-ups were queued; max_bounces 0 and 1.  A last case has the instance, material and light tables at
their LDS limits (128 / 96 / 32)."""
import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, scenes

pytestmark = pytest.mark.gpu

SIZES = [(24, 20), (40, 24)]
SPP = [1, 3]
BOUNCE_DEBUG_OUTPUTS = [abi.DEBUG_OUTPUT_BOUNCE_DIRECTION, abi.DEBUG_OUTPUT_BOUNCE_BSDF, abi.DEBUG_OUTPUT_BOUNCE_PDF, abi.DEBUG_OUTPUT_BOUNCE_WEIGHT,
                        abi.DEBUG_BOUNCE_IS_TRANSMISSION]
WALL = 1                                              # the instance of scenes.test_scene with two UV sets: the back wall


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def parking_scene(width, height):
    """scenes.test_scene (16^2 textures) at width x height, its back wall -- the mesh with a second UV set -- given a material whose albedo
    and emissive textures sample set 1 and whose normal map samples set 0; the floor under it and the spheres in front sample set 0."""
    s = scenes.test_scene(32, 16)
    TS = abi.PtTextureSample
    m = s.add_material(scenes.material(albedo=TS(4, 0, 1), normal=TS(2, 0, 0), emissive=TS(3, 0, 1, 0.2, (0.3, 0.1), (1.5, 0.5)), emissive_factor=(0.5, 0.5, 0.5),
                                       metalness_factor=0.0, roughness_factor=0.6))
    assert s.instances[WALL].gpu.texcoord_descriptors[1] != -1
    s.instances[WALL].gpu.material_id = m
    s.width, s.height = width, height
    s.name = "parking_%dx%d" % (width, height)
    return s


def cases(s):
    """(name, settings) of every case; all accumulate from a reset."""
    base = copy_settings(s.settings); base.reset = 1
    assert base.flags == abi.APP_DEFAULT_FLAGS and base.max_bounces == 4
    env_only = copy_settings(base); env_only.flags &= ~abi.FLAG_POINT_LIGHTS
    light_only = copy_settings(base); light_only.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS); light_only.environment_color[:] = (0.6, 0.7, 0.9)
    neither = copy_settings(base); neither.flags &= ~(abi.FLAG_POINT_LIGHTS | abi.FLAG_ENVIRONMENT_MIS)
    out = [("both", base), ("environment_only", env_only), ("light_only", light_only), ("neither", neither)]
    for dbg in BOUNCE_DEBUG_OUTPUTS:
        st = copy_settings(base); st.debug_output = dbg
        out.append((abi.DEBUG_OUTPUT_NAMES[dbg], st))
    for mb in (0, 1):
        st = copy_settings(base); st.max_bounces = mb; st.min_bounces = 0
        out.append(("max_bounces_%d" % mb, st))
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def compare_sample_for_sample(A, B, what):
    """tests/test_gpu_tables.py's bar: equal finiteness, no pixel beyond 1e-3 relative error."""
    A = A[..., :3].astype(np.float64); B = B[..., :3].astype(np.float64)
    assert np.array_equal(np.isfinite(A), np.isfinite(B)), what
    fin = np.isfinite(B).all(axis=2)
    rel = np.where(fin, np.abs(A - B).max(axis=2) / np.maximum(np.abs(B).max(axis=2), 1e-4), 0)
    assert (rel > 1e-3).sum() == 0, (what, int((rel > 1e-3).sum()), float(rel.max()))


def run_cases(R, oracle_lib, s, case_list, spp, first_frame=5):
    """Every case on the wavefront pipeline, the megakernel and the oracle: `spp` samples accumulated from a reset (one pt_trace of `spp`
    on the GPU, `spp` calls in the oracle; a debug output is not batched -- pt_trace then stands for one call whatever the batch is set
    to).  Wavefront == megakernel bit for bit, both against the oracle, equal ray counts."""
    rw = R(); hw = s.upload(rw); rw.set_kernel_mode(abi.MODE_WAVEFRONT); rw.set_samples_per_trace(spp)
    rm = R(); hm = s.upload(rm); rm.set_kernel_mode(abi.MODE_MEGAKERNEL); rm.set_samples_per_trace(spp)
    o = oracle_lib.Oracle(); ho = s.upload(o, env_raw=rw.env_read(hw["env"]))
    ow, om = rw.create_output(s.width, s.height), rm.create_output(s.width, s.height)
    images = {}
    for name, st in case_list:
        what = (s.name, spp, name)
        n = spp if st.debug_output == abi.DEBUG_OUTPUT_NONE else 1
        rw.reset_stats(); rm.reset_stats(); o.counters()
        rw.trace(st, s.execute_params(first_frame, env_handle=hw["env"]), ow)
        rm.trace(st, s.execute_params(first_frame, env_handle=hm["env"]), om)
        b = np.zeros((s.height, s.width, 4), np.float32)
        so = copy_settings(st); oracle_rays = 0
        for f in range(n):
            o.trace(so, s.execute_params(first_frame + f, env_handle=ho["env"]), b); so.reset = 0
            oracle_rays += o.counters()["rays"]
        W, M = rw.readback(ow), rm.readback(om)
        assert rw.stats().accumulated_frames == n and rm.stats().accumulated_frames == n, what
        assert same_bits(W, M), (what, int((W.view(np.uint32) != M.view(np.uint32)).any(axis=2).sum()))
        compare_sample_for_sample(W, b, what)
        assert rw.stats().rays == oracle_rays and rm.stats().rays == oracle_rays, (what, rw.stats().rays, rm.stats().rays, oracle_rays)
        images[name] = W
    rw.close(); rm.close(); o.close()
    return images


@pytest.mark.parametrize("spp", SPP)
@pytest.mark.parametrize("size", SIZES, ids=lambda z: "%dx%d" % z)
def test_every_path_of_the_parked_values_leaves_the_megakernels_bits(R, oracle_lib, size, spp):
    s = parking_scene(*size)
    img = run_cases(R, oracle_lib, s, cases(s), spp)
    # the cases are the paths they are named after: the lights and the environment sample each change the image, the transmission debug
    # output shows refracted bounces (green) next to reflected ones (red), and a path of no bounce differs from one of one
    assert not same_bits(img["both"], img["environment_only"]) and not same_bits(img["both"], img["light_only"])
    assert not same_bits(img["neither"], img["environment_only"]) and not same_bits(img["max_bounces_0"], img["max_bounces_1"])
    tr = img[abi.DEBUG_OUTPUT_NAMES[abi.DEBUG_BOUNCE_IS_TRANSMISSION]]
    assert (tr[..., 1] > 0).any() and (tr[..., 0] > 0).any()


@pytest.mark.parametrize("size", SIZES, ids=lambda z: "%dx%d" % z)
def test_a_wave_holds_hits_on_both_uv_sets(R, size):
    """Coverage of the scene: some 8 x 8 pixel block -- a wave of the first shade launch -- has primary hits on the wall (albedo and
    emissive on UV set 1, normal map on set 0) and on the floor or a sphere (set 0), and the wall's set-1 coordinates differ from its
    set-0 ones there (TEXCOORD_0 / TEXCOORD_1 debug outputs)."""
    from ray_hook import gpu_intersect
    s = parking_scene(*size)
    r = R(); hg = s.upload(r)
    W2V = np.asarray(s.world_to_view, np.float64)
    C2W = np.linalg.inv(camera.view_to_clip(s.width / s.height, s.y_fov, s.z_near, s.z_far) @ W2V)
    cam = np.linalg.inv(W2V)[:3, 3]
    y, x = np.mgrid[0:s.height, 0:s.width]
    ndc = np.stack([(x.ravel() + 0.5) / s.width * 2 - 1, 1 - (y.ravel() + 0.5) / s.height * 2, np.full(x.size, 0.5), np.ones(x.size)], axis=1)
    p = ndc @ C2W.T; p = p[:, :3] / p[:, 3:4]
    d = p - cam; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((x.size, 8), np.float32)
    rays[:, 0:3] = cam; rays[:, 4:7] = d; rays[:, 7] = 1000.0
    h = gpu_intersect(r, rays)
    inst = np.where(h[:, 0] > 0, h[:, 4].astype(np.int64), -1).reshape(s.height, s.width)
    mixed = 0
    for by in range(0, s.height, 8):
        for bx in range(0, s.width, 8):
            blk = inst[by:by + 8, bx:bx + 8]
            mixed += int((blk == WALL).any() and ((blk >= 0) & (blk != WALL)).any())
    assert mixed >= 1, inst
    uv = []
    og = r.create_output(s.width, s.height)
    for dbg in (abi.DEBUG_OUTPUT_TEXCOORD_0, abi.DEBUG_OUTPUT_TEXCOORD_1):
        st = copy_settings(s.settings); st.debug_output = dbg; st.flags &= ~abi.FLAG_ACCUMULATE; st.use_frame_as_seed = 0; st.seed = 4
        r.trace(st, s.execute_params(0, env_handle=hg["env"]), og)
        uv.append(r.readback(og)[..., :2].copy())
    r.close()
    assert (np.abs(uv[0] - uv[1]).max(axis=2) > 0.05).any()


def test_tables_at_their_lds_limits(R, oracle_lib):
    """128 instances, 96 materials and 32 lights -- the SMALL shade copies with every LDS table full beside the parking -- at 40 x 24,
    under the app defaults (the copy for punctual lights) and without point lights (the copy without), 3 samples per trace."""
    from test_gpu_tables import tables_scene
    s = tables_scene(128, 96, 32)
    s.width, s.height = 40, 24
    base = copy_settings(s.settings); base.reset = 1
    assert base.flags == abi.APP_DEFAULT_FLAGS
    no_lights = copy_settings(base); no_lights.flags &= ~abi.FLAG_POINT_LIGHTS
    run_cases(R, oracle_lib, s, [("defaults", base), ("no_point_lights", no_lights)], 3)
