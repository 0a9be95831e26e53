"""GPU tests of the shade stage's LDS table limits (run with -m gpu on an MI355X).

The wavefront shade stage (k_wf_shade, csrc/pt_wavefront.hip) keeps up to 128 instance rows, 96 materials and 32 lights in LDS
(csrc/pt_shading.h kInstCacheMax / kMatCacheMax / kLightCacheMax) and reads whatever lies past a limit from global memory: rows
>= 128 are packed from sc.instances (load_shade_inst), every material header and slot-0..2 descriptor comes from sc.rmats once
the table has more than 96 (material_header / material_slot012), and a light >= 32 is read from memory with its spot-cone terms
computed in light_ray instead of taken from the staged padding (load_light).  launch_wavefront picks one of four shade copies:
<kShadeDefaults, SMALL>, <kShadeDefaultsNoLights, SMALL>, <0, SMALL> while all three tables fit (small_tables), else <0, general>.
The megakernel stages nothing: it is a second implementation over the same tables.

Every table size of the matrix below is compared with the CPU oracle sample for sample (no pixel-sample beyond 1e-3, equal
finiteness, equal ray counts), at each limit, one past each limit, all past and with 0 / 1 light, under flag sets that select each
copy; the first-vertex debug outputs that read the instance row or the material are compared bit for bit; coverage assertions make
sure the high-index rows, materials and lights are actually hit.  A last test resizes the tables across the limits inside one context."""
import importlib.util
import os

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes

pytestmark = pytest.mark.gpu

INST_MAX, MAT_MAX, LIGHT_MAX = 128, 96, 32          # csrc/pt_shading.h kInstCacheMax, kMatCacheMax, kLightCacheMax


def copy_settings(s):
    return abi.PtSettings.from_buffer_copy(bytes(s))


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def _material_fuzz():
    spec = importlib.util.spec_from_file_location("material_fuzz", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "material_fuzz.py"))
    mf = importlib.util.module_from_spec(spec); spec.loader.exec_module(mf)
    return mf


def special_materials(n_mat):
    """The material ids the builder makes textured + normal-mapped (slots 0..2 bound): every id >= 96 and the last six below it."""
    return list(range(min(MAT_MAX, n_mat) - 6, n_mat))


def tables_scene(n_inst, n_mat, n_lights, seed=3):
    """scenes.test_scene (112 x 112, 48^2 textures) with its instance, material and light tables grown (or, for the lights, cut) to
    the given sizes.  Materials: grown with defaults, then all redrawn by tools/material_fuzz.randomize (the camera is kept: the
    coverage below must not depend on a random pose); the ids of special_materials() get slots 0..2 bound and cycle through
    opaque / MASK / double-sided.  Instances: small spheres and quads with UVs, tangents and normal maps, mirrored and non-uniformly
    scaled, placed in the camera's view, every third one with a special material; the rows >= 128 are larger, nearer and take the
    special materials (highest first).  Lights: typed by index (spot, point, directional in turn from index 32, so that 32 itself is
    a spot light), spot lights aimed at the scene, the other fields in material_fuzz's ranges (from index 32 on a range cutoff of 0 or
    8-10, so that they reach the scene); the spot lights at indices 2, 11, 20, 29 and 38 have inner = outer angle."""
    rng = np.random.default_rng(1000 + 7 * n_inst + 13 * n_mat + n_lights + seed)
    s = scenes.test_scene(112, 48, seed=seed)
    assert n_inst >= len(s.instances) and n_mat >= len(s.materials)
    while len(s.materials) < n_mat:
        s.add_material(scenes.material())
    pose = (s.world_to_view, s.y_fov, s.ortho)
    _material_fuzz().randomize(s, rng)
    s.world_to_view, s.y_fov, s.ortho = pose
    n_tex = len(s.textures)
    special = special_materials(n_mat)
    for j, k in enumerate(special):
        m = s.materials[k]
        for slot in ("normal", "albedo", "metallic_roughness"):
            ts = getattr(m, slot)
            if ts.descriptor == -1:
                ts.descriptor = int(rng.integers(0, n_tex)); ts.sampler = 0; ts.tex_coord = 0
        kind = j % 3
        m.alpha_mode = abi.ALPHA_MODE_MASK if kind == 1 else abi.ALPHA_MODE_OPAQUE
        m.alpha_cutoff = 0.5 if kind == 1 else 0.0
        m.flags = abi.MATERIAL_FLAG_DOUBLE_SIDED if kind == 2 else 0
    for k in range(MAT_MAX, n_mat):
        assert all(getattr(s.materials[k], slot).descriptor != -1 for slot in ("normal", "albedo", "metallic_roughness")), k

    # extra instances, placed along random camera rays
    W2V = np.asarray(s.world_to_view, np.float64)
    C2W = np.linalg.inv(camera.view_to_clip(s.width / s.height, s.y_fov, s.z_near, s.z_far) @ W2V)
    cam = np.linalg.inv(W2V)[:3, 3]
    def in_view(nx, ny, dist):
        p = C2W @ np.array([nx, ny, 0.5, 1.0]); p = p[:3] / p[3]
        d = (p - cam) / np.linalg.norm(p - cam)
        return cam + dist * d
    sphere, quad = meshgen.uv_sphere(10, 6, 1.0), meshgen.grid(2, 2, (-1, -1, 0), (2, 0, 0), (0, 2, 0))
    quad.uv1 = quad.uv0 * 2.0
    hi = 0
    for i in range(len(s.instances), n_inst):
        if i >= INST_MAX:
            c = in_view(rng.uniform(-0.75, 0.75), rng.uniform(-0.75, 0.75), rng.uniform(1.3, 2.2)); size = rng.uniform(0.25, 0.4)
            mid = special[len(special) - 1 - hi % len(special)]; hi += 1
        else:
            c = in_view(rng.uniform(-0.95, 0.95), rng.uniform(-0.95, 0.95), rng.uniform(1.5, 3.8)); size = rng.uniform(0.06, 0.14)
            mid = special[len(special) - 1 - (i // 3) % len(special)] if i % 3 == 0 else int(rng.integers(0, n_mat))
        sc = size * rng.uniform(0.6, 1.4, 3) * np.where(rng.random(3) < 0.25, -1.0, 1.0)        # non-uniform, mirrored a quarter of the time per axis
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        s.add_mesh(sphere if i % 2 == 0 else quad, camera.trs(tuple(c), tuple(q), tuple(sc)), mid)
    assert len(s.instances) == n_inst and len(s.materials) == n_mat

    # lights: types by index, the rest of the fields as material_fuzz draws them
    u = lambda a=0.0, b=1.0: float(rng.uniform(a, b))
    while len(s.lights) < n_lights:
        s.add_light(abi.LIGHT_POINT)
    del s.lights[n_lights:]
    for i, l in enumerate(s.lights):
        l.type = (abi.LIGHT_SPOT, abi.LIGHT_POINT, abi.LIGHT_DIRECTIONAL)[(i - LIGHT_MAX) % 3]
        l.position[:] = (u(-3, 3), u(-3, 3), u(0.2, 4))
        d = rng.standard_normal(3)
        if l.type == abi.LIGHT_SPOT:
            d = np.array([u(-1, 1), u(-1, 1), u(0.2, 0.8)]) - np.array(l.position[:])          # aimed at the scene
        l.direction[:] = d / np.linalg.norm(d)
        l.cutoff = float(rng.choice([0.0, u(1, 10) if i < LIGHT_MAX else u(8, 10)])); l.intensity = u(0.5, 30); l.color[:] = (u(), u(), u())
        l.inner_angle = u(0, 1.2); l.outer_angle = l.inner_angle + u(0.05, 0.5)
        if i % 9 == 2 and l.type == abi.LIGHT_SPOT:
            l.outer_angle = l.inner_angle                                                           # the 0.001 floor of the cone scale
    s.name = "tables_%d_%d_%d" % (n_inst, n_mat, n_lights)
    return s


def primary_rays(s):
    """One ray per pixel centre from the camera (float32 rows: origin, tmin, direction, tmax)."""
    W2V = np.asarray(s.world_to_view, np.float64)
    C2W = np.linalg.inv(camera.view_to_clip(s.width / s.height, s.y_fov, s.z_near, s.z_far) @ W2V)
    cam = np.linalg.inv(W2V)[:3, 3]
    y, x = np.mgrid[0:s.height, 0:s.width]
    ndc = np.stack([(x.ravel() + 0.5) / s.width * 2 - 1, 1 - (y.ravel() + 0.5) / s.height * 2, np.full(x.size, 0.5), np.ones(x.size)], axis=1)
    p = ndc @ C2W.T; p = p[:, :3] / p[:, 3:4]
    d = p - cam; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((x.size, 8), np.float32)
    rays[:, 0:3] = cam; rays[:, 4:7] = d; rays[:, 7] = 1000.0
    return rays


# ---- the matrix: table sizes x flag sets x kernel modes, against the oracle sample for sample ---------------------------------------
SIZES = [(128, 96, 32), (129, 96, 32), (128, 97, 32), (128, 96, 33), (150, 110, 40), (11, 9, 0), (11, 9, 1)]
OVER = [z for z in SIZES if z[0] > INST_MAX or z[1] > MAT_MAX or z[2] > LIGHT_MAX]
SWEEP_FLAGS = [abi.FLAG_CULL_BACKFACE, abi.FLAG_LUMINANCE_CLAMP, abi.FLAG_INDIRECT_ENVIRONMENT_ONLY, abi.FLAG_POINT_LIGHTS, abi.FLAG_SHADOW_RAYS,
               abi.FLAG_ALPHA_SHADOWS, abi.FLAG_ENVIRONMENT_MAP, abi.FLAG_ENVIRONMENT_MIS, abi.FLAG_MATERIAL_DIFFUSE_WHITE,
               abi.FLAG_MATERIAL_USE_GEOMETRIC_NORMALS, abi.FLAG_MATERIAL_MIS, abi.FLAG_SHOW_NAN, abi.FLAG_SHOW_INF, abi.FLAG_SHADING_NORMAL_ADAPTATION]
MODES = [abi.MODE_WAVEFRONT, abi.MODE_MEGAKERNEL]
MODE_IDS = ["wavefront", "megakernel"]
size_id = lambda z: "%d-%d-%d" % z


def flag_sets(s):
    """(name, settings, frames): the app defaults without accumulation (shade copy kShadeDefaults while the tables fit), the same
    without point lights (kShadeDefaultsNoLights), with alpha shadows and back-face culling (the general traversal copy), and three
    random sets drawn as in the flag-sweep test of test_gpu_round3 (mostly the <0, ...> shade copy)."""
    base = copy_settings(s.settings); base.flags &= ~abi.FLAG_ACCUMULATE
    assert base.flags == abi.APP_DEFAULT_FLAGS & ~abi.FLAG_ACCUMULATE
    no_lights = copy_settings(base); no_lights.flags &= ~abi.FLAG_POINT_LIGHTS
    trav = copy_settings(base); trav.flags |= abi.FLAG_ALPHA_SHADOWS | abi.FLAG_CULL_BACKFACE
    out = [("defaults", base, [0, 1]), ("no_point_lights", no_lights, [2, 3]), ("alpha_shadows_cull_backface", trav, [4, 5])]
    rng = np.random.default_rng(29)
    for c in range(3):
        st = copy_settings(s.settings)
        fl = 0
        for f in SWEEP_FLAGS:
            if rng.random() < (0.7 if f & abi.APP_DEFAULT_FLAGS else 0.3): fl |= f
        st.flags = fl
        st.max_bounces = int(rng.integers(0, s.bounce_limit + 1)); st.min_bounces = int(rng.integers(0, st.max_bounces + 1))
        st.min_russian_roulette_continue_prob = float(rng.choice([0.0, 0.1, 0.5])); st.max_russian_roulette_continue_prob = float(rng.choice([0.5, 0.9, 1.0]))
        st.luminance_clamp = float(rng.choice([1.0, 10.0, 100.0]))
        st.use_frame_as_seed = int(rng.integers(0, 2)); st.seed = int(rng.integers(0, 1 << 30))
        out.append(("random%d" % c, st, [int(x) for x in rng.integers(0, 1000, 2)]))
    return out


def compare_sample_for_sample(A, B, what):
    """The comparison of test_random_materials_and_lights_...: equal finiteness, no pixel-sample beyond 1e-3 relative error."""
    A = A[..., :3].astype(np.float64); B = B[..., :3].astype(np.float64)
    assert np.array_equal(np.isfinite(A), np.isfinite(B)), what
    fin = np.isfinite(B).all(axis=2)
    rel = np.where(fin, np.abs(A - B).max(axis=2) / np.maximum(np.abs(B).max(axis=2), 1e-4), 0)
    assert (rel > 1e-3).sum() == 0, (what, int((rel > 1e-3).sum()), float(rel.max()))


class OracleSide:
    """A size's scene on the oracle and its renders, kept for the module: the oracle does not depend on the GPU's kernel mode."""

    def __init__(self, oracle_lib, s, env_raw):
        self.s = s
        self.o = oracle_lib.Oracle()
        self.h = s.upload(self.o, env_raw=env_raw)
        self.renders = {}

    def render(self, key, st, frame, params=None):
        """(radiance or debug image, ray count) of one single-sample frame."""
        if key not in self.renders:
            b = np.zeros((self.s.height, self.s.width, 4), np.float32)
            self.o.counters()
            self.o.trace(st, params or self.s.execute_params(frame, env_handle=self.h["env"]), b)
            self.renders[key] = (b, self.o.counters()["rays"])
        return self.renders[key]


_oracles = {}


def setup_pair(R, oracle_lib, size, mode):
    if size not in _oracles:
        s = tables_scene(*size)
        r = R(); hg = s.upload(r)
        _oracles[size] = OracleSide(oracle_lib, s, r.env_read(hg["env"]))
    else:
        s = _oracles[size].s
        r = R(); hg = s.upload(r)
    r.set_kernel_mode(mode)
    return s, r, hg, _oracles[size]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_table_sizes_across_the_lds_limits_match_the_oracle_sample_for_sample(R, oracle_lib, size, mode):
    """Each table size x each flag set, two single-sample frames: no pixel-sample beyond 1e-3 of the oracle's, equal finiteness,
    equal ray counts.  In wavefront mode (128, 96, 32) and the 0- / 1-light scenes run the SMALL shade copies (kShadeDefaults,
    kShadeDefaultsNoLights, <0, SMALL> for the random sets), every other size the general <0, false> copy."""
    s, r, hg, O = setup_pair(R, oracle_lib, size, mode)
    assert (len(s.instances), len(s.materials), len(s.lights)) == size
    og = r.create_output(s.width, s.height)
    for name, st, frames in flag_sets(s):
        for frame in frames:
            r.reset_stats()
            r.trace(st, s.execute_params(frame, env_handle=hg["env"]), og)
            B, rays = O.render((name, frame), st, frame)
            what = (size, MODE_IDS[mode], name, hex(st.flags), frame)
            compare_sample_for_sample(r.readback(og), B, what)
            assert r.stats().rays == rays, what
    r.close()


# debug outputs that read the instance row (transforms, streams) or the material (header, slots)
MATERIAL_DEBUG_OUTPUTS = [abi.DEBUG_OUTPUT_COLOR, abi.DEBUG_OUTPUT_ALPHA, abi.DEBUG_OUTPUT_TEXCOORD_0, abi.DEBUG_OUTPUT_TEXCOORD_1,
                          abi.DEBUG_OUTPUT_SHADING_NORMAL, abi.DEBUG_OUTPUT_SHADING_TANGENT, abi.DEBUG_OUTPUT_METALNESS, abi.DEBUG_OUTPUT_ROUGHNESS,
                          abi.DEBUG_OUTPUT_SPECULAR, abi.DEBUG_OUTPUT_SPECULAR_COLOR, abi.DEBUG_OUTPUT_CLEARCOAT, abi.DEBUG_OUTPUT_CLEARCOAT_NORMAL,
                          abi.DEBUG_OUTPUT_TRANSMISSIVE]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("size", OVER, ids=size_id)
def test_first_vertex_debug_outputs_past_the_limits_are_bit_identical(R, oracle_lib, size, mode):
    """The first-vertex quantities that read the instance row or the material, bit for bit (a NaN on both sides and +0 against -0
    aside), at every size past a limit."""
    s, r, hg, O = setup_pair(R, oracle_lib, size, mode)
    og = r.create_output(s.width, s.height)
    for dbg in MATERIAL_DEBUG_OUTPUTS:
        st = copy_settings(s.settings); st.debug_output = dbg; st.flags &= ~abi.FLAG_ACCUMULATE; st.use_frame_as_seed = 0; st.seed = 4
        r.trace(st, s.execute_params(0, env_handle=hg["env"]), og)
        B, _ = O.render(("debug", dbg), st, 0)
        a, b = r.readback(og)[..., :3], B[..., :3]
        both_nan = np.isnan(a) & np.isnan(b)
        err = (a.view(np.uint32) != b.view(np.uint32)) & ~both_nan & ~((a == 0) & (b == 0))
        assert err.sum() == 0, (size, MODE_IDS[mode], abi.DEBUG_OUTPUT_NAMES[dbg], int(err.sum()))
    r.close()


@pytest.mark.parametrize("size", OVER, ids=size_id)
def test_the_rows_materials_and_lights_past_the_limits_are_hit(R, oracle_lib, size):
    """Coverage of the matrix above: primary rays cast through the product's traversal (pt_debug_intersect) land on instance rows
    >= 128 in at least 2 % of the pixels and on materials >= 96 (slots 0..2 bound) in at least 1 % wherever those tables are past
    their limit; zeroing the intensity of lights 32 and up (on the oracle) changes at least 1 % of the pixel-samples of the
    app-default frames wherever the light table is."""
    from ray_hook import gpu_intersect
    s, r, hg, O = setup_pair(R, oracle_lib, size, abi.MODE_WAVEFRONT)
    n_inst, n_mat, n_lights = size
    h = gpu_intersect(r, primary_rays(s))
    hit = h[:, 0] > 0
    inst = np.where(hit, h[:, 4].astype(np.int64), -1)
    mids = np.array([d.gpu.material_id for d in s.instances])
    mat = np.where(hit, mids[np.maximum(inst, 0)], -1)
    inst_share, mat_share = float((inst >= INST_MAX).mean()), float((mat >= MAT_MAX).mean())
    for k in np.unique(mat[mat >= MAT_MAX]):
        assert all(getattr(s.materials[k], slot).descriptor != -1 for slot in ("normal", "albedo", "metallic_roughness")), k
    light_share = 0.0
    if n_lights > LIGHT_MAX:
        name, st, frames = flag_sets(s)[0]
        full = [O.render((name, frame), st, frame)[0] for frame in frames]
        dark = [abi.PtLight.from_buffer_copy(bytes(l)) for l in s.lights]
        for l in dark[LIGHT_MAX:]: l.intensity = 0.0
        O.o.set_lights(dark)
        changed = 0
        for frame, a in zip(frames, full):
            b = np.zeros((s.height, s.width, 4), np.float32)
            O.o.trace(st, s.execute_params(frame, env_handle=O.h["env"]), b)
            changed += int((b[..., :3] != a[..., :3]).any(axis=2).sum())
        O.o.set_lights(s.lights)
        light_share = changed / (len(frames) * s.width * s.height)
    print("%s: primary hits on instances >= 128 %.4f, on materials >= 96 %.4f; pixel-samples changed by lights >= 32 %.4f"
          % (size_id(size), inst_share, mat_share, light_share))
    if n_inst > INST_MAX: assert inst_share >= 0.02, inst_share
    if n_mat > MAT_MAX: assert mat_share >= 0.01, mat_share
    if n_lights > LIGHT_MAX: assert light_share >= 0.01, light_share
    r.close()


# ---- resizing the tables inside one context -----------------------------------------------------------------------------------------
def test_tables_resized_across_the_limits_in_one_context_match_the_oracle(R, oracle_lib):
    """One Renderer and one Oracle; the material table goes 96 -> 97 -> 96, the instance table 128 -> 129 -> 128 (with an accel
    rebuild), the light table 32 -> 33 -> 0 -> 32, then 40 lights are uploaded with light_count 32 (the SMALL copies: the limit is
    checked against light_count) and 33 (the general copy).  The kernel copy is chosen per launch and rmats is reallocated on the
    host: every frame must match the oracle sample for sample, with equal ray counts."""
    s = tables_scene(129, 97, 40)
    r = R(); hg = s.upload(r)
    o = oracle_lib.Oracle(); ho = s.upload(o, env_raw=r.env_read(hg["env"]))
    mats = {}
    for name, h, b in (("gpu", hg, r), ("oracle", ho, o)):
        mm = []
        for m in s.materials:
            c = abi.PtMaterial.from_buffer_copy(bytes(m))
            for slot in abi.PtMaterial.TEXTURE_SLOTS:
                ts = getattr(c, slot)
                if ts.descriptor != -1: ts.descriptor = h["textures"][ts.descriptor]
                ts.sampler = h["samplers"][ts.sampler]
            mm.append(c)
        mats[name] = mm

    def instances(h, n_inst, n_mat):
        out = []
        for d in h["instances"][:n_inst]:
            c = abi.PtInstanceDesc.from_buffer_copy(bytes(d))
            if c.gpu.material_id >= n_mat: c.gpu.material_id = c.gpu.material_id % n_mat
            out.append(c)
        return out

    st = copy_settings(s.settings); st.flags &= ~abi.FLAG_ACCUMULATE
    og = r.create_output(s.width, s.height); b = np.zeros((s.height, s.width, 4), np.float32)
    # (materials, instances, lights uploaded, light_count)
    states = [(96, 128, 32, 32), (97, 128, 32, 32), (96, 128, 32, 32), (96, 129, 32, 32), (96, 128, 32, 32),
              (96, 128, 33, 33), (96, 128, 0, 0), (96, 128, 32, 32), (96, 128, 40, 32), (96, 128, 40, 33)]
    prev = (97, 129, 40, 40)
    for frame, (n_mat, n_inst, n_lights, light_count) in enumerate(states):
        p_mat, p_inst, p_lights, _ = prev
        for (name, h), be in zip((("gpu", hg), ("oracle", ho)), (r, o)):
            if n_mat < p_mat:                          # the instances first: a shorter material table may not leave an id dangling
                be.set_instances(instances(h, n_inst, n_mat)); be.set_materials(mats[name][:n_mat])
            elif n_mat > p_mat:
                be.set_materials(mats[name][:n_mat]); be.set_instances(instances(h, n_inst, n_mat))
            elif n_inst != p_inst:
                be.set_instances(instances(h, n_inst, n_mat))
            if n_mat != p_mat or n_inst != p_inst:
                be.build_accel()
            if n_lights != p_lights:
                be.set_lights(s.lights[:n_lights])
        prev = (n_mat, n_inst, n_lights, light_count)
        r.reset_stats(); o.counters()
        for be, h, out in ((r, hg, og), (o, ho, b)):
            p = s.execute_params(frame, env_handle=h["env"]); p.light_count = light_count
            be.trace(st, p, out)
        what = (frame, n_mat, n_inst, n_lights, light_count)
        compare_sample_for_sample(r.readback(og), b, what)
        assert r.stats().rays == o.counters()["rays"], what
    r.close(); o.close()
