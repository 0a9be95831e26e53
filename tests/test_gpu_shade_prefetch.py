"""GPU tests of the shade stage's chunk loop (run with -m gpu on an MI355X).

Every wave of k_wf_shade (csrc/pt_wavefront.hip) pulls 64 queue entries at a time from its shard's head counter and shades them: the
entry's records, the hit's shading packet and the path's state records, then the vertex.  How early a wave asks for the records of its
NEXT chunk moves data and changes no operation, so whatever the loop does with them the wavefront pipeline must leave the accumulation
buffer of the megakernel -- which has no chunk loop -- bit for bit, and where the oracle is affordable both must match it sample for
sample (tests/test_gpu_tables.py's bar: equal finiteness, no pixel beyond 1e-3 relative, equal ray counts).

What the cases put into the loop:
  ragged chunks      24 x 20 and 40 x 24 pixels, 1 and 3 samples per trace: partial tiles, so the very first chunk of a wave has lanes past
                     the end of the queue (i >= n);
  steady state       64 x 48 pixels at 64 samples per trace on one workgroup per shard (256 stage workgroups, the smallest grid
                     pt_set_kernel_mode accepts): 768 first-vertex entries per shard, a dozen chunks for four waves, so a wave runs its
                     first chunk, several in a row and a last one; later bounces leave queues that are no multiple of 64 and empty
                     shards.  The same on the default grid;
  a chunk's content  an open scene of quads in front of the sky: hits and misses in one wave, a mesh with a second UV set and vertex
                     colours (the voted second packet fetch) beside meshes without, and EVERY triangle of the scene hit by a camera ray
                     -- triangle 0, whose packet is the one a miss reads, and the last one among them;
  every kernel copy  the app defaults with and without punctual lights, a non-default flag set (the general copy), tables past the LDS
                     limits (<0, general>) and tables exactly at 128 / 96 / 32;
  shard composition  two tile ranks add up to the unsharded image; the same trace twice gives the same bits."""
import numpy as np
import pytest

from gltf_renderer_amd import abi, meshgen, scenes
from test_gpu_shade_parking import copy_settings, parking_scene, run_cases, same_bits

pytestmark = pytest.mark.gpu

ONE_WORKGROUP_PER_SHARD = 256                       # csrc/pt_workspace.h: kShards; fewer stage workgroups are rounded up to it


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


def default_and_no_lights(s):
    base = copy_settings(s.settings); base.reset = 1
    assert base.flags == abi.APP_DEFAULT_FLAGS
    no_lights = copy_settings(base); no_lights.flags &= ~abi.FLAG_POINT_LIGHTS
    return [("defaults", base), ("no_point_lights", no_lights)]


def trace_both(R, s, st, spp, stage_blocks=0, frame=5, **kw):
    """One pt_trace of `spp` samples on the wavefront pipeline and on the megakernel: (wavefront image, megakernel image, ray counts)."""
    out = []
    for mode in (abi.MODE_WAVEFRONT, abi.MODE_MEGAKERNEL):
        r = R(); h = s.upload(r); r.set_kernel_mode(mode, stage_blocks); r.set_samples_per_trace(spp)
        o = r.create_output(s.width, s.height)
        r.reset_stats()
        r.trace(st, s.execute_params(frame, env_handle=h["env"], **kw), o)
        q = r.stats()
        out.append((r.readback(o), (q.rays_primary, q.rays_bounce, q.rays_shadow, q.closest_hits)))
        r.close()
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- ragged chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("size", [(24, 20), (40, 24)], ids=lambda z: "%dx%d" % z)
def test_ragged_first_chunks_leave_the_megakernels_bits_and_the_oracles_samples(R, oracle_lib, size, spp):
    s = parking_scene(*size)
    assert (s.width % 16 or s.height % 16)                              # partial tiles: lanes past the end of a shard's queue
    run_cases(R, oracle_lib, s, default_and_no_lights(s), spp)


# ---- steady state ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage_blocks", [ONE_WORKGROUP_PER_SHARD, 0], ids=["one_workgroup_per_shard", "default_grid"])
def test_a_dozen_chunks_per_shard_leave_the_megakernels_bits(R, stage_blocks):
    s = parking_scene(64, 48)
    spp = 64
    assert s.width * s.height * spp // (256 * 64) == 12                  # first-vertex chunks per shard
    st = copy_settings(s.settings); st.reset = 1
    W, M, rw, rm = trace_both(R, s, st, spp, stage_blocks)
    assert same_bits(W, M), int((W.view(np.uint32) != M.view(np.uint32)).any(axis=2).sum())
    assert rw == rm
    assert rw[0] == s.width * s.height * spp and 0 < rw[1] < rw[0] * s.settings.max_bounces and rw[1] % 64 != 0     # the later queues thin out
    assert rw[3] < rw[0] + rw[1]                                         # some rays escape: misses among the entries


# ---- what a chunk may hold -------------------------------------------------------------------------------------------------------------
def open_scene(width=64, height=48):
    """Three meshes on a plane that faces the camera, the sky around and between them: a 2 x 2 grid with a second UV set and vertex colours
    whose material samples set 1 (albedo) and set 0 (normal map), a plain quad on a set-0 material, and a non-indexed triangle without
    UVs on the default material.  11 triangles, every one of them in view."""
    s = scenes.test_scene(32, 16)
    del s.instances[:]; del s.mesh_records[:]; s.triangles = 0
    TS = abi.PtTextureSample
    m1 = s.add_material(scenes.material(albedo=TS(0, 0, 1), normal=TS(2, 0, 0), metalness_factor=0.0, roughness_factor=0.5))
    m0 = s.add_material(scenes.material(albedo=TS(4, 0, 0), metalness_factor=0.2, roughness_factor=0.4))
    V2W = np.linalg.inv(np.asarray(s.world_to_view, np.float64))
    cam, right, up, fwd = V2W[:3, 3], V2W[:3, 0], V2W[:3, 1], -V2W[:3, 2]
    at = lambda x, y: tuple(cam + 3.0 * fwd + x * right + y * up)
    vec = lambda x, y: tuple(x * right + y * up)
    a = meshgen.grid(2, 2, at(-2.6, -1.5), vec(2.0, 0), vec(0, 3.0))
    a.colors = np.concatenate([np.random.default_rng(2).random((a.num_vertices, 3)), np.ones((a.num_vertices, 1))], axis=1)
    a.uv1 = a.uv0 * 2.5 + 0.25
    s.add_mesh(a, None, m1)
    s.add_mesh(meshgen.grid(1, 1, at(-0.6, -1.6), vec(1.5, 0), vec(0, 2.0)), None, m0)        # edge to edge with the grid: both in one 8 x 8 block
    p = np.array([at(1.9, 0.8), at(3.0, 1.0), at(2.4, 2.4)], np.float32)
    s.add_mesh(meshgen.Mesh(p, None), None, 0)
    assert s.triangles == 11 and s.instances[0].gpu.texcoord_descriptors[1] != -1 and s.instances[0].gpu.color_descriptor != -1
    assert s.instances[1].gpu.texcoord_descriptors[1] == -1 and s.instances[1].gpu.color_descriptor == -1
    s.width, s.height = width, height
    s.name = "open_%dx%d" % (width, height)
    return s


def test_a_chunk_of_hits_and_misses_two_packet_sizes_and_the_first_and_last_triangle(R, oracle_lib):
    from ray_hook import gpu_intersect
    from test_gpu_tables import primary_rays
    s = open_scene()
    r = R(); s.upload(r)
    h = gpu_intersect(r, primary_rays(s))
    r.close()
    hit = h[:, 0] > 0
    seen = set(zip(h[hit, 4].astype(int).tolist(), h[hit, 5].astype(int).tolist()))
    assert len(seen) == s.triangles, sorted(seen)                        # every triangle: the first and the last packet among them
    inst = np.where(hit, h[:, 4].astype(np.int64), -1).reshape(s.height, s.width)
    blocks = [inst[y:y + 8, x:x + 8] for y in range(0, s.height, 8) for x in range(0, s.width, 8)]
    assert any((b == -1).any() and (b >= 0).any() for b in blocks)       # a wave of the first shade launch holds hits and misses
    assert any((b == 0).any() and (b > 0).any() for b in blocks)         # ... and hits with and without the second packet fetch
    s.width, s.height = 40, 24
    run_cases(R, oracle_lib, s, default_and_no_lights(s), 3)
    s.width, s.height = 64, 48
    st = copy_settings(s.settings); st.reset = 1
    W, M, rw, rm = trace_both(R, s, st, 16, ONE_WORKGROUP_PER_SHARD)
    assert same_bits(W, M) and rw == rm


# ---- every copy of the kernel ----------------------------------------------------------------------------------------------------------
def test_the_general_copy_under_a_non_default_flag_set(R, oracle_lib):
    s = parking_scene(40, 24)
    st = copy_settings(s.settings); st.reset = 1
    st.flags |= abi.FLAG_MATERIAL_USE_GEOMETRIC_NORMALS; st.flags &= ~abi.FLAG_SHADING_NORMAL_ADAPTATION
    assert st.flags != abi.APP_DEFAULT_FLAGS and st.flags != abi.APP_DEFAULT_FLAGS & ~abi.FLAG_POINT_LIGHTS
    run_cases(R, oracle_lib, s, [("geometric_normals", st)], 3)


@pytest.mark.parametrize("tables", [(128, 96, 32), (129, 96, 32), (128, 97, 32)], ids=lambda z: "%d-%d-%d" % z)
def test_tables_at_and_past_the_lds_limits(R, oracle_lib, tables):
    """At 128 / 96 / 32 the SMALL copies run with every table full beside the chunk buffers; one instance or one material more runs
    <0, general>."""
    from test_gpu_tables import tables_scene
    s = tables_scene(*tables)
    s.width, s.height = 40, 24
    run_cases(R, oracle_lib, s, default_and_no_lights(s), 3)


# ---- shard composition, repeatability ---------------------------------------------------------------------------------------------------
def test_two_tile_ranks_compose_and_a_trace_repeats(R):
    s = parking_scene(64, 48)
    spp = 8
    r = R(); h = s.upload(r); r.set_samples_per_trace(spp)
    st = copy_settings(s.settings); st.flags &= ~abi.FLAG_ACCUMULATE

    def trace(**kw):
        o = r.create_output(s.width, s.height)
        r.trace(st, s.execute_params(3, env_handle=h["env"], **kw), o)
        return r.readback(o)
    full = trace()
    assert same_bits(full, trace())
    parts = [trace(tile_rank=k, tile_rank_count=2) for k in range(2)]
    assert (parts[0] != 0).any() and (parts[1] != 0).any()
    assert same_bits(parts[0] + parts[1], full)
    assert same_bits(parts[1], trace(tile_rank=1, tile_rank_count=2))
    r.close()
