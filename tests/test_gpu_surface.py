"""The vertex fetch and the material evaluation of a path vertex (pt_shading.h: load_shade_packet_*, load_shade_inst, get_vertex_attributes,
get_surface with fetch_pbr_texels, emissive_of; pt_vertex.h: the back-face flip and offset_ray as shade_closest_hit runs them; pt_traverse.h:
candidate_alpha), query by query, through the test hook pt_debug_surface_query on both kernel builds:
  unit 0  the wavefront build: lookup tables, instance rows and materials staged into LDS as k_wf_shade stages them, with small_tables as the
          shade kernel's SMALL copy has it wherever the scene fits, and without;
  unit 1  the megakernel build: every table in global memory.

Every GPU query set is checked
  A  unit 0 against the CPU oracle (orc_surface_query_many: GetVertexAttributes, the flip, OffsetRay, GetSurfaceProperties, GetEmissive and
     the any-hit base colour, the functions pathtrace_scene calls): all 72 output floats bit-identical, NaN positions included (payloads
     are not compared); no tolerance and no signed-zero allowance;
  B  unit 0 against unit 1, and small_tables 1 against 0: bit-identical;
  C  on the well-conditioned sets, the oracle against tests/surface_ref.py, a float64 restatement from the shader text, within the bounds
     C_BOUND below (CPU only: the oracle is the same code on the GPU host).

Query i runs in lane i % 64 of wave i / 64 (the hook's contract), so the tests compose waves by ordering the queries: the second packet
fetch, the interleaved / general texel fetch and the edge reload are behind votes of a wave's active lanes.

What this does NOT show: the hook compiles the same source functions in the same translation units with the same flags as the shade
kernels, but it is not the machine code of the k_wf_shade copies or of pt_megakernel; the tie test at the end and the image tests are the
check on those.  The NEE / Russian-roulette control flow of shade_closest_hit is not run here.

The tests that carry no gpu mark run the same query sets on the oracle alone: check C, orc_surface_query_many against the debug outputs
of pathtrace_scene on a small frame, and the non-vacuity conditions of every set (so the seeds are proven without a GPU)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from gltf_renderer_amd import abi, camera, meshgen, scenes
from tests import hooks

import surface_ref
from accel_hook import accel_read

f32 = np.float32
u32 = np.uint32
ADAPT, GEOM = abi.FLAG_SHADING_NORMAL_ADAPTATION, abi.FLAG_MATERIAL_USE_GEOMETRIC_NORMALS
FLAG_SETS = [0, ADAPT, GEOM, ADAPT | GEOM]
OUT = 72
SLOTS = abi.PtMaterial.TEXTURE_SLOTS
INST_MAX, MAT_MAX = 128, 96                      # csrc/pt_shading.h kInstCacheMax, kMatCacheMax
ONE_BELOW, TINY = np.nextafter(f32(1), f32(0)), np.nextafter(f32(0), f32(1))

# Non-vacuity, stated once and asserted on the ORACLE's outputs (so that the CPU tests at the end prove the seeds):
MIN_BACK_SHARE = 0.25             # of every set's queries are back faces
MIN_ADAPTED = 100                 # queries of the material set whose shading normal NormalAdaptation changes, and as many it leaves alone
MAX_NON_FINITE = 0.001            # share of non-finite output floats on the sets that are not degenerate
MAX_ILL_CONDITIONED = 0.10        # share of a well-conditioned set's queries check C may leave out (surface_ref's predicate)
# Also asserted there: both sides of the MASK comparison and the exact tie are hit; every slot bound alone changes the record of its
# unbound twin; interleaved-footprint (RM_TRIO) and general materials are both in the material set (counted on the GPU by
# pt_debug_interleaved_materials / _emissive against TRIO_EXPECTED); every degenerate kind that must produce a NaN does.

# Check C: the oracle's largest deviation from float64 per output group, |oracle - float64| / max(1, |float64|), measured over the
# well-conditioned queries of the vertex set (flags 0) and of the material set under all four flag sets (x86-64, gcc -O2
# -ffp-contract=off): position 4.115e-6 (the vertex set's instances scaled by 100: 100 x 2^-24 a term), unit vectors 1.241e-5 (a
# normalised vector 1e-2 of its inputs' scale amplifies a rounding a hundredfold), colours and scalars 7.43e-7, roughnesses 6.39e-7,
# offset origins 4.113e-6 (the position's).  The constants are those values rounded up; the bound is 4 x: the margin is for another libm
# and compiler where the oracle is rebuilt.
C_MEASURED = {"position": 4.2e-6, "unit vectors": 1.25e-5, "colours and scalars": 7.5e-7, "roughnesses": 6.4e-7, "offset origins": 4.2e-6}
C_BOUND = {k: 4 * v for k, v in C_MEASURED.items()}


# ---------------------------------------------------------------- meshes
class RawMesh(meshgen.Mesh):
    """A mesh whose index format (None: not indexed, 16, 32) and packed tangent-space words can be set directly."""
    index_bits = 16
    ts_words = None

    def index_stream(self):
        if self.indices is None:
            return None, None
        return (self.indices.astype(np.uint16), abi.FORMAT_R16_UINT) if self.index_bits == 16 else (self.indices.astype(np.uint32), abi.FORMAT_R32_UINT)

    def tangent_space_stream(self):
        return self.ts_words if self.ts_words is not None else super().tangent_space_stream()


def unit_rows(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def random_mesh(rng, n_tris, tangent_space, uv0, uv1, colours, index_bits):
    """Random triangles in [-1, 1]^3 (sides of order one) with random unit normals, tangents perpendicular to them and both windings."""
    nv = 3 * n_tris if index_bits is None else n_tris + 3
    p = rng.uniform(-1, 1, (nv, 3))
    idx = None if index_bits is None else np.stack([rng.permutation(nv)[:3] for _ in range(n_tris)]).reshape(-1)
    nrm = unit_rows(rng.standard_normal((nv, 3)))
    t = rng.standard_normal((nv, 3)); t = unit_rows(t - (t * nrm).sum(1, keepdims=True) * nrm)
    t4 = np.concatenate([t, rng.choice([-1.0, 1.0], (nv, 1))], 1)
    m = RawMesh(p, idx, nrm if tangent_space else None, t4 if tangent_space else None, rng.uniform(-1, 2, (nv, 2)) if uv0 else None,
                rng.uniform(-1, 2, (nv, 2)) if uv1 else None, rng.uniform(0, 1, (nv, 4)) if colours else None)
    m.index_bits = index_bits
    return m


def rotation(rng):
    q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    q[:, 0] *= np.sign(np.linalg.det(q))
    return q


def affine(linear, translation=(0, 0, 0)):
    T = np.eye(4)
    T[:3, :3] = linear; T[:3, 3] = translation
    return T


# ---------------------------------------------------------------- query sets
class Queries:
    """Hits addressed by (instance, primitive): front 0 / 1, barycentrics u, v, ray direction d."""
    def __init__(self, inst, prim, front, u, v, d):
        self.inst, self.prim, self.front = np.asarray(inst, u32), np.asarray(prim, u32), np.asarray(front, u32)
        self.u, self.v, self.d = np.asarray(u, f32), np.asarray(v, f32), np.ascontiguousarray(d, f32)

    def __len__(self):
        return len(self.inst)

    def take(self, index):
        return Queries(self.inst[index], self.prim[index], self.front[index], self.u[index], self.v[index], self.d[index])

    def records(self, packet=None):
        """The hook's (n, 8) input records; word 0 = packet[(instance, primitive)] (0 without a map: the oracle does not read it)."""
        r = np.zeros((len(self), 8), f32)
        w = r.view(u32)
        if packet is not None:
            w[:, 0] = [packet[k] for k in zip(self.inst.tolist(), self.prim.tolist())]
        w[:, 1] = self.front
        r[:, 2], r[:, 3], r[:, 4:7] = self.u, self.v, self.d
        return r


SPECIAL_BARY = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (f32(1) / f32(3), f32(1) / f32(3)), (0.25, 0.75), (0.375, 0.625),
                (TINY, TINY), (TINY, 0), (ONE_BELOW, 0), (0, ONE_BELOW), (ONE_BELOW, TINY)]     # vertices, edge midpoints, centroid, u + v == 1, nextafter of 0 and of 1


def world_normal(scene, inst, prim):
    """The unit geometric normal of a triangle in world space, float64 (only to aim grazing views)."""
    g = scene.instances[inst].gpu
    P = scene.buffers[g.position_descriptor][0].reshape(-1, 3).astype(np.float64)
    vi = np.array([3 * prim, 3 * prim + 1, 3 * prim + 2])
    if g.index_descriptor != -1:
        vi = scene.buffers[g.index_descriptor][0].astype(np.int64)[vi]
    n = np.array(g.normal_transform[:], np.float64).reshape(4, 4).T[:3, :3] @ np.cross(P[vi[1]] - P[vi[0]], P[vi[2]] - P[vi[0]])
    return n / max(np.linalg.norm(n), 1e-300)


def instance_queries(rng, scene, inst, n_tris, per_tri, specials):
    """per_tri queries on every triangle of an instance: the special barycentrics first, random ones after; two fifths back faces; seven tenths
    of the ray directions uniform on the sphere, three tenths grazing the triangle's plane from either side."""
    rows = []
    for prim in range(n_tris):
        ng = world_normal(scene, inst, prim)
        a = np.cross(ng, [1.0, 0, 0] if abs(ng[0]) < 0.9 else [0, 1.0, 0]); a /= max(np.linalg.norm(a), 1e-300); b = np.cross(ng, a)
        for k in range(per_tri):
            if k < len(specials):
                u, v = specials[k]
            else:
                u = rng.uniform(0, 1); v = rng.uniform(0, 1 - u)
            if rng.random() < 0.3 and np.isfinite(a).all():
                phi = rng.uniform(0, 2 * math.pi)
                d = -(math.cos(phi) * a + math.sin(phi) * b + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, -0.5) * ng)
            else:
                d = rng.standard_normal(3)
            rows.append((inst, prim, 0 if rng.random() < 0.4 else 1, u, v, d * 10.0 ** rng.uniform(-1, 1)))
    return rows


def to_queries(rows):
    return Queries([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], np.array([r[5] for r in rows]))


class Case:
    def __init__(self, name, scene, queries, flag_sets=(0,), info=None):
        self.name, self.scene, self.q, self.flag_sets, self.info = name, scene, queries, tuple(flag_sets), info or {}
        self._oracle, self._expected = None, {}

    def expected(self, oracle_lib, flags):
        """The oracle's records of the set under `flags`: computed once, shared, read-only."""
        if flags not in self._expected:
            if self._oracle is None:
                self._oracle = oracle_lib.Oracle()
                self.scene.upload(self._oracle)
            e = self._oracle.surface_query_many(flags, self.q.records(), self.q.inst, self.q.prim)
            e.setflags(write=False)
            self._expected[flags] = e
        return self._expected[flags]


def new_scene(name):
    s = scenes.SceneData(name)
    s.smp_wrap = s.add_sampler(abi.ADDRESS_WRAP, abi.ADDRESS_WRAP, abi.FILTER_LINEAR, abi.FILTER_LINEAR)
    s.smp_point = s.add_sampler(abi.ADDRESS_CLAMP, abi.ADDRESS_CLAMP, abi.FILTER_POINT, abi.FILTER_POINT)
    s.smp_mirror = s.add_sampler(abi.ADDRESS_MIRROR, abi.ADDRESS_WRAP, abi.FILTER_LINEAR, abi.FILTER_LINEAR)
    return s


def bind(m, slot, tex, smp, tex_coord=0, rotation=0.0, offset=(0.0, 0.0), scale=(1.0, 1.0)):
    setattr(m, slot, abi.PtTextureSample(tex, smp, tex_coord, rotation, offset, scale))


def random_factors(rng):
    m = abi.PtMaterial.default()
    u = lambda a=0.0, b=1.0: float(rng.uniform(a, b))
    m.base_color_factor[:] = (u(0.2, 1), u(0.2, 1), u(0.2, 1), u(0.2, 1))
    m.metalness_factor, m.roughness_factor = u(), u(0.1, 1)
    m.emissive_factor[:] = (u(0, 2), u(0, 2), u(0, 2))
    m.ior, m.normal_scale, m.clearcoat_normal_scale = u(1.1, 2), u(0.5, 1.5), u(0.5, 1.5)
    m.specular_factor = u(); m.specular_color_factor[:] = (u(), u(), u())
    m.clearcoat_factor, m.clearcoat_roughness_factor = u(), u(0.1, 1)
    m.anisotropy_strength, m.anisotropy_rotation = u(0.1, 1), u(-math.pi, math.pi)
    m.sheen_color_factor[:] = (u(), u(), u()); m.sheen_roughness_factor = u(0.1, 1)
    m.transmission_factor, m.thickness_factor = u(), u()
    return m


def copy_material(m):
    return abi.PtMaterial.from_buffer_copy(bytes(m))


# ---------------------------------------------------------------- the vertex set
STREAMS = {"none": (0, 0, 0, 0), "tangent space": (1, 0, 0, 0), "+uv0": (1, 1, 0, 0), "+uv1": (1, 1, 1, 0), "+colour": (1, 1, 0, 1), "all": (1, 1, 1, 1)}
TRANSFORMS = ["identity", "rotation + 1e3", "scale (1, 0.01, 100)", "mirrored"]


@functools.lru_cache(None)
def vertex_case():
    """Six stream combinations x four instance transforms, index formats none / 16 / 32 bits in turn, 8 random triangles a mesh; the
    all-streams mesh once more under a second material.  Two materials read both UV sets and the vertex colours through textures."""
    rng = np.random.default_rng(20261019)
    s = new_scene("surface_vertex")
    t0 = s.add_texture(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), True)
    t1 = s.add_texture(rng.integers(0, 256, (3, 5, 4), dtype=np.uint8), False)
    ma = random_factors(rng); bind(ma, "albedo", t0, s.smp_wrap, 0); bind(ma, "normal", t1, s.smp_mirror, 1, 0.3, (0.13, 0.21), (1.5, 0.75))
    mb = random_factors(rng); bind(mb, "albedo", t1, s.smp_mirror, 1); bind(mb, "emissive", t0, s.smp_wrap, 0); mb.alpha_mode = abi.ALPHA_MODE_BLEND
    ida, idb = s.add_material(ma), s.add_material(mb)
    rows, kinds = [], {}
    k = 0
    for sname, st in STREAMS.items():
        for tname in TRANSFORMS:
            mesh = random_mesh(rng, 8, *st, index_bits=[None, 16, 32][k % 3])
            R = rotation(rng)
            T = {"identity": np.eye(4), "rotation + 1e3": affine(R, rng.uniform(-1, 1, 3) * 1e3), "scale (1, 0.01, 100)": affine(R @ np.diag([1, 0.01, 100.0]), (1, 2, 3)),
                 "mirrored": affine(R @ np.diag([-1.3, 0.8, 1.1]), (-2, 0.5, 4))}[tname]
            inst = s.add_mesh(mesh, T, ida if k % 2 == 0 else idb)
            kinds[inst] = (sname, tname, mesh.index_bits)
            rows += instance_queries(rng, s, inst, 8, 20, SPECIAL_BARY)
            if sname == "all" and tname == "identity":
                twin = s.add_mesh(mesh, T, idb if k % 2 == 0 else ida)          # one mesh instanced twice with different materials
                kinds[twin] = (sname, tname + " (second material)", mesh.index_bits)
                rows += instance_queries(rng, s, twin, 8, 20, SPECIAL_BARY)
            k += 1
    # Coordinates of 1e12 under a scale of 1e-10: cross(p1 - p0, p2 - p0) is of the order 1e24 and its squared length is past float32, so the
    # geometric normal survives only because it is transformed UN-normalised (:292, by a normal matrix given here with the scale 1e-20: the
    # API takes the two matrices as they come, and a normalised vector does not depend on that scale).
    mesh = random_mesh(rng, 8, 1, 1, 0, 0, 16)
    mesh.positions *= f32(1e12)
    mesh.normals = unit_rows(np.array([0.3, -0.5, 0.8]) + rng.uniform(-0.3, 0.3, mesh.normals.shape)).astype(f32)     # normals that do not cancel when interpolated
    R = rotation(rng)
    inst = s.add_mesh(mesh, affine(R * 1e-10, (1, 2, 3)), ida)
    s.instances[inst].gpu.normal_transform[:] = camera.cm(affine(R * 1e-20))
    kinds[inst] = ("+uv0", "coordinates of 1e12", 16)
    rows += instance_queries(rng, s, inst, 8, 20, SPECIAL_BARY)
    return Case("vertex", s, to_queries(rows), info=dict(kinds=kinds))


# ---------------------------------------------------------------- the degenerate set (checks A and B only)
DEGENERATE_MUST_NAN = ["zero-area triangle", "tangent parallel to the normal", "zero instance scale"]


@functools.lru_cache(None)
def degenerate_case():
    rng = np.random.default_rng(20261020)
    s = new_scene("surface_degenerate")
    tex = s.add_texture(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), False)
    m = random_factors(rng); bind(m, "normal", tex, s.smp_wrap); bind(m, "albedo", tex, s.smp_wrap)
    mid = s.add_material(m)
    rows, kinds = [], {}

    def add(kind, mesh, T=None, transform=None, normal_transform=None, n_tris=2):
        """transform / normal_transform: the instance's two matrices set directly (the API takes both as they come)."""
        inst = s.add_mesh(mesh, T, mid)
        if transform is not None:
            s.instances[inst].gpu.transform[:] = camera.cm(affine(transform))
        if normal_transform is not None:
            s.instances[inst].gpu.normal_transform[:] = camera.cm(affine(normal_transform))
        kinds[inst] = kind
        rows.extend(instance_queries(rng, s, inst, n_tris, 48, SPECIAL_BARY))

    flat = random_mesh(rng, 2, 0, 1, 0, 0, 16)
    flat.positions[flat.indices[2]] = flat.positions[flat.indices[1]]                     # triangle 0 has two equal corners
    flat.positions[flat.indices[5]] = 2 * flat.positions[flat.indices[4]] - flat.positions[flat.indices[3]]   # triangle 1's corners are collinear
    add("zero-area triangle", flat)
    quad = meshgen.grid(1, 1, (-1, -1, 0), (2, 0, 0), (0, 2, 0))
    bare = RawMesh(quad.positions, quad.indices, uv0=quad.uv0)      # no tangent space: ng = (0, 0, 4) exactly, GenerateTangent gives (0, -1, 0) exactly
    add("tangent parallel to the normal", bare, normal_transform=np.array([[1.0, 0, 0], [0, 0, 1], [0, 1, 0]]))    # the normal matrix sends the normal to +y: cross(n, t) = 0
    add("zero instance scale", bare, transform=np.diag([1.0, 0, 1]), normal_transform=np.eye(3))                   # the tangent's axis is scaled to nothing
    for word in (0, 0xffffffff):
        w = RawMesh(quad.positions, quad.indices, quad.normals, quad.tangents, quad.uv0)
        w.ts_words = np.full(len(quad.positions), word, np.uint32)
        add("tangent-space word %#x" % word, w, affine(rotation(rng)))
    opp = RawMesh(quad.positions, quad.indices, quad.normals.copy(), quad.tangents, quad.uv0)
    opp.normals[opp.indices[1]] = (0, 0, -1)                                               # opposite normals at two vertices of triangle 0: they cancel at the midpoint (0.5, 0), up to the 10-bit packing
    add("cancelling normals", opp)
    return Case("degenerate", s, to_queries(rows), flag_sets=(0, ADAPT), info=dict(kinds=kinds))


# ---------------------------------------------------------------- the material set
TRIO_EXPECTED = (3, 1)          # materials reading the interleaved footprint, and those of them whose emissive texture rides in it


@functools.lru_cache(None)
def material_case():
    """One instance a material on a 2 x 2 grid with every stream (a second grid without colours for the exact MASK products), under a
    slight rotation so that no normal is axis-aligned.  Vertex 0 of triangle 0 has uv0 (0.5, 0.25): through a binding without a UV transform
    (the anisotropy texture that cancels) the weight-1/2 point between the two columns of a 2-texel-wide row.  Which hits have a
    footprint over the WRAP seam depends on each binding's transform: albedo_edge() tells, from the float64 sampler's taps."""
    rng = np.random.default_rng(20261021)
    s = new_scene("surface_material")
    g = meshgen.grid(2, 2, (-1, -1, 0), (2, 0, 0), (0, 2, 0))
    nv = len(g.positions)
    nrm = unit_rows(g.normals + rng.uniform(-0.3, 0.3, (nv, 3)))
    tan = g.tangents.copy(); tan[:, :3] = unit_rows(tan[:, :3] + rng.uniform(-0.3, 0.3, (nv, 3))); tan[:, 3] = rng.choice([-1.0, 1.0], nv)
    uv0 = rng.uniform(-1, 2, (nv, 2)); uv0[g.indices[0]] = (0.5, 0.25); uv0[g.indices[1]] = (0.01, 0.3)
    full = RawMesh(g.positions, g.indices, nrm, tan, uv0, rng.uniform(-1, 2, (nv, 2)), rng.uniform(0.3, 1, (nv, 4)))
    plain = RawMesh(g.positions, g.indices, nrm, tan, uv0)
    tex = lambda shape, srgb: s.add_texture(rng.integers(0, 256, shape + (4,), dtype=np.uint8), srgb)
    pool = [tex((2, 2), False), tex((4, 4), True), tex((8, 8), False), tex((5, 3), True), tex((4, 4), False), tex((8, 8), True)]
    uniform = lambda rgba: s.add_texture(np.tile(np.array(rgba, np.uint8), (2, 2, 1)), False)
    a128 = rng.integers(0, 256, (2, 2, 4), dtype=np.uint8); a128[..., 3] = 128
    t_a128 = s.add_texture(a128, False)
    tie = np.zeros((2, 2, 4), np.uint8); tie[:, 0] = (127, 127, 200, 255); tie[:, 1] = (128, 128, 200, 255)
    t_tie = s.add_texture(tie, False)
    mats = []                                     # (name, material, mesh, queries per triangle)

    def add(name, m, mesh=full, per_tri=12):
        mats.append((name, m, mesh, per_tri))
        return m

    none = add("none", random_factors(rng))
    for k, slot in enumerate(SLOTS):                                                      # each slot bound alone, the factors of "none"
        m = add("only " + slot, copy_material(none))
        bind(m, slot, pool[k % len(pool)], [s.smp_wrap, s.smp_point, s.smp_mirror][k % 3], tex_coord=1 if k % 4 == 1 else 0,
             rotation=0.7 if k % 3 == 2 else 0.0, offset=(0.25, -0.375) if k % 2 else (0, 0), scale=(1.5, 0.75) if k % 5 == 0 else (1, 1))
    m = add("all", random_factors(rng))
    for k, slot in enumerate(SLOTS):
        bind(m, slot, pool[(k + 2) % len(pool)], [s.smp_mirror, s.smp_wrap, s.smp_point][k % 3], tex_coord=k % 2, rotation=0.1 * k)
    add("opaque", random_factors(rng))
    product = f32(0.75) * f32(128.0 / 255.0)                                              # factor x colour (none: 1) x texel, as both sides form it
    for name, cutoff in (("mask at the cutoff", product), ("mask one ulp above the cutoff", np.nextafter(product, f32(0))),
                         ("mask one ulp below the cutoff", np.nextafter(product, f32(1)))):
        m = add(name, random_factors(rng), plain, 4)
        m.base_color_factor[3] = 0.75; m.alpha_mode = abi.ALPHA_MODE_MASK; m.alpha_cutoff = float(cutoff)
        bind(m, "albedo", t_a128, s.smp_point)
    m = add("mask over vertex alpha", random_factors(rng)); m.alpha_mode = abi.ALPHA_MODE_MASK; m.alpha_cutoff = 0.12; bind(m, "albedo", pool[1], s.smp_wrap)
    m = add("blend", random_factors(rng)); m.alpha_mode = abi.ALPHA_MODE_BLEND; bind(m, "albedo", pool[2], s.smp_mirror, 1)
    for name, rgba in (("normal map (128, 128, 255)", (128, 128, 255, 255)), ("normal map (0, 0, 0)", (0, 0, 0, 255)), ("normal map (255, 255, 0)", (255, 255, 0, 255))):
        m = add(name, random_factors(rng)); bind(m, "normal", uniform(rgba), s.smp_wrap); bind(m, "clearcoat_normal", uniform(rgba), s.smp_point)
    m = add("normal_scale 0", random_factors(rng)); m.normal_scale = 0.0; bind(m, "normal", pool[0], s.smp_wrap)
    m = add("anisotropy texture cancels", random_factors(rng)); bind(m, "anisotropy", t_tie, s.smp_wrap)
    for name, rot, strength in (("anisotropy rotation 0", 0.0, 0.6), ("anisotropy rotation pi/2", math.pi / 2, 0.6), ("anisotropy strength 0", 1.0, 0.0),
                                ("anisotropy strength 1", -2.0, 1.0)):
        m = add(name, random_factors(rng)); m.anisotropy_rotation, m.anisotropy_strength = rot, strength
        if strength == 1.0: bind(m, "anisotropy", pool[4], s.smp_wrap)

    def trio(name, emissive=None, **other):
        """albedo, normal and metal-rough on one footprint (RM_TRIO); `other`: one slot's binding moved off it."""
        m = add(name, random_factors(rng))
        for slot, t in (("albedo", pool[1]), ("normal", pool[4]), ("metallic_roughness", pool[4])):
            bind(m, slot, t, s.smp_wrap, 0, 0.3, (0.1, 0.2), (1.0, 1.0))
        if emissive == "joins": bind(m, "emissive", pool[4], s.smp_wrap, 0, 0.3, (0.1, 0.2), (1.0, 1.0))
        if emissive == "apart": bind(m, "emissive", pool[4], s.smp_wrap, 0, 0.3, (0.3, 0.2), (1.0, 1.0))
        for slot, (t, smp, tcs, off) in other.items():
            bind(m, slot, t, smp, tcs, 0.3, off, (1.0, 1.0))
        return m
    trio("trio")
    trio("trio, emissive joins", "joins")
    trio("trio, emissive apart", "apart")
    trio("not a trio: size", normal=(pool[2], s.smp_wrap, 0, (0.1, 0.2)))
    trio("not a trio: sampler", metallic_roughness=(pool[4], s.smp_mirror, 0, (0.1, 0.2)))
    trio("not a trio: UV set", normal=(pool[4], s.smp_wrap, 1, (0.1, 0.2)))
    trio("not a trio: transform", metallic_roughness=(pool[4], s.smp_wrap, 0, (0.1, 0.25)))

    R = rotation(np.random.default_rng(5))
    rows, names, template = [], {}, {}
    for k, (name, m, mesh, per_tri) in enumerate(mats):
        inst = s.add_mesh(mesh, affine(R, (0.7 + 3.0 * (k % 8), 0.7 + 3.0 * (k // 8), 0.5)), s.add_material(m))
        names[name] = inst
        if per_tri not in template:                                                       # the same hits on every instance: twins differ by the material alone
            template[per_tri] = instance_queries(np.random.default_rng(77 + per_tri), s, inst, 8, per_tri, SPECIAL_BARY[:3] + [SPECIAL_BARY[5], SPECIAL_BARY[7]])
        rows += [(inst,) + r[1:] for r in template[per_tri]]
    return Case("material", s, to_queries(rows), flag_sets=FLAG_SETS, info=dict(names=names, mats={n: m for n, m, _, _ in mats}))


# ---------------------------------------------------------------- table limits
TABLE_SIZES = [(127, 95), (128, 96), (129, 96), (128, 97), (129, 97)]


@functools.lru_cache(None)
def table_case(n_inst, n_mat):
    """n_inst two-triangle instances over n_mat materials (the scene's default material included), on the pattern of test_gpu_tables.py's
    tables_scene: every row and every material is queried; every third material has slots 0..2 bound (material_slot012 reads those from the
    LDS copy or from memory), every seventh of those on one footprint."""
    rng = np.random.default_rng(1000 + 7 * n_inst + 13 * n_mat)
    s = new_scene("surface_tables_%d_%d" % (n_inst, n_mat))
    pool = [s.add_texture(rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), bool(k % 2)) for k in range(3)]
    for k in range(1, n_mat):
        m = random_factors(rng)
        if k % 3 == 0:
            for j, slot in enumerate(("normal", "albedo", "metallic_roughness")):
                bind(m, slot, pool[0] if k % 7 == 0 else pool[(k + j) % 3], s.smp_wrap, 0, 0.0, (0.1 * (j if k % 7 else 0), 0.0))
        s.add_material(m)
    quad = meshgen.grid(1, 1, (-1, -1, 0), (2, 0, 0), (0, 2, 0))
    quad.uv1 = quad.uv0 * 2.0
    rows = []
    for i in range(n_inst):
        T = affine(rotation(rng) @ np.diag(rng.uniform(0.5, 1.5, 3) * np.where(rng.random(3) < 0.25, -1.0, 1.0)), rng.uniform(-5, 5, 3))
        inst = s.add_mesh(quad, T, (n_mat - 1 - i) % n_mat)                               # the highest material ids on the lowest rows and the other way round
        rows += instance_queries(rng, s, inst, 2, 4, SPECIAL_BARY[:2])
    assert len(s.instances) == n_inst and len(s.materials) == n_mat
    return Case("tables %d/%d" % (n_inst, n_mat), s, to_queries(rows), flag_sets=(ADAPT,))


# ---------------------------------------------------------------- comparing
def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def differing(got, want):
    """Rows in which some float differs in its bits, NaN equal to NaN (payloads not compared)."""
    both_nan = np.isnan(got) & np.isnan(want)
    return np.nonzero(((bits(got) != bits(want)) & ~both_nan).any(1))[0]


def assert_same(got, want, what, q=None):
    bad = differing(got, want)
    if len(bad):
        k = bad[0]
        cols = np.nonzero((bits(got[k]) != bits(want[k])) & ~(np.isnan(got[k]) & np.isnan(want[k])))[0]
        where = "" if q is None else " (instance %d primitive %d front %d u %r v %r d %s)" % (q.inst[k], q.prim[k], q.front[k], q.u[k], q.v[k], q.d[k])
        raise AssertionError("%s: %d of %d queries differ, first query %d%s in columns %s: %s vs %s" % (
            what, len(bad), len(got), k, where, cols.tolist(), got[k, cols].tolist(), want[k, cols].tolist()))


def back_share(q):
    return float((q.front == 0).mean())


def non_finite_share(e):
    return float((~np.isfinite(e)).mean())


# ---------------------------------------------------------------- the GPU side
def hook(r, unit, small, flags, records):
    f = hooks.lib().pt_debug_surface_query
    rec = np.ascontiguousarray(records, f32)
    out = np.zeros((len(rec), OUT), f32)
    rc = f(r.h, unit, small, flags, rec.ctypes.data_as(C.c_void_p), len(rec), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, (rc, r.L.pt_last_error(r.h))
    return out


def packet_map(r, scene):
    """(instance, primitive) -> packet index from the TriPacket array, asserted to be a bijection onto the scene's triangles, with the
    ShadePacket's instance word equal to the TriPacket's (k_shade_packets de-indexes every index format the scene uses)."""
    info, _, _, tris, shade = accel_read(r)
    tw, sw = tris.view(u32).reshape(len(tris), 16), shade.view(u32).reshape(len(shade), 32)
    pairs = list(zip(tw[:, 3].tolist(), tw[:, 7].tolist()))
    want = {(i, p) for i, d in enumerate(scene.instances) for p in range(d.num_of_indices // 3)}
    assert len(pairs) == len(want) and set(pairs) == want, (len(pairs), len(want))
    assert np.array_equal(sw[:, 18], tw[:, 3])
    return {k: n for n, k in enumerate(pairs)}


class Gpu:
    """A case's scene on the device."""
    def __init__(self, R, case):
        self.case = case
        self.r = R()
        case.scene.upload(self.r)
        self.packet = packet_map(self.r, case.scene)
        self.small_ok = len(case.scene.instances) <= INST_MAX and len(case.scene.materials) <= MAT_MAX

    def run(self, q, flags, unit=0, small=0):
        return hook(self.r, unit, small, flags, q.records(self.packet))

    def check_a_b(self, oracle_lib, q=None, expected=None, flag_sets=None):
        """Checks A and B of a query set (default: the case's own) under each flag set; returns the unit-0 records of the last."""
        q = self.case.q if q is None else q
        for flags in (self.case.flag_sets if flag_sets is None else flag_sets):
            want = self.case.expected(oracle_lib, flags) if expected is None else expected[flags]
            what = "%s, flags %#x" % (self.case.name, flags)
            got = self.run(q, flags, 0, 0)
            assert_same(got, want, what + ": check A, unit 0 against the oracle", q)
            assert_same(self.run(q, flags, 1), got, what + ": check B, unit 1 against unit 0", q)
            if self.small_ok:
                assert_same(self.run(q, flags, 0, 1), got, what + ": check B, small_tables 1 against 0", q)
        return got

    def close(self):
        self.r.close()


@pytest.fixture(scope="module")
def R():
    from gltf_renderer_amd.renderer import Renderer
    return Renderer


@pytest.mark.gpu
def test_vertex_fetch_on_every_stream_combination_index_format_and_transform(R, oracle_lib):
    g = Gpu(R, vertex_case())
    try:
        g.check_a_b(oracle_lib)
    finally:
        g.close()


@pytest.mark.gpu
def test_degenerate_inputs_give_the_oracles_bits(R, oracle_lib):
    g = Gpu(R, degenerate_case())
    try:
        g.check_a_b(oracle_lib)
    finally:
        g.close()


@pytest.fixture(scope="module")
def material_gpu(R):
    g = Gpu(R, material_case())
    yield g
    g.close()


@pytest.mark.gpu
def test_materials_under_the_four_flag_sets(material_gpu, oracle_lib):
    """None bound, each slot alone, all bound, the alpha modes with the MASK tie, the normal-map and anisotropy edges, interleaved and
    general footprints; normal adaptation and geometric normals on and off, under random and grazing views."""
    g = material_gpu
    L = g.r.L
    assert (hooks.lib().pt_debug_interleaved_materials(g.r.h), hooks.lib().pt_debug_interleaved_emissive(g.r.h)) == TRIO_EXPECTED
    g.check_a_b(oracle_lib)


@pytest.mark.gpu
def test_any_hit_alpha_is_the_closest_hit_alpha(material_gpu):
    """candidate_alpha (its own fetch of colour, texcoords and albedo, from the whole packet and the instance row in memory) against
    get_surface for the same hit: alpha bit for bit on every query, base_alpha where the mode (BLEND) lets get_surface show it."""
    g = material_gpu
    got = g.run(g.case.q, ADAPT)
    nan = np.isnan(got[:, 27]) & np.isnan(got[:, 66])
    assert np.all((bits(got[:, 66]) == bits(got[:, 27])) | nan)
    blend = np.array([g.case.scene.materials[g.case.scene.instances[i].gpu.material_id].alpha_mode == abi.ALPHA_MODE_BLEND for i in g.case.q.inst.tolist()])
    assert blend.sum() >= 64 and np.all(bits(got[blend, 65]) == bits(got[blend, 27]))
    cut = np.array([g.case.scene.materials[g.case.scene.instances[i].gpu.material_id].alpha_cutoff for i in g.case.q.inst.tolist()], f32)
    assert np.array_equal(bits(got[:, 67]), bits(cut))


def albedo_edge(case, oracle_lib, name):
    """The queries of material `name`'s instance, and for each whether its albedo footprint needs the edge reload of texture_taps
    (pt_shading.h): the second column i1 lies off the texel pair loaded at ia = clamp(i0, 0, width - 2), as for i0 = width - 1 under WRAP.
    From the taps of the float64 sampler (which test_gpu_texture.py holds the product's taps to, exactly) at the oracle's texcoords."""
    from texture_ref import sample_level0, transform_rows
    rows = np.nonzero(case.q.inst == case.info["names"][name])[0]
    ts = case.info["mats"][name].albedo
    tc = case.expected(oracle_lib, 0)[rows, 20:24]
    data, srgb = case.scene.textures[ts.descriptor]
    au, av, _, magf = case.scene.samplers[ts.sampler - 1]
    _, taps, _ = sample_level0(data, srgb, (au, av, magf), transform_rows(ts.rotation, tuple(ts.offset), tuple(ts.scale)), tc[:, 2:4] if ts.tex_coord else tc[:, 0:2])
    ia = np.clip(taps[:, 0], 0, max(data.shape[1] - 2, 0))
    return rows, (taps[:, 1] != ia) & (taps[:, 1] != ia + 1)


EDGE_MATERIALS = {"interleaved": "trio, emissive joins", "general": "not a trio: size"}        # fetch_pbr_texels' edge vote, and tap_quad's


def wave_orders(oracle_lib):
    """(case, name, index array, label of every lane): orderings of a case's queries that put chosen kinds of hits side by side in a wave.
    test_wave_orders_hold_what_they_name asserts the labels, on the CPU."""
    case_vertex, case_material = vertex_case(), material_case()
    out = []
    kinds = case_vertex.info["kinds"]
    qi = case_vertex.q.inst
    of_kind = lambda name: np.nonzero(np.isin(qi, [i for i, k in kinds.items() if k[0] == name]))[0]
    stream_label = lambda index: np.array([kinds[i][0] for i in qi[index].tolist()])
    def alternate(a, b):
        n = min(len(a), len(b)) // 64 * 64
        z = np.empty(2 * n, np.int64); z[0::2], z[1::2] = a[:n], b[:n]
        return z
    def add(case, name, index, label):
        out.append((case, name, index, label(index)))
    add(case_vertex, "homogeneous waves", np.concatenate([np.nonzero(qi == i)[0][:128] for i in kinds]), stream_label)       # two whole waves an instance
    add(case_vertex, "with and without the extra streams, lane by lane", alternate(of_kind("+uv0"), of_kind("all")), stream_label)
    add(case_vertex, "one lane with the extra streams in a wave without", np.concatenate([of_kind("none")[:63], of_kind("+colour")[:1], of_kind("tangent space")[:64]]), stream_label)
    names, mq = case_material.info["names"], case_material.q
    name_of = {i: n for n, i in names.items()}
    of_mat = lambda name: np.nonzero(mq.inst == names[name])[0]
    add(case_material, "trio and general materials, lane by lane", alternate(np.concatenate([of_mat("trio"), of_mat("trio, emissive joins")]),
                                                                             np.concatenate([of_mat("not a trio: size"), of_mat("all")])),
        lambda index: np.array(["trio" if name_of[i].startswith("trio") else "general" for i in mq.inst[index].tolist()]))
    for path, material in EDGE_MATERIALS.items():
        rows, is_edge = albedo_edge(case_material, oracle_lib, material)
        edge_of = dict(zip(rows.tolist(), is_edge.tolist()))
        label = lambda index: np.array(["edge" if edge_of[k] else "interior" for k in index.tolist()])
        interior, edge = rows[~is_edge], rows[is_edge]
        add(case_material, "%s path: edge and interior footprints, lane by lane" % path, alternate(np.resize(interior, 64), np.resize(edge, 64)), label)
        add(case_material, "%s path: one edge footprint in a wave of interior ones" % path, np.concatenate([np.resize(interior, 40), edge[:1], np.resize(interior, 23)]), label)
    perm = np.random.default_rng(9).permutation(len(mq))
    none = lambda index: np.full(len(index), "")
    add(case_material, "shuffled", perm, none)
    add(case_material, "a one-query call", perm[:1], none)
    add(case_material, "n % 64 == 1", perm[:129], none)
    return out


@pytest.mark.gpu
def test_wave_composition_does_not_change_a_query(R, material_gpu, oracle_lib):
    """The voted fetches: whatever shares a wave with a query, its record is the oracle's."""
    gv = Gpu(R, vertex_case())
    try:
        for case, name, index, _ in wave_orders(oracle_lib):
            g = gv if case is vertex_case() else material_gpu
            assert len(index) > 0
            flags = ADAPT
            q = case.q.take(index)
            expected = {flags: case.expected(oracle_lib, flags)[index]}
            g.check_a_b(oracle_lib, q, expected, flag_sets=(flags,))
    finally:
        gv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", TABLE_SIZES, ids=lambda z: "%d-%d" % z)
def test_table_limits(R, oracle_lib, size):
    """Instance rows 127 / 128 / 129 and materials 95 / 96 / 97: the LDS copies, what lies past them, and small_tables where the scene fits."""
    g = Gpu(R, table_case(*size))
    try:
        assert g.small_ok == (size[0] <= INST_MAX and size[1] <= MAT_MAX)
        g.check_a_b(oracle_lib)
        if not g.small_ok:                                                                # the host refuses what the LDS copies cannot hold
            rec = g.case.q.take(np.arange(1)).records(g.packet); out = np.zeros((1, OUT), f32)
            assert hooks.lib().pt_debug_surface_query(g.r.h, 0, 1, 0, rec.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) == -1
    finally:
        g.close()


def hook_camera_rays(r, st, params, queries):
    q = np.ascontiguousarray(queries, u32).reshape(-1, 3)
    out = np.zeros((len(q), 8), f32)
    f = hooks.lib().pt_debug_camera_rays
    assert f(r.h, C.byref(st), C.byref(params), q.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def frame_scene():
    s = scenes.test_scene(32, 16, with_env=False)
    s.width, s.height = 32, 32
    return s


@pytest.mark.gpu
def test_the_hook_gives_what_the_production_kernels_write(R):
    """A 32 x 32 frame of the small textured scene: the hits of pt_debug_camera_rays + pt_debug_intersect through the hook against what
    the wavefront kernels write for the same frame -- the first-hit albedo and normal records of pt_set_aov and the COLOR debug output."""
    from ray_hook import gpu_intersect
    s = frame_scene()
    r = R()
    try:
        s.upload(r)
        st = abi.PtSettings.from_buffer_copy(bytes(s.settings)); st.flags &= ~abi.FLAG_ACCUMULATE
        st.use_frame_as_seed = 1
        frame = 3
        params = s.execute_params(frame)
        y, x = np.mgrid[0:32, 0:32]
        rays = hook_camera_rays(r, st, params, np.stack([x.ravel(), y.ravel(), np.full(1024, frame)], 1))
        hits = gpu_intersect(r, rays, 1 if st.flags & abi.FLAG_CULL_BACKFACE else 0, 0)
        hit = hits[:, 0] > 0
        assert 200 <= hit.sum() <= 1000, int(hit.sum())
        packet = packet_map(r, s)
        q = Queries(hits[hit, 4], hits[hit, 5], hits[hit, 6], hits[hit, 2], hits[hit, 3], rays[hit, 4:7])
        flags = st.flags & (ADAPT | GEOM)
        got = [hook(r, unit, small, flags, q.records(packet)) for unit, small in ((0, 0), (0, 1), (1, 0))]
        assert_same(got[1], got[0], "small_tables"); assert_same(got[2], got[0], "unit 1")
        out, alb, nd = (r.create_output(32, 32) for _ in range(3))
        r.set_aov(alb, nd)
        r.trace(st, params, out)
        alb_h, nd_h = r.readback(alb).reshape(-1, 4)[hit], r.readback(nd).reshape(-1, 4)[hit]
        assert_same(got[0][:, 24:27], alb_h[:, :3], "albedo against the AOV record")
        assert_same(got[0][:, 31:34], nd_h[:, :3], "shading normal against the AOV record")
        r.set_aov(None, None)
        sd = abi.PtSettings.from_buffer_copy(bytes(st)); sd.debug_output = abi.DEBUG_OUTPUT_COLOR
        r.trace(sd, params, out)
        assert_same(got[0][:, 24:27], r.readback(out).reshape(-1, 4)[hit][:, :3], "albedo against the COLOR debug output")
    finally:
        r.close()


@pytest.mark.gpu
def test_surface_hook_rejects_bad_arguments(R):
    """Argument errors come back as error codes; no query reaches the device."""
    g = Gpu(R, table_case(129, 97))
    try:
        f = hooks.lib().pt_debug_surface_query
        rec = g.case.q.take(np.arange(2)).records(g.packet)
        out = np.zeros((2, OUT), f32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        n_tris = len(g.packet)
        assert f(None, 0, 0, 0, p(rec), 2, p(out)) != 0
        assert f(g.r.h, 2, 0, 0, p(rec), 2, p(out)) != 0 and f(g.r.h, -1, 0, 0, p(rec), 2, p(out)) != 0
        assert f(g.r.h, 0, 0, 0, None, 2, p(out)) != 0 and f(g.r.h, 0, 0, 0, p(rec), 2, None) != 0
        assert f(g.r.h, 0, 1, 0, p(rec), 2, p(out)) != 0                                  # small_tables with 129 instances and 97 materials
        for word, value in ((0, n_tris), (0, 0xffffffff), (1, 2)):
            bad = rec.copy(); bad.view(u32)[1, word] = value
            for unit in (0, 1):
                assert f(g.r.h, unit, 0, 0, p(bad), 2, p(out)) != 0, (word, value, unit)
        assert not out.any()
        assert f(g.r.h, 0, 0, 0, None, 0, None) == 0                                      # no queries: nothing to do
        assert f(g.r.h, 1, 1, 0, p(rec), 2, p(out)) == 0 and out.any()                    # unit 1 does not look at small_tables
    finally:
        g.close()


# ---------------------------------------------------------------- CPU only: the sets on the oracle alone
ALL_CASES = [vertex_case, degenerate_case, material_case] + [functools.partial(table_case, *z) for z in TABLE_SIZES]


def test_every_set_has_its_back_faces_and_finite_outputs(oracle_lib):
    for make in ALL_CASES:
        case = make()
        assert len(case.q) >= 512 and back_share(case.q) >= MIN_BACK_SHARE, (case.name, len(case.q), back_share(case.q))
        for flags in case.flag_sets:
            e = case.expected(oracle_lib, flags)
            share = non_finite_share(e)
            print("%s, flags %#x: %d queries, %.1f %% back faces, %.4f %% non-finite floats" % (case.name, flags, len(case.q), 100 * back_share(case.q), 100 * share))
            if case.name != "degenerate":
                assert share <= MAX_NON_FINITE, (case.name, flags, share)


def test_the_vertex_set_reaches_every_combination(oracle_lib):
    case = vertex_case()
    kinds = case.info["kinds"]
    assert {k[0] for k in kinds.values()} == set(STREAMS) and {k[2] for k in kinds.values()} == {None, 16, 32}
    assert {k[1] for k in kinds.values()} >= set(TRANSFORMS)
    for sname in STREAMS:
        assert {k[2] for k in kinds.values() if k[0] == sname} == {None, 16, 32} or len(TRANSFORMS) < 3, sname
    e = case.expected(oracle_lib, 0)
    q = case.q
    for inst, (sname, tname, _) in kinds.items():
        rows = e[q.inst == inst]
        has_ts, has_uv0, has_uv1, has_col = STREAMS[sname]
        assert (rows[:, 20:22] != 0).any() == bool(has_uv0) and (rows[:, 22:24] != 0).any() == bool(has_uv1), (sname, tname)
        assert (rows[:, 16:20] != 1).any() == bool(has_col), (sname, tname)
        assert set(np.unique(rows[:, 12])) == ({-1.0, 1.0}), (sname, tname)               # the winding, flipped on the back faces
    # the special barycentrics are there: a vertex, an edge, u + v == 1, the ulps
    for u, v in SPECIAL_BARY:
        assert ((q.u == f32(u)) & (q.v == f32(v))).sum() >= len(kinds) * 8
    mirrored = [i for i, k in kinds.items() if k[1] == "mirrored"]
    assert all(np.linalg.det(np.array(case.scene.instances[i].gpu.transform[:]).reshape(4, 4)[:3, :3]) < 0 for i in mirrored)


def test_the_degenerate_kinds_produce_their_nans(oracle_lib):
    case = degenerate_case()
    e = case.expected(oracle_lib, 0)
    kinds = case.info["kinds"]
    count = {}
    for inst, kind in kinds.items():
        count[kind] = count.get(kind, 0) + int(np.isnan(e[case.q.inst == inst]).any(1).sum())
    print("degenerate set: %d queries, queries with a NaN by kind: %s" % (len(case.q), count))
    assert np.isnan(e).any()
    for kind in DEGENERATE_MUST_NAN:
        assert count[kind] > 0, (kind, count)
    assert set(kinds.values()) >= set(DEGENERATE_MUST_NAN) | {"tangent-space word 0x0", "tangent-space word 0xffffffff", "cancelling normals"}
    # The other three kinds give finite records; what makes each of them an edge is asserted on the decoded words instead.
    import skin_ref
    q = case.q
    for inst, kind in kinds.items():
        g = case.scene.instances[inst].gpu
        rows = q.inst == inst
        if kind.startswith("tangent-space word"):
            # all-zero and all-one fields: a corner of the octahedral square (the normal folds onto -z), the first / last tangent angle, and
            # the two windings -- the record is finite and carries that winding, negated on the back faces
            word = np.unique(case.scene.buffers[g.tangent_space_descriptor][0])
            assert len(word) == 1 and int(word[0]) in (0, 0xffffffff)
            n, _, winding = skin_ref.decode(oracle_lib, word)
            assert np.array_equal(n[0], f32([0, 0, -1])) and winding[0] == (-1 if word[0] == 0 else 1)
            assert np.isfinite(e[rows]).all()
            assert np.array_equal(e[rows][:, 12] * np.where(q.front[rows] == 1, 1, -1), np.full(rows.sum(), winding[0]))
        if kind == "cancelling normals":
            # the decoded normals of vertices 0 and 1 of triangle 0 nearly cancel at (0.5, 0): what is normalised there is far shorter than the
            # 1e-2 of its inputs' scale that surface_ref calls well-conditioned, and its predicate says so
            words = case.scene.buffers[g.tangent_space_descriptor][0][case.scene.buffers[g.index_descriptor][0][:2]]
            n, _, _ = skin_ref.decode(oracle_lib, words.astype(u32))
            assert np.linalg.norm(0.5 * n[0].astype(np.float64) + 0.5 * n[1].astype(np.float64)) < 1e-3
            mid = np.nonzero(rows & (q.prim == 0) & (q.u == f32(0.5)) & (q.v == 0))[0]
            assert len(mid) >= 1
            _, ok, _ = surface_ref.surface(case.scene, oracle_lib, 0, q.inst[mid], q.prim[mid], q.front[mid], q.u[mid], q.v[mid], q.d[mid])
            assert not ok.any()


def test_the_material_set_takes_every_branch(oracle_lib):
    case = material_case()
    names, q = case.info["names"], case.q
    plain, adapted = case.expected(oracle_lib, 0), case.expected(oracle_lib, ADAPT)
    rows = lambda name: q.inst == names[name]
    # normal adaptation: the shading normal changes where the branch is taken
    taken = (bits(plain[:, 31:34]) != bits(adapted[:, 31:34])).any(1)
    print("material set: %d queries; normal adaptation taken in %d, not taken in %d" % (len(q), taken.sum(), (~taken).sum()))
    assert taken.sum() >= MIN_ADAPTED and (~taken).sum() >= MIN_ADAPTED
    geometric = case.expected(oracle_lib, GEOM)
    assert np.array_equal(bits(geometric[:, 31:34]), bits(geometric[:, 3:6])) and np.array_equal(bits(geometric[:, 47:50]), bits(geometric[:, 3:6]))
    assert (bits(plain[:, 31:34]) != bits(plain[:, 3:6])).any(1).mean() > 0.9
    # MASK: both sides and the exact tie
    at, above, below = (plain[rows("mask " + k)] for k in ("at the cutoff", "one ulp above the cutoff", "one ulp below the cutoff"))
    assert np.all(bits(at[:, 65]) == bits(at[:, 67])) and np.all(at[:, 27] == 1) and np.all(at[:, 66] == 1)          # a tie is not below the cutoff
    assert np.all(above[:, 65] > above[:, 67]) and np.all(above[:, 27] == 1)
    assert np.all(below[:, 65] < below[:, 67]) and np.all(below[:, 27] == 0) and np.all(below[:, 66] == 0)
    assert np.all(np.abs(above[:, 65].astype(np.float64) - above[:, 67]) < 1e-7) and np.all(np.abs(below[:, 65].astype(np.float64) - below[:, 67]) < 1e-7)
    mixed = plain[rows("mask over vertex alpha")]
    print("MASK over vertex alpha: %d below the cutoff, %d not; ties %d" % ((mixed[:, 27] == 0).sum(), (mixed[:, 27] == 1).sum(), len(at)))
    assert (mixed[:, 27] == 0).sum() >= 10 and (mixed[:, 27] == 1).sum() >= 10
    blend = plain[rows("blend")]
    assert np.array_equal(bits(blend[:, 27]), bits(blend[:, 65])) and len(np.unique(blend[:, 27])) > 10
    # every slot bound alone changes the record of its unbound twin (the same hits on the same mesh)
    base = plain[rows("none")]
    for slot in SLOTS:
        twin = plain[rows("only " + slot)]
        changed = (bits(twin[:, 24:58]) != bits(base[:, 24:58])).any(1)                  # the Surface and the emissive value; not the offset origins (the twins
        if slot in ("occlusion", "thickness"):                                            # stand in different places) and not the tap count
            assert not changed.any(), slot                                                # dead fetches: a tap and nothing else
        else:
            assert changed.all(), (slot, int(changed.sum()))
        assert np.all(twin[:, 64] == (2 if slot == "emissive" else 1)) and np.all(base[:, 64] == 0), slot          # the tap counts, the dead fetches included
    assert np.all(plain[rows("all")][:, 64] == 16)
    # the anisotropy texture that cancels: av.xy == (0, 0) exactly at vertex 0 of triangle 0, and normalize(0) follows
    tie = rows("anisotropy texture cancels") & (q.prim == 0) & (q.u == 0) & (q.v == 0)
    assert tie.sum() >= 1 and np.isnan(plain[tie][:, 34:40]).all()
    assert np.all(plain[rows("anisotropy strength 0")][:, 29] == plain[rows("anisotropy strength 0")][:, 30])
    s1 = plain[rows("anisotropy strength 1")]
    assert (s1[:, 29] > s1[:, 30]).mean() > 0.9
    # interleaved and general footprints: by construction (counted on the device in test_materials_under_the_four_flag_sets)
    mats = case.info["mats"]
    same_footprint = lambda m, a, b: bytes(getattr(m, a))[4:] == bytes(getattr(m, b))[4:] and case.scene.textures[getattr(m, a).descriptor][0].shape == case.scene.textures[getattr(m, b).descriptor][0].shape
    trio = [n for n, m in mats.items() if all(getattr(m, k).descriptor != -1 for k in ("albedo", "normal", "metallic_roughness")) and
            same_footprint(m, "albedo", "normal") and same_footprint(m, "albedo", "metallic_roughness")]
    assert len(trio) == TRIO_EXPECTED[0] and sum(1 for n in trio if mats[n].emissive.descriptor != -1 and same_footprint(mats[n], "albedo", "emissive")) == TRIO_EXPECTED[1], trio
    assert sum(1 for n in mats if n.startswith("not a trio")) == 4
    # the emissive value is there and depends on its texture
    assert (plain[rows("trio, emissive joins")][:, 55:58] != plain[rows("trio")][:, 55:58]).any()


def test_wave_orders_hold_what_they_name(oracle_lib):
    """The orderings of test_wave_composition_does_not_change_a_query put in a wave what their names say: lane by lane, from the labels."""
    orders = {name: (index, label) for _, name, index, label in wave_orders(oracle_lib)}
    index, label = orders["homogeneous waves"]
    assert all(len(set(label[k:k + 64])) == 1 for k in range(0, len(label), 64)) and len(set(label)) == len(STREAMS)
    index, label = orders["with and without the extra streams, lane by lane"]
    assert len(label) >= 128 and set(label[0::2]) == {"+uv0"} and set(label[1::2]) == {"all"}
    index, label = orders["one lane with the extra streams in a wave without"]
    assert set(label[:63]) == {"none"} and label[63] == "+colour" and set(label[64:]) == {"tangent space"}
    index, label = orders["trio and general materials, lane by lane"]
    assert len(label) >= 128 and set(label[0::2]) == {"trio"} and set(label[1::2]) == {"general"}
    for path, material in EDGE_MATERIALS.items():
        rows, is_edge = albedo_edge(material_case(), oracle_lib, material)
        print("%s path (%s): %d of %d queries have an edge footprint" % (path, material, is_edge.sum(), len(rows)))
        assert is_edge.sum() >= 8 and (~is_edge).sum() >= 8
        index, label = orders["%s path: edge and interior footprints, lane by lane" % path]
        assert len(label) == 128 and set(label[0::2]) == {"interior"} and set(label[1::2]) == {"edge"}
        assert len(set(index[1::2].tolist())) >= 8                                          # several different edge hits, not one repeated
        index, label = orders["%s path: one edge footprint in a wave of interior ones" % path]
        assert len(label) == 64 and label[40] == "edge" and set(np.delete(label, 40)) == {"interior"}
    assert len(orders["a one-query call"][0]) == 1 and len(orders["n % 64 == 1"][0]) % 64 == 1
    mats = material_case().info["mats"]
    same = lambda a, b: bytes(a)[4:] == bytes(b)[4:]
    t, g = mats[EDGE_MATERIALS["interleaved"]], mats[EDGE_MATERIALS["general"]]
    assert same(t.albedo, t.normal) and same(t.albedo, t.metallic_roughness) and same(g.albedo, g.normal)
    assert material_case().scene.textures[g.normal.descriptor][0].shape != material_case().scene.textures[g.albedo.descriptor][0].shape   # what keeps it off the interleaved path


def test_table_sets_query_every_row_and_material(oracle_lib):
    for size in TABLE_SIZES:
        case = table_case(*size)
        assert set(case.q.inst.tolist()) == set(range(size[0]))
        assert {d.gpu.material_id for d in case.scene.instances} == set(range(size[1]))


def c_errors(case, oracle_lib, flags):
    """Per output group: the oracle's largest deviation from surface_ref over the well-conditioned queries; and the share left out."""
    q = case.q
    ref, ok, _ = surface_ref.surface(case.scene, oracle_lib, flags, q.inst, q.prim, q.front, q.u, q.v, q.d)
    e = case.expected(oracle_lib, flags).astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(e - ref) / np.maximum(1.0, np.abs(ref))
    err[np.isnan(e) & np.isnan(ref)] = 0
    worst = {}
    for name, cols in surface_ref.GROUPS.items():
        sub = err[ok][:, cols]
        worst[name] = (float(np.nan_to_num(sub, nan=np.inf).max()), int(np.argmax(np.nan_to_num(sub, nan=np.inf).max(1))))
    return worst, 1.0 - float(ok.mean()), np.nonzero(ok)[0]


@pytest.mark.parametrize("which", ["vertex", "material"])
def test_check_c_the_oracle_against_the_float64_restatement(oracle_lib, which):
    """Check C.  A wrong operation -- tangent and bitangent swapped, a missing winding, the wrong UV set, sRGB on a linear slot -- moves a unit
    vector or a scalar by 1e-2 or more; the bounds stay below 1e-4 there."""
    assert C_BOUND["unit vectors"] < 1e-4 and C_BOUND["colours and scalars"] < 1e-4
    case = vertex_case() if which == "vertex" else material_case()
    for flags in (FLAG_SETS if which == "material" else (0,)):
        worst, left_out, kept = c_errors(case, oracle_lib, flags)
        print("check C, %s set, flags %#x: %d of %d queries kept (%.1f %% left out); largest deviation %s" % (
            which, flags, len(kept), len(case.q), 100 * left_out, {k: "%.2e" % v[0] for k, v in worst.items()}))
        assert left_out <= MAX_ILL_CONDITIONED, (which, flags, left_out)
        for name, (value, row) in worst.items():
            k = kept[row]
            assert value <= C_BOUND[name], (which, flags, name, value, C_BOUND[name], "query %d: instance %d primitive %d" % (k, case.q.inst[k], case.q.prim[k]))


DEBUG_COLUMNS = [            # (debug output, columns of the record, encoding: None as it is, "unit" (x + 1) / 2, "sqrt", "flip" pre-flip value)
    (abi.DEBUG_OUTPUT_VERTEX_COLOR, [16, 17, 18], None), (abi.DEBUG_OUTPUT_VERTEX_ALPHA, [19, 19, 19], None),
    (abi.DEBUG_OUTPUT_VERTEX_NORMAL, [6, 7, 8], "flip"), (abi.DEBUG_OUTPUT_VERTEX_TANGENT, [9, 10, 11], "flip"), (abi.DEBUG_OUTPUT_VERTEX_BITANGENT, [13, 14, 15], "unit"),
    (abi.DEBUG_OUTPUT_TEXCOORD_0, [20, 21], None), (abi.DEBUG_OUTPUT_TEXCOORD_1, [22, 23], None),
    (abi.DEBUG_OUTPUT_COLOR, [24, 25, 26], None), (abi.DEBUG_OUTPUT_ALPHA, [27, 27, 27], None), (abi.DEBUG_OUTPUT_SHADING_NORMAL, [31, 32, 33], "unit"),
    (abi.DEBUG_OUTPUT_SHADING_TANGENT, [34, 35, 36], "unit"), (abi.DEBUG_OUTPUT_SHADING_BITANGENT, [37, 38, 39], "unit"),
    (abi.DEBUG_OUTPUT_METALNESS, [28, 28, 28], None), (abi.DEBUG_OUTPUT_ROUGHNESS, [30, 30, 30], "sqrt"), (abi.DEBUG_OUTPUT_SPECULAR, [44, 44, 44], None),
    (abi.DEBUG_OUTPUT_SPECULAR_COLOR, [41, 42, 43], None), (abi.DEBUG_OUTPUT_CLEARCOAT, [45, 45, 45], None), (abi.DEBUG_OUTPUT_CLEARCOAT_ROUGHNESS, [46, 46, 46], None),
    (abi.DEBUG_OUTPUT_CLEARCOAT_NORMAL, [47, 48, 49], "unit"), (abi.DEBUG_OUTPUT_TRANSMISSIVE, [54, 54, 54], None)]


def test_the_export_gives_what_pathtrace_scene_shows(oracle_lib):
    """orc_surface_query_many against pathtrace_scene itself on a 32 x 32 frame: the primary ray of every pixel from the ray log, its hit
    from orc_intersect, and the record of that hit against the twenty first-vertex debug outputs of the traced frame, bit for bit."""
    s = frame_scene()
    o = oracle_lib.Oracle()
    h = s.upload(o)
    st = abi.PtSettings.from_buffer_copy(bytes(s.settings)); st.flags &= ~abi.FLAG_ACCUMULATE
    params = s.execute_params(0)
    frames = {}
    for dbg, _, _ in DEBUG_COLUMNS + [(abi.DEBUG_OUTPUT_HIT_KIND, None, None)]:
        sd = abi.PtSettings.from_buffer_copy(bytes(st)); sd.debug_output = dbg
        b = np.zeros((32, 32, 4), f32)
        o.trace(sd, params, b, nthreads=4)
        frames[dbg] = b.reshape(-1, 4)
    sd = abi.PtSettings.from_buffer_copy(bytes(st)); sd.debug_output = abi.DEBUG_OUTPUT_COLOR
    pixels, rows = [], []
    scratch = np.zeros((32, 32, 4), f32)
    for py in range(0, 32):
        for px in range(0, 32):
            o.set_window(px, py, px + 1, py + 1); o.ray_log(px, py)
            o.trace(sd, params, scratch, nthreads=1)
            log = o.read_ray_log()
            assert len(log) == 1 and log[0, 8] == 0
            if log[0, 9] == 0: continue
            hit = o.intersect(log[0, 0:3], log[0, 4:7], float(log[0, 3]), float(log[0, 7]), 0x10 if st.flags & abi.FLAG_CULL_BACKFACE else 0)
            assert hit[0] == 1 and hit[4] == log[0, 11] and hit[5] == log[0, 12] and hit[1] == log[0, 10]
            pixels.append(py * 32 + px)
            rows.append((int(hit[4]), int(hit[5]), int(hit[6]), hit[2], hit[3], log[0, 4:7].copy()))
    o.set_window(); o.ray_log(-1, -1)
    assert len(rows) >= 200, len(rows)
    q = to_queries(rows)
    e = o.surface_query_many(st.flags, q.records(), q.inst, q.prim)
    front = q.front == 1
    assert np.array_equal(frames[abi.DEBUG_OUTPUT_HIT_KIND][pixels][:, 0] == 1, front)
    for dbg, cols, enc in DEBUG_COLUMNS:
        got = e[:, cols]
        if enc == "flip": got = np.where(front[:, None], got, -got)                       # the VERTEX_* outputs come before the flip
        if enc in ("unit", "flip"): got = (got + f32(1)) / f32(2)
        if enc == "sqrt": got = np.sqrt(got)
        want = frames[dbg][pixels][:, :len(cols)]
        assert_same(np.ascontiguousarray(got, f32), np.ascontiguousarray(want), "debug output %d" % dbg, q)
    o.close()
