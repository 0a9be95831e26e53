"""A host model of what include/mipt.h promises about scene edits and the acceleration structure (the comment above pt_build_accel, and the
snapshot rule above pt_motion_snapshot), a generator of random edit sequences, and the driver that plays a sequence into a backend (the product's
Renderer or the oracle).  CPU only: numpy, the plain-data layouts of gltf_renderer_amd.abi and, for the skinned row's expected vertices, the
oracle's GpuSkin::Run (k_skin with use_mfma = 0 gives the oracle's bits, tests/test_gpu_skin.py).  It restates the HEADER, not csrc/mipt_api.hip:

  after upload                  pending = rebuild
  set_instances(T), refused     nothing changes
  set_instances(T)              row count or a row's triangle count differs from the current table, or no full build yet -> pending = rebuild;
                                all rows identical -> nothing changes; rows that differ only in material_id leave the tree alone; any other
                                differing row is touched and pending = max(pending, refit)
  buffer_update(b), skin -> b   the rows of the current table that read b through any of the six streams are touched, pending = max(pending,
                                refit); no such row -> nothing changes
  request_rebuild               pending = rebuild
  set_accel_builder(other)      pending = rebuild; the builder in force -> nothing changes
  a realisation                 rebuild: accel_builds + 1, the touched set is cleared; refit: accel_refits + 1; clean: neither
  a snapshot                    VALID iff the current table has the row count and the per-row triangle counts of the last take, else STALE; NONE
                                before any take

The starting scene (start_scene): 7 rows, 578 triangles (three 256-lane blocks, a 1024-leaf segment tree: one pass more than the 256-leaf minimum,
a wide tree of several levels), every position within +-10, four materials:
  0  non-indexed soup, 90 triangles                     4  the same mesh again, mirrored (the two rows share every stream)
  1  16-bit indexed soup, 100, rotated, uneven scale    5  grid with UV0, UV1, colours and tangents, textured normal-mapped MASK material, 72
  2  32-bit indexed soup, 100                           6  one skinned limb of the figure (a cut of scenes.add_skinned_figure), 96: its position
  3  UV sphere, 60                                         and tangent-space streams are the outputs of pt_skin_run (scenes.SkinBinding)
Beside them live buffers no row reads at the start: a second position stream for row 1 and a second UV0 stream for row 5 (edit h re-points at
them), a 16-bit index stream for row 0 (edit i) and one idle buffer (edit n).

An edit is a short tuple, (kind, parameters...), whose bulk data (new vertices, a permutation) comes from a seed inside it: a sequence prints in
a line and replays anywhere.  sequence(seed, steps) -> [Step]: 0-4 edits, then one realisation.  The kinds:
  a resend the table        e rewrite a position stream          i row 0 indexed <-> non-indexed      m a refused call
  b move rows (also         f permute an index stream            j drop / add a row, change a count   n update a buffer no row reads
    mirror, there and back) g rewrite uv0 / uv1 / colour /       k request_rebuild                    o pt_skin_run
  c material_id only          tangent stream                     l set_accel_builder (same / other)
  d mask / flags only       h re-point a stream at its twin"""
import copy
import types
from collections import namedtuple

import numpy as np

from gltf_renderer_amd import abi, camera, meshgen, scenes

f32, u32 = np.float32, np.uint32
CLEAN, REFIT, REBUILD = 0, 1, 2
PREDICTIONS = ("nothing", "refit", "build")
REALISATIONS = ("build_accel", "trace", "focus_at", "motion_snapshot", "debug_intersect", "accel_read")
KINDS = "abcdefghijklmno"
BUILDERS = (abi.BUILDER_LBVH, abi.BUILDER_PLOC, abi.BUILDER_PLOC_REINSERT)
ERR_BAD_HANDLE = -4                                              # include/mipt.h PT_ERR_BAD_HANDLE
DEAD, OUT_OF_RANGE = -2, 1_000_000                               # scene-local stand-ins: a destroyed buffer's handle, a handle no context has
STREAM_FIELDS = ("index", "position", "tangent", "uv0", "uv1", "color")
POSE_TIMES = (0.1, 0.35, 0.6, 0.85, 1.1, 1.6)                    # seconds of the walk cycle (edit o); the first is the starting pose
MAX_ROWS, MIN_ROWS = 9, 5
WIDTH, HEIGHT = 40, 24
RAY_EYE = (0.0, 0.0, 0.8)                                        # where make_rays' camera rays start: between the rows

Step = namedtuple("Step", "edits realise predict tags")


# ---- the instance row, field by name -------------------------------------------------------------------------------------------------------
def get_stream(d, name):
    g = d.gpu
    return {"index": g.index_descriptor, "position": g.position_descriptor, "tangent": g.tangent_space_descriptor, "uv0": g.texcoord_descriptors[0],
            "uv1": g.texcoord_descriptors[1], "color": g.color_descriptor}[name]


def set_stream(d, name, value):
    g = d.gpu
    if name == "uv0": g.texcoord_descriptors[0] = value
    elif name == "uv1": g.texcoord_descriptors[1] = value
    else: setattr(g, {"index": "index_descriptor", "position": "position_descriptor", "tangent": "tangent_space_descriptor", "color": "color_descriptor"}[name], value)


def clone(table):
    return [abi.PtInstanceDesc.from_buffer_copy(bytes(d)) for d in table]


def set_transform(d, T):
    d.gpu.transform[:] = camera.cm(T); d.gpu.normal_transform[:] = camera.cm(camera.inverse_transpose(T))


def row_key(d, with_material=True):
    """What of a row the tree and the packets depend on (plus the material id)."""
    g = abi.PtMeshInstance.from_buffer_copy(bytes(d.gpu))
    if not with_material: g.material_id = 0
    return bytes(g), d.instance_mask, d.instance_flags, d.num_of_indices


# ---- the starting scene ------------------------------------------------------------------------------------------------------------------
def _soup(n, seed, centre, spread=1.3, size=0.45):
    rng = np.random.default_rng(seed)
    return (np.asarray(centre) + rng.uniform(-spread, spread, (n, 1, 3)) + rng.normal(0, size, (n, 3, 3)) * rng.uniform(0.3, 1.2, (n, 1, 1))).astype(f32)


def _indexed(tris, seed):
    pos = tris.reshape(-1, 3)
    perm = np.random.default_rng(seed).permutation(len(pos))
    back = np.empty(len(pos), np.int64); back[perm] = np.arange(len(pos))
    return meshgen.Mesh(pos[perm], back)


def _limb():
    """The figure's left thigh (scenes.add_skinned_figure's bone 11 -> 12) as a mesh of its own, with that figure's joints and weights."""
    a, b, r = 11, 12, 0.075
    m, tf = meshgen.capsule_tube(scenes.JOINT_REST[a], scenes.JOINT_REST[b], r, nseg=8, nring=3)
    pa = scenes.JOINT_PARENT[a]
    m.joints = np.tile(np.array([a, b, pa, 0], dtype=np.uint16), (m.num_vertices, 1))
    w = np.stack([(1 - tf) * 0.85, tf * 0.85 + 0.05, np.full_like(tf, 0.10), np.zeros_like(tf)], axis=1)
    m.weights = w / w.sum(axis=1, keepdims=True)
    return m


_SKIN_CACHE = {}


def skinned(t):
    """(positions [vertices, 3] float32, packed tangent spaces [vertices] uint32) of the limb at walk-cycle time t: GpuSkin::Run on the oracle."""
    if t not in _SKIN_CACHE:
        from oracle import pyoracle
        s = scenes.SceneData("limb")
        _add_limb(s, None)
        o = pyoracle.Oracle(); h = s.upload(o)
        b = scenes.SkinBinding(o, s, h, 0, use_mfma=0); b.pose(t)
        nv = s.skins[0]["mesh"].num_vertices
        _SKIN_CACHE[t] = (o.buffer_read(b.out_position, f32, nv * 3).reshape(-1, 3).copy(), o.buffer_read(b.out_tangent_space, u32, nv).copy())
        o.close()
    return _SKIN_CACHE[t]


def _add_limb(s, T, material=0):
    m = _limb()
    inst = s.add_mesh(m, T, material, dynamic=True)
    d = s.instances[inst]
    jw = s.add_buffer(meshgen.pack_joint_weight(m.joints, m.weights), abi.FORMAT_JOINT_WEIGHT)
    s.skins.append({"instance": inst, "mesh": m, "joint_weight": jw, "inverse_bind": [np.linalg.inv(camera.translate(scenes.JOINT_REST[j])) for j in range(19)],
                    "input_position": d.gpu.position_descriptor, "input_tangent_space": d.gpu.tangent_space_descriptor})
    return inst


_TEMPLATE = []


def start_scene():
    """A copy of the starting scene that a Model may edit: the tables are its own, the arrays are shared with every other copy and are never
    written in place (a rewritten buffer is a new array)."""
    if not _TEMPLATE: _TEMPLATE.append(_make_start_scene())
    t = _TEMPLATE[0]
    s = copy.copy(t)
    s.buffers, s.instances, s.materials, s.home_T = list(t.buffers), clone(t.instances), list(t.materials), list(t.home_T)
    return s


def _make_start_scene():
    """The scene every sequence starts from, as a scenes.SceneData whose LAST TWO buffers are the skinned row's output streams (row 6 reads them).
    s.twin: {buffer: the same-sized buffer edit h swaps it with}; s.index0: the index stream edit i gives row 0; s.idle: the buffer nobody reads;
    s.home: {buffer: its starting contents}; s.home_T: the rows' starting transforms."""
    rng = np.random.default_rng(11)
    s = scenes.SceneData("scene_edits")
    TS = abi.PtTextureSample
    tex = 16
    h = scenes.value_noise(rng, tex, 3, 2)
    checker = ((np.indices((tex, tex)).sum(axis=0) // 2) % 2).astype(f32)
    t_mask = s.add_texture(scenes.rgba(0.2 + 0.6 * h, 0.8 * np.ones_like(h), 0.3 + 0.5 * checker, np.maximum(checker, (h > 0.45).astype(f32))), True)
    t_nrm = s.add_texture(scenes.normal_map_from_height(h, 2.0), False)
    m_two = s.add_material(scenes.material(flags=abi.MATERIAL_FLAG_DOUBLE_SIDED, base_color_factor=(0.8, 0.5, 0.2, 1), metalness_factor=0.0, roughness_factor=0.7))
    m_mask = s.add_material(scenes.material(alpha_mode=abi.ALPHA_MODE_MASK, alpha_cutoff=0.5, albedo=TS(t_mask), normal=TS(t_nrm, 0, 0, 0.2, (0.1, 0.05), (2.0, 1.5)),
                                            normal_scale=0.8, metalness_factor=0.0, roughness_factor=0.6))
    m_metal = s.add_material(scenes.material(base_color_factor=(0.9, 0.85, 0.6, 1), metalness_factor=1.0, roughness_factor=0.3))
    T = [None,
         camera.trs((2.2, 1.8, 1.0), (0.0, 0.0, np.sin(0.35), np.cos(0.35)), (1.4, 0.75, 1.2)),
         camera.trs((-0.3, -2.6, 0.2)),
         camera.trs((2.4, -1.6, 1.0)),
         camera.trs((0.4, -0.4, 2.2), scale=(-1.3, 1.0, 0.8)),
         camera.trs((-1.0, 2.6, 0.0)),
         camera.trs((-2.9, 0.6, -2.6), scale=(3.5, 3.5, 3.5))]
    s.add_mesh(meshgen.Mesh(_soup(90, 1, (-2.4, -1.2, 1.0)).reshape(-1, 3), None), T[0], 0)
    s.add_mesh(_indexed(_soup(100, 2, (0, 0, 0)), 2), T[1], m_two)
    s.add_mesh(_indexed(_soup(100, 3, (0, 0, 1.0)), 3), T[2], m_metal)
    b = s.instances[2].gpu.index_descriptor
    s.buffers[b] = (s.buffers[b][0].astype(np.uint32), abi.FORMAT_R32_UINT)
    sphere = meshgen.uv_sphere(6, 5, 0.9)
    s.add_mesh(sphere, T[3], 0)
    d = abi.PtInstanceDesc.from_buffer_copy(bytes(s.instances[3]))
    set_transform(d, T[4]); d.gpu.material_id = m_metal
    s.instances.append(d); s.mesh_records.append((sphere, np.asarray(T[4], np.float64), m_metal)); s.triangles += d.num_of_indices // 3
    full = meshgen.grid(6, 6, (0, 0, 0.2), (2.4, 0, 0.3), (0, 0.4, 2.2))
    full.uv1 = (full.uv0 * 3.0 + 0.25).astype(f32)
    full.colors = np.concatenate([np.random.default_rng(5).random((full.num_vertices, 3)), np.ones((full.num_vertices, 1))], axis=1)
    s.add_mesh(full, T[5], m_mask)
    _add_limb(s, T[6], 0)
    s.home_T = [np.eye(4) if t is None else np.asarray(t, np.float64) for t in T]
    # the buffers no row reads yet
    g1, g5 = s.instances[1].gpu, s.instances[5].gpu
    pos1 = s.buffers[g1.position_descriptor][0]
    alt_pos = s.add_buffer((pos1 + np.random.default_rng(21).normal(0, 0.15, pos1.shape)).astype(f32), abi.FORMAT_R32G32B32_FLOAT)
    alt_uv = s.add_buffer((s.buffers[g5.texcoord_descriptors[0]][0] * f32(1.5) + f32(0.125)).astype(f32), abi.FORMAT_R32G32_FLOAT)
    s.twin = {g1.position_descriptor: alt_pos, alt_pos: g1.position_descriptor, g5.texcoord_descriptors[0]: alt_uv, alt_uv: g5.texcoord_descriptors[0]}
    s.index0 = s.add_buffer(_permuted_indices(np.arange(270), 31).astype(np.uint16), abi.FORMAT_R16_UINT)
    s.idle = s.add_buffer(np.random.default_rng(22).normal(0, 1, (64, 3)).astype(f32), abi.FORMAT_R32G32B32_FLOAT)
    # the skinned row reads pt_skin_run's outputs: the last two buffers, holding the starting pose
    pos, ts = skinned(POSE_TIMES[0])
    s.skin_out = (s.add_buffer(pos, abi.FORMAT_R32G32B32_FLOAT), s.add_buffer(ts, abi.FORMAT_R10G10B10A2_UNORM))
    s.instances[6].gpu.position_descriptor, s.instances[6].gpu.tangent_space_descriptor = s.skin_out
    s.home = {k: a.copy() for k, (a, _) in enumerate(s.buffers)}
    s.add_light(abi.LIGHT_POINT, position=(0.5, -1.0, 5.0), color=(1, 0.9, 0.8), intensity=40.0)
    s.add_light(abi.LIGHT_DIRECTIONAL, direction=(0.3, 0.4, -0.8), color=(1, 1, 0.9), intensity=1.5)
    s.world_to_view = camera.orbit_world_to_view((0, 0, 0.8), 7.5, 0.4, -0.4)
    s.width, s.height = WIDTH, HEIGHT
    st = abi.PtSettings.app_defaults()
    st.min_bounces, st.max_bounces = 2, 3
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS | abi.FLAG_ACCUMULATE | abi.FLAG_ALPHA_SHADOWS)
    st.environment_color[:] = (0.6, 0.7, 0.9)
    s.settings = st
    assert len(s.instances) == 7 and 500 <= s.triangles <= 700 and all(np.abs(np.asarray(a, np.float64)).max() <= 10 for a, fmt in s.buffers if fmt == abi.FORMAT_R32G32B32_FLOAT)
    return s


def _permuted_indices(idx, seed):
    """The same triangles in another order, the corners of each in another order (any of the six, so some windings flip)."""
    rng = np.random.default_rng(seed)
    t = np.asarray(idx).reshape(-1, 3)[rng.permutation(len(idx) // 3)]
    corner = np.argsort(rng.random(t.shape), axis=1)
    return np.take_along_axis(t, corner, axis=1).reshape(-1)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
class Model:
    """The scene as the device must hold it (self.scene: buffers, instance table, materials; self.builder) and what the header says of the tree:
    self.pending, self.touched (rows touched since the last full build), self.builds / self.refits (what stats() must count), self.snapshot."""

    def __init__(self, builder):
        self.scene = start_scene()
        self.builder = builder
        self.pending, self.built, self.touched = REBUILD, False, set()
        self.builds = self.refits = 0
        self.snapshot = None
        self.home_T = list(self.scene.home_T)
        self.pose = POSE_TIMES[0]

    # -- the header's rules
    def counts(self, table=None):
        return [d.num_of_indices // 3 for d in (self.scene.instances if table is None else table)]

    def set_instances(self, table, refused=False):
        if refused: return
        cur = self.scene.instances
        if len(table) != len(cur) or self.counts(table) != self.counts(cur) or not self.built:
            self.pending = REBUILD
        else:
            differ = [i for i, (a, b) in enumerate(zip(cur, table)) if row_key(a) != row_key(b)]
            if not differ: return
            for i in differ:
                if row_key(cur[i], False) != row_key(table[i], False):
                    self.touched.add(i); self.pending = max(self.pending, REFIT)
        self.scene.instances = clone(table)

    def readers(self, b):
        return [i for i, d in enumerate(self.scene.instances) if any(get_stream(d, n) == b for n in STREAM_FIELDS)]

    def buffer_written(self, b, data):
        a, fmt = self.scene.buffers[b]
        data = np.ascontiguousarray(data)
        assert data.dtype == a.dtype and data.shape == a.shape
        self.scene.buffers[b] = (data, fmt)
        for i in self.readers(b):
            self.touched.add(i); self.pending = max(self.pending, REFIT)

    def request_rebuild(self):
        self.pending = REBUILD

    def set_builder(self, b):
        if b != self.builder: self.builder = b; self.pending = REBUILD

    def realise(self, how):
        """-> "build", "refit" or "nothing": what the call must do to the tree."""
        predict = PREDICTIONS[self.pending]
        if self.pending == REBUILD: self.builds += 1; self.touched = set(); self.built = True
        elif self.pending == REFIT: self.refits += 1
        self.pending = CLEAN
        if how == "motion_snapshot": self.snapshot = (len(self.scene.instances), self.counts())
        return predict

    def snapshot_state(self):
        if self.snapshot is None: return abi.MOTION_SNAPSHOT_NONE
        return abi.MOTION_SNAPSHOT_VALID if self.snapshot == (len(self.scene.instances), self.counts()) else abi.MOTION_SNAPSHOT_STALE

    def touched_triangles(self, inst_of_packet):
        return np.isin(inst_of_packet, sorted(self.touched))

    def state_bytes(self):
        """Every table and buffer, for "nothing changed"."""
        return (b"".join(bytes(d) for d in self.scene.instances), b"".join(bytes(m) for m in self.scene.materials),
                tuple(a.tobytes() for a, _ in self.scene.buffers), self.builder, self.pending, tuple(sorted(self.touched)), self.snapshot)

    # -- what an edit may be now
    def rows(self, pred):
        return [i for i, d in enumerate(self.scene.instances) if pred(d)]

    def choices(self, kind):
        """The parameters edit `kind` can take in this state, as lists to draw from; None if it cannot be made."""
        s, t = self.scene, self.scene.instances
        if kind in "aklmn": return {}
        if kind in "bcde": return {"rows": list(range(len(t)))}
        if kind == "f":
            r = self.rows(lambda d: d.gpu.index_descriptor != -1 and d.gpu.index_descriptor != s.index0)
            return {"rows": r} if r else None
        if kind == "g":
            r = [(i, n) for i, d in enumerate(t) for n in ("tangent", "uv0", "uv1", "color") if get_stream(d, n) != -1]
            return {"row_stream": r} if r else None
        if kind == "h":
            r = [(i, n) for i, d in enumerate(t) for n in ("position", "uv0") if get_stream(d, n) in s.twin]
            return {"row_stream": r} if r else None
        if kind == "i":
            return {"rows": [0]}                                                      # (row 0 is never dropped: MIN_ROWS)
        if kind == "j":
            what = ["count"] + (["drop"] if len(t) > MIN_ROWS else []) + (["add"] if len(t) < MAX_ROWS else [])
            return {"what": what}
        if kind == "o": return {"times": [p for p in POSE_TIMES if p != self.pose]}
        raise KeyError(kind)

    # -- an edit: the model follows it and says what to send
    def apply(self, edit):
        """-> the calls that carry the edit out, for Live.send: ("set_instances", table, rc), ("buffer_update", buffer, array), ("request_rebuild",),
        ("set_builder", b), ("set_materials", count, rc), ("skin", t).  Tables and buffers are scene-local."""
        s = self.scene
        kind, args = edit[0], edit[1:]
        table, before = clone(s.instances), clone(s.instances)
        ops = []

        def send(tb, rc=0):
            ops.append(("set_instances", clone(tb), rc)); self.set_instances(tb, rc != 0)

        def write(b, data):
            ops.append(("buffer_update", b, data)); self.buffer_written(b, data)

        if kind == "a":
            send(table)
        elif kind == "b":
            rows, salt, mode = args
            rng = np.random.default_rng(salt)
            for i in rows:
                q = rng.normal(0, 1, 4) * (0.15, 0.15, 0.15, 0) + (0, 0, 0, 1); q /= np.linalg.norm(q)
                sc = rng.uniform(0.8, 1.25, 3) * ((-1, 1, 1) if mode == "mirror" else (1, 1, 1))
                set_transform(table[i], camera.translate(rng.uniform(-0.4, 0.4, 3)) @ self.home_T[i] @ camera.trs((0, 0, 0), q, sc))
            send(table)
            if mode == "there_and_back": send(before)
        elif kind == "c":
            i, m = args; table[i].gpu.material_id = m; send(table)
        elif kind == "d":
            i, what, value = args
            if what == "mask": table[i].instance_mask = value
            else: table[i].instance_flags ^= value
            send(table)
        elif kind == "e":
            i, salt = args
            b = table[i].gpu.position_descriptor
            write(b, (s.home[b] + np.random.default_rng(salt).normal(0, 0.06, s.home[b].shape)).astype(f32))
        elif kind == "f":
            i, salt = args
            b = table[i].gpu.index_descriptor
            write(b, _permuted_indices(s.home[b], salt).astype(s.home[b].dtype))
        elif kind == "g":
            i, name, salt = args
            b = get_stream(table[i], name); a = s.home[b]; rng = np.random.default_rng(salt)
            if name in ("uv0", "uv1"): new = (a + rng.uniform(-0.3, 0.3, a.shape)).astype(f32)
            elif name == "color": new = rng.integers(0, 65536, a.shape).astype(a.dtype)
            else: new = a[rng.permutation(len(a))]                                   # packed tangent spaces: valid words, other vertices'
            write(b, new)
        elif kind == "h":
            i, name = args; set_stream(table[i], name, s.twin[get_stream(table[i], name)]); send(table)
        elif kind == "i":
            i, = args; table[i].gpu.index_descriptor = s.index0 if table[i].gpu.index_descriptor == -1 else -1; send(table)
        elif kind == "j":
            what = args[0]
            if what == "drop":
                table.pop(); self.home_T.pop()
            elif what == "add":
                d = abi.PtInstanceDesc.from_buffer_copy(bytes(start_row(3))); rng = np.random.default_rng(args[1])
                T = camera.trs(rng.uniform((-3, -3, 2.5), (3, 3, 4.5)), scale=rng.uniform(0.6, 1.2, 3)); set_transform(d, T); d.gpu.material_id = 1
                d.instance_flags = abi.INSTANCE_FLAG_TRIANGLE_CULL_DISABLE
                table.append(d); self.home_T.append(T)
            else:
                i = args[1]; full = start_count(table[i]); table[i].num_of_indices = full - 3 if table[i].num_of_indices == full else full
            send(table)
        elif kind == "k":
            ops.append(("request_rebuild",)); self.request_rebuild()
        elif kind == "l":
            ops.append(("set_builder", args[0])); self.set_builder(args[0])
        elif kind == "m":
            what = args[0]
            if what == "materials_short":
                ops.append(("set_materials", max(d.gpu.material_id for d in table), ERR_BAD_HANDLE))          # one short of the largest id in use
            else:
                i = args[1]
                if what == "dead": table[i].gpu.position_descriptor = DEAD
                elif what == "range": table[i].gpu.index_descriptor = OUT_OF_RANGE
                else: table[i].gpu.material_id = len(s.materials)
                send(table, ERR_BAD_HANDLE)
        elif kind == "n":
            b = s.idle
            assert not self.readers(b)
            write(b, np.random.default_rng(args[0]).normal(0, 1, s.home[b].shape).astype(f32))
        elif kind == "o":
            t, = args
            ops.append(("skin", t)); self.pose = t
            pos, ts = skinned(t)
            self.buffer_written(s.skin_out[0], pos); self.buffer_written(s.skin_out[1], ts)
        else:
            raise KeyError(kind)
        return ops

def start_row(i):
    start_scene()
    return _TEMPLATE[0].instances[i]


def start_count(d):
    """The full index count of the mesh a row shows (rows are told apart by their position stream, which no edit but h changes, and h keeps sizes)."""
    start_scene()
    s = _TEMPLATE[0]
    for e in s.instances:
        if e.gpu.position_descriptor == d.gpu.position_descriptor or s.twin.get(e.gpu.position_descriptor) == d.gpu.position_descriptor: return e.num_of_indices
    raise KeyError("no starting row reads buffer %d" % d.gpu.position_descriptor)


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
QUIET = "acmnl"                                                  # the kinds that can leave the tree alone (l: with the builder in force)


def draw_edit(model, rng, quiet=False):
    """One edit that can be made in the model's state; quiet: one that asks nothing of the tree."""
    while True:
        kind = QUIET[int(rng.integers(0, len(QUIET)))] if quiet else KINDS[int(rng.integers(0, len(KINDS)))]
        c = model.choices(kind)
        if c is None: continue
        pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
        salt = int(rng.integers(0, 2 ** 31))
        t = model.scene.instances
        if kind == "a": return ("a",)
        if kind == "b":
            k = int(rng.integers(1, 4))
            rows = tuple(sorted(int(x) for x in rng.choice(len(t), size=min(k, len(t)), replace=False)))
            return ("b", rows, salt, pick(["move", "move", "mirror", "there_and_back"]))
        if kind == "c":
            i = pick(c["rows"]); return ("c", i, pick([m for m in range(len(model.scene.materials)) if m != t[i].gpu.material_id]))
        if kind == "d":
            i = pick(c["rows"])
            if rng.random() < 0.5: return ("d", i, "mask", pick([m for m in (1, 2, 3) if m != t[i].instance_mask]))
            return ("d", i, "flags", pick([abi.INSTANCE_FLAG_TRIANGLE_CULL_DISABLE, abi.INSTANCE_FLAG_FORCE_NON_OPAQUE]))
        if kind == "e": return ("e", pick(c["rows"]), salt)
        if kind == "f": return ("f", pick(c["rows"]), salt)
        if kind == "g":
            n = pick(sorted({n for _, n in c["row_stream"]})); return ("g", pick([i for i, m in c["row_stream"] if m == n]), n, salt)
        if kind == "h": i, n = pick(c["row_stream"]); return ("h", i, n)
        if kind == "i": return ("i", c["rows"][0])
        if kind == "j":
            what = pick(c["what"])
            if what == "drop": return ("j", "drop")
            if what == "add": return ("j", "add", salt)
            return ("j", "count", pick(list(range(len(t)))))
        if kind == "k": return ("k",)
        if kind == "l": return ("l", model.builder if quiet or rng.random() < 0.3 else pick([b for b in BUILDERS if b != model.builder]))
        if kind == "m":
            what = pick(["dead", "range", "material", "materials_short"])
            return ("m", what) if what == "materials_short" else ("m", what, pick(list(range(len(t)))))
        if kind == "n": return ("n", salt)
        if kind == "o": return ("o", pick(c["times"]))


def sequence(seed, steps, builder=abi.BUILDER_PLOC_REINSERT):
    """-> [Step(edits, realise, predict, tags)]: `steps` steps of 0-4 edits and one realisation, drawn from `seed` alone against a model that
    starts with `builder`.  predict is the model's word on the realisation; tags names the orders of events the suite wants to have seen."""
    rng = np.random.default_rng([int(seed), int(builder), 0x5CE9E])
    model = Model(builder)
    out = []
    for _ in range(steps):
        quiet = rng.random() < 0.2                                       # a step that must come out as "nothing" (unless work was pending before it)
        n = int(rng.choice(3, p=(0.4, 0.35, 0.25))) if quiet else int(rng.choice(5, p=(0.03, 0.27, 0.30, 0.24, 0.16)))
        edits, tags = [], set()
        for _ in range(n):
            e = draw_edit(model, rng, quiet)
            was = model.pending, model.built, set(model.touched)
            model.apply(e)
            edits.append(e)
            if e[0] == "l" and was[0] == REFIT and model.pending == REBUILD: tags.add("refit pending, then builder change")
            if was[0] == REBUILD and was[1] and model.touched - was[2]: tags.add("rebuild pending, then same-shape edit")
            if e[0] == "b" and e[3] == "there_and_back": tags.add("edit moved and moved back")
        how = REALISATIONS[int(rng.integers(0, len(REALISATIONS)))]
        out.append(Step(tuple(edits), how, model.realise(how), frozenset(tags)))
    return out


def replay(builder, steps, upto=None):
    """A fresh model taken through steps[:upto] (edits and realisations)."""
    m = Model(builder)
    for st in steps[:upto]:
        for e in st.edits: m.apply(e)
        m.realise(st.realise)
    return m


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------
def world_triangles(scene):
    from tests import accel_ref as ar
    return np.concatenate([ar.mul_point(r["transform"], ar.row_vertices(r)).astype(np.float64) for r in ar.scene_rows(scene)]), \
           np.concatenate([np.full(r["triangles"], i) for i, r in enumerate(ar.scene_rows(scene))])


def make_rays(seed, oracle, scene, aimed=2000, surface=2000):
    """[aimed + surface, 8] float32 rays (origin, tmin, direction, tmax) for a sequence: `aimed` from a sphere around the scene at points of the
    STARTING scene's triangles, `surface` as the path tracer casts them (ray_hook.surface_rays: camera rays, then rays from the points they hit).
    oracle: a backend holding the starting scene."""
    from tests import ray_hook
    rng = np.random.default_rng([int(seed), 0x4A15])
    tris, _ = world_triangles(scene)
    tk = tris[rng.integers(0, len(tris), aimed)]
    w = rng.dirichlet((1, 1, 1), aimed)
    target = (tk * w[:, :, None]).sum(axis=1)
    d = rng.standard_normal((aimed, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    origin = (np.array([0.0, 0.0, 0.8]) + 25.0 * d).astype(f32)
    to = target - origin; to /= np.linalg.norm(to, axis=1, keepdims=True)
    a = np.zeros((aimed, 8), f32); a[:, 0:3] = origin; a[:, 4:7] = to.astype(f32); a[:, 7] = 1000.0
    # surface_rays casts its camera rays in every direction from the camera: from the picture's camera, outside the scene, one in twenty hits;
    # from the middle of the scene four in ten do, and each hit starts a second ray
    eye = types.SimpleNamespace(world_to_view=np.linalg.inv(camera.translate(RAY_EYE)))
    first, second = ray_hook.surface_rays(oracle, eye, surface + surface // 2, seed)
    both = np.concatenate([second, first])[:surface]                       # the rays from surface points first: they are the ones with no slack
    assert len(both) == surface and len(second) >= surface // 4, (len(first), len(second))
    return np.ascontiguousarray(np.concatenate([a, both]))


# ---- playing a sequence into a backend -----------------------------------------------------------------------------------------------------
def _resolve_materials(scene, handles, count):
    mats = []
    for m in scene.materials[:count]:
        c = abi.PtMaterial.from_buffer_copy(bytes(m))
        for slot in abi.PtMaterial.TEXTURE_SLOTS:
            ts = getattr(c, slot)
            if ts.descriptor != -1: ts.descriptor = handles["textures"][ts.descriptor]
            ts.sampler = handles["samplers"][ts.sampler]
        mats.append(c)
    return mats


class Live:
    """A backend (the product's Renderer, or the oracle) that follows a model edit by edit.  The starting scene goes in as a host would load it:
    every buffer but the skinned row's outputs, the row on its bind-pose streams; scenes.SkinBinding then creates the outputs, re-points the row
    and skins the starting pose.  send() carries out what Model.apply returned; a call the model marks refused must come back with that code (the
    oracle has no refusals: it is not sent those)."""

    def __init__(self, backend, model, is_product=True):
        import ctypes as C
        self.C, self.backend, self.is_product = C, backend, is_product
        s = model.scene
        pre = copy.copy(s)
        pre.buffers = s.buffers[:-2]
        pre.instances = clone(s.instances)
        sk = s.skins[0]
        pre.instances[sk["instance"]].gpu.position_descriptor = sk["input_position"]
        pre.instances[sk["instance"]].gpu.tangent_space_descriptor = sk["input_tangent_space"]
        if is_product: backend.set_accel_builder(model.builder)
        self.handles = pre.upload(backend)
        self.binding = scenes.SkinBinding(backend, pre, self.handles, 0, use_mfma=0)
        self.binding.pose(POSE_TIMES[0])
        self.bmap = list(self.handles["buffers"]) + [self.binding.out_position, self.binding.out_tangent_space]
        self.dead = None
        if is_product:
            self.dead = backend.buffer_create(np.zeros(16, f32), abi.FORMAT_R32G32B32_FLOAT)
            backend.buffer_destroy(self.dead)
        self.scene = s

    def handle(self, b):
        return -1 if b == -1 else self.dead if b == DEAD else b if b == OUT_OF_RANGE else self.bmap[b]

    def table(self, local):
        out = clone(local)
        for d in out:
            for n in STREAM_FIELDS: set_stream(d, n, self.handle(get_stream(d, n)))
        return out

    def send(self, ops):
        C, r = self.C, self.backend
        for op in ops:
            if op[0] == "set_instances":
                _, tb, want = op
                if not self.is_product:
                    if want == 0: r.set_instances(self.table(tb))
                    continue
                t = self.table(tb)
                arr = (abi.PtInstanceDesc * len(t))(*t)
                rc = r.L.pt_scene_set_instances(r.h, C.byref(arr), len(t))
                assert rc == want, "pt_scene_set_instances returned %d (%s), the model expects %d" % (rc, r.L.pt_last_error(r.h).decode(), want)
            elif op[0] == "set_materials":
                _, count, want = op
                if not self.is_product: continue
                mats = _resolve_materials(self.scene, self.handles, count)
                arr = (abi.PtMaterial * max(len(mats), 1))(*mats)
                rc = r.L.pt_scene_set_materials(r.h, C.byref(arr), len(mats))
                assert rc == want, "pt_scene_set_materials returned %d (%s), the model expects %d" % (rc, r.L.pt_last_error(r.h).decode(), want)
            elif op[0] == "buffer_update": r.buffer_update(self.bmap[op[1]], op[2])
            elif op[0] == "request_rebuild":
                if self.is_product: r.request_rebuild()
            elif op[0] == "set_builder":
                if self.is_product: r.set_accel_builder(op[1])
            elif op[0] == "skin": self.binding.pose(op[1])
            else: raise KeyError(op[0])


def load_fresh(backend, model, is_product=True):
    """The model's state into a new context, as one upload: what the edited context must be indistinguishable from."""
    if is_product: backend.set_accel_builder(model.builder)
    return model.scene.upload(backend)


def describe(seed, builder, k, step):
    return "seed %d builder %d step %d: edits %r then %s (the model predicts %s)" % (seed, builder, k, list(step.edits), step.realise, step.predict)


# The cases the suite runs: every builder with each of these seeds, STEPS steps each (a builder's sequence of a seed is its own).
# tests/test_scene_edit_model_host.py asserts what these 96 steps cover; STEPS is what fits the time a GPU case may take
# (tests/test_gpu_scene_edits.py has the figures); tools/scene_edit_fuzz.py runs sequences of any length.
SEEDS = (0, 1, 2, 3)
STEPS = 8
