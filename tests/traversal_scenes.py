"""Scenes and rays shared by the traversal tests (tests/test_gpu_traversal_driver.py, tests/test_traversal_host.py, tests/test_gpu_round3.py)."""
import numpy as np

from gltf_renderer_amd import abi, meshgen, scenes

f32 = np.float32


def _deep_chain_scene(dups=4096, size=32):
    """A legal scene whose radix tree needs more traversal-stack entries than a lane holds on chip, and whose rays really use them.
    57 thin sheets perpendicular to the view direction (+x) whose bounding-box centres are (C,0,0), (0,C,0) or (0,0,C) with
    C = (2^j + 1/4) 2^-10, j = 0..18 -- long thin triangles for the y and z kinds: every Morton code has a different highest bit, so the
    radix tree is one chain, 57 binary levels deep -- plus `dups` coincident copies of the nearest sheet (equal codes: a subtree balanced by
    index below the chain's end).  Each chain level's sheet lies farther along the ray than everything below it, so a ray enters the inner
    child first and leaves the sheets on its stack: ~3 entries per wide level all the way down, then 3 more per level of the copies."""
    from gltf_renderer_amd import camera, meshgen
    f32 = np.float32
    u, h, w, eps = 2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 2.0 ** -20
    tris = [[(-eps, -h, -h), (-eps, h, -h), (-eps, 0, h)]] * dups                 # the nearest sheet, `dups` times
    k = 0
    for j in range(19):
        C = (2.0 ** j + 0.25) * u
        xk = (k + 1) * eps; k += 1
        tris.append([(xk, -h, -w), (xk, -h, 2 * C + w), (xk, h, -w)])             # centre (~0, 0, C): long along z
        xk = (k + 1) * eps; k += 1
        tris.append([(xk, -w, -h), (xk, 2 * C + w, -h), (xk, -w, h)])             # centre (~0, C, 0): long along y
        k += 1
        tris.append([(C, -h, -h), (C, h, -h), (C, 0, h)])                         # centre (C, 0, 0)
    pos = np.array(tris, f32)[:, [0, 2, 1], :].reshape(-1, 3)                     # wound so that the geometric normal faces the camera (-x)
    n = len(pos) // 3
    mesh = meshgen.Mesh(pos, np.arange(3 * n), normals=np.tile(np.array([[-1, 0, 0]], f32), (3 * n, 1)),
                        uv0=np.tile(np.array([[0, 1], [1, 1], [0.5, 0]], f32), (n, 1)))
    s = scenes.single_triangle(size)
    s.instances.clear(); s.mesh_records.clear(); s.buffers.clear(); s.triangles = 0
    m = s.add_material(scenes.material(base_color_factor=(0.8, 0.6, 0.4, 1.0), flags=abi.MATERIAL_FLAG_DOUBLE_SIDED))
    s.add_mesh(mesh, None, m)
    s.world_to_view = camera.free_world_to_view((-0.5, 0.0, 0.0), yaw=-np.pi / 2)
    assert np.allclose(s.world_to_view @ np.array([1.0, 0, 0, 0]), [0, 0, -1, 0], atol=1e-12)          # looking along +x
    s.ortho = (1.0 / (0.15 * h), 1.0 / (0.15 * h))                                # half extents 1 / mag: every ray inside every sheet
    st = abi.PtSettings.app_defaults(); st.min_bounces, st.max_bounces = 1, 2
    st.flags &= ~(abi.FLAG_ENVIRONMENT_MAP | abi.FLAG_ENVIRONMENT_MIS)            # no map: the constant colour lights the scene
    st.environment_color[:] = (1.0, 1.0, 1.0)
    s.settings = st
    return s, n


# ---- eight parallel alpha sheets --------------------------------------------------------------------------------------------------------
SHEET_KINDS = ("opaque single-sided", "mask 0.5", "blend", "mask 0 (never ignored)", "blend mirrored", "mask 1.5 (always ignored)", "blend vertex alpha 0",
               "opaque double-sided")
SHEET_SPACING = 0.5


def _sheet_texel(i, j, k):
    """The texel of the 8x8 alpha pattern that triangle k of quad (i, j) reads."""
    return 2 * i + k, 2 * j + (k ^ (i & 1))


def _sheet_mesh(colors_alpha=None):
    """A 4x4 grid of quads over [-1, 1]^2 at z = 0, front faces towards +z, NO shared vertices: each triangle carries its own texture
    coordinates, all three inside ONE texel of an 8x8 pattern (a quarter texel from its edges), so that which texel a hit reads does not
    depend on the last bits of its barycentrics."""
    pos, uv = [], []
    corner = ((0.25, 0.25), (0.75, 0.25), (0.5, 0.75))
    for j in range(4):
        for i in range(4):
            x0, y0 = -1.0 + 0.5 * i, -1.0 + 0.5 * j
            p = [(x0, y0, 0.0), (x0 + 0.5, y0, 0.0), (x0 + 0.5, y0 + 0.5, 0.0), (x0, y0 + 0.5, 0.0)]
            for k, tri in enumerate(((0, 1, 2), (0, 2, 3))):
                ti, tj = _sheet_texel(i, j, k)
                for c, vtx in enumerate(tri):
                    pos.append(p[vtx]); uv.append(((ti + corner[c][0]) / 8.0, (tj + corner[c][1]) / 8.0))
    n = len(pos)
    colors = None
    if colors_alpha is not None:
        rng = np.random.default_rng(4)
        colors = np.concatenate([rng.random((n, 3)), np.full((n, 1), colors_alpha)], axis=1)
    return meshgen.Mesh(np.array(pos, f32), np.arange(n), normals=np.tile(np.array([[0, 0, 1]], f32), (n, 1)), uv0=np.array(uv, f32), colors=colors)


def _alpha_pattern(seed):
    """8x8 RGBA8: the alpha of the 32 texels the sheets' triangles read cycles through 0, 127, 128, 255 every fourth triangle (127 / 255 and
    128 / 255 straddle a cutoff of 0.5), the others are 1 .. 252 (alpha <= 0.99)."""
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 253, (8, 8, 4)).astype(np.uint8)
    special = (0, 127, 128, 255)
    m = 0
    for j in range(4):
        for i in range(4):
            for k in range(2):
                ti, tj = _sheet_texel(i, j, k)
                if (m + j) % 3 == 0: t[tj, ti, 3] = special[(m // 3) % 4]
                m += 1
    return t


def layered_alpha_scene():
    """Eight parallel sheets 0.5 apart (256 triangles), each its own instance and material (SHEET_KINDS, bottom to top); the two opaque sheets
    and the never-ignored MASK sheet are shifted sideways by half their width so that rays also pass beside them.  Every alpha is a product
    of exactly reproducible factors (tests/traversal_ref.py): base_color_factor.w, a POINT-filtered texel, a vertex alpha of 0."""
    s = scenes.SceneData("layered_alpha")
    TS = abi.PtTextureSample
    point = s.add_sampler(abi.ADDRESS_WRAP, abi.ADDRESS_WRAP, abi.FILTER_POINT, abi.FILTER_POINT)
    t_mask = s.add_texture(_alpha_pattern(11), True)
    t_blend = s.add_texture(_alpha_pattern(12), False)
    DS = abi.MATERIAL_FLAG_DOUBLE_SIDED
    mats = [scenes.material(base_color_factor=(0.8, 0.2, 0.2, 1.0)),
            scenes.material(flags=DS, alpha_mode=abi.ALPHA_MODE_MASK, alpha_cutoff=0.5, albedo=TS(t_mask, point)),
            scenes.material(alpha_mode=abi.ALPHA_MODE_BLEND, base_color_factor=(0.2, 0.9, 0.3, 1.0), albedo=TS(t_blend, point)),
            scenes.material(alpha_mode=abi.ALPHA_MODE_MASK, alpha_cutoff=0.0, albedo=TS(t_mask, point)),
            scenes.material(alpha_mode=abi.ALPHA_MODE_BLEND, alpha_cutoff=0.5, base_color_factor=(0.3, 0.3, 0.9, 0.75), albedo=TS(t_blend, point)),
            scenes.material(flags=DS, alpha_mode=abi.ALPHA_MODE_MASK, alpha_cutoff=1.5, albedo=TS(t_mask, point)),
            scenes.material(flags=DS, alpha_mode=abi.ALPHA_MODE_BLEND, alpha_cutoff=0.25, base_color_factor=(0.9, 0.9, 0.2, 1.0), albedo=TS(t_blend, point)),
            scenes.material(flags=DS, base_color_factor=(0.5, 0.5, 0.5, 1.0))]
    shift = {0: (1.0, 0.0), 3: (0.0, 1.0), 7: (-1.0, 0.0)}
    for k, m in enumerate(mats):
        T = np.eye(4)
        if k == 4: T[0, 0] = -1.0                                         # the mirrored instance
        sx, sy = shift.get(k, (0.0, 0.0))
        T[:3, 3] = (sx, sy, k * SHEET_SPACING)
        s.add_mesh(_sheet_mesh(0.0 if k == 6 else None), T, s.add_material(m))
    assert s.triangles == 256
    return s


def layered_rays(n, seed, tmax=100.0):
    """[n, 8] float32 rays (tmin = 0) for layered_alpha_scene: a third aimed at interior points of random triangles from anywhere around the
    stack, a third nearly along the stack's axis (up and down: six to eight crossings), a third between random points of the surrounding box."""
    from traversal_ref import Triangles
    rng = np.random.default_rng(seed)
    P = Triangles(layered_alpha_scene()).P
    k = n // 3
    o = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.5, 2.5, n), np.where(rng.random(n) < 0.5, rng.uniform(-1.5, -0.2, n), rng.uniform(3.7, 5.0, n))], axis=1)
    inside = rng.random(n) < 0.25                                          # some origins between the sheets, a tenth of the spacing off their planes
    zi = (rng.integers(0, 7, n) + rng.uniform(0.1, 0.9, n)) * SHEET_SPACING
    o[inside, 2] = zi[inside]
    w = 0.08 + 0.76 * rng.dirichlet((1, 1, 1), k)
    target = (P[rng.integers(0, len(P), k)] * w[:, :, None]).sum(axis=1)
    d = np.zeros((n, 3))
    d[:k] = target - o[:k]
    m = n - 2 * k
    o[k:k + m, 0:2] = rng.uniform(-1.9, 1.9, (m, 2)); up = rng.random(m) < 0.5
    o[k:k + m, 2] = np.where(up, -1.0, 4.5)
    d[k:k + m] = np.stack([rng.normal(0, 0.08, m), rng.normal(0, 0.08, m), np.where(up, 1.0, -1.0)], axis=1)
    q = np.stack([rng.uniform(-2.5, 2.5, k), rng.uniform(-2.5, 2.5, k), rng.uniform(-1.5, 5.0, k)], axis=1)
    d[k + m:] = q - o[k + m:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), f32); rays[:, 0:3] = o; rays[:, 4:7] = d; rays[:, 7] = tmax
    return rays


def alpha_aimed_rays(s, n, seed, tmax=1000.0):
    """[n, 8] float32 rays (tmin = 0) through a scene's MASK and BLEND instances: from random points of the scene's box (grown by a quarter)
    towards random points of their triangles, and on past them."""
    from traversal_ref import Triangles
    rng = np.random.default_rng(seed)
    T = Triangles(s)
    pick = np.nonzero(np.array([s.materials[m].alpha_mode != abi.ALPHA_MODE_OPAQUE for _, _, m in s.mesh_records])[T.inst])[0]
    lo, hi = T.P.reshape(-1, 3).min(0), T.P.reshape(-1, 3).max(0)
    o = lo - 0.25 * (hi - lo) + rng.random((n, 3)) * 1.5 * (hi - lo)
    target = (T.P[pick[rng.integers(0, len(pick), n)]] * rng.dirichlet((1, 1, 1), n)[:, :, None]).sum(axis=1)
    d = target - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), f32); rays[:, 0:3] = o; rays[:, 4:7] = d; rays[:, 7] = tmax
    return rays
