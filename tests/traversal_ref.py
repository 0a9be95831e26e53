"""A float64 restatement of what a ray finds in a scene: every triangle crossing, then the any-hit rules.  Plain numpy, no tree.

Written from the rules csrc/pt_traverse.h's header states and the DXR semantics they name, for checking the product's two traversal
drivers AND the CPU oracle's port of them (tests/test_traversal_host.py, tests/test_gpu_traversal_driver.py):

  * a triangle is a candidate of a ray if the ray crosses it (Moeller-Trumbore, u >= 0, v >= 0, u + v <= 1) at tmin < t < tmax, the ray's
    instance mask meets the instance's, and it is not culled: the FRONT face is the counter-clockwise one in OBJECT space (under a mirrored
    instance transform the world-space winding is the other way round); RF_CULL_BACK drops back faces and RF_CULL_FRONT front faces unless the
    instance disables culling;
  * a candidate is NON-OPAQUE if its instance is flagged so (MASK materials) or the ray forces it; only those run an any-hit rule;
  * closest-hit rays (mode 0): a non-opaque candidate whose BASE alpha is below the material's cutoff is ignored (whatever the alpha mode);
    the nearest candidate left is the hit;
  * occlusion rays that accept the first hit (mode 1 without RF_FORCE_NON_OPAQUE): the shadow payload starts at 0, so the any-hit rule of
    a non-opaque candidate (payload *= 1 - alpha; end the search at 0) ends the search too: ANY candidate occludes, cut-outs included;
  * alpha-shadow rays (mode 1 with RF_FORCE_NON_OPAQUE): the payload starts at 1 and is multiplied by 1 - alpha of EVERY candidate of the
    interval; a payload of exactly 0 ends the search (and is 0 whatever the order).  Any candidate "commits"; a ray with none reports 1.

Alpha comes from sources a float64 restatement reproduces EXACTLY, as the fp32 numbers the kernels form: base_color_factor.w, a vertex-colour
alpha that is the same at the three vertices AND 0 (c * w0 + c * w1 + c * w2 is c in fp32 for every weight triple only then), and the alpha
of a POINT-filtered or 1x1 albedo texture (texel / 255 correctly rounded; the texel by floor(uv * size), so keep a triangle's uv inside one texel).
The factors 1 - alpha are then exact fp32 numbers and only the ORDER of the fp32 products is left open: k factors, any two orders differ by
at most 2 (k - 1) 2^-24 relative.

A ray is UNDECIDED -- left out of every comparison -- if for any triangle its float64 barycentrics lie within MARGIN of an edge, its t within
MARGIN (relative) of tmin, tmax or another candidate's t, or |det| < 1e-9 |e1| |e2| |d|: there fp32 and float64 may legitimately differ."""
import numpy as np

from gltf_renderer_amd import abi

MARGIN = 1e-4
RF_CULL_BACK, RF_CULL_FRONT, RF_FORCE_NON_OPAQUE, RF_ACCEPT_FIRST = 1, 2, 4, 8
f32 = np.float32


class Triangles:
    """The scene's triangles in world space (float64) with what the rules need of their instances and materials."""

    def __init__(self, s):
        P, inst, prim = [], [], []
        self.scene = s
        for i, (mesh, T, mat_id) in enumerate(s.mesh_records):
            T = np.asarray(T, np.float64)
            p = mesh.positions.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            idx = np.arange(len(p)) if mesh.indices is None else mesh.indices.astype(np.int64)
            P.append(p[idx].reshape(-1, 3, 3)); n = len(idx) // 3
            inst.append(np.full(n, i)); prim.append(np.arange(n))
        self.P = np.concatenate(P); self.inst = np.concatenate(inst); self.prim = np.concatenate(prim)
        d = s.instances
        self.mirrored = np.array([np.linalg.det(np.asarray(T, np.float64)[:3, :3]) < 0 for _, T, _ in s.mesh_records])[self.inst]
        self.cull_disable = np.array([bool(x.instance_flags & abi.INSTANCE_FLAG_TRIANGLE_CULL_DISABLE) for x in d])[self.inst]
        self.non_opaque = np.array([bool(x.instance_flags & abi.INSTANCE_FLAG_FORCE_NON_OPAQUE) for x in d])[self.inst]
        self.mask = np.array([int(x.instance_mask) & 0xff for x in d])[self.inst]

    # ---- alpha of crossings (tri index arrays + float64 barycentrics) ------------------------------------------------------------
    def alpha(self, tri, u, v):
        """-> (base alpha, alpha, cutoff) as the fp32 numbers the any-hit rules see, float32 arrays."""
        s = self.scene
        base = np.zeros(len(tri), f32); alpha = np.zeros(len(tri), f32); cutoff = np.zeros(len(tri), f32)
        for i in np.unique(self.inst[tri]):
            sel = np.nonzero(self.inst[tri] == i)[0]
            mesh, _, mat_id = s.mesh_records[i]
            m = s.materials[mat_id]
            idx = (np.arange(mesh.num_vertices) if mesh.indices is None else mesh.indices.astype(np.int64)).reshape(-1, 3)[self.prim[tri[sel]]]
            w = np.stack([1.0 - u[sel] - v[sel], u[sel], v[sel]], axis=1)
            col = np.full(len(sel), f32(m.base_color_factor[3]), f32)
            if mesh.colors is not None:
                q = np.round(np.clip(mesh.colors[:, 3].astype(f32), 0, 1) * f32(65535.0)).astype(np.float64) / 65535.0     # R16G16B16A16_UNORM
                c = q[idx]
                assert np.all(c == 0.0), "a vertex-colour alpha other than 0 is not reproduced exactly (see the module docstring)"
                col = (col * f32(0.0)).astype(f32)
            ts = m.albedo
            if ts.descriptor != -1:
                tex, _srgb = s.textures[ts.descriptor]                      # (alpha is linear in an sRGB texture too)
                H, W = tex.shape[:2]
                if not (H == 1 and W == 1):
                    assert ts.sampler != 0 and s.samplers[ts.sampler - 1][2:] == (abi.FILTER_POINT, abi.FILTER_POINT), "alpha texture must be POINT-filtered or 1x1"
                    assert s.samplers[ts.sampler - 1][:2] == (abi.ADDRESS_WRAP, abi.ADDRESS_WRAP)
                assert ts.rotation == 0.0 and tuple(ts.offset) == (0.0, 0.0) and tuple(ts.scale) == (1.0, 1.0) and ts.tex_coord == 0
                uv = (mesh.uv0.astype(np.float64)[idx] * w[:, :, None]).sum(axis=1) if mesh.uv0 is not None else np.zeros((len(sel), 2))
                ti = np.floor(uv[:, 0] * W).astype(np.int64) % W; tj = np.floor(uv[:, 1] * H).astype(np.int64) % H
                texel = (tex[tj, ti, 3].astype(np.float64) / 255.0).astype(f32)      # correctly rounded x / 255
                col = (col * texel).astype(f32)
            base[sel] = col; cutoff[sel] = f32(m.alpha_cutoff)
            if m.alpha_mode == abi.ALPHA_MODE_BLEND: alpha[sel] = col
            elif m.alpha_mode == abi.ALPHA_MODE_MASK: alpha[sel] = np.where(col < f32(m.alpha_cutoff), f32(0), f32(1))
            else: alpha[sel] = f32(1)
        return base, alpha, cutoff


class Crossings:
    """Every triangle crossing of every ray of a set, in float64, found once and shared by all modes and flags: arrays over crossings (ray,
    tri, t, u, v, front) for t > 0 -- the interval is applied per query -- and per ray the geometric part of `undecided`."""

    def __init__(self, tris, rays, chunk=2048, with_alpha=True):
        self.tris = tris
        rays = np.asarray(rays, np.float32).reshape(-1, 8).astype(np.float64)
        self.n = len(rays); self.rays = rays
        v0 = tris.P[:, 0]; e1 = tris.P[:, 1] - v0; e2 = tris.P[:, 2] - v0
        ne = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
        R, Tr, tt, uu, vv, ff = [], [], [], [], [], []
        fuzzy = np.zeros(self.n, bool)
        chunk = max(16, min(chunk, 1_000_000 // max(len(tris.P), 1)))       # the [rays, triangles, 3] temporaries stay small
        for a in range(0, self.n, chunk):
            o = rays[a:a + chunk, 0:3]; d = rays[a:a + chunk, 4:7]
            p = np.cross(d[:, None, :], e2[None])                         # [r, t, 3]
            det = (e1[None] * p).sum(-1)
            small = np.abs(det) < 1e-9 * ne[None] * np.linalg.norm(d, axis=1)[:, None]
            inv = 1.0 / np.where(det == 0, 1.0, det)
            tv = o[:, None, :] - v0[None]
            u = (tv * p).sum(-1) * inv
            q = np.cross(tv, e1[None])
            v = (d[:, None, :] * q).sum(-1) * inv
            t = (e2[None] * q).sum(-1) * inv
            inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (det != 0)
            near_edge = (np.minimum(np.minimum(u, v), 1 - u - v) > -MARGIN) & (np.minimum(np.minimum(u, v), 1 - u - v) < MARGIN) & (u > -MARGIN) & (v > -MARGIN) & (u + v < 1 + MARGIN)
            ahead = t > -MARGIN
            fuzzy[a:a + chunk] |= ((near_edge | (small & (np.abs(u) < 2) & (np.abs(v) < 2))) & ahead).any(axis=1)
            r, k = np.nonzero(inside & (t > 0))
            R.append(r + a); Tr.append(k); tt.append(t[r, k]); uu.append(u[r, k]); vv.append(v[r, k])
            ff.append((det[r, k] > 0) != tris.mirrored[k])
        self.ray = np.concatenate(R); self.tri = np.concatenate(Tr); self.t = np.concatenate(tt); self.u = np.concatenate(uu); self.v = np.concatenate(vv)
        self.front = np.concatenate(ff)
        self.fuzzy = fuzzy
        if with_alpha: self.base, self.alpha, self.cutoff = tris.alpha(self.tri, self.u, self.v)

    def count(self, tmax):
        """Per ray, the crossings in (0, tmax) of any facing and material: an upper bound of the candidates of any query."""
        return np.bincount(self.ray[self.t < tmax], minlength=self.n)

    def query(self, rf, mode, mask=0xff, tmin=None, tmax=None):
        """-> dict of per-ray arrays: committed, t, u, v, instance, primitive, front (mode 0: the closest accepted hit; -1 / 0 for a miss),
        transmission (mode 1: the product in float64, 1 where nothing is committed), zero (a factor of exactly 0 among the candidates),
        k (candidates that took part), undecided."""
        T = self.tris; n = self.n
        tmin = self.rays[:, 3] if tmin is None else np.broadcast_to(np.float64(tmin), (n,))
        tmax = self.rays[:, 7] if tmax is None else np.broadcast_to(np.float64(tmax), (n,))
        r = self.ray
        und = self.fuzzy.copy()
        lo, hi = tmin[r], tmax[r]
        edge_t = (np.abs(self.t - lo) <= MARGIN * np.maximum(np.abs(lo), 1.0)) | (np.abs(self.t - hi) <= MARGIN * np.abs(hi))
        np.logical_or.at(und, r[edge_t], True)
        # two crossings of one ray at (nearly) the same distance
        order = np.lexsort((self.t, r))
        same = (r[order][1:] == r[order][:-1]) & (self.t[order][1:] - self.t[order][:-1] <= MARGIN * self.t[order][1:])
        np.logical_or.at(und, r[order][1:][same], True)
        cand = (self.t > lo) & (self.t < hi) & ((T.mask[self.tri] & mask) != 0)
        culled = ~T.cull_disable[self.tri] & (((rf & RF_CULL_BACK) != 0) & ~self.front | ((rf & RF_CULL_FRONT) != 0) & self.front)
        cand &= ~culled
        non_opaque = T.non_opaque[self.tri] | bool(rf & RF_FORCE_NON_OPAQUE)
        out = {"undecided": und, "k": np.bincount(r[cand], minlength=n)}
        if mode == 0:
            acc = cand & ~(non_opaque & (self.base < self.cutoff))
            best = np.full(n, np.inf)
            np.minimum.at(best, r[acc], self.t[acc])
            win = acc & (self.t == best[r])
            which = np.full(n, -1); which[r[win]] = np.nonzero(win)[0]
            hit = which >= 0
            w = np.where(hit, which, 0)
            out.update(committed=hit, t=np.where(hit, self.t[w], 0.0), u=np.where(hit, self.u[w], 0.0), v=np.where(hit, self.v[w], 0.0),
                       instance=np.where(hit, T.inst[self.tri[w]], -1), primitive=np.where(hit, T.prim[self.tri[w]], -1), front=hit & self.front[w])
            return out
        committed = np.zeros(n, bool); committed[r[cand]] = True
        out["committed"] = committed
        if not (rf & RF_FORCE_NON_OPAQUE):                                 # accept-first: any candidate occludes
            out["transmission"] = np.where(committed, 0.0, 1.0); out["zero"] = committed.copy()
            return out
        factor = (f32(1) - self.alpha).astype(f32).astype(np.float64)        # the exact fp32 factors
        prod = np.ones(n); np.multiply.at(prod, r[cand], factor[cand])
        zero = np.zeros(n, bool); zero[r[cand & (factor == 0.0)]] = True
        prod[zero] = 0.0
        out["transmission"] = prod; out["zero"] = zero
        return out
