"""A numpy restatement of the frames of an instanced scene, written from include/crt.h (the contracts of crt_instances_trace,
crt_scene_create_instanced and crt_scene_create_instanced_lit) and from tests/integrator_ref.py — not from rt_kernels.hip, instances.hip or
oracle/, and importing nothing from oracle/ (DESIGN.md "Instanced frames as tested").

The integrator is integrator_ref.render_frame itself: `InstancedRef` answers the questions that loop asks of a scene (visibility with a
ray class, hit -> triangle row and material, the normal's way to world space, the emitter's light, the light table), each as ONE float32
IEEE operation per step, nothing fused.  What the header states and this module restates:

  world_to_object  in double, rounded once: adj(A) / det(A), det = (a c00 + b c01) + c c02 along the first row, each adjugate entry one
                   difference of two products (the forms below), translation 0 - ((x t0 + y t1) + z t2) from the unrounded row
  object ray       o'_r = ((W_r0 o.x + W_r1 o.y) + W_r2 o.z) + W_r3, d' likewise without W_r3, not renormalised; a bitwise-identity matrix
                   keeps the ray; an object origin that is not finite hits nothing in that instance
  visibility       brute force over every triangle of every visible instance, the minimum of (t, instance, id) with 0 <= t < tmax
  material         v[3] + material_offset
  normal           identity flag: n_obj; else m_c = (W_0c n.x + W_1c n.y) + W_2c n.z, n = m (|n_obj| / |m|), n = m when |m| is 0 or not finite
  hit point        (o + d t) + n 0.0002f on the WORLD ray (integrator_ref's line, fed the world ray)
  light table      static lights, then instance by instance the mesh's lights moved (`moved_lights`), the pdf column by the tree sum
  emitter's light  first[instance] + min(ew, nl - 1) on a light-bearing mesh, min(ew, total - 1) on any other, weight 1 with an empty table;
                   lights[ew] in a scene without mesh lights

Disney materials stay outside, as in integrator_ref.  `breaks` are deliberate mistakes (tests/test_instanced_ref.py's sensitivity table):
each must change words of some scene, or the scenes do not test the rule it breaks."""
import numpy as np

import integrator_ref as ir
from integrator_ref import F, f32, f64

IDENTITY_BITS = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32).view(np.uint32)

CLASSES = ("primary", "bounce", "shadow")
CENSUS_KEYS = tuple(f"hits_{kind}_{c}" for kind in ("identity", "general", "mirrored") for c in CLASSES[:2]) + (
    "hits_with_offset", "textured_through_offset", "mirror_on_general", "emitter_after_bounce_clamped", "emitter_after_bounce_unclamped",
    "emitter_after_bounce_lightless_mesh", "emitter_empty_table", "nee_moved_light", "nee_mirrored_lamp_light",
    "mask_changes_primary", "mask_changes_bounce", "shadow_blocked_only_by_hidden", "cross_instance_ties")

BREAKS = ("light_normal_by_A", "shadow_mask_bounce", "bounce_mask_primary", "clamp_nl", "first_in_other_order", "unit_normal",
          "hit_point_object_ray", "vt_without_base", "lightless_uses_first", "empty_table_prev_pdf", "pdf_as_given", "ties_to_higher_instance",
          "mirror_keeps_is_specular")


def world_to_object(m):
    """crt_instance_inverse's rule in float64 (Python floats: one IEEE double operation each), rounded once to float32"""
    a, b, c, t0, d, e, f, t1, g, h, i, t2 = (float(x) for x in F(m).reshape(12))
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    adj = ((c00, c * h - b * i, b * f - c * e), (c01, a * i - c * g, c * d - a * f), (c02, b * g - a * h, a * e - b * d))
    out = []
    for r in adj:
        x, y, z = r[0] / det, r[1] / det, r[2] / det
        out += [x, y, z, 0.0 - ((x * t0 + y * t1) + z * t2)]
    return np.array(out, f64).astype(f32).reshape(3, 4)


def is_identity(m):
    return bool(np.array_equal(F(m).reshape(3, 4).view(np.uint32), IDENTITY_BITS))


def _rows(A, x, translate):
    """(A_r0 x.x + A_r1 x.y) + A_r2 x.z [+ A_r3] for points x (n, 3) and one 3x4 matrix"""
    out = F(F(F(A[:, 0] * x[:, 0:1]) + F(A[:, 1] * x[:, 1:2])) + F(A[:, 2] * x[:, 2:3]))
    return F(out + A[:, 3]) if translate else out


def moved_lights(A, W, lights, normal_by_A=False):
    """np_light of tests/test_instance_lights.py for a whole (n, 18) array: p', u', v', n', area' as the header writes them"""
    A, W, l = F(A).reshape(3, 4), F(W).reshape(3, 4), F(lights).reshape(-1, 18)
    out = np.zeros_like(l)
    with np.errstate(all="ignore"):
        out[:, 0:3] = _rows(A, l[:, 0:3], True)
        out[:, 3:6] = _rows(A, l[:, 3:6], False)
        out[:, 6:9] = _rows(A, l[:, 6:9], False)
        n = l[:, 9:12]
        m = _rows(A, n, False) if normal_by_A else _rows(W[:, :3].T, n, False)          # m_c = (W_0c n.x + W_1c n.y) + W_2c n.z
        inv = F(f32(1.0) / np.sqrt(ir.dot(m, m)))
        out[:, 9:12] = F(m * inv[:, None])
        out[:, 12:15] = l[:, 12:15]
        u, v = out[:, 3:6], out[:, 6:9]
        c = np.stack([F(F(u[:, 1] * v[:, 2]) - F(u[:, 2] * v[:, 1])), F(F(u[:, 2] * v[:, 0]) - F(u[:, 0] * v[:, 2])),
                      F(F(u[:, 0] * v[:, 1]) - F(u[:, 1] * v[:, 0]))], -1)
        out[:, 15] = np.sqrt(ir.dot(c, c))
    return out


def finish_lights(table):
    """np_finish: a_k = area if finite and positive else +0, S = pairwise tree sum, pdf = a_k (1 / S), 0 when S is not positive"""
    t = np.array(table, f32).reshape(-1, 18)
    with np.errstate(all="ignore"):
        a = np.where(np.isfinite(t[:, 15]) & (t[:, 15] > 0), t[:, 15], f32(0)).astype(f32)
        n = 1
        while n < a.shape[0]:
            n *= 2
        s = np.concatenate([a, np.zeros(n - a.shape[0], f32)])
        while s.shape[0] > 1:
            s = F(s[0::2] + s[1::2])
        S = s[0] if a.shape[0] else f32(0)
        t[:, 16] = F(a * F(f32(1.0) / S)) if S > 0 else f32(0)
    return t


class InstancedRef(ir.RefScene):
    """meshes: objects with vertices, normals, texcoords, triangles (object space, source order); matrices (n, 3, 4) object_to_world;
    mesh_of, masks, offsets per instance; materials (m, 16); static_lights (l, 18) world space; mesh_lights: None or per mesh an (l, 18)
    array or None, object space; options: instance_masks, mask_primary, mask_bounce, mask_shadow.  log=True keeps every ray and its answer
    (`rays`) for a comparison with another walk."""

    census_keys = CENSUS_KEYS

    def __init__(self, meshes, matrices, mesh_of, masks, offsets, materials, static_lights, mesh_lights, textures, camera, width, height,
                 options=None, breaks=(), first_order=None, log=False):
        assert set(breaks) <= set(BREAKS), breaks
        self.breaks = frozenset(breaks)
        self.mirror_keeps_is_specular = "mirror_keeps_is_specular" in self.breaks
        opt = {"instance_masks": 0, "mask_primary": 255, "mask_bounce": 255, "mask_shadow": 255, **(options or {})}
        self.masked = bool(opt["instance_masks"])
        self.class_mask = [opt["mask_primary"], opt["mask_bounce"], opt["mask_shadow"]]
        if "shadow_mask_bounce" in self.breaks:
            self.class_mask[2] = opt["mask_bounce"]
        if "bounce_mask_primary" in self.breaks:
            self.class_mask[1] = opt["mask_primary"]
        # ---- the meshes: edges as RefScene has them, normals and texcoords side by side with each mesh's base
        self.geo, rows, N, TC, self.mesh_tri_base = [], [], [], [], []
        n_base = t_base = r_base = 0
        for m in meshes:
            V = F(m.vertices).reshape(-1, 3)
            tri = np.asarray(m.triangles, np.int32).reshape(-1, 12).copy()
            idx = tri[:, :3].astype(np.int64)
            v0 = V[idx[:, 0]]
            self.geo.append((v0, F(V[idx[:, 1]] - v0), F(V[idx[:, 2]] - v0)))
            nn, tc = F(m.normals).reshape(-1, 3), F(m.texcoords).reshape(-1, 2)
            tri[:, 4:7] += np.where(tri[:, 7:8] != 0, n_base, 0).astype(np.int32)          # vn.w == 0: a flat integer normal, no index
            if "vt_without_base" not in self.breaks:
                tri[:, 8:11] += t_base
            self.mesh_tri_base.append(r_base)
            rows.append(tri); N.append(nn); TC.append(tc)
            n_base, t_base, r_base = n_base + nn.shape[0], t_base + tc.shape[0], r_base + tri.shape[0]
        self.tri, self.N, self.TC = np.concatenate(rows), np.concatenate(N), np.concatenate(TC)
        self.mesh_tri_base = np.array(self.mesh_tri_base, np.int64)
        self.mat = F(materials).reshape(-1, 16)
        self.tex = None if textures is None else np.asarray(textures, np.uint8)
        # ---- the instances
        self.M = F(matrices).reshape(-1, 3, 4)
        n = self.M.shape[0]
        self.mesh_of = np.asarray(mesh_of, np.int64).reshape(n)
        self.masks = (np.zeros(n, np.int64) if masks is None else np.asarray(masks, np.int64).reshape(n)) & 0xff
        self.offsets = np.zeros(n, np.int64) if offsets is None else np.asarray(offsets, np.int64).reshape(n)
        self.Wm = np.array([world_to_object(m) for m in self.M], f32).reshape(n, 3, 4)
        self.flag = np.array([is_identity(m) for m in self.M], bool).reshape(n)
        self.mirrored = np.array([np.linalg.det(m[:, :3].astype(f64)) < 0 for m in self.M], bool).reshape(n)
        counts = np.array([self.geo[k][0].shape[0] for k in self.mesh_of], np.int64)
        self.tri_base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)             # hit = tri_base[instance] + id
        self.inst_of_col = np.repeat(np.arange(n), counts)
        # ---- the light table
        static = F(static_lights).reshape(-1, 18)
        self.lit = mesh_lights is not None and any(l is not None and len(l) for l in mesh_lights)
        self.nl = np.zeros(len(meshes), np.int64)
        self.first = np.zeros(n, np.int64)
        self.light_moved = np.zeros(static.shape[0], bool)
        self.light_mirrored = np.zeros(static.shape[0], bool)
        if self.lit:
            ml = [F(l).reshape(-1, 18) if l is not None else np.zeros((0, 18), f32) for l in mesh_lights]
            self.nl = np.array([l.shape[0] for l in ml], np.int64)
            parts, at = [static], static.shape[0]
            for k in range(n):
                l = ml[self.mesh_of[k]]
                self.first[k] = at
                at += l.shape[0]
                parts.append(l.copy() if self.flag[k] else moved_lights(self.M[k], self.Wm[k], l, "light_normal_by_A" in self.breaks))
                self.light_moved = np.concatenate([self.light_moved, np.full(l.shape[0], not self.flag[k])])
                self.light_mirrored = np.concatenate([self.light_mirrored, np.full(l.shape[0], bool(self.mirrored[k]))])
            table = np.concatenate(parts)
            self.lights = table if "pdf_as_given" in self.breaks else finish_lights(table)
            if "first_in_other_order" in self.breaks:                                         # first[] summed in another order of the instances
                at = static.shape[0]
                for k in (range(n - 1, -1, -1) if first_order is None else first_order):
                    self.first[k] = at
                    at += self.nl[self.mesh_of[k]]
        else:
            self.lights = static
        c = camera.c if hasattr(camera, "c") else camera
        self.cam_pos, self.cam_right = F(c.position[:]), F(c.right[:])
        self.cam_up, self.cam_forward = F(c.up[:]), F(c.forward[:])
        self.fov = f32(c.fov)
        self.W, self.H = int(width), int(height)
        self.rays = [] if log else None

    # ---------------------------------------------------------------------------------------- the questions render_frame asks
    def object_rays(self, k, o, d):
        if self.flag[k]:
            return o, d
        return _rows(self.Wm[k], o, True), _rows(self.Wm[k], d, False)

    def _walk(self, o, d, tmax, visible):
        """the minimum of (t, instance, id) over the instances of `visible`: (hit or -1, t, u, v, rays whose best t two instances share)"""
        n, cols = o.shape[0], int(self.tri_base[-1])
        key = np.full((n, max(cols, 1)), np.inf, f32)
        U, V, T = np.zeros_like(key), np.zeros_like(key), np.zeros_like(key)
        tmax = np.broadcast_to(F(tmax), (n,))
        for k in np.nonzero(visible)[0]:
            oo, dd = self.object_rays(k, o, d)
            u, v, t, ok = ir.moller_trumbore(oo, dd, *self.geo[self.mesh_of[k]])
            ok &= np.isfinite(oo).all(1)[:, None] & (t < tmax[:, None])
            sl = slice(self.tri_base[k], self.tri_base[k + 1])
            key[:, sl], U[:, sl], V[:, sl], T[:, sl] = np.where(ok, t, f32(np.inf)), u, v, t
        rows = np.arange(n)
        best = key.min(1) if cols else np.full(n, np.inf, f32)
        found = np.isfinite(best)
        per_inst = np.stack([key[:, self.tri_base[k]:self.tri_base[k + 1]].min(1) if visible[k] else np.full(n, np.inf, f32)
                             for k in range(self.M.shape[0])], 1) if self.M.shape[0] else np.zeros((n, 0), f32)
        shared = found & ((per_inst == best[:, None]).sum(1) >= 2)
        if "ties_to_higher_instance" in self.breaks and cols:
            inst = per_inst.shape[1] - 1 - np.argmin(per_inst[:, ::-1], axis=1)
            k = np.argmin(np.where(self.inst_of_col[None, :] == inst[:, None], key, f32(np.inf)), axis=1)
        else:
            k = np.argmin(key, axis=1)                  # columns run instance by instance, id by id: the first minimum is min (t, instance, id)
        return np.where(found, k, -1), T[rows, k], U[rows, k], V[rows, k], shared

    def visibility(self, cen, ray_class, o, d, tmax):
        with np.errstate(all="ignore"):
            everyone = np.ones(self.M.shape[0], bool)
            visible = (self.masks & self.class_mask[ray_class]) != 0 if self.masked else everyone
            hit, t, u, v, shared = self._walk(o, d, tmax, visible)
            cen["cross_instance_ties"] += int(shared.sum())
            if self.masked:
                plain = self._walk(o, d, tmax, everyone)[0]
                if ray_class == 2:
                    cen["shadow_blocked_only_by_hidden"] += int(((plain >= 0) & (hit < 0)).sum())
                else:
                    cen["mask_changes_" + CLASSES[ray_class]] += int((plain != hit).sum())
        if self.rays is not None:
            inst = self.instance_of(hit)
            self.rays.append(dict(ray_class=ray_class, o=o.copy(), d=d.copy(), tmax=np.broadcast_to(F(tmax), (o.shape[0],)).copy(), t=t, u=u, v=v,
                                  instance=np.where(hit >= 0, inst, -1), tri=np.where(hit >= 0, hit - self.tri_base[inst], -1)))
        return hit, t, u, v

    def instance_of(self, hit):
        return np.clip(np.searchsorted(self.tri_base, hit, side="right") - 1, 0, max(self.M.shape[0] - 1, 0))

    def hit_rows(self, cen, ray_class, hit):
        inst = self.instance_of(hit)
        row = self.tri[self.mesh_tri_base[self.mesh_of[inst]] + (hit - self.tri_base[inst])]
        c = CLASSES[ray_class]
        cen["hits_identity_" + c] += int(self.flag[inst].sum())
        cen["hits_general_" + c] += int((~self.flag[inst] & ~self.mirrored[inst]).sum())
        cen["hits_mirrored_" + c] += int(self.mirrored[inst].sum())
        cen["hits_with_offset"] += int((self.offsets[inst] != 0).sum())
        return row, row[:, 3] + self.offsets[inst]

    def world_normal(self, n_obj, hit):
        inst = self.instance_of(hit)
        W = self.Wm[inst]
        with np.errstate(all="ignore"):
            m = np.stack([F(F(F(W[:, 0, c] * n_obj[:, 0]) + F(W[:, 1, c] * n_obj[:, 1])) + F(W[:, 2, c] * n_obj[:, 2])) for c in range(3)], -1)
            lm = ir.length(m)
            scale = F(f32(1.0) / lm) if "unit_normal" in self.breaks else F(ir.length(n_obj) / lm)
            n = np.where(((lm == 0) | ~np.isfinite(lm))[:, None], m, F(m * scale[:, None]))
        return np.where(self.flag[inst][:, None], n_obj, n).astype(f32)

    def shading_ray(self, o, d, hit):
        if "hit_point_object_ray" not in self.breaks:
            return o, d
        inst = self.instance_of(hit)
        oo, dd = o.copy(), d.copy()
        for k in np.unique(inst):
            sel = inst == k
            oo[sel], dd[sel] = self.object_rays(k, o[sel], d[sel])
        return oo, dd

    def emitter_light(self, cen, ew, hit):
        ew = ew.astype(np.int64)
        if not self.lit:
            return self.lights[ew, 15:18], np.ones(ew.shape[0], bool)
        total = self.lights.shape[0]
        if total == 0:
            cen["emitter_empty_table"] += int(ew.shape[0])
            if "empty_table_prev_pdf" in self.breaks:
                return np.ones((ew.shape[0], 3), f32), np.ones(ew.shape[0], bool)
            return np.zeros((ew.shape[0], 3), f32), np.zeros(ew.shape[0], bool)
        inst = self.instance_of(hit)
        nl = self.nl[self.mesh_of[inst]]
        own = nl > 0
        cen["emitter_after_bounce_clamped"] += int((own & (ew > nl - 1)).sum())
        cen["emitter_after_bounce_unclamped"] += int((own & (ew <= nl - 1)).sum())
        cen["emitter_after_bounce_lightless_mesh"] += int((~own).sum())
        local = np.minimum(ew, nl if "clamp_nl" in self.breaks else nl - 1)
        other = np.minimum(ew, total - 1)
        if "lightless_uses_first" in self.breaks:
            other = self.first[inst] + other
        li = np.where(own, self.first[inst] + local, other)
        return self.lights[np.minimum(li, total - 1), 15:18], np.ones(ew.shape[0], bool)

    def note(self, cen, what, hit):
        if what == "nee_light":
            if self.lit:
                cen["nee_moved_light"] += int(self.light_moved[hit].sum())
                cen["nee_mirrored_lamp_light"] += int(self.light_mirrored[hit].sum())
            return
        inst = self.instance_of(hit)
        if what == "textured":
            cen["textured_through_offset"] += int((self.offsets[inst] != 0).sum())
        elif what == "mirror":
            cen["mirror_on_general"] += int((~self.flag[inst]).sum())
