"""A numpy restatement of the environment (crt_set_environment), written from include/crt.h on top of
tests/integrator_ref.py's helpers — not from rt_kernels.hip, and importing nothing from oracle/.  The C oracle has no environment: frames
with one are held to numpy alone.

`radiance(env, d)` is E(d), every step ONE float32 IEEE operation in the header's order:

  e    = (R[0].d, R[1].d, R[2].d)           each (r0 d.x + r1 d.y) + r2 d.z
  s    = (|e.x| + |e.y|) + |e.z|            not (s > 0) or s not finite: 0
  px   = e.x / s, py = e.y / s;   e.z < 0: (px, py) = ((1 - |py|) sgn(px), (1 - |px|) sgn(py)) from the old pair, sgn(x) = x < 0 ? -1 : 1
  fx   = (px 0.5 + 0.5) size - 0.5, fy likewise;  i0 = floor(fx), tx = fx - i0, j0 = floor(fy), ty = fy - j0
  tap(i, j) with the octahedral edge identification, then clamped
  c    = (tap(i0,j0) (1 - tx) + tap(i1,j0) tx) (1 - ty) + (tap(i0,j1) (1 - tx) + tap(i1,j1) tx) ty
  E    = c scale

`render_frame` is integrator_ref.render_frame's loop, copied line for line, with two changes: the primary rays come from `primary`, and the
miss line adds T * E(d) to the paths that leave the scene (not at segment 0 when env.hide_from_camera).  integrator_ref.render_frame exposes
neither T nor the path ids at its miss line, hence the copy; tests/test_environment.py holds it to integrator_ref.render by bits with
env = None on every scene it is used on, which is what keeps the copy from drifting."""
import numpy as np

import integrator_ref as ir
from integrator_ref import (F, MIRROR_TYPE, _EPS, _INF, _PI, _PI2, _interp, _pow_double_once, dot, f32, f64, length, normalize, pinned_cos,
                            pinned_sin)


class Env:
    """texels (size, size, 3) float32, row 0 first; rotation: 3 x 3, rows, world -> map; scale: RGB; hide_from_camera"""

    def __init__(self, texels, rotation=None, scale=(1.0, 1.0, 1.0), hide_from_camera=False):
        self.texels = np.ascontiguousarray(texels, f32)
        assert self.texels.ndim == 3 and self.texels.shape[0] == self.texels.shape[1] and self.texels.shape[2] == 3
        self.size = int(self.texels.shape[0])
        self.rotation = np.eye(3, dtype=f32) if rotation is None else np.ascontiguousarray(rotation, f32).reshape(3, 3)
        self.scale = F(scale).reshape(3)
        self.hide_from_camera = bool(hide_from_camera)


def _tap(env, i, j, clamp_only=False):
    m = env.size - 1
    i, j = i.copy(), j.copy()
    if not clamp_only:
        lo, hi = i < 0, i > m
        j = np.where(lo | hi, m - j, j)
        i = np.where(lo, 0, np.where(hi, m, i))
        lo, hi = j < 0, j > m
        i = np.where(lo | hi, m - i, i)
        j = np.where(lo, 0, np.where(hi, m, j))
    i, j = np.clip(i, 0, m), np.clip(j, 0, m)
    return env.texels[j, i]


def radiance(env, d, clamp_only=False):
    """E(d) for directions (n, 3) -> (n, 3) float32.  clamp_only drops the edge identification (a deliberate mistake for the tests)."""
    d = F(d).reshape(-1, 3)
    R = env.rotation
    with np.errstate(all="ignore"):
        e = np.stack([F(F(F(R[k, 0] * d[:, 0]) + F(R[k, 1] * d[:, 1])) + F(R[k, 2] * d[:, 2])) for k in range(3)], -1)
        s = F(F(np.abs(e[:, 0]) + np.abs(e[:, 1])) + np.abs(e[:, 2]))
        ok = (s > 0) & np.isfinite(s)
        ss = np.where(ok, s, f32(1.0)).astype(f32)
        ee = np.where(ok[:, None], e, f32(0.0)).astype(f32)
        px, py = F(ee[:, 0] / ss), F(ee[:, 1] / ss)
        sgn = lambda x: np.where(x < 0, f32(-1.0), f32(1.0)).astype(f32)
        qx = F(F(f32(1.0) - np.abs(py)) * sgn(px))
        qy = F(F(f32(1.0) - np.abs(px)) * sgn(py))
        low = ee[:, 2] < 0
        px, py = np.where(low, qx, px).astype(f32), np.where(low, qy, py).astype(f32)
        size = f32(env.size)
        fx = F(F(F(F(px * f32(0.5)) + f32(0.5)) * size) - f32(0.5))
        fy = F(F(F(F(py * f32(0.5)) + f32(0.5)) * size) - f32(0.5))
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = F(fx - x0)[:, None], F(fy - y0)[:, None]
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        ux, uy = F(f32(1.0) - tx), F(f32(1.0) - ty)
        t = lambda i, j: _tap(env, i, j, clamp_only)
        bot = F(F(t(i0, j0) * ux) + F(t(i0 + 1, j0) * tx))
        top = F(F(t(i0, j0 + 1) * ux) + F(t(i0 + 1, j0 + 1) * tx))
        c = F(F(bot * uy) + F(top * ty))
        E = F(c * env.scale[None, :])
    return np.where(ok[:, None], E, f32(0.0)).astype(f32)


def render_frame(scene, rx, ry, max_depth, env=None, primary=None):
    """integrator_ref.render_frame with the primary rays from `primary(scene, rx, ry)` (default: integrator_ref.primary_rays, jitter on) and
    the miss line of the module docstring.  The same two return values."""
    o, d, rng, jc = ir.primary_rays(scene, rx, ry, jitter=True) if primary is None else primary(scene, rx, ry)
    n = o.shape[0]
    n_lights = scene.lights.shape[0]
    L = np.zeros((n, 3), f32)
    T = np.ones((n, 3), f32)
    prev_pdf = np.ones(n, f32)
    is_specular = np.ones(n, bool)
    alive = np.ones(n, bool)
    bounced = np.zeros(n, bool)
    cen = {k: 0 for k in ir.CENSUS_KEYS + tuple(scene.census_keys)}
    cen.update(jc)
    frames, censuses = [], []
    with np.errstate(all="ignore"):
        for seg in range(max_depth):
            ids = np.nonzero(alive)[0]
            cen["closest_rays"] += int(ids.size)
            tri, t, u, v = scene.visibility(cen, min(seg, 1), o[ids], d[ids], _INF)
            miss = tri < 0
            cen["miss_first" if seg == 0 else "miss_later"] += int(miss.sum())
            alive[ids[miss]] = False
            if env is not None and not (seg == 0 and env.hide_from_camera):                    # the one added line: L += T * E(d), and the path ends
                L[ids[miss]] = F(L[ids[miss]] + F(T[ids[miss]] * radiance(env, d[ids[miss]])))
            ids, tri, t, u, v = ids[~miss], tri[~miss], t[~miss], u[~miss], v[~miss]
            ro, rd = o[ids], d[ids]
            row, mtl = scene.hit_rows(cen, min(seg, 1), tri)
            flat = row[:, 7] == 0
            nrm = np.where(flat[:, None], row[:, 4:7].astype(f32),
                           _interp(scene.N[np.where(flat, 0, row[:, 4])], scene.N[np.where(flat, 0, row[:, 5])],
                                   scene.N[np.where(flat, 0, row[:, 6])], u, v) if scene.N.shape[0] else row[:, 4:7].astype(f32)).astype(f32)
            nrm = scene.world_normal(nrm, tri)
            cen["flat_normal_hit"] += int(flat.sum())
            cen["non_unit_normal_hit"] += int((np.abs(dot(nrm, nrm).astype(f64) - 1.0) > 1e-3).sum())
            m = scene.mat[mtl]
            albedo, emission, specular, tex_ind = m[:, 0:4].copy(), m[:, 4:8], m[:, 8:12], m[:, 12:16]
            textured = (tex_ind[:, 0] != f32(-1.0)) & (scene.tex is not None) & (scene.TC.shape[0] > 0)
            if textured.any():
                k = np.nonzero(textured)[0]
                r = row[k]
                tc = _interp(scene.TC[r[:, 8]], scene.TC[r[:, 9]], scene.TC[r[:, 10]], u[k], v[k])
                c = scene.sample_albedo(tc[:, 0], tc[:, 1], tex_ind[k, 0].astype(np.int64))
                albedo[k, 0:3] = _pow_double_once(c, 2.2)
            cen["textured_hit"] += int(textured.sum())
            scene.note(cen, "textured", tri[textured])
            original_n = nrm
            cos_incident = dot(rd, nrm)
            flipped = cos_incident > 0
            nrm = np.where(flipped[:, None], -nrm, nrm).astype(f32)
            emit = emission[:, 3] != f32(-1.0)
            spec_here = is_specular[ids]
            e1 = emit & spec_here
            L[ids[e1]] = F(L[ids[e1]] + F(T[ids[e1]] * emission[e1, 0:3]))
            cen["emitter_direct" if seg == 0 else "emitter_through_mirror"] += int(e1.sum())
            cen["emitter_through_mirror_after_bounce"] += int((e1 & bounced[ids]).sum())
            e2 = emit & ~spec_here
            if e2.any():
                k = np.nonzero(e2)[0]
                ld = F(rd[k] * t[k, None])
                ln = length(ld)
                ld = normalize(ld)
                cos_light = F(f32(-1.0) * dot(ld, nrm[k]))
                length2 = F(ln * ln)
                ap, weighed = scene.emitter_light(cen, emission[k, 3], tri[k])
                pdf_light = F(F(length2 / F(ap[:, 0] * cos_light)) * ap[:, 1])
                a2 = F(prev_pdf[ids[k]] * prev_pdf[ids[k]])
                mis = np.where(weighed, F(a2 / F(F(pdf_light * pdf_light) + a2)), f32(1.0)).astype(f32)
                L[ids[k]] = F(L[ids[k]] + F(F(T[ids[k]] * emission[k, 0:3]) * mis[:, None]))
                cen["emitter_cos_light_le_0"] += int((~(cos_light > 0)).sum())
                cen["emitter_after_bounce_front"] += int(((cos_light > 0) & ~flipped[k]).sum())
                cen["emitter_after_bounce_back"] += int(((cos_light > 0) & flipped[k]).sum())
            alive[ids[emit]] = False
            keep = ~emit
            ids, t, tri = ids[keep], t[keep], tri[keep]
            ro, rd = scene.shading_ray(ro[keep], rd[keep], tri)
            nrm, original_n, albedo, specular = nrm[keep], original_n[keep], albedo[keep], specular[keep]
            hit_point = F(F(ro + F(rd * t[:, None])) + F(nrm * f32(0.0002)))
            mirror = albedo[:, 3] == MIRROR_TYPE
            cen["mirror_hit"] += int(mirror.sum())
            scene.note(cen, "mirror", tri[mirror])
            nee = (specular[:, 3] == f32(0.0)) & ~mirror
            k = np.nonzero(nee)[0]
            gk = ids[k]
            r0 = rng.draw(gk)
            r1 = rng.draw(gk)
            r2 = rng.draw(gk)
            if n_lights > 0 and k.size:
                li = F(r0 * f32(n_lights)).astype(np.int64)
                cen["light_index_clamped"] += int((li > n_lights - 1).sum())
                li = np.minimum(li, n_lights - 1)
                scene.note(cen, "nee_light", li)
                lt = scene.lights[li]
                s = np.sqrt(r1)
                b0 = F(f32(1.0) - s)
                b1 = F(r2 * s)
                pos = F(F(lt[:, 0:3] + F(b0[:, None] * lt[:, 3:6])) + F(b1[:, None] * lt[:, 6:9]))
                ld = F(pos - hit_point[k])
                ln = length(ld)
                iln = F(f32(1.0) / ln)
                ld = F(ld * iln[:, None])
                cos_mtl = dot(ld, original_n[k])
                cos_light = dot(ld, lt[:, 9:12])
                ok_mtl, ok_light = cos_mtl > 0, cos_light < 0
                cen["nee_refused_cos_mtl"] += int((~ok_mtl).sum())
                cen["nee_refused_cos_mtl_flipped_accepts"] += int((~ok_mtl & (dot(ld, nrm[k]) > 0)).sum())
                cen["nee_refused_cos_light"] += int((ok_mtl & ~ok_light).sum())
                sh = np.nonzero(ok_mtl & ok_light)[0]
                cen["shadow_rays"] += int(sh.size)
                if sh.size:
                    ks = k[sh]
                    blocked = scene.visibility(cen, 2, hit_point[ks], ld[sh], F(ln[sh] - _EPS))[0] >= 0
                    cen["shadow_occluded"] += int(blocked.sum())
                    cen["shadow_clear"] += int((~blocked).sum())
                    c = sh[~blocked]
                    kc = k[c]
                    ap = lt[c, 15:18]
                    pdf_light = F(F(F(ln[c] * ln[c]) / F(ap[:, 0] * -cos_light[c])) * ap[:, 1])
                    bsdf_pdf = F(F(dot(ld[c], nrm[kc]) * f32(1.0)) / _PI)
                    a2 = F(pdf_light * pdf_light)
                    mis = F(a2 / F(F(bsdf_pdf * bsdf_pdf) + a2))
                    contrib = F(F(F(F(T[ids[kc]] * lt[c, 12:15]) * albedo[kc, 0:3]) * mis[:, None]) / pdf_light[:, None])
                    L[ids[kc]] = F(L[ids[kc]] + contrib)
            if mirror.any():
                k = np.nonzero(mirror)[0]
                nn = normalize(nrm[k])
                dn = dot(rd[k], nn)
                refl = F(rd[k] - F(nn * F(f32(2.0) * dn)[:, None]))
                T[ids[k]] = F(T[ids[k]] * albedo[k, 0:3])
                if not scene.mirror_keeps_is_specular:
                    is_specular[ids[k]] = True
                o[ids[k]], d[ids[k]] = hit_point[k], refl
            k = np.nonzero(~mirror)[0]
            gk = ids[k]
            nk = nrm[k]
            sing = nk[:, 2] < f32(-0.9999999)
            cen["onb_singular"] += int(sing.sum())
            cen["onb_regular"] += int((~sing).sum())
            a = F(f32(1.0) / F(f32(1.0) + nk[:, 2]))
            b = F(F(-nk[:, 0] * nk[:, 1]) * a)
            bu = np.stack([F(f32(1.0) + b), b, -nk[:, 0]], -1)
            bv = np.stack([b, F(f32(1.0) + b), -nk[:, 1]], -1)
            bu[sing], bv[sing] = F([0.0, -1.0, 0.0]), F([-1.0, 0.0, 0.0])
            u1 = rng.draw(gk)
            u2 = rng.draw(gk)
            rr = np.sqrt(u1)
            phi = F(_PI2 * u2)
            sx, sy, sz = F(rr * pinned_cos(phi)), F(rr * pinned_sin(phi)), np.sqrt(F(f32(1.0) - u1))
            sd = F(F(F(bu * sx[:, None]) + F(bv * sy[:, None])) + F(nk * sz[:, None]))
            prev_pdf[gk] = F(F(dot(sd, nk) * f32(1.0)) / _PI)
            T[gk] = F(T[gk] * albedo[k, 0:3])
            is_specular[gk] = False
            bounced[gk] = True
            o[gk], d[gk] = hit_point[k], sd
            frames.append(L.reshape(scene.H, scene.W, 3).copy())
            censuses.append(dict(cen))
    return frames, censuses


def render(scene, rvs, max_depth, env, primary=None):
    """integrator_ref.render with an environment: the same four return values"""
    sums = [np.zeros((scene.H, scene.W, 3), f32) for _ in range(max_depth)]
    radiance_, census = [], []
    for rx, ry in rvs:
        frames, cens = render_frame(scene, rx, ry, max_depth, env, primary)
        radiance_.append(frames)
        census.append(cens)
        for k in range(max_depth):
            sums[k] = F(frames[k] + sums[k])
    total = [{key: sum(c[k][key] for c in census) for key in census[0][k]} for k in range(max_depth)]
    return sums, radiance_, total, census
