"""A numpy restatement of the frame path's integrator, written from Shader/path_trace.fs and the floating-point rules of DESIGN.md §3
— not from oracle/oracle.c, and importing nothing from oracle/ — so that the HIP kernel (`k_segment` and its shell) and the C oracle are
both held to a third reading of the shader (DESIGN.md "The integrator as tested").

Every arithmetic step is ONE float32 IEEE operation on numpy arrays, vectorised over pixels; nothing is fused.  The line numbers cite
Shader/path_trace.fs.  What GLSL leaves to the implementation is fixed as DESIGN.md fixes it:

  dot        (x x' + y y') + z z'
  normalize  v * (1 / sqrt(dot(v, v))), `/` and sqrt correctly rounded
  sin, cos   the pinned sequence: Cody-Waite reduction by pi with three fused multiply-adds in double, a Taylor polynomial whose two highest
             coefficients meet by a multiply and an add and whose remaining Horner steps are fused, one rounding to float32.  numpy has no
             fma, so `fma` below builds an exact one from error-free transformations (tested against fractions.Fraction).
  tan(fov/2) once per frame, the host's float tanf
  texture    GL_LINEAR / GL_REPEAT on RGB8: texel = c / 255, x = u W - 0.5, i0 = floor(x), f = x - i0, indices modulo the size,
             top = t00 (1 - fx) + t10 fx, bot likewise on the next row, result = top (1 - fy) + bot fy
  pow        pow(c, 2.2f) and the resolve's pow(x, 1 / 2.2f) in double (libm), rounded once to float32
  visibility brute force over all triangles: nearest t, equal t to the lowest original id; a shadow ray is blocked by any triangle with
             t < length - eps (hit_shadow, :376-412 and :968)

Scope: Lambert, emissive, textured and Mirror materials.  Disney materials have no shader text and are not restated here.  `render_frame`
asks the scene five questions (RefScene.visibility, hit_rows, world_normal, emitter_light, and its light table); RefScene answers them for
a flat scene, tests/instanced_ref.py for an instanced one, so that one loop serves both.
"""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
f64 = np.float64


def F(x):
    return np.asarray(x, dtype=f32)


# ------------------------------------------------------------------------------------------------ an exact double fma

_SPLIT = f64(134217729.0)          # 2^27 + 1 (Veltkamp)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_to_odd(a, b):
    """a + b rounded to odd: the exact sum when it is a double, else the neighbour whose last mantissa bit is 1."""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    # s is the nearest double and even; the odd neighbour lies on e's side.  Stepping the bit pattern by +-1 moves away from / towards zero.
    away = (e > 0) == (s > 0)
    step = np.where(away, 1, -1).astype(np.int64)
    # s == 0 with e != 0 cannot happen: a sum that rounds to zero is exact
    out = np.where(fix, bits + step, bits)
    return out.view(f64)


def fma(a, b, c):
    """a * b + c with ONE rounding (IEEE 754 fusedMultiplyAdd) for float64 arrays, exact wherever the product's error term is representable
    (|a b| well inside 2^-960 .. 2^1000: everything the pinned sine meets).  Boldo-Melquiond: Dekker's two-product, two-sum with c, the two
    small parts added with round-to-odd, one final rounded addition."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f64), np.asarray(b, f64), np.asarray(c, f64))
    a, b, c = a.copy(), b.copy(), c.copy()
    with np.errstate(all="ignore"):
        ph, pl = _two_prod(a, b)
        sh, sl = _two_sum(c, ph)
        v = _add_round_to_odd(sl, pl)
        return sh + v


# ------------------------------------------------------------------------------------------------ pinned sine and cosine

_PI_1, _PI_2, _PI_3 = float.fromhex("0x1.921fb544p+1"), float.fromhex("0x1.0b4611a6p-33"), float.fromhex("0x1.3198a2ep-68")
_INV_PI = float.fromhex("0x1.45f306dc9c883p-2")
_SIN_C = [1.0 / 51090942171709440000.0, -1.0 / 121645100408832000.0, 1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0,
          -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0]
_COS_C = [1.0 / 1124000727777607680000.0, -1.0 / 2432902008176640000.0, 1.0 / 6402373705728000.0, -1.0 / 20922789888000.0,
          1.0 / 87178291200.0, -1.0 / 479001600.0, 1.0 / 3628800.0, -1.0 / 40320.0, 1.0 / 720.0, -1.0 / 24.0, 0.5]


def _reduce_pi(x):
    k = np.rint(x * f64(_INV_PI))
    r = fma(k, -_PI_3, fma(k, -_PI_2, fma(k, -_PI_1, x)))
    return k, r


def _horner(z, coef):
    p = z * f64(coef[0]) + f64(coef[1])
    for c in coef[2:]:
        p = fma(p, z, c)
    return p


def pinned_sin(xf):
    x = np.atleast_1d(F(xf)).astype(f64)
    ok = np.abs(x) < 1e9
    xs = np.where(ok, x, 0.0)
    k, r = _reduce_pi(xs)
    z = r * r
    s = fma(r * z, _horner(z, _SIN_C), r)
    s = np.where((k.astype(np.int64) & 1) == 1, -s, s)
    return np.where(ok, s.astype(f32), f32(0.0)).astype(f32)


def pinned_cos(xf):
    x = np.atleast_1d(F(xf)).astype(f64)
    ok = np.abs(x) < 1e9
    xs = np.where(ok, x, 0.0)
    k, r = _reduce_pi(xs)
    z = r * r
    c = fma(-z, _horner(z, _COS_C), 1.0)
    c = np.where((k.astype(np.int64) & 1) == 1, -c, c)
    return np.where(ok, c.astype(f32), f32(1.0)).astype(f32)


# ------------------------------------------------------------------------------------------------ small vector helpers

def dot(a, b):
    return F(F(a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def length(a):
    return np.sqrt(dot(a, a))


def normalize(a):
    inv = f32(1.0) / np.sqrt(dot(a, a))
    return F(a * inv[..., None])


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]


def _pow_double_once(x, e):
    """float32(pow(double(x), double(e))) per element through libm (math.pow), so that no vector library's pow stands in."""
    x = F(x)
    e = float(f32(e))
    flat = x.reshape(-1)
    out = np.empty(flat.shape, f32)
    for i, v in enumerate(flat.tolist()):
        try:
            out[i] = f32(math.pow(v, e))
        except (ValueError, OverflowError):
            out[i] = f32(np.nan) if (v < 0 or v != v) else f32(np.inf)
    return out.reshape(x.shape)


# ------------------------------------------------------------------------------------------------ the scene as the shader sees it

def moller_trumbore(o, d, v0, e1, e2):
    """:322-374 for rays (n, 3) against triangles (m, 3): (u, v, t, accepted) as (n, m) arrays, the bound on t left to the caller"""
    oo, dd = o[:, None, :], d[:, None, :]
    v0, e1, e2 = v0[None], e1[None], e2[None]
    pv = cross(np.broadcast_to(dd, (dd.shape[0],) + e2.shape[1:]), e2)
    tv = F(oo - v0)
    qv = cross(tv, e1)
    u, v, t = dot(tv, pv), dot(dd, qv), dot(e2, qv)
    inv = F(f32(1.0) / dot(e1, pv))
    u, v, t = F(u * inv), F(v * inv), F(t * inv)
    w = F(F(f32(1.0) - u) - v)
    return u, v, t, (u >= 0) & (v >= 0) & (t >= 0) & (w >= 0)


class RefScene:
    """The arrays of a Mesh (source triangle order: a triangle's index is its original id) and a camera."""

    def __init__(self, mesh, camera, width, height, lights=None, albedo_textures=None):
        self.V = F(mesh.vertices).reshape(-1, 3)
        self.N = F(mesh.normals).reshape(-1, 3)
        self.TC = F(mesh.texcoords).reshape(-1, 2)
        self.tri = np.asarray(mesh.triangles, np.int32).reshape(-1, 12)
        self.mat = F(mesh.materials).reshape(-1, 16)
        self.lights = F(mesh.lights if lights is None else lights).reshape(-1, 18)
        tex = albedo_textures if albedo_textures is not None else getattr(mesh, "albedo_textures", None)
        self.tex = None if tex is None else np.asarray(tex, np.uint8)
        c = camera.c if hasattr(camera, "c") else camera
        self.cam_pos, self.cam_right = F(c.position[:]), F(c.right[:])
        self.cam_up, self.cam_forward = F(c.up[:]), F(c.forward[:])
        self.fov = f32(c.fov)
        self.W, self.H = int(width), int(height)
        idx = self.tri[:, :3].astype(np.int64)
        self.v0 = self.V[idx[:, 0]]
        self.e1 = F(self.V[idx[:, 1]] - self.v0)                 # :337-338
        self.e2 = F(self.V[idx[:, 2]] - self.v0)

    # -- :322-374 over all triangles.  Returns (tri, t, u, v); tri = -1 where nothing is hit below tmax.
    def closest(self, o, d, tmax, chunk=512):
        n = o.shape[0]
        tri = np.full(n, -1, np.int64)
        tt, uu, vv = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
        tmax = np.broadcast_to(F(tmax), (n,))
        with np.errstate(all="ignore"):
            for a in range(0, n, chunk):
                sl = slice(a, min(n, a + chunk))
                u, v, t, ok = moller_trumbore(o[sl], d[sl], self.v0, self.e1, self.e2)
                ok &= t < tmax[sl, None]
                key = np.where(ok, t, f32(np.inf))
                k = np.argmin(key, axis=1)                      # the first index of the minimum: the lowest id among equal t
                rows = np.arange(k.shape[0])
                hit = ok[rows, k]
                tri[sl] = np.where(hit, k, -1)
                tt[sl], uu[sl], vv[sl] = t[rows, k], u[rows, k], v[rows, k]
        return tri, tt, uu, vv

    # -- what render_frame asks of a scene; tests/instanced_ref.py answers the same questions for an instanced scene.  `hit` is what
    #    visibility returned: here a triangle's id.  ray_class: 0 the path rays of segment 0, 1 those of later segments, 2 shadow rays.
    census_keys = ()
    # True is a deliberate mistake, break 13 of tests/test_instanced_ref.py's sensitivity table (DESIGN.md "Instanced frames as tested"): a
    # Mirror hit then leaves is_specular as it was, which this module did until that section.  Nothing in the flat tests sets it.
    mirror_keeps_is_specular = False

    def visibility(self, cen, ray_class, o, d, tmax):
        return self.closest(o, d, tmax)

    def hit_rows(self, cen, ray_class, hit):
        """-> (the hit triangles' rows, vn / vt indexing self.N / self.TC; their material indices)"""
        row = self.tri[hit]
        return row, row[:, 3]

    def world_normal(self, n_obj, hit):
        return n_obj

    def shading_ray(self, o, d, hit):
        return o, d

    def emitter_light(self, cen, ew, hit):
        """-> (area_pdf rows of the lights an emitter hit names, False where there is no light to weigh against: MIS weight 1)"""
        return self.lights[ew.astype(np.int64), 15:18], np.ones(ew.shape[0], bool)

    def note(self, cen, what, hit):
        pass

    # -- texture(albedo_textures, vec3(uv, layer)).xyz, the filter as the module docstring defines it
    def sample_albedo(self, u, v, layer):
        L, H, W, _ = self.tex.shape
        layer = np.clip(layer, 0, L - 1)
        x = F(F(u * f32(W)) - f32(0.5))
        y = F(F(v * f32(H)) - f32(0.5))
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = F(x - x0), F(y - y0)
        i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
        i1, j1 = (i0 + 1) % W, (j0 + 1) % H
        i0, j0 = i0 % W, j0 % H
        t = lambda j, i: F(self.tex[layer, j, i].astype(f32) / f32(255.0))
        gx, gy = F(f32(1.0) - fx)[:, None], F(f32(1.0) - fy)[:, None]
        fx, fy = fx[:, None], fy[:, None]
        top = F(F(t(j0, i0) * gx) + F(t(j0, i1) * fx))
        bot = F(F(t(j1, i0) * gx) + F(t(j1, i1) * fx))
        return F(F(top * gy) + F(bot * fy))


def _interp(a, b, c, u, v):
    """:312-320: a * (1 - u - v) + b * u + c * v, left to right"""
    w = F(F(f32(1.0) - u) - v)[:, None]
    return F(F(F(a * w) + F(b * u[:, None])) + F(c * v[:, None]))


# ------------------------------------------------------------------------------------------------ :38-42

class _Rng:
    def __init__(self, sx, sy, rx, ry):
        self.sx, self.sy = F(sx).copy(), F(sy).copy()
        self.rv = F(f32(rx) * f32(ry))

    def draw(self, mask):
        """one rand() for the pixels of `mask` (the others keep their seed); returns the values at those pixels"""
        self.sx[mask] = F(self.sx[mask] - self.rv)
        self.sy[mask] = F(self.sy[mask] - self.rv)
        d = F(F(self.sx[mask] * f32(12.9898)) + F(self.sy[mask] * f32(78.233)))
        v = F(pinned_sin(d) * f32(43758.5453))
        return F(v - np.floor(v))


def _jitter(r):
    """:1035-1036"""
    with np.errstate(invalid="ignore"):
        lo = F(np.sqrt(r) - f32(1.0))
        hi = F(f32(1.0) - np.sqrt(F(f32(2.0) - r)))
    return np.where(r < f32(1.0), lo, hi).astype(f32)


def primary_rays(scene, rx, ry, jitter=True):
    """:1026-1047 for every pixel, row py = gl_FragCoord.y - 0.5 first.  Returns (origins, directions, rng, census of the jitter arms)."""
    W, H = scene.W, scene.H
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx = F(px.reshape(-1).astype(f32) + f32(0.5))
    fy = F(py.reshape(-1).astype(f32) + f32(0.5))
    rng = _Rng(fx, fy, rx, ry)
    n = fx.shape[0]
    everyone = np.ones(n, bool)
    census = {}
    tex_x, tex_y = F(fx / f32(W)), F(fy / f32(H))                 # the quad's texCoords interpolated: gl_FragCoord / resolution
    dx = F(F(f32(2.0) * tex_x) - f32(1.0))
    dy = F(F(f32(2.0) * tex_y) - f32(1.0))
    if jitter:
        r1 = F(f32(2.0) * rng.draw(everyone))
        r2 = F(f32(2.0) * rng.draw(everyone))
        census = {"jitter_x_low": int((r1 < 1).sum()), "jitter_x_high": int((r1 >= 1).sum()),
                  "jitter_y_low": int((r2 < 1).sum()), "jitter_y_high": int((r2 >= 1).sum())}
        jx = F(_jitter(r1) / F(f32(W) * f32(0.5)))
        jy = F(_jitter(r2) / F(f32(H) * f32(0.5)))
        dx, dy = F(dx + jx), F(dy + jy)
    tan_fov = f32(_libm.tanf(float(F(scene.fov * f32(0.5)))))
    dx = F(dx * F(F(f32(W) / f32(H)) * tan_fov))
    dy = F(dy * tan_fov)
    v = F(F(F(dx[:, None] * scene.cam_right) + F(dy[:, None] * scene.cam_up)) + scene.cam_forward)
    d = normalize(v)
    o = np.broadcast_to(scene.cam_pos, d.shape).astype(f32)
    return o, d, rng, census


# ------------------------------------------------------------------------------------------------ :857-1024

CENSUS_KEYS = ("closest_rays", "shadow_rays", "jitter_x_low", "jitter_x_high", "jitter_y_low", "jitter_y_high", "miss_first", "miss_later",
               "emitter_direct", "emitter_through_mirror", "emitter_through_mirror_after_bounce", "emitter_after_bounce_front", "emitter_after_bounce_back",
               "emitter_cos_light_le_0", "nee_refused_cos_mtl_flipped_accepts", "nee_refused_cos_mtl", "nee_refused_cos_light",
               "shadow_occluded", "shadow_clear", "flat_normal_hit", "non_unit_normal_hit", "mirror_hit", "textured_hit",
               "onb_singular", "onb_regular", "light_index_clamped")

_EPS = f32(1e-4)
_INF = f32(1e9)
_PI = f32(3.1415926)
_PI2 = f32(6.2831853)
MIRROR_TYPE = f32(1.0)


def render_frame(scene, rx, ry, max_depth):
    """One sample per pixel.  Returns (radiance[max_depth], census[max_depth]): radiance[k - 1] is the (H, W, 3) float32 frame of a path cut
    at k segments — the loop of :867 with bound k returns exactly the L it holds after k passes — and census[k - 1] counts, over that
    frame, the pixel-samples that took each branch (CENSUS_KEYS)."""
    o, d, rng, jc = primary_rays(scene, rx, ry, jitter=True)
    n = o.shape[0]
    n_lights = scene.lights.shape[0]
    L = np.zeros((n, 3), f32)
    T = np.ones((n, 3), f32)
    prev_pdf = np.ones(n, f32)
    is_specular = np.ones(n, bool)
    alive = np.ones(n, bool)
    bounced = np.zeros(n, bool)                                                                # census only: the path has left a diffuse surface
    cen = {k: 0 for k in CENSUS_KEYS + tuple(scene.census_keys)}
    cen.update(jc)
    frames, censuses = [], []
    with np.errstate(all="ignore"):
        for seg in range(max_depth):
            ids = np.nonzero(alive)[0]
            cen["closest_rays"] += int(ids.size)
            tri, t, u, v = scene.visibility(cen, min(seg, 1), o[ids], d[ids], _INF)
            miss = tri < 0
            cen["miss_first" if seg == 0 else "miss_later"] += int(miss.sum())
            alive[ids[miss]] = False                                                        # :1020-1021
            ids, tri, t, u, v = ids[~miss], tri[~miss], t[~miss], u[~miss], v[~miss]
            ro, rd = o[ids], d[ids]
            # ---- :414-489
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
                albedo[k, 0:3] = _pow_double_once(c, 2.2)                                      # :482
            cen["textured_hit"] += int(textured.sum())
            scene.note(cen, "textured", tri[textured])
            # ---- :872-877
            original_n = nrm
            cos_incident = dot(rd, nrm)
            flipped = cos_incident > 0
            nrm = np.where(flipped[:, None], -nrm, nrm).astype(f32)
            # ---- :894-928
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
                mis = np.where(weighed, F(a2 / F(F(pdf_light * pdf_light) + a2)), f32(1.0)).astype(f32)   # :214-218
                L[ids[k]] = F(L[ids[k]] + F(F(T[ids[k]] * emission[k, 0:3]) * mis[:, None]))
                cen["emitter_cos_light_le_0"] += int((~(cos_light > 0)).sum())
                cen["emitter_after_bounce_front"] += int(((cos_light > 0) & ~flipped[k]).sum())
                cen["emitter_after_bounce_back"] += int(((cos_light > 0) & flipped[k]).sum())
            alive[ids[emit]] = False
            keep = ~emit
            ids, t, tri = ids[keep], t[keep], tri[keep]
            ro, rd = scene.shading_ray(ro[keep], rd[keep], tri)
            nrm, original_n, albedo, specular = nrm[keep], original_n[keep], albedo[keep], specular[keep]
            hit_point = F(F(ro + F(rd * t[:, None])) + F(nrm * f32(0.0002)))                  # :930
            mirror = albedo[:, 3] == MIRROR_TYPE
            cen["mirror_hit"] += int(mirror.sum())
            scene.note(cen, "mirror", tri[mirror])
            # ---- :938-1002 next-event estimation
            nee = (specular[:, 3] == f32(0.0)) & ~mirror
            k = np.nonzero(nee)[0]
            gk = ids[k]
            r0 = rng.draw(gk)
            r1 = rng.draw(gk)
            r2 = rng.draw(gk)
            if n_lights > 0 and k.size:
                li = F(r0 * f32(n_lights)).astype(np.int64)                                  # :940
                cen["light_index_clamped"] += int((li > n_lights - 1).sum())
                li = np.minimum(li, n_lights - 1)
                scene.note(cen, "nee_light", li)
                lt = scene.lights[li]
                s = np.sqrt(r1)                                                                # :849-854
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
                    blocked = scene.visibility(cen, 2, hit_point[ks], ld[sh], F(ln[sh] - _EPS))[0] >= 0    # :968
                    cen["shadow_occluded"] += int(blocked.sum())
                    cen["shadow_clear"] += int((~blocked).sum())
                    c = sh[~blocked]
                    kc = k[c]
                    ap = lt[c, 15:18]
                    pdf_light = F(F(F(ln[c] * ln[c]) / F(ap[:, 0] * -cos_light[c])) * ap[:, 1])  # :986
                    bsdf_pdf = F(F(dot(ld[c], nrm[kc]) * f32(1.0)) / _PI)                          # :293-294, ipi expands to 1.0f / pi
                    a2 = F(pdf_light * pdf_light)
                    mis = F(a2 / F(F(bsdf_pdf * bsdf_pdf) + a2))
                    contrib = F(F(F(F(T[ids[kc]] * lt[c, 12:15]) * albedo[kc, 0:3]) * mis[:, None]) / pdf_light[:, None])   # :998
                    L[ids[kc]] = F(L[ids[kc]] + contrib)
            # ---- the Mirror branch (this project's definition): reflect about the normalised shading normal
            if mirror.any():
                k = np.nonzero(mirror)[0]
                nn = normalize(nrm[k])
                dn = dot(rd[k], nn)
                refl = F(rd[k] - F(nn * F(f32(2.0) * dn)[:, None]))
                T[ids[k]] = F(T[ids[k]] * albedo[k, 0:3])
                if not scene.mirror_keeps_is_specular:
                    is_specular[ids[k]] = True                                                 # §2: the next emitter hit takes the :896 branch
                o[ids[k]], d[ids[k]] = hit_point[k], refl
            # ---- :1005-1018 the cosine bounce
            k = np.nonzero(~mirror)[0]
            gk = ids[k]
            nk = nrm[k]
            sing = nk[:, 2] < f32(-0.9999999)                                                  # :46
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
            sd = F(F(F(bu * sx[:, None]) + F(bv * sy[:, None])) + F(nk * sz[:, None]))        # :286
            prev_pdf[gk] = F(F(dot(sd, nk) * f32(1.0)) / _PI)
            T[gk] = F(T[gk] * albedo[k, 0:3])
            is_specular[gk] = False
            bounced[gk] = True
            o[gk], d[gk] = hit_point[k], sd
            frames.append(L.reshape(scene.H, scene.W, 3).copy())
            censuses.append(dict(cen))
    return frames, censuses


def render(scene, rvs, max_depth):
    """The running sums after the frames `rvs` = [(rx, ry), ...]: color = pixelColor + accumulate_color (:1059), from zero.
    Returns (sums[max_depth] of (H, W, 3) float32, per-frame radiance [frame][depth], census[max_depth] summed over the frames,
    per-frame census [frame][depth]); index depth - 1 is a path of that many segments."""
    sums = [np.zeros((scene.H, scene.W, 3), f32) for _ in range(max_depth)]
    radiance, census = [], []
    for rx, ry in rvs:
        frames, cens = render_frame(scene, rx, ry, max_depth)
        radiance.append(frames)
        census.append(cens)
        for k in range(max_depth):
            sums[k] = F(frames[k] + sums[k])
    total = [{key: sum(c[k][key] for c in census) for key in census[0][k]} for k in range(max_depth)]
    return sums, radiance, total, census


# ------------------------------------------------------------------------------------------------ Shader/output.fs:9-20

def resolve_ref(sum_buf, inv_count):
    """RGBA8 of a running sum: c = s * inv; lum = (0.3 c.x + 0.6 c.y) + 0.1 c.z; k = 1 / (1 + lum / 2); x = c * 1 * k;
    v = float32(pow(double(x), double(1.0f / 2.2f))) clamped to [0, 1]; byte = uint8(v * 255 + 0.5).  The exponent is the shader's
    `1.0 / 2.2` between two float literals, 0x3ee8ba2e — not the float nearest to the real 1 / 2.2, which is one ulp above it.  NaN and
    negatives give 0, alpha is 255.  Evaluated per value: no threshold table."""
    s = F(sum_buf)
    shape = s.shape[:-1]
    s = s.reshape(-1, 3)
    with np.errstate(all="ignore"):
        c = F(s * f32(inv_count))
        lum = F(F(F(f32(0.3) * c[:, 0]) + F(f32(0.6) * c[:, 1])) + F(f32(0.1) * c[:, 2]))
        k = F(f32(1.0) / F(f32(1.0) + F(lum / f32(2.0))))
        x = F(F(c * f32(1.0)) * k[:, None])
        v = _pow_double_once(x, f32(1.0) / f32(2.2))
        v = np.where(v != v, f32(0.0), v)
        v = np.minimum(np.maximum(v, f32(0.0)), f32(1.0)).astype(f32)
        b = F(F(v * f32(255.0)) + f32(0.5)).astype(np.uint8)
    out = np.full((s.shape[0], 4), 255, np.uint8)
    out[:, :3] = b
    return out.reshape(shape + (4,))
