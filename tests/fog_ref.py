"""A numpy restatement of fog with light shafts (crt_render_fog, crt_fog_segments, crt_fog_composite), written from the
definition in include/crt.h — steps 1 to 7, the view mode and the composite — not from the kernels.  Every arithmetic step is ONE float32
IEEE operation on whole arrays, nothing fused; exp_neg is float64 numpy from the header's constants with one rounding to float32.  The pinned
sine, dot, length, the primary rays and the scenes are integrator_ref's and instanced_ref's, rand_at is ao_ref's; occlusion is their brute
force over every triangle (`scene.visibility(cen, 2, x, ld, tmax)[0] >= 0`), which knows the masks of an instanced scene.

`breaks` are deliberate mistakes (tests/test_fog.py C5): each must change words of some test scene, or the scenes do not test the rule."""
import collections

import numpy as np

from ao_ref import rand_at
from instanced_ref import InstancedRef                                                          # noqa: F401  (the instanced scenes this module is asked about)
from integrator_ref import F, RefScene, dot, f32, length, primary_rays                          # noqa: F401

BREAKS = ("rand_zero_based", "stratum_jitter_dropped", "tmax_without_epsilon", "ct_wrong_sign", "att_without_ln", "sum_reversed",
          "seed_before_jitter")

FOG_SEGMENT_DT = np.dtype([("o", "<f4", 3), ("seed_x", "<f4"), ("e", "<f4", 3), ("seed_y", "<f4")])
UNBOUNDED = f32(1e9)
_EPS = f32(1e-4)
_INV_4PI = f32(0.07957747)

# what crt_fog_params holds; the defaults are the header's NULL
Params = collections.namedtuple("Params", "K density albedo anisotropy max_distance ambient",
                                defaults=(16, 0.05, (1.0, 1.0, 1.0), 0.0, 100.0, (0.0, 0.0, 0.0)))

_LOG2E = float.fromhex("0x1.71547652b82fep+0")
_LN2_HI = float.fromhex("0x1.62e42feep-1")
_LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
_FACTORIALS = (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0)


def exp_neg(xf):
    """step 6's pinned e^-x: float32 in, float32 out, every operation between them a float64 multiply or add"""
    x = np.asarray(xf, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        live = x < 104.0
        xs = np.where(live, x, 0.0)
        k = np.rint(xs * _LOG2E)
        r = (xs - k * _LN2_HI) - k * _LN2_LO
        q = -r
        p = np.full_like(xs, 1.0 / _FACTORIALS[0])
        for fact in _FACTORIALS[1:]:
            p = p * q + 1.0 / fact
        p = p * q + 1.0
        out = (p * np.ldexp(1.0, -k.astype(np.int64))).astype(f32)
    return np.where(live, out, f32(0.0)).astype(f32)


def frame(segments, K):
    """step 1: (has rays, o, dir, D, h) of FOG_SEGMENT_DT segments"""
    seg = np.asarray(segments, FOG_SEGMENT_DT).reshape(-1)
    o, e = F(seg["o"]), F(seg["e"])
    with np.errstate(all="ignore"):
        D2 = dot(e, e)
        ok = (D2 > 0) & np.isfinite(D2) & np.isfinite(o).all(1)
        D = np.sqrt(D2)
        direction = F(e * F(f32(1.0) / D)[:, None])
        h = F(D / f32(K))
    return ok, o, direction, D, h


def samples(lights, seg, o, direction, h, K, rv, breaks=()):
    """steps 3 - 5 for every (segment, j): a dict of (m, K[, 3]) arrays; `lit` is false for a dark sample"""
    m = o.shape[0]
    lights = F(lights).reshape(-1, 18)
    n_lights = lights.shape[0]
    out = dict(s=np.zeros((m, K), f32), x=np.zeros((m, K, 3), f32), ld=np.zeros((m, K, 3), f32), ln=np.zeros((m, K), f32),
               cos_light=np.zeros((m, K), f32), li=np.zeros((m, K), np.int64), lit=np.zeros((m, K), bool), tmax=np.zeros((m, K), f32))
    first = 0 if "rand_zero_based" in breaks else 1
    sx, sy = seg["seed_x"], seg["seed_y"]
    with np.errstate(all="ignore"):
        for j in range(K):
            u0, r0, r1, r2 = (rand_at(sx, sy, 4 * j + first + i, rv) for i in range(4))
            if "stratum_jitter_dropped" in breaks:
                u0 = np.full_like(u0, f32(0.5))
            s = F(F(f32(j) + u0) * h)
            x = F(o + F(direction * s[:, None]))
            out["s"][:, j], out["x"][:, j] = s, x
            if n_lights == 0:
                continue
            li = np.minimum(F(r0 * f32(n_lights)).astype(np.int64), n_lights - 1)
            lt = lights[li]
            sq = np.sqrt(r1)
            b0 = F(f32(1.0) - sq)
            b1 = F(r2 * sq)
            pos = F(F(lt[:, 0:3] + F(lt[:, 3:6] * b0[:, None])) + F(lt[:, 6:9] * b1[:, None]))
            ld = F(pos - x)
            ln = length(ld)
            ld = F(ld * F(f32(1.0) / ln)[:, None])
            cos_light = dot(ld, lt[:, 9:12])
            out["ld"][:, j], out["ln"][:, j], out["cos_light"][:, j], out["li"][:, j] = ld, ln, cos_light, li
            out["lit"][:, j] = cos_light < 0
            out["tmax"][:, j] = ln if "tmax_without_epsilon" in breaks else F(ln - _EPS)
    return out


def contributions(lights, direction, h, sm, p, breaks=()):
    """step 6 for every (segment, j), as if each were unoccluded: (m, K, 3)"""
    lights = F(lights).reshape(-1, 18)
    m, K = sm["s"].shape
    if lights.shape[0] == 0:
        return np.zeros((m, K, 3), f32)
    sigma, g = f32(p.density), f32(p.anisotropy)
    albedo = F(p.albedo)
    lt = lights[sm["li"]]
    with np.errstate(all="ignore"):
        ln, cl = sm["ln"], sm["cos_light"]
        pdf = F(F(F(ln * ln) / F(lt[..., 15] * -cl)) * lt[..., 16])
        ct = dot(np.broadcast_to(direction[:, None, :], sm["ld"].shape), sm["ld"])
        if "ct_wrong_sign" in breaks:
            ct = -ct
        g2 = F(g * g)
        den = F(F(f32(1.0) + g2) - F(F(f32(2.0) * g) * ct))
        ph = F(F(F(f32(1.0) - g2) * _INV_4PI) / F(den * np.sqrt(den)))
        att = exp_neg(F(sigma * sm["s"])) if "att_without_ln" in breaks else exp_neg(F(sigma * F(sm["s"] + ln)))
        w = F(F(F(att * ph) * F(sigma * h)[:, None]) / pdf)
        return F(F(lt[..., 12:15] * albedo) * w[..., None])


def fold(ok, D, contrib, add, p, breaks=()):
    """steps 2 and 7: (m, 4) from the contributions and which of them count (m, K): lit and unoccluded"""
    m, K = add.shape
    TD = exp_neg(F(f32(p.density) * D))
    with np.errstate(all="ignore"):
        b = F(F(F(p.ambient) * F(p.albedo))[None, :] * F(f32(1.0) - TD)[:, None])
        order = range(K - 1, -1, -1) if "sum_reversed" in breaks else range(K)
        for j in order:
            b = np.where(add[:, j:j + 1], F(b + contrib[:, j]), b).astype(f32)
    out = np.zeros((m, 4), f32)
    out[:, :3] = b
    out[:, 3] = TD
    out[~ok] = F([0.0, 0.0, 0.0, -1.0])
    return out


def occlusion(scene, ok, sm):
    """step 5 by brute force: unoccluded (m, K); dark samples and the samples of segments without rays are not traced"""
    want = sm["lit"] & ok[:, None]
    visible = np.zeros(want.shape, bool)
    idx = np.nonzero(want)
    if idx[0].size:
        cen = collections.defaultdict(int)
        hit = scene.visibility(cen, 2, sm["x"][idx], sm["ld"][idx], sm["tmax"][idx])[0] >= 0
        visible[idx] = ~hit
    return visible


def fog_segments(scene, segments, rx, ry, p=Params(), breaks=(), lights=None, visible=None):
    """crt_fog_segments: (m, 4) float32; also the rays and their answers for a comparison with another walk.  lights: the table to sample
    in place of the scene's own (what crt_scene_read_lights returned).  visible: the answers of an earlier call on the same segments, seeds,
    K and lights, in place of the brute force: the rays do not depend on the medium"""
    seg = np.asarray(segments, FOG_SEGMENT_DT).reshape(-1)
    rv = F(f32(rx) * f32(ry))
    lights = scene.lights if lights is None else lights
    ok, o, direction, D, h = frame(seg, p.K)
    sm = samples(lights, seg, o, direction, h, p.K, rv, breaks)
    contrib = contributions(lights, direction, h, sm, p, breaks)
    if visible is None:
        visible = occlusion(scene, ok, sm)
    add = visible & sm["lit"] & ok[:, None]
    rays = dict(ok=ok, D=D, x=sm["x"], ld=sm["ld"], tmax=sm["tmax"], lit=sm["lit"] & ok[:, None], visible=visible, contrib=contrib, add=add)
    return fold(ok, D, contrib, add, p, breaks), rays


def view_segments(scene, rx, ry, jitter, max_distance, breaks=()):
    """view mode: the fog segments of the scene's W x H view, linear pixel order"""
    o, d, rng, _ = primary_rays(scene, rx, ry, jitter=bool(jitter))
    seg = np.zeros(o.shape[0], FOG_SEGMENT_DT)
    if "seed_before_jitter" in breaks:
        py, px = np.meshgrid(np.arange(scene.H), np.arange(scene.W), indexing="ij")
        seg["seed_x"], seg["seed_y"] = F(px.reshape(-1).astype(f32) + f32(0.5)), F(py.reshape(-1).astype(f32) + f32(0.5))
    else:
        seg["seed_x"], seg["seed_y"] = rng.sx, rng.sy
    cen = collections.defaultdict(int)
    with np.errstate(all="ignore"):
        tri, t, _, _ = scene.visibility(cen, 0, o, d, UNBOUNDED)
        t = np.where(tri >= 0, t, UNBOUNDED).astype(f32)
        Dv = np.minimum(t, f32(max_distance))
        seg["o"] = o
        seg["e"] = F(d * Dv[:, None])
    return seg, tri


def render_fog(scene, rx, ry, p=Params(), jitter=1, breaks=(), lights=None, known=None):
    """crt_render_fog: (H, W, 4) float32 and the rays behind it.  known: the rays of an earlier call with the same view, jitter, K,
    max_distance and lights, whose segments and occlusion answers are taken over (another density, albedo, anisotropy or ambient term)"""
    seg, tri = view_segments(scene, rx, ry, jitter, p.max_distance, breaks) if known is None else (known["segments"], known["tri"])
    out, rays = fog_segments(scene, seg, rx, ry, p, breaks, lights, None if known is None else known["visible"])
    rays["segments"], rays["tri"] = seg, tri
    return out.reshape(scene.H, scene.W, 4), rays


def composite(image, fog, inv_count=None):
    """crt_fog_composite: image (H, W, 3) — the running sum with its inv_count, or a denoised / accumulated image with None — under
    crt_render_fog's (H, W, 4)"""
    c = F(image) if inv_count is None else F(F(image) * f32(inv_count))
    fog = F(fog)
    with np.errstate(all="ignore"):
        out = F(F(c * fog[..., 3:4]) + fog[..., 0:3])
    return np.where(fog[..., 3:4] == f32(-1.0), c, out).astype(f32)
