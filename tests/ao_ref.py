"""A numpy restatement of ambient occlusion (crt_render_ao, crt_ao_points), written from the definition in include/crt.h —
steps 1 to 7 and the view mode — not from the kernels.  Every arithmetic step is ONE float32 IEEE operation on whole arrays, nothing fused.
The pinned sine and cosine, dot, normalize, the primary rays and the scenes are integrator_ref's and instanced_ref's; occlusion is their
brute force over every triangle (`scene.visibility(cen, 2, o, d, radius)[0] >= 0`), which knows the masks of an instanced scene.

`breaks` are deliberate mistakes (tests/test_ao.py C5): each must change words of some test scene, or the scenes do not test the rule."""
import collections

import numpy as np

from instanced_ref import InstancedRef                                                          # noqa: F401  (the instanced scenes this module is asked about)
from integrator_ref import F, RefScene, dot, f32, normalize, pinned_cos, pinned_sin, primary_rays, _interp    # noqa: F401

BREAKS = ("normal_unnormalised", "offset_dropped", "rand_zero_based", "basis_of_the_integrator", "sum_reversed", "seed_before_jitter")

AO_POINT_DT = np.dtype([("p", "<f4", 3), ("seed_x", "<f4"), ("n", "<f4", 3), ("seed_y", "<f4")])
UNBOUNDED = f32(1e9)
OFFSET = f32(0.0002)


def frame(p, n, offset, breaks=()):
    """steps 1 - 3: (has rays, nn, o, bu, bv) of points p (m, 3) with normals n (m, 3)"""
    p, n, offset = F(p), F(n), f32(offset)
    with np.errstate(all="ignore"):
        l2 = dot(n, n)
        ok = (l2 > 0) & np.isfinite(l2) & np.isfinite(p).all(1)
        nn = F(n * F(f32(1.0) / np.sqrt(l2))[:, None])
        if "normal_unnormalised" in breaks:
            nn = n
        o = p if "offset_dropped" in breaks else F(p + F(nn * offset))
        a = F(f32(1.0) / F(f32(1.0) + nn[:, 2]))
        b = F(F(-nn[:, 0] * nn[:, 1]) * a)
        if "basis_of_the_integrator" in breaks:
            ux, vy = F(f32(1.0) + b), F(f32(1.0) + b)
        else:
            ux = F(f32(1.0) - F(F(nn[:, 0] * nn[:, 0]) * a))
            vy = F(f32(1.0) - F(F(nn[:, 1] * nn[:, 1]) * a))
        bu = np.stack([ux, b, -nn[:, 0]], -1).astype(f32)
        bv = np.stack([b, vy, -nn[:, 1]], -1).astype(f32)
        singular = nn[:, 2] < f32(-0.9999999)
        bu = np.where(singular[:, None], F([0.0, -1.0, 0.0]), bu).astype(f32)
        bv = np.where(singular[:, None], F([-1.0, 0.0, 0.0]), bv).astype(f32)
    return ok, nn, o, bu, bv


def rand_at(seed_x, seed_y, j, rv):
    """step 4: the j-th draw (j = 1, 2, ...) from the seed, by index"""
    s = F(f32(j) * f32(rv))
    ax, ay = F(F(seed_x) - s), F(F(seed_y) - s)
    d = F(F(ax * f32(12.9898)) + F(ay * f32(78.233)))
    v = F(pinned_sin(d) * f32(43758.5453))
    return F(v - np.floor(v))


def directions(nn, bu, bv, seed_x, seed_y, K, rv, breaks=()):
    """steps 4 - 5: sd (m, K, 3)"""
    out = np.zeros((nn.shape[0], K, 3), f32)
    first = 0 if "rand_zero_based" in breaks else 1
    with np.errstate(all="ignore"):
        for k in range(K):
            u1, u2 = rand_at(seed_x, seed_y, 2 * k + first, rv), rand_at(seed_x, seed_y, 2 * k + first + 1, rv)
            r = np.sqrt(u1)
            phi = F(f32(6.2831853) * u2)
            sx, sy, sz = F(r * pinned_cos(phi)), F(r * pinned_sin(phi)), np.sqrt(F(f32(1.0) - u1))
            out[:, k] = F(F(F(bu * sx[:, None]) + F(bv * sy[:, None])) + F(nn * sz[:, None]))
    return out


def fold(ok, sd, visible, breaks=()):
    """step 7: (m, 4) from the directions and which of them are unoccluded (m, K)"""
    m, K = visible.shape
    b = np.zeros((m, 3), f32)
    order = range(K - 1, -1, -1) if "sum_reversed" in breaks else range(K)
    for k in order:
        b = np.where(visible[:, k:k + 1], F(b + sd[:, k]), b).astype(f32)
    out = np.zeros((m, 4), f32)
    out[:, :3] = b
    out[:, 3] = F(visible.sum(1).astype(f32) / f32(K))
    out[~ok] = F([0.0, 0.0, 0.0, -1.0])
    return out


def rays_of(points, K, rv, offset=OFFSET, breaks=()):
    """-> (ok (m), o (m, 3), sd (m, K, 3)) of AO_POINT_DT points"""
    pts = np.asarray(points, AO_POINT_DT).reshape(-1)
    ok, nn, o, bu, bv = frame(pts["p"], pts["n"], offset, breaks)
    sd = directions(nn, bu, bv, pts["seed_x"], pts["seed_y"], K, rv, breaks)
    return ok, o, sd


def occlusion(scene, ok, o, sd, radius):
    """step 6 by brute force: unoccluded (m, K); the rays of points without rays are not traced"""
    m, K = sd.shape[:2]
    visible = np.zeros((m, K), bool)
    idx = np.nonzero(ok)[0]
    if idx.size:
        oo = np.repeat(o[idx], K, 0)
        dd = sd[idx].reshape(-1, 3)
        cen = collections.defaultdict(int)
        hit = scene.visibility(cen, 2, oo, dd, f32(radius))[0] >= 0
        visible[idx] = ~hit.reshape(idx.size, K)
    return visible


def ao_points(scene, points, K, rx, ry, radius=UNBOUNDED, offset=OFFSET, breaks=()):
    """crt_ao_points: (m, 4) float32; also the rays and their answers for a comparison with another walk"""
    rv = F(f32(rx) * f32(ry))
    ok, o, sd = rays_of(points, K, rv, offset, breaks)
    visible = occlusion(scene, ok, o, sd, radius)
    return fold(ok, sd, visible, breaks), dict(ok=ok, o=o, sd=sd, visible=visible)


def view_points(scene, rx, ry, jitter, breaks=()):
    """view mode: the AO points of the scene's W x H view, linear pixel order"""
    o, d, rng, _ = primary_rays(scene, rx, ry, jitter=bool(jitter))
    n = o.shape[0]
    pts = np.zeros(n, AO_POINT_DT)
    if "seed_before_jitter" in breaks:
        py, px = np.meshgrid(np.arange(scene.H), np.arange(scene.W), indexing="ij")
        pts["seed_x"], pts["seed_y"] = F(px.reshape(-1).astype(f32) + f32(0.5)), F(py.reshape(-1).astype(f32) + f32(0.5))
    else:
        pts["seed_x"], pts["seed_y"] = rng.sx, rng.sy
    cen = collections.defaultdict(int)
    with np.errstate(all="ignore"):
        tri, t, u, v = scene.visibility(cen, 0, o, d, UNBOUNDED)
        ids = np.nonzero(tri >= 0)[0]
        tri, t, u, v = tri[ids], t[ids], u[ids], v[ids]
        row, _ = scene.hit_rows(cen, 0, tri)
        flat = row[:, 7] == 0
        nrm = np.where(flat[:, None], row[:, 4:7].astype(f32),
                       _interp(scene.N[np.where(flat, 0, row[:, 4])], scene.N[np.where(flat, 0, row[:, 5])],
                               scene.N[np.where(flat, 0, row[:, 6])], u, v) if scene.N.shape[0] else row[:, 4:7].astype(f32)).astype(f32)
        nrm = scene.world_normal(nrm, tri)
        flipped = dot(d[ids], nrm) > 0
        nrm = np.where(flipped[:, None], -nrm, nrm).astype(f32)
        pts["p"][ids] = F(o[ids] + F(d[ids] * t[:, None]))
        pts["n"][ids] = nrm
    return pts, tri, ids


def render_ao(scene, rx, ry, K, radius=UNBOUNDED, offset=OFFSET, jitter=1, breaks=()):
    """crt_render_ao: (H, W, 4) float32 and the rays behind it"""
    pts, _, _ = view_points(scene, rx, ry, jitter, breaks)
    out, rays = ao_points(scene, pts, K, rx, ry, radius, offset, breaks)
    rays["points"] = pts
    return out.reshape(scene.H, scene.W, 4), rays
