"""A numpy restatement of the thin-lens camera, written from include/crt.h (the contract at crt_camera) on top of
tests/integrator_ref.py's helpers — not from rt_kernels.hip, and importing nothing from oracle/.  The C oracle has no lens: frames through
a lens are held to numpy alone.

Per pixel-sample, every step ONE float32 IEEE operation:

  v   = (right dx + up dy) + forward        integrator_ref.primary_rays' direction before normalize(), jitter included
  u1, u2                                    two more draws of the shader RNG, directly behind the jitter draws
  r   = aperture sqrt(u1),  phi = 6.2831853f u2
  lx  = r pinned_cos(phi),  ly = r pinned_sin(phi)
  lo  = right lx + up ly
  o   = position + lo
  d   = normalize(v focal_dist - lo)

and the path's RNG goes on behind u2.  aperture == 0 is integrator_ref.primary_rays itself: no draws, focal_dist not looked at.

The integrator is integrator_ref.render_frame's own loop: `render` runs integrator_ref.render with `primary_rays` substituted for the
duration of the call, over a RefScene or — an instanced scene — an instanced_ref.InstancedRef, whose questions that loop asks."""
from unittest import mock

import numpy as np

import integrator_ref as ir
from integrator_ref import F, f32


def view_vectors(scene, rx, ry, jitter=True):
    """primary_rays' lines up to v = (right dx + up dy) + forward.  Returns (v, rng behind the jitter draws, census of the jitter arms)."""
    W, H = scene.W, scene.H
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx = F(px.reshape(-1).astype(f32) + f32(0.5))
    fy = F(py.reshape(-1).astype(f32) + f32(0.5))
    rng = ir._Rng(fx, fy, rx, ry)
    everyone = np.ones(fx.shape[0], bool)
    census = {}
    tex_x, tex_y = F(fx / f32(W)), F(fy / f32(H))
    dx = F(F(f32(2.0) * tex_x) - f32(1.0))
    dy = F(F(f32(2.0) * tex_y) - f32(1.0))
    if jitter:
        r1 = F(f32(2.0) * rng.draw(everyone))
        r2 = F(f32(2.0) * rng.draw(everyone))
        census = {"jitter_x_low": int((r1 < 1).sum()), "jitter_x_high": int((r1 >= 1).sum()),
                  "jitter_y_low": int((r2 < 1).sum()), "jitter_y_high": int((r2 >= 1).sum())}
        jx = F(ir._jitter(r1) / F(f32(W) * f32(0.5)))
        jy = F(ir._jitter(r2) / F(f32(H) * f32(0.5)))
        dx, dy = F(dx + jx), F(dy + jy)
    tan_fov = f32(ir._libm.tanf(float(F(scene.fov * f32(0.5)))))
    dx = F(dx * F(F(f32(W) / f32(H)) * tan_fov))
    dy = F(dy * tan_fov)
    v = F(F(F(dx[:, None] * scene.cam_right) + F(dy[:, None] * scene.cam_up)) + scene.cam_forward)
    return v, rng, census


def lens_rays(scene, rx, ry, aperture, focal_dist, jitter=True):
    """The primary rays of every pixel, row py first: a dict of o, d, rng (behind u2), census, and v, lx, ly for the tests of the lens
    itself.  aperture == 0: integrator_ref.primary_rays' own return values (v, lx, ly are then None)."""
    aperture, focal_dist = f32(aperture), f32(focal_dist)
    if aperture == 0:
        o, d, rng, census = ir.primary_rays(scene, rx, ry, jitter=jitter)
        return dict(o=o, d=d, rng=rng, census=census, v=None, lx=None, ly=None)
    v, rng, census = view_vectors(scene, rx, ry, jitter)
    everyone = np.ones(v.shape[0], bool)
    u1 = rng.draw(everyone)
    u2 = rng.draw(everyone)
    r = F(aperture * np.sqrt(u1))
    phi = F(ir._PI2 * u2)
    lx, ly = F(r * ir.pinned_cos(phi)), F(r * ir.pinned_sin(phi))
    lo = F(F(scene.cam_right * lx[:, None]) + F(scene.cam_up * ly[:, None]))
    o = F(scene.cam_pos + lo)
    d = ir.normalize(F(F(v * focal_dist) - lo))
    return dict(o=o, d=d, rng=rng, census=census, v=v, lx=lx, ly=ly)


def render(scene, rvs, max_depth, aperture, focal_dist, jitter=True):
    """integrator_ref.render(scene, rvs, max_depth) seen through the lens: the same four return values"""
    def primary_rays(sc, rx, ry, jitter=jitter):
        out = lens_rays(sc, rx, ry, aperture, focal_dist, jitter=through_jitter)
        return out["o"].copy(), out["d"].copy(), out["rng"], out["census"]
    through_jitter = jitter               # render_frame always asks for jitter=True: the lens frame's own setting wins
    with mock.patch.object(ir, "primary_rays", primary_rays):
        return ir.render(scene, rvs, max_depth)
