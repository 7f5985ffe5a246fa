"""A numpy restatement of frames along the caller's camera rays, written from include/crt.h (the contract at crt_set_camera_rays; DESIGN.md
§34) on top of tests/integrator_ref.py's helpers — not from rt_kernels.hip, and importing nothing from oracle/.  The C oracle has no such
frames: they are held to numpy alone.

Per pixel-sample (px, py), with the entry at py * width + px:

  o, d   the entry's, AS GIVEN: d is not normalised; the primary ray's bound is 1e9f whatever the entry's tmax says
  rng    the pixel's initial state (px + 0.5, py + 0.5) with no draw taken, whatever "jitter" says
  path   L = 0, pdf = 1, T = 1, specular: what integrator_ref.render_frame starts from

The integrator is integrator_ref.render_frame's own loop: `render` runs it with `primary_rays` substituted (mock.patch, as lens_ref.render
does) over a RefScene or an instanced_ref.InstancedRef; with an environment it runs env_ref.render_frame, which takes the primary rays as an
argument.  An entry without a path — a component of o or d that is not finite, or d == (0, 0, 0) — adds +0: pixels are independent in the
integrator, so the loop runs with a harmless ray in that entry's place and the pixel's radiance is set to +0 afterwards.  The census then
counts that stand-in: ray counts are compared only where every entry has a path.

`mistake` makes one deliberate error of reading the contract (tests/test_camera_rays.py C5 shows that each changes words)."""
from unittest import mock

import numpy as np

import integrator_ref as ir
from integrator_ref import F, f32

MISTAKES = ("normalised_again", "seed_behind_jitter", "rows_flipped", "px_py_swapped", "entry_tmax")


def valid_entries(o, d):
    """(n,) bool: the entries that have a path"""
    o, d = F(o).reshape(-1, 3), F(d).reshape(-1, 3)
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def entries(scene, o, d):
    """(o, d) as (n, 3) float32 in pixel order, a (3,) origin broadcast"""
    d = F(d).reshape(-1, 3)
    assert d.shape[0] == scene.W * scene.H
    o = F(o)
    o = np.broadcast_to(o, d.shape) if o.shape == (3,) else o.reshape(-1, 3)
    return o.astype(f32), d.astype(f32)


def primary(scene, o, d, rx, ry, mistake=None):
    """What integrator_ref.primary_rays returns, for the caller's rays: (o, d, rng, {}) — entries without a path replaced by a stand-in"""
    W, H = scene.W, scene.H
    o, d = entries(scene, o, d)
    if mistake == "rows_flipped":
        o, d = o.reshape(H, W, 3)[::-1].reshape(-1, 3), d.reshape(H, W, 3)[::-1].reshape(-1, 3)
    if mistake == "px_py_swapped":                      # the entry of (px, py) looked up at px * height + py
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        idx = (px * H + py).reshape(-1)
        o, d = o[idx], d[idx]
    ok = valid_entries(o, d)
    o = np.where(ok[:, None], o, f32(0.0)).astype(f32)
    d = np.where(ok[:, None], d, F([0.0, 0.0, 1.0])).astype(f32)
    if mistake == "normalised_again":
        d = ir.normalize(d)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = ir._Rng(F(px.reshape(-1).astype(f32) + f32(0.5)), F(py.reshape(-1).astype(f32) + f32(0.5)), rx, ry)
    if mistake == "seed_behind_jitter":
        everyone = np.ones(W * H, bool)
        rng.draw(everyone)
        rng.draw(everyone)
    return o.copy(), d.copy(), rng, {}


class _ShortPrimaries:
    """the scene with segment 0's rays bounded by a short tmax (the "entry_tmax" mistake); everything else is the scene's"""

    def __init__(self, scene, short_tmax):
        self._scene, self._short = scene, f32(short_tmax)

    def __getattr__(self, name):
        return getattr(self._scene, name)

    def visibility(self, cen, ray_class, o, d, tmax):
        return self._scene.visibility(cen, ray_class, o, d, self._short if ray_class == 0 else tmax)


def render(scene, o, d, rvs, max_depth, env=None, mistake=None, short_tmax=None):
    """The running sums after the frames `rvs` along the rays (o, d): integrator_ref.render's four return values (sums[max_depth], per-frame
    radiance, census summed over the frames, per-frame census).  `env`: an env_ref.Env; short_tmax: the bound the "entry_tmax" mistake takes from the entries."""
    assert mistake is None or mistake in MISTAKES
    holes = ~valid_entries(*entries(scene, o, d))
    if mistake in ("rows_flipped", "px_py_swapped"):
        assert not holes.any()
    sc = _ShortPrimaries(scene, short_tmax) if mistake == "entry_tmax" else scene

    def primary_rays(s, rx, ry, jitter=True):
        return primary(s, o, d, rx, ry, mistake)

    def frame(rx, ry):
        if env is not None:
            import env_ref as er
            return er.render_frame(sc, rx, ry, max_depth, env, lambda s, a, b: primary_rays(s, a, b))
        with mock.patch.object(ir, "primary_rays", primary_rays):
            return ir.render_frame(sc, rx, ry, max_depth)

    sums = [np.zeros((scene.H, scene.W, 3), f32) for _ in range(max_depth)]
    radiance, census = [], []
    for rx, ry in rvs:
        frames, cens = frame(rx, ry)
        for k in range(max_depth):
            frames[k].reshape(-1, 3)[holes] = f32(0.0)              # +0: an entry without a path
            sums[k] = F(frames[k] + sums[k])
        radiance.append(frames)
        census.append(cens)
    total = [{key: sum(c[k][key] for c in census) for key in census[0][k]} for k in range(max_depth)]
    return sums, radiance, total, census
