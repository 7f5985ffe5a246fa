"""Ray builders for Scene.set_camera_rays (include/crt.h at crt_set_camera_rays): float32 numpy, no library needed.

Each returns (o, d), both (height, width, 3) float32 with rows as Scene.read_sum()'s (row 0 = the lowest py), ready for
Scene.set_camera_rays(o, d).  Directions are unit vectors; a pixel that has no ray gets d = (0, 0, 0), which the library renders as +0.
Each accepts a sub-pixel offset `jitter` = (jx, jy) in pixel units, added to the pixel centre (px + 0.5, py + 0.5): a caller who wants
antialiasing sets newly offset rays per frame (the library draws no jitter of its own along camera rays).

pinhole_rays restates the library's own "jitter" 0 primary rays operation for operation in float32, so that frames along them are the
pinhole's frames bit for bit.  The other three are computed in float64 and rounded once per component."""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
f64 = np.float64


def _F(x):
    return np.asarray(x, dtype=f32)


def _tanf(x):
    """the host's float tanf: what the library's frame set-up calls once per frame"""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.tanf.restype = ctypes.c_float
    libm.tanf.argtypes = [ctypes.c_float]
    return f32(libm.tanf(float(f32(x))))


def _camera_fields(camera):
    c = camera.c if hasattr(camera, "c") else camera
    return (_F(c.position[:]), _F(c.right[:]), _F(c.up[:]), _F(c.forward[:]), f32(c.fov))


def _pixel_centres(width, height, jitter, dtype):
    """(fx, fy) of every pixel, (height, width) each: px + 0.5 + jx, py + 0.5 + jy in `dtype`, one operation per step"""
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError("width and height must be >= 1")
    jx, jy = (dtype(jitter[0]), dtype(jitter[1]))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx = ((px.astype(dtype) + dtype(0.5)).astype(dtype) + jx).astype(dtype)
    fy = ((py.astype(dtype) + dtype(0.5)).astype(dtype) + jy).astype(dtype)
    return fx, fy


def _unit64(v, what):
    v = np.asarray(v, f64).reshape(3)
    n = math.sqrt(float(v @ v))
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError(what + " must be a finite non-zero vector")
    return v / n


def _frame64(forward, up):
    """an orthonormal (right, up, forward) in float64 from a forward and an up hint: right = forward x up, up = right x forward"""
    f = _unit64(forward, "forward")
    r = np.cross(f, np.asarray(up, f64).reshape(3))
    r = _unit64(r, "forward x up")
    return r, np.cross(r, f), f


def _round_unit(d64):
    """float64 directions, normalised there, rounded once per component to float32; zero rows stay zero"""
    n = np.sqrt((d64 * d64).sum(-1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(n > 0.0, d64 / n, 0.0)
    return out.astype(f32)


def pinhole_rays(camera, width, height, jitter=(0.0, 0.0)):
    """The library's own primary rays at option "jitter" 0 (path_trace.fs:1026-1047 without its two jitter draws), bit for bit: every
    step one float32 operation in the shader's order.  `camera` is a Camera (or anything with the crt_camera fields, directly or as .c)."""
    pos, right, up, fwd, fov = _camera_fields(camera)
    W, H = int(width), int(height)
    fx, fy = _pixel_centres(W, H, jitter, f32)
    fx, fy = fx.reshape(-1), fy.reshape(-1)
    tex_x, tex_y = _F(fx / f32(W)), _F(fy / f32(H))
    dx = _F(_F(f32(2.0) * tex_x) - f32(1.0))
    dy = _F(_F(f32(2.0) * tex_y) - f32(1.0))
    tan_fov = _tanf(_F(fov * f32(0.5)))
    dx = _F(dx * _F(_F(f32(W) / f32(H)) * tan_fov))
    dy = _F(dy * tan_fov)
    v = _F(_F(_F(dx[:, None] * right) + _F(dy[:, None] * up)) + fwd)
    dot = _F(_F(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    inv = _F(f32(1.0) / np.sqrt(dot))
    d = _F(v * inv[:, None])
    o = np.broadcast_to(pos, d.shape).astype(f32)
    return o.reshape(H, W, 3), d.reshape(H, W, 3)


def panorama_rays(position, width, height, forward=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), jitter=(0.0, 0.0)):
    """Equirectangular, the full sphere, from one point.  Column px spans longitude ((px + 0.5) / width * 2 - 1) * pi, 0 along `forward`
    and growing towards forward x up; row py latitude ((py + 0.5) / height * 2 - 1) * pi / 2, growing towards `up`.  With an odd width
    the centre column looks along `forward`."""
    r, u, f = _frame64(forward, up)
    fx, fy = _pixel_centres(width, height, jitter, f64)
    lon = (fx / f64(width) * 2.0 - 1.0) * math.pi
    lat = (fy / f64(height) * 2.0 - 1.0) * (math.pi / 2.0)
    cl = np.cos(lat)
    d = (cl * np.cos(lon))[..., None] * f + (cl * np.sin(lon))[..., None] * r + np.sin(lat)[..., None] * u
    d = _round_unit(d)
    o = np.broadcast_to(_F(position).reshape(3), d.shape).astype(f32)
    return o, d


def orthographic_rays(position, forward, up, width, height, extent_x, extent_y, jitter=(0.0, 0.0)):
    """Parallel rays along `forward` from a window of extent_x by extent_y world units centred at `position`: pixel (px, py) starts at
    position + ((px + 0.5) / width - 0.5) extent_x right + ((py + 0.5) / height - 0.5) extent_y up, right = forward x up."""
    r, u, f = _frame64(forward, up)
    fx, fy = _pixel_centres(width, height, jitter, f64)
    sx = (fx / f64(width) - 0.5) * f64(extent_x)
    sy = (fy / f64(height) - 0.5) * f64(extent_y)
    o = np.asarray(position, f64).reshape(3) + sx[..., None] * r + sy[..., None] * u
    d = np.broadcast_to(_round_unit(f[None, :])[0], o.shape).astype(f32)
    return o.astype(f32), d


def fisheye_rays(camera, width, height, fov_deg=180.0, jitter=(0.0, 0.0)):
    """Equidistant fisheye through `camera`'s position and basis: the image circle is the largest one the frame holds (radius
    min(width, height) / 2 pixels about the frame's centre), a pixel at the fraction rho of that radius looks fov_deg / 2 * rho away from
    forward, towards its own side.  Pixels outside the circle get d = (0, 0, 0): no path, +0."""
    pos, right, up, fwd, _ = _camera_fields(camera)
    r, u, f = _unit64(right, "right"), _unit64(up, "up"), _unit64(fwd, "forward")
    if not (0.0 < float(fov_deg) <= 360.0):
        raise ValueError("fov_deg must be in (0, 360]")
    W, H = int(width), int(height)
    fx, fy = _pixel_centres(W, H, jitter, f64)
    cx, cy = fx - W / 2.0, fy - H / 2.0
    radius = min(W, H) / 2.0
    rr = np.sqrt(cx * cx + cy * cy)
    rho = rr / radius
    theta = rho * math.radians(float(fov_deg)) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ux, uy = np.where(rr > 0.0, cx / rr, 0.0), np.where(rr > 0.0, cy / rr, 0.0)
    st = np.sin(theta)
    d = (st * ux)[..., None] * r + (st * uy)[..., None] * u + np.cos(theta)[..., None] * f
    d = _round_unit(d)
    d[rho > 1.0] = 0.0
    o = np.broadcast_to(pos, d.shape).astype(f32)
    return o, d
