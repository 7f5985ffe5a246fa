"""Host helpers that build the octahedral environment maps Scene.set_environment takes (include/crt.h at crt_set_environment;
DESIGN.md §28).  Plain numpy, float64 inside, float32 out; nothing here is part of the bit-exact contract — that begins at the texels.

The map is a square of size x size texels over [-1, 1]^2: texel (row j, column i) has its centre at px = (2 i + 1) / size - 1,
py = (2 j + 1) / size - 1.  A point of the square is the direction (px, py, 1 - |px| - |py|) where that z is >= 0 — the upper hemisphere,
+z at the centre — and ((1 - |py|) sgn(px), (1 - |px|) sgn(py), 1 - |px| - |py|) where it is negative: the lower hemisphere folded
outwards, -z at the four corners."""
import numpy as np


def octahedral_directions(size):
    """(size, size, 3) float64 unit vectors through the texel centres, indexed [row j][column i]"""
    size = int(size)
    if size < 1:
        raise ValueError("size must be >= 1")
    c = (2.0 * np.arange(size) + 1.0) / size - 1.0
    px, py = np.meshgrid(c, c, indexing="xy")
    z = 1.0 - np.abs(px) - np.abs(py)
    sgn = lambda a: np.where(a < 0, -1.0, 1.0)
    x = np.where(z < 0, (1.0 - np.abs(py)) * sgn(px), px)
    y = np.where(z < 0, (1.0 - np.abs(px)) * sgn(py), py)
    d = np.stack([x, y, z], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def octahedral_from_function(fn, size):
    """fn takes (n, 3) float64 unit directions and returns (n, 3) RGB radiance; -> (size, size, 3) float32 texels"""
    d = octahedral_directions(size)
    rgb = np.asarray(fn(d.reshape(-1, 3)), np.float64).reshape(size, size, 3)
    return np.ascontiguousarray(rgb, np.float32)


def equirect_lookup(img, d, up="y"):
    """Bilinear lookup of a lat-long image (H, W, 3) at unit directions d (n, 3): row 0 is the pole `up` points to, v = acos(d.up) / pi;
    u = atan2 of the two other axes in cyclic order / 2 pi, wrapped (up "y": atan2(d.x, d.z); up "z": atan2(d.y, d.x)); texel centres at
    (i + 0.5) / W, (j + 0.5) / H; columns wrap, rows clamp."""
    img = np.asarray(img, np.float64)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("img must be (H, W, 3)")
    k = {"x": 0, "y": 1, "z": 2}[up]
    a, b = d[:, (k + 1) % 3], d[:, (k + 2) % 3]
    H, W = img.shape[:2]
    u = (np.arctan2(b, a) / (2.0 * np.pi)) % 1.0
    v = np.arccos(np.clip(d[:, k], -1.0, 1.0)) / np.pi
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    i0, i1 = x0.astype(np.int64) % W, (x0.astype(np.int64) + 1) % W
    j0, j1 = np.clip(y0.astype(np.int64), 0, H - 1), np.clip(y0.astype(np.int64) + 1, 0, H - 1)
    top = img[j0, i0] * (1 - fx) + img[j0, i1] * fx
    bot = img[j1, i0] * (1 - fx) + img[j1, i1] * fx
    return top * (1 - fy) + bot * fy


def octahedral_from_equirect(img, size, up="y"):
    """A lat-long (equirectangular) RGB image (H, W, 3), e.g. a decoded HDR panorama, resampled at the octahedral texel centres
    (equirect_lookup's convention) -> (size, size, 3) float32 texels"""
    return octahedral_from_function(lambda d: equirect_lookup(img, d, up), size)


def constant_environment(rgb):
    """A size-1 map: the same radiance from every direction"""
    return np.ascontiguousarray(np.asarray(rgb, np.float32).reshape(1, 1, 3))


__all__ = ["octahedral_directions", "octahedral_from_function", "octahedral_from_equirect", "equirect_lookup", "constant_environment"]
