"""crt_bloom restated from include/crt.h in float32 numpy: the reference the GPU's bits are held to.  Every line is one
float32 operation in the header's order, on whole levels: the horizontal pass over every row of the parent, then the vertical pass over its
result.  No tile, no halo and no kernel enters it.

    out = bloom(image, inv_count, Params(levels=8, conserve=False, threshold=1.0, clamp=50.0))

`image` is what the device holds, read back (read_sum / read_denoised / read_temporal), so no walk and no layout enters a comparison.
"""
import numpy as np

from integrator_ref import F, f32

SOURCES = ("sum", "denoised", "temporal")


class Params:
    """crt_bloom_params; the defaults are the header's NULL"""

    def __init__(self, source="sum", levels=6, conserve=True, threshold=0.0, clamp=0.0, scatter=0.7, strength=0.05):
        assert source in SOURCES
        self.source, self.levels, self.conserve = source, int(levels), bool(conserve)
        self.threshold, self.clamp, self.scatter, self.strength = f32(threshold), f32(clamp), f32(scatter), f32(strength)

    def kwargs(self):
        """what Scene.bloom takes"""
        return dict(source=self.source, levels=self.levels, conserve=self.conserve, threshold=self.threshold, clamp=self.clamp, scatter=self.scatter,
                    strength=self.strength)


def level_sizes(width, height, levels):
    """[(w_0, h_0), ..., (w_n, h_n)]: n is the largest n <= levels such that every level 1..n has a parent at least 2 wide and 2 high"""
    sizes = [(int(width), int(height))]
    while len(sizes) <= levels and min(sizes[-1]) >= 2:
        w, h = sizes[-1]
        sizes.append(((w + 1) >> 1, (h + 1) >> 1))
    return sizes


def level_count(width, height, levels):
    return len(level_sizes(width, height, levels)) - 1


def input_pixels(image, inv_count, source="sum"):
    """c: image * inv_count for the sum, the image itself for the other two"""
    image = F(image)
    with np.errstate(all="ignore"):
        return F(image * f32(inv_count)) if source == "sum" else image


def luminance(c):
    return F(F(F(f32(0.3) * c[..., 0]) + F(f32(0.6) * c[..., 1])) + F(f32(0.1) * c[..., 2]))


def bright(c, threshold, clamp):
    """b = c * k: k = max(min(L, clamp) - threshold, 0) / max(L, 2^-16), 0 where not L > 0"""
    L = luminance(c)
    Lc = L if f32(clamp) == f32(0.0) else np.minimum(L, f32(clamp))
    k = F(np.maximum(F(Lc - f32(threshold)), f32(0.0)) / np.maximum(L, f32(2.0 ** -16)))
    k = np.where(L > f32(0.0), k, f32(0.0)).astype(f32)
    return F(c * k[..., None])


def _down_axis(a, axis):
    n = a.shape[axis]
    x0 = 2 * np.arange((n + 1) >> 1)
    t = [np.take(a, np.clip(x0 + d, 0, n - 1), axis=axis) for d in (-1, 0, 1, 2)]
    return F(F(F(t[0] + t[3]) + F(f32(3.0) * F(t[1] + t[2]))) * f32(0.125))


def down(a):
    """(h, w, 3) -> ((h + 1) >> 1, (w + 1) >> 1, 3): the 1 3 3 1 filter along x on the parent's rows, then along y on the result"""
    return _down_axis(_down_axis(F(a), 1), 0)


def _up_axis(a, n, axis):
    ns = a.shape[axis]
    x = np.arange(n)
    near = x >> 1
    far = np.clip(np.where(x & 1, near + 1, near - 1), 0, ns - 1)
    return F(F(np.take(a, near, axis=axis) * f32(0.75)) + F(np.take(a, far, axis=axis) * f32(0.25)))


def up(a, w, h):
    """(hs, ws, 3) -> (h, w, 3): 3/4 of the near and 1/4 of the far coarse pixel along x, then along y"""
    return _up_axis(_up_axis(F(a), w, 1), h, 0)


def bloom(image, inv_count, p):
    """one crt_bloom call on `image` (height, width, 3): the bloomed image"""
    with np.errstate(all="ignore"):
        c = input_pixels(image, inv_count, p.source)
        height, width = c.shape[:2]
        sizes = level_sizes(width, height, p.levels)
        n = len(sizes) - 1
        if n == 0:
            return c.copy()
        D = [None, down(bright(c, p.threshold, p.clamp))]
        for k in range(2, n + 1):
            D.append(down(D[k - 1]))
        U = D[n]
        for k in range(n - 1, 0, -1):
            U = F(D[k] + F(F(up(U, *sizes[k]) - D[k]) * p.scatter))
        G = up(U, width, height)
        if p.conserve:
            return F(c + F(F(G - c) * p.strength))
        return F(c + F(G * p.strength))
