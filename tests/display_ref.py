"""crt_display restated from include/crt.h in float32 numpy and Python integers: the reference the GPU's bytes, bins and
exposure bits are held to.  Every float line is one float32 operation in the header's order; the meter is Python integers throughout; the
byte is integrator_ref's, float32(pow(double(y), double(1.0f / 2.2f))) evaluated per value, with no threshold table.

    params = Params(curve="aces", auto=True, adapt=0.25)
    meter = Meter()                                   # the adaptation state of one scene, from create or crt_display_reset on
    rgba, state, hist = display(image, inv_count, params, meter)

`image` is what the device holds, read back (read_sum / read_denoised / read_temporal), so no walk and no layout enters a comparison.
"""
import numpy as np

from integrator_ref import F, f32, _pow_double_once

FIRST_BIN = 111 << 3                  # bits(0x1p-16f) >> 20
CURVES = ("reference", "reinhard", "aces", "clamp")


class Params:
    """crt_display_params; the defaults are the header's NULL"""

    def __init__(self, source="sum", curve="reference", exposure=1.0, auto=False, white=4.0, key=0.18, adapt=1.0, exposure_min=1e-6, exposure_max=1e6,
                 low_permille=0, high_permille=1000):
        assert source in ("sum", "denoised", "temporal") and curve in CURVES
        self.source, self.curve, self.auto = source, curve, bool(auto)
        self.exposure, self.white, self.key, self.adapt = f32(exposure), f32(white), f32(key), f32(adapt)
        self.exposure_min, self.exposure_max = f32(exposure_min), f32(exposure_max)
        self.low_permille, self.high_permille = int(low_permille), int(high_permille)

    def kwargs(self):
        """what Scene.display takes"""
        return dict(source=self.source, curve=self.curve, exposure=self.exposure, auto=self.auto, white=self.white, key=self.key, adapt=self.adapt,
                    exposure_min=self.exposure_min, exposure_max=self.exposure_max, low_permille=self.low_permille, high_permille=self.high_permille)


class Meter:
    """the adaptation: E of the previous metered call and the number of metered calls since create or reset"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.adapted, self.calls = None, 0


def luminance(c):
    """(0.3f*c.x + 0.6f*c.y) + 0.1f*c.z, the resolve's weights and order"""
    c = F(c)
    with np.errstate(all="ignore"):
        return F(F(F(f32(0.3) * c[..., 0]) + F(f32(0.6) * c[..., 1])) + F(f32(0.1) * c[..., 2]))


def input_pixels(image, inv_count, source="sum"):
    """c: image * inv_count for the sum, the image itself for the other two"""
    image = F(image)
    with np.errstate(all="ignore"):
        return F(image * f32(inv_count)) if source == "sum" else image


def bins_of(L):
    """per value: the bin 0..255, or -1 for one that does not count (not finite, or below 0x1p-16f: zero, negatives, NaN)"""
    L = F(L)
    b = np.ascontiguousarray(L).view(np.uint32).astype(np.int64)
    with np.errstate(all="ignore"):
        counts = np.isfinite(L) & (L >= f32(2.0 ** -16))
    return np.where(counts, np.minimum((b >> 20) - FIRST_BIN, 255), -1)


def histogram(L, owned=None):
    """h[256] as Python integers; `owned` (bool per value) leaves out the pixels of other shard ranks"""
    k = bins_of(L).reshape(-1)
    if owned is not None:
        k = k[np.asarray(owned, bool).reshape(-1)]
    return [int(x) for x in np.bincount(k[k >= 0], minlength=256)]


def trimmed(h, low_permille, high_permille):
    """(N, M, S): the counted pixels, how many of them ranks [lo, hi) keep, the sum of the kept pixels' bin indices"""
    N = sum(h)
    lo, hi = N * low_permille // 1000, N * high_permille // 1000
    S, below = 0, 0
    for k, n in enumerate(h):
        first, end = max(below, lo), min(below + n, hi)
        if end > first:
            S += (end - first) * k
        below += n
    return N, hi - lo, S


def float_from_bits(b):
    return np.array([b], np.uint32).view(f32)[0]


def meter_call(h, p, meter):
    """one call with CRT_DISPLAY_AUTO_EXPOSURE on the counts h: advances `meter`, returns the state dict of crt_display_get_state"""
    N, M, S = trimmed(h, p.low_permille, p.high_permille)
    if M == 0:
        E = meter.adapted if meter.calls else p.exposure
        return {"exposure": f32(E), "metered": f32(0.0), "counted": N, "q": 0, "calls": meter.calls}
    Q = S * 256 // M + 128
    L_avg = float_from_bits((FIRST_BIN << 20) + (Q << 12))
    E_target = np.minimum(np.maximum(f32(p.key / L_avg), p.exposure_min), p.exposure_max)
    if meter.calls == 0 or p.adapt == f32(1.0):
        E = f32(E_target)
    else:
        E = f32(meter.adapted + f32(f32(E_target - meter.adapted) * p.adapt))
    meter.adapted, meter.calls = E, meter.calls + 1
    return {"exposure": E, "metered": L_avg, "counted": N, "q": Q, "calls": meter.calls}


def curve(c, E, p):
    """y per channel: x = c * E through the tone curve"""
    with np.errstate(all="ignore"):
        x = F(F(c) * f32(E))
        if p.curve == "clamp":
            return x
        if p.curve == "aces":
            n = F(x * F(F(f32(2.51) * x) + f32(0.03)))
            d = F(F(x * F(F(f32(2.43) * x) + f32(0.59))) + f32(0.14))
            return F(n / d)
        lum = luminance(x)
        if p.curve == "reference":
            k = F(f32(1.0) / F(f32(1.0) + F(lum / f32(2.0))))
        else:
            w2 = f32(p.white * p.white)
            k = F(F(f32(1.0) + F(lum / w2)) / F(f32(1.0) + lum))
        return F(x * k[..., None])


def gamma_bytes(y):
    """the pinned gamma of integrator_ref.resolve_ref: NaN and negatives give 0.  -inf, which a curve's k = 1 / 0 makes of a negative x and
    the resolve never meets, is a negative: libm's pow(-inf, e) is +inf, so it is taken out before."""
    with np.errstate(all="ignore"):
        y = F(y)
        v = _pow_double_once(y, f32(1.0) / f32(2.2))
        v = np.where((v != v) | (y < 0), f32(0.0), v)
        v = np.minimum(np.maximum(v, f32(0.0)), f32(1.0)).astype(f32)
        return F(F(v * f32(255.0)) + f32(0.5)).astype(np.uint8)


def display(image, inv_count, p, meter, owned=None):
    """one crt_display call on `image` (..., 3): (rgba (..., 4) uint8, the state dict, the bins of this call or None for a manual one).
    `owned`: the pixels of this shard rank; the others are not counted and their bytes are 0."""
    c = input_pixels(image, inv_count, p.source)
    if p.auto:
        hist = histogram(luminance(c), owned)
        state = meter_call(hist, p, meter)
    else:
        hist = None
        state = {"exposure": p.exposure, "metered": f32(0.0), "counted": 0, "q": 0, "calls": meter.calls}
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = gamma_bytes(curve(c, state["exposure"], p))
    if owned is not None:
        out[~np.asarray(owned, bool)] = 0
    return out, state, hist


def census(image, inv_count, source="sum"):
    """(occupied bins, pixels not counted) of the image a case meters"""
    k = bins_of(luminance(input_pixels(image, inv_count, source))).reshape(-1)
    return len(set(k[k >= 0].tolist())), int((k < 0).sum())
