"""crt_denoise's definition in plain vectorised float32 numpy: the reference the GPU is held to by bytes.  Not a test, and
no code shared with the kernels: every intermediate is a float32 array, every step one IEEE float32 operation in the order DESIGN writes
it, so numpy's correctly rounded add / subtract / multiply / divide / sqrt give what the device must give.

denoise_ref(sum, aov, inv_count, ...) -> (image (H, W, 3) float32, census): `aov` holds Scene.read_aov's arrays under "HIT", "IDS",
"NORMAL", "ALBEDO".  census[i] counts, over pass i's (filterable pixel, off-centre tap) pairs, what cut them: the frame edge, an
unfilterable neighbour, another key; and over the pairs none of those cut, per edge-stopping term, how many it set to 0 and how many it
left strictly inside (0, 1)."""
import numpy as np

f32 = np.float32
KERNEL = (f32(0.375), f32(0.25), f32(0.0625))
DEFAULTS = dict(passes=5, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7)


def shifted(a, ox, oy):
    """b[y, x] = a[y + oy, x + ox] where that lies in the frame (else 0), and the mask of where it does"""
    H, W = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((H, W), bool)
    x0, x1, y0, y1 = max(0, -ox), min(W, W - ox), max(0, -oy), min(H, H - oy)
    if x0 < x1 and y0 < y1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def prepare(total, aov, inv_count, demodulate):
    """(c, x, divisor, unit normal, t, key, filterable) per pixel"""
    S = np.asarray(total, f32)
    c = (S * f32(inv_count)).astype(f32)
    hit, ids = aov["HIT"], aov["IDS"]
    n = np.asarray(aov["NORMAL"], f32)[..., :3]
    albedo = np.asarray(aov["ALBEDO"], f32)[..., :3]
    with np.errstate(all="ignore"):
        nn = ((n[..., 0] * n[..., 0]).astype(f32) + (n[..., 1] * n[..., 1]).astype(f32)).astype(f32)
        nn = (nn + (n[..., 2] * n[..., 2]).astype(f32)).astype(f32)
        F = (hit["tri"] >= 0) & (hit["t"] >= f32(1e-20)) & ((ids["flags"] & 2) == 0) & (nn > 0) & (nn < f32(np.inf))
        r = (f32(1.0) / np.sqrt(np.where(F, nn, f32(1.0))).astype(f32)).astype(f32)
        unit = (n * r[..., None]).astype(f32)
        d = np.maximum(albedo, f32(1e-3)).astype(f32) if demodulate else np.ones_like(albedo)
        x = np.where(F[..., None], (c / d).astype(f32), c).astype(f32)
    t = np.where(F, hit["t"], f32(0)).astype(f32)
    key = np.where(F, ids["instance"].astype(np.int64) + 1, 0)
    unit = np.where(F[..., None], unit, f32(0)).astype(f32)
    return c, x, d, unit, t, key, F


def one_pass(x, unit, t, key, F, i, sigma_color, sigma_depth, normal_power_log2):
    s = 1 << i
    use_color = f32(sigma_color) != 0
    if use_color:
        sigma_i = f32(f32(sigma_color) * f32(2.0 ** -i))
        inv_c = f32(f32(1.0) / f32(sigma_i * sigma_i))
    with np.errstate(all="ignore"):
        r1 = (f32(1.0) / ((f32(sigma_depth) * t).astype(f32) * f32(s)).astype(f32)).astype(f32)
        r2 = (r1 * f32(0.5)).astype(f32)
    acc = np.zeros_like(x)
    sw = np.zeros(x.shape[:2], f32)
    census = dict(pairs=0, edge=0, unfilterable=0, key=0, normal_zero=0, normal_partial=0, depth_zero=0, depth_partial=0, color_zero=0, color_partial=0)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            xq, inside = shifted(x, s * dx, s * dy)
            nq, _ = shifted(unit, s * dx, s * dy)
            tq, _ = shifted(t, s * dx, s * dy)
            kq, _ = shifted(key, s * dx, s * dy)
            Fq, _ = shifted(F, s * dx, s * dy)
            use = F & inside & Fq & (kq == key)
            terms = {}
            with np.errstate(all="ignore"):
                w = np.full(sw.shape, f32(KERNEL[abs(dx)] * KERNEL[abs(dy)]), f32)
                a = ((unit[..., 0] * nq[..., 0]).astype(f32) + (unit[..., 1] * nq[..., 1]).astype(f32)).astype(f32)
                a = (a + (unit[..., 2] * nq[..., 2]).astype(f32)).astype(f32)
                a = np.maximum(a, f32(0)).astype(f32)
                for _ in range(normal_power_log2):
                    a = (a * a).astype(f32)
                w = (w * a).astype(f32)
                terms["normal"] = a
                m = max(abs(dx), abs(dy))
                if m > 0:
                    z = (np.abs((t - tq).astype(f32)).astype(f32) * (r1 if m == 1 else r2)).astype(f32)
                    g = np.maximum((f32(1.0) - (z * z).astype(f32)).astype(f32), f32(0)).astype(f32)
                    gg = (g * g).astype(f32)
                    w = (w * gg).astype(f32)
                    terms["depth"] = gg
                if use_color:
                    e = (x - xq).astype(f32)
                    d2 = ((e[..., 0] * e[..., 0]).astype(f32) + (e[..., 1] * e[..., 1]).astype(f32)).astype(f32)
                    d2 = (d2 + (e[..., 2] * e[..., 2]).astype(f32)).astype(f32)
                    g = np.maximum((f32(1.0) - (d2 * inv_c).astype(f32)).astype(f32), f32(0)).astype(f32)
                    gg = (g * g).astype(f32)
                    w = (w * gg).astype(f32)
                    terms["color"] = gg
                acc = np.where(use[..., None], (acc + (w[..., None] * xq).astype(f32)).astype(f32), acc)
                sw = np.where(use, (sw + w).astype(f32), sw)
            if m > 0:
                census["pairs"] += int(F.sum())
                census["edge"] += int((F & ~inside).sum())
                census["unfilterable"] += int((F & inside & ~Fq).sum())
                census["key"] += int((F & inside & Fq & (kq != key)).sum())
                for name, v in terms.items():
                    census[name + "_zero"] += int((use & (v == 0)).sum())
                    census[name + "_partial"] += int((use & (v > 0) & (v < 1)).sum())
    with np.errstate(all="ignore"):
        out = np.where(F[..., None], (acc / sw[..., None]).astype(f32), x).astype(f32)
    assert out.dtype == f32 and acc.dtype == f32 and sw.dtype == f32
    return out, census


def denoise_ref(total, aov, inv_count, passes=5, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7):
    c, x, d, unit, t, key, F = prepare(total, aov, inv_count, demodulate)
    census = []
    for i in range(passes):
        x, cs = one_pass(x, unit, t, key, F, i, sigma_color, sigma_depth, normal_power_log2)
        census.append(cs)
    out = np.where(F[..., None], (x * d).astype(f32), c).astype(f32)
    assert out.dtype == f32
    return out, census


def filterable(aov):
    z = np.zeros(aov["HIT"].shape + (3,), f32)
    return prepare(z, aov, 1.0, False)[6]
