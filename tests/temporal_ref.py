"""crt_temporal's definition in plain vectorised float32 numpy: the reference the GPU is held to by bytes.  Not a test, and
no code shared with the kernel: every intermediate is a float32 array, every step one IEEE float32 operation in the order DESIGN writes
it.  Step 1 (filterable, unit normal, key, x and the divisor) is denoise_ref.prepare's, as §23 says it is k_denoise_prepare's.

temporal_ref(state, source, aov, d, view, o2w, w2o, params) -> (image (H, W, 3), N (H, W), new state, census)
  state   None (no history) or what an earlier call returned
  source  (H, W, 3) float32: c, the source pixel (the sum times inv_count, or the denoised image)
  aov     Scene.read_aov's arrays under "HIT", "IDS", "NORMAL", "ALBEDO"
  d       (H, W, 3) float32: the primary-ray directions of the view HIT was rendered from (the oracle's primary_rays)
  view    view_record(camera, W, H): pos, right, up, fwd, aspect_tan, tan_fov
  o2w, w2o  None for a flat scene, else (n, 3, 4) float32: the live object_to_world / world_to_object
  params  dict(demodulate, clamp, max_history, sigma_depth, normal_min)
census counts, over F pixels: new_instance, behind, off_frame, low_weight (sw < 0.01), with_history, without_history, clamped (pixels
whose h the clamp changed), moved (pixels that took the matrix path) and, per (pixel, tap) pair of the pixels that reached the taps,
tap_edge, tap_key, tap_normal, tap_depth, tap_counted."""
import ctypes as C
import ctypes.util

import numpy as np

from denoise_ref import prepare, shifted

f32 = np.float32
DEFAULTS = dict(demodulate=True, clamp=False, max_history=32, sigma_depth=0.1, normal_min=0.9)
CENSUS = ("new_instance", "behind", "off_frame", "low_weight", "tap_edge", "tap_key", "tap_normal", "tap_depth", "tap_counted", "with_history",
          "without_history", "clamped", "moved")


def tanf(x):
    """the C library's float tangent: what the host forms tan_fov with"""
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.tanf.restype, m.tanf.argtypes = C.c_float, [C.c_float]
    return f32(m.tanf(float(f32(x))))


def view_record(camera, W, H):
    """the view as the library records it at crt_render_aov: aspect_tan and tan_fov formed as FrameArgs' are"""
    c = camera.c if hasattr(camera, "c") else camera
    tan_fov = tanf(f32(c.fov) * f32(0.5))
    return dict(pos=np.array(c.position[:], f32), right=np.array(c.right[:], f32), up=np.array(c.up[:], f32), fwd=np.array(c.forward[:], f32),
                aspect_tan=f32(f32(f32(W) / f32(H)) * tan_fov), tan_fov=tan_fov)


def dot3(a, b):
    s = ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32)
    return (s + (a[..., 2] * b[..., 2]).astype(f32)).astype(f32)


def rows_point(M, a):
    """M (..., 3, 4) applied to the points a (..., 3): each row ((m0*a0 + m1*a1) + m2*a2) + m3"""
    out = []
    for r in range(3):
        s = ((M[..., r, 0] * a[..., 0]).astype(f32) + (M[..., r, 1] * a[..., 1]).astype(f32)).astype(f32)
        s = (s + (M[..., r, 2] * a[..., 2]).astype(f32)).astype(f32)
        out.append((s + M[..., r, 3]).astype(f32))
    return np.stack(out, -1)


def temporal_ref(state, source, aov, d, view, o2w, w2o, params):
    p = dict(DEFAULTS, **params)
    dem, clamp, maxh = bool(p["demodulate"]), bool(p["clamp"]), int(p["max_history"])
    sigma_depth, normal_min = f32(p["sigma_depth"]), f32(p["normal_min"])
    c, x, m, unit, t, key, F = prepare(source, aov, 1.0, dem)
    H, W = F.shape
    d = np.asarray(d, f32).reshape(H, W, 3)
    census = dict.fromkeys(CENSUS, 0)
    y, N = x.copy(), np.ones((H, W), f32)
    if o2w is not None:
        o2w, w2o = np.asarray(o2w, f32).reshape(-1, 3, 4), np.asarray(w2o, f32).reshape(-1, 3, 4)
    # history-less: no state, a change of the DEMODULATE bit, max_history 1
    if state is not None and state["demodulate"] == dem and maxh > 1:
        with np.errstate(all="ignore"):
            alive = F.copy()
            X = (view["pos"] + (d * t[..., None]).astype(f32)).astype(f32)
            Xp = X
            if o2w is not None:
                inst = aov["IDS"]["instance"].astype(np.int64)
                prev = state["o2w"]
                n = min(prev.shape[0], o2w.shape[0])
                new = alive & ((inst >= prev.shape[0]) | (inst >= o2w.shape[0]))
                census["new_instance"] = int(new.sum())
                alive &= ~new
                if n and alive.any():
                    ii = np.where(alive, inst, 0)
                    changed = (o2w[:n].reshape(n, 12).view(np.uint32) != prev[:n].reshape(n, 12).view(np.uint32)).any(1)
                    moved = alive & changed[ii]
                    census["moved"] = int(moved.sum())
                    Xp = np.where(moved[..., None], rows_point(prev[ii], rows_point(w2o[ii], X)), X).astype(f32)
            pv = state["view"]
            v = (Xp - pv["pos"]).astype(f32)
            cz, cx, cy = dot3(v, pv["fwd"]), dot3(v, pv["right"]), dot3(v, pv["up"])
            behind = alive & ~(cz > 0)
            census["behind"] = int(behind.sum())
            alive &= ~behind
            tp = np.sqrt(dot3(v, v)).astype(f32)
            Wf, Hf = f32(W), f32(H)
            fx = ((((((cx / cz).astype(f32) / pv["aspect_tan"]).astype(f32) + f32(1)).astype(f32) * f32(0.5)).astype(f32) * Wf).astype(f32) - f32(0.5)).astype(f32)
            fy = ((((((cy / cz).astype(f32) / pv["tan_fov"]).astype(f32) + f32(1)).astype(f32) * f32(0.5)).astype(f32) * Hf).astype(f32) - f32(0.5)).astype(f32)
            off = alive & ~((fx > f32(-1)) & (fx < Wf) & (fy > f32(-1)) & (fy < Hf))
            census["off_frame"] = int(off.sum())
            alive &= ~off
            fx, fy = np.where(alive, fx, f32(0)).astype(f32), np.where(alive, fy, f32(0)).astype(f32)
            x0, y0 = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
            ax, ay = (fx - x0).astype(f32), (fy - y0).astype(f32)
            wx, wy = ((f32(1) - ax).astype(f32), ax), ((f32(1) - ay).astype(f32), ay)
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            tol = (sigma_depth * tp).astype(f32)
            sw, acc, an = np.zeros((H, W), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    kq, gq, hq = state["key"][qyc, qxc], state["guide"][qyc, qxc], state["hist"][qyc, qxc]
                    edge = alive & ~inside
                    keycut = alive & inside & (kq != key)
                    rest = alive & inside & (kq == key)
                    ncut = rest & ~(dot3(unit, gq) >= normal_min)
                    rest &= ~ncut
                    dcut = rest & ~(np.abs((gq[..., 3] - tp).astype(f32)) <= tol)
                    use = rest & ~dcut
                    for name, mask in (("tap_edge", edge), ("tap_key", keycut), ("tap_normal", ncut), ("tap_depth", dcut), ("tap_counted", use)):
                        census[name] += int(mask.sum())
                    b = (wx[i] * wy[j]).astype(f32)
                    sw = np.where(use, (sw + b).astype(f32), sw)
                    acc = np.where(use[..., None], (acc + (b[..., None] * hq[..., :3]).astype(f32)).astype(f32), acc)
                    an = np.where(use, (an + (b * hq[..., 3]).astype(f32)).astype(f32), an)
            low = alive & ~(sw >= f32(0.01))
            census["low_weight"] = int(low.sum())
            alive &= ~low
            h = (acc / sw[..., None]).astype(f32)
            nh = (an / sw).astype(f32)
            if clamp:
                lo, hi = x.copy(), x.copy()
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if dx == 0 and dy == 0:
                            continue
                        xq, inside = shifted(x, dx, dy)
                        kq, _ = shifted(key, dx, dy)
                        ok = inside & (kq == key)
                        lo = np.where(ok[..., None], np.minimum(lo, xq), lo)
                        hi = np.where(ok[..., None], np.maximum(hi, xq), hi)
                hc = np.minimum(np.maximum(h, lo), hi).astype(f32)
                census["clamped"] = int((alive & (hc.view(np.uint32) != h.view(np.uint32)).any(2)).sum())
                h = hc
            Nh = np.minimum((nh + f32(1)).astype(f32), f32(maxh)).astype(f32)
            a = (f32(1) / Nh).astype(f32)
            yh = (h + (a[..., None] * (x - h).astype(f32)).astype(f32)).astype(f32)
            y = np.where(alive[..., None], yh, x).astype(f32)
            N = np.where(alive, Nh, f32(1)).astype(f32)
            census["with_history"] = int(alive.sum())
    census["without_history"] = int(F.sum()) - census["with_history"]
    image = np.where(F[..., None], (y * m).astype(f32), y).astype(f32)
    new_state = dict(hist=np.concatenate([y, N[..., None]], 2).astype(f32), guide=np.concatenate([unit, t[..., None]], 2).astype(f32), key=key.copy(),
                     view=dict(view), o2w=None if o2w is None else o2w.copy(), demodulate=dem)
    assert image.dtype == f32 and N.dtype == f32 and new_state["hist"].dtype == f32
    return image, N, new_state, census
