"""The deformer's definition (include/crt.h, "Deformation on the device") in float32 numpy on whole arrays: every line below is one
IEEE float32 operation per element in the header's order, numpy rounds each ufunc result once and fuses nothing, and its float32
square root and division are correctly rounded.  Written from the header, not from the kernel or the host entry."""
import numpy as np

f32 = np.float32
L2_MIN = f32(2.0) ** f32(-126)      # 0x1p-126f


def _blend(bones, b, w):
    """M (n, 12): w_0 * B[b_0], then + w_k * B[b_k] for k = 1, 2, 3 where w_k != 0"""
    B = np.ascontiguousarray(bones, f32).reshape(-1, 12)
    b = np.asarray(b).reshape(-1, 4).astype(np.int64)
    w = np.ascontiguousarray(w, f32).reshape(-1, 4)
    M = (w[:, 0:1] * B[b[:, 0]]).astype(f32)
    for k in (1, 2, 3):
        on = w[:, k] != 0
        prod = (w[on, k:k + 1] * B[b[on, k]]).astype(f32)
        M[on] = (M[on] + prod).astype(f32)
    return M


def deform_ref(bones, rest_vertices, vertex_bones, vertex_weights, rest_normals=None, normal_bones=None, normal_weights=None,
               morph_targets=None, morph_weights=None):
    """-> (vertices (n, 3), normals (m, 3) or None).  morph_targets: [(vertex indices strictly ascending, deltas (k, 3)), ...];
    morph_weights None = all zeros, and the arithmetic still applies (0 * d is added)."""
    with np.errstate(all="ignore"):
        p = np.ascontiguousarray(rest_vertices, f32).reshape(-1, 3).copy()
        targets = list(morph_targets or [])
        mw = np.zeros(len(targets), f32) if morph_weights is None else np.ascontiguousarray(morph_weights, f32).reshape(-1)
        for t, (idx, d) in enumerate(targets):                 # ascending t; a target lists a vertex at most once
            idx = np.asarray(idx).astype(np.int64).reshape(-1)
            d = np.ascontiguousarray(d, f32).reshape(-1, 3)
            p[idx] = (p[idx] + (mw[t] * d).astype(f32)).astype(f32)
        M = _blend(bones, vertex_bones, vertex_weights)
        out = np.empty_like(p)
        for r in range(3):
            a = ((M[:, 4 * r] * p[:, 0]).astype(f32) + (M[:, 4 * r + 1] * p[:, 1]).astype(f32)).astype(f32)
            a = (a + (M[:, 4 * r + 2] * p[:, 2]).astype(f32)).astype(f32)
            out[:, r] = (a + M[:, 4 * r + 3]).astype(f32)
        if rest_normals is None:
            return out, None
        n = np.ascontiguousarray(rest_normals, f32).reshape(-1, 3)
        M = _blend(bones, normal_bones, normal_weights)
        q = np.empty_like(n)
        for r in range(3):
            a = ((M[:, 4 * r] * n[:, 0]).astype(f32) + (M[:, 4 * r + 1] * n[:, 1]).astype(f32)).astype(f32)
            q[:, r] = (a + (M[:, 4 * r + 2] * n[:, 2]).astype(f32)).astype(f32)
        l2 = ((q[:, 0] * q[:, 0]).astype(f32) + (q[:, 1] * q[:, 1]).astype(f32)).astype(f32)
        l2 = (l2 + (q[:, 2] * q[:, 2]).astype(f32)).astype(f32)
        unit = (l2 >= L2_MIN) & np.isfinite(l2)
        length = np.sqrt(np.where(unit, l2, f32(1.0))).astype(f32)
        nout = np.where(unit[:, None], (q / length[:, None]).astype(f32), q).astype(f32)
        return out, nout
