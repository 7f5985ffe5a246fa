"""Deformation on the device (include/crt.h crt_deformer_create): linear blend skinning with four influences per
element and morph targets on the positions.  `Deformer` holds the rest pose in HBM and writes posed positions and normals there;
`deform_host` is the same arithmetic on the CPU; `Scene.deform` is the per-frame call that feeds a pose into the refit or rebuild.
"""
import ctypes as C

import numpy as np

from ._lib import CRT_ABI_VERSION, check, crt_deformer_desc, lib
from .host import _ptr

# how the kernel reads the bone palette; the environment variable CRT_DEFORM_PALETTE, read by crt_deformer_create, holds one form against
# the other (tools/deform_probe.py, tests/test_deform.py): "lds" is the default up to 256 bones, "global" above and on request
PALETTE_FORMS = ("global", "lds")


def _morph_arrays(morph_targets):
    """[(vertex indices, deltas), ...] -> target_first, target_vertex, target_delta"""
    first, verts, deltas = [0], [], []
    for idx, d in (morph_targets or []):
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
        if d.shape[0] != idx.shape[0]:
            raise ValueError("a morph target needs one delta per listed vertex")
        verts.append(idx)
        deltas.append(d)
        first.append(first[-1] + idx.shape[0])
    return (np.array(first, np.uint32), np.concatenate(verts) if verts else np.zeros(0, np.uint32),
            np.concatenate(deltas) if deltas else np.zeros((0, 3), np.float32))


class _Desc:
    """A crt_deformer_desc and the arrays it points to, kept alive together."""

    def __init__(self, rest_vertices, vertex_bones, vertex_weights, rest_normals=None, normal_bones=None, normal_weights=None,
                 morph_targets=None, n_bones=None, device=0):
        f32, u16 = np.float32, np.uint16
        self.v = np.ascontiguousarray(rest_vertices, dtype=f32).reshape(-1, 3)
        self.vb = np.ascontiguousarray(vertex_bones, dtype=u16).reshape(-1, 4)
        self.vw = np.ascontiguousarray(vertex_weights, dtype=f32).reshape(-1, 4)
        self.n = None if rest_normals is None else np.ascontiguousarray(rest_normals, dtype=f32).reshape(-1, 3)
        self.nb = None if normal_bones is None else np.ascontiguousarray(normal_bones, dtype=u16).reshape(-1, 4)
        self.nw = None if normal_weights is None else np.ascontiguousarray(normal_weights, dtype=f32).reshape(-1, 4)
        if self.vb.shape[0] != self.v.shape[0] or self.vw.shape[0] != self.v.shape[0]:
            raise ValueError("vertex_bones and vertex_weights need four entries per vertex")
        self.n_normals = 0 if self.n is None else self.n.shape[0]
        for a in (self.nb, self.nw):
            if a is not None and a.shape[0] != self.n_normals:
                raise ValueError("normal_bones and normal_weights need four entries per normal")
        self.first, self.tv, self.td = _morph_arrays(morph_targets)
        self.n_targets = self.first.shape[0] - 1
        if n_bones is None:
            n_bones = 1 + max(int(self.vb.max()) if self.vb.size else 0, int(self.nb.max()) if self.nb is not None and self.nb.size else 0)
        self.n_bones = int(n_bones)
        d = crt_deformer_desc()
        d.abi_version = CRT_ABI_VERSION
        d.rest_vertices, d.n_vertices, d.vertex_bones, d.vertex_weights = _ptr(self.v), self.v.shape[0], _ptr(self.vb), _ptr(self.vw)
        d.rest_normals, d.n_normals, d.normal_bones, d.normal_weights = _ptr(self.n), self.n_normals, _ptr(self.nb), _ptr(self.nw)
        d.n_bones, d.n_targets = self.n_bones, self.n_targets
        d.target_first, d.target_vertex, d.target_delta = (_ptr(self.first) if self.n_targets else None), _ptr(self.tv), _ptr(self.td)
        d.device = int(device)
        self.c = d

    def pose(self, bones, morph_weights):
        b = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1)
        if b.size != 12 * self.n_bones:
            raise ValueError(f"bones must hold {self.n_bones} 3x4 matrices")
        w = None if morph_weights is None else np.ascontiguousarray(morph_weights, dtype=np.float32).reshape(-1)
        if w is not None and w.size != self.n_targets:
            raise ValueError(f"morph_weights must hold {self.n_targets} weights")
        return b, w


def deform_host(bones, rest_vertices, vertex_bones, vertex_weights, rest_normals=None, normal_bones=None, normal_weights=None,
                morph_targets=None, morph_weights=None, n_bones=None):
    """crt_deform_host: the deformer's checks and arithmetic on the CPU, no GPU needed.  Returns (vertices, normals); normals is None
    without rest_normals.  n_bones None: as many as `bones` holds."""
    if n_bones is None:
        n_bones = np.asarray(bones).size // 12
    d = _Desc(rest_vertices, vertex_bones, vertex_weights, rest_normals, normal_bones, normal_weights, morph_targets, n_bones)
    b, w = d.pose(bones, morph_weights)
    out_v = np.zeros((d.v.shape[0], 3), np.float32)
    out_n = np.zeros((d.n_normals, 3), np.float32) if d.n_normals else None
    check(lib().crt_deform_host(C.byref(d.c), _ptr(b), _ptr(w), _ptr(out_v), _ptr(out_n)))
    return out_v, out_n


class Deformer:
    """crt_deformer: rest pose, influences and morph targets uploaded once; pose() writes the deformed positions and normals in HBM.
    morph_targets: a list of (vertex indices ascending, deltas (k, 3)) pairs.  bones: (n_bones, 3, 4) skinning matrices."""

    def __init__(self, rest_vertices, vertex_bones, vertex_weights, rest_normals=None, normal_bones=None, normal_weights=None,
                 morph_targets=None, n_bones=None, device=0):
        self._h = C.c_void_p()
        d = _Desc(rest_vertices, vertex_bones, vertex_weights, rest_normals, normal_bones, normal_weights, morph_targets, n_bones, device)
        self._d = d
        self.n_vertices, self.n_normals, self.n_bones, self.n_targets = d.v.shape[0], d.n_normals, d.n_bones, d.n_targets
        check(lib().crt_deformer_create(C.byref(d.c), C.byref(self._h)))

    def pose(self, bones, morph_weights=None, sync=True):
        """crt_deformer_pose on the deformer's own stream."""
        b, w = self._d.pose(bones, morph_weights)
        check(lib().crt_deformer_pose(self._h, _ptr(b), _ptr(w), 1 if sync else 0))

    def sync(self):
        check(lib().crt_deformer_sync(self._h))

    @property
    def vertices_ptr(self):
        """device address of the posed positions (n_vertices x 3 float32), valid until close()"""
        p = C.c_void_p()
        check(lib().crt_deformer_vertices_device(self._h, C.byref(p)))
        return p.value

    @property
    def normals_ptr(self):
        """device address of the posed normals (n_normals x 3 float32), None for a deformer without normals"""
        p = C.c_void_p()
        check(lib().crt_deformer_normals_device(self._h, C.byref(p)))
        return p.value

    def read(self):
        """(vertices, normals) of the last pose; normals is None for a deformer without normals."""
        v = np.zeros((self.n_vertices, 3), np.float32)
        n = np.zeros((self.n_normals, 3), np.float32) if self.n_normals else None
        check(lib().crt_deformer_read(self._h, _ptr(v), v.size, _ptr(n), 0 if n is None else n.size))
        return v, n

    def last_ms(self):
        """stream time of the last pose's kernel, ms"""
        ms = C.c_float()
        check(lib().crt_deformer_last_ms(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if self._h:
            lib().crt_deformer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def normal_influences(triangles, vertex_bones, vertex_weights, n_normals):
    """Influences for the normals of a mesh whose triangles index positions and normals apart (crt_triangle: v = t[0:3], vn = t[4:7],
    t[7] == 1 where the corners carry normals): each normal takes those of the vertex at the first corner that uses it, by lowest
    triangle index, then lowest corner.  A normal no corner uses gets bone 0 with weight 1."""
    t = np.asarray(triangles).reshape(-1, 12)
    vb = np.ascontiguousarray(vertex_bones, dtype=np.uint16).reshape(-1, 4)
    vw = np.ascontiguousarray(vertex_weights, dtype=np.float32).reshape(-1, 4)
    nb = np.zeros((int(n_normals), 4), np.uint16)
    nw = np.zeros((int(n_normals), 4), np.float32)
    nw[:, 0] = 1.0
    has = t[:, 7] == 1
    vn = t[has][:, 4:7].reshape(-1).astype(np.int64)      # corner order: triangle, then corner
    v = t[has][:, 0:3].reshape(-1).astype(np.int64)
    uniq, first = np.unique(vn, return_index=True)        # the first occurrence of every used normal
    ok = (uniq >= 0) & (uniq < int(n_normals))
    nb[uniq[ok]] = vb[v[first[ok]]]
    nw[uniq[ok]] = vw[v[first[ok]]]
    return nb, nw
