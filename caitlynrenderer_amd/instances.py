"""Instanced scenes: one bottom-level CWBVH per mesh, built once on the device, under a top-level CWBVH over transformed instances that
is rebuilt on the device at every `set` (include/crt.h crt_instances_*) or refitted in place by `refit`, which moves the
instances and keeps the TLAS's topology (§13).  An updatable scene also moves the vertices of its meshes: a GPU refit of their BLASes and a
TLAS rebuild per update.  Instances carry 8-bit visibility masks that a masked trace ANDs with each ray's (§14).  Meshes
can be appended to a live scene and, in an updatable one, replaced by new geometry (§15).  The handle answers ray queries; `frame_scene`
returns a Scene that renders frames of it (§16); those frames add each instance's material offset to its triangles' material indices and,
with the scene's option "instance_masks", walk masked per ray class (§17).  Meshes may carry lights that follow their instances (§18)."""
import ctypes as C

import numpy as np

from ._lib import (CRT_ABI_VERSION, CRT_BUILD_LBVH_ON_DEVICE, CRT_BUILD_PLOC, CRT_BUILD_SAH, CRT_INSTANCES_UPDATABLE, CRT_TRACE_CLOSEST,
                   CRT_TRACE_INSTANCE_MASK, check, crt_blas_desc, crt_instanced_scene_desc, crt_instances_info, crt_mesh_lights, crt_mesh_shading,
                   crt_tree_cost, lib)
from .host import Rnd, _cost_dict, _ptr
from .scene import HIT_DT, RAY_DT, STATS_DT, Scene

# crt_instance, 64 B.  material_offset is the first of the two reserved words (byte 56): the fields overlap
INSTANCE_DT = np.dtype({"names": ["object_to_world", "mesh", "mask", "reserved", "material_offset"],
                        "formats": [("<f4", 12), "<u4", "<u4", ("<u4", 2), "<u4"],
                        "offsets": [0, 48, 52, 56, 56], "itemsize": 64})


def instances_array(matrices, meshes, masks=None, material_offsets=None):
    """crt_instance records from (n, 3, 4) or (n, 12) object_to_world matrices (row-major, world = A p + t), n mesh indices and, optionally,
    n visibility masks (bits 0..7; read by masked traces and by the frames of a scene with `instance_masks` 1) and n
    material offsets (added to the material index of every triangle of the instance's mesh by the frames of a bound scene, §17).  Without
    them the mask and offset words stay 0."""
    m = np.asarray(matrices, np.float32).reshape(-1, 12)
    out = np.zeros(m.shape[0], INSTANCE_DT)
    out["object_to_world"] = m
    out["mesh"] = np.asarray(meshes, np.uint32).reshape(-1)
    if masks is not None:
        out["mask"] = np.asarray(masks, np.uint32).reshape(-1)
    if material_offsets is not None:
        out["material_offset"] = np.asarray(material_offsets, np.uint32).reshape(-1)
    return out


def _records(instances):
    """a contiguous INSTANCE_DT array of crt_instance records given as INSTANCE_DT or as any other 64-byte layout of the struct (e.g. the
    fields without `material_offset`): the bytes are taken as they are"""
    a = np.asarray(instances)
    if a.dtype != INSTANCE_DT and a.dtype.itemsize == INSTANCE_DT.itemsize:
        return np.ascontiguousarray(a).view(INSTANCE_DT).reshape(-1)
    return np.ascontiguousarray(a, INSTANCE_DT)


def _build_flags(builder):
    f = CRT_BUILD_LBVH_ON_DEVICE
    if builder.startswith("ploc"):
        f |= CRT_BUILD_PLOC | ((int(builder[4:]) if len(builder) > 4 else 0) << 8)
    elif builder.startswith("sah"):
        f |= CRT_BUILD_SAH | ((int(builder[3:]) if len(builder) > 3 else 0) << 8)
    elif builder != "lbvh":
        raise ValueError(f"unknown builder {builder!r}")
    return f


def instance_inverse(object_to_world):
    """crt_instance_inverse [host]: world_to_object (12 floats) of a 3x4 object_to_world."""
    m = np.ascontiguousarray(object_to_world, np.float32).reshape(12)
    w = np.empty(12, np.float32)
    check(lib().crt_instance_inverse(_ptr(m), _ptr(w)))
    return w


def instance_world_box(object_to_world, box):
    """crt_instance_world_box [host]: the padded world box (lo[3], hi[3]) of an object box (lo[3], hi[3])."""
    m = np.ascontiguousarray(object_to_world, np.float32).reshape(12)
    b = np.ascontiguousarray(box, np.float32).reshape(6)
    out = np.empty(6, np.float32)
    check(lib().crt_instance_world_box(_ptr(m), _ptr(b), _ptr(out)))
    return out


def instance_lights(object_to_world, lights):
    """crt_instance_lights [host]: (n, 18) object-space lights through a 3x4 object_to_world, bit for bit the device's arithmetic
    (DESIGN.md §18): area set, the pdf column left 0 for lights_finish."""
    m = np.ascontiguousarray(object_to_world, np.float32).reshape(12)
    src = np.ascontiguousarray(lights, np.float32).reshape(-1, 18)
    out = np.empty_like(src)
    check(lib().crt_instance_lights(_ptr(m), _ptr(src), src.shape[0], _ptr(out)))
    return out


def lights_finish(lights):
    """crt_lights_finish [host]: a copy of an (n, 18) light table with its pdf column (index 16) filled by the tree-sum rule."""
    out = np.array(lights, np.float32).reshape(-1, 18)
    check(lib().crt_lights_finish(_ptr(out), out.shape[0]))
    return out


def _blas_descs(meshes):
    """-> (crt_blas_desc array, the arrays it points into) of Mesh objects or (vertices, triangles) pairs"""
    descs = (crt_blas_desc * max(len(meshes), 1))()
    keep = []
    for k, m in enumerate(meshes):
        v, t = (m.vertices, m.triangles) if hasattr(m, "vertices") else m
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        t = np.asarray(t, np.int32)
        if t.ndim == 2 and t.shape[1] == 3:
            t = np.concatenate([t, np.zeros((t.shape[0], 9), np.int32)], 1)
        t = np.ascontiguousarray(t, np.int32).reshape(-1, 12)
        keep += [v, t]
        descs[k].vertices, descs[k].n_vertices = _ptr(v), v.shape[0]
        descs[k].triangles, descs[k].n_triangles = _ptr(t), t.shape[0]
    return descs, keep


def set_mesh_lights(scene, mesh, lights):
    """crt_scene_set_mesh_lights: new OBJECT-space lights (same count) for one mesh of a frame_scene with mesh_lights; call reset()"""
    la = np.ascontiguousarray(lights, np.float32).reshape(-1, 18)
    check(lib().crt_scene_set_mesh_lights(scene._h, int(mesh), _ptr(la) if la.shape[0] else None, la.shape[0]))


def read_lights(scene):
    """crt_scene_read_lights: the (n, 18) float32 world light table the next frame of a frame_scene samples (rebuilt first if stale)"""
    n = C.c_size_t()
    check(lib().crt_scene_read_lights(scene._h, None, 0, C.byref(n)))
    out = np.empty((n.value, 18), np.float32)
    if n.value:
        check(lib().crt_scene_read_lights(scene._h, _ptr(out), n.value, C.byref(n)))
    return out


class InstancedScene:
    """meshes: Mesh objects (or (vertices, triangles) pairs, triangles (n, 12) int32 or (n, 3)); instances: an INSTANCE_DT array
    (instances_array); capacity: the most instances a later `set` may hold (default: len(instances)); builder: "sah", "ploc", "lbvh";
    updatable: keep the refit state of update_meshes (CRT_INSTANCES_UPDATABLE)."""

    def __init__(self, meshes, instances, capacity=None, builder="sah", updatable=False):
        self._h = C.c_void_p()
        descs, keep = _blas_descs(meshes)
        inst = _records(instances)
        cap = inst.shape[0] if capacity is None else int(capacity)
        flags = _build_flags(builder) | (CRT_INSTANCES_UPDATABLE if updatable else 0)
        check(lib().crt_instances_create(descs, len(meshes), _ptr(inst), inst.shape[0], cap, flags, C.byref(self._h)))
        del keep

    def set(self, instances):
        inst = _records(instances)
        check(lib().crt_instances_set(self._h, _ptr(inst), inst.shape[0]))

    def set_device(self, ptr, n, sync=True):
        """instances already in device memory (e.g. a torch uint8 / float tensor of n * 64 bytes: pass tensor.data_ptr())."""
        check(lib().crt_instances_set_device(self._h, C.c_void_p(ptr), int(n), 1 if sync else 0))

    def refit(self, instances):
        """same count, new matrices (and meshes): the TLAS refitted in place, its topology kept (crt_instances_refit)"""
        inst = _records(instances)
        check(lib().crt_instances_refit(self._h, _ptr(inst), inst.shape[0]))

    def refit_device(self, ptr, n, sync=True):
        """refit from instances already in device memory (n * 64 bytes at ptr)"""
        check(lib().crt_instances_refit_device(self._h, C.c_void_p(ptr), int(n), 1 if sync else 0))

    def update_meshes(self, vertices_by_mesh):
        """{mesh index: (n, 3) float32 positions in the create's order}: one crt_instances_update_meshes call for all of them."""
        ids = np.array(list(vertices_by_mesh.keys()), np.uint32)
        vs = [np.ascontiguousarray(v, np.float32).reshape(-1, 3) for v in vertices_by_mesh.values()]
        ptrs = (C.c_void_p * max(len(vs), 1))(*[v.ctypes.data for v in vs])
        counts = np.array([v.shape[0] for v in vs], np.uint64)
        check(lib().crt_instances_update_meshes(self._h, _ptr(ids), len(vs), ptrs, _ptr(counts)))

    def add_meshes(self, meshes):
        """appends meshes (what the constructor takes) to the live scene -> the index of the first; instances, the TLAS and the existing
        BLASes stay (crt_instances_add_meshes)"""
        meshes = list(meshes)
        descs, keep = _blas_descs(meshes)
        first = C.c_uint32()
        check(lib().crt_instances_add_meshes(self._h, descs, len(meshes), C.byref(first)))
        del keep
        return first.value

    def replace_meshes(self, meshes_by_index):
        """{mesh index: mesh}: new geometry (any vertex and triangle count) for existing meshes, each BLAS rebuilt from scratch and the TLAS
        rebuilt over the live instances (crt_instances_replace_meshes; updatable scenes only)"""
        ids = np.array(list(meshes_by_index.keys()), np.uint32)
        descs, keep = _blas_descs(list(meshes_by_index.values()))
        check(lib().crt_instances_replace_meshes(self._h, _ptr(ids), ids.shape[0], descs))
        del keep

    def update_mesh(self, k, vertices):
        self.update_meshes({k: vertices})

    def update_meshes_device(self, ptrs_by_mesh, sync=True):
        """{mesh index: (device pointer, n_vertices)}: positions already in device memory (e.g. a torch float32 tensor's data_ptr())."""
        ids = np.array(list(ptrs_by_mesh.keys()), np.uint32)
        items = list(ptrs_by_mesh.values())
        ptrs = (C.c_void_p * max(len(items), 1))(*[int(p) for p, _ in items])
        counts = np.array([int(nv) for _, nv in items], np.uint64)
        check(lib().crt_instances_update_meshes_device(self._h, _ptr(ids), len(items), ptrs, _ptr(counts), 1 if sync else 0))

    def tree_cost(self, mesh=-1):
        """crt_instances_tree_cost: the SAH cost (a dict of crt_tree_cost's fields) of the live TLAS (mesh = -1) or of mesh m's BLAS,
        computed on the device.  A TLAS's cost compares TLASes over the same instances only."""
        c = crt_tree_cost()
        check(lib().crt_instances_tree_cost(self._h, int(mesh), C.byref(c)))
        return _cost_dict(c)

    def last_update(self):
        """{device_ms, wall_ms, state_bytes} of the last update (crt_instances_last_update)"""
        d, w, b = C.c_float(), C.c_float(), C.c_uint64()
        check(lib().crt_instances_last_update(self._h, C.byref(d), C.byref(w), C.byref(b)))
        return {"device_ms": d.value, "wall_ms": w.value, "state_bytes": b.value}

    def trace(self, rays, mode=CRT_TRACE_CLOSEST, stats=False, ray_mask=None):
        """-> (hits HIT_DT, instance ids int32 (-1 = miss)[, stats STATS_DT]).  ray_mask: None (masks ignored), or an int or a per-ray
        uint8 array, written into a copy of the rays' pad words, and the trace sees only the instances whose mask meets it
        (CRT_TRACE_INSTANCE_MASK)."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DT)
        n = rays.shape[0]
        if ray_mask is not None:
            rays = rays.copy()
            rays["pad"] = np.broadcast_to(np.asarray(ray_mask).astype(np.uint32) & 0xff, (n,))
            mode = int(mode) | CRT_TRACE_INSTANCE_MASK
        hits, ids = np.empty(n, HIT_DT), np.empty(n, np.int32)
        st = np.zeros(n, STATS_DT) if stats else None
        check(lib().crt_instances_trace(self._h, _ptr(rays), n, _ptr(hits), _ptr(ids), int(mode), _ptr(st) if stats else None))
        return (hits, ids, st) if stats else (hits, ids)

    def trace_device(self, d_rays, n, d_hits, d_instance_ids=None, mode=CRT_TRACE_CLOSEST, d_stats=None, sync=True):
        """device pointers (e.g. torch tensors' data_ptr()) of n crt_ray / crt_hit / int32 / crt_ray_stats records; mode may carry
        CRT_TRACE_INSTANCE_MASK (the rays' pad words then hold their masks)"""
        check(lib().crt_instances_trace_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_hits),
                                               C.c_void_p(d_instance_ids) if d_instance_ids else None, int(mode),
                                               C.c_void_p(d_stats) if d_stats else None, 1 if sync else 0))

    def _read(self, which, dtype, width):
        n = C.c_size_t()
        check(lib().crt_instances_debug_read(self._h, which, None, 0, C.byref(n)))
        out = np.empty((n.value, width), dtype)
        if n.value:
            check(lib().crt_instances_debug_read(self._h, which, _ptr(out), out.nbytes, C.byref(n)))
        return out

    def world_to_object(self):
        """(n, 12) float32: the device-computed inverse of every instance, instance order"""
        return self._read(0, np.float32, 12)

    def world_boxes(self):
        return self._read(1, np.float32, 6)

    def tlas_nodes(self):
        return self._read(2, np.uint8, 80)

    def instance_records(self):
        """(n, 16) float32: the instance records in TLAS leaf order (row 3: BLAS root node, instance index, identity flag as uint32 bits)"""
        return self._read(3, np.float32, 16)

    def blas_nodes(self):
        """(n, 80) uint8: every BLAS node8 of the packed array (after the TLAS region; child / triangle bases rebased)"""
        return self._read(4, np.uint8, 80)

    def blas_records(self):
        """(n, 12) float32: every BLAS record, (v0 | id) (e1 | slot) (e2 | w); the w words are int32 bits"""
        return self._read(5, np.float32, 12)

    def tlas_child_masks(self):
        """(n_tlas8, 8) uint8: per TLAS node8, per meta slot, the OR of the masks of every instance under that child (recomputed first if
        stale)"""
        return self._read(6, np.uint8, 8)

    def object_to_world(self):
        """(n, 12) float32: the live object_to_world of every instance, as the last successful set / refit gave them"""
        return self._read(7, np.float32, 12)

    def frame_scene(self, shading, materials, lights, width, height, max_depth=3, textures=None, mesh_lights=None):
        """A Scene that renders frames of this handle's LIVE instances (crt_scene_create_instanced): every Scene method works
        on it, and a set / refit / update_meshes between frames changes what the next frame sees (call reset()).  Its options
        "instance_masks" (0 / 1), "mask_primary", "mask_bounce", "mask_shadow" (0..255) apply the instances' masks to its rays (§17).  shading: per mesh, in mesh
        order, (triangles (n, 12) int32 in source order [, normals (k, 3) [, texcoords (k, 2)]]) or an object with those attributes;
        materials (m, 16) float32, lights (l, 18) float32 in WORLD space, textures (layers, H, W, 3) uint8 or None.  Close the returned scene
        before this handle: destroy, add_meshes and replace_meshes are refused while it lives.
        mesh_lights: None, or per mesh an (l, 18) float32 array (or None) of OBJECT-space lights that every instance of the mesh carries
        and that follow it through set / refit / update_meshes (crt_scene_create_instanced_lit); on such a mesh a
        material's emission.w is the light's index within the mesh.  set_mesh_lights(scene, mesh, lights) and read_lights(scene) act on it."""
        keep = []

        def arr(a, dtype, shape):
            a = np.ascontiguousarray(a if a is not None else np.zeros((0,) + shape[1:]), dtype=dtype).reshape(shape)
            keep.append(a)
            return a

        descs = (crt_mesh_shading * max(len(shading), 1))()
        for k, m in enumerate(shading):
            if hasattr(m, "triangles"):
                m = (m.triangles, getattr(m, "normals", None), getattr(m, "texcoords", None))
            m = tuple(m) + (None,) * (3 - len(m))
            t, n, uv = arr(m[0], np.int32, (-1, 12)), arr(m[1], np.float32, (-1, 3)), arr(m[2], np.float32, (-1, 2))
            descs[k].triangles, descs[k].n_triangles = _ptr(t), t.shape[0]
            descs[k].normals, descs[k].n_normals = (_ptr(n) if n.shape[0] else None), n.shape[0]
            descs[k].texcoords, descs[k].n_texcoords = (_ptr(uv) if uv.shape[0] else None), uv.shape[0]
        d = crt_instanced_scene_desc()
        d.abi_version, d.instances, d.meshes, d.n_meshes = CRT_ABI_VERSION, self._h, descs, len(shading)
        mt, lt = arr(materials, np.float32, (-1, 16)), arr(lights, np.float32, (-1, 18))
        d.materials, d.n_materials = _ptr(mt), mt.shape[0]
        d.lights, d.n_lights = (_ptr(lt) if lt.shape[0] else None), lt.shape[0]
        if textures is not None:
            tex = np.ascontiguousarray(textures, np.uint8)
            assert tex.ndim == 4 and tex.shape[3] == 3, "textures must be (layers, H, W, 3) uint8"
            keep.append(tex)
            d.albedo_textures, d.n_textures, d.tex_height, d.tex_width = _ptr(tex), tex.shape[0], tex.shape[1], tex.shape[2]
        d.width, d.height, d.max_depth = int(width), int(height), int(max_depth)
        sc = Scene.__new__(Scene)
        sc._h = C.c_void_p()
        sc.width, sc.height, sc.max_depth, sc.frame_count, sc.rnd, sc.create_ms = int(width), int(height), int(max_depth), 0, Rnd(), 0.0
        if mesh_lights is None:
            check(lib().crt_scene_create_instanced(C.byref(d), C.byref(sc._h)))
        else:
            ml = (crt_mesh_lights * max(len(mesh_lights), 1))()
            assert len(mesh_lights) == len(shading), "mesh_lights: one entry per mesh"
            for k, l in enumerate(mesh_lights):
                la = arr(l, np.float32, (-1, 18))
                ml[k].lights, ml[k].n_lights = (_ptr(la) if la.shape[0] else None), la.shape[0]
            check(lib().crt_scene_create_instanced_lit(C.byref(d), ml, C.byref(sc._h)))
        sc._instances = self                       # the handle must outlive the scene
        del keep
        return sc

    def set_mesh_lights(self, scene, mesh, lights):
        """new OBJECT-space lights (the create's count) for one mesh of a frame_scene made with mesh_lights; call scene.reset()"""
        set_mesh_lights(scene, mesh, lights)

    def read_lights(self, scene):
        """(n, 18) float32: the world light table the next frame of a frame_scene samples (rebuilt first if stale)"""
        return read_lights(scene)

    def info(self):
        st = crt_instances_info()
        check(lib().crt_instances_get_info(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self):
        if self._h:
            check(lib().crt_instances_destroy(self._h))       # refused while a frame_scene lives: the handle then stays open
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["InstancedScene", "INSTANCE_DT", "instances_array", "instance_inverse", "instance_world_box", "instance_lights", "lights_finish",
           "set_mesh_lights", "read_lights"]
