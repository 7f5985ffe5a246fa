"""Descriptors that crt_scene_create, crt_scene_create_instanced and crt_scene_create_instanced_lit refuse, one fault each, and what a refusal
looks like from outside: (return code, crt_last_error() text, whether *out came back NULL).  tests/test_create_refusals.py holds the library
to a recording of these (tests/golden/create_refusals.json, made by tests/golden/make_create_refusals.py); both import the cases from here.

The flat cases start from the Cornell box (host-built: SceneData.build; device-built: the source-order arrays) at 32 x 24, three segments;
the instanced ones from a handle of two meshes, both the Cornell box."""
import ctypes as C

import numpy as np

W, H, DEPTH = 32, 24, 3
F32, I32 = np.float32, np.int32
SENTINEL = 0x10                  # what *out holds before the call: a refusal has to overwrite it with NULL


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Flat:
    """The arrays and scalars of a crt_scene_desc, copied so that a case may edit them in place."""

    def __init__(self, cr, mesh, data=None):
        from caitlynrenderer_amd._lib import CRT_ABI_VERSION, CRT_BUILD_LBVH_ON_DEVICE
        cp = lambda a, dt, cols: None if a is None else np.array(a, dt).reshape(-1, cols)
        self.abi = CRT_ABI_VERSION
        self.vertices, self.normals, self.texcoords = cp(mesh.vertices, F32, 3), cp(mesh.normals, F32, 3), None
        self.materials, self.lights = cp(mesh.materials, F32, 16), cp(mesh.lights, F32, 18)
        self.n_lights = self.lights.shape[0]
        self.textures = None                     # (layers, H, W, 3) uint8
        self.tex_width = self.tex_height = None  # None: the array's own
        if data is None:                         # built on the device: the triangles in source order and nothing else
            self.triangles, self.ids, self.bvh, self.bvh8, self.slots = cp(mesh.triangles, I32, 12), None, None, None, None
            self.build_flags = CRT_BUILD_LBVH_ON_DEVICE
        else:
            self.triangles, self.ids = cp(data.triangles, I32, 12), cp(data.tri_orig_ids, I32, 1)
            self.bvh, self.bvh8, self.slots = cp(data.bvh, F32, 8), np.array(data.bvh8, np.uint8), cp(data.bvh8_tri_slots, I32, 1)
            self.build_flags = 0
        self.width, self.height, self.max_depth = W, H, DEPTH

    def with_textures(self, textured_material=3):
        """one 4 x 4 layer, four texcoords that every triangle indexes, and `textured_material` reading layer 0"""
        self.textures = np.full((1, 4, 4, 3), 128, np.uint8)
        self.texcoords = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32)
        self.triangles[:, 8:11] = (0, 1, 2)
        self.materials[textured_material, 12] = 0.0
        return self

    def desc(self):
        from caitlynrenderer_amd._lib import crt_scene_desc
        d = crt_scene_desc()
        n = lambda a: 0 if a is None else a.shape[0]
        d.abi_version = self.abi
        d.vertices, d.n_vertices = _ptr(self.vertices), n(self.vertices)
        d.normals, d.n_normals = _ptr(self.normals), n(self.normals)
        d.texcoords, d.n_texcoords = _ptr(self.texcoords), n(self.texcoords)
        d.triangles, d.n_triangles = _ptr(self.triangles), n(self.triangles)
        d.tri_orig_ids = _ptr(self.ids)
        d.materials, d.n_materials = _ptr(self.materials), n(self.materials)
        d.lights, d.n_lights = _ptr(self.lights), self.n_lights
        d.bvh, d.n_bvh = _ptr(self.bvh), n(self.bvh)
        d.bvh8, d.n_bvh8 = _ptr(self.bvh8), 0 if self.bvh8 is None else self.bvh8.size // 80
        d.bvh8_tri_slots, d.n_bvh8_tris = _ptr(self.slots), n(self.slots)
        if self.textures is not None:
            d.albedo_textures, d.n_textures = _ptr(self.textures), self.textures.shape[0]
            d.tex_height = self.textures.shape[1] if self.tex_height is None else self.tex_height
            d.tex_width = self.textures.shape[2] if self.tex_width is None else self.tex_width
        d.width, d.height, d.max_depth, d.build_flags = self.width, self.height, self.max_depth, self.build_flags
        return d


def _textured_triangle(f):
    return int(np.flatnonzero(f.triangles[:, 3] == 3)[0])


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _edit(name, index, value):
    def go(f):
        getattr(f, name)[index] = value
    return go


def _leaf(f):
    return int(np.flatnonzero(f.bvh[:, 7] != 0.0)[0])


# name -> (base: "host" / "device", edit of the Flat).  These return before the library asks for a device: they run anywhere.
FLAT_HOST_CHECKS = {
    "abi_mismatch": ("host", lambda f: _set(f, abi=f.abi + 1)),
    "vertices_missing": ("host", lambda f: _set(f, vertices=None)),
    "materials_missing": ("host", lambda f: _set(f, materials=None)),
    "lights_missing": ("host", lambda f: _set(f, lights=None)),
    "neither_bvh_nor_bvh8": ("host", lambda f: _set(f, bvh=None, bvh8=None, slots=None)),
    "device_build_given_a_bvh": ("host", lambda f: _set(f, build_flags=1)),
    "unknown_build_flags": ("host", lambda f: _set(f, build_flags=1 << 16)),
    "ploc_without_device_build": ("host", lambda f: _set(f, build_flags=2)),
    "width_0": ("host", lambda f: _set(f, width=0)),
    "width_too_large": ("host", lambda f: _set(f, width=65535 * 8 + 1)),
    "max_depth_0": ("host", lambda f: _set(f, max_depth=0)),
    "max_depth_17": ("host", lambda f: _set(f, max_depth=17)),
    "vertex_index": ("host", lambda f: _edit("triangles", (5, 0), f.vertices.shape[0])(f)),
    "material_index": ("host", lambda f: _edit("triangles", (5, 3), f.materials.shape[0])(f)),
    "normal_index": ("host", lambda f: _edit("triangles", (5, 4), f.normals.shape[0])(f)),
    "vertex_not_finite": ("host", _edit("vertices", (3, 1), np.nan)),
    "texture_size": ("host", lambda f: _set(f.with_textures(), tex_width=0)),
    "material_texture_index": ("host", lambda f: _edit("materials", (3, 12), 1.0)(f.with_textures())),
    "textured_without_texcoords": ("host", lambda f: _set(f.with_textures(), texcoords=None)),
    "texcoord_index": ("host", lambda f: _edit("triangles", (_textured_triangle(f), 8), 4)(f.with_textures())),
    "emissive_without_light": ("host", lambda f: _edit("materials", (1, 7), float(f.n_lights))(f)),
}

# These pass the host checks above: the library has asked for a device by the time it refuses them.
FLAT_DEVICE_CHECKS = {
    "bvh8_without_slots": ("host", lambda f: _set(f, slots=None)),
    "slot_out_of_range": ("host", lambda f: _edit("slots", (0, 0), f.triangles.shape[0])(f)),
    "bvh2_leaf_range": ("host", lambda f: _edit("bvh", (_leaf(f), 3), float(f.triangles.shape[0]))(f)),
    "bvh2_child_link": ("host", _edit("bvh", (0, 3), 0.0)),
    "device_built_vertex_index": ("device", lambda f: _edit("triangles", (5, 0), f.vertices.shape[0])(f)),
    "device_built_material_index": ("device", lambda f: _edit("triangles", (5, 3), f.materials.shape[0])(f)),
    "device_built_normal_index": ("device", lambda f: _edit("triangles", (5, 4), f.normals.shape[0])(f)),
    "device_built_texcoord_index": ("device", lambda f: _edit("triangles", (_textured_triangle(f), 8), 4)(f.with_textures())),
}


class Instanced:
    """The arrays of a crt_instanced_scene_desc over a handle of two Cornell boxes, and per-mesh lights for the lit entry."""

    def __init__(self, mesh):
        self.shading = [{"triangles": np.array(mesh.triangles, I32).reshape(-1, 12), "normals": np.array(mesh.normals, F32).reshape(-1, 3),
                         "texcoords": None} for _ in range(2)]
        self.n_triangles = [None, None]          # None: the array's own
        self.n_meshes = 2
        self.materials, self.lights = np.array(mesh.materials, F32).reshape(-1, 16), np.array(mesh.lights, F32).reshape(-1, 18)
        self.textures = None
        # the lit entry: mesh 0 carries three lights, mesh 1 none; the emissive material (1) names light 0
        self.mesh_lights = [np.tile(self.lights[:1], (3, 1)), None]

    def with_textures(self):
        self.textures = np.full((1, 4, 4, 3), 128, np.uint8)
        for m in self.shading:
            m["texcoords"] = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32)
            m["triangles"][:, 8:11] = (0, 1, 2)
        self.materials[3, 12] = 0.0
        return self

    def desc(self, handle):
        """-> (crt_instanced_scene_desc, crt_mesh_lights array, what both point into)"""
        from caitlynrenderer_amd._lib import CRT_ABI_VERSION, crt_instanced_scene_desc, crt_mesh_lights, crt_mesh_shading
        n = lambda a: 0 if a is None else a.shape[0]
        meshes = (crt_mesh_shading * 2)()
        for k, m in enumerate(self.shading):
            meshes[k].triangles = _ptr(m["triangles"])
            meshes[k].n_triangles = n(m["triangles"]) if self.n_triangles[k] is None else self.n_triangles[k]
            meshes[k].normals, meshes[k].n_normals = _ptr(m["normals"]), n(m["normals"])
            meshes[k].texcoords, meshes[k].n_texcoords = _ptr(m["texcoords"]), n(m["texcoords"])
        d = crt_instanced_scene_desc()
        d.abi_version, d.instances, d.meshes, d.n_meshes = CRT_ABI_VERSION, handle, meshes, self.n_meshes
        d.materials, d.n_materials = _ptr(self.materials), n(self.materials)
        d.lights, d.n_lights = _ptr(self.lights), n(self.lights)
        if self.textures is not None:
            d.albedo_textures, d.n_textures, d.tex_height, d.tex_width = _ptr(self.textures), 1, 4, 4
        d.width, d.height, d.max_depth = W, H, DEPTH
        ml = (crt_mesh_lights * 2)()
        for k, l in enumerate(self.mesh_lights):
            ml[k].lights, ml[k].n_lights = _ptr(l), n(l)
        return d, ml, meshes


def _mesh_edit(k, name, index, value):
    def go(i):
        i.shading[k][name][index] = value
    return go


def _lit_mesh_light_missing(i):            # mesh 0 carries one light, its emissive triangles name light 1 (a static light has that index)
    i.mesh_lights[0] = i.mesh_lights[0][:1]
    i.materials[1, 7] = 1.0


# name -> (entry: "plain" / "lit", edit of the Instanced)
INSTANCED_CHECKS = {
    "mesh_count": ("plain", lambda i: _set(i, n_meshes=1)),
    "triangle_count": ("plain", lambda i: _set(i, n_triangles=[None, i.shading[1]["triangles"].shape[0] - 1])),
    "normal_not_finite": ("plain", _mesh_edit(1, "normals", (2, 0), np.inf)),
    "material_index": ("plain", lambda i: _mesh_edit(1, "triangles", (5, 3), i.materials.shape[0])(i)),
    "normal_index": ("plain", lambda i: _mesh_edit(1, "triangles", (5, 4), i.shading[1]["normals"].shape[0])(i)),
    "texcoord_index": ("plain", lambda i: _mesh_edit(1, "triangles", (_textured_triangle(Flat_like(i, 1)), 8), 4)(i.with_textures())),
    "lit_light_not_finite": ("lit", lambda i: _edit("lights", (1, 4), np.nan)(i)),
    "lit_mesh_does_not_carry_the_light": ("lit", _lit_mesh_light_missing),
    "lit_static_light_does_not_exist": ("lit", lambda i: _edit("materials", (1, 7), 2.0)(i)),     # 2 < three mesh lights, but mesh 1 has two static ones
}


class Flat_like:
    """mesh k of an Instanced, for _textured_triangle"""

    def __init__(self, i, k):
        self.triangles = i.shading[k]["triangles"]


def _observe(rc, out):
    from caitlynrenderer_amd._lib import lib
    return {"rc": int(rc), "error": lib().crt_last_error().decode("utf-8", "replace"), "out_null": None if out is None else not out.value}


def _destroy_if_made(out):
    from caitlynrenderer_amd._lib import lib
    if out is not None and out.value and out.value != SENTINEL:      # a case the library did NOT refuse: the comparison will say so
        lib().crt_scene_destroy(out)


def observe_null_arguments(cr, mesh, data):
    """-> {case: observation} of the two calls that are no descriptor edits"""
    from caitlynrenderer_amd._lib import lib
    d = Flat(cr, mesh, data).desc()
    out = C.c_void_p(SENTINEL)
    return {"null_out": _observe(lib().crt_scene_create(C.byref(d), None), None),
            "null_desc": _observe(lib().crt_scene_create(None, C.byref(out)), out)}


def observe_flat(cr, mesh, data, case):
    from caitlynrenderer_amd._lib import lib
    base, edit = {**FLAT_HOST_CHECKS, **FLAT_DEVICE_CHECKS}[case]
    f = Flat(cr, mesh, data if base == "host" else None)
    edit(f)
    d = f.desc()
    out = C.c_void_p(SENTINEL)
    got = _observe(lib().crt_scene_create(C.byref(d), C.byref(out)), out)
    _destroy_if_made(out)
    return got


def make_handle(cr, mesh):
    identity = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    return cr.InstancedScene([mesh, mesh], cr.instances_array([identity, identity], [0, 1]), builder="sah")


def observe_instanced(cr, mesh, handle, case):
    from caitlynrenderer_amd._lib import lib
    entry, edit = INSTANCED_CHECKS[case]
    i = Instanced(mesh)
    edit(i)
    d, ml, keep = i.desc(handle._h)
    out = C.c_void_p(SENTINEL)
    if entry == "lit":
        rc = lib().crt_scene_create_instanced_lit(C.byref(d), ml, C.byref(out))
    else:
        rc = lib().crt_scene_create_instanced(C.byref(d), C.byref(out))
    got = _observe(rc, out)
    _destroy_if_made(out)
    del keep
    return got
