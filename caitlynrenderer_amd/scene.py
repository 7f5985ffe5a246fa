"""Device-side scene: the drop-in for Scene::gpu_data / update / Render (Caitlyn/Scene.h:1000-1246).

`SceneData` is the bundle of host arrays the reference uploads; `Scene` owns the device copy and
dispatches the HIP path through the C ABI.  There is no CPU fallback: constructing a `Scene`
without a GPU raises CrtError(CRT_ERR_NO_DEVICE).
"""
import ctypes as C

import numpy as np

from ._lib import (CRT_ABI_VERSION, CRT_ENV_HIDE_FROM_CAMERA, crt_environment, CRT_AOV_ALBEDO, CRT_AOV_ALL, CRT_AOV_EMISSION, CRT_AOV_HIT, CRT_AOV_IDS, CRT_AOV_NORMAL, CRT_BUILD_LBVH_ON_DEVICE, CRT_DENOISE_DEMODULATE, CRT_TEMPORAL_CLAMP, CRT_TEMPORAL_DEMODULATE, CRT_TEMPORAL_SOURCE_DENOISED, CRT_TEMPORAL_SOURCE_SUM, CRT_TRACE_ANY, CRT_TRACE_CLOSEST, check, crt_bvh_info, crt_denoise_params, crt_frame_stats, crt_temporal_params, crt_ao_params, crt_fog_params,
                   crt_scene_desc, crt_tree_cost, lib,
                   CRT_DISPLAY_AUTO_EXPOSURE, CRT_DISPLAY_CURVE_ACES, CRT_DISPLAY_CURVE_CLAMP, CRT_DISPLAY_CURVE_REFERENCE, CRT_DISPLAY_CURVE_REINHARD,
                   CRT_DISPLAY_SOURCE_DENOISED, CRT_DISPLAY_SOURCE_SUM, CRT_DISPLAY_SOURCE_TEMPORAL, crt_display_params, crt_display_state,
                   CRT_DEFORM_KEEP_NORMALS, CRT_DEFORM_REBUILD,
                   CRT_BLOOM_CONSERVE, CRT_BLOOM_SOURCE_DENOISED, CRT_BLOOM_SOURCE_SUM, CRT_BLOOM_SOURCE_TEMPORAL, crt_bloom_params)
from .host import CWBVH, SBVH, Camera, Mesh, Rnd, _cost_dict, _ptr

RAY_DT = np.dtype([("o", "<f4", 3), ("tmax", "<f4"), ("d", "<f4", 3), ("pad", "<u4")])
HIT_DT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<i4")])
STATS_DT = np.dtype([("nodes", "<u2"), ("tris", "<u2")])
# crt_render_aov's channels (include/crt.h): 16 bytes per pixel each
AOV_HIT, AOV_IDS, AOV_NORMAL, AOV_ALBEDO, AOV_EMISSION, AOV_ALL = CRT_AOV_HIT, CRT_AOV_IDS, CRT_AOV_NORMAL, CRT_AOV_ALBEDO, CRT_AOV_EMISSION, CRT_AOV_ALL
AOV_IDS_DT = np.dtype([("instance", "<i4"), ("mesh", "<i4"), ("material", "<i4"), ("flags", "<i4")])
# what Scene.read_aov returns per channel: (dtype, trailing shape behind (height, width))
AOV_DTYPES = {AOV_HIT: (HIT_DT, ()), AOV_IDS: (AOV_IDS_DT, ()), AOV_NORMAL: (np.dtype("<f4"), (4,)), AOV_ALBEDO: (np.dtype("<f4"), (4,)),
              AOV_EMISSION: (np.dtype("<f4"), (4,))}
# an AO point of ao_points / ao_points_device (include/crt.h at crt_render_ao): 32 bytes, laid out like RAY_DT
AO_POINT_DT = np.dtype([("p", "<f4", 3), ("seed_x", "<f4"), ("n", "<f4", 3), ("seed_y", "<f4")])


def _ao_params(samples, radius, offset):
    p = crt_ao_params()
    p.samples, p.flags = int(samples), 0
    p.radius = float(np.float32(1e9 if radius is None else radius))
    p.offset = float(np.float32(offset))
    return p


# a fog segment of fog_segments / fog_segments_device (include/crt.h at crt_render_fog): 32 bytes, laid out like RAY_DT
FOG_SEGMENT_DT = np.dtype([("o", "<f4", 3), ("seed_x", "<f4"), ("e", "<f4", 3), ("seed_y", "<f4")])


def _fog_params(samples, density, albedo, anisotropy, max_distance, ambient):
    p = crt_fog_params()
    p.samples, p.flags = int(samples), 0
    p.density, p.anisotropy, p.max_distance = (float(np.float32(v)) for v in (density, anisotropy, max_distance))
    for k in range(3):
        p.albedo[k], p.ambient[k] = float(np.float32(albedo[k])), float(np.float32(ambient[k]))
    return p


class SceneData:
    """Host arrays in upload order (Scene.h:1015-1062) + the CWBVH the shader was meant to get."""

    def __init__(self, mesh, sbvh, cwbvh, camera):
        self.vertices, self.normals, self.texcoords = mesh.vertices, mesh.normals, mesh.texcoords
        self.materials, self.lights = mesh.materials, mesh.lights
        self.triangles = sbvh.triangles                 # leaf order with duplicates (sbvh.h:130-139)
        self.tri_orig_ids = sbvh.triangle_indices
        self.bvh = sbvh.flat_nodes
        self.bvh8 = cwbvh.nodes if cwbvh is not None else None
        self.bvh8_tri_slots = cwbvh.tri_slots if cwbvh is not None else None
        self.camera = camera
        self.albedo_textures = getattr(mesh, "albedo_textures", None)   # (layers, H, W, 3) uint8 or None (Scene.h:1065-1078)
        self.n_source_triangles = int(mesh.triangles.shape[0])
        self.build_flags = 0

    @staticmethod
    def build(mesh, camera, sbvh_flags=0, with_cwbvh=True, builder="sbvh", convert="host"):
        """Scene::build_bvh (Scene.h:929-959) followed by the intended CWBVH::convert.
        builder="lbvh" swaps the host SBVH for the GPU linear BVH (crt_lbvh_build); convert="device" runs
        the CWBVH conversion on the GPU (crt_cwbvh_convert_device, same bytes as the host converter)."""
        sbvh = SBVH(mesh.triangles, mesh.vertices, sbvh_flags, builder=builder)
        cw = CWBVH().convert(sbvh, device=(convert == "device")) if with_cwbvh else None
        return SceneData(mesh, sbvh, cw, camera)

    @staticmethod
    def for_device_build(mesh, camera, builder="lbvh"):
        """The seven input arrays only (triangles in source order): Scene() then builds the BVH2 (builder "lbvh", or "ploc" /
        "ploc<radius>"), the CWBVH and the intersection records in HBM (crt_scene_desc.build_flags =
        CRT_BUILD_LBVH_ON_DEVICE [| CRT_BUILD_PLOC | radius << 8]) — nothing but these arrays crosses PCIe."""
        class _NoBvh:
            triangles, triangle_indices, flat_nodes = mesh.triangles, None, None
        data = SceneData(mesh, _NoBvh, None, camera)
        data.build_flags = CRT_BUILD_LBVH_ON_DEVICE
        if builder.startswith("ploc"):
            data.build_flags |= 2 | ((int(builder[4:]) if len(builder) > 4 else 0) << 8)
        elif builder.startswith("sah"):
            data.build_flags |= 4 | ((int(builder[3:]) if len(builder) > 3 else 0) << 8)
        return data

    @staticmethod
    def from_obj(path, camera):
        """Scene(file_name, …) up to gpu_data (Scene.h:447-495): load, translate, build."""
        mesh = Mesh.read_object(path, camera)
        return SceneData.build(mesh, camera)


class Scene:
    def __init__(self, data, width, height, max_depth=3):
        self._h = C.c_void_p()
        self.width, self.height, self.max_depth = int(width), int(height), int(max_depth)
        self.frame_count = 0                       # Scene.h:384
        self.rnd = Rnd()                           # Rnd.h:7
        d = crt_scene_desc()
        d.abi_version = CRT_ABI_VERSION
        keep = []

        def arr(a, dtype):
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            return a

        v = arr(data.vertices, np.float32); d.vertices, d.n_vertices = _ptr(v), v.shape[0]
        n = arr(data.normals, np.float32); d.normals, d.n_normals = _ptr(n), n.shape[0]
        t = arr(data.texcoords, np.float32); d.texcoords, d.n_texcoords = _ptr(t), t.shape[0]
        tr = arr(data.triangles, np.int32); d.triangles, d.n_triangles = _ptr(tr), tr.shape[0]
        if data.tri_orig_ids is not None:
            ids = arr(data.tri_orig_ids, np.int32); d.tri_orig_ids = _ptr(ids)
        m = arr(data.materials, np.float32); d.materials, d.n_materials = _ptr(m), m.shape[0]
        l = arr(data.lights, np.float32); d.lights, d.n_lights = _ptr(l), l.shape[0]
        if data.bvh is not None:
            b = arr(data.bvh, np.float32); d.bvh, d.n_bvh = _ptr(b), b.shape[0]
        if data.bvh8 is not None:
            b8 = arr(data.bvh8, np.uint8); d.bvh8, d.n_bvh8 = _ptr(b8), b8.shape[0]
            sl = arr(data.bvh8_tri_slots, np.int32); d.bvh8_tri_slots, d.n_bvh8_tris = _ptr(sl), sl.shape[0]
        tex = getattr(data, "albedo_textures", None)
        if tex is not None:
            tex = arr(tex, np.uint8)
            assert tex.ndim == 4 and tex.shape[3] == 3, "albedo_textures must be (layers, H, W, 3) uint8"
            d.albedo_textures = _ptr(tex)
            d.n_textures, d.tex_height, d.tex_width = tex.shape[0], tex.shape[1], tex.shape[2]
        d.width, d.height, d.max_depth = self.width, self.height, self.max_depth
        d.build_flags = int(getattr(data, "build_flags", 0))
        import time
        t0 = time.perf_counter()
        check(lib().crt_scene_create(C.byref(d), C.byref(self._h)))
        self.create_ms = (time.perf_counter() - t0) * 1e3        # wall time of crt_scene_create itself (the arrays were marshalled before)
        if data.camera is not None:
            self.update(data.camera)

    # -- reference-shaped API ------------------------------------------------------------
    def update(self, camera):
        """Scene::update (Scene.h:1233-1246)."""
        check(lib().crt_set_camera(self._h, C.byref(camera.c)))

    def set_environment(self, texels, rotation=None, scale=(1.0, 1.0, 1.0), hide_from_camera=False):
        """crt_set_environment (include/crt.h): `texels` is a (size, size, 3) float32 octahedral map, row 0 first
        (caitlynrenderer_amd.environment builds them), `rotation` a 3 x 3 matrix whose rows take world directions to the map's (default: the
        identity), `scale` an RGB factor.  Rays that leave the scene then return the map's radiance; hide_from_camera keeps the backdrop
        black.  The sum is not cleared: reset() as after update(camera)."""
        t = np.ascontiguousarray(texels, np.float32)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
            raise ValueError("texels must be (size, size, 3)")
        env = crt_environment()
        env.texels, env.size = _ptr(t), t.shape[0]
        env.flags = CRT_ENV_HIDE_FROM_CAMERA if hide_from_camera else 0
        r = np.eye(3, dtype=np.float32) if rotation is None else np.ascontiguousarray(rotation, np.float32).reshape(3, 3)
        env.rotation[:] = [float(x) for x in r.reshape(-1)]
        env.scale[:] = [float(np.float32(x)) for x in scale]
        check(lib().crt_set_environment(self._h, C.byref(env)))

    def clear_environment(self):
        """crt_set_environment(NULL): frames are again what they were without one"""
        check(lib().crt_set_environment(self._h, None))

    def set_camera_rays(self, o, d):
        """crt_set_camera_rays (include/crt.h): frames follow the caller's own rays until clear_camera_rays().  `d` is
        (height, width, 3) float32, rows as read_sum()'s; `o` the same shape, or (3,) for one origin (caitlynrenderer_amd.cameras builds
        both).  Directions are taken as given: supply unit vectors.  An entry whose o or d has a component that is not finite, or whose d is
        zero, has no path: its pixel gets +0.  The rays are copied; the sum is not cleared: reset() as after update(camera)."""
        rays = self.camera_rays_array(o, d)
        check(lib().crt_set_camera_rays(self._h, _ptr(rays), rays.shape[0]))

    def camera_rays_array(self, o, d):
        """the width * height RAY_DT entries set_camera_rays(o, d) hands over, entry of pixel (px, py) at py * width + px (tmax and pad, which
        the library does not read, are 0): what a caller copies to the device for set_camera_rays_device"""
        d = np.asarray(d, np.float32)
        if d.shape != (self.height, self.width, 3):
            raise ValueError("d must be (height, width, 3)")
        o = np.asarray(o, np.float32)
        if o.shape not in ((3,), d.shape):
            raise ValueError("o must be (3,) or (height, width, 3)")
        rays = np.zeros(self.height * self.width, RAY_DT)
        rays["o"] = np.broadcast_to(o, d.shape).reshape(-1, 3)
        rays["d"] = d.reshape(-1, 3)
        return rays

    def set_camera_rays_device(self, ptr, n=None):
        """crt_set_camera_rays_device: width * height entries of 32 bytes (RAY_DT) at the device pointer `ptr` (an int), copied"""
        check(lib().crt_set_camera_rays_device(self._h, C.c_void_p(ptr), self.width * self.height if n is None else int(n)))

    def clear_camera_rays(self):
        """crt_clear_camera_rays: the next frame is the camera's again"""
        check(lib().crt_clear_camera_rays(self._h))

    def Render(self):
        """Scene::Render (Scene.h:1158-1231) minus the present pass: draw one sample, ++frame_count."""
        r1, r2 = self.rnd.randf2(), self.rnd.randf2()          # Scene.h:1208
        self.render_frame(r1, r2)
        self.frame_count += 1
        return r1, r2

    def reset(self):
        """camera.isMoving branch (Scene.h:1160-1172)."""
        check(lib().crt_reset(self._h))
        self.frame_count = 0

    # -- explicit API ----------------------------------------------------------------------
    def render_frame(self, rx, ry, sync=True):
        fn = lib().crt_render_frame if sync else lib().crt_render_frame_async
        check(fn(self._h, float(np.float32(rx)), float(np.float32(ry))))

    def render_frames(self, rvs, sync=True):
        """crt_render_frames: rvs = sequence of (rx, ry); the same sums as render_frame per pair, fewer launches where
        the path allows (shadow rays in place: up to 8 samples per launch; on a shard or a small frame the samples of a
        launch run side by side on the waves of a workgroup, option "wave_samples")."""
        rx = np.ascontiguousarray([r[0] for r in rvs], dtype=np.float32)
        ry = np.ascontiguousarray([r[1] for r in rvs], dtype=np.float32)
        fn = lib().crt_render_frames if sync else lib().crt_render_frames_async
        check(fn(self._h, int(rx.size), _ptr(rx), _ptr(ry)))

    def sync(self):
        check(lib().crt_sync(self._h))

    def set_option(self, name, value):
        check(lib().crt_set_option(self._h, name.encode(), int(value)))

    def read_sum(self):
        out = np.empty((self.height, self.width, 3), np.float32)
        check(lib().crt_read_sum(self._h, _ptr(out), out.size))
        return out

    def resolve(self, inv_count=None):
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().crt_resolve(self._h, float(np.float32(inv_count)), _ptr(out), out.size))
        return out

    def resolve_device(self, inv_count=None, sync=True):
        """crt_resolve_device: the tone-mapped RGBA8 frame left in device memory (what the reference's output pass leaves in the default
        framebuffer); returns the device pointer"""
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        p = C.c_void_p()
        check(lib().crt_resolve_device(self._h, float(np.float32(inv_count)), C.byref(p), 1 if sync else 0))
        return p.value

    def render_aov(self, rx=0.0, ry=0.0, channels=AOV_ALL, sync=True):
        """crt_render_aov: the first-hit feature buffers of the current view, through the primary rays of render_frame(rx, ry): `channels` is
        a set of AOV_* bits.  Touches nothing a frame reads or reports."""
        check(lib().crt_render_aov(self._h, float(np.float32(rx)), float(np.float32(ry)), int(channels), 1 if sync else 0))

    def read_aov(self, channel):
        """crt_read_aov: one channel as an (height, width) array, rows as read_sum has them: AOV_HIT as HIT_DT, AOV_IDS as AOV_IDS_DT
        (instance, mesh, material, flags), the others float32 (height, width, 4)."""
        if channel not in AOV_DTYPES:
            raise ValueError("read_aov: channel is ONE of the AOV_* bits")
        dt, tail = AOV_DTYPES[channel]
        out = np.empty((self.height, self.width) + tail, dt)
        check(lib().crt_read_aov(self._h, int(channel), _ptr(out), out.nbytes))
        return out

    def aov_device(self, channel):
        """crt_aov_device: device pointer (int) of one channel's array, width * height * 16 bytes, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_aov_device(self._h, int(channel), C.byref(ptr)))
        return ptr.value

    def render_ao(self, rx=0.0, ry=0.0, samples=16, radius=None, offset=2e-4, sync=True):
        """crt_render_ao: ambient occlusion at the first hits of the current view, `samples` cosine-distributed rays per pixel of length
        `radius` (None = unbounded), built on the device where they are walked.  Touches nothing a frame or render_aov reads or reports
        (DESIGN.md §32)."""
        p = _ao_params(samples, radius, offset)
        check(lib().crt_render_ao(self._h, float(np.float32(rx)), float(np.float32(ry)), C.byref(p), 1 if sync else 0))

    def read_ao(self):
        """crt_read_ao: (height, width, 4) float32, rows as read_sum has them: the sum of the unoccluded directions (normalise it for a
        bent normal) and the unoccluded share; a miss pixel holds (0, 0, 0, -1)"""
        out = np.empty((self.height, self.width, 4), np.float32)
        check(lib().crt_read_ao(self._h, _ptr(out), out.size))
        return out

    def ao_device(self):
        """crt_ao_device: device pointer (int) of render_ao's image, width * height * 16 bytes, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_ao_device(self._h, C.byref(ptr)))
        return ptr.value

    def ao_points(self, points, rx=0.0, ry=0.0, samples=16, radius=None, offset=2e-4):
        """crt_ao_points: ambient occlusion at the caller's points (an AO_POINT_DT array); returns (n, 4) float32, the bytes render_ao
        gives for the same points"""
        pts = np.ascontiguousarray(points, AO_POINT_DT).reshape(-1)
        out = np.empty((pts.shape[0], 4), np.float32)
        p = _ao_params(samples, radius, offset)
        check(lib().crt_ao_points(self._h, _ptr(pts) if pts.shape[0] else None, pts.shape[0], float(np.float32(rx)), float(np.float32(ry)), C.byref(p),
                                  _ptr(out) if pts.shape[0] else None))
        return out

    def ao_points_device(self, d_points, n, d_out, rx=0.0, ry=0.0, samples=16, radius=None, offset=2e-4, sync=True):
        """crt_ao_points_device: the same with device pointers (ints): n AO points of 32 bytes in, n float4 out"""
        p = _ao_params(samples, radius, offset)
        check(lib().crt_ao_points_device(self._h, C.c_void_p(d_points), int(n), float(np.float32(rx)), float(np.float32(ry)), C.byref(p),
                                         C.c_void_p(d_out), 1 if sync else 0))

    def render_fog(self, rx=0.0, ry=0.0, samples=16, density=0.05, albedo=(1.0, 1.0, 1.0), anisotropy=0.0, max_distance=100.0, ambient=(0.0, 0.0, 0.0),
                   sync=True):
        """crt_render_fog: homogeneous fog with shadowed single scattering along the primary rays of the current view, each cut into
        `samples` strata that aim one shadow ray each at the scene's area lights, built on the device where they are walked.  A miss pixel
        marches to `max_distance`.  Touches nothing a frame, render_aov or render_ao reads or reports."""
        p = _fog_params(samples, density, albedo, anisotropy, max_distance, ambient)
        check(lib().crt_render_fog(self._h, float(np.float32(rx)), float(np.float32(ry)), C.byref(p), 1 if sync else 0))

    def read_fog(self):
        """crt_read_fog: (height, width, 4) float32, rows as read_sum has them: the in-scattered radiance S and the transmittance TD of what
        lies at the segment's end (a fogged pixel is c * TD + S)"""
        out = np.empty((self.height, self.width, 4), np.float32)
        check(lib().crt_read_fog(self._h, _ptr(out), out.size))
        return out

    def fog_device(self):
        """crt_fog_device: device pointer (int) of render_fog's image, width * height * 16 bytes, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_fog_device(self._h, C.byref(ptr)))
        return ptr.value

    def fog_segments(self, segments, rx=0.0, ry=0.0, samples=16, density=0.05, albedo=(1.0, 1.0, 1.0), anisotropy=0.0, ambient=(0.0, 0.0, 0.0)):
        """crt_fog_segments: the fog along the caller's segments (a FOG_SEGMENT_DT array); returns (n, 4) float32, the bytes render_fog
        gives for the same segments; a segment without length or with a non-finite end holds (0, 0, 0, -1)"""
        seg = np.ascontiguousarray(segments, FOG_SEGMENT_DT).reshape(-1)
        out = np.empty((seg.shape[0], 4), np.float32)
        p = _fog_params(samples, density, albedo, anisotropy, 100.0, ambient)
        check(lib().crt_fog_segments(self._h, _ptr(seg) if seg.shape[0] else None, seg.shape[0], float(np.float32(rx)), float(np.float32(ry)), C.byref(p),
                                     _ptr(out) if seg.shape[0] else None))
        return out

    def fog_segments_device(self, d_segments, n, d_out, rx=0.0, ry=0.0, samples=16, density=0.05, albedo=(1.0, 1.0, 1.0), anisotropy=0.0,
                            ambient=(0.0, 0.0, 0.0), sync=True):
        """crt_fog_segments_device: the same with device pointers (ints): n fog segments of 32 bytes in, n float4 out"""
        p = _fog_params(samples, density, albedo, anisotropy, 100.0, ambient)
        check(lib().crt_fog_segments_device(self._h, C.c_void_p(d_segments), int(n), float(np.float32(rx)), float(np.float32(ry)), C.byref(p),
                                            C.c_void_p(d_out), 1 if sync else 0))

    def fog_composite(self, inv_count=None, source="sum", sync=True):
        """crt_fog_composite: render_fog's image put on one float image ("sum": the running sum times inv_count, "denoised", "temporal"):
        c * TD + S per pixel, the fogged image that read_fogged, fogged_device and display_fogged hand on.  inv_count None =
        1 / max(frame_count, 1).  An unknown source name raises KeyError."""
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        sources = {"sum": CRT_DISPLAY_SOURCE_SUM, "denoised": CRT_DISPLAY_SOURCE_DENOISED, "temporal": CRT_DISPLAY_SOURCE_TEMPORAL}
        check(lib().crt_fog_composite(self._h, float(np.float32(inv_count)), sources[source], 1 if sync else 0))

    def read_fogged(self):
        """crt_read_fogged: the fogged MEAN radiance, (height, width, 3) float32, rows as read_sum has them"""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(lib().crt_read_fogged(self._h, _ptr(out), out.size))
        return out

    def fogged_device(self):
        """crt_fogged_device: device pointer (int) of the fogged image, width * height * 3 floats, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_fogged_device(self._h, C.byref(ptr)))
        return ptr.value

    def display_fogged(self, **display_options):
        """crt_display_fogged: display() on fog_composite()'s image, which takes no inv_count; the options are display()'s"""
        return self.display(source="fogged", **display_options)

    def denoise(self, inv_count=None, passes=5, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7, sync=True):
        """crt_denoise: an edge-avoiding a-trous filter over the running sum, guided by the HIT, IDS, NORMAL and ALBEDO channels of the most
        recent render_aov (the caller keeps them in step with the view and the geometry).  inv_count None = 1 / max(frame_count, 1), as in
        resolve.  Touches nothing a frame reads or reports, no AOV channel and not resolve_device's buffer."""
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        p = crt_denoise_params()
        p.passes, p.flags = int(passes), (CRT_DENOISE_DEMODULATE if demodulate else 0)
        p.sigma_color, p.sigma_depth, p.normal_power_log2 = float(np.float32(sigma_color)), float(np.float32(sigma_depth)), int(normal_power_log2)
        check(lib().crt_denoise(self._h, float(np.float32(inv_count)), C.byref(p), 1 if sync else 0))

    def read_denoised(self):
        """crt_read_denoised: the denoised MEAN radiance, (height, width, 3) float32, rows as read_sum has them"""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(lib().crt_read_denoised(self._h, _ptr(out), out.size))
        return out

    def denoised_device(self):
        """crt_denoised_device: device pointer (int) of the denoised image, width * height * 3 floats, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_denoised_device(self._h, C.byref(ptr)))
        return ptr.value

    def resolve_denoised(self):
        """crt_resolve_denoised: resolve's tone map and pinned gamma on the denoised image, (height, width, 4) uint8"""
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().crt_resolve_denoised(self._h, _ptr(out), out.size))
        return out

    def resolve_denoised_device(self, sync=True):
        """crt_resolve_denoised_device: the same RGBA8 left in device memory, in a buffer of its own; returns the device pointer"""
        p = C.c_void_p()
        check(lib().crt_resolve_denoised_device(self._h, C.byref(p), 1 if sync else 0))
        return p.value

    def temporal(self, inv_count=None, source="sum", demodulate=True, clamp=False, max_history=32, sigma_depth=0.1, normal_min=0.9, sync=True):
        """crt_temporal: blend the source ("sum": the running sum times inv_count, "denoised": crt_denoise's image) into the previous call's
        result, reprojected through the camera's and the instances' motion and guided by the HIT, IDS, NORMAL and ALBEDO channels of the most
        recent render_aov.  inv_count None = 1 / max(frame_count, 1).  reset() does not touch the history."""
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        sources = {"sum": CRT_TEMPORAL_SOURCE_SUM, "denoised": CRT_TEMPORAL_SOURCE_DENOISED}
        if source not in sources:
            raise ValueError('source is "sum" or "denoised"')
        p = crt_temporal_params()
        p.flags = (CRT_TEMPORAL_DEMODULATE if demodulate else 0) | (CRT_TEMPORAL_CLAMP if clamp else 0)
        p.source, p.max_history = sources[source], int(max_history)
        p.sigma_depth, p.normal_min = float(np.float32(sigma_depth)), float(np.float32(normal_min))
        check(lib().crt_temporal(self._h, float(np.float32(inv_count)), C.byref(p), 1 if sync else 0))

    def temporal_reset(self):
        """crt_temporal_reset: the next temporal() starts every pixel at N = 1; the buffers stay"""
        check(lib().crt_temporal_reset(self._h))

    def read_temporal(self):
        """crt_read_temporal: the accumulated MEAN radiance, (height, width, 3) float32, rows as read_sum has them"""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(lib().crt_read_temporal(self._h, _ptr(out), out.size))
        return out

    def read_temporal_history(self):
        """crt_read_temporal_history: N per pixel, (height, width) float32"""
        out = np.empty((self.height, self.width), np.float32)
        check(lib().crt_read_temporal_history(self._h, _ptr(out), out.size))
        return out

    def temporal_device(self):
        """crt_temporal_device: device pointer (int) of the accumulated image, width * height * 3 floats, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_temporal_device(self._h, C.byref(ptr)))
        return ptr.value

    def resolve_temporal(self):
        """crt_resolve_temporal: resolve's tone map and pinned gamma on the accumulated image, (height, width, 4) uint8"""
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().crt_resolve_temporal(self._h, _ptr(out), out.size))
        return out

    def resolve_temporal_device(self, sync=True):
        """crt_resolve_temporal_device: the same RGBA8 left in device memory, in a buffer of its own; returns the device pointer"""
        p = C.c_void_p()
        check(lib().crt_resolve_temporal_device(self._h, C.byref(p), 1 if sync else 0))
        return p.value

    def display(self, inv_count=None, source="sum", curve="reference", exposure=1.0, auto=False, white=4.0, key=0.18, adapt=1.0, exposure_min=1e-6,
                exposure_max=1e6, low_permille=0, high_permille=1000, sync=True):
        """crt_display: the display transform of one float image ("sum": the running sum times inv_count, "denoised", "temporal", "bloom":
        crt_display_bloom on bloom()'s image, or "fogged": crt_display_fogged on fog_composite()'s; those two take no inv_count) into RGBA8
        in device memory: exposure (given, or with auto=True metered on the device from the image's luminance histogram and adapted by
        `adapt` per call), a tone curve ("reference", "reinhard", "aces", "clamp") and the pinned gamma.  inv_count None =
        1 / max(frame_count, 1).  The defaults are the header's NULL: resolve()'s bytes.  Returns the (height, width, 4) uint8 image, or None
        with sync=False (read_display() after sync()).  An unknown source or curve name raises KeyError."""
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        sources = {"sum": CRT_DISPLAY_SOURCE_SUM, "denoised": CRT_DISPLAY_SOURCE_DENOISED, "temporal": CRT_DISPLAY_SOURCE_TEMPORAL, "bloom": 0,
                   "fogged": 0}
        curves = {"reference": CRT_DISPLAY_CURVE_REFERENCE, "reinhard": CRT_DISPLAY_CURVE_REINHARD, "aces": CRT_DISPLAY_CURVE_ACES,
                  "clamp": CRT_DISPLAY_CURVE_CLAMP}
        p = crt_display_params()
        p.source, p.curve = sources[source], curves[curve]
        p.flags = CRT_DISPLAY_AUTO_EXPOSURE if bool(auto) else 0
        p.exposure, p.white, p.key, p.adapt = (float(np.float32(v)) for v in (exposure, white, key, adapt))
        p.exposure_min, p.exposure_max = float(np.float32(exposure_min)), float(np.float32(exposure_max))
        p.low_permille, p.high_permille = int(low_permille), int(high_permille)
        if source == "bloom":
            check(lib().crt_display_bloom(self._h, C.byref(p), 1 if sync else 0))
        elif source == "fogged":
            check(lib().crt_display_fogged(self._h, C.byref(p), 1 if sync else 0))
        else:
            check(lib().crt_display(self._h, float(np.float32(inv_count)), C.byref(p), 1 if sync else 0))
        return self.read_display() if sync else None

    def read_display(self):
        """crt_read_display: the RGBA8 of the last display(), (height, width, 4) uint8, rows as resolve has them"""
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().crt_read_display(self._h, _ptr(out), out.size))
        return out

    def display_device(self):
        """crt_display_device: device pointer (int) of display()'s RGBA8, width * height * 4 bytes, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_display_device(self._h, C.byref(ptr)))
        return ptr.value

    def display_state(self):
        """crt_display_get_state: what the last display() left on the device: dict of exposure (E of that call), metered (L_avg, 0 when
        nothing was metered), counted (N), q (Q) and calls (metered calls since the last display_reset)"""
        st = crt_display_state()
        check(lib().crt_display_get_state(self._h, C.byref(st)))
        return {"exposure": np.float32(st.exposure), "metered": np.float32(st.metered), "counted": int(st.counted), "q": int(st.q), "calls": int(st.calls)}

    def display_histogram(self):
        """crt_read_display_histogram: the 256 luminance bins of the last display(auto=True), before trimming, uint32"""
        out = np.empty(256, np.uint32)
        check(lib().crt_read_display_histogram(self._h, _ptr(out)))
        return out

    def display_reset(self):
        """crt_display_reset: the next display(auto=True) takes its metered exposure at once; the buffers stay"""
        check(lib().crt_display_reset(self._h))

    def bloom(self, inv_count=None, source="sum", levels=6, conserve=True, threshold=0.0, clamp=0.0, scatter=0.7, strength=0.05, sync=True):
        """crt_bloom: the light of the bright parts of one float image ("sum": the running sum times inv_count, "denoised", "temporal") spread
        over an image pyramid of up to `levels` levels and put back on the image: read_bloom(), resolve_bloom() or display(source="bloom")
        afterwards.  threshold: the luminance below which nothing blooms; clamp (0 = none): the luminance a pixel feeds the pyramid with at
        most; scatter: the share taken from the coarser level at each step up; conserve: out = c + (G - c) * strength in place of
        c + G * strength.  inv_count None = 1 / max(frame_count, 1).  The defaults are the header's NULL."""
        if inv_count is None:
            inv_count = 1.0 / max(self.frame_count, 1)
        sources = {"sum": CRT_BLOOM_SOURCE_SUM, "denoised": CRT_BLOOM_SOURCE_DENOISED, "temporal": CRT_BLOOM_SOURCE_TEMPORAL}
        p = crt_bloom_params()
        p.source, p.levels, p.flags = sources[source], int(levels), (CRT_BLOOM_CONSERVE if conserve else 0)
        p.threshold, p.clamp, p.scatter, p.strength = (float(np.float32(v)) for v in (threshold, clamp, scatter, strength))
        check(lib().crt_bloom(self._h, float(np.float32(inv_count)), C.byref(p), 1 if sync else 0))

    def read_bloom(self):
        """crt_read_bloom: the bloomed MEAN radiance, (height, width, 3) float32, rows as read_sum has them"""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(lib().crt_read_bloom(self._h, _ptr(out), out.size))
        return out

    def bloom_device(self):
        """crt_bloom_device: device pointer (int) of the bloomed image, width * height * 3 floats, valid until the scene is closed"""
        ptr = C.c_void_p()
        check(lib().crt_bloom_device(self._h, C.byref(ptr)))
        return ptr.value

    def resolve_bloom(self):
        """crt_resolve_bloom: resolve's tone map and pinned gamma on the bloomed image, (height, width, 4) uint8"""
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().crt_resolve_bloom(self._h, _ptr(out), out.size))
        return out

    def resolve_bloom_device(self, sync=True):
        """crt_resolve_bloom_device: the same RGBA8 left in device memory, in a buffer of its own; returns the device pointer"""
        p = C.c_void_p()
        check(lib().crt_resolve_bloom_device(self._h, C.byref(p), 1 if sync else 0))
        return p.value

    def launch_times(self):
        """crt_get_launch_times: ms of every event-carrying launch since the spans were restarted (options timing / timing_accumulate)"""
        n = C.c_size_t()
        check(lib().crt_get_launch_times(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        if n.value:
            check(lib().crt_get_launch_times(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def trace(self, rays, mode=CRT_TRACE_CLOSEST, stats=False):
        rays = np.ascontiguousarray(rays, dtype=RAY_DT)
        hits = np.empty(rays.shape[0], HIT_DT)
        st = np.zeros(rays.shape[0], STATS_DT) if stats else None
        check(lib().crt_trace(self._h, _ptr(rays), rays.shape[0], _ptr(hits), int(mode), _ptr(st) if stats else None))
        return (hits, st) if stats else hits

    def trace_device(self, d_rays, n, d_hits, mode=CRT_TRACE_CLOSEST, d_stats=None, sync=True):
        check(lib().crt_trace_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_hits), int(mode),
                                     C.c_void_p(d_stats) if d_stats else None, 1 if sync else 0))

    def debug_read_queue(self, which, segment):
        """Rays entering `segment` (which=0) or its shadow rays (which=2) as left by the last frame."""
        n = C.c_size_t()
        check(lib().crt_debug_read_queue(self._h, int(which), int(segment), None, 0, C.byref(n)))
        out = np.empty(n.value, RAY_DT)
        check(lib().crt_debug_read_queue(self._h, int(which), int(segment), _ptr(out), n.value, C.byref(n)))
        return out

    def debug_launch_form(self):
        """0: the last launch ran its samples one after the other in each wave (or had one); 1: side by side on the waves
        of a workgroup (option "wave_samples")."""
        form = C.c_int32()
        check(lib().crt_debug_launch_form(self._h, C.byref(form)))
        return form.value

    def debug_launch_info(self):
        """crt_debug_launch_info of the last first-segment launch: {"form": 0 | 1 | 2 (2 = four samples of a 4x4 pixel quadrant in the
        lanes of a wave), "wide": the 6-waves-per-SIMD build ran, "one_pass": a build without the sample loop ran (k_segment<..., ONE>),
        "samples": samples per pixel of the launch, "shards": tile shards side by side (streams / devices)}"""
        info = (C.c_int32 * 4)()
        check(lib().crt_debug_launch_info(self._h, info))
        return {"form": info[0], "wide": bool(info[1] & 1), "one_pass": bool(info[1] & 2), "samples": info[2], "shards": info[3]}

    def launch_info(self):
        """crt_debug_launch_info's four words as they are: [form, build word, samples per launch chain, shards].  Bit 4 of the build word
        (16): segment 0 was fed by the lens ray generator (camera aperture > 0), and bits 0-3 are then clear.  Bit 5 (32): the frame ran with an
        environment (set_environment).  Bit 6 (64): segment 0 was fed by the caller's camera rays (set_camera_rays); bits 0-4 are then clear."""
        info = (C.c_int32 * 4)()
        check(lib().crt_debug_launch_info(self._h, info))
        return [int(x) for x in info]

    def debug_last_build(self):
        """True when the last first-segment launch ran a one-pass build compiled as a path's last segment (bit 2 of
        crt_debug_launch_info's build word; option "last_build")"""
        info = (C.c_int32 * 4)()
        check(lib().crt_debug_launch_info(self._h, info))
        return bool(info[1] & 4)

    def debug_lean_build(self):
        """True when that build ran in its LEAN form (bit 3 of crt_debug_launch_info's build word; option "lean_build")"""
        info = (C.c_int32 * 4)()
        check(lib().crt_debug_launch_info(self._h, info))
        return bool(info[1] & 8)

    def debug_step_hist(self, stop=False):
        """crt_debug_step_hist: (closest[65], any[65]) node steps of the counting frames since the previous call by number of enabled lanes"""
        if stop:
            check(lib().crt_debug_step_hist(self._h, None))
            return None
        h = np.zeros(130, np.uint64)
        check(lib().crt_debug_step_hist(self._h, _ptr(h)))
        return h[:65].copy(), h[65:].copy()

    def update_vertices(self, vertices, normals=None, lights=None):
        """crt_update_vertices: new positions (same count), optionally new normals / lights; refits the trees and records on the
        device and clears the sum (frame_count restarts)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        l = None if lights is None else np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 18)
        check(lib().crt_update_vertices(self._h, _ptr(v), v.shape[0], _ptr(n), 0 if n is None else n.shape[0],
                                        _ptr(l), 0 if l is None else l.shape[0]))
        self.frame_count = 0

    def update_vertices_device(self, ptr, n, sync=True):
        """crt_update_vertices_device: positions already on the scene's device (ptr = device address of n x 3 float32)."""
        check(lib().crt_update_vertices_device(self._h, C.c_void_p(int(ptr)), int(n), int(bool(sync))))
        self.frame_count = 0

    def last_update_ms(self):
        """(device ms of the last update's refit kernels, host wall ms of the call)"""
        d, w = C.c_float(), C.c_float()
        check(lib().crt_last_update_ms(self._h, C.byref(d), C.byref(w)))
        return d.value, w.value

    def rebuild_vertices(self, vertices, normals=None, lights=None):
        """crt_rebuild_vertices: new positions (same count), optionally new normals / lights, and the tree built again from them in place
        with the scene's own builder (scenes from for_device_build only); clears the sum (frame_count restarts).  A torch
        tensor that lives on the GPU goes through crt_rebuild_vertices_device without leaving it (positions only)."""
        if getattr(vertices, "is_cuda", False):
            if normals is not None or lights is not None:
                raise ValueError("rebuild_vertices: the device form takes positions only")
            t = vertices.detach().reshape(-1, 3).contiguous()
            if str(t.dtype) != "torch.float32":
                raise TypeError("rebuild_vertices: a device tensor must be float32")
            import torch
            torch.cuda.current_stream(t.device).synchronize()          # the library reads it on the scene's own stream
            self.rebuild_vertices_device(t.data_ptr(), t.shape[0])
            return
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        l = None if lights is None else np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 18)
        check(lib().crt_rebuild_vertices(self._h, _ptr(v), v.shape[0], _ptr(n), 0 if n is None else n.shape[0],
                                         _ptr(l), 0 if l is None else l.shape[0]))
        self.frame_count = 0

    def rebuild_vertices_device(self, ptr, n, sync=True):
        """crt_rebuild_vertices_device: positions already on the scene's device (ptr = device address of n x 3 float32)."""
        check(lib().crt_rebuild_vertices_device(self._h, C.c_void_p(int(ptr)), int(n), int(bool(sync))))
        self.frame_count = 0

    def deform(self, deformer, bones, morph_weights=None, rebuild=False, keep_normals=False, sync=True):
        """crt_deform_scene: the whole per-frame step of a deforming scene on its stream: the deformer's pose (only `bones` and
        `morph_weights` cross PCIe), the coordinate check, the new normals into the scene's buffer unless keep_normals, and the refit,
        or with rebuild=True a rebuild under rebuild_vertices' rules; clears the sum (frame_count restarts).  DESIGN.md §31."""
        b, w = deformer._d.pose(bones, morph_weights)
        flags = (CRT_DEFORM_REBUILD if rebuild else 0) | (CRT_DEFORM_KEEP_NORMALS if keep_normals else 0)
        check(lib().crt_deform_scene(self._h, deformer._h, _ptr(b), _ptr(w), flags, 1 if sync else 0))
        self.frame_count = 0

    def tree_cost(self):
        """crt_get_tree_cost: the SAH cost of the live CWBVH, computed on the device (a dict of crt_tree_cost's fields).  Compare a
        refitted scene's with a rebuilt one's over the same positions."""
        c = crt_tree_cost()
        check(lib().crt_get_tree_cost(self._h, C.byref(c)))
        return _cost_dict(c)

    def debug_read_accel(self, which):
        """crt_debug_read_accel: 0 node8 (n,80) u8, 1 CWBVH-order records (n,12) f32, 2 BVH2 (n,8) f32, 3 slot-order records (n,12) f32."""
        n = C.c_size_t()
        check(lib().crt_debug_read_accel(self._h, int(which), None, 0, C.byref(n)))
        out = np.zeros((n.value, 80), np.uint8) if which == 0 else np.zeros((n.value, 8 if which == 2 else 12), np.float32)
        check(lib().crt_debug_read_accel(self._h, int(which), _ptr(out), out.nbytes, C.byref(n)))
        return out

    def set_shard(self, rank, world, tile=16):
        check(lib().crt_set_shard(self._h, int(rank), int(world), int(tile)))

    def sum_device(self):
        """crt_sum_device: device pointer (int) of the whole frame's running sum on the first device (gathered when there are several)."""
        ptr = C.c_void_p()
        check(lib().crt_sum_device(self._h, C.byref(ptr)))
        return ptr.value

    def set_devices(self, devices, tile=16):
        """crt_set_devices: this one handle renders on all of `devices` (HIP device ids, the scene's own first); read_sum / resolve
        gather the other devices' tiles to the first.  The same id more than once = virtual devices on one GPU (tests)."""
        ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        check(lib().crt_set_devices(self._h, ids, len(devices), int(tile)))

    def devices(self):
        """{"devices": [...], "transport": "rccl" | "copy", "last_gather_ms": ms of the last gather}"""
        n, tr, ms = C.c_uint32(), C.c_int32(), C.c_float()
        ids = (C.c_int32 * 64)()
        check(lib().crt_get_devices(self._h, C.byref(n), ids, 64, C.byref(tr), C.byref(ms)))
        return {"devices": [int(ids[k]) for k in range(n.value)], "transport": "rccl" if tr.value == 0 else "copy", "last_gather_ms": float(ms.value)}

    def packed_info(self):
        nt, tile, nf = C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(lib().crt_packed_info(self._h, C.byref(nt), C.byref(tile), C.byref(nf)))
        return nt.value, tile.value, nf.value

    def read_packed(self):
        _, _, nf = self.packed_info()
        out = np.empty(nf, np.float32)
        check(lib().crt_read_packed(self._h, _ptr(out), nf))
        return out

    def copy_packed_device(self, d_dst, n_floats, sync=True):
        check(lib().crt_copy_packed_device(self._h, C.c_void_p(d_dst), int(n_floats), 1 if sync else 0))

    def frame_stats(self):
        st = crt_frame_stats()
        check(lib().crt_get_frame_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def bvh_info(self):
        st = crt_bvh_info()
        check(lib().crt_get_bvh_info(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self):
        if self._h:
            lib().crt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["Scene", "SceneData", "Camera", "Mesh", "SBVH", "CWBVH", "RAY_DT", "HIT_DT", "STATS_DT", "AO_POINT_DT", "FOG_SEGMENT_DT", "AOV_IDS_DT", "AOV_DTYPES",
           "AOV_HIT", "AOV_IDS", "AOV_NORMAL", "AOV_ALBEDO", "AOV_EMISSION", "AOV_ALL",
           "CRT_TRACE_CLOSEST", "CRT_TRACE_ANY", "CRT_BUILD_LBVH_ON_DEVICE"]
