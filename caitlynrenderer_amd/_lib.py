"""ctypes binding of libcrt.so (the C ABI declared in include/crt.h).

The library is the product: if it is missing this module raises — there is no Python or CPU
fallback for the traversal path.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C caitlynrenderer_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRT_LIB points the binding at another build of the same library (A/B measurements of kernel variants in one gpurun call)
LIB_PATH = os.environ.get("CRT_LIB") or os.path.join(_HERE, "libcrt.so")

CRT_ABI_VERSION = int(os.environ.get("CRT_LIB_ABI", "6"))      # CRT_LIB_ABI: with CRT_LIB, an older build of the library measured beside this one (tools/ab_run.sh)
CRT_OK, CRT_ERR_INVALID, CRT_ERR_NO_DEVICE, CRT_ERR_HIP, CRT_ERR_IO, CRT_ERR_LIMIT, CRT_ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6
CRT_TRACE_CLOSEST, CRT_TRACE_ANY, CRT_TRACE_BVH2, CRT_TRACE_TIE_LOWEST_ID = 0, 1, 2, 4
CRT_TRACE_INSTANCE_MASK = 8              # crt_instances_trace only: the low 8 bits of crt_ray.pad are the ray's instance mask
CRT_AOV_HIT, CRT_AOV_IDS, CRT_AOV_NORMAL, CRT_AOV_ALBEDO, CRT_AOV_EMISSION, CRT_AOV_ALL = 1, 2, 4, 8, 16, 31    # crt_render_aov's channels
CRT_DENOISE_DEMODULATE = 1               # crt_denoise_params.flags
DENOISE_DEMODULATE = CRT_DENOISE_DEMODULATE
CRT_TEMPORAL_DEMODULATE, CRT_TEMPORAL_CLAMP = 1, 2                       # crt_temporal_params.flags
CRT_TEMPORAL_SOURCE_SUM, CRT_TEMPORAL_SOURCE_DENOISED = 0, 1             # crt_temporal_params.source
CRT_DISPLAY_SOURCE_SUM, CRT_DISPLAY_SOURCE_DENOISED, CRT_DISPLAY_SOURCE_TEMPORAL = 0, 1, 2          # crt_display_params.source
CRT_DISPLAY_CURVE_REFERENCE, CRT_DISPLAY_CURVE_REINHARD, CRT_DISPLAY_CURVE_ACES, CRT_DISPLAY_CURVE_CLAMP = 0, 1, 2, 3    # crt_display_params.curve
CRT_DISPLAY_AUTO_EXPOSURE = 1            # crt_display_params.flags
CRT_BLOOM_SOURCE_SUM, CRT_BLOOM_SOURCE_DENOISED, CRT_BLOOM_SOURCE_TEMPORAL = 0, 1, 2                # crt_bloom_params.source
CRT_BLOOM_CONSERVE = 1                   # crt_bloom_params.flags
CRT_ENV_HIDE_FROM_CAMERA = 1             # crt_environment.flags
CRT_DEFORM_REBUILD, CRT_DEFORM_KEEP_NORMALS = 1, 2                       # crt_deform_scene's flags
CRT_BUILD_LBVH_ON_DEVICE = 1
CRT_BUILD_PLOC, CRT_BUILD_SAH = 2, 4
CRT_INSTANCES_UPDATABLE = 1 << 16


class CrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"crt error {code}: {msg}")
        self.code = code


class crt_camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("forward", C.c_float * 3), ("fov", C.c_float), ("focal_dist", C.c_float), ("aperture", C.c_float)]


class crt_environment(C.Structure):
    # struct crt_environment: crt_set_environment's octahedral map, rotation and scale
    _fields_ = [("texels", C.c_void_p), ("size", C.c_uint32), ("flags", C.c_uint32), ("rotation", C.c_float * 9), ("scale", C.c_float * 3),
                ("reserved", C.c_uint32 * 2)]


class crt_scene_desc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("vertices", C.c_void_p), ("n_vertices", C.c_size_t),
        ("normals", C.c_void_p), ("n_normals", C.c_size_t),
        ("texcoords", C.c_void_p), ("n_texcoords", C.c_size_t),
        ("triangles", C.c_void_p), ("n_triangles", C.c_size_t),
        ("tri_orig_ids", C.c_void_p),
        ("materials", C.c_void_p), ("n_materials", C.c_size_t),
        ("lights", C.c_void_p), ("n_lights", C.c_size_t),
        ("bvh", C.c_void_p), ("n_bvh", C.c_size_t),
        ("bvh8", C.c_void_p), ("n_bvh8", C.c_size_t),
        ("bvh8_tri_slots", C.c_void_p), ("n_bvh8_tris", C.c_size_t),
        ("albedo_textures", C.c_void_p), ("tex_width", C.c_uint32), ("tex_height", C.c_uint32), ("n_textures", C.c_uint32),
        ("width", C.c_uint32), ("height", C.c_uint32), ("max_depth", C.c_uint32), ("build_flags", C.c_uint32),
    ]


class crt_frame_stats(C.Structure):
    _fields_ = [("closest_rays", C.c_uint64), ("any_rays", C.c_uint64), ("ms_total", C.c_float),
                ("ms_trace_closest", C.c_float), ("ms_trace_any", C.c_float), ("ms_shade", C.c_float),
                ("ms_raygen", C.c_float), ("n_trace_launches", C.c_uint32),
                ("nodes_closest", C.c_uint64), ("tris_closest", C.c_uint64), ("nodes_any", C.c_uint64), ("tris_any", C.c_uint64),
                ("stack_overflows", C.c_uint32),
                ("wave_steps_closest_nodes", C.c_uint64), ("wave_steps_closest_tris", C.c_uint64),
                ("wave_steps_any_nodes", C.c_uint64), ("wave_steps_any_tris", C.c_uint64), ("closest_hits", C.c_uint64),
                ("nodes_closest_uniform", C.c_uint64), ("nodes_any_uniform", C.c_uint64)]


class crt_bvh_info(C.Structure):
    _fields_ = [("n_nodes8", C.c_uint64), ("n_tris8", C.c_uint64), ("n_bvh2_nodes", C.c_uint64), ("max_depth8", C.c_uint64),
                ("built_on_device", C.c_uint32), ("bvh2_depth", C.c_uint32), ("build_wall_ms", C.c_float), ("build_upload_ms", C.c_float),
                ("build_lbvh_device_ms", C.c_float), ("build_convert_device_ms", C.c_float)]


class crt_tree_cost(C.Structure):
    _fields_ = [("root_area", C.c_double), ("inner_area", C.c_double), ("leaf_area", C.c_double),
                ("n_nodes8", C.c_uint64), ("n_inner_slots", C.c_uint64), ("n_leaf_slots", C.c_uint64), ("n_leaf_items", C.c_uint64),
                ("cost", C.c_double)]


class crt_blas_desc(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("n_vertices", C.c_size_t), ("triangles", C.c_void_p), ("n_triangles", C.c_size_t)]


class _crt_instance_tail_words(C.Structure):
    _fields_ = [("material_offset", C.c_uint32), ("reserved1", C.c_uint32)]


class _crt_instance_tail(C.Union):
    # the two words at bytes 56..63: `reserved` as they were, `material_offset` the first of them
    _anonymous_ = ("words",)
    _fields_ = [("reserved", C.c_uint32 * 2), ("words", _crt_instance_tail_words)]


class crt_instance(C.Structure):
    _anonymous_ = ("tail",)
    _fields_ = [("object_to_world", C.c_float * 12), ("mesh", C.c_uint32), ("mask", C.c_uint32), ("tail", _crt_instance_tail)]


class crt_mesh_shading(C.Structure):
    _fields_ = [("triangles", C.c_void_p), ("n_triangles", C.c_size_t), ("normals", C.c_void_p), ("n_normals", C.c_size_t),
                ("texcoords", C.c_void_p), ("n_texcoords", C.c_size_t)]


class crt_instanced_scene_desc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("instances", C.c_void_p), ("meshes", C.POINTER(crt_mesh_shading)), ("n_meshes", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_size_t), ("lights", C.c_void_p), ("n_lights", C.c_size_t),
                ("albedo_textures", C.c_void_p), ("tex_width", C.c_uint32), ("tex_height", C.c_uint32), ("n_textures", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("max_depth", C.c_uint32)]


class crt_mesh_lights(C.Structure):
    # struct crt_mesh_lights: one mesh's OBJECT-space lights (crt_scene_create_instanced_lit)
    _fields_ = [("lights", C.c_void_p), ("n_lights", C.c_size_t)]


class crt_instances_info(C.Structure):
    _fields_ = [("n_meshes", C.c_uint32), ("n_instances", C.c_uint32), ("capacity", C.c_uint32), ("stack_entries", C.c_uint32),
                ("tlas_nodes8", C.c_uint32), ("tlas_depth8", C.c_uint32), ("max_blas_depth8", C.c_uint32), ("stack_overflows", C.c_uint32),
                ("blas_nodes8", C.c_uint64), ("blas_tris", C.c_uint64), ("blas_bytes", C.c_uint64), ("tlas_bytes", C.c_uint64),
                ("instance_bytes", C.c_uint64), ("tlas_build_bytes", C.c_uint64), ("set_device_ms", C.c_float), ("set_wall_ms", C.c_float), ("create_wall_ms", C.c_float),
                ("reserved_f", C.c_float)]


class crt_ao_params(C.Structure):
    # struct crt_ao_params (32 bytes): samples, radius and offset of the ambient-occlusion entries
    _fields_ = [("samples", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_float), ("offset", C.c_float), ("reserved", C.c_uint32 * 4)]


class crt_fog_params(C.Structure):
    # struct crt_fog_params (64 bytes): samples, density, albedo, anisotropy, range and ambient term of the fog entries
    _fields_ = [("samples", C.c_uint32), ("flags", C.c_uint32), ("density", C.c_float), ("albedo", C.c_float * 3), ("anisotropy", C.c_float),
                ("max_distance", C.c_float), ("ambient", C.c_float * 3), ("reserved", C.c_uint32 * 5)]


class crt_denoise_params(C.Structure):
    # struct crt_denoise_params (32 bytes): crt_denoise's filter settings
    _fields_ = [("passes", C.c_uint32), ("flags", C.c_uint32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float),
                ("normal_power_log2", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class crt_temporal_params(C.Structure):
    # struct crt_temporal_params (32 bytes): crt_temporal's settings
    _fields_ = [("flags", C.c_uint32), ("source", C.c_uint32), ("max_history", C.c_uint32), ("sigma_depth", C.c_float),
                ("normal_min", C.c_float), ("reserved", C.c_uint32 * 3)]


class crt_display_params(C.Structure):
    # struct crt_display_params (48 bytes): crt_display's source, curve and exposure settings
    _fields_ = [("source", C.c_uint32), ("curve", C.c_uint32), ("flags", C.c_uint32), ("exposure", C.c_float), ("white", C.c_float),
                ("key", C.c_float), ("adapt", C.c_float), ("exposure_min", C.c_float), ("exposure_max", C.c_float),
                ("low_permille", C.c_uint32), ("high_permille", C.c_uint32), ("reserved", C.c_uint32)]


class crt_display_state(C.Structure):
    # struct crt_display_state (32 bytes): what the last crt_display call left on the device
    _fields_ = [("exposure", C.c_float), ("metered", C.c_float), ("counted", C.c_uint32), ("q", C.c_uint32), ("calls", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class crt_bloom_params(C.Structure):
    # struct crt_bloom_params (32 bytes): crt_bloom's source, pyramid depth and blend settings
    _fields_ = [("source", C.c_uint32), ("levels", C.c_uint32), ("flags", C.c_uint32), ("threshold", C.c_float), ("clamp", C.c_float),
                ("scatter", C.c_float), ("strength", C.c_float), ("reserved", C.c_uint32)]


class crt_deformer_desc(C.Structure):
    # struct crt_deformer_desc: crt_deformer_create's rest pose, influences and morph targets
    _fields_ = [("abi_version", C.c_uint32), ("rest_vertices", C.c_void_p), ("n_vertices", C.c_size_t),
                ("vertex_bones", C.c_void_p), ("vertex_weights", C.c_void_p),
                ("rest_normals", C.c_void_p), ("n_normals", C.c_size_t), ("normal_bones", C.c_void_p), ("normal_weights", C.c_void_p),
                ("n_bones", C.c_uint32), ("n_targets", C.c_uint32),
                ("target_first", C.c_void_p), ("target_vertex", C.c_void_p), ("target_delta", C.c_void_p), ("device", C.c_int32)]


# every symbol include/crt.h declares: name -> (restype, argtypes)
_P, _SZ, _I, _U32, _F = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_float
SYMBOLS = {
    "crt_scene_create": (_I, [C.POINTER(crt_scene_desc), C.POINTER(_P)]),
    "crt_scene_destroy": (_I, [_P]),
    "crt_set_camera": (_I, [_P, C.POINTER(crt_camera)]),
    "crt_set_environment": (_I, [_P, C.POINTER(crt_environment)]),
    "crt_set_camera_rays": (_I, [_P, _P, _SZ]),
    "crt_set_camera_rays_device": (_I, [_P, _P, _SZ]),
    "crt_clear_camera_rays": (_I, [_P]),
    "crt_render_frame": (_I, [_P, _F, _F]),
    "crt_render_frame_async": (_I, [_P, _F, _F]),
    "crt_render_frames": (_I, [_P, C.c_uint32, _P, _P]),
    "crt_render_frames_async": (_I, [_P, C.c_uint32, _P, _P]),
    "crt_sync": (_I, [_P]),
    "crt_set_option": (_I, [_P, C.c_char_p, _I]),
    "crt_reset": (_I, [_P]),
    "crt_read_sum": (_I, [_P, _P, _SZ]),
    "crt_resolve": (_I, [_P, _F, _P, _SZ]),
    "crt_sum_device": (_I, [_P, C.POINTER(_P)]),
    "crt_trace": (_I, [_P, _P, _SZ, _P, _I, _P]),
    "crt_trace_device": (_I, [_P, _P, _SZ, _P, _I, _P, _I]),
    "crt_resolve_device": (_I, [_P, C.c_float, C.POINTER(C.c_void_p), _I]),
    "crt_render_aov": (_I, [_P, _F, _F, _U32, _I]),
    "crt_read_aov": (_I, [_P, _U32, _P, _SZ]),
    "crt_aov_device": (_I, [_P, _U32, C.POINTER(_P)]),
    "crt_render_ao": (_I, [_P, _F, _F, C.POINTER(crt_ao_params), _I]),
    "crt_read_ao": (_I, [_P, _P, _SZ]),
    "crt_ao_device": (_I, [_P, C.POINTER(_P)]),
    "crt_ao_points": (_I, [_P, _P, _SZ, _F, _F, C.POINTER(crt_ao_params), _P]),
    "crt_ao_points_device": (_I, [_P, _P, _SZ, _F, _F, C.POINTER(crt_ao_params), _P, _I]),
    "crt_denoise": (_I, [_P, _F, C.POINTER(crt_denoise_params), _I]),
    "crt_read_denoised": (_I, [_P, _P, _SZ]),
    "crt_denoised_device": (_I, [_P, C.POINTER(_P)]),
    "crt_resolve_denoised": (_I, [_P, _P, _SZ]),
    "crt_resolve_denoised_device": (_I, [_P, C.POINTER(_P), _I]),
    "crt_temporal": (_I, [_P, _F, C.POINTER(crt_temporal_params), _I]),
    "crt_temporal_reset": (_I, [_P]),
    "crt_read_temporal": (_I, [_P, _P, _SZ]),
    "crt_read_temporal_history": (_I, [_P, _P, _SZ]),
    "crt_temporal_device": (_I, [_P, C.POINTER(_P)]),
    "crt_resolve_temporal": (_I, [_P, _P, _SZ]),
    "crt_resolve_temporal_device": (_I, [_P, C.POINTER(_P), _I]),
    "crt_display": (_I, [_P, _F, C.POINTER(crt_display_params), _I]),
    "crt_read_display": (_I, [_P, _P, _SZ]),
    "crt_display_device": (_I, [_P, C.POINTER(_P)]),
    "crt_display_get_state": (_I, [_P, C.POINTER(crt_display_state)]),
    "crt_read_display_histogram": (_I, [_P, _P]),
    "crt_display_reset": (_I, [_P]),
    "crt_bloom": (_I, [_P, _F, C.POINTER(crt_bloom_params), _I]),
    "crt_read_bloom": (_I, [_P, _P, _SZ]),
    "crt_bloom_device": (_I, [_P, C.POINTER(_P)]),
    "crt_resolve_bloom": (_I, [_P, _P, _SZ]),
    "crt_resolve_bloom_device": (_I, [_P, C.POINTER(_P), _I]),
    "crt_display_bloom": (_I, [_P, C.POINTER(crt_display_params), _I]),
    "crt_render_fog": (_I, [_P, _F, _F, C.POINTER(crt_fog_params), _I]),
    "crt_read_fog": (_I, [_P, _P, _SZ]),
    "crt_fog_device": (_I, [_P, C.POINTER(_P)]),
    "crt_fog_segments": (_I, [_P, _P, _SZ, _F, _F, C.POINTER(crt_fog_params), _P]),
    "crt_fog_segments_device": (_I, [_P, _P, _SZ, _F, _F, C.POINTER(crt_fog_params), _P, _I]),
    "crt_fog_composite": (_I, [_P, _F, _U32, _I]),
    "crt_read_fogged": (_I, [_P, _P, _SZ]),
    "crt_fogged_device": (_I, [_P, C.POINTER(_P)]),
    "crt_display_fogged": (_I, [_P, C.POINTER(crt_display_params), _I]),
    "crt_get_launch_times": (_I, [_P, _P, _SZ, C.POINTER(_SZ)]),
    "crt_update_vertices": (_I, [_P, _P, _SZ, _P, _SZ, _P, _SZ]),
    "crt_update_vertices_device": (_I, [_P, _P, _SZ, _I]),
    "crt_last_update_ms": (_I, [_P, C.POINTER(_F), C.POINTER(_F)]),
    "crt_rebuild_vertices": (_I, [_P, _P, _SZ, _P, _SZ, _P, _SZ]),
    "crt_rebuild_vertices_device": (_I, [_P, _P, _SZ, _I]),
    "crt_deformer_create": (_I, [C.POINTER(crt_deformer_desc), C.POINTER(_P)]),
    "crt_deformer_destroy": (_I, [_P]),
    "crt_deformer_pose": (_I, [_P, _P, _P, _I]),
    "crt_deformer_sync": (_I, [_P]),
    "crt_deformer_vertices_device": (_I, [_P, C.POINTER(_P)]),
    "crt_deformer_normals_device": (_I, [_P, C.POINTER(_P)]),
    "crt_deformer_read": (_I, [_P, _P, _SZ, _P, _SZ]),
    "crt_deformer_last_ms": (_I, [_P, C.POINTER(_F)]),
    "crt_deform_scene": (_I, [_P, _P, _P, _P, _U32, _I]),
    "crt_deform_host": (_I, [C.POINTER(crt_deformer_desc), _P, _P, _P, _P]),
    "crt_get_tree_cost": (_I, [_P, C.POINTER(crt_tree_cost)]),
    "crt_instances_tree_cost": (_I, [_P, C.c_int32, C.POINTER(crt_tree_cost)]),
    "crt_debug_read_accel": (_I, [_P, _I, _P, _SZ, C.POINTER(_SZ)]),
    "crt_instances_create": (_I, [C.POINTER(crt_blas_desc), _U32, _P, _U32, _U32, _U32, C.POINTER(_P)]),
    "crt_instances_set": (_I, [_P, _P, _U32]),
    "crt_instances_set_device": (_I, [_P, _P, _U32, _I]),
    "crt_instances_refit": (_I, [_P, _P, _U32]),
    "crt_instances_refit_device": (_I, [_P, _P, _U32, _I]),
    "crt_instances_trace": (_I, [_P, _P, _SZ, _P, _P, _I, _P]),
    "crt_instances_trace_device": (_I, [_P, _P, _SZ, _P, _P, _I, _P, _I]),
    "crt_instances_get_info": (_I, [_P, C.POINTER(crt_instances_info)]),
    "crt_instances_debug_read": (_I, [_P, _I, _P, _SZ, C.POINTER(_SZ)]),
    "crt_instances_update_meshes": (_I, [_P, _P, _U32, _P, _P]),
    "crt_instances_update_meshes_device": (_I, [_P, _P, _U32, _P, _P, _I]),
    "crt_instances_add_meshes": (_I, [_P, _P, _U32, C.POINTER(_U32)]),
    "crt_instances_replace_meshes": (_I, [_P, _P, _U32, _P]),
    "crt_instances_last_update": (_I, [_P, C.POINTER(_F), C.POINTER(_F), C.POINTER(C.c_uint64)]),
    "crt_instances_destroy": (_I, [_P]),
    "crt_scene_create_instanced": (_I, [C.POINTER(crt_instanced_scene_desc), C.POINTER(_P)]),
    "crt_scene_create_instanced_lit": (_I, [C.POINTER(crt_instanced_scene_desc), C.POINTER(crt_mesh_lights), C.POINTER(_P)]),
    "crt_scene_set_mesh_lights": (_I, [_P, _U32, _P, _SZ]),
    "crt_scene_read_lights": (_I, [_P, _P, _SZ, C.POINTER(_SZ)]),
    "crt_instance_lights": (_I, [_P, _P, _SZ, _P]),
    "crt_lights_finish": (_I, [_P, _SZ]),
    "crt_instance_inverse": (_I, [_P, _P]),
    "crt_instance_world_box": (_I, [_P, _P, _P]),
    "crt_debug_read_queue": (_I, [_P, _I, _U32, _P, _SZ, C.POINTER(_SZ)]),
    "crt_debug_time_graph": (_I, [_P, _U32, _P, _U32, C.POINTER(_F), C.POINTER(_F)]),
    "crt_debug_launch_form": (_I, [_P, C.POINTER(C.c_int32)]),
    "crt_debug_launch_info": (_I, [_P, C.POINTER(C.c_int32)]),
    "crt_debug_step_hist": (_I, [_P, _P]),
    "crt_set_shard": (_I, [_P, _U32, _U32, _U32]),
    "crt_set_devices": (_I, [_P, C.POINTER(C.c_int32), _U32, _U32]),
    "crt_shard_tiles": (_I, [_U32] * 7 + [_P, _SZ, C.POINTER(_SZ)]),
    "crt_get_devices": (_I, [_P, C.POINTER(_U32), C.POINTER(C.c_int32), _U32, C.POINTER(C.c_int32), C.POINTER(_F)]),
    "crt_packed_info": (_I, [_P, C.POINTER(_U32), C.POINTER(_U32), C.POINTER(_SZ)]),
    "crt_read_packed": (_I, [_P, _P, _SZ]),
    "crt_copy_packed_device": (_I, [_P, _P, _SZ, _I]),
    "crt_get_frame_stats": (_I, [_P, C.POINTER(crt_frame_stats)]),
    "crt_get_bvh_info": (_I, [_P, C.POINTER(crt_bvh_info)]),
    "crt_device_count": (_I, []),
    "crt_has_experiments": (_I, []),
    "crt_warmup": (_I, []),
    "crt_camera_look_at": (_I, [C.POINTER(_F), C.POINTER(_F), _F, C.POINTER(crt_camera)]),
    "crt_pcg_hash": (_U32, [_U32]),
    "crt_randf2": (_F, [C.POINTER(_U32)]),
    "crt_sbvh_build": (_I, [_P, _SZ, _P, _SZ, _U32, C.POINTER(_P)]),
    "crt_sbvh_num_nodes": (_SZ, [_P]),
    "crt_sbvh_num_slots": (_SZ, [_P]),
    "crt_sbvh_nodes": (_P, [_P]),
    "crt_sbvh_triangle_indices": (_P, [_P]),
    "crt_sbvh_triangles": (_P, [_P]),
    "crt_sbvh_free": (None, [_P]),
    "crt_lbvh_build": (_I, [_P, _SZ, _P, _SZ, _U32, C.POINTER(_P)]),
    "crt_lbvh_last_build_ms": (None, [C.POINTER(_F), C.POINTER(_F)]),
    "crt_cwbvh_convert": (_I, [_P, _SZ, _SZ, C.POINTER(_P)]),
    "crt_cwbvh_convert_device": (_I, [_P, _SZ, _SZ, C.POINTER(_P)]),
    "crt_cwbvh_last_convert_ms": (None, [C.POINTER(_F), C.POINTER(_F)]),
    "crt_cwbvh_num_nodes": (_SZ, [_P]),
    "crt_cwbvh_num_tris": (_SZ, [_P]),
    "crt_cwbvh_nodes": (_P, [_P]),
    "crt_cwbvh_tri_slots": (_P, [_P]),
    "crt_cwbvh_child_bvh2": (_P, [_P]),
    "crt_cwbvh_depth": (_U32, [_P]),
    "crt_cwbvh_free": (None, [_P]),
    "crt_bvh2_refit": (_I, [_P, _SZ, _P, _SZ, _P, _SZ]),
    "crt_cwbvh_refit": (_I, [_P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ]),
    "crt_cwbvh_cost": (_I, [_P, _SZ, _SZ, _SZ, C.POINTER(crt_tree_cost)]),
    "crt_load_obj": (_I, [C.c_char_p, C.POINTER(_F), C.POINTER(_P)]),
    "crt_mesh_counts": (_SZ, [_P] + [C.POINTER(_SZ)] * 6),
    "crt_mesh_vertices": (_P, [_P]),
    "crt_mesh_normals": (_P, [_P]),
    "crt_mesh_texcoords": (_P, [_P]),
    "crt_mesh_triangles": (_P, [_P]),
    "crt_mesh_materials": (_P, [_P]),
    "crt_mesh_lights": (_P, [_P]),
    "crt_mesh_vertex_min": (_P, [_P]),
    "crt_mesh_albedo_textures": (_P, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "crt_mesh_free": (None, [_P]),
    "crt_image_decode": (_I, [_P, _SZ, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _SZ]),
    "crt_image_encode_png": (_I, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _SZ, C.POINTER(C.c_size_t)]),
    "crt_texture_to_array_bytes": (_I, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "crt_last_error": (C.c_char_p, []),
    "crt_abi_version": (_U32, []),
}

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same SONAME as
    /opt/rocm's); if both copies get loaded, the second one initialised sees no devices.  When torch
    is installed, load ITS runtime first (RTLD_GLOBAL) so libcrt.so's NEEDED libamdhip64.so.7 binds to
    it, whichever of torch / this package is imported first.  Without torch, /opt/rocm's is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        libdir = os.path.join(os.path.dirname(spec.origin), "lib")
        for name in ("libamdhip64.so",):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libcrt.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run __graft_entry__.build() or `make -C caitlynrenderer_amd/csrc`); there is no fallback path")
        _share_hip_runtime_with_torch()
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)   # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if l.crt_abi_version() != CRT_ABI_VERSION:
            raise ImportError("libcrt.so ABI version mismatch; rebuild")
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise CrtError(rc, lib().crt_last_error().decode("utf-8", "replace"))
