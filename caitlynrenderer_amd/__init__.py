"""MI355X-native ray/BVH-traversal hot path of a Caitlyn-style path tracer.

The compute path lives in libcrt.so (hand-written HIP for gfx950 behind the C ABI of
include/crt.h); this package is the thin host-side mirror of the reference's Scene / Camera /
SBVH / CWBVH interface plus tile sharding helpers.  Importing it without a built libcrt.so fails.
"""
from . import _lib
from ._lib import CRT_TRACE_ANY, CRT_TRACE_BVH2, CRT_TRACE_CLOSEST, CRT_TRACE_INSTANCE_MASK, CRT_TRACE_TIE_LOWEST_ID, CrtError
from .host import CWBVH, SBVH, Camera, Mesh, Rnd, pcg_hash
from .scene import (AO_POINT_DT, FOG_SEGMENT_DT, AOV_ALBEDO, AOV_ALL, AOV_DTYPES, AOV_EMISSION, AOV_HIT, AOV_IDS, AOV_IDS_DT, AOV_NORMAL, HIT_DT, RAY_DT, STATS_DT, Scene,
                    SceneData)
from .cameras import fisheye_rays, orthographic_rays, panorama_rays, pinhole_rays
from .deform import Deformer, deform_host, normal_influences
from .environment import constant_environment, octahedral_directions, octahedral_from_equirect, octahedral_from_function
from .instances import (INSTANCE_DT, InstancedScene, instance_inverse, instance_lights, instance_world_box, instances_array, lights_finish,
                        read_lights, set_mesh_lights)

_lib.lib()   # fail loudly at import time if the HIP extension is missing


def has_experiments():
    """True when libcrt.so was built with the experimental kernel variants (make EXPERIMENTS=1, include/crt.h crt_set_option)."""
    return bool(_lib.lib().crt_has_experiments())


def warmup():
    """crt_warmup: HIP context + the library's code objects on the current device, so that the first scene does not pay for them."""
    _lib.check(_lib.lib().crt_warmup())


__all__ = ["has_experiments", "warmup", "pinhole_rays", "panorama_rays", "orthographic_rays", "fisheye_rays", "constant_environment", "octahedral_directions", "octahedral_from_equirect", "octahedral_from_function", "Scene", "SceneData", "Deformer", "deform_host", "normal_influences", "InstancedScene", "INSTANCE_DT", "instances_array", "instance_inverse",
           "instance_world_box", "instance_lights", "lights_finish", "set_mesh_lights", "read_lights", "Camera", "Mesh", "SBVH", "CWBVH", "Rnd", "pcg_hash", "CrtError",
           "RAY_DT", "HIT_DT", "STATS_DT", "CRT_TRACE_CLOSEST", "CRT_TRACE_ANY", "CRT_TRACE_BVH2", "CRT_TRACE_TIE_LOWEST_ID",
           "CRT_TRACE_INSTANCE_MASK", "AOV_HIT", "AOV_IDS", "AOV_NORMAL", "AOV_ALBEDO", "AOV_EMISSION", "AOV_ALL", "AOV_IDS_DT", "AOV_DTYPES", "AO_POINT_DT", "FOG_SEGMENT_DT"]
