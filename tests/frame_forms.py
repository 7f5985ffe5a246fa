"""The table of frame forms: which chain of launches each option combination produces, observed through the public entry points.

Shared by tests/golden/make_frame_forms.py, which records the table into tests/golden/frame_forms.json, and tests/test_frame_forms.py,
which holds the library to the recording.  A configuration is one axis moved off the defaults (Cornell box or the tessellated box or a
two-instance scene, max_depth 3, four frames per call); what is observed of it is the SHA-256 of the sum's bytes, crt_debug_launch_info's
four words, the number of timed launches and the two ray counts of crt_frame_stats.  An option the library refuses is recorded as the
error code in place of a frame."""
import ctypes as C
import hashlib
import types

import numpy as np

W, H = 48, 40          # 3 x 3 tiles of 16: the last tile row is cut by the frame edge
RVS = [(0.3719, 0.8123), (0.1357, 0.2468), (0.9021, 0.5519), (0.4242, 0.0917), (0.7071, 0.3333), (0.0531, 0.6789), (0.6111, 0.9434)]
SCENES = ("cornell", "big", "instanced")
LENS = (0.03, 1.5)     # (aperture, focal_dist)

# one axis at a time: (label, options, extras)
AXES = [
    ("defaults", (), {}),
    ("depth1", (), {"depth": 1}),
    ("n1", (), {"n": 1}),
    ("n7", (), {"n": 7}),
    ("depth1_n1", (), {"depth": 1, "n": 1}),
    ("depth1_n7", (), {"depth": 1, "n": 7}),
    ("inplace_shadow0", (("inplace_shadow", 0),), {}),
    ("inplace_shadow1", (("inplace_shadow", 1),), {}),
    ("inplace_shadow2", (("inplace_shadow", 2),), {}),
    ("bounce_refill1", (("bounce_refill", 1),), {}),
    ("ray_bins1", (("ray_bins", 1),), {}),
    ("ray_bins4", (("ray_bins", 4),), {}),
    ("sort_shadow1", (("sort_shadow", 1),), {}),
    ("accel1", (("accel", 1),), {}),
    ("count_visits1", (("count_visits", 1),), {}),
    ("count_visits2", (("count_visits", 2),), {}),
    ("wave_samples0", (("wave_samples", 0),), {}),
    ("wave_samples1", (("wave_samples", 1),), {}),
    ("wave_samples3", (("wave_samples", 3),), {}),
    ("wide_first0", (("wide_first", 0),), {}),
    ("wide_first1", (("wide_first", 1),), {}),
    ("streams2", (("streams", 2),), {}),
    ("lens", (), {"lens": True}),
    ("env", (), {"env": "shown"}),
    ("env_lens", (), {"env": "shown", "lens": True}),
    ("env_hidden", (), {"env": "hidden"}),
]


def configurations():
    """[(id, dict)]: every axis on every scene, the instance masks on the instanced scene, and one configuration that leaves the tile
    order adaptive (its hash alone is compared: when the tile measurement arrives is a host race that moves launch_info[0])"""
    out = []
    for scene in SCENES:
        for label, options, extra in AXES:
            cfg = {"scene": scene, "depth": 3, "n": 4, "options": [list(o) for o in options], "lens": False, "env": None, "adaptive": False}
            cfg.update(extra)
            out.append((f"{scene}-{label}", cfg))
    out.append(("instanced-instance_masks1", {"scene": "instanced", "depth": 3, "n": 4, "options": [["instance_masks", 1]], "lens": False,
                                              "env": None, "adaptive": False}))
    out.append(("big-adaptive_tiles", {"scene": "big", "depth": 3, "n": 7, "options": [], "lens": False, "env": None, "adaptive": True}))
    return out


def environment_texels():
    """a 4 x 4 map of exactly representable radiances"""
    return ((np.arange(4 * 4 * 3).reshape(4, 4, 3) % 7 + 1) / 8.0).astype(np.float32)


def lens_camera(cam):
    from caitlynrenderer_amd._lib import crt_camera
    c = crt_camera()
    C.memmove(C.byref(c), C.byref(cam.c), C.sizeof(crt_camera))
    c.aperture, c.focal_dist = float(np.float32(LENS[0])), float(np.float32(LENS[1]))
    return types.SimpleNamespace(c=c)


class Scenes:
    """cornell: conftest's (mesh, camera); candidates: [(name, mesh, SceneData)] by growing size, of which "big" is the first whose CWBVH has
    64 nodes or more (checked on the scene the library creates, once)"""

    def __init__(self, cr, cornell, cornell_data, candidates):
        self.cr, self.cornell, self.cornell_data, self.candidates = cr, cornell, cornell_data, candidates
        self.big_name = None

    def create(self, cfg):
        """-> (scene, what to close behind it)"""
        cr, (mesh, cam) = self.cr, self.cornell
        if cfg["scene"] == "cornell":
            sc = cr.Scene(self.cornell_data, W, H, cfg["depth"])
            assert sc.bvh_info()["n_nodes8"] < 64
            return sc, []
        if cfg["scene"] == "big":
            for name, _, data in self.candidates:
                if self.big_name not in (None, name):
                    continue
                sc = cr.Scene(data, W, H, cfg["depth"])
                if sc.bvh_info()["n_nodes8"] >= 64:
                    self.big_name = name
                    return sc, []
                sc.close()
            raise AssertionError("no candidate mesh has a CWBVH of 64 nodes")
        from test_instances_frames import shading_of, split_mesh
        from test_instances_oracle import IDENTITY
        meshes, _ = split_mesh(cr, mesh, 2)
        inst = cr.InstancedScene(meshes, cr.instances_array([IDENTITY, IDENTITY], np.arange(2), masks=[1, 2]), builder="sah")
        sc = inst.frame_scene(shading_of(meshes), mesh.materials, mesh.lights, W, H, cfg["depth"], textures=mesh.albedo_textures)
        sc.update(cam)
        return sc, [inst]


def observe(scenes, cfg):
    """One configuration on a fresh scene -> the record"""
    from caitlynrenderer_amd._lib import CrtError
    sc, behind = scenes.create(cfg)
    try:
        try:
            sc.set_option("adaptive_tiles", 1 if cfg["adaptive"] else 0)
            sc.set_option("timing", 2)
            sc.set_option("timing_accumulate", 256)
            for name, value in cfg["options"]:
                sc.set_option(name, value)
            if cfg["lens"]:
                sc.update(lens_camera(scenes.cornell[1]))
            if cfg["env"]:
                sc.set_environment(environment_texels(), hide_from_camera=cfg["env"] == "hidden")
            sc.render_frames(RVS[:cfg["n"]])
            rec = {"sha256": hashlib.sha256(sc.read_sum().tobytes()).hexdigest()}
            if not cfg["adaptive"]:
                st = sc.frame_stats()
                rec.update({"launch_info": sc.launch_info(), "n_launch_times": int(len(sc.launch_times())),
                            "closest_rays": int(st["closest_rays"]), "any_rays": int(st["any_rays"])})
            return rec
        except CrtError as e:
            return {"error": int(e.code)}
    finally:
        sc.close()
        for x in behind:
            x.close()
