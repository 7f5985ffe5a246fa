"""Frames along the caller's camera rays on the GPU: prints ONE JSON line.

The 1,004,672-triangle mesh at 1920 x 1080 from the Cornell camera, four ways, at max_depth 1 and 4 and at 1 and 4 samples per call:

  pinhole    the camera at option "jitter" 0: the fused first-segment kernels;
  same_rays  camera rays equal to cameras.pinhole_rays: the same rays, the same bits, through k_raygen_rays and the queue-fed segments —
             the price of the queue-fed form;
  lens       a small lens (1/1000 of the scene's extent, focused on its centre), for comparison: the other queue-fed generator;
  panorama   camera rays of an equirectangular panorama from the scene's centre: rays of a wave that leave in all directions.

  ms         ms per frame: wall time of --frames frames queued back to back in calls of that many samples and one synchronise, divided
             by the frames; median, minimum and maximum of --reps such batches after two warm-up batches;
  launches   option "timing" 2 on one further call of one sample: the ray-generation launch alone beside its bandwidth floor — 32 B of
             ray read, 32 B of ray and 40 B of path state written per path at 8 TB/s — and segment 0's launch;
  set        wall ms of one set of 1080p rays through crt_set_camera_rays (host pointer) and crt_set_camera_rays_device (device pointer),
             median, minimum and maximum of --reps calls after two.

Nothing here is tuned.

    python tools/camera_rays_probe.py [--reps 7] [--frames 16]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_MS = 8e12 / 1e3
BYTES_PER_PATH = 32 + 32 + 40


def spread(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def frame_ms(scene, rvs, per_call, reps):
    def batch():
        for i in range(0, len(rvs), per_call):
            scene.render_frames(rvs[i:i + per_call], sync=False)
        scene.sync()
    batch()                                        # warm-up: allocations, code objects, the pinhole's tile measurement
    batch()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        batch()
        ts.append((time.perf_counter() - t0) * 1e3 / len(rvs))
    return spread(ts)


def call_ms(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd._lib import crt_camera
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = 1920, 1080
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(args.frames)]
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    ext = float((hi - lo).max())
    centre = 0.5 * (lo + hi)
    pos, fwd = np.array(cam.c.position[:]), np.array(cam.c.forward[:])
    lens = crt_camera()
    C.memmove(C.byref(lens), C.byref(cam.c), C.sizeof(crt_camera))
    lens.aperture, lens.focal_dist = ext / 1000.0, float(np.dot(centre - pos, fwd))
    ways = {"pinhole": None, "same_rays": cr.pinhole_rays(cam, W, H), "lens": lens,
            "panorama": cr.panorama_rays(centre, W, H, forward=fwd, up=np.array(cam.c.up[:]))}
    out = {"probe": "camera_rays", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "frames": args.frames, "reps": args.reps,
           "raygen_floor_ms_per_sample": round(W * H * BYTES_PER_PATH / HBM_BYTES_PER_MS, 5)}
    data = cr.SceneData.for_device_build(mesh, cam, builder="sah")
    for depth in (1, 4):
        for name, way in ways.items():
            scene = cr.Scene(data, W, H, depth)
            scene.set_option("jitter", 0)
            if isinstance(way, tuple):
                scene.set_camera_rays(*way)
            elif way is not None:
                scene.update(type("Cam", (), {"c": way})())
            for per_call in (1, 4):
                out[f"{name}_d{depth}_spc{per_call}_ms"] = frame_ms(scene, rvs, per_call, args.reps)
            out[f"{name}_d{depth}_launch_info"] = scene.launch_info()
            scene.set_option("timing", 2)
            scene.render_frame(*rvs[0])
            scene.render_frame(*rvs[1])
            times = [round(float(t), 4) for t in scene.launch_times()]
            if way is not None:
                out[f"{name}_d{depth}_raygen_ms"] = times[0]
                out[f"{name}_d{depth}_segment0_ms"] = times[1]
            else:
                out[f"{name}_d{depth}_segment0_ms"] = times[0]
            out[f"{name}_d{depth}_launch_ms"] = times
            st = scene.frame_stats()
            out[f"{name}_d{depth}_rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
            if name == "panorama" and depth == 1:
                rays = scene.camera_rays_array(*way)
                dev = torch.from_numpy(rays.view(np.uint8)).cuda()
                torch.cuda.synchronize()
                from caitlynrenderer_amd._lib import check, lib
                from caitlynrenderer_amd.host import _ptr
                out["set_host_ms"] = call_ms(lambda: check(lib().crt_set_camera_rays(scene._h, _ptr(rays), rays.shape[0])), args.reps)
                out["set_device_ms"] = call_ms(lambda: scene.set_camera_rays_device(dev.data_ptr()), args.reps)
                out["set_bytes"] = int(rays.nbytes)
                del dev
            scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
