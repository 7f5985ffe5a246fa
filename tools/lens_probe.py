"""Frames through the thin lens on the GPU: prints ONE JSON line.

The 1,004,672-triangle mesh at 1920 x 1080 from the Cornell camera, with aperture 0 (the pinhole: the fused first-segment kernels), a
SMALL aperture (1/1000 of the scene's extent, focused on the scene's centre: the rays of a wave still travel together) and a LARGE one
(1/10 of the extent, focused a tenth of the way in: the whole frame is out of focus and the primary rays of a wave diverge).  Per lens,
at max_depth 1 and 4 and at 1 and 4 samples per call:

  ms       ms per frame: wall time of --frames frames queued back to back in calls of that many samples and one synchronise, divided by
           the frames; median, minimum and maximum of --reps such batches after two warm-up batches;
  launches option "timing" 2 on one further call of one sample: the ray-generation launch alone (lens) beside its bandwidth floor — 32 B
           of ray and 40 B of path state written per path at 8 TB/s — and segment 0's launch: the queue-fed bounce kernel for a lens,
           the fused first-segment kernel for the pinhole.

Segment 0 of a lens frame runs the bounce kernel's lock-step walk: no uniform node steps, no origin kept in scalar registers, no tile
order; the table says what that costs.  Nothing here is tuned.

    python tools/lens_probe.py [--reps 7] [--frames 16]
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
BYTES_PER_PATH = 32 + 40


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
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
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
    pos, fwd = np.array(cam.c.position[:]), np.array(cam.c.forward[:])
    to_centre = float(np.dot(0.5 * (lo + hi) - pos, fwd))
    lenses = {"pinhole": (0.0, 0.1), "small": (ext / 1000.0, to_centre), "large": (ext / 10.0, 0.1 * to_centre)}
    out = {"probe": "lens", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "frames": args.frames, "reps": args.reps,
           "lenses": {k: [round(a, 6), round(f, 6)] for k, (a, f) in lenses.items()},
           "raygen_floor_ms_per_sample": round(W * H * BYTES_PER_PATH / HBM_BYTES_PER_MS, 5)}
    data = cr.SceneData.for_device_build(mesh, cam, builder="sah")
    for depth in (1, 4):
        for name, (aperture, focal) in lenses.items():
            c = crt_camera()
            C.memmove(C.byref(c), C.byref(cam.c), C.sizeof(crt_camera))
            c.aperture, c.focal_dist = aperture, focal
            scene = cr.Scene(data, W, H, depth)
            scene.update(type("Cam", (), {"c": c})())
            for per_call in (1, 4):
                out[f"{name}_d{depth}_spc{per_call}_ms"] = frame_ms(scene, rvs, per_call, args.reps)
            info = scene.launch_info()
            out[f"{name}_d{depth}_launch_info"] = info
            scene.set_option("timing", 2)
            scene.render_frame(*rvs[0])
            scene.render_frame(*rvs[1])
            times = [round(float(t), 4) for t in scene.launch_times()]
            if aperture > 0:
                out[f"{name}_d{depth}_raygen_ms"] = times[0]
                out[f"{name}_d{depth}_segment0_ms"] = times[1]
            else:
                out[f"{name}_d{depth}_segment0_ms"] = times[0]
            out[f"{name}_d{depth}_launch_ms"] = times
            st = scene.frame_stats()
            out[f"{name}_d{depth}_rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
            scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
