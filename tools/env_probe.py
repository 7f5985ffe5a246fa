"""Frames with an environment on the GPU: prints ONE JSON line.

The 1,004,672-triangle mesh at 1920 x 1080 from the Cornell camera, with and without a 64 x 64 octahedral environment (a smooth sky
function, rotated, scale 1), through the pinhole and through §27's SMALL lens (aperture 1/1000 of the scene's extent, focused on the
scene's centre).  Per arm, at max_depth 1 and 4:

  ms       ms per frame: wall time of --frames frames queued back to back, one sample per call, and one synchronise, divided by the
           frames; median, minimum and maximum of --reps such batches after two warm-up batches (tools/lens_probe.py's measure);
  env_miss option "timing" 2 on one further frame: k_env_miss' own spans, one per segment, beside the bytes it moves / 8 TB/s — 4 B of hit
           word per queue entry and, per miss, 16 B of ray row, 16 B of throughput, 64 B of taps, 16 B of slot and 4 B of flag word.  The
           misses of a frame, all segments together, come from one counting frame (closest rays - closest hits), and the floor of segment 0
           is given for no miss and for every entry missing.

Without an environment the pinhole frame is the parent commit's fused frame; with one it is k_raygen, then per segment k_closest_queue,
k_env_miss and the shade-only pass, then k_shadow_deferred and k_fold_paths.  Nothing here is tuned.

    python tools/env_probe.py [--reps 7] [--frames 16]
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
BYTES_PER_ENTRY, BYTES_PER_MISS = 4, 16 + 16 + 64 + 16 + 4


def frame_ms(scene, rvs, reps):
    def batch():
        for rv in rvs:
            scene.render_frames([rv], sync=False)
        scene.sync()
    batch()                                        # warm-up: allocations, code objects, the pinhole's tile measurement
    batch()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        batch()
        ts.append((time.perf_counter() - t0) * 1e3 / len(rvs))
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def sky(d):
    up = 0.5 + 0.5 * d[:, 1]
    return np.stack([0.4 + 0.6 * up, 0.5 + 0.5 * up, 0.7 + 0.3 * up * up], -1) * (1.0 + 0.25 * d[:, [0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd._lib import crt_camera
    from caitlynrenderer_amd.environment import octahedral_from_function
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = args.width, args.height
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(args.frames)]
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    ext = float((hi - lo).max())
    pos, fwd = np.array(cam.c.position[:]), np.array(cam.c.forward[:])
    to_centre = float(np.dot(0.5 * (lo + hi) - pos, fwd))
    lenses = {"pinhole": (0.0, 0.1), "small": (ext / 1000.0, to_centre)}
    texels = octahedral_from_function(sky, 64)
    c_, s_ = np.cos(0.6), np.sin(0.6)
    rotation = np.array([[c_, 0, s_], [0, 1, 0], [-s_, 0, c_]], np.float32)
    out = {"probe": "env", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "frames": args.frames, "reps": args.reps,
           "map_size": 64, "lenses": {k: [round(a, 6), round(f, 6)] for k, (a, f) in lenses.items()}}
    data = cr.SceneData.for_device_build(mesh, cam, builder="sah")
    for depth in (1, 4):
        for name, (aperture, focal) in lenses.items():
            c = crt_camera()
            C.memmove(C.byref(c), C.byref(cam.c), C.sizeof(crt_camera))
            c.aperture, c.focal_dist = aperture, focal
            for env in (False, True):
                scene = cr.Scene(data, W, H, depth)
                scene.update(type("Cam", (), {"c": c})())
                if env:
                    scene.set_environment(texels, rotation)
                key = f"{name}_d{depth}_{'env' if env else 'none'}"
                out[key + "_ms"] = frame_ms(scene, rvs, args.reps)
                out[key + "_launch_info"] = scene.launch_info()
                if env:
                    scene.set_option("timing", 2)
                    scene.render_frame(*rvs[0])
                    scene.render_frame(*rvs[1])
                    times = [round(float(t), 4) for t in scene.launch_times()]
                    # span order: ray generation, then per segment (closest hit + shade-only pass, k_env_miss inside it), then the shadow launch
                    out[key + "_launch_ms"] = times
                    out[key + "_env_miss_ms"] = [times[2 + 2 * k] for k in range(depth) if 2 + 2 * k < len(times)]
                    st = scene.frame_stats()
                    out[key + "_closest_rays"] = int(st["closest_rays"])
                    scene.set_option("timing", 0)
                    scene.set_option("count_visits", 1)            # a counting frame: the rays that found a surface, all segments together
                    scene.render_frame(*rvs[1])
                    st = scene.frame_stats()
                    out[key + "_misses_all_segments"] = int(st["closest_rays"] - st["closest_hits"])
                    entries = W * H
                    out[key + "_env_miss_floor_ms_segment0"] = {"no_miss": round(entries * BYTES_PER_ENTRY / HBM_BYTES_PER_MS, 5),
                                                                 "all_miss": round(entries * (BYTES_PER_ENTRY + BYTES_PER_MISS) / HBM_BYTES_PER_MS, 5)}
                scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
