"""Frames of an instanced scene on the GPU: prints ONE JSON line.

At 1920 x 1080, max_depth 1 and 4, ms per frame (wall time of --frames frames queued back to back and one synchronise, divided by the
frames; median, minimum and maximum of --reps such batches after a warm-up batch) of

  grid     8 x 8 rotated copies of the 1,004,672-triangle mesh (one stored), seen from above the grid;
  one      ONE identity instance of that mesh through the instanced frame path, from the Cornell camera;
  flat_q   the flat crt_scene of the same mesh from the same camera with bounce_refill 1, inplace_shadow 0: the same launch structure
           (closest hits by a pool kernel, a shade-only pass, every shadow ray deferred to one any-hit launch), flat walk instead of the
           two-level one, first segment fused — what the two-level walk costs in frames;
  flat     the flat crt_scene with its default options (what a user who flattens one copy gets).

The flat kernels are the machine code of every earlier build of the library ("assembly"), so they are measured from this
library.

    python tools/instance_frame_probe.py [--reps 7] [--frames 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_ms(scene, rvs, reps):
    scene.render_frames(rvs)                       # warm-up: allocations, code objects, the flat scene's tile measurement
    scene.render_frames(rvs)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scene.render_frames(rvs)
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
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = 1920, 1080
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(args.frames)]
    out = {"probe": "instance_frames", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "frames": args.frames, "reps": args.reps}
    shading = [(mesh.triangles, mesh.normals, mesh.texcoords)]
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(8)
    M = []
    for gx in range(8):
        for gy in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
    from caitlynrenderer_amd._lib import crt_camera
    above = crt_camera()
    for k in ("right", "up", "forward"):
        for i in range(3):
            getattr(above, k)[i] = getattr(cam.c, k)[i]
    for i, x in enumerate((5.25 * ext, 5.25 * ext, 6 * ext)):
        above.position[i] = x
    above.fov, above.focal_dist, above.aperture = 1.2, 0.1, 0.0
    for depth in (1, 4):
        grid = cr.InstancedScene([mesh], cr.instances_array(np.array(M, np.float32), np.zeros(64)))
        sc = grid.frame_scene(shading, mesh.materials, mesh.lights, W, H, depth)
        sc.update(type("Cam", (), {"c": above})())
        out[f"grid_d{depth}_ms"] = frame_ms(sc, rvs, args.reps)
        st = sc.frame_stats()
        out[f"grid_d{depth}_rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
        out[f"grid_d{depth}_stack_overflows"] = int(st["stack_overflows"])
        sc.close(); grid.close()
        one = cr.InstancedScene([mesh], cr.instances_array([np.eye(3, 4, dtype=np.float32)], [0]))
        sc = one.frame_scene(shading, mesh.materials, mesh.lights, W, H, depth)
        sc.update(cam)
        out[f"one_d{depth}_ms"] = frame_ms(sc, rvs, args.reps)
        st = sc.frame_stats()
        out[f"one_d{depth}_rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
        sc.close(); one.close()
        data = cr.SceneData.for_device_build(mesh, cam, builder="sah")
        for name, opts in (("flat_q", {"bounce_refill": 1, "inplace_shadow": 0}), ("flat", {})):
            flat = cr.Scene(data, W, H, depth)
            flat.update(cam)
            for k, v in opts.items():
                flat.set_option(k, v)
            out[f"{name}_d{depth}_ms"] = frame_ms(flat, rvs, args.reps)
            flat.close()
        out[f"one_over_flat_q_d{depth}"] = round(out[f"one_d{depth}_ms"]["median"] / out[f"flat_q_d{depth}_ms"]["median"], 3)
        out[f"one_over_flat_d{depth}"] = round(out[f"one_d{depth}_ms"]["median"] / out[f"flat_d{depth}_ms"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
