"""Material offsets and visibility masks in the frames of an instanced scene on the GPU: prints ONE JSON line.

The scene and the method are tools/instance_frame_probe.py's: 8 x 8 rotated copies of the 1,004,672-triangle mesh (one stored), seen from
above the grid, 1920 x 1080, max_depth 1 and 4; ms per frame = wall time of --frames frames queued back to back and one synchronise,
divided by the frames; median, minimum and maximum of --reps such batches after two warm-up batches.  Per depth, on ONE handle and scene:

  plain              instance_masks 0, every offset 0 (what the parent library renders too: see --only-plain)
  masks_on           (a) instance_masks 1, every instance and class mask 0xff: the cost of the mode
  hide_half_masked   (b) a contiguous half (the first 32 instances) hidden by mask 0, instance_masks 1
  hide_checker_masked    the checkerboard half hidden the same way
  half_set, checker_set  instance_masks 0 and the handle `set` to the visible half: what hiding by a set renders
  random_offsets     (c) instance_masks 0, every instance a random multiple of the table's period as offset into the material table
                     repeated 8 times: the same pictures from other table rows

--only-plain measures `plain` alone: with CRT_LIB pointing at another build of the library (this change adds no exported symbol) it is
the A/B of the shade kernel's one more load, run alternately from a job script.

    python tools/instance_frame_mask_probe.py [--reps 5] [--frames 16] [--only-plain]
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
    scene.render_frames(rvs)                       # two warm-up batches: allocations, code objects, the child-mask pass
    scene.render_frames(rvs)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scene.render_frames(rvs)
        ts.append((time.perf_counter() - t0) * 1e3 / len(rvs))
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--only-plain", action="store_true")
    ap.add_argument("--depths", default="1,4")
    args = ap.parse_args()
    import __graft_entry__ as g
    if not os.environ.get("CRT_LIB"):
        g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd._lib import LIB_PATH, crt_camera
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = 1920, 1080
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(args.frames)]
    out = {"probe": "instance_frame_masks", "library": os.path.relpath(LIB_PATH, ROOT), "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H,
           "frames": args.frames, "reps": args.reps}
    shading = [(mesh.triangles, mesh.normals, mesh.texcoords)]
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(8)
    M, checker = [], []
    for gx in range(8):
        for gy in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
            checker.append((gx + gy) & 1)
    M, checker = np.array(M, np.float32), np.array(checker, bool)
    first_half = np.arange(64) < 32
    above = crt_camera()
    for k in ("right", "up", "forward"):
        for i in range(3):
            getattr(above, k)[i] = getattr(cam.c, k)[i]
    for i, x in enumerate((5.25 * ext, 5.25 * ext, 6 * ext)):
        above.position[i] = x
    above.fov, above.focal_dist, above.aperture = 1.2, 0.1, 0.0
    period = mesh.materials.shape[0]
    table = np.tile(mesh.materials, (8, 1))
    offsets = (period * rng.integers(0, 8, 64)).astype(np.uint32)
    zeros64 = np.zeros(64, np.uint32)

    def records(hidden=None, offs=None, keep=None):
        masks = np.where(hidden, 0, 0xff) if hidden is not None else np.full(64, 0xff)
        a = cr.instances_array(M, zeros64, masks)
        if offs is not None:
            a["reserved"][:, 0] = offs             # the word at byte 56, under its old name: every build's binding has it
        return a if keep is None else a[keep]

    for depth in (int(x) for x in args.depths.split(",")):
        grid = cr.InstancedScene([mesh], records(), capacity=64)
        sc = grid.frame_scene(shading, table, mesh.lights, W, H, depth)
        sc.update(type("Cam", (), {"c": above})())
        key = f"d{depth}_"
        out[key + "plain_ms"] = frame_ms(sc, rvs, args.reps)
        st = sc.frame_stats()
        out[key + "rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
        if not args.only_plain:
            sc.set_option("instance_masks", 1)
            out[key + "masks_on_ms"] = frame_ms(sc, rvs, args.reps)
            for name, hidden in (("half", first_half), ("checker", checker)):
                sc.set_option("instance_masks", 1)
                grid.refit(records(hidden))
                out[key + f"hide_{name}_masked_ms"] = frame_ms(sc, rvs, args.reps)
                st = sc.frame_stats()
                out[key + f"hide_{name}_rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
                sc.set_option("instance_masks", 0)
                grid.set(records(keep=~hidden))
                out[key + f"{name}_set_ms"] = frame_ms(sc, rvs, args.reps)
                st = sc.frame_stats()
                out[key + f"{name}_set_rays_per_frame"] = int(st["closest_rays"] + st["any_rays"])
                grid.set(records())
            grid.set(records(offs=offsets))
            out[key + "random_offsets_ms"] = frame_ms(sc, rvs, args.reps)
            grid.set(records())
            out[key + "plain_again_ms"] = frame_ms(sc, rvs, args.reps)
            st = sc.frame_stats()
            out[key + "stack_overflows"] = int(st["stack_overflows"])
            p = out[key + "plain_ms"]["median"]
            out[key + "masks_on_over_plain"] = round(out[key + "masks_on_ms"]["median"] / p, 4)
            out[key + "random_offsets_over_plain"] = round(out[key + "random_offsets_ms"]["median"] / out[key + "plain_again_ms"]["median"], 4)
            for name in ("half", "checker"):
                out[key + f"hide_{name}_masked_over_set"] = round(out[key + f"hide_{name}_masked_ms"]["median"] / out[key + f"{name}_set_ms"]["median"], 4)
        sc.close(); grid.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
