"""First-hit feature buffers on the GPU: prints ONE JSON line.

At 1920 x 1080, ms per crt_render_aov call (wall time of --calls calls queued back to back and one synchronise, divided by the calls;
median, minimum and maximum of --reps such batches after two warm-up batches), all channels and HIT | IDS only, of

  flat     the flat crt_scene of the 1,004,672-triangle mesh from the Cornell camera;
  grid     8 x 8 rotated copies of that mesh (one stored), seen from above the grid, through the instanced path;

and beside each a max_depth 1 frame of the same scene in the same session, measured the same way.

    python tools/aov_probe.py [--reps 5] [--calls 16] [--png DIR]

--png DIR writes the normal, albedo and depth views of both scenes as PNG files.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch_ms(enqueue, sync, n, reps):
    """enqueue() n times and one sync(): ms per call; two warm-up batches, then `reps` timed ones"""
    ts = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        for i in range(n):
            enqueue(i)
        sync()
        if k >= 2:
            ts.append((time.perf_counter() - t0) * 1e3 / n)
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def measure(cr, sc, rvs, reps):
    out = {}
    for name, channels in (("aov_all", cr.AOV_ALL), ("aov_hit_ids", cr.AOV_HIT | cr.AOV_IDS)):
        out[name + "_ms"] = batch_ms(lambda i: sc.render_aov(rvs[i][0], rvs[i][1], channels=channels, sync=False), sc.sync, len(rvs), reps)
    out["frame_d1_ms"] = batch_ms(lambda i: sc.render_frame(rvs[i][0], rvs[i][1], sync=False), sc.sync, len(rvs), reps)
    out["aov_all_over_frame"] = round(out["aov_all_ms"]["median"] / out["frame_d1_ms"]["median"], 3)
    return out


def views(cr, sc):
    """(normal, albedo, depth) as bottom-up RGBA8 images: n / |n| mapped to [0, 1], the albedo as it is, t scaled to its largest hit value"""
    sc.render_aov(0.5, 0.5)
    hit, nrm, alb = sc.read_aov(cr.AOV_HIT), sc.read_aov(cr.AOV_NORMAL), sc.read_aov(cr.AOV_ALBEDO)
    seen = hit["tri"] >= 0
    ln = np.sqrt((nrm[..., :3].astype(np.float64) ** 2).sum(-1, keepdims=True))
    n01 = np.where(seen[..., None], 0.5 + 0.5 * nrm[..., :3] / np.where(ln > 0, ln, 1.0), 0.0)
    t = np.where(seen, hit["t"], 0.0).astype(np.float64)
    d01 = np.where(seen, 1.0 - t / max(float(t.max()), 1e-30), 0.0)

    def rgba(a):
        img = np.full(a.shape[:2] + (4,), 255, np.uint8)
        img[..., :3] = np.clip(a * 255.0 + 0.5, 0, 255).astype(np.uint8)
        return img
    return rgba(n01), rgba(np.clip(alb[..., :3], 0, 1)), rgba(np.repeat(d01[..., None], 3, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--png", default=None, help="directory for the normal / albedo / depth views")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.image import write_png
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = args.width, args.height
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(args.calls)]
    out = {"probe": "aov", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "calls": args.calls, "reps": args.reps}
    if args.png:
        os.makedirs(args.png, exist_ok=True)

    def pictures(name, sc):
        if args.png:
            for what, img in zip(("normal", "albedo", "depth"), views(cr, sc)):
                write_png(os.path.join(args.png, f"{name}_{what}.png"), img)

    flat = cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder="sah"), W, H, 1)
    flat.update(cam)
    out["flat"] = measure(cr, flat, rvs, args.reps)
    pictures("flat", flat)
    flat.close()
    # the 8 x 8 grid of tools/instance_frame_probe.py
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
    grid = cr.InstancedScene([mesh], cr.instances_array(np.array(M, np.float32), np.zeros(64)))
    sc = grid.frame_scene([(mesh.triangles, mesh.normals, mesh.texcoords)], mesh.materials, mesh.lights, W, H, 1)
    sc.update(type("Cam", (), {"c": above})())
    out["grid"] = measure(cr, sc, rvs, args.reps)
    pictures("grid", sc)
    sc.close(); grid.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
