"""Lights that follow emissive instances on the GPU: prints ONE JSON line.

  rebuild   ms of one rebuild of the world light table — per-instance counts and scan, the read of the total, transform, tree sum, pdf
            column — at 1 k, 16 k and 256 k instances of a two-triangle mesh that carries two lights: the wall time of a
            crt_scene_read_lights count query behind a crt_instances_refit plus the wait for the scene's stream (median, minimum and
            maximum of --reps refits), and what the refit itself took, for scale;
  frames    ms per frame at 1920 x 1080, max_depth 1 and 4, of §16's scene — 8 x 8 rotated copies of the 1,004,672-triangle mesh seen from
            above — created with crt_scene_create_instanced (the figure tools/instance_frame_probe.py reports, and what the parent
            commit's library is compared by) and created with the mesh's lights as mesh lights (64 x 2 lights instead of 2).

    python tools/instance_lights_probe.py [--reps 7] [--frames 16] [--skip-frames]
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


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def rebuild_ms(cr, n, reps):
    from caitlynrenderer_amd._lib import lib
    rng = np.random.default_rng(18)
    v = np.array([[-1, 0, -1], [-1, 0, 1], [1, 0, 1], [1, 0, -1]], np.float32)
    t = np.array([[0, 1, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 2, 3, 0, 0, 0, 0, 1, 0, 0, 0, 0]], np.int32)
    mats = np.zeros((1, 16), np.float32)
    mats[0, 4:8], mats[0, 12:16] = (3, 3, 3, 0), -1
    lights = np.array([np.concatenate([v[0], v[1] - v[0], v[2] - v[0], (0, -1, 0), (3, 3, 3), (4, 0, 0)]),
                       np.concatenate([v[0], v[2] - v[0], v[3] - v[0], (0, -1, 0), (3, 3, 3), (4, 0, 0)])], np.float32)

    def matrices():
        M = np.zeros((n, 3, 4), np.float32)
        a = rng.uniform(0, 2 * np.pi, n)
        s = rng.uniform(0.5, 2.0, n)
        M[:, 0, 0], M[:, 0, 2], M[:, 2, 0], M[:, 2, 2], M[:, 1, 1] = np.cos(a) * s, np.sin(a) * s, -np.sin(a) * s, np.cos(a) * s, s
        M[:, :, 3] = rng.uniform(-1, 1, (n, 3)) * (4.0 * n ** (1 / 3))
        return M

    inst = cr.InstancedScene([(v, t)], cr.instances_array(matrices(), np.zeros(n)))
    sc = inst.frame_scene([(t, np.array([[0, 1, 0]], np.float32), None)], mats, np.zeros((0, 18), np.float32), 64, 64, 2, mesh_lights=[lights])
    count = C.c_size_t()
    ts, refit = [], []
    for k in range(reps + 1):
        inst.refit(cr.instances_array(matrices(), np.zeros(n)))
        refit.append(inst.info()["set_wall_ms"])
        t0 = time.perf_counter()
        lib().crt_scene_read_lights(sc._h, None, 0, C.byref(count))
        sc.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    assert count.value == 2 * n
    sc.close(); inst.close()
    return {"lights": 2 * n, "rebuild_ms": stats(ts[1:]), "refit_wall_ms": stats(refit[1:])}       # the first rebuild allocates the table


def frame_ms(scene, rvs, reps):
    scene.render_frames(rvs)
    scene.render_frames(rvs)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scene.render_frames(rvs)
        ts.append((time.perf_counter() - t0) * 1e3 / len(rvs))
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--skip-rebuild", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    cr.warmup()
    out = {"probe": "instance_lights", "reps": args.reps}
    if not args.skip_rebuild:
        for n in (1024, 16384, 262144):
            out[f"rebuild_{n}"] = rebuild_ms(cr, n, args.reps)
    if not args.skip_frames:
        from caitlynrenderer_amd._lib import crt_camera
        from caitlynrenderer_amd.meshgen import tessellated_cornell
        base, cam = g._cornell()
        mesh = tessellated_cornell(base, args.tess)
        W, H = 1920, 1080
        rnd = cr.Rnd()
        rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(args.frames)]
        ext = float((mesh.vertices.max(0) - mesh.vertices.min(0)).max())
        rng = np.random.default_rng(8)
        M = []
        for gx in range(8):
            for gy in range(8):
                q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
                M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
        above = crt_camera()
        for k in ("right", "up", "forward"):
            for i in range(3):
                getattr(above, k)[i] = getattr(cam.c, k)[i]
        for i, x in enumerate((5.25 * ext, 5.25 * ext, 6 * ext)):
            above.position[i] = x
        above.fov, above.focal_dist, above.aperture = 1.2, 0.1, 0.0
        shading = [(mesh.triangles, mesh.normals, mesh.texcoords)]
        out.update({"triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "frames": args.frames})
        for depth in (1, 4):
            for name, kw in (("grid", {}), ("grid_lit", {"mesh_lights": [mesh.lights]})):
                grid = cr.InstancedScene([mesh], cr.instances_array(np.array(M, np.float32), np.zeros(64)))
                lights = mesh.lights if name == "grid" else np.zeros((0, 18), np.float32)
                sc = grid.frame_scene(shading, mesh.materials, lights, W, H, depth, **kw)
                sc.update(type("Cam", (), {"c": above})())
                out[f"{name}_d{depth}_ms"] = frame_ms(sc, rvs, args.reps)
                sc.close(); grid.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
