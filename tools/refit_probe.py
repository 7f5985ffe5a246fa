"""Measurement, not a test: what crt_update_vertices costs on mesh1m and what refitting instead of rebuilding costs the frames.

Prints one JSON line: device / wall ms of the host and device update forms, the wall ms of crt_scene_create with the device SAH build
on the same mesh, and the frame ms of one- and four-segment frames (1920 x 1080, four samples per launch) at displacement amplitudes
0.02 (the mesh as built), 0.1 and 0.5 — once on the scene built at 0.02 and refitted, once on a scene built fresh at that amplitude.

    python tools/refit_probe.py [--n 183] [--reps 10] [--out refit_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_ms(scene, reps):
    rvs = [(0.25 + 0.01 * k, 0.75 - 0.01 * k) for k in range(4)]
    scene.render_frames(rvs)                          # warm-up: tile costs measured, code objects loaded
    scene.render_frames(rvs)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scene.render_frames(rvs)
        ts.append((time.perf_counter() - t0) * 1e3 / len(rvs))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=183, help="tessellation (183 = mesh1m)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, cam = g._cornell()
    amps = (0.02, 0.1, 0.5)
    meshes = {amp: tessellated_cornell(base, a.n, amp) for amp in amps}
    m0 = meshes[0.02]
    out = {"triangles": int(m0.triangles.shape[0]), "vertices": int(m0.vertices.shape[0])}
    W, H = 1920, 1080

    # crt_scene_create with the device SAH build, and the update forms on that scene
    creates = []
    for _ in range(3):
        s = cr.Scene(cr.SceneData.for_device_build(m0, cam, "sah"), W, H, 1)
        creates.append(s.create_ms)
        out["node8"] = int(s.bvh_info()["n_nodes8"])
        s.close()
    out["create_sah_wall_ms"] = statistics.median(creates)
    sc = cr.Scene(cr.SceneData.for_device_build(m0, cam, "sah"), W, H, 1)
    sc.update_vertices(meshes[0.1].vertices)          # the first update allocates the refit's state and finds the levels
    first = sc.last_update_ms()
    out["first_update_host_ms"] = {"device": first[0], "wall": first[1]}
    host = [None] * a.reps
    for k in range(a.reps):
        sc.update_vertices(meshes[0.1 if k % 2 else 0.5].vertices)
        host[k] = sc.last_update_ms()
    t = torch.from_numpy(meshes[0.1].vertices).to("cuda")
    t2 = torch.from_numpy(meshes[0.5].vertices).to("cuda")
    torch.cuda.synchronize()
    dev = [None] * a.reps
    for k in range(a.reps):
        x = t if k % 2 else t2
        sc.update_vertices_device(x.data_ptr(), x.shape[0], sync=True)
        dev[k] = sc.last_update_ms()
    out["update_host_form_ms"] = {"device": statistics.median(h[0] for h in host), "wall": statistics.median(h[1] for h in host)}
    out["update_device_form_ms"] = {"device": statistics.median(d[0] for d in dev), "wall": statistics.median(d[1] for d in dev)}
    sc.close()

    # frame cost of a refitted tree against a fresh build, one and four segments
    frames = {}
    for depth in (1, 4):
        refit = cr.Scene(cr.SceneData.for_device_build(m0, cam, "sah"), W, H, depth)
        for amp in amps:
            refit.update_vertices(meshes[amp].vertices)
            fresh = cr.Scene(cr.SceneData.for_device_build(meshes[amp], cam, "sah"), W, H, depth)
            fr, fx = frame_ms(refit, a.reps), frame_ms(fresh, a.reps)
            frames[f"depth{depth}_amp{amp}"] = {"refit_ms": fr, "fresh_ms": fx, "refit_over_fresh": fr / fx}
            fresh.close()
        refit.close()
    out["frames"] = frames
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
