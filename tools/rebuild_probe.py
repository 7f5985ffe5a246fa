"""Measurement, not a test: what crt_rebuild_vertices costs on mesh1m, and how well crt_get_tree_cost predicts what a rebuild gains.

Prints one JSON line (the method of tools/refit_probe.py: medians of --reps after warm-up, 1920 x 1080, device SAH build):
  - device / wall ms of both rebuild forms, the first rebuild separately, beside crt_update_vertices and beside crt_scene_destroy +
    crt_scene_create of the same positions in the same session;
  - for both deformations of DESIGN.md §19 (the displacement field of tessellated_cornell, and blocks of (n+1)^2 vertices scattered at
    random), several amplitudes each: tree_cost().cost and ms per frame at max_depth 1 and 4 of the refitted scene and of the rebuilt
    one, so the cost ratio can be read beside the frame-time ratio;
  - the TLAS cost after crt_instances_refit to scattered placements against a crt_instances_set of the same array, 16 k instances.

    python tools/rebuild_probe.py [--n 183] [--reps 10] [--instances 16384] [--out rebuild_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

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


def scatter(vertices, block, amp, seed):
    """amp * (pcg_hash(3 * (i // block) + k + 7919 * seed) / 2^32 - 0.5) added to coordinate k of vertex i (tests/test_rebuild.py)"""
    from caitlynrenderer_amd.meshgen import pcg_hash_np
    V = vertices.astype(np.float64)
    i = np.arange(V.shape[0], dtype=np.uint64)
    for k in range(3):
        h = pcg_hash_np((np.uint64(3) * (i // np.uint64(block)) + np.uint64(k + 7919 * seed)) & np.uint64(0xFFFFFFFF)).astype(np.float64)
        V[:, k] += amp * (h / 4294967296.0 - 0.5)
    return V.astype(np.float32)


def med(pairs):
    return {"device": statistics.median(p[0] for p in pairs), "wall": statistics.median(p[1] for p in pairs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=183, help="tessellation (183 = mesh1m)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--instances", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, cam = g._cornell()
    m0 = tessellated_cornell(base, a.n, 0.02)
    block = (a.n + 1) ** 2
    poses = {"displace": {amp: tessellated_cornell(base, a.n, amp).vertices for amp in (0.1, 0.5, 2.0)},
             "scatter": {amp: scatter(m0.vertices, block, amp, 1) for amp in (1.5, 3.0, 6.0)}}
    out = {"triangles": int(m0.triangles.shape[0]), "vertices": int(m0.vertices.shape[0])}
    W, H = 1920, 1080
    va, vb = poses["scatter"][3.0], poses["scatter"][6.0]

    def fresh_mesh(v):
        return cr.Mesh(v, m0.normals, m0.texcoords, m0.triangles, m0.materials, m0.lights, m0.vertex_min)

    # the rebuild forms, an update, and destroy + create of the same positions, one session
    sc = cr.Scene(cr.SceneData.for_device_build(m0, cam, "sah"), W, H, 1)
    out["node8"] = int(sc.bvh_info()["n_nodes8"])
    sc.rebuild_vertices(va)                           # the first rebuild scatters the triangles back to source order and allocates
    first = sc.last_update_ms()
    out["first_rebuild_host_ms"] = {"device": first[0], "wall": first[1]}
    host = []
    for k in range(a.reps):
        sc.rebuild_vertices(vb if k % 2 else va)
        host.append(sc.last_update_ms())
    ta, tb = torch.from_numpy(va).to("cuda"), torch.from_numpy(vb).to("cuda")
    torch.cuda.synchronize()
    dev = []
    for k in range(a.reps):
        x = tb if k % 2 else ta
        sc.rebuild_vertices_device(x.data_ptr(), x.shape[0])
        dev.append(sc.last_update_ms())
    upd = []
    sc.update_vertices(va)
    for k in range(a.reps):
        sc.update_vertices(vb if k % 2 else va)
        upd.append(sc.last_update_ms())
    out["rebuild_host_form_ms"], out["rebuild_device_form_ms"], out["update_host_form_ms"] = med(host), med(dev), med(upd)
    recreate = []
    for k in range(a.reps):
        data = cr.SceneData.for_device_build(fresh_mesh(vb if k % 2 else va), cam, "sah")
        t0 = time.perf_counter()
        sc.close()
        sc = cr.Scene(data, W, H, 1)                  # create_ms: crt_scene_create alone; the pair: destroy + create as a caller pays it
        recreate.append((sc.create_ms, (time.perf_counter() - t0) * 1e3))
    out["destroy_create_ms"] = {"create": statistics.median(r[0] for r in recreate), "destroy_plus_create": statistics.median(r[1] for r in recreate)}
    sc.close()

    # does the cost ratio predict the frame-time ratio?  Refitted against rebuilt, same positions, one and four segments
    frames = {}
    for depth in (1, 4):
        for kind, by_amp in poses.items():
            for amp, v in by_amp.items():
                s = cr.Scene(cr.SceneData.for_device_build(m0, cam, "sah"), W, H, depth)
                s.update_vertices(v)
                c_refit, f_refit = s.tree_cost()["cost"], frame_ms(s, a.reps)
                s.rebuild_vertices(v)
                c_rebuilt, f_rebuilt = s.tree_cost()["cost"], frame_ms(s, a.reps)
                s.close()
                frames[f"depth{depth}_{kind}{amp}"] = {"cost_refit": c_refit, "cost_rebuilt": c_rebuilt, "cost_ratio": c_refit / c_rebuilt,
                                                       "refit_ms": f_refit, "rebuilt_ms": f_rebuilt, "frame_ratio": f_refit / f_rebuilt}
    out["frames"] = frames

    # TLAS: a refit to scattered placements against a set of the same array
    n_i = a.instances
    small = tessellated_cornell(base, 8, 0.02)
    rng = np.random.default_rng(5)
    mats = np.zeros((n_i, 3, 4), np.float32)
    mats[:, :, :3] = np.eye(3, dtype=np.float32)
    side = int(np.ceil(n_i ** (1.0 / 3.0)))
    grid = np.stack(np.unravel_index(np.arange(n_i), (side, side, side)), 1).astype(np.float32)
    mats[:, :, 3] = grid * np.float32(700.0)
    inst = cr.instances_array(mats, np.zeros(n_i, np.uint32))
    h = cr.InstancedScene([small], inst, builder="sah")
    tl = {"instances": n_i, "cost_built": h.tree_cost(-1)["cost"]}
    moved = inst.copy()
    mm = mats.copy()
    mm[:, :, 3] = rng.uniform(0.0, 700.0 * side, (n_i, 3)).astype(np.float32)
    moved["object_to_world"] = mm.reshape(n_i, 12)
    h.refit(moved)
    tl["cost_refit"], tl["refit_wall_ms"] = h.tree_cost(-1)["cost"], h.info()["set_wall_ms"]
    h.set(moved)
    tl["cost_set"], tl["set_wall_ms"] = h.tree_cost(-1)["cost"], h.info()["set_wall_ms"]
    tl["cost_ratio"] = tl["cost_refit"] / tl["cost_set"]
    h.close()
    out["tlas"] = tl
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
