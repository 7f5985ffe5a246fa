"""Measurement, not a test: what crt_instances_update_meshes costs, and what the refitted BLAS costs the trace.

Prints one JSON line:
  (a) mesh1m under 64 instances (8 x 8 rotated copies): device / wall ms of the host and the device update forms (medians after
      warm-up), against the wall ms of crt_instances_create of the same scene;
  (b) 256 small displaced meshes, one instance each: one call updating all 256 against 256 single-mesh calls (wall ms);
  (c) closest-hit Mray/s on (a)'s scene after an update to displacement amplitude 0.1 and 0.5, against a fresh create from the same
      vertices (2 M rays, medians of synchronous crt_instances_trace_device calls after two warm-ups, wall time around the call, as
      tools/instance_probe.py measures).

    python tools/instance_update_probe.py [--n 183] [--reps 10] [--out instance_update_probe.json]
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
f32 = np.float32


def grid_instances(ext, rng):
    M = []
    for gx in range(8):
        for gy in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
    return np.array(M, f32)


def grid_rays(cr, rng, n, ext, M):
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"] = (rng.uniform(-6 * ext, 6 * ext, (n, 3)) + 5.25 * ext * np.array([1, 1, 0])).astype(f32)
    d = rng.normal(size=(n, 3))
    k = n // 2
    tgt = M[rng.integers(0, len(M), k), :, 3] + rng.normal(scale=ext * 0.3, size=(k, 3))
    d[:k] = tgt - rays["o"][:k]
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmax"] = f32(1e9)
    return rays


def mrays(sc, torch, rays, reps):
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        sc.trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_ids.data_ptr())
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sc.trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_ids.data_ptr())
        ts.append(time.perf_counter() - t0)
    return n / statistics.median(ts) / 1e6


def median_update(sc, fn, reps):
    dev, wall = [], []
    for r in range(reps + 2):
        fn(r)
        t = sc.last_update()
        if r >= 2:
            dev.append(t["device_ms"]); wall.append(t["wall_ms"])
    return {"device_ms": statistics.median(dev), "wall_ms": statistics.median(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=183, help="tessellation (183 = mesh1m)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, _ = g._cornell()
    rng = np.random.default_rng(64)
    amps = (0.02, 0.1, 0.5)
    meshes = {amp: tessellated_cornell(base, a.n, amp) for amp in amps}
    m0 = meshes[0.02]
    ext = float((m0.vertices.max(0) - m0.vertices.min(0)).max())
    M = grid_instances(ext, rng)
    inst = cr.instances_array(M, np.zeros(64))
    out = {"triangles": int(m0.triangles.shape[0]), "vertices": int(m0.vertices.shape[0]), "instances": 64}

    # (a) create, then the two update forms
    creates = []
    for _ in range(3):
        t0 = time.perf_counter()
        s = cr.InstancedScene([m0], inst)
        creates.append((time.perf_counter() - t0) * 1e3)
        s.close()
    out["create_wall_ms"] = statistics.median(creates)
    t0 = time.perf_counter()
    sc = cr.InstancedScene([m0], inst, updatable=True)
    out["create_updatable_wall_ms"] = (time.perf_counter() - t0) * 1e3
    out["state_bytes"] = None
    verts = [meshes[0.1].vertices, m0.vertices]
    out["update_host"] = median_update(sc, lambda r: sc.update_mesh(0, verts[r % 2]), a.reps)
    d_verts = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in verts]
    torch.cuda.synchronize()
    out["update_device"] = median_update(sc, lambda r: sc.update_meshes_device({0: (d_verts[r % 2].data_ptr(), verts[0].shape[0])}), a.reps)
    out["state_bytes"] = sc.last_update()["state_bytes"]
    out["tlas_depth8"] = sc.info()["tlas_depth8"]

    # (c) the trace after an update against a fresh create
    rays = grid_rays(cr, rng, 1 << 21, ext, M)
    out["trace_mrays"] = {}
    for amp in amps:
        sc.update_mesh(0, meshes[amp].vertices)
        fresh = cr.InstancedScene([meshes[amp]], inst)
        out["trace_mrays"][str(amp)] = {"updated": mrays(sc, torch, rays, a.reps), "fresh": mrays(fresh, torch, rays, a.reps)}
        fresh.close()
    sc.close()

    # (b) 256 small meshes in one call against 256 calls
    small = [tessellated_cornell(base, 4, 0.02 + 0.001 * k) for k in range(256)]
    moved = [tessellated_cornell(base, 4, 0.1 + 0.001 * k).vertices for k in range(256)]
    Ms = np.zeros((256, 3, 4), f32)
    Ms[:, :, :3] = np.eye(3, dtype=f32)
    Ms[:, 0, 3] = (np.arange(256) % 16) * 1.5 * ext
    Ms[:, 1, 3] = (np.arange(256) // 16) * 1.5 * ext
    ss = cr.InstancedScene(small, cr.instances_array(Ms, np.arange(256)), updatable=True)
    sets = [{k: moved[k] for k in range(256)}, {k: small[k].vertices for k in range(256)}]
    one, many = [], []
    for r in range(a.reps + 2):
        t0 = time.perf_counter()
        ss.update_meshes(sets[r % 2])
        t1 = time.perf_counter()
        for k in range(256):
            ss.update_mesh(k, sets[(r + 1) % 2][k])
        t2 = time.perf_counter()
        if r >= 2:
            one.append((t1 - t0) * 1e3); many.append((t2 - t1) * 1e3)
    out["small256"] = {"triangles_each": int(small[0].triangles.shape[0]), "one_call_wall_ms": statistics.median(one),
                       "single_calls_wall_ms": statistics.median(many)}
    ss.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
