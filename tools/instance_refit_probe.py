"""Measurement, not a test: what crt_instances_refit costs against crt_instances_set, and what the refitted TLAS costs the trace as the
instances move away from the placement it was built for.

Prints one JSON line:
  (a) device / wall ms of a set, of a host-form refit and of a device-form refit at 1 k / 16 k / 256 k instances of the 1,922-triangle mesh
      (§11's scene: random rotations, translations in [-200, 200]^3; each call alternates between two placements 0.5 apart, medians of
      --reps calls after two warm-ups), and the wall ms of the first refit after a set, which finds the TLAS's levels;
  (b) closest-hit Mray/s on the mesh1m 8 x 8 grid (2 M rays aimed at the grid, medians of synchronous crt_instances_trace_device calls
      after two warm-ups) after 1 and 20 frames of small motion (each frame moves every instance by 1 % of the mesh size) and after a full
      reshuffle of the placements, each against a fresh set of the same placement.

    python tools/instance_refit_probe.py [--reps 10] [--out instance_refit_probe.json]
    python tools/instance_refit_probe.py --only-refit 16384 [--reps 50]     # refits only, for a kernel trace of one refit's launches
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


def scattered(rng, count):
    q = np.linalg.qr(rng.normal(size=(count, 3, 3)))[0]
    t = rng.uniform(-200, 200, (count, 3, 1))
    return np.concatenate([q, t], 2).astype(f32)


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
    return round(n / statistics.median(ts) / 1e6, 1)


def median_calls(sc, fn, reps):
    """fn(r) for r < reps + 2; medians of set_device_ms / set_wall_ms over the last reps calls"""
    dev, wall = [], []
    for r in range(reps + 2):
        fn(r)
        i = sc.info()
        if r >= 2:
            dev.append(i["set_device_ms"]); wall.append(i["set_wall_ms"])
    return {"device_ms": round(statistics.median(dev), 3), "wall_ms": round(statistics.median(wall), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-refit", type=int, default=0, help="only refits of this many instances (for rocprofv3 --kernel-trace)")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, _ = g._cornell()
    rng = np.random.default_rng(13)
    small = tessellated_cornell(base, 8)
    out = {"mesh_triangles": int(small.triangles.shape[0])}

    if a.only_refit:
        M = scattered(rng, a.only_refit)
        two = [cr.instances_array(M, np.zeros(a.only_refit)), cr.instances_array(M + f32(0.5), np.zeros(a.only_refit))]
        sc = cr.InstancedScene([small], two[0])
        out["only_refit"] = a.only_refit
        out["refit"] = median_calls(sc, lambda r: sc.refit(two[r % 2]), a.reps)
        sc.close()
        print(json.dumps(out))
        return

    # (a) set against refit
    for count in (1024, 16384, 262144):
        M = scattered(rng, count)
        two = [cr.instances_array(M, np.zeros(count)), cr.instances_array(M + f32(0.5), np.zeros(count))]
        d_two = [torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in two]
        torch.cuda.synchronize()
        sc = cr.InstancedScene([small], two[0])
        r = {"set": median_calls(sc, lambda k: sc.set(two[k % 2]), a.reps)}
        sc.set(two[0])
        t0 = time.perf_counter()
        sc.refit(two[1])
        r["first_refit_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        r["refit"] = median_calls(sc, lambda k: sc.refit(two[k % 2]), a.reps)
        r["refit_device"] = median_calls(sc, lambda k: sc.refit_device(d_two[k % 2].data_ptr(), count), a.reps)
        i = sc.info()
        r["tlas_nodes8"] = int(i["tlas_nodes8"]); r["tlas_depth8"] = int(i["tlas_depth8"])
        out[f"a_{count}"] = r
        sc.close()

    # (b) the trace as the instances move
    mesh = tessellated_cornell(base, 183)
    ext = float((mesh.vertices.max(0) - mesh.vertices.min(0)).max())
    M = grid_instances(ext, rng)
    rays = grid_rays(cr, rng, 1 << 21, ext, M)
    sc = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(64)))
    out["b_triangles"] = int(mesh.triangles.shape[0])
    out["b_built"] = mrays(sc, torch, rays, a.reps)
    fresh = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(64)))
    b = {}
    for frame in range(1, 21):
        M[:, :, 3] += rng.normal(scale=0.01 * ext, size=(64, 3)).astype(f32)
        sc.refit(cr.instances_array(M, np.zeros(64)))
        if frame in (1, 20):
            fresh.set(cr.instances_array(M, np.zeros(64)))
            b[f"frames_{frame}"] = {"refit": mrays(sc, torch, rays, a.reps), "fresh_set": mrays(fresh, torch, rays, a.reps)}
    M = M[rng.permutation(64)]
    sc.refit(cr.instances_array(M, np.zeros(64)))
    fresh.set(cr.instances_array(M, np.zeros(64)))
    b["reshuffle"] = {"refit": mrays(sc, torch, rays, a.reps), "fresh_set": mrays(fresh, torch, rays, a.reps)}
    out["b_mrays"] = b
    sc.close(); fresh.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
