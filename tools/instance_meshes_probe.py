"""Measurement, not a test: what crt_instances_add_meshes and crt_instances_replace_meshes cost beside the re-create they replace
(DESIGN.md §15).

Prints one JSON line.  The handle is updatable and holds mesh1m (1,004,672 triangles) under 64 instances; medians after two warm-ups:
  (a) adding a 1,922-triangle mesh (each repetition adds one more: the handle grows by 1,922 triangles per call);
  (b) replacing that small mesh, alternately by a displaced copy and by itself;
  (c) replacing mesh1m with itself;
each as wall and device ms (crt_instances_info set_wall_ms / set_device_ms), beside create_wall_ms of fresh creates of the final handle
[mesh1m, small] (what a caller pays without these calls) and of single-mesh handles [small] and [mesh1m] (the floor: one BLAS build),
plain and updatable.  Also closest-hit Mray/s before and after the first add: the same trace of the same arrays.

    python tools/instance_meshes_probe.py [--n 183] [--reps 10] [--creates-only] [--only add_small] [--out instance_meshes_probe.json]

--creates-only measures the creates alone (it uses nothing newer than crt_instances_create, so it runs on an older checkout too).
--only add_small | replace_small | replace_big runs that one series alone, for a kernel trace of its own (rocprofv3 --kernel-trace --stats).
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


def median_create(cr, meshes, inst, updatable, reps):
    ms = []
    for r in range(reps + 2):
        s = cr.InstancedScene(meshes, inst, updatable=updatable)
        if r >= 2:
            ms.append(s.info()["create_wall_ms"])
        s.close()
    return statistics.median(ms)


def median_call(sc, fn, reps):
    dev, wall = [], []
    for r in range(reps + 2):
        fn(r)
        i = sc.info()
        if r >= 2:
            dev.append(i["set_device_ms"]); wall.append(i["set_wall_ms"])
    return {"device_ms": statistics.median(dev), "wall_ms": statistics.median(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=183, help="tessellation (183 = mesh1m)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--creates-only", action="store_true")
    ap.add_argument("--only", default=None, choices=("add_small", "replace_small", "replace_big"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, _ = g._cornell()
    rng = np.random.default_rng(64)
    big = tessellated_cornell(base, a.n, 0.02)
    small = tessellated_cornell(base, 8, 0.02)
    small2 = tessellated_cornell(base, 8, 0.1)
    ext = float((big.vertices.max(0) - big.vertices.min(0)).max())
    M = grid_instances(ext, rng)
    inst = cr.instances_array(M, np.zeros(64))
    one = cr.instances_array(M[:1], np.zeros(1))
    out = {"triangles": int(big.triangles.shape[0]), "small_triangles": int(small.triangles.shape[0]), "instances": 64, "reps": a.reps}

    out["create_wall_ms"] = {}
    for name, meshes, ins in () if a.only else (("final", [big, small], inst), ("small_alone", [small], one), ("big_alone", [big], inst)):
        out["create_wall_ms"][name] = {"plain": median_create(cr, meshes, ins, False, a.reps),
                                       "updatable": median_create(cr, meshes, ins, True, a.reps)}
    if a.only:
        sc = cr.InstancedScene([big] if a.only == "add_small" else [big, small], inst, updatable=True)
        fn = {"add_small": lambda r: sc.add_meshes([small]), "replace_small": lambda r: sc.replace_meshes({1: (small2, small)[r % 2]}),
              "replace_big": lambda r: sc.replace_meshes({0: big})}[a.only]
        out[a.only] = median_call(sc, fn, a.reps)
        sc.close()
    elif not a.creates_only:
        sc = cr.InstancedScene([big], inst, updatable=True)
        rays = grid_rays(cr, rng, 1 << 21, ext, M)
        out["trace_mrays"] = {"before_add": mrays(sc, torch, rays, a.reps)}
        sc.add_meshes([small])
        out["trace_mrays"]["after_add"] = mrays(sc, torch, rays, a.reps)
        sc.close()
        sc = cr.InstancedScene([big], inst, updatable=True)
        out["add_small"] = median_call(sc, lambda r: sc.add_meshes([small]), a.reps)
        sc.close()
        sc = cr.InstancedScene([big, small], inst, updatable=True)
        out["replace_small"] = median_call(sc, lambda r: sc.replace_meshes({1: (small2, small)[r % 2]}), a.reps)
        out["replace_big"] = median_call(sc, lambda r: sc.replace_meshes({0: big}), a.reps)
        sc.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
