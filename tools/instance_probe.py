"""Instanced scenes on the GPU: prints ONE JSON line.

  (a) Mray/s of crt_trace on the flat 1,004,672-triangle scene against ONE identity instance of the same mesh, on the same 2 M camera-like
      rays (a pinhole grid from the Cornell camera) and the same 2 M random rays (origins in the mesh box, uniform directions);
  (b) Mray/s and device bytes (tlas_build_bytes: what the sets keep reserved) of 8 x 8 rotated copies of that mesh (64 M triangles seen, one stored), the same two ray kinds aimed at the grid;
  (c) device and wall ms of crt_instances_set at 1 k / 16 k / 256 k instances of the 1,922-triangle mesh.

Every figure is the median of --reps timed calls after two warm-up calls.  A timed trace is one synchronous *_trace_device call on
device-resident rays (wall time around the call: the launch and the final stream synchronise are included, ~20 us).

    python tools/instance_probe.py [--reps 10] [--rays 2000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn(); fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def camera_rays(cr, cam, n, origin_shift=None):
    w = int(np.sqrt(n * 16 / 9))
    h = n // w
    c = cam.c
    pos, right, up, fwd = (np.array(getattr(c, k)[:], np.float32) for k in ("position", "right", "up", "forward"))
    tan = np.float32(np.tan(c.fov / 2))
    ys, xs = np.mgrid[0:h, 0:w]
    sx = ((xs + 0.5) / w * 2 - 1) * tan * w / h
    sy = ((ys + 0.5) / h * 2 - 1) * tan
    d = fwd[None, None] + sx[..., None] * right[None, None] + sy[..., None] * up[None, None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    rays = np.zeros(d.shape[0], cr.RAY_DT)
    rays["o"] = pos if origin_shift is None else pos + origin_shift
    rays["d"] = d.astype(np.float32)
    rays["tmax"] = np.float32(1e9)
    return rays


def random_rays(cr, lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"] = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["tmax"] = np.float32(1e9)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=2_000_000)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, 183)
    out = {"probe": "instances", "triangles": int(mesh.triangles.shape[0]), "rays": args.rays, "reps": args.reps}

    def dev(rays):
        return torch.from_numpy(rays.view(np.uint8).copy()).cuda()

    n = args.rays
    hits = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    kinds = {"camera": camera_rays(cr, cam, n), "random": random_rays(cr, lo, hi, n, 1)}
    # (a) flat against one identity instance
    flat = cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder="sah"), 16, 16, 1)
    one = cr.InstancedScene([mesh], cr.instances_array([np.eye(3, 4, dtype=np.float32)], [0]))
    for kind, rays in kinds.items():
        m = rays.shape[0]
        d = dev(rays)
        for mode, name in ((cr.CRT_TRACE_CLOSEST, "closest"), (cr.CRT_TRACE_ANY, "any")):
            ms_f = median_ms(lambda: flat.trace_device(d.data_ptr(), m, hits.data_ptr(), mode, None, True), args.reps)
            ms_i = median_ms(lambda: one.trace_device(d.data_ptr(), m, hits.data_ptr(), ids.data_ptr(), mode, None, True), args.reps)
            out[f"a_{kind}_{name}_flat_mrays"] = round(m / ms_f / 1e3, 1)
            out[f"a_{kind}_{name}_instance_mrays"] = round(m / ms_i / 1e3, 1)
    one_info = one.info()
    one.close(); flat.close()
    # (b) 8 x 8 rotated copies on a grid
    rng = np.random.default_rng(8)
    ext = float((hi - lo).max())
    M = []
    for gx in range(8):
        for gy in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
    grid = cr.InstancedScene([mesh], cr.instances_array(np.array(M, np.float32), np.zeros(64)))
    centre = np.array([5.25 * ext, 5.25 * ext, 0.0], np.float32)
    gk = {"camera": camera_rays(cr, cam, n, origin_shift=centre + np.array([0, 0, 6 * ext], np.float32) - np.array(cam.c.position[:], np.float32)),
          "random": random_rays(cr, centre - 6 * ext, centre + 6 * ext, n, 2)}
    for kind, rays in gk.items():
        m = rays.shape[0]
        d = dev(rays)
        ms = median_ms(lambda: grid.trace_device(d.data_ptr(), m, hits.data_ptr(), ids.data_ptr(), cr.CRT_TRACE_CLOSEST, None, True), args.reps)
        out[f"b_{kind}_closest_mrays"] = round(m / ms / 1e3, 1)
        out[f"b_{kind}_hit_fraction"] = round(float((ids.cpu().numpy()[:m] >= 0).mean()), 3)
    info = grid.info()
    out["b_blas_bytes"] = int(info["blas_bytes"]); out["b_tlas_bytes"] = int(info["tlas_bytes"]); out["b_instance_bytes"] = int(info["instance_bytes"])
    out["b_tlas_build_bytes"] = int(info["tlas_build_bytes"])
    out["b_stack_entries"] = int(info["stack_entries"]); out["one_stack_entries"] = int(one_info["stack_entries"])
    grid.close()
    # (c) sets
    small = tessellated_cornell(base, 8)
    for count in (1024, 16384, 262144):
        q = np.linalg.qr(rng.normal(size=(count, 3, 3)))[0]
        t = rng.uniform(-200, 200, (count, 3, 1))
        inst = cr.instances_array(np.concatenate([q, t], 2).astype(np.float32), np.zeros(count))
        sc = cr.InstancedScene([small], inst)
        dms, wms = [], []
        for r in range(args.reps + 2):
            sc.set(inst)
            i = sc.info()
            if r >= 2:
                dms.append(i["set_device_ms"]); wms.append(i["set_wall_ms"])
        out[f"c_set_{count}_device_ms"] = round(float(np.median(dms)), 3)
        out[f"c_set_{count}_wall_ms"] = round(float(np.median(wms)), 3)
        out[f"c_set_{count}_stack_entries"] = int(sc.info()["stack_entries"])
        out[f"c_set_{count}_tlas_build_bytes"] = int(sc.info()["tlas_build_bytes"])
        sc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
