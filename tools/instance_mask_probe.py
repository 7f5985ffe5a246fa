"""Measurement, not a test: what instance visibility masks cost and save (CRT_TRACE_INSTANCE_MASK).

Prints one JSON line.  Scenes: the mesh1m 8 x 8 grid of tools/instance_probe.py (64 rotated copies of the 1,004,672-triangle mesh, 2 M
camera-like rays from above the grid) and the 1,922-triangle mesh at 1 k / 16 k / 256 k instances (random rotations, translations in
[-200, 200]^3; 2 M rays, half aimed at instances).  Mray/s are medians of --reps synchronous crt_instances_trace_device calls after two
warm-ups, on device-resident rays.
  (a) the masked trace with every instance and ray mask 0xff against the unmasked trace, closest and any: the cost of the mode;
  (b) half of the instances hidden, as one contiguous half (grid: columns 0..3; scattered: x < 0) and interleaved (grid: a checkerboard;
      scattered: odd instance indices): the masked closest trace against an unmasked closest trace of a handle set to the visible half;
  (c) scattered scenes: the wall ms of a 1-ray masked trace right after a refit (the child-mask pass runs first) minus that of one
      without, and a refit that only toggles masks against a set of the same array (the handle's device / wall ms, medians).

    python tools/instance_mask_probe.py [--reps 10] [--out instance_mask_probe.json]
    python tools/instance_mask_probe.py --only-cmask 16384 [--reps 50]    # refit + child-mask pass only, for rocprofv3 --kernel-trace
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


def camera_rays(cr, cam, n, origin_shift):
    w = int(np.sqrt(n * 16 / 9))
    h = n // w
    c = cam.c
    pos, right, up, fwd = (np.array(getattr(c, k)[:], f32) for k in ("position", "right", "up", "forward"))
    tan = f32(np.tan(c.fov / 2))
    ys, xs = np.mgrid[0:h, 0:w]
    sx = ((xs + 0.5) / w * 2 - 1) * tan * w / h
    sy = ((ys + 0.5) / h * 2 - 1) * tan
    d = fwd[None, None] + sx[..., None] * right[None, None] + sy[..., None] * up[None, None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    rays = np.zeros(d.shape[0], cr.RAY_DT)
    rays["o"] = pos + origin_shift
    rays["d"] = d.astype(f32)
    rays["tmax"] = f32(1e9)
    return rays


def scattered(rng, count):
    q = np.linalg.qr(rng.normal(size=(count, 3, 3)))[0]
    t = rng.uniform(-200, 200, (count, 3, 1))
    return np.concatenate([q, t], 2).astype(f32)


def aimed_rays(cr, rng, n, M, spread):
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"] = rng.uniform(-spread, spread, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3))
    k = n // 2
    d[:k] = M[rng.integers(0, len(M), k), :, 3] + rng.normal(scale=2.0, size=(k, 3)) - rays["o"][:k]
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmax"] = f32(1e9)
    return rays


class Bufs:
    def __init__(self, torch, cr, rays):
        r = rays.copy()
        r["pad"] = 0xff
        self.n = r.shape[0]
        self.rays = torch.from_numpy(r.view(np.uint8).copy()).cuda()
        self.hits = torch.empty(self.n * 16, dtype=torch.uint8, device="cuda")
        self.ids = torch.empty(self.n, dtype=torch.int32, device="cuda")
        one = r[:1].copy()
        self.one = torch.from_numpy(one.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()

    def mrays(self, sc, mode, reps):
        call = lambda: sc.trace_device(self.rays.data_ptr(), self.n, self.hits.data_ptr(), self.ids.data_ptr(), mode)
        call(); call()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return round(self.n / statistics.median(ts) / 1e6, 1)

    def one_ray_ms(self, sc, mode):
        t0 = time.perf_counter()
        sc.trace_device(self.one.data_ptr(), 1, self.hits.data_ptr(), self.ids.data_ptr(), mode)
        return (time.perf_counter() - t0) * 1e3


def median_calls(sc, fn, reps):
    dev, wall = [], []
    for r in range(reps + 2):
        fn(r)
        i = sc.info()
        if r >= 2:
            dev.append(i["set_device_ms"]); wall.append(i["set_wall_ms"])
    return {"device_ms": round(statistics.median(dev), 3), "wall_ms": round(statistics.median(wall), 3)}


def measure(cr, torch, meshes, M, mesh_of, rays, halves, reps, with_c):
    """(a), (b) and, with_c, (c) for one scene; halves: {name: bool array of the visible instances}"""
    CL, ANY, MK = cr.CRT_TRACE_CLOSEST, cr.CRT_TRACE_ANY, cr.CRT_TRACE_INSTANCE_MASK
    n = M.shape[0]
    b = Bufs(torch, cr, rays)
    full = cr.instances_array(M, mesh_of, np.full(n, 0xff))
    sc = cr.InstancedScene(meshes, full)
    info = sc.info()
    out = {"instances": n, "tlas_nodes8": int(info["tlas_nodes8"]), "tlas_depth8": int(info["tlas_depth8"])}
    out["a"] = {"closest": {"unmasked": b.mrays(sc, CL, reps), "masked_ff": b.mrays(sc, CL | MK, reps)},
                "any": {"unmasked": b.mrays(sc, ANY, reps), "masked_ff": b.mrays(sc, ANY | MK, reps)}}
    sub = cr.InstancedScene(meshes, full, capacity=n)
    out["b"] = {}
    for name, vis in halves.items():
        masks = np.where(vis, 0x01, 0x02)             # visible half: bit 0, hidden half: bit 1; the rays carry mask 1
        inst = cr.instances_array(M, mesh_of, masks)
        sc.set(inst)
        r = b.rays.clone()
        r.view(-1, 32)[:, 28] = 0x01                  # ray mask 1 in the low byte of pad
        saved, b.rays = b.rays, r
        masked = b.mrays(sc, CL | MK, reps)
        b.rays = saved
        sub.set(cr.instances_array(M[vis], mesh_of[vis]))
        out["b"][name] = {"masked": masked, "subset_handle": b.mrays(sub, CL, reps), "visible": int(vis.sum())}
    sub.close()
    if with_c:
        sc.set(full)
        b.one_ray_ms(sc, CL | MK)
        stale, warm = [], []
        for _ in range(reps + 2):
            sc.refit(full)
            stale.append(b.one_ray_ms(sc, CL | MK))
            warm.append(b.one_ray_ms(sc, CL | MK))
        out["c_child_mask_pass_wall_ms"] = round(statistics.median(stale[2:]) - statistics.median(warm[2:]), 4)
        out["c_one_ray_masked_wall_ms"] = round(statistics.median(warm[2:]), 4)
        two = [cr.instances_array(M, mesh_of, np.where(halves[k], 1, 2)) for k in halves]
        out["c_set"] = median_calls(sc, lambda r: sc.set(two[r % 2]), reps)
        out["c_toggle_refit"] = median_calls(sc, lambda r: sc.refit(two[r % 2]), reps)
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-cmask", type=int, default=0, help="only refits followed by a 1-ray masked trace (for rocprofv3 --kernel-trace)")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    rng = np.random.default_rng(17)
    small = tessellated_cornell(base, 8)

    if a.only_cmask:
        M = scattered(rng, a.only_cmask)
        inst = cr.instances_array(M, np.zeros(a.only_cmask), np.full(a.only_cmask, 0xff))
        sc = cr.InstancedScene([small], inst)
        b = Bufs(torch, cr, aimed_rays(cr, rng, 1, M, 220.0))
        for _ in range(a.reps):
            sc.refit(inst)
            b.one_ray_ms(sc, cr.CRT_TRACE_CLOSEST | cr.CRT_TRACE_INSTANCE_MASK)
        sc.close()
        print(json.dumps({"only_cmask": a.only_cmask, "reps": a.reps}))
        return

    out = {"probe": "instance_mask", "rays": a.rays, "reps": a.reps}
    # the grid
    mesh = tessellated_cornell(base, 183)
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    ext = float((hi - lo).max())
    M, gx, gy = [], [], []
    for x in range(8):
        for y in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[x * 1.5 * ext], [y * 1.5 * ext], [0.0]])], 1))
            gx.append(x); gy.append(y)
    M, gx, gy = np.array(M, f32), np.array(gx), np.array(gy)
    centre = np.array([5.25 * ext, 5.25 * ext, 0.0], f32)
    rays = camera_rays(cr, cam, a.rays, centre + np.array([0, 0, 6 * ext], f32) - np.array(cam.c.position[:], f32))
    out["grid_triangles"] = int(mesh.triangles.shape[0])
    out["grid"] = measure(cr, torch, [mesh], M, np.zeros(64), rays, {"contiguous": gx < 4, "checkerboard": (gx + gy) % 2 == 0}, a.reps, False)
    # the 1,922-triangle mesh, scattered
    out["small_triangles"] = int(small.triangles.shape[0])
    for count in (1024, 16384, 262144):
        M = scattered(rng, count)
        rays = aimed_rays(cr, rng, a.rays, M, 220.0)
        halves = {"contiguous": M[:, 0, 3] < 0, "interleaved": np.arange(count) % 2 == 1}
        out[f"small_{count}"] = measure(cr, torch, [small], M, np.zeros(count), rays, halves, a.reps, True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
