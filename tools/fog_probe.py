"""Fog with light shafts on the GPU: prints ONE JSON line.

At 1920 x 1080, ms per crt_render_fog call and shadow rays per second at K = 4, 16 and 64 samples, on

  flat     the flat crt_scene of the 1,004,672-triangle mesh from the Cornell camera;
  grid     8 x 8 rotated copies of that mesh (one stored), seen from above the grid, through the instanced path; the mesh carries its
           two lights (crt_scene_create_instanced_lit), so the world table holds 128 that follow the copies;

and beside each case the parent's only path to the same result: crt_trace_device / crt_instances_trace_device (ANY) over the rays of the
same call MATERIALISED in device memory (32 bytes per ray in, 16 per ray out), where they fit into --max-rays.  The materialised rays are
built by torch from the view's HIT channel by the steps of include/crt.h (same segments, same index-based RNG, same light sampler, same
tmax; dark samples are left out, as the fused call traces none for them); torch's sine is not the pinned one, so they are the same rays up
to its last bits, which the hash spreads over [0, 1): the same distribution, not the same words.  Building them is NOT part of the
yardstick's time: it times the walk alone, where the fused call also finds the first hits, builds its segments and its rays and folds them.
One crt_render_aov(HIT) call is timed beside both.  The share of pixels that at least one sample's light reaches is printed from both as a
sanity column, and the unoccluded share of the materialised rays beside it.

k_fog_composite is timed on the denoised image (one kernel: the running sum would add its un-tiling) beside the 40 bytes per pixel it has
to move over 8 TB/s.

Every figure is the min / median / max of --calls (>= 20) synchronous calls by the host clock, after two warm-up calls, the fused call and
the materialised walk taking turns.  "jitter" is 0, so that the segments' seeds are the pixel centres.

--grid-static-lights gives the grid the mesh's two lights as STATIC lights instead (one place, facing away from nearly every sample of this
view): almost every sample is then dark, so the call's time is that of generating the samples with next to no ray walked.

    python tools/fog_probe.py [--calls 20] [--max-rays 140000000] [--samples 4,16,64] [--scenes flat,grid] [--grid-static-lights] [--option NAME=INT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_MS = 8e12 / 1e3
DENSITY, ANISOTROPY = 0.05, 0.6


def spread(ts):
    return {"min": round(float(np.min(ts)), 4), "median": round(float(np.median(ts)), 4), "max": round(float(np.max(ts)), 4)}


def timed(calls, *fns):
    """each of fns() `calls` times in turn (every one ends in a synchronise), two warm-up rounds first: ms per call of each"""
    ts = [[] for _ in fns]
    for k in range(calls + 2):
        for j, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            if k >= 2:
                ts[j].append((time.perf_counter() - t0) * 1e3)
    return [spread(t) for t in ts]


def materialised_rays(torch, cr, sc, cam, lights, W, H, K, max_distance, rv):
    """the shadow rays of crt_render_fog's call as a device tensor of crt_ray records (lit samples only), by the header's steps in torch"""
    sc.render_aov(rv[0], rv[1], channels=cr.AOV_HIT)
    hit = sc.read_aov(cr.AOV_HIT)
    f = torch.float32
    dev = "cuda"
    t = torch.from_numpy(np.where(hit["tri"] >= 0, hit["t"], np.float32(1e9)).astype(np.float32).reshape(-1)).to(dev)
    py, px = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    sx, sy = (px.reshape(-1).to(f) + 0.5), (py.reshape(-1).to(f) + 0.5)
    c = cam.c
    vec = lambda a: torch.tensor([a[0], a[1], a[2]], dtype=f, device=dev)
    tan_fov = float(np.tan(np.float32(c.fov) * np.float32(0.5)))
    dx = (2.0 * (sx / W) - 1.0) * (W / H * tan_fov)
    dy = (2.0 * (sy / H) - 1.0) * tan_fov
    d = dx[:, None] * vec(c.right) + dy[:, None] * vec(c.up) + vec(c.forward)
    d = d / d.norm(dim=1, keepdim=True)
    e = d * torch.clamp(t, max=max_distance)[:, None]
    D = e.norm(dim=1)
    direction = e / D[:, None]
    h = D / K
    o = vec(c.position)
    L = torch.from_numpy(np.ascontiguousarray(lights, np.float32).reshape(-1, 18)).to(dev)
    n_lights = int(L.shape[0])
    r = np.float32(rv[0]) * np.float32(rv[1])

    def rand_at(j):
        s = float(np.float32(j) * r)
        x = (sx - s) * 12.9898 + (sy - s) * 78.233
        v = torch.sin(x.double()).to(f) * 43758.5453
        return v - torch.floor(v)
    parts, pixels = [], []
    for j in range(K):
        u0, r0, r1, r2 = (rand_at(4 * j + i) for i in (1, 2, 3, 4))
        x = o + direction * ((j + u0) * h)[:, None]
        lt = L[torch.clamp((r0 * n_lights).long(), max=n_lights - 1)]
        sq = torch.sqrt(r1)
        pos = lt[:, 0:3] + lt[:, 3:6] * (1.0 - sq)[:, None] + lt[:, 6:9] * (r2 * sq)[:, None]
        ld = pos - x
        ln = ld.norm(dim=1)
        ld = ld / ln[:, None]
        lit = (ld * lt[:, 9:12]).sum(1) < 0
        rays = torch.zeros((int(lit.sum()), 8), dtype=f, device=dev)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7] = x[lit], ln[lit] - 1e-4, ld[lit]
        parts.append(rays)
        pixels.append(torch.nonzero(lit).reshape(-1))
    return torch.cat(parts), torch.cat(pixels)


def measure(torch, cr, sc, inst, cam, lights, W, H, max_distance, calls, max_rays, samples):
    out = {}
    rv = (0.3719, 0.8123)
    sc.set_option("jitter", 0)
    out["aov_hit_ms"] = timed(calls, lambda: sc.render_aov(rv[0], rv[1], channels=cr.AOV_HIT))[0]
    for K in samples:
        case = {}
        fused = lambda: sc.render_fog(rv[0], rv[1], samples=K, density=DENSITY, anisotropy=ANISOTROPY, max_distance=max_distance)
        if W * H * K <= max_rays:
            rays, pixel_of = materialised_rays(torch, cr, sc, cam, lights, W, H, K, max_distance, rv)
            hits = torch.zeros((rays.shape[0], 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            trace = sc.trace_device if inst is None else inst.trace_device
            walk = lambda: trace(rays.data_ptr(), rays.shape[0], hits.data_ptr(), mode=cr.CRT_TRACE_ANY)
            case["fused_ms"], case["materialised_walk_ms"] = timed(calls, fused, walk)
            case["fused_over_materialised"] = round(case["fused_ms"]["median"] / case["materialised_walk_ms"]["median"], 3)
            case["rays"] = int(rays.shape[0])
            unoccluded = hits.view(torch.int32)[:, 3] < 0
            with_light = torch.zeros(W * H, dtype=torch.bool, device="cuda")
            with_light[pixel_of[unoccluded]] = True
            # a pixel of the fused call has S > 0 exactly where one of its samples arrived (no ambient term here)
            fog = sc.read_fog()
            case["lit_rays_share"] = round(float(unoccluded.float().mean()), 4)
            case["pixels_with_light"] = {"materialised": round(float(with_light.float().mean()), 4), "fused": round(float((fog[..., :3].sum(-1) > 0).mean()), 4)}
            del rays, hits, pixel_of
            torch.cuda.empty_cache()
        else:
            case["fused_ms"] = timed(calls, fused)[0]
            case["materialised_walk_ms"] = None          # the rays do not fit into --max-rays
            case["rays"] = None
        case["samples"] = W * H * K
        case["fused_gsamples_per_s"] = round(case["samples"] / case["fused_ms"]["median"] / 1e6, 3)
        if case["rays"]:
            case["fused_grays_per_s"] = round(case["rays"] / case["fused_ms"]["median"] / 1e6, 3)
        out[f"K{K}"] = case
    # the composite alone: one kernel over the denoised image
    sc.render_frame(*rv)
    sc.render_aov(rv[0], rv[1])
    sc.denoise(1.0, passes=1)
    out["composite_ms"] = timed(calls, lambda: sc.fog_composite(1.0, source="denoised"))[0]
    out["composite_floor_ms"] = round(40 * W * H / HBM_BYTES_PER_MS, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max-rays", type=int, default=140_000_000, help="materialise the rays of a case up to this many (32 + 16 bytes each, and torch's temporaries)")
    ap.add_argument("--samples", default="4,16,64", help="the sample counts to run")
    ap.add_argument("--scenes", default="flat,grid", help="a subset of the cases, e.g. for a profiler run of one of them")
    ap.add_argument("--grid-static-lights", action="store_true", help="the grid's lights as static lights of the scene, not as lights of the mesh: nearly every sample dark")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=INT", help="crt_set_option passthrough (e.g. shadow_refill_min=32: the flat walk's refill threshold)")
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    assert args.calls >= 20, "at least 20 timed calls"
    import torch
    assert torch.cuda.is_available(), "fog_probe measures on a GPU"
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = args.width, args.height
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    ext = float((hi - lo).max())
    samples, scenes = [int(k) for k in args.samples.split(",")], args.scenes.split(",")
    out = {"probe": "fog", "options": args.option, "triangles": int(mesh.triangles.shape[0]), "lights": int(np.asarray(mesh.lights).reshape(-1, 18).shape[0]),
           "grid_static_lights": bool(args.grid_static_lights), "width": W, "height": H, "calls": args.calls, "max_rays": args.max_rays, "density": DENSITY, "anisotropy": ANISOTROPY}
    if "flat" in scenes:
        flat = cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder="sah"), W, H, 1)
        flat.update(cam)
        for o in args.option:
            flat.set_option(o.split("=")[0], int(o.split("=")[1]))
        out["flat"] = measure(torch, cr, flat, None, cam, mesh.lights, W, H, 3.0 * ext, args.calls, args.max_rays, samples)
        flat.close()
    if "grid" not in scenes:
        print(json.dumps(out))
        return
    # the 8 x 8 grid of tools/instance_frame_probe.py
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
    if args.grid_static_lights:
        sc = grid.frame_scene([(mesh.triangles, mesh.normals, mesh.texcoords)], mesh.materials, mesh.lights, W, H, 1)
    else:
        sc = grid.frame_scene([(mesh.triangles, mesh.normals, mesh.texcoords)], mesh.materials, np.zeros((0, 18), np.float32), W, H, 1,
                              mesh_lights=[mesh.lights])
    cam_above = type("Cam", (), {"c": above})()
    sc.update(cam_above)
    for o in args.option:
        sc.set_option(o.split("=")[0], int(o.split("=")[1]))
    out["grid"] = measure(torch, cr, sc, grid, cam_above, cr.read_lights(sc), W, H, 8.0 * ext, args.calls, args.max_rays, samples)
    sc.close(); grid.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
