"""crt_temporal on the GPU: prints a table and ONE JSON line.

At 1920 x 1080, per scene: 4 samples, render_aov, denoise, then ms per crt_temporal call (wall time of --calls calls queued back to back
and one synchronise, divided by the calls; median, minimum and maximum of --reps such batches after two warm-up batches) of

  flat     the flat crt_scene of the 1,004,672-triangle mesh from the Cornell camera;
  grid     8 x 8 rotated copies of that mesh (one stored), seen from above the grid, through the instanced path;

for each flag combination {0, DEMODULATE, CLAMP, both}, both sources (the sum, which the call first un-tiles, and crt_denoise's image) and,
with CLAMP, both forms of the neighbourhood (option "temporal_form" 1 = staged in LDS, 2 = read from global memory); in the same session
crt_denoise, crt_resolve_device, crt_resolve_temporal_device and one max_depth 1 frame, measured the same way.  The view is static, so
every call after a batch's first is one with history on every filterable pixel (the full gather), and the grid's transforms compare
equal (no matrix products).  Beside each time, the share of its bandwidth floor the call reaches: the bytes the definition must move per
pixel (144, and 16 more for ALBEDO with DEMODULATE; source SUM adds the un-tiling's 36) at 8 TB/s.

    python tools/temporal_probe.py [--reps 5] [--calls 16]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8.0e12
# per pixel: source 12, HIT 16, IDS 16, NORMAL 16; the previous (hist 16, guide 16, key 4), each pixel of which is gathered once on average;
# written: hist 16, guide 16, key 4, image 12
KERNEL_BYTES = 12 + 16 + 16 + 16 + 36 + 48
ALBEDO_BYTES = 16
UNTILE_BYTES = 36                                             # source SUM: the linear sum is cleared (12 written), then un-tiled into (12 read, 12 written)


def floor_ms(W, H, demodulate, source):
    b = KERNEL_BYTES + (ALBEDO_BYTES if demodulate else 0) + (UNTILE_BYTES if source == "sum" else 0)
    return b * W * H / HBM_BYTES_PER_S * 1e3


def measure(cr, sc, rvs, reps, calls):
    from aov_probe import batch_ms
    sc.render_frames(rvs[:4])
    sc.render_aov(*rvs[0])
    sc.denoise(0.25)
    W, H = sc.width, sc.height
    out = {}
    for source in ("sum", "denoised"):
        for flags in (0, 1, 2, 3):
            for form in ((1, 2) if flags & 2 else (0,)):
                sc.set_option("temporal_form", form)
                sc.temporal_reset()
                t = batch_ms(lambda i: sc.temporal(0.25, source=source, demodulate=bool(flags & 1), clamp=bool(flags & 2), sync=False), sc.sync, calls, reps)
                fl = floor_ms(W, H, flags & 1, source)
                t["floor_ms"], t["share_of_floor"] = round(fl, 5), round(fl / t["median"], 3)
                out[f"temporal_{source}_flags{flags}" + ("" if not form else "_staged" if form == 1 else "_direct")] = t
    sc.set_option("temporal_form", 0)
    n = sc.read_temporal_history()
    out["pixels_with_history"] = int((n > 1).sum())
    out["denoise_ms"] = batch_ms(lambda i: sc.denoise(0.25, sync=False), sc.sync, calls, reps)
    out["resolve_device_ms"] = batch_ms(lambda i: sc.resolve_device(0.25, sync=False), sc.sync, calls, reps)
    out["resolve_temporal_device_ms"] = batch_ms(lambda i: sc.resolve_temporal_device(sync=False), sc.sync, calls, reps)
    sc.set_option("jitter", 1)
    out["frame_d1_ms"] = batch_ms(lambda i: sc.render_frame(rvs[i][0], rvs[i][1], sync=False), sc.sync, calls, reps)
    return out


def table(title, res):
    print(title)
    print(f"{'call':44s} {'ms per call, median (min - max)':32s} floor ms   share of the floor")
    for k, v in res.items():
        if not isinstance(v, dict):
            print(f"{k:44s} {v}")
            continue
        line = f"{k:44s} {v['median']:.4f} ({v['min']:.4f} - {v['max']:.4f})".ljust(78)
        if "floor_ms" in v:
            line += f"{v['floor_ms']:.5f}    {v['share_of_floor']:.3f}"
        print(line)
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = args.width, args.height
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(max(args.calls, 4))]
    out = {"probe": "temporal", "library": os.path.relpath(_lib.LIB_PATH, ROOT), "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H,
           "calls": args.calls, "reps": args.reps}
    flat = cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder="sah"), W, H, 1)
    flat.update(cam)
    out["flat"] = measure(cr, flat, rvs, args.reps, args.calls)
    flat.close()
    table(f"flat scene ({out['triangles']:,} triangles, Cornell camera), {W} x {H}", out["flat"])
    # the 8 x 8 grid of tools/aov_probe.py
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
    out["grid"] = measure(cr, sc, rvs, args.reps, args.calls)
    sc.close(); grid.close()
    table(f"8 x 8 instanced grid of that mesh, from above, {W} x {H}", out["grid"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
