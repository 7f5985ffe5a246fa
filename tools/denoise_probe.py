"""crt_denoise on the GPU: prints ONE JSON line.

At 1920 x 1080, per scene: 4 samples, render_aov, then ms per crt_denoise call at passes 1..6 (wall time of --calls calls queued back to
back and one synchronise, divided by the calls; median, minimum and maximum of --reps such batches after two warm-up batches), of

  flat     the flat crt_scene of the 1,004,672-triangle mesh from the Cornell camera;
  grid     8 x 8 rotated copies of that mesh (one stored), seen from above the grid, through the instanced path;

and in the same session crt_resolve_device, crt_resolve_denoised_device and one max_depth 1 frame, measured the same way.  The passes are
measured three times in that session, in one process: as the product runs them (option "denoise_form" 0: each pass in the form measured
faster at its tap spacing), with the taps staged in LDS at every spacing (1) and with the taps read from global memory at every spacing
(2).  A pass's cost is the difference between k and k - 1 passes (which also turns pass k - 1 from the kernel that writes the image into
the one that writes the next pass's input); its floor is 32 bytes read and 16 written per pixel at 8 TB/s (100 MB, 12.4 us at 1080p), and
the share of that floor each pass reaches is printed.

    python tools/denoise_probe.py [--reps 5] [--calls 16] [--png DIR]

--png DIR writes the noisy and the denoised resolve of both scenes as PNG files.
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


def measure(cr, sc, rvs, reps, calls):
    from aov_probe import batch_ms
    sc.render_frames(rvs[:4])
    sc.render_aov(*rvs[0])
    W, H = sc.width, sc.height
    floor_ms = (32 + 16) * W * H / HBM_BYTES_PER_S * 1e3
    out = {"pass_floor_ms": round(floor_ms, 5)}
    for form, label in ((0, "product"), (1, "staged"), (2, "direct")):
        sc.set_option("denoise_form", form)
        res, prev = {}, None
        for passes in range(1, 7):
            t = batch_ms(lambda i: sc.denoise(0.25, passes=passes, sync=False), sc.sync, calls, reps)
            res[f"denoise_{passes}_ms"] = t
            if prev is not None:
                step = t["median"] - prev
                res[f"pass_{passes - 1}_ms"] = round(step, 4)                   # pass index from 0: tap spacing 2^(passes - 1)
                res[f"pass_{passes - 1}_share_of_floor"] = round(floor_ms / step, 3) if step > 0 else None
            prev = t["median"]
        out[label] = res
    sc.set_option("denoise_form", 0)
    out["resolve_device_ms"] = batch_ms(lambda i: sc.resolve_device(0.25, sync=False), sc.sync, calls, reps)
    out["resolve_denoised_device_ms"] = batch_ms(lambda i: sc.resolve_denoised_device(sync=False), sc.sync, calls, reps)
    sc.set_option("jitter", 1)
    out["frame_d1_ms"] = batch_ms(lambda i: sc.render_frame(rvs[i][0], rvs[i][1], sync=False), sc.sync, calls, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--png", default=None, help="directory for the noisy and the denoised resolve")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd.image import write_png
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = args.width, args.height
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(max(args.calls, 4))]
    out = {"probe": "denoise", "library": os.path.relpath(_lib.LIB_PATH, ROOT), "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H,
           "calls": args.calls, "reps": args.reps}
    if args.png:
        os.makedirs(args.png, exist_ok=True)

    def pictures(name, sc):
        if args.png:
            sc.reset()
            sc.render_frames(rvs[:4])
            sc.render_aov(*rvs[0])
            sc.denoise(0.25)
            write_png(os.path.join(args.png, f"{name}_noisy.png"), sc.resolve(0.25))
            write_png(os.path.join(args.png, f"{name}_denoised.png"), sc.resolve_denoised())

    flat = cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder="sah"), W, H, 1)
    flat.update(cam)
    out["flat"] = measure(cr, flat, rvs, args.reps, args.calls)
    pictures("flat", flat)
    flat.close()
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
    pictures("grid", sc)
    sc.close(); grid.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
