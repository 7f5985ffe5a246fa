"""crt_bloom on the GPU: prints ONE JSON line.

The 1,004,672-triangle mesh at 1920 x 1080 from the Cornell camera under the 64 x 64 sky of tools/env_probe.py, four frames at depth 3 in
the sum, then render_aov, denoise and temporal so that all three sources exist.  Per arm:

  ms       ms per call: wall time of --calls calls queued back to back with sync = 0 and one synchronise, divided by the calls; median,
           minimum and maximum of --reps such batches after two warm-up batches.  Arms: crt_bloom at levels 1 .. 8 on each source; beside them, from the same session, crt_display (ACES, given exposure) on the sum and on the bloomed image, and one crt_denoise pass.
  floor    the bytes the stage has to move over 8 TB/s, counted from the level sizes: level 0 read and level 1 written; every further level's
           parent read and the level written; on the way up the coarser level read and the level read and written; the composite's two
           reads and one write.  Source sum adds the un-tiling every read of the sum does (a clear, a read and a write of the frame).

There is no pass threshold: the feature is opt-in.

    python tools/bloom_probe.py [--reps 7] [--calls 64]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bloom_probe.py --loop 200
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_MS = 8e12 / 1e3
SOURCES = ("sum", "denoised", "temporal")


def level_sizes(w, h, levels):
    sizes = [(w, h)]
    while len(sizes) <= levels and min(sizes[-1]) >= 2:
        sizes.append(((sizes[-1][0] + 1) >> 1, (sizes[-1][1] + 1) >> 1))
    return sizes


def floor_bytes(w, h, levels, source):
    px = [a * b for a, b in level_sizes(w, h, levels)]
    n = len(px) - 1
    total = 12 * 2 * px[0]                                 # the image read and the result written: the composite, or without a level the copy
    if n > 0:
        total += 12 * px[1]                                # U_1 read by the composite
        total += 12 * sum(px[k - 1] + px[k] for k in range(1, n + 1))                 # down
        total += 12 * sum(px[k + 1] + 2 * px[k] for k in range(1, n))                 # up
    if source == "sum":
        total += 12 * 3 * px[0]
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--loop", type=int, default=0, help="only N default crt_bloom calls on the sum (for a kernel trace)")
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.environment import octahedral_from_function
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    from caitlynrenderer_amd.scene import AOV_ALL
    from display_probe import call_ms
    from env_probe import sky
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    W, H = args.width, args.height
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(4)]
    c_, s_ = np.cos(0.6), np.sin(0.6)
    rotation = np.array([[c_, 0, s_], [0, 1, 0], [-s_, 0, c_]], np.float32)
    scene = cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder="sah"), W, H, 3)
    scene.update(cam)
    scene.set_environment(octahedral_from_function(sky, 64), rotation)
    scene.render_frames(rvs)
    inv = 0.25
    if args.loop:
        for _ in range(args.loop):
            scene.bloom(inv, sync=False)
        scene.sync()
        print(json.dumps({"probe": "bloom_loop", "calls": args.loop}))
        scene.close()
        return
    scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
    scene.denoise(inv)
    scene.temporal(inv)
    out = {"probe": "bloom", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "calls": args.calls, "reps": args.reps}
    ms = lambda call: call_ms(call, scene.sync, args.calls, args.reps)
    out["display_sum_aces_manual_ms"] = ms(lambda: scene.display(inv, curve="aces", exposure=0.5, sync=False))
    out["denoise_one_pass_ms"] = ms(lambda: scene.denoise(inv, passes=1, sync=False))
    out["read_sum_untile_only_floor_ms"] = round(12 * 3 * W * H / HBM_BYTES_PER_MS, 5)
    for source in SOURCES:
        for levels in range(1, 9):
            arm = ms(lambda: scene.bloom(inv, source=source, levels=levels, sync=False))
            arm["floor"] = round(floor_bytes(W, H, levels, source) / HBM_BYTES_PER_MS, 5)
            out[f"{source}_levels_{levels}_ms"] = arm
    out["display_bloom_aces_manual_ms"] = ms(lambda: scene.display(source="bloom", curve="aces", exposure=0.5, sync=False))
    scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
