"""crt_display on the GPU: prints ONE JSON line.

The 1,004,672-triangle mesh at 1920 x 1080 from the Cornell camera under the 64 x 64 sky of tools/env_probe.py, four frames at depth 3 in
the sum, then render_aov, denoise and temporal so that all three sources exist.  Per arm:

  ms       ms per call: wall time of --calls calls queued back to back with sync = 0 and one synchronise, divided by the calls; median,
           minimum and maximum of --reps such batches after two warm-up batches.  Arms: crt_resolve_device on the same sum; crt_display
           with a given exposure and with the metered one, for each curve on the sum and for ACES on the denoised and the accumulated image.

A call with a given exposure is two launches (the one-workgroup state kernel, k_display), a metered one three (k_display_hist,
k_display_meter, k_display).  The floors are bytes over 8 TB/s: 12 B per pixel for the histogram, 16 B per pixel for the display.  The
kernels' own times come from a run of `--loop N` under `rocprofv3 --kernel-trace --stats`: N metered ACES calls on the sum and nothing else
after the set-up.  There is no pass threshold: the feature is opt-in.

    python tools/display_probe.py [--reps 7] [--calls 64]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/display_probe.py --loop 200
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
CURVES = ("reference", "reinhard", "aces", "clamp")


def call_ms(call, sync, calls, reps):
    def batch():
        for _ in range(calls):
            call()
        sync()
    batch()
    batch()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        batch()
        ts.append((time.perf_counter() - t0) * 1e3 / calls)
    return {"median": round(float(np.median(ts)), 5), "min": round(float(np.min(ts)), 5), "max": round(float(np.max(ts)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--loop", type=int, default=0, help="only N metered ACES calls on the sum (for a kernel trace)")
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
            scene.display(inv, curve="aces", auto=True, adapt=0.5, sync=False)
        scene.sync()
        print(json.dumps({"probe": "display_loop", "calls": args.loop, "state": {k: float(v) for k, v in scene.display_state().items()}}))
        scene.close()
        return
    scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
    scene.denoise(inv)
    scene.temporal(inv)
    out = {"probe": "display", "triangles": int(mesh.triangles.shape[0]), "width": W, "height": H, "calls": args.calls, "reps": args.reps,
           "floor_ms": {"k_display_hist": round(W * H * 12 / HBM_BYTES_PER_MS, 5), "k_display": round(W * H * 16 / HBM_BYTES_PER_MS, 5)}}
    out["resolve_device_ms"] = call_ms(lambda: scene.resolve_device(inv, sync=False), scene.sync, args.calls, args.reps)
    for curve in CURVES:
        out[f"sum_{curve}_manual_ms"] = call_ms(lambda: scene.display(inv, curve=curve, exposure=0.5, sync=False), scene.sync, args.calls, args.reps)
        out[f"sum_{curve}_auto_ms"] = call_ms(lambda: scene.display(inv, curve=curve, auto=True, adapt=0.5, sync=False), scene.sync, args.calls, args.reps)
    for source in ("denoised", "temporal"):
        out[f"{source}_aces_manual_ms"] = call_ms(lambda: scene.display(inv, source=source, curve="aces", exposure=0.5, sync=False), scene.sync, args.calls, args.reps)
        out[f"{source}_aces_auto_ms"] = call_ms(lambda: scene.display(inv, source=source, curve="aces", auto=True, adapt=0.5, sync=False), scene.sync, args.calls, args.reps)
    st = scene.display_state()
    out["state"] = {k: float(v) for k, v in st.items()}
    hist = scene.display_histogram()
    out["occupied_bins"] = int((hist != 0).sum())
    out["largest_bin_share"] = round(float(hist.max()) / max(int(hist.sum()), 1), 4)
    scene.close()
    print(json.dumps(out))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
