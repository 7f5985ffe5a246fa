"""The deformer on the GPU: prints ONE JSON line.

The 1,004,672-triangle mesh with a synthetic rig: bones along the y axis, each turned a little about it; "smooth" gives every vertex
four neighbouring bones with Gaussian weights, "single" one bone at weight 1 (the three zero weights skip their bones' loads).  Normals
take their influences from normal_influences.

  pose     per palette form (CRT_DEFORM_PALETTE: "lds" = staged per workgroup where n_bones <= 256, "global" = through the vector
           cache), n_bones 16 / 256 / 4096 and rig: kernel_us, the stream time of one synchronised pose's kernel (device events; median,
           minimum and maximum of --reps after two warm-ups), and call_us, the wall time of --calls unsynchronised poses and one
           synchronise over the calls (copy of the pose, launch and kernel, the host running one pose ahead).  floor_us: the element
           streams, 48 B per vertex and per normal, over 8 TB/s.
  frame    Scene.deform (wall ms per synchronised call, 1920 x 1080 scene, 16 smooth bones) beside the two ways there were before:
           deform_host + update_vertices with normals (the CPU deform and the upload apart), and a torch tensor skinned by torch ops
           + update_vertices_device (positions only).  frame_ms: four-sample frames at depth 3 after each; the trees hold the same
           positions (torch's to its own rounding), so the three agree.

There is no pass threshold.

    python tools/deform_probe.py [--reps 7] [--calls 64] [--out profiles/deform_probe.txt]
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

HBM_BYTES_PER_US = 8e12 / 1e6
f32 = np.float32


def rig(cr, mesh, n_bones, smooth):
    V = mesh.vertices
    y = (V[:, 1] - V[:, 1].min()) / max(float(np.ptp(V[:, 1])), 1e-6) * (n_bones - 1)
    if smooth and n_bones >= 4:
        b0 = np.clip(np.floor(y).astype(np.int64) - 1, 0, n_bones - 4)
        vb = (b0[:, None] + np.arange(4)).astype(np.uint16)
        w = np.exp(-(y[:, None] - vb) ** 2)
        vw = (w / w.sum(1, keepdims=True)).astype(f32)
    else:
        vb = np.repeat(np.rint(y).astype(np.uint16)[:, None], 4, 1)
        vw = np.tile(np.array([1, 0, 0, 0], f32), (V.shape[0], 1))
    nb, nw = cr.normal_influences(mesh.triangles, vb, vw, mesh.normals.shape[0])
    return dict(rest_vertices=V, vertex_bones=vb, vertex_weights=vw, rest_normals=mesh.normals, normal_bones=nb, normal_weights=nw)


def pose_of(n_bones, phase):
    """every bone a rotation about the y axis, the angle a smooth function of the bone"""
    a = 0.15 * np.sin(phase + np.linspace(0.0, 3.0, n_bones))
    B = np.zeros((n_bones, 3, 4), f32)
    B[:, 0, 0], B[:, 0, 2], B[:, 1, 1], B[:, 2, 0], B[:, 2, 2] = np.cos(a), np.sin(a), 1.0, -np.sin(a), np.cos(a)
    return B


def stats(ts):
    return {"median": round(float(np.median(ts)), 3), "min": round(float(np.min(ts)), 3), "max": round(float(np.max(ts)), 3)}


def pose_arm(d, poses, calls, reps):
    for k in range(2):
        d.pose(poses[k])
    kernel = []
    for k in range(reps):
        d.pose(poses[k & 1])
        kernel.append(d.last_ms() * 1e3)
    call = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for k in range(calls):
            d.pose(poses[k & 1], sync=False)
        d.sync()
        call.append((time.perf_counter() - t0) * 1e6 / calls)
    return {"kernel_us": stats(kernel), "call_us": stats(call)}


def frame_ms(scene, reps):
    rvs = [(0.25 + 0.01 * k, 0.75 - 0.01 * k) for k in range(4)]
    scene.render_frames(rvs)
    scene.render_frames(rvs)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scene.render_frames(rvs)
        ts.append((time.perf_counter() - t0) * 1e3 / len(rvs))
    return round(statistics.median(ts), 4)


def wall_ms(call, reps):
    call(0)
    call(1)
    ts = []
    for k in range(reps):
        t0 = time.perf_counter()
        call(k & 1)
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--tess", type=int, default=183, help="tessellation of the Cornell box: 183 = 1,004,672 triangles")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    cr.warmup()
    base, cam = g._cornell()
    mesh = tessellated_cornell(base, args.tess)
    nv, nn = int(mesh.vertices.shape[0]), int(mesh.normals.shape[0])
    out = {"probe": "deform", "triangles": int(mesh.triangles.shape[0]), "vertices": nv, "normals": nn, "calls": args.calls, "reps": args.reps,
           "floor_us": round(48 * (nv + nn) / HBM_BYTES_PER_US, 3)}

    for form in cr.deform.PALETTE_FORMS:
        os.environ["CRT_DEFORM_PALETTE"] = form
        for n_bones in (16, 256, 4096):
            poses = [pose_of(n_bones, 0.0), pose_of(n_bones, 1.0)]
            for name, smooth in (("smooth", True), ("single", False)):
                d = cr.Deformer(n_bones=n_bones, **rig(cr, mesh, n_bones, smooth))
                arm = pose_arm(d, poses, args.calls, args.reps)
                if form == "lds" and n_bones > 256:
                    arm["note"] = "above the LDS limit: the global form ran"
                out[f"pose_{form}_{n_bones}_{name}"] = arm
                d.close()
    os.environ.pop("CRT_DEFORM_PALETTE", None)

    # the per-frame step, three ways, each on a scene of its own
    n_bones = 16
    case = rig(cr, mesh, n_bones, True)
    poses = [pose_of(n_bones, 0.0), pose_of(n_bones, 1.0)]
    W, H = 1920, 1080
    data = cr.SceneData.for_device_build(mesh, cam, builder="sah")
    d = cr.Deformer(n_bones=n_bones, **case)
    a, b, c = (cr.Scene(data, W, H, 3) for _ in range(3))
    for s in (a, b, c):
        s.update(cam)
    out["scene_deform_ms"] = wall_ms(lambda k: a.deform(d, poses[k]), args.reps)
    out["scene_deform_refit_device_ms"] = round(a.last_update_ms()[0], 4)
    host_part, upload_part = [], []

    def host_way(k):
        t0 = time.perf_counter()
        V, N = cr.deform_host(poses[k], **case)
        t1 = time.perf_counter()
        b.update_vertices(V, N)
        host_part.append((t1 - t0) * 1e3)
        upload_part.append((time.perf_counter() - t1) * 1e3)
    out["host_deform_plus_update_vertices_ms"] = wall_ms(host_way, args.reps)
    out["host_deform_alone_ms"] = stats(host_part[2:])
    out["update_vertices_with_normals_alone_ms"] = stats(upload_part[2:])

    dev = torch.device("cuda")
    t_rest = torch.from_numpy(case["rest_vertices"]).to(dev)
    t_idx = torch.from_numpy(case["vertex_bones"].astype(np.int64)).to(dev)
    t_w = torch.from_numpy(case["vertex_weights"]).to(dev)

    def torch_way(k):
        B = torch.from_numpy(poses[k]).to(dev)                                      # the pose crosses PCIe here too
        M = (t_w[:, :, None, None] * B[t_idx]).sum(1)                               # (nv, 3, 4)
        p = (torch.matmul(M[:, :, :3], t_rest[:, :, None])[:, :, 0] + M[:, :, 3]).contiguous()
        torch.cuda.synchronize()                                                    # the library reads it on the scene's own stream
        c.update_vertices_device(p.data_ptr(), nv)
    out["torch_skin_plus_update_vertices_device_ms"] = wall_ms(torch_way, args.reps)
    # all three hold pose (reps - 1) & 1 now
    # all three hold pose (reps - 1) & 1 now; two rounds, so that a drift of the clocks shows as one
    out["frame_ms_after"] = [{"scene_deform": frame_ms(a, args.reps), "host": frame_ms(b, args.reps), "torch": frame_ms(c, args.reps)} for _ in range(2)]
    for s in (a, b, c):
        s.close()
    d.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
