"""Instanced scenes (include/crt.h crt_instances_*): the host arithmetic of the numerical contract without a GPU; on the GPU the two-level
walk against a flat trace of the same geometry, against per-instance flat traces of object rays (reference (a)) and against the numpy
brute force (reference (b)), sets, refused sets, sharing, scale and the device form."""
import ctypes as C

import numpy as np
import pytest

from conftest import numpy_brute_force, seeded_rays

f32 = np.float32


# ---------------------------------------------------------------- host restatements of the contract ----

def np_inverse(m):
    """float64 restatement of crt_instance_inverse: adjugate / det, det along the first row, translation 0 - (W_A . t)."""
    m = np.asarray(m, np.float32).astype(np.float64).reshape(3, 4)
    a, b, c, d, e, f, g, h, i = m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2], m[2, 0], m[2, 1], m[2, 2]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    adj = np.array([[c00, c * h - b * i, b * f - c * e], [c01, a * i - c * g, c * d - a * f], [c02, b * g - a * h, a * e - b * d]])
    W = adj / det
    t = 0.0 - ((W[:, 0] * m[0, 3] + W[:, 1] * m[1, 3]) + W[:, 2] * m[2, 3])
    return np.concatenate([W, t[:, None]], 1).astype(np.float32).reshape(12)


def random_matrices(rng, n, scale_lo=1e-3, scale_hi=1e3, shear=True):
    """rotations x non-uniform scales (with mirrors) x shears, plus translations"""
    out = np.zeros((n, 3, 4), np.float64)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        s = np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), 3)) * rng.choice([-1.0, 1.0], 3)
        A = q @ np.diag(s)
        if shear and rng.random() < 0.5:
            S = np.eye(3)
            S[0, 1], S[1, 2] = rng.uniform(-0.5, 0.5, 2)
            A = A @ S
        out[k, :, :3] = A
        out[k, :, 3] = rng.uniform(-20, 20, 3)
    return out.astype(np.float32)


IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def object_rays(rays, w, identity):
    """the kernel's world -> object ray: fp32, no fma, in the contract's order; bitwise-identity instances keep the ray as it is"""
    out = rays.copy()
    if identity:
        return out
    W = np.asarray(w, np.float32).reshape(3, 4)
    o, d = rays["o"].astype(f32), rays["d"].astype(f32)
    with np.errstate(all="ignore"):
        for r in range(3):
            out["o"][:, r] = (((W[r, 0] * o[:, 0] + W[r, 1] * o[:, 1]).astype(f32) + W[r, 2] * o[:, 2]).astype(f32) + W[r, 3]).astype(f32)
            out["d"][:, r] = ((W[r, 0] * d[:, 0] + W[r, 1] * d[:, 1]).astype(f32) + W[r, 2] * d[:, 2]).astype(f32)
    return out


def is_identity(m):
    return np.array_equal(np.asarray(m, np.float32).reshape(12).view(np.uint32), IDENTITY.reshape(12).view(np.uint32))


# ---------------------------------------------------------------- CPU ----

def test_layouts(cr):
    from caitlynrenderer_amd import _lib
    assert C.sizeof(_lib.crt_instance) == 64 and cr.INSTANCE_DT.itemsize == 64
    assert _lib.crt_instance.mesh.offset == 48
    d = _lib.crt_blas_desc
    assert (d.vertices.offset, d.n_vertices.offset, d.triangles.offset, d.n_triangles.offset) == (0, 8, 16, 24) and C.sizeof(d) == 32


def test_inverse_is_the_float64_adjugate_bit_for_bit(cr):
    rng = np.random.default_rng(7)
    M = random_matrices(rng, 10000)
    worst = 0.0
    for m in M:
        w = cr.instance_inverse(m)
        assert np.array_equal(w.view(np.uint32), np_inverse(m).view(np.uint32))
        # W . M = I up to the conditioning of A (float rounding of both matrices)
        A, W = m[:, :3].astype(np.float64), w.reshape(3, 4)[:, :3].astype(np.float64)
        cond = np.linalg.cond(A)
        err = np.abs(W @ A - np.eye(3)).max()
        worst = max(worst, err / cond)
        p = np.array([0.3, -1.2, 2.5])
        back = W @ (A @ p + m[:, 3]) + w.reshape(3, 4)[:, 3]
        assert np.abs(back - p).max() <= 1e-5 * cond * (1 + np.abs(m[:, 3]).max() / np.abs(A).max() + np.abs(p).max())
    assert worst < 1e-6, worst                       # |W A - I| <= 1e-6 cond(A)


def test_inverse_identity_singular_and_non_finite(cr):
    from caitlynrenderer_amd import _lib
    w = cr.instance_inverse(IDENTITY)
    assert np.array_equal(w.view(np.uint32), IDENTITY.reshape(12).view(np.uint32))
    bad = [np.zeros((3, 4), np.float32), np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 0, 1, 0]], np.float32)]
    for k in range(12):
        for v in (np.nan, np.inf, -np.inf):
            m = IDENTITY.copy().reshape(12)
            m[k] = v
            bad.append(m)
    bad.append(np.array([[1e-39, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32))       # inverse overflows float
    for m in bad:
        with pytest.raises(cr.CrtError) as e:
            cr.instance_inverse(m)
        assert e.value.code == _lib.CRT_ERR_INVALID


def test_world_box_contains_the_transformed_corners_within_the_margin(cr):
    rng = np.random.default_rng(3)
    for m in random_matrices(rng, 2000):
        lo = rng.uniform(-5, 5, 3).astype(f32)
        box = np.concatenate([lo, lo + rng.uniform(0, 4, 3).astype(f32)])
        out = cr.instance_world_box(m, box).astype(np.float64)
        corners = np.array([[box[3 * ((k >> a) & 1) + a] for a in range(3)] for k in range(8)], np.float64)
        wc = corners @ m[:, :3].astype(np.float64).T + m[:, 3].astype(np.float64)
        tlo, thi = wc.min(0), wc.max(0)
        assert (out[:3] <= tlo).all() and (out[3:] >= thi).all()
        big = np.abs(np.concatenate([tlo, thi])).max()
        pad = big * 2.0 ** -16
        slack = pad + 2 * np.spacing(np.float32(big)).astype(np.float64)
        assert (tlo - out[:3] <= slack).all() and (out[3:] - thi <= slack).all()


def test_device_entry_points_fail_loudly_without_gpu(cr, cornell):
    from caitlynrenderer_amd import _lib
    if _lib.lib().crt_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    mesh, _ = cornell
    with pytest.raises(cr.CrtError) as e:
        cr.InstancedScene([mesh], cr.instances_array([IDENTITY], [0]))
    assert e.value.code == _lib.CRT_ERR_NO_DEVICE


# ---------------------------------------------------------------- GPU ----

def flat_scene(cr, mesh, cam, builder="sah"):
    return cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder=builder), 16, 16, 1)


def concat_meshes(cr, meshes):
    vs, ns, ts, off_v, off_n = [], [], [], 0, 0
    offsets = []
    for m in meshes:
        t = m.triangles.copy()
        t[:, 0:3] += off_v
        t[:, 4:7] += off_n
        offsets.append(sum(x.shape[0] for x in ts))
        vs.append(m.vertices); ns.append(m.normals); ts.append(t)
        off_v += m.vertices.shape[0]; off_n += m.normals.shape[0]
    m0 = meshes[0]
    return cr.Mesh(np.concatenate(vs), np.concatenate(ns), np.zeros((0, 2), f32), np.concatenate(ts), m0.materials, m0.lights), np.array(offsets)


def edge_rays(cr, n=4096):
    rng = np.random.default_rng(2)
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"] = (0.3 + 4.9 * rng.random((n, 3))).astype(f32)
    dirs = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0.6, 0.8), (0.6, 0, -0.8),
                     (-0.0, 1, 0), (0, 0, 0)], f32)
    rays["d"] = dirs[np.arange(n) % len(dirs)]
    rays["tmax"] = f32(1e9)
    rays["o"][5] = (np.nan, 1, 1); rays["o"][6] = (1, -np.inf, 1); rays["d"][7] = (np.nan, 1, 0)
    return rays


def reference_a(flat_scenes, mesh_of, w2o, ident, rays, any_hit=False):
    """per instance: crt_trace of the object rays on that mesh's flat scene; reduced over instances by (t, instance, id).
    Returns (t, u, v, tri, inst) for closest; (hit matrix [instance, ray]) for any."""
    n = rays.shape[0]
    T = np.full((len(mesh_of), n), np.inf, np.float64)
    hits = []
    for k, mk in enumerate(mesh_of):
        h = flat_scenes[mk].trace(object_rays(rays, w2o[k], ident[k]))
        hits.append(h)
        T[k] = np.where(h["tri"] >= 0, h["t"].astype(np.float64), np.inf)
    if any_hit:
        return np.isfinite(T)
    best = np.argmin(T, axis=0)                           # first minimum = the lowest instance among equal t
    hit = np.isfinite(T[best, np.arange(n)])
    out = np.zeros(n, [("t", f32), ("u", f32), ("v", f32), ("tri", np.int32), ("inst", np.int32)])
    for k in range(len(mesh_of)):
        sel = hit & (best == k)
        for f in ("t", "u", "v", "tri"):
            out[f][sel] = hits[k][f][sel]
        out["inst"][sel] = k
    out["tri"][~hit] = -1
    out["inst"][~hit] = -1
    return out


def assert_closest_equal(got, ids, want):
    assert np.array_equal(got["tri"], want["tri"]), np.nonzero(got["tri"] != want["tri"])[0][:10]
    assert np.array_equal(ids, want["inst"])
    h = want["tri"] >= 0
    for f in ("t", "u", "v"):
        assert np.array_equal(got[f][h].view(np.uint32), want[f][h].view(np.uint32)), f


@pytest.fixture(scope="module")
def meshes3(cr, cornell, tess8, tess40):
    return [cornell[0], tess8[0], tess40[0]]


def side_by_side(cr, meshes):
    """the meshes moved apart in their own vertex data (the three boxes coincide otherwise: surfaces of different meshes then cross each
    other, and which of two hits a few ulps apart a walk keeps depends on its tree's culling, flat or not)"""
    out = []
    for k, m in enumerate(meshes):
        v = (m.vertices + np.array([8.0 * k, 0.0, 0.0], f32)).astype(f32)
        out.append(cr.Mesh(v, m.normals, m.texcoords, m.triangles, m.materials, m.lights))
    return out


@pytest.mark.gpu
def test_identity_instances_equal_a_flat_trace(cr, cornell, meshes3):
    _, cam = cornell
    ms = side_by_side(cr, meshes3)
    flat_mesh, offsets = concat_meshes(cr, ms)
    flat = flat_scene(cr, flat_mesh, cam)
    inst = cr.instances_array([IDENTITY] * 3, [0, 1, 2])
    sc = cr.InstancedScene(ms, inst)
    er = edge_rays(cr)
    er["o"][:, 0] += f32(8.0) * (np.arange(er.shape[0]) % 3)
    rays = np.concatenate([seeded_rays(flat_mesh, 20000, 5, cr.RAY_DT), er])
    want = flat.trace(rays)
    got, ids = sc.trace(rays)
    h = want["tri"] >= 0
    assert h.sum() > 10000
    mesh_of_tri = np.searchsorted(offsets, np.maximum(want["tri"], 0), side="right") - 1
    bad = np.nonzero(ids != np.where(h, mesh_of_tri, -1))[0]
    assert bad.size == 0, (bad.size, bad[:8], want[bad[:8]], got[bad[:8]], ids[bad[:8]])
    assert np.array_equal(np.where(ids >= 0, got["tri"] + offsets[np.maximum(ids, 0)], -1), want["tri"])
    for f in ("t", "u", "v"):
        assert np.array_equal(got[f][h].view(np.uint32), want[f][h].view(np.uint32)), f
    ga, ia = sc.trace(rays, cr.CRT_TRACE_ANY)
    wa = flat.trace(rays, cr.CRT_TRACE_ANY)
    assert np.array_equal(ga["tri"] >= 0, wa["tri"] >= 0) and np.array_equal(ia >= 0, wa["tri"] >= 0)
    assert sc.info()["stack_overflows"] == 0
    sc.close(); flat.close()


@pytest.mark.gpu
def test_one_identity_instance_walks_the_same_tree(cr, cornell, tess40):
    _, cam = cornell
    mesh = tess40[0]
    flat = flat_scene(cr, mesh, cam)
    sc = cr.InstancedScene([mesh], cr.instances_array([IDENTITY], [0]))
    rays = np.concatenate([seeded_rays(mesh, 20000, 9, cr.RAY_DT), edge_rays(cr)])
    want, wst = flat.trace(rays, stats=True)
    got, ids, gst = sc.trace(rays, stats=True)
    h = want["tri"] >= 0
    assert np.array_equal(got["tri"], want["tri"]) and np.array_equal(got["t"][h].view(np.uint32), want["t"][h].view(np.uint32))
    assert np.array_equal(gst["nodes"][h], wst["nodes"][h].astype(np.int64) + 1)      # + the TLAS root
    assert np.array_equal(gst["tris"][h], wst["tris"][h])
    sc.close(); flat.close()


def placed_instances(rng, n, n_meshes, spread=12.0, scale=(0.5, 2.0)):
    M = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        s = rng.uniform(*scale, 3) * rng.choice([-1.0, 1.0], 3)
        A = q @ np.diag(s)
        M.append(np.concatenate([A, rng.uniform(-spread, spread, (3, 1))], 1))
    return np.array(M, f32), rng.integers(0, n_meshes, n)


def world_rays(cr, rng, n, spread=16.0, centres=None):
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"] = rng.uniform(-spread, spread, (n, 3)).astype(f32)
    d = rng.normal(size=(n, 3))
    if centres is not None:             # half of them aimed at instance origins, so that most hit something
        k = n // 2
        tgt = centres[rng.integers(0, len(centres), k)] + rng.normal(scale=1.0, size=(k, 3))
        d[:k] = tgt - rays["o"][:k]
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmax"] = f32(1e9)
    rays["tmax"][::7] = f32(9.0)
    return rays


@pytest.fixture(scope="module")
def transformed(cr, cornell, meshes3):
    _, cam = cornell
    rng = np.random.default_rng(21)
    M, mesh_of = placed_instances(rng, 300, 3)
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of))
    flats = [flat_scene(cr, m, cam) for m in meshes3]
    w2o = sc.world_to_object()
    ident = [is_identity(m) for m in M]
    yield sc, flats, M, mesh_of, w2o, ident, rng
    sc.close()
    for s in flats:
        s.close()


@pytest.mark.gpu
def test_transformed_instances_against_two_references(cr, meshes3, transformed):
    sc, flats, M, mesh_of, w2o, ident, rng = transformed
    for k, m in enumerate(M):
        assert np.array_equal(w2o[k].view(np.uint32), cr.instance_inverse(m).view(np.uint32))
    rays = world_rays(cr, rng, 8192, centres=M[:, :, 3])
    got, ids = sc.trace(rays)
    want = reference_a(flats, mesh_of, w2o, ident, rays)
    assert (want["tri"] >= 0).sum() > 2000
    assert_closest_equal(got, ids, want)
    # (b) the numpy brute force, per instance on the same object rays, reduced the same way
    sub = rays[:48]
    T = np.full((len(M), sub.shape[0]), np.inf)
    TRI = np.full((len(M), sub.shape[0]), -1)
    for k in range(len(M)):
        tri, t, u, v = numpy_brute_force(meshes3[mesh_of[k]], object_rays(sub, w2o[k], ident[k]))
        T[k] = np.where(tri >= 0, t.astype(np.float64), np.inf)
        TRI[k] = tri
    best = np.argmin(T, axis=0)
    hit = np.isfinite(T[best, np.arange(sub.shape[0])])
    assert np.array_equal(ids[:48], np.where(hit, best, -1))
    assert np.array_equal(got["tri"][:48], np.where(hit, TRI[best, np.arange(sub.shape[0])], -1))
    assert np.array_equal(got["t"][:48][hit].view(np.uint32), T[best, np.arange(sub.shape[0])][hit].astype(f32).view(np.uint32))
    # any hit: same flag, and the reported instance is one that has a hit
    ga, ia = sc.trace(rays, cr.CRT_TRACE_ANY)
    H = reference_a(flats, mesh_of, w2o, ident, rays, any_hit=True)
    occ = H.any(0)
    assert np.array_equal(ga["tri"] >= 0, occ) and np.array_equal(ia >= 0, occ)
    assert H[ia[occ], np.nonzero(occ)[0]].all()
    assert sc.info()["stack_overflows"] == 0


def tight_world_corners(mesh, m):
    """the 8 corners of the mesh's float vertex box through object_to_world, in float64 (the exact box the margin pads)"""
    V = mesh.vertices[mesh.triangles[:, :3].reshape(-1)]
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    c = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])
    return c @ m[:, :3].astype(np.float64).T + m[:, 3].astype(np.float64)


def grazing_rays(cr, rng, corners, per_face=12):
    """Rays in the planes of the faces of the EXACT world box, through a point where the box touches the mesh (on the edge or the face
    of corners that attain it).  The origin sits 0 to 2 float steps outside the face (beyond the face rounded outward), 2 to 4 box
    magnitudes away along the plane.  The world ray then misses the exact box, while the object ray, rounded on its way into object space,
    may pass a few ulps inside it and cross a wall next to the edge: what the margin is for.  Returns the rays and which of them lie
    outside the exact box."""
    tlo, thi = corners.min(0), corners.max(0)
    B = np.abs(np.concatenate([tlo, thi])).max()
    rays, outside = [], []
    for a in range(3):
        for side in (0, 1):
            f = tlo[a] if side == 0 else thi[a]
            touching = corners[np.abs(corners[:, a] - f) <= 1e-9 * B]        # 1 (vertex), 2 (edge) or 4 (face) corners
            for _ in range(per_face):
                w = rng.random(len(touching))
                c = (w / w.sum()) @ touching
                c[a] = f
                d = rng.normal(size=3)
                d[a] = 0.0
                d /= np.linalg.norm(d)
                o = c - rng.uniform(2.0, 4.0) * B * d
                of = o.astype(f32)
                face = f32(f)                                   # the face rounded outward, then `steps` float steps further out
                if side == 0 and np.float64(face) > f:
                    face = np.nextafter(face, f32(-np.inf))
                if side == 1 and np.float64(face) < f:
                    face = np.nextafter(face, f32(np.inf))
                steps = int(rng.integers(0, 3))
                for _ in range(steps):
                    face = np.nextafter(face, f32(-np.inf) if side == 0 else f32(np.inf))
                of[a] = face
                rays.append((of, d.astype(f32)))
                outside.append(np.float64(face) < f if side == 0 else np.float64(face) > f)
    r = np.zeros(len(rays), cr.RAY_DT)
    r["o"] = np.array([x[0] for x in rays]); r["d"] = np.array([x[1] for x in rays]); r["tmax"] = f32(1e9)
    return r, np.array(outside)


@pytest.mark.gpu
def test_grazing_rays_at_the_exact_world_box_need_the_margin(cr, cornell, meshes3):
    """Rays that graze the exact (unpadded) world box of an instance at the corner where the box touches the mesh, from 2 to 4 box
    magnitudes away, against reference (a).  One instance per set, so that the TLAS root's child box is the world box itself (no
    quantisation slack on its low faces).  Rotations, mirrors and uniform scales 0.5 to 2 (cond_inf(A) <= 2), origins within 5 B: inside
    the bound crt.h states for the margin.
    Some of the hits come from rays that lie entirely outside the exact box: without the margin the TLAS would cull them."""
    _, cam = cornell
    rng = np.random.default_rng(77)
    meshes = meshes3[:2]
    flats = [flat_scene(cr, m, cam) for m in meshes]
    M, mesh_of = [], []
    for _ in range(48):
        # a signed axis permutation x a rotation about one axis x a uniform scale: the world box then touches the box-shaped mesh along
        # whole edges (and faces), where a grazing ray can meet it
        c = int(rng.integers(0, 3))
        th = rng.uniform(0.2, 1.3)
        R = np.eye(3)
        i, j = [k for k in range(3) if k != c]
        R[i, i], R[i, j], R[j, i], R[j, j] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
        P = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)
        A = rng.uniform(0.5, 2.0) * (P @ R)
        M.append(np.concatenate([A, rng.uniform(-12, 12, (3, 1))], 1))
        mesh_of.append(int(rng.integers(0, 2)))
    M = np.array(M, f32)
    sc = cr.InstancedScene(meshes, cr.instances_array(M[:1], mesh_of[:1]), capacity=len(M))
    n_hits = n_outside_hits = 0
    all_rays = []
    for k in range(len(M)):
        sc.set(cr.instances_array(M[k:k + 1], mesh_of[k:k + 1]))
        r, outside = grazing_rays(cr, rng, tight_world_corners(meshes[mesh_of[k]], M[k]))
        got, ids = sc.trace(r)
        want = reference_a(flats, [mesh_of[k]], sc.world_to_object(), [False], r)
        assert_closest_equal(got, ids, want)
        hit = want["tri"] >= 0
        n_hits += int(hit.sum()); n_outside_hits += int((hit & outside).sum())
        all_rays.append(r)
    assert n_hits >= 50 and n_outside_hits >= 10, (n_hits, n_outside_hits)
    # all of them together: grazing rays of one instance pass other instances' boxes too
    sc.set(cr.instances_array(M, mesh_of))
    r = np.concatenate(all_rays)
    got, ids = sc.trace(r)
    assert_closest_equal(got, ids, reference_a(flats, mesh_of, sc.world_to_object(), [False] * len(M), r))
    sc.close()
    for f in flats:
        f.close()


@pytest.mark.gpu
def test_sets_refused_sets_and_counts(cr, cornell, meshes3, transformed):
    from caitlynrenderer_amd import _lib
    import torch
    _, flats, M, mesh_of, _, _, rng = transformed
    rays = world_rays(cr, rng, 8192, centres=M[:, :, 3])
    inst_a = cr.instances_array(M[:200], mesh_of[:200])
    M2, mo2 = placed_instances(np.random.default_rng(5), 250, 3)
    inst_b = cr.instances_array(M2, mo2)
    sc = cr.InstancedScene(meshes3, inst_a, capacity=300)
    fresh_b = cr.InstancedScene(meshes3, inst_b)
    want_b = fresh_b.trace(rays, stats=True)
    fresh_b.close()
    sc.set(inst_b)
    got = sc.trace(rays, stats=True)
    for g, w in zip(got, want_b):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    # the device form
    sc.set(inst_a)
    dev = torch.from_numpy(inst_b.view(np.uint8).copy()).cuda()
    sc.set_device(dev.data_ptr(), len(inst_b))
    got = sc.trace(rays, stats=True)
    for g, w in zip(got, want_b):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    # refused sets leave the previous state tracing bit-identically
    nan_m = inst_b.copy(); nan_m["object_to_world"][17, 5] = np.nan
    sing = inst_b.copy(); sing["object_to_world"][3] = 0
    badmesh = inst_b.copy(); badmesh["mesh"][9] = 3
    for bad in (nan_m, sing, badmesh):
        with pytest.raises(cr.CrtError) as e:
            sc.set(bad)
        assert e.value.code == _lib.CRT_ERR_INVALID
        d = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
        with pytest.raises(cr.CrtError) as e:
            sc.set_device(d.data_ptr(), len(bad))
        assert e.value.code == _lib.CRT_ERR_INVALID
    with pytest.raises(cr.CrtError) as e:
        sc.set(cr.instances_array(np.concatenate([M2, M2]), np.concatenate([mo2, mo2])))
    assert e.value.code == _lib.CRT_ERR_INVALID
    got = sc.trace(rays, stats=True)
    for g, w in zip(got, want_b):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    with pytest.raises(cr.CrtError) as e:
        sc.trace(rays, cr.CRT_TRACE_BVH2)
    assert e.value.code == _lib.CRT_ERR_INVALID
    # count changes within capacity; zero instances: every ray misses; one instance
    sc.set(inst_b[:1])
    g1, i1 = sc.trace(rays)
    w2o = sc.world_to_object()
    assert_closest_equal(g1, i1, reference_a(flats, mo2[:1], w2o, [False], rays))
    sc.set(inst_b[:0])
    g0, i0 = sc.trace(rays)
    assert (g0["tri"] == -1).all() and (i0 == -1).all()
    ga, ia = sc.trace(rays, cr.CRT_TRACE_ANY)
    assert (ga["tri"] == -1).all() and (ia == -1).all()
    sc.set(inst_b)
    assert sc.info()["n_instances"] == 250 and sc.info()["stack_overflows"] == 0
    sc.close()
    empty = cr.InstancedScene(meshes3, inst_b[:0], capacity=4)
    assert (empty.trace(rays)[1] == -1).all()
    empty.close()


def clustered_mesh(K):
    """K clusters of 8 triangles, each cluster 4x smaller than the previous and beside it: a SAH builder splits one cluster off per level,
    and the CWBVH converter spends its expansions on the big cluster, so the CWBVH is about K node8 levels deep"""
    V, T = [], []
    for k in range(K):
        s = 4.0 ** -k
        for j in range(8):
            b = len(V)
            cx, cy = s + s * (j % 4) / 4, s * (j // 4) / 2
            V += [(cx, cy, 0.0), (cx + s / 4, cy, 0.0), (cx, cy + s / 2, s / 8)]
            T.append([b, b + 1, b + 2])
    t = np.zeros((len(T), 12), np.int32)
    t[:, :3] = T
    return np.array(V, f32), t


def clustered_instances(K, first=0):
    """8 instances per cluster, each cluster 4x smaller (uniform scale) and beside the previous: a TLAS about K node8 levels deep"""
    M = []
    for k in range(first, first + K):
        s = 4.0 ** -k
        for j in range(8):
            M.append(np.concatenate([np.eye(3) * s, np.array([[s * (10.0 + 3.0 * j)], [0.0], [0.0]])], 1))
    return np.array(M, f32)


@pytest.mark.gpu
def test_stack_limit_refuses_and_keeps_the_previous_state(cr):
    """TLAS depth + deepest BLAS depth beyond the walk's 40 stack entries: CRT_ERR_LIMIT at create and at set, and a refused set leaves
    the previous instances tracing bit for bit."""
    from caitlynrenderer_amd import _lib
    V, T = clustered_mesh(30)
    inst1 = cr.instances_array(clustered_instances(1), np.zeros(8))
    sc = cr.InstancedScene([(V, T)], inst1, capacity=8 * 48)
    info = sc.info()
    db = info["max_blas_depth8"]
    assert 20 <= db <= 38 and info["stack_entries"] <= 40, info
    rng = np.random.default_rng(4)
    rays = np.zeros(4096, cr.RAY_DT)
    rays["o"] = np.array([-1.0, 0.2, 0.05], f32) + rng.normal(scale=0.02, size=(4096, 3)).astype(f32)
    rays["o"][:, 0] = rng.uniform(0.0, 40.0, 4096).astype(f32)
    rays["o"][:, 2] = f32(5.0)
    rays["d"] = np.array([0.0, 0.0, -1.0], f32)
    rays["tmax"] = f32(1e9)
    before = sc.trace(rays, stats=True)
    assert (before[1] >= 0).sum() > 100
    deep = cr.instances_array(clustered_instances(48 - db), np.zeros(8 * (48 - db)))
    with pytest.raises(cr.CrtError) as e:
        sc.set(deep)
    assert e.value.code == _lib.CRT_ERR_LIMIT
    after = sc.trace(rays, stats=True)
    for g, w in zip(after, before):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert sc.info()["n_instances"] == 8 and sc.info()["stack_entries"] == info["stack_entries"]
    sc.close()
    with pytest.raises(cr.CrtError) as e:
        cr.InstancedScene([(V, T)], deep)
    assert e.value.code == _lib.CRT_ERR_LIMIT


@pytest.mark.gpu
def test_one_mesh_shared_by_4096_instances(cr, cornell, tess8):
    _, cam = cornell
    mesh = tess8[0]
    rng = np.random.default_rng(33)
    M, _ = placed_instances(rng, 4096, 1, spread=60.0)
    one = cr.InstancedScene([mesh], cr.instances_array(M[:1], [0]))
    many = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(4096)))
    i1, i2 = one.info(), many.info()
    assert i1["blas_bytes"] == i2["blas_bytes"] and i1["blas_nodes8"] == i2["blas_nodes8"]
    one.close()
    flat = flat_scene(cr, mesh, cam)
    rays = world_rays(cr, rng, 2048, spread=64.0, centres=M[:, :, 3])
    got, ids = many.trace(rays)
    w2o = many.world_to_object()
    want = reference_a([flat], np.zeros(4096, int), w2o, [is_identity(m) for m in M], rays)
    assert (want["tri"] >= 0).sum() > 500
    assert_closest_equal(got, ids, want)
    many.close(); flat.close()


@pytest.mark.gpu
def test_64_instances_of_the_million_triangle_mesh(cr, cornell):
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, cam = cornell
    mesh = tessellated_cornell(base, 183)
    assert mesh.triangles.shape[0] == 1004672
    rng = np.random.default_rng(64)
    ext = float((mesh.vertices.max(0) - mesh.vertices.min(0)).max())
    M = []
    for gx in range(8):
        for gy in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
    M = np.array(M, f32)
    sc = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(64)))
    flat = flat_scene(cr, mesh, cam)
    rays = world_rays(cr, rng, 100000, spread=6 * ext, centres=M[:, :, 3])
    rays["o"] += f32(5.25 * ext) * np.array([1, 1, 0], f32)
    got, ids = sc.trace(rays)
    w2o = sc.world_to_object()
    want = reference_a([flat], np.zeros(64, int), w2o, [False] * 64, rays)
    assert (want["tri"] >= 0).sum() > 20000
    assert_closest_equal(got, ids, want)
    assert sc.info()["stack_overflows"] == 0
    sc.close(); flat.close()


@pytest.mark.gpu
def test_trace_device_with_torch_tensors(cr, meshes3, transformed):
    import torch
    sc, _, M, _, _, _, rng = transformed
    rays = world_rays(cr, rng, 5000, centres=M[:, :, 3])
    want, wid, wst = sc.trace(rays, stats=True)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.empty(5000 * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.empty(5000, dtype=torch.int32, device="cuda")
    d_st = torch.empty(5000 * 4, dtype=torch.uint8, device="cuda")
    sc.trace_device(d_rays.data_ptr(), 5000, d_hits.data_ptr(), d_ids.data_ptr(), cr.CRT_TRACE_CLOSEST, d_st.data_ptr(), sync=False)
    torch.cuda.synchronize()                  # the device synchronise covers the handle's own stream
    assert np.array_equal(d_hits.cpu().numpy(), want.view(np.uint8))
    assert np.array_equal(d_ids.cpu().numpy(), wid)
    assert np.array_equal(d_st.cpu().numpy(), wst.view(np.uint8))
