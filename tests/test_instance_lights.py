"""Lights that follow emissive instances in the frames of an instanced scene (include/crt.h crt_scene_create_instanced_lit).

CPU: the new symbols, the host arithmetic (crt_instance_lights, crt_lights_finish) against a numpy float32 restatement of the header's
rules, and the premise of G3: the flat oracle alone, fed inputs moved by 64 ulps, stays within the bounds G3 holds the GPU to.
GPU: G1 identity instances with mesh lights render the flat oracle's frames bit for bit; G2 the world light table under general
transforms equals the host functions applied to the handle's live matrices, across refits, sets and crt_scene_set_mesh_lights; G3 the
lamp moves: frames against the flat oracle before and after a refit; G4 the clamp and the refusals; G5 asynchronous frames and shards.
The scene helpers are those of tests/test_instances_frames.py."""
import ctypes as C
import types

import numpy as np
import pytest

from test_instances_frames import (IDENTITY, PIXEL_CAP, RVS, THREADS, H6, W6, close, compare_sums, rot, separated_scene, shading_of, split_mesh)
from test_instances_oracle import placed_instances

f32 = np.float32


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- the header's arithmetic in numpy float32 ----

def np_light(A, W, light):
    """one object-space light through A | t (3x4) with W = world_to_object, operation for operation as include/crt.h states it"""
    A, W, l = np.asarray(A, f32).reshape(3, 4), np.asarray(W, f32).reshape(3, 4), np.asarray(light, f32)
    out = np.zeros(18, f32)
    p, u, v, n = l[0:3], l[3:6], l[6:9], l[9:12]
    m = np.zeros(3, f32)
    for r in range(3):
        out[r] = f32(f32(f32(f32(A[r, 0] * p[0]) + f32(A[r, 1] * p[1])) + f32(A[r, 2] * p[2])) + A[r, 3])
        out[3 + r] = f32(f32(f32(A[r, 0] * u[0]) + f32(A[r, 1] * u[1])) + f32(A[r, 2] * u[2]))
        out[6 + r] = f32(f32(f32(A[r, 0] * v[0]) + f32(A[r, 1] * v[1])) + f32(A[r, 2] * v[2]))
        m[r] = f32(f32(f32(W[0, r] * n[0]) + f32(W[1, r] * n[1])) + f32(W[2, r] * n[2]))
    inv = f32(f32(1.0) / np.sqrt(f32(f32(f32(m[0] * m[0]) + f32(m[1] * m[1])) + f32(m[2] * m[2]))))
    out[9:12] = (m * inv).astype(f32)
    out[12:15] = l[12:15]
    uu, vv = out[3:6], out[6:9]
    c = np.array([f32(f32(uu[1] * vv[2]) - f32(uu[2] * vv[1])), f32(f32(uu[2] * vv[0]) - f32(uu[0] * vv[2])), f32(f32(uu[0] * vv[1]) - f32(uu[1] * vv[0]))], f32)
    out[15] = np.sqrt(f32(f32(f32(c[0] * c[0]) + f32(c[1] * c[1])) + f32(c[2] * c[2])))
    return out


def np_finish(table):
    """the pdf column by the tree-sum rule: a_k = area if finite and positive else +0, S = pairwise tree sum, pdf = a_k * (1 / S)"""
    t = np.array(table, f32).reshape(-1, 18)
    with np.errstate(all="ignore"):
        a = np.where(np.isfinite(t[:, 15]) & (t[:, 15] > 0), t[:, 15], f32(0)).astype(f32)
    n = 1
    while n < a.shape[0]:
        n *= 2
    s = np.concatenate([a, np.zeros(n - a.shape[0], f32)])
    while s.shape[0] > 1:
        s = (s[0::2] + s[1::2]).astype(f32)
    S = s[0] if s.shape[0] else f32(0)
    t[:, 16] = (a * f32(f32(1.0) / S)).astype(f32) if S > 0 else f32(0)
    return t


def random_lights(rng, n):
    l = np.zeros((n, 18), f32)
    l[:, 0:9] = rng.uniform(-2, 2, (n, 9))
    nn = rng.normal(size=(n, 3))
    l[:, 9:12] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    l[:, 12:15] = rng.uniform(0.5, 9, (n, 3))
    l[:, 15] = np.linalg.norm(np.cross(l[:, 3:6].astype(np.float64), l[:, 6:9].astype(np.float64)), axis=1)
    l[:, 16] = rng.uniform(0, 1, n)           # given pdfs and third words: the table must not depend on them
    l[:, 17] = rng.uniform(0, 1, n)
    return l


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- CPU 1: symbols and ABI ----

def test_library_exports_the_light_entries_and_refuses_null_arguments(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("crt_scene_create_instanced_lit", "crt_scene_set_mesh_lights", "crt_scene_read_lights", "crt_instance_lights", "crt_lights_finish"):
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    assert L.crt_abi_version() == 6
    assert C.sizeof(_lib.crt_mesh_lights) == 16
    refused = (_lib.CRT_ERR_INVALID, _lib.CRT_ERR_NO_DEVICE)
    out, n = C.c_void_p(), C.c_size_t()
    d = _lib.crt_instanced_scene_desc()
    assert L.crt_scene_create_instanced_lit(None, None, C.byref(out)) in refused
    assert L.crt_scene_create_instanced_lit(C.byref(d), None, None) in refused
    assert L.crt_scene_create_instanced_lit(C.byref(d), None, C.byref(out)) in refused and not out.value
    assert L.crt_scene_set_mesh_lights(None, 0, None, 0) == _lib.CRT_ERR_INVALID
    assert L.crt_scene_read_lights(None, None, 0, C.byref(n)) == _lib.CRT_ERR_INVALID
    one = np.zeros((1, 18), f32)
    m = IDENTITY.copy()
    assert L.crt_instance_lights(None, _ptr(one), 1, _ptr(one)) == _lib.CRT_ERR_INVALID
    assert L.crt_instance_lights(_ptr(m), None, 1, _ptr(one)) == _lib.CRT_ERR_INVALID
    assert L.crt_instance_lights(_ptr(m), _ptr(one), 1, None) == _lib.CRT_ERR_INVALID
    assert L.crt_lights_finish(None, 1) == _lib.CRT_ERR_INVALID
    assert L.crt_lights_finish(None, 0) == 0
    singular = np.zeros((3, 4), f32)
    assert L.crt_instance_lights(_ptr(singular), _ptr(one), 1, _ptr(one)) == _lib.CRT_ERR_INVALID


# ---------------------------------------------------------------- CPU 2: the host arithmetic ----

def test_host_light_arithmetic_equals_the_numpy_restatement(cr, cornell):
    rng = np.random.default_rng(1801)
    lights = random_lights(rng, 7)
    # a bitwise identity returns its input bytes, pdf and third word included
    assert np.array_equal(bits(cr.instance_lights(IDENTITY, lights)), bits(lights))
    # 50 random matrices: rotations, scales 0.5 - 2, mirrors
    M, _ = placed_instances(rng, 50, 1, spread=9.0)
    assert (np.linalg.det(M[:, :, :3].astype(np.float64)) < 0).sum() >= 10          # mirrors among them
    for A in M:
        W = cr.instance_inverse(A)
        got = cr.instance_lights(A, lights)
        want = np.stack([np_light(A, W, l) for l in lights])
        assert np.array_equal(bits(got), bits(want)), (A, got[0], want[0])
        assert (got[:, 16:18] == 0).all()
        # the light's side follows the shading normal: n' is the normalised inverse transpose applied to n, for mirrors too
        nn = lights[:, 9:12].astype(np.float64) @ np.linalg.inv(A[:, :3].astype(np.float64))
        assert np.allclose(got[:, 9:12], nn / np.linalg.norm(nn, axis=1, keepdims=True), atol=2e-6)
    # a translated identity takes the general path: the translation is added, the rest survives the multiplications by 1 and 0
    T = IDENTITY.copy()
    T[:, 3] = (1.5, -2.0, 0.25)
    got = cr.instance_lights(T, lights)
    assert np.array_equal(bits(got), bits(np.stack([np_light(T, cr.instance_inverse(T), l) for l in lights])))
    assert np.array_equal(got[:, 3:9], lights[:, 3:9])
    # the pdf column: tree sums at sizes around the powers of two and the 256-light blocks the device reduces by
    for n in (1, 2, 3, 5, 64, 65, 1000):
        t = random_lights(rng, n)
        t[:, 15] = rng.uniform(1e-3, 50.0, n) * 10.0 ** rng.integers(-3, 4, n)
        got = cr.lights_finish(t)
        want = np_finish(t)
        assert np.array_equal(bits(got), bits(want)), n
        assert abs(float(got[:, 16].astype(np.float64).sum()) - 1.0) < 1e-5
        cols = [c for c in range(18) if c != 16]
        assert np.array_equal(bits(got[:, cols]), bits(t[:, cols]))
    # areas that are not finite positive floats count as +0, and their lights are never chosen
    t = random_lights(rng, 6)
    t[:, 15] = (2.0, np.inf, np.nan, -1.0, 0.0, 6.0)
    got = cr.lights_finish(t)
    assert np.array_equal(bits(got[:, 16]), bits(np.array([0.25, 0, 0, 0, 0, 0.75], f32)))
    assert np.array_equal(bits(got), bits(np_finish(t)))
    t[:, 15] = (-3.0, np.nan, -np.inf, 0.0, -0.0, np.inf)          # S = 0: every pdf 0
    assert (cr.lights_finish(t)[:, 16] == 0).all() and not np.signbit(cr.lights_finish(t)[:, 16]).any()
    # the Cornell box's two lights: the loader's table bit for bit
    mesh = cornell[0]
    scrambled = mesh.lights.copy()
    scrambled[:, 16] = 7.0
    assert np.array_equal(bits(cr.lights_finish(scrambled)), bits(mesh.lights))


# ---------------------------------------------------------------- the scene of G3 ----

# the lamp quad of tests/test_instances_frames.py::separated_scene in OBJECT space, and its two poses (it keeps facing the scene)
LAMP_P, LAMP_U, LAMP_V = np.array([-0.75, 0.0, -0.65]), np.array([0.0, 0.0, 1.3]), np.array([1.5, 0.0, 0.0])
Q1 = np.concatenate([rot((0, 1, 0), 0.6) @ np.diag([1.2, 1.0, 0.8]), np.array([[-0.3], [5.0], [0.2]])], 1)
Q2 = np.concatenate([rot((0, 1, 0), -1.0) @ rot((0, 0, 1), 0.1) * 0.9, np.array([[1.5], [4.5], [1.0]])], 1)
# Bounds from the REFERENCE ALONE (test_reference_alone_moving_lamp re-measures them; DESIGN.md §18 records the measurements): the
# per-pixel bound and cap of check 6 of test_instances_frames.py (1e-3 * max(|ref|, 1), at most 19 of 19,200 pixels; the reference alone
# within 4), and a relative difference of the image means of at most 4 x the largest value three 64-ulp perturbations of the oracle's own
# input (vertices and the lights' p, u, v; the seeds of that file's experiment) gave on this scene, these frames and both poses:
# 2.13e-5 (pose Q1, depth 3, seed 2; Q1 leaves at most 2 pixels beyond the bound, Q2 none and at most 6.6e-6).
MEAN_RTOL_LAMP = 4 * 2.13e-5


def lamp_scene(cr):
    """separated_scene with the lamp as a mesh in object space that carries its two lights: (meshes, matrices with the lamp at Q1,
    materials, the lamp's object-space lights, camera)"""
    meshes, M, mats, _, _, cam = separated_scene(cr)
    lp, lu, lv = LAMP_P, LAMP_U, LAMP_V
    v = np.array([lp, lp + lu, lp + lu + lv, lp + lv], f32)
    lamp = cr.Mesh(v, meshes[4].normals, np.zeros((0, 2), f32), meshes[4].triangles, mats, np.zeros((0, 18), f32))
    area = 1.3 * 1.5
    obj = np.array([np.concatenate([lp, lu, lu + lv, (0, -1, 0), (6, 6, 6), (area, 0.5, 0)]),
                    np.concatenate([lp, lu + lv, lv, (0, -1, 0), (6, 6, 6), (area, 0.5, 0)])], f32)
    meshes = meshes[:4] + [lamp]
    M = M.copy()
    M[4] = Q1.astype(f32)
    return meshes, M, mats, obj, cam


def flatten(meshes, M, mats, obj_lights, lamp=4):
    """flatten(S) for the oracle, in double from the float32 matrices the handle gets, rounded once: vertices A v + t, normals by the
    inverse transpose at the object normal's length, the lamp's lights p' = A p + t, u' = A u, v' = A v, n' = unit inverse transpose,
    area = |u' x v'|, pdf = area / sum"""
    V, N, Tr = [], [], []
    for mesh, m in zip(meshes, np.asarray(M, f32).astype(np.float64)):
        a, tr = m[:, :3], m[:, 3]
        t = mesh.triangles.copy()
        t[:, 0:3] += sum(len(x) for x in V)
        t[:, 4:7] += sum(len(x) for x in N)
        V.append(mesh.vertices.astype(np.float64) @ a.T + tr)
        n = mesh.normals.astype(np.float64)
        nn = n @ np.linalg.inv(a)
        N.append(nn / np.linalg.norm(nn, axis=1, keepdims=True) * np.linalg.norm(n, axis=1, keepdims=True))
        Tr.append(t)
    m = np.asarray(M[lamp], f32).astype(np.float64)
    a, tr = m[:, :3], m[:, 3]
    o = obj_lights.astype(np.float64)
    L = np.zeros((o.shape[0], 18))
    L[:, 0:3], L[:, 3:6], L[:, 6:9] = o[:, 0:3] @ a.T + tr, o[:, 3:6] @ a.T, o[:, 6:9] @ a.T
    nn = o[:, 9:12] @ np.linalg.inv(a)
    L[:, 9:12] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    L[:, 12:15] = o[:, 12:15]
    L[:, 15] = np.linalg.norm(np.cross(L[:, 3:6], L[:, 6:9]), axis=1)
    L[:, 16] = L[:, 15] / L[:, 15].sum()
    return types.SimpleNamespace(vertices=np.concatenate(V).astype(f32), normals=np.concatenate(N).astype(f32), texcoords=None, triangles=np.concatenate(Tr),
                                 tri_orig_ids=None, materials=mats, lights=L.astype(f32), bvh=None, bvh8=None, bvh8_tri_slots=None, camera=None)


_LAMP_ORACLE = {}


def lamp_oracle_sum(ob, flat, cam, depth, key=None):
    """the flat oracle's 8-frame sum at 160 x 120; with a key, computed once and shared (never written to)"""
    if key is not None and (key, depth) in _LAMP_ORACLE:
        return _LAMP_ORACLE[(key, depth)]
    o = ob.Oracle(flat, W6, H6, depth, camera=cam)
    s = np.zeros((H6, W6, 3), f32)
    for rx, ry in RVS:
        o.render_frame(rx, ry, s, accel=ob.BRUTE, threads=THREADS)
    if key is not None:
        s.setflags(write=False)
        _LAMP_ORACLE[(key, depth)] = s
    return s


def posed(cr, pose):
    meshes, M, mats, obj, cam = lamp_scene(cr)
    M = M.copy()
    M[4] = np.asarray(pose, f32)
    return meshes, M, mats, obj, cam


# ---------------------------------------------------------------- CPU 3: the reference alone ----

@pytest.mark.parametrize("depth", [1, 3, 4])
def test_reference_alone_moving_lamp(cr, ob, depth):
    """The premise of G3: the flat oracle on the flattened scene at both poses of the lamp, and again with every vertex and every light's
    p, u, v moved by up to 64 ulps of its largest coordinate, three seeds: at most a quarter of the pixel cap beyond the per-pixel bound
    and a mean difference within the bound the GPU test uses (4 x the largest value measured here).  And the two poses give different
    pictures: a table that stayed behind could not pass G3."""
    sums = {}
    for name, pose in (("Q1", Q1), ("Q2", Q2)):
        meshes, M, mats, obj, cam = posed(cr, pose)
        flat = flatten(meshes, M, mats, obj)
        a = sums[name] = lamp_oracle_sum(ob, flat, cam, depth, key=name)
        assert (a.max(-1) > 0).mean() > 0.3
        for seed in (1, 2, 3):
            rng = np.random.default_rng(6400 + seed)
            step = np.spacing(np.abs(flat.vertices).max(1, keepdims=True))
            verts = (flat.vertices + rng.integers(-64, 65, flat.vertices.shape) * step).astype(f32)
            lights = flat.lights.copy()
            for c in (0, 3, 6):
                lstep = np.spacing(np.abs(lights[:, c:c + 3]).max(1, keepdims=True))
                lights[:, c:c + 3] = (lights[:, c:c + 3] + rng.integers(-64, 65, (lights.shape[0], 3)) * lstep).astype(f32)
            moved = types.SimpleNamespace(**{**vars(flat), "vertices": verts, "lights": lights})
            pixels, mean = compare_sums(a, lamp_oracle_sum(ob, moved, cam, depth))
            print("reference alone, pose", name, "depth", depth, "seed", seed, "pixels beyond", pixels, "mean diff %.2e" % mean)
            assert pixels <= PIXEL_CAP // 4 and mean <= MEAN_RTOL_LAMP / 4, (name, depth, seed, pixels, mean)
    differ = int((np.abs(sums["Q1"] - sums["Q2"]).max(-1) > 1e-3 * np.maximum(np.abs(sums["Q1"]).max(-1), 1.0)).sum())
    shift = abs(float(sums["Q1"].mean()) - float(sums["Q2"].mean())) / float(sums["Q1"].mean())
    print("poses Q1 / Q2, depth", depth, "pixels that differ", differ, "mean shift %.3f" % shift)
    assert differ > 5000, (depth, differ)


# ---------------------------------------------------------------- GPU helpers ----

def crt_cam(cam):
    from caitlynrenderer_amd._lib import crt_camera
    c = crt_camera()
    for k in ("position", "right", "up", "forward"):
        for i in range(3):
            getattr(c, k)[i] = getattr(cam, k)[i]
    c.fov, c.focal_dist, c.aperture = cam.fov, 0.1, 0.0
    return types.SimpleNamespace(c=c)


def expected_table(cr, inst, static, mesh_lights, mesh_of):
    """the world light table by the host functions from the handle's live object_to_world (debug read 7)"""
    o2w = inst.object_to_world()
    assert o2w.shape[0] == len(mesh_of)
    parts = [np.asarray(static, f32).reshape(-1, 18)]
    for m, mesh in zip(o2w, mesh_of):
        if mesh_lights[mesh] is not None and len(mesh_lights[mesh]):
            parts.append(cr.instance_lights(m, mesh_lights[mesh]))
    return cr.lights_finish(np.concatenate(parts))


def render(sc, frames=RVS, sync=True):
    for rx, ry in frames:
        sc.render_frame(rx, ry, sync=sync)


# ---------------------------------------------------------------- G1 ----

def static_light():
    """a light without geometry: a small quad under the Cornell box's ceiling, facing down"""
    p, u, v = np.array([0.6, 5.2, 0.7]), np.array([0.0, 0.0, 0.5]), np.array([0.7, 0.0, 0.0])
    return np.concatenate([p, u, v, (0, -1, 0), (1.5, 1.2, 0.9), (0.35, 0.123, 0)]).astype(f32)[None]


def unequal_lamp_lights(mesh):
    """the Cornell box's two lights with the first shrunk to 0.37 of its edges, so that the two areas (and pdfs) differ clearly: the
    light's area cancels in an emitter hit's pdf only algebraically, so a wrong index INSIDE the mesh changes the rounding, which a
    bit-for-bit comparison sees"""
    l = mesh.lights.copy()
    l[0, 3:9] = (l[0, 3:9] * f32(0.37)).astype(f32)
    l[0, 15] = np.linalg.norm(np.cross(l[0, 3:6].astype(np.float64), l[0, 6:9].astype(np.float64)))
    assert l[0, 15] < 0.2 * l[1, 15]
    return l


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [1, 2])
def test_identity_instances_with_mesh_lights_render_the_flat_oracles_frames(cr, ob, cornell, copies):
    """G1: the Cornell box split into 4 meshes, the lamp's mesh last and carrying the box's two lights, plus one static light, so that
    first[] != 0: sums and ray counters of the flat oracle on the unsplit scene given the finished table and emission.w patched to the
    table index.  The mesh's two lights have clearly different areas and the lamp's material names the SECOND (mesh-local 1), so the
    index inside the mesh is pinned too: first[inst] alone, or a clamp to 0, would read the other area and round differently.  copies = 2: a second instance of the lamp's mesh under a material offset, so that each copy has its own material in the
    flat scene (the copies coincide: whichever wins a tie, its light has the other's area and pdf)."""
    mesh, cam = cornell
    meshes, _ = split_mesh(cr, mesh, 4)
    assert (meshes[3].triangles[:, 3] == 1).sum() == 2 and all((m.triangles[:, 3] != 1).all() for m in meshes[:3])
    st = static_light()
    nm = mesh.materials.shape[0]
    lamp = unequal_lamp_lights(mesh)
    mats = np.concatenate([mesh.materials] * copies)                 # instanced: emission.w is mesh-local (1) in every copy
    mats[1::nm, 7] = 1
    mesh_of = [0, 1, 2, 3] + [3] * (copies - 1)
    offsets = [0, 0, 0, 0] + [nm * k for k in range(1, copies)]
    table = cr.lights_finish(np.concatenate([st] + [lamp] * copies))
    # the flat scene: the lamp mesh's triangles once per copy, copy k on materials [k nm, (k + 1) nm) whose lamp names table index 2 + 2 k
    flat_mats = mats.copy()
    tris = [mesh.triangles]
    for k in range(copies):
        flat_mats[k * nm + 1, 7] = 2 + 2 * k
        if k:
            t = meshes[3].triangles.copy()
            t[:, 3] += k * nm
            tris.append(t)
    flat = cr.Mesh(mesh.vertices, mesh.normals, mesh.texcoords, np.concatenate(tris), flat_mats, table, mesh.vertex_min)
    data = cr.SceneData.build(flat, cam)
    inst = cr.InstancedScene(meshes, cr.instances_array([IDENTITY] * len(mesh_of), mesh_of, material_offsets=offsets), builder="sah")
    for W, H in ((67, 45), (231, 130)):
        for depth in (1, 3, 4):
            o = ob.Oracle(data, W, H, depth)
            ref = np.zeros((H, W, 3), f32)
            for rx, ry in RVS[:3]:
                _, cnt = o.render_frame(rx, ry, ref, accel=ob.BVH8, tie=ob.TIE_LOWEST_ID, threads=THREADS)
            sc = inst.frame_scene(shading_of(meshes), mats, st, W, H, depth, mesh_lights=[None, None, None, lamp])
            sc.update(cam)
            assert np.array_equal(bits(cr.read_lights(sc)), bits(table))
            render(sc, RVS[:3])
            got = sc.read_sum()
            bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(-1))
            assert bad[0].size == 0, (copies, W, H, depth, bad[0].size, got[bad][:3], ref[bad][:3])
            fs = sc.frame_stats()
            assert (fs["closest_rays"], fs["any_rays"]) == (cnt[0], cnt[1]), (fs["closest_rays"], fs["any_rays"], cnt)
            assert fs["stack_overflows"] == 0
            sc.close()
    inst.close()


# ---------------------------------------------------------------- G2 ----

def quad_mesh(cr, mats, size):
    v = np.array([[-size, 0, -size], [-size, 0, size], [size, 0, size], [size, 0, -size]], f32)
    t = np.array([[0, 1, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 2, 3, 0, 0, 0, 0, 1, 0, 0, 0, 0]], np.int32)
    return cr.Mesh(v, np.array([[0, 1, 0]], f32), np.zeros((0, 2), f32), t, mats, np.zeros((0, 18), f32))


def g2_instances(rng, n):
    M, mesh_of = placed_instances(rng, n, 3, spread=9.0)
    if n >= 12:
        mesh_of[:6] = (0, 1, 2, 2, 1, 0)
        M[1], M[2] = IDENTITY, IDENTITY                              # bitwise identities on light-bearing meshes
        for k in (3, 4):                                             # translated identities
            M[k] = IDENTITY
            M[k, :, 3] = rng.uniform(-5, 5, 3)
        M[6, :, 0] *= -1                                             # mirrors, whatever the random signs gave
        M[7, :, 1] *= -1
        mesh_of[6:8] = (1, 2)
    return M, mesh_of


@pytest.mark.gpu
def test_the_light_table_under_general_transforms(cr):
    """G2: meshes with 0, 2 and 5 lights, 120 instances (bitwise identities, translated identities, mirrors), one static light:
    crt_scene_read_lights equals the host functions applied to the live matrices (debug read 7), and again after a refit, a device-form
    refit, a set to 260 instances, a set to 0 instances (the static light alone) and crt_scene_set_mesh_lights"""
    import torch
    rng = np.random.default_rng(1802)
    mats = np.zeros((1, 16), f32)
    mats[0, :3], mats[0, 7], mats[0, 12:16] = 0.7, -1, -1
    meshes = [quad_mesh(cr, mats, s) for s in (1.0, 0.7, 1.3)]
    ml = [None, random_lights(rng, 2), random_lights(rng, 5)]
    st = random_lights(rng, 1)
    M, mesh_of = g2_instances(rng, 120)
    inst = cr.InstancedScene(meshes, cr.instances_array(M, mesh_of), capacity=300)
    sc = inst.frame_scene(shading_of(meshes), mats, st, 32, 32, 2, mesh_lights=ml)

    def check(M, mesh_of, what):
        assert np.array_equal(bits(inst.object_to_world()), bits(np.asarray(M, f32).reshape(-1, 12))), what
        want = expected_table(cr, inst, st, ml, mesh_of)
        got = cr.read_lights(sc)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.nonzero((bits(got) != bits(want)).any(1))[0]
        assert bad.size == 0, (what, bad[:4], got[bad[:2]], want[bad[:2]])
        assert want.shape[0] == 1 + sum(len(ml[m]) if ml[m] is not None else 0 for m in mesh_of)
        return got

    got = check(M, mesh_of, "create")
    assert np.array_equal(bits(got[0, :16]), bits(st[0, :16])) and got[0, 17] == st[0, 17]      # a static light as given, its pdf recomputed
    assert np.array_equal(bits(got[1:3]), bits(cr.lights_finish(got)[1:3]))
    assert np.array_equal(bits(got[1:3, :16]), bits(ml[1][:, :16]))                              # instance 1: a bitwise identity copies area and all
    M2 = M.copy()
    M2[:, :, 3] += rng.uniform(-1.5, 1.5, (120, 3)).astype(f32)
    mesh_of2 = mesh_of.copy()
    mesh_of2[10:20] = (mesh_of2[10:20] + 1) % 3                                                  # a refit may change meshes: the total changes
    inst.refit(cr.instances_array(M2, mesh_of2))
    check(M2, mesh_of2, "refit")
    M3 = M2.copy()
    M3[:, :, :3] = (M3[:, :, :3] * f32(1.25)).astype(f32)
    rec = cr.instances_array(M3, mesh_of2)
    d = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    inst.refit_device(d.data_ptr(), 120)
    check(M3, mesh_of2, "refit_device")
    M4, mesh_of4 = g2_instances(rng, 260)
    inst.set(cr.instances_array(M4, mesh_of4))
    check(M4, mesh_of4, "set 260")
    inst.set(cr.instances_array(np.zeros((0, 12), f32), np.zeros(0, np.uint32)))
    got = check(np.zeros((0, 12), f32), np.zeros(0, np.int64), "set 0")
    assert got.shape[0] == 1 and got[0, 16] == 1.0
    inst.set(cr.instances_array(M, mesh_of))
    check(M, mesh_of, "set back")
    ml[2] = random_lights(rng, 5)
    cr.set_mesh_lights(sc, 2, ml[2])
    check(M, mesh_of, "set_mesh_lights")
    # a refused set leaves the table as it is
    bad = M.copy()
    bad[5, :, :3] = 0
    with pytest.raises(cr.CrtError):
        inst.set(cr.instances_array(bad, mesh_of))
    check(M, mesh_of, "refused set")
    close(inst, sc)


# ---------------------------------------------------------------- G3 ----

@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3, 4])
def test_the_lamp_moves(cr, ob, depth):
    """G3: the scene of CPU test 3 as an instanced scene whose lamp carries its lights (no static light): 8 frames at pose Q1 against
    the flat oracle, the lamp refitted to Q2, crt_reset, 8 frames against the oracle at Q2, within the bounds of the reference alone.
    Measured on an MI355X: 0 pixels beyond the bound at both poses and every depth, mean differences 0 to 8.0e-8.
    What a failure that is NOT an error of the table would look like: the bounds come from three seeds of the perturbation experiment
    (DESIGN.md §18); other seeds, which push the light's sample points a few ulps behind the lamp's own quad, left the reference alone
    up to 156 pixels and 6.2e-4 apart at Q2, all of them receivers that see the lamp at a grazing angle and lose single shadow rays to
    the lamp itself.  A change of rounding in the transform could in principle do the same on the GPU: the pixels beyond the bound would
    then be such receivers (dark by one light sample, scattered over the floor and box sides far from the lamp), while a table that
    stayed behind or a wrong transform moves whole shadows and changes thousands of pixels (the two poses differ in over 10,000)."""
    meshes, M, mats, obj, cam = lamp_scene(cr)
    inst = cr.InstancedScene(meshes, cr.instances_array(M, np.arange(5)))
    sc = inst.frame_scene(shading_of(meshes), mats, np.zeros((0, 18), f32), W6, H6, depth, mesh_lights=[None] * 4 + [obj])
    sc.update(crt_cam(cam))
    for name, pose in (("Q1", Q1), ("Q2", Q2)):
        if name == "Q2":
            M = M.copy()
            M[4] = Q2.astype(f32)
            inst.refit(cr.instances_array(M, np.arange(5)))
            sc.reset()
        render(sc)
        got = sc.read_sum()
        want = lamp_oracle_sum(ob, flatten(meshes, M, mats, obj), cam, depth, key=name)
        pixels, mean = compare_sums(want, got)
        print("GPU against the flat oracle, pose", name, "depth", depth, "pixels beyond", pixels, "mean diff %.2e" % mean)
        assert sc.frame_stats()["stack_overflows"] == 0
        assert pixels <= PIXEL_CAP and mean <= MEAN_RTOL_LAMP, (name, depth, pixels, mean)
    close(inst, sc)


# ---------------------------------------------------------------- G4 ----

@pytest.mark.gpu
def test_clamp_and_refusals(cr, cornell):
    """G4: an emission.w that a material offset lands beyond its mesh's lights is clamped (the same bits as the scene with nl - 1
    written there); what create, crt_scene_set_mesh_lights and crt_scene_read_lights refuse, each leaving the sum untouched; and
    mesh_lights == NULL (or every entry empty) renders crt_scene_create_instanced's bytes"""
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    mesh, cam = cornell
    meshes, _ = split_mesh(cr, mesh, 4)
    W, H, depth = 67, 45, 3
    nm = mesh.materials.shape[0]
    st = np.concatenate([static_light()] * 4)
    st[:, 0] += np.arange(4) * 0.1
    ml = [None, None, None, unequal_lamp_lights(mesh)]              # two areas: light 0 and light 1 of the mesh round differently
    sh = shading_of(meshes)
    # the lamp's mesh (2 lights) moved onto materials [nm, 2 nm): its lamp material names light 3 (< n_static = 4, so create admits it)
    inst = cr.InstancedScene(meshes, cr.instances_array([IDENTITY] * 4, np.arange(4), material_offsets=[0, 0, 0, nm]), builder="sah")
    sums = {}
    for ew in (3, 1, 0):
        mats = np.concatenate([mesh.materials, mesh.materials])
        mats[nm + 1, 7] = ew
        sc = inst.frame_scene(sh, mats, st, W, H, depth, mesh_lights=ml)
        sc.update(cam)
        render(sc, RVS[:3])
        sums[ew] = sc.read_sum()
        assert sc.frame_stats()["stack_overflows"] == 0
        sc.close()
    assert np.array_equal(bits(sums[3]), bits(sums[1]))
    assert not np.array_equal(bits(sums[3]), bits(sums[0]))          # the clamp lands on nl - 1, not on 0: the other light's area rounds differently
    assert (sums[3].max(-1) > 5.0).sum() > 20                        # the lamp is in the picture: emitter hits took the clamped branch
    # create refuses what it can see; nothing is bound by a refused create
    mats = np.concatenate([mesh.materials, mesh.materials])

    def refused(mats_, st_, ml_):
        with pytest.raises(cr.CrtError) as e:
            inst.frame_scene(sh, mats_, st_, W, H, depth, mesh_lights=ml_)
        assert e.value.code == _lib.CRT_ERR_INVALID

    m = mats.copy(); m[1, 7] = 2                                       # a triangle of the light-bearing mesh, own material, ew >= nl
    refused(m, st, ml)
    m = mats.copy(); m[3, 4:8] = (1, 1, 1, 1)                          # a triangle of a light-less mesh, ew >= n_static
    refused(m, st[:1], ml)
    m = mats.copy(); m[nm + 4, 4:8] = (1, 1, 1, 4)                     # any emissive material with ew >= max(n_static, max nl) ...
    refused(m, st, ml)
    m = mats.copy(); m[nm + 4, 4:8] = (1, 1, 1, -2)                    # ... or ew < 0
    refused(m, st, ml)
    for bad in (np.inf, np.nan):                                       # a non-finite light field, static or mesh
        s2 = st.copy(); s2[2, 5] = bad
        refused(mats, s2, ml)
        l2 = mesh.lights.copy(); l2[1, 15] = bad
        refused(mats, st, [None, None, None, l2])
    # the scene-side refusals leave the sum untouched
    sc = inst.frame_scene(sh, mats, st, W, H, depth, mesh_lights=ml)
    sc.update(cam)
    render(sc, RVS[:2])
    before = sc.read_sum()
    table = cr.read_lights(sc)
    n = C.c_size_t()
    two = mesh.lights.copy()
    nf = two.copy(); nf[0, 1] = np.nan
    small = np.zeros((2, 18), f32)
    calls = [lambda: L.crt_scene_set_mesh_lights(sc._h, 4, _ptr(two), 2),            # a wrong mesh
             lambda: L.crt_scene_set_mesh_lights(sc._h, 3, _ptr(two), 1),            # a wrong count
             lambda: L.crt_scene_set_mesh_lights(sc._h, 0, _ptr(two), 2),            # a mesh without lights takes none
             lambda: L.crt_scene_set_mesh_lights(sc._h, 3, None, 2),
             lambda: L.crt_scene_set_mesh_lights(sc._h, 3, _ptr(nf), 2),             # a field that is not finite
             lambda: L.crt_scene_read_lights(sc._h, _ptr(small), 2, C.byref(n))]     # a destination too small
    for k, call in enumerate(calls):
        assert call() == _lib.CRT_ERR_INVALID, k
        assert len(L.crt_last_error()) > 20, k
    assert n.value == 6
    assert np.array_equal(bits(cr.read_lights(sc)), bits(table))
    assert np.array_equal(bits(sc.read_sum()), bits(before))
    sc.reset()
    render(sc, RVS[:2])
    assert np.array_equal(bits(sc.read_sum()), bits(before))
    sc.close()
    # flat scenes, and instanced scenes without mesh lights
    flat = cr.Scene(cr.SceneData.build(mesh, cam), W, H, depth)
    assert L.crt_scene_set_mesh_lights(flat._h, 0, _ptr(two), 2) == _lib.CRT_ERR_INVALID
    assert L.crt_scene_read_lights(flat._h, None, 0, C.byref(n)) == _lib.CRT_ERR_INVALID
    flat.close()
    inst.close()
    # mesh_lights == NULL, and a list of empty entries: crt_scene_create_instanced's bytes
    inst = cr.InstancedScene(meshes, cr.instances_array([IDENTITY] * 4, np.arange(4)), builder="sah")
    sums = []
    for arg in ("plain", None, [None] * 4):
        sc = inst.frame_scene(sh, mesh.materials, mesh.lights, W, H, depth) if arg == "plain" else \
            inst.frame_scene(sh, mesh.materials, mesh.lights, W, H, depth, mesh_lights=arg)
        sc.update(cam)
        render(sc, RVS[:3])
        sums.append(sc.read_sum())
        assert L.crt_scene_set_mesh_lights(sc._h, 3, _ptr(two), 2) == _lib.CRT_ERR_INVALID
        assert np.array_equal(bits(cr.read_lights(sc)), bits(mesh.lights))     # without mesh lights: desc->lights as given
        sc.close()
    assert np.array_equal(bits(sums[0]), bits(sums[1])) and np.array_equal(bits(sums[0]), bits(sums[2]))
    assert sums[0].any()
    inst.close()


# ---------------------------------------------------------------- G5 ----

@pytest.mark.gpu
def test_async_frames_and_shards(cr):
    """G5: a refit behind frames queued with _async, then more frames: the sum of the same calls made synchronously; and two
    crt_set_shard ranks of the moved lamp's scene add up to the one-rank sum"""
    from caitlynrenderer_amd import tiles
    meshes, M, mats, obj, cam = lamp_scene(cr)
    M2 = M.copy()
    M2[4] = Q2.astype(f32)
    none = np.zeros((0, 18), f32)
    ml = [None] * 4 + [obj]
    W, H, depth = 96, 64, 3
    sums = []
    for sync in (True, False):
        inst = cr.InstancedScene(meshes, cr.instances_array(M, np.arange(5)))
        sc = inst.frame_scene(shading_of(meshes), mats, none, W, H, depth, mesh_lights=ml)
        sc.update(crt_cam(cam))
        render(sc, RVS[:3], sync=sync)
        inst.refit(cr.instances_array(M2, np.arange(5)))            # no crt_reset: both poses add into the one sum
        render(sc, RVS[3:6], sync=sync)
        sums.append(sc.read_sum())
        close(inst, sc)
    assert np.array_equal(bits(sums[0]), bits(sums[1]))
    # the frames behind the refit saw the moved lamp: not the sum of six frames at Q1
    inst = cr.InstancedScene(meshes, cr.instances_array(M, np.arange(5)))
    sc = inst.frame_scene(shading_of(meshes), mats, none, W, H, depth, mesh_lights=ml)
    sc.update(crt_cam(cam))
    render(sc, RVS[:6])
    assert (np.abs(sc.read_sum() - sums[0]).max(-1) > 1e-3).sum() > 500
    close(inst, sc)
    # shards, after a refit that each rank's scene has to notice
    frame = np.zeros((H, W, 3), f32)
    for rank in (None, 0, 1):
        inst = cr.InstancedScene(meshes, cr.instances_array(M, np.arange(5)))
        sc = inst.frame_scene(shading_of(meshes), mats, none, W, H, depth, mesh_lights=ml)
        sc.update(crt_cam(cam))
        if rank is not None:
            sc.set_shard(rank, 2, 16)
        render(sc, RVS[:1])
        inst.refit(cr.instances_array(M2, np.arange(5)))
        sc.reset()
        render(sc, RVS[:3])
        if rank is None:
            whole = sc.read_sum()
        else:
            n_tiles, tile, _ = sc.packed_info()
            tl = tiles.shard_tiles_of_library(W, H, 16, rank, 2)
            part = np.zeros((H, W, 3), f32)
            tiles.untile_into(part, sc.read_packed(), tl, 16)
            assert np.array_equal(bits(part), bits(sc.read_sum()))
            frame += part
        close(inst, sc)
    assert np.array_equal(bits(frame), bits(whole)) and whole.any()
