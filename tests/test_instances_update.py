"""Moving the meshes of an instanced scene (include/crt.h crt_instances_update_meshes*): the entry points and their refusals
without a GPU; on the GPU the refitted BLASes against the host crt_cwbvh_refit byte for byte, the records against numpy, hits against a
fresh create from the moved vertices and against the numpy brute force, an animation, refused updates with the state kept, the device form,
the 1 M-triangle mesh, and sets and updates interleaved.  The helpers of tests/test_instances.py are restated here."""
import ctypes as C

import numpy as np
import pytest

from conftest import numpy_brute_force

f32 = np.float32
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


def no_negative_zero(v):
    """x + 0 turns -0 into +0 and keeps every other float: the update's mesh box orders -0 below +0, create keeps the first of equal zeros"""
    return (np.asarray(v, f32) + f32(0.0)).astype(f32)


def displaced(v, amp, seed):
    rng = np.random.default_rng(seed)
    return no_negative_zero(np.asarray(v, f32) + (amp * rng.standard_normal(np.shape(v))).astype(f32))


def referenced_box(v, tris):
    p = np.asarray(v, f32)[np.asarray(tris)[:, :3].reshape(-1)]
    return np.concatenate([p.min(0), p.max(0)]).astype(f32)


def with_vertices(cr, mesh, v):
    return cr.Mesh(np.ascontiguousarray(v, f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials, mesh.lights)


def assert_same_closest(a, b):
    (ga, ia), (gb, ib) = a, b
    assert np.array_equal(ga["tri"], gb["tri"]), np.nonzero(ga["tri"] != gb["tri"])[0][:10]
    assert np.array_equal(ia, ib)
    h = ga["tri"] >= 0
    for f in ("t", "u", "v"):
        assert np.array_equal(ga[f][h].view(np.uint32), gb[f][h].view(np.uint32)), f


def snapshot(sc, rays):
    """everything the walk reads that a refused update must leave: hits + stats, BLAS nodes and records, TLAS, instance records, boxes"""
    h, i, s = sc.trace(rays, stats=True)
    return [h.view(np.uint8), i, s.view(np.uint8), sc.blas_nodes(), sc.blas_records().view(np.uint8), sc.tlas_nodes(),
            sc.instance_records().view(np.uint8), sc.world_boxes().view(np.uint8), sc.world_to_object().view(np.uint8)]


def assert_snapshot_equal(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k


# ---------------------------------------------------------------- CPU ----

NEW_SYMBOLS = ("crt_instances_update_meshes", "crt_instances_update_meshes_device", "crt_instances_last_update")


def test_entry_points_are_exported_and_bound(cr):
    from caitlynrenderer_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    assert _lib.CRT_INSTANCES_UPDATABLE == 1 << 16
    for m in ("update_meshes", "update_mesh", "update_meshes_device", "last_update", "blas_nodes", "blas_records"):
        assert callable(getattr(cr.InstancedScene, m)), m


def test_null_handle_is_invalid(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    v = np.zeros((3, 3), f32)
    ids = np.zeros(1, np.uint32)
    counts = np.array([3], np.uint64)
    ptrs = (C.c_void_p * 1)(v.ctypes.data)
    assert L.crt_instances_update_meshes(None, ids.ctypes.data, 1, ptrs, counts.ctypes.data) == _lib.CRT_ERR_INVALID
    assert L.crt_instances_update_meshes_device(None, ids.ctypes.data, 1, ptrs, counts.ctypes.data, 1) == _lib.CRT_ERR_INVALID
    b = C.c_uint64(7)
    assert L.crt_instances_last_update(None, None, None, C.byref(b)) == _lib.CRT_ERR_INVALID
    assert b.value == 0


def test_updatable_create_fails_loudly_without_gpu(cr, cornell):
    from caitlynrenderer_amd import _lib
    if _lib.lib().crt_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    mesh, _ = cornell
    with pytest.raises(cr.CrtError) as e:
        cr.InstancedScene([mesh], cr.instances_array([IDENTITY], [0]), updatable=True)
    assert e.value.code == _lib.CRT_ERR_NO_DEVICE


# ---------------------------------------------------------------- GPU ----

@pytest.fixture(scope="module")
def meshes3(cr, cornell, tess8, tess40):
    return [with_vertices(cr, m, no_negative_zero(m.vertices)) for m in (cornell[0], tess8[0], tess40[0])]


def blas_layout(sc, meshes):
    """per mesh: (first node8 in the BLAS region, node8 count, BLAS root as a global node index, first record)"""
    root_of = {}
    inst = sc.instance_records()[:, 12:16].view(np.uint32)
    info = sc.info()
    tlas_cap = info["tlas_bytes"] // 80
    roots = np.array(sorted(set(int(r) for r in inst[:, 0])), np.int64)
    assert len(roots) == len(meshes), "every mesh needs an instance for the layout"
    ends = list(roots[1:] - tlas_cap) + [int(info["blas_nodes8"])]
    tri_off = np.concatenate([[0], np.cumsum([m.triangles.shape[0] for m in meshes])])
    for k in range(len(meshes)):              # BLASes are packed in mesh order
        root_of[k] = (int(roots[k] - tlas_cap), int(ends[k] - (roots[k] - tlas_cap)), int(roots[k]), int(tri_off[k]))
    return root_of


def unrebased(nodes, root, tri_off):
    out = np.ascontiguousarray(nodes).copy()
    w = out.view(np.uint32).reshape(-1, 20)
    w[:, 4] -= np.uint32(root)
    w[:, 5] -= np.uint32(tri_off)
    return out


def host_refit(cr, nodes, recs, mesh, v):
    """crt_cwbvh_refit of one un-rebased BLAS: leaf-order triangles rebuilt from the records' (slot, id)"""
    from caitlynrenderer_amd import _lib
    nodes = np.ascontiguousarray(nodes).copy()
    ids = recs[:, 3].view(np.int32)
    slots = np.ascontiguousarray(recs[:, 7].view(np.int32))
    leaf = np.zeros((mesh.triangles.shape[0], 12), np.int32)
    leaf[slots] = mesh.triangles[ids]
    v = np.ascontiguousarray(v, f32)
    _lib.check(_lib.lib().crt_cwbvh_refit(nodes.ctypes.data, nodes.shape[0], slots.ctypes.data, slots.shape[0], leaf.ctypes.data,
                                          leaf.shape[0], v.ctypes.data, v.shape[0]))
    return nodes


def expected_records(old, mesh, v):
    t = mesh.triangles
    v = np.asarray(v, f32)
    out = old.copy()
    ids = old[:, 3].view(np.int32)
    p0, p1, p2 = v[t[ids, 0]], v[t[ids, 1]], v[t[ids, 2]]
    out[:, 0:3] = p0
    out[:, 4:7] = (p1 - p0).astype(f32)
    out[:, 8:11] = (p2 - p0).astype(f32)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "ploc", "lbvh"])
def test_refit_equals_the_host_refit_byte_for_byte(cr, meshes3, builder):
    rng = np.random.default_rng(3)
    M, _ = placed_instances(rng, 6, 3)
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, [0, 1, 2, 0, 1, 2]), builder=builder, updatable=True)
    lay = blas_layout(sc, meshes3)
    nodes0, recs0, w2o0 = sc.blas_nodes(), sc.blas_records(), sc.world_to_object()
    for step, upd in enumerate(({1: 0.05}, {0: 0.1, 2: 0.02})):
        new = {k: displaced(meshes3[k].vertices, a, 10 * step + k) for k, a in upd.items()}
        sc.update_meshes(new)
        nodes1, recs1 = sc.blas_nodes(), sc.blas_records()
        for k, m in enumerate(meshes3):
            n0, n8, root, to = lay[k]
            nt = m.triangles.shape[0]
            if k in new:
                want = host_refit(cr, unrebased(nodes0[n0:n0 + n8], root, to), recs0[to:to + nt], m, new[k])
                assert np.array_equal(unrebased(nodes1[n0:n0 + n8], root, to), want), (builder, k)
                assert np.array_equal(recs1[to:to + nt].view(np.uint32), expected_records(recs0[to:to + nt], m, new[k]).view(np.uint32))
            else:
                assert np.array_equal(nodes1[n0:n0 + n8], nodes0[n0:n0 + n8]), (builder, k)
                assert np.array_equal(recs1[to:to + nt].view(np.uint32), recs0[to:to + nt].view(np.uint32))
        assert np.array_equal(sc.world_to_object().view(np.uint32), w2o0.view(np.uint32))
        nodes0, recs0 = nodes1, recs1
    t = sc.last_update()
    assert t["device_ms"] > 0 and t["wall_ms"] > 0 and t["state_bytes"] > 0
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "ploc", "lbvh"])
def test_update_to_the_own_vertices(cr, meshes3, builder):
    rng = np.random.default_rng(5)
    M, mesh_of = placed_instances(rng, 40, 3)
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of), builder=builder, updatable=True)
    with pytest.raises(cr.CrtError):
        sc.last_update()                     # no update yet
    rays = world_rays(cr, rng, 8192, centres=M[:, :, 3])
    before = sc.trace(rays, stats=True)
    nodes0, tlas0 = sc.blas_nodes(), sc.tlas_nodes()
    sc.update_meshes({k: m.vertices for k, m in enumerate(meshes3)})
    after = sc.trace(rays, stats=True)
    assert_same_closest(before[:2], after[:2])
    same_blas = np.array_equal(sc.blas_nodes(), nodes0)
    print(f"{builder}: BLAS bytes after an update to the create's own vertices unchanged: {same_blas}")
    assert np.array_equal(sc.tlas_nodes(), tlas0)
    if same_blas:
        assert np.array_equal(after[2].view(np.uint8), before[2].view(np.uint8))
    if builder == "sah":
        assert same_blas
    sc.close()


@pytest.fixture(scope="module")
def placed300(cr, meshes3):
    rng = np.random.default_rng(21)
    M, mesh_of = placed_instances(rng, 300, 3)
    return M, mesh_of, rng


@pytest.mark.gpu
def test_update_against_a_fresh_create_and_brute_force(cr, meshes3, placed300):
    M, mesh_of, rng = placed300
    inst = cr.instances_array(M, mesh_of)
    sc = cr.InstancedScene(meshes3, inst, updatable=True)
    new = {0: displaced(meshes3[0].vertices, 0.08, 1), 2: displaced(meshes3[2].vertices, 0.03, 2)}
    sc.update_meshes(new)
    moved = [with_vertices(cr, m, new.get(k, m.vertices)) for k, m in enumerate(meshes3)]
    fresh = cr.InstancedScene(moved, inst)
    boxes = sc.world_boxes()
    for k, m in enumerate(M):
        want = cr.instance_world_box(m, referenced_box(moved[mesh_of[k]].vertices, moved[mesh_of[k]].triangles))
        assert np.array_equal(boxes[k].view(np.uint32), want.view(np.uint32)), k
    assert np.array_equal(boxes.view(np.uint32), fresh.world_boxes().view(np.uint32))
    rays = world_rays(cr, rng, 8192, centres=M[:, :, 3])
    got = sc.trace(rays)
    assert (got[0]["tri"] >= 0).sum() > 2000
    assert_same_closest(got, fresh.trace(rays))
    ga, ia = sc.trace(rays, cr.CRT_TRACE_ANY)
    fa, _ = fresh.trace(rays, cr.CRT_TRACE_ANY)
    assert np.array_equal(ga["tri"] >= 0, fa["tri"] >= 0) and np.array_equal(ia >= 0, fa["tri"] >= 0)
    # the numpy brute force per instance on the contract's object rays, reduced by (t, instance, id)
    w2o = sc.world_to_object()
    sub = rays[:48]
    T = np.full((len(M), sub.shape[0]), np.inf)
    TRI = np.full((len(M), sub.shape[0]), -1)
    for k in range(len(M)):
        tri, t, u, v = numpy_brute_force(moved[mesh_of[k]], object_rays(sub, w2o[k], is_identity(M[k])))
        T[k] = np.where(tri >= 0, t.astype(np.float64), np.inf)
        TRI[k] = tri
    best = np.argmin(T, axis=0)
    hit = np.isfinite(T[best, np.arange(sub.shape[0])])
    assert np.array_equal(got[1][:48], np.where(hit, best, -1))
    assert np.array_equal(got[0]["tri"][:48], np.where(hit, TRI[best, np.arange(sub.shape[0])], -1))
    assert np.array_equal(got[0]["t"][:48][hit].view(np.uint32), T[best, np.arange(sub.shape[0])][hit].astype(f32).view(np.uint32))
    # any hit: the reported instance has a hit of its own
    occ = ga["tri"][:48] >= 0
    assert np.isfinite(T[ia[:48][occ], np.nonzero(occ)[0]]).all()
    assert sc.info()["stack_overflows"] == 0
    sc.close(); fresh.close()


@pytest.mark.gpu
def test_animation_of_one_mesh_under_4096_instances(cr, meshes3):
    mesh = meshes3[1]
    rng = np.random.default_rng(33)
    M, _ = placed_instances(rng, 4096, 1, spread=60.0)
    inst = cr.instances_array(M, np.zeros(4096))
    sc = cr.InstancedScene([mesh], inst, updatable=True)
    rays = world_rays(cr, rng, 4096, spread=64.0, centres=M[:, :, 3])
    first = sc.trace(rays, stats=True)
    for step in range(1, 9):
        v = displaced(mesh.vertices, 0.02 * step, 100 + step)
        sc.update_mesh(0, v)
        fresh = cr.InstancedScene([with_vertices(cr, mesh, v)], inst)
        got = sc.trace(rays)
        assert (got[0]["tri"] >= 0).sum() > 500
        assert_same_closest(got, fresh.trace(rays))
        assert np.array_equal(sc.world_boxes().view(np.uint32), fresh.world_boxes().view(np.uint32))
        fresh.close()
    sc.update_mesh(0, mesh.vertices)
    last = sc.trace(rays, stats=True)
    assert_same_closest(first[:2], last[:2])
    assert np.array_equal(last[2].view(np.uint8), first[2].view(np.uint8))
    sc.close()


@pytest.mark.gpu
def test_refused_updates_keep_the_state(cr, meshes3):
    from caitlynrenderer_amd import _lib
    rng = np.random.default_rng(8)
    M, mesh_of = placed_instances(rng, 60, 3)
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of), updatable=True)
    rays = world_rays(cr, rng, 4096, centres=M[:, :, 3])
    ok = displaced(meshes3[0].vertices, 0.05, 4)
    before = snapshot(sc, rays)

    def refused(fn, code=_lib.CRT_ERR_INVALID, words=None):
        with pytest.raises(cr.CrtError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        if words:
            assert words in str(e.value), str(e.value)
        assert_snapshot_equal(snapshot(sc, rays), before)

    for bad in (np.nan, np.inf, -np.inf, 1e19):
        v = meshes3[1].vertices.copy()
        v[len(v) // 2, 1] = bad
        refused(lambda: sc.update_meshes({0: ok, 1: v}), words="not finite")        # all or nothing: mesh 0 is not taken either
        refused(lambda: sc.update_mesh(1, v))
    refused(lambda: sc.update_mesh(0, ok[:-1]))                                     # wrong count
    refused(lambda: sc.update_mesh(3, ok))                                          # mesh out of range
    L = _lib.lib()
    ids = np.array([0, 0], np.uint32)                                               # repeated
    ptrs = (C.c_void_p * 2)(ok.ctypes.data, ok.ctypes.data)
    counts = np.array([len(ok), len(ok)], np.uint64)
    refused(lambda: _lib.check(L.crt_instances_update_meshes(sc._h, ids.ctypes.data, 2, ptrs, counts.ctypes.data)), words="repeated")
    one = np.array([0], np.uint32)
    nullp = (C.c_void_p * 1)(None)
    refused(lambda: _lib.check(L.crt_instances_update_meshes(sc._h, one.ctypes.data, 1, nullp, counts.ctypes.data)))
    refused(lambda: _lib.check(L.crt_instances_update_meshes(sc._h, None, 1, ptrs, counts.ctypes.data)))
    sc.close()
    # a world box beyond 1e18: coordinates within the bound that instances scaled by 2 carry past it
    G = np.zeros((8, 3, 4), f32)
    G[:, :, :3] = np.eye(3, dtype=f32) * f32(2.0)
    G[:, 0, 3] = (np.arange(8) * f32(15.0)).astype(f32)
    m0 = meshes3[0]
    assert 4.0 < np.abs(m0.vertices).max() < 6.0
    huge = cr.InstancedScene([m0], cr.instances_array(G, np.zeros(8)), updatable=True)
    grays = world_rays(cr, rng, 1024, spread=60.0, centres=G[:, :, 3])
    sc, rays = huge, grays
    before = snapshot(sc, rays)
    refused(lambda: sc.update_mesh(0, no_negative_zero(m0.vertices * f32(1.5e17))), words="1e18")
    sc.update_mesh(0, displaced(m0.vertices, 0.01, 5))                              # the state still takes an update
    sc.close()
    plain = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of))
    with pytest.raises(cr.CrtError) as e:
        plain.update_mesh(0, ok)
    assert e.value.code == _lib.CRT_ERR_INVALID and "CRT_INSTANCES_UPDATABLE" in str(e.value)
    with pytest.raises(cr.CrtError):
        plain.last_update()
    plain.close()


@pytest.mark.gpu
def test_device_form_equals_the_host_form(cr, meshes3, placed300):
    import torch
    M, mesh_of, rng = placed300
    inst = cr.instances_array(M[:100], mesh_of[:100])
    a = cr.InstancedScene(meshes3, inst, updatable=True)
    b = cr.InstancedScene(meshes3, inst, updatable=True)
    new = {1: displaced(meshes3[1].vertices, 0.06, 11), 2: displaced(meshes3[2].vertices, 0.04, 12)}
    a.update_meshes(new)
    d = {k: torch.from_numpy(v).cuda() for k, v in new.items()}
    torch.cuda.synchronize()
    b.update_meshes_device({k: (t.data_ptr(), t.shape[0]) for k, t in d.items()})
    rays = world_rays(cr, rng, 4096, centres=M[:100, :, 3])
    ha, hb = a.trace(rays, stats=True), b.trace(rays, stats=True)
    for x, y in zip(ha, hb):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for read in ("blas_nodes", "blas_records", "tlas_nodes", "instance_records", "world_boxes"):
        assert np.array_equal(getattr(a, read)().view(np.uint8), getattr(b, read)().view(np.uint8)), read
    a.close(); b.close()


@pytest.mark.gpu
def test_64_instances_of_the_million_triangle_mesh(cr, cornell):
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    base, _ = cornell
    mesh = tessellated_cornell(base, 183)
    mesh = with_vertices(cr, mesh, no_negative_zero(mesh.vertices))
    assert mesh.triangles.shape[0] == 1004672
    rng = np.random.default_rng(64)
    ext = float((mesh.vertices.max(0) - mesh.vertices.min(0)).max())
    M = []
    for gx in range(8):
        for gy in range(8):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            M.append(np.concatenate([q, np.array([[gx * 1.5 * ext], [gy * 1.5 * ext], [0.0]])], 1))
    M = np.array(M, f32)
    inst = cr.instances_array(M, np.zeros(64))
    sc = cr.InstancedScene([mesh], inst, updatable=True)
    v = displaced(mesh.vertices, 0.01 * ext, 7)
    sc.update_mesh(0, v)
    fresh = cr.InstancedScene([with_vertices(cr, mesh, v)], inst)
    rays = world_rays(cr, rng, 1 << 20, spread=6 * ext, centres=M[:, :, 3])
    rays["o"] += f32(5.25 * ext) * np.array([1, 1, 0], f32)
    got = sc.trace(rays)
    assert (got[0]["tri"] >= 0).sum() > 200000
    assert_same_closest(got, fresh.trace(rays))
    assert sc.info()["stack_overflows"] == 0
    sc.close(); fresh.close()


@pytest.mark.gpu
def test_sets_and_updates_interleaved(cr, meshes3, placed300):
    M, mesh_of, rng = placed300
    A = cr.instances_array(M[:120], mesh_of[:120])
    B = cr.instances_array(M[120:260], mesh_of[120:260])
    sc = cr.InstancedScene(meshes3, A, capacity=300, updatable=True)
    v1 = displaced(meshes3[1].vertices, 0.07, 21)
    v0 = displaced(meshes3[0].vertices, 0.05, 22)
    rays = world_rays(cr, rng, 4096, centres=M[:, :, 3])
    # set, then update: the update sees the newly set instances
    sc.set(B)
    sc.update_mesh(1, v1)
    moved = [meshes3[0], with_vertices(cr, meshes3[1], v1), meshes3[2]]
    fresh = cr.InstancedScene(moved, B)
    assert sc.info()["n_instances"] == 140
    assert_same_closest(sc.trace(rays), fresh.trace(rays))
    assert np.array_equal(sc.world_boxes().view(np.uint32), fresh.world_boxes().view(np.uint32))
    fresh.close()
    # update, then set: the set uses the new mesh boxes
    sc.update_mesh(0, v0)
    sc.set(A)
    moved[0] = with_vertices(cr, meshes3[0], v0)
    fresh = cr.InstancedScene(moved, A)
    assert_same_closest(sc.trace(rays), fresh.trace(rays))
    assert np.array_equal(sc.world_boxes().view(np.uint32), fresh.world_boxes().view(np.uint32))
    fresh.close()
    # an empty set, an update, then a set again
    sc.set(A[:0])
    sc.update_mesh(2, displaced(meshes3[2].vertices, 0.02, 23))
    assert (sc.trace(rays)[1] == -1).all()
    sc.set(B)
    assert sc.info()["n_instances"] == 140
    sc.close()
