"""Moving the instances of an instanced scene without a TLAS rebuild (include/crt.h crt_instances_refit*): the entry points
and their refusals without a GPU; on the GPU a refit to the live instances as a no-op, the refitted TLAS against the host crt_cwbvh_refit
byte for byte, an animation against a second handle set to the same instances and against the numpy brute force, refused refits with
the state kept, a refit after a set refused with CRT_ERR_LIMIT, refits interleaved with sets and mesh updates, the device form, and two
larger scenes.  The helpers of tests/test_instances*.py are restated here."""
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


def random_matrix(rng, spread, scale=(0.5, 2.0)):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    s = rng.uniform(*scale, 3) * rng.choice([-1.0, 1.0], 3)
    return np.concatenate([q @ np.diag(s), rng.uniform(-spread, spread, (3, 1))], 1)


def placed_instances(rng, n, n_meshes, spread=12.0, scale=(0.5, 2.0)):
    return np.array([random_matrix(rng, spread, scale) for _ in range(n)], f32), rng.integers(0, n_meshes, n)


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
    """x + 0 turns -0 into +0 and keeps every other float"""
    return (np.asarray(v, f32) + f32(0.0)).astype(f32)


def displaced(v, amp, seed):
    rng = np.random.default_rng(seed)
    return no_negative_zero(np.asarray(v, f32) + (amp * rng.standard_normal(np.shape(v))).astype(f32))


def with_vertices(cr, mesh, v):
    return cr.Mesh(np.ascontiguousarray(v, f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials, mesh.lights)


def assert_same_closest(a, b):
    (ga, ia), (gb, ib) = a[:2], b[:2]
    assert np.array_equal(ga["tri"], gb["tri"]), np.nonzero(ga["tri"] != gb["tri"])[0][:10]
    assert np.array_equal(ia, ib)
    h = ga["tri"] >= 0
    for f in ("t", "u", "v"):
        assert np.array_equal(ga[f][h].view(np.uint32), gb[f][h].view(np.uint32)), f


def snapshot(sc, rays):
    """everything a refit writes and the walk reads: hits, instance ids and stats, world_to_object, world boxes, TLAS, instance records"""
    h, i, s = sc.trace(rays, stats=True)
    return [h.view(np.uint8), i, s.view(np.uint8), sc.world_to_object().view(np.uint8), sc.world_boxes().view(np.uint8), sc.tlas_nodes(),
            sc.instance_records().view(np.uint8)]


def assert_snapshot_equal(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k


def leaf_instances(sc):
    """instance index of every TLAS leaf slot (row 3 .y of the instance records)"""
    return sc.instance_records()[:, 13].view(np.uint32).copy()


def records_by_instance(sc):
    rec = sc.instance_records()
    out = np.empty_like(rec)
    out[rec[:, 13].view(np.uint32)] = rec
    return out


def assert_same_instance_state(sc, ref, same_blas=True):
    """world_to_object, world boxes and the records (per instance: the two TLASes order their leaves differently) of two handles of the
    same capacity (a record's BLAS root is a node index in the one node array, where the TLAS region sized for the capacity comes first;
    same_blas=False: the BLASes differ in size, e.g. a refitted one against one built from the moved vertices, and the roots are skipped)"""
    assert np.array_equal(sc.world_to_object().view(np.uint32), ref.world_to_object().view(np.uint32))
    assert np.array_equal(sc.world_boxes().view(np.uint32), ref.world_boxes().view(np.uint32))
    a, b = records_by_instance(sc).view(np.uint32), records_by_instance(ref).view(np.uint32)
    if not same_blas:
        a, b = np.delete(a, 12, 1), np.delete(b, 12, 1)
    assert np.array_equal(a, b)


def tlas_shape(sc):
    i = sc.info()
    return i["tlas_nodes8"], i["tlas_depth8"], i["stack_entries"]


# ---------------------------------------------------------------- CPU ----

def test_entry_points_are_exported_and_bound(cr):
    from caitlynrenderer_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in ("crt_instances_refit", "crt_instances_refit_device"):
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    for m in ("refit", "refit_device"):
        assert callable(getattr(cr.InstancedScene, m)), m


def test_null_handle_is_invalid(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    inst = cr.instances_array([IDENTITY], [0])
    assert L.crt_instances_refit(None, inst.ctypes.data, 1) == _lib.CRT_ERR_INVALID
    assert L.crt_instances_refit(None, None, 0) == _lib.CRT_ERR_INVALID
    assert L.crt_instances_refit_device(None, inst.ctypes.data, 1, 1) == _lib.CRT_ERR_INVALID
    assert b"null" in L.crt_last_error()


def test_python_methods_refuse_loudly_without_a_handle(cr):
    from caitlynrenderer_amd import _lib
    sc = object.__new__(cr.InstancedScene)
    sc._h = C.c_void_p()
    inst = cr.instances_array([IDENTITY], [0])
    with pytest.raises(cr.CrtError) as e:
        sc.refit(inst)
    assert e.value.code == _lib.CRT_ERR_INVALID and "crt_instances_refit" in str(e.value)
    with pytest.raises(cr.CrtError) as e:
        sc.refit_device(inst.ctypes.data, 1)
    assert e.value.code == _lib.CRT_ERR_INVALID and "crt_instances_refit_device" in str(e.value)


# ---------------------------------------------------------------- GPU ----

@pytest.fixture(scope="module")
def meshes3(cr, cornell, tess8, tess40):
    return [with_vertices(cr, m, no_negative_zero(m.vertices)) for m in (cornell[0], tess8[0], tess40[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 300, 4096])
def test_refit_to_the_live_instances_is_a_no_op(cr, meshes3, n):
    rng = np.random.default_rng(40 + n)
    M, mesh_of = placed_instances(rng, n, 3, spread=12.0 * max(1.0, (n / 300) ** (1 / 3)))
    inst = cr.instances_array(M, mesh_of)
    sc = cr.InstancedScene(meshes3, inst)
    rays = world_rays(cr, rng, 4096, spread=20.0, centres=M[:, :, 3])
    before = snapshot(sc, rays)
    shape = tlas_shape(sc)
    for _ in range(2):                        # the first refit finds the TLAS's levels, the second reuses them
        sc.refit(inst)
        assert_snapshot_equal(snapshot(sc, rays), before)
        assert tlas_shape(sc) == shape
    i = sc.info()
    assert i["set_device_ms"] > 0 and i["set_wall_ms"] > 0 and i["stack_overflows"] == 0
    sc.close()


def host_tlas_refit(cr, nodes, order, boxes):
    """crt_cwbvh_refit of a TLAS: leaf slot k holds one triangle (lo, hi, lo) of the world box of the instance order[k]"""
    from caitlynrenderer_amd import _lib
    nodes = np.ascontiguousarray(nodes).copy()
    n = order.shape[0]
    b = np.asarray(boxes, f32)[order]
    verts = np.ascontiguousarray(np.stack([b[:, :3], b[:, 3:]], 1).reshape(-1, 3), f32)
    leaf = np.zeros((n, 12), np.int32)
    leaf[:, 0] = 2 * np.arange(n)
    leaf[:, 1] = 2 * np.arange(n) + 1
    leaf[:, 2] = 2 * np.arange(n)
    slots = np.arange(n, dtype=np.int32)
    _lib.check(_lib.lib().crt_cwbvh_refit(nodes.ctypes.data, nodes.shape[0], slots.ctypes.data, n, leaf.ctypes.data, n, verts.ctypes.data,
                                          verts.shape[0]))
    return nodes


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 300])
def test_refit_equals_the_host_refit_byte_for_byte(cr, meshes3, n):
    rng = np.random.default_rng(70 + n)
    X, mesh_x = placed_instances(rng, n, 3)
    Y, mesh_y = placed_instances(rng, n, 3, spread=16.0)
    Y[: n // 2] = X[: n // 2] + rng.normal(scale=0.3, size=(n // 2, 3, 4)).astype(f32)     # half of them moved a little
    mesh_y[: n // 3] = mesh_x[: n // 3]
    sc = cr.InstancedScene(meshes3, cr.instances_array(X, mesh_x))
    nodes_x, order = sc.tlas_nodes(), leaf_instances(sc)
    iy = cr.instances_array(Y, mesh_y)
    sc.refit(iy)
    fresh = cr.InstancedScene(meshes3, iy)
    boxes = fresh.world_boxes()
    assert np.array_equal(boxes.view(np.uint32), no_negative_zero(boxes).view(np.uint32)), "a -0 box face"
    assert np.array_equal(sc.tlas_nodes(), host_tlas_refit(cr, nodes_x, order, boxes))
    assert np.array_equal(leaf_instances(sc), order)          # every leaf slot keeps its instance
    assert_same_instance_state(sc, fresh)
    rays = world_rays(cr, rng, 4096, spread=20.0, centres=Y[:, :, 3])
    got = sc.trace(rays)
    assert (got[0]["tri"] >= 0).sum() > 500
    assert_same_closest(got, fresh.trace(rays))
    sc.close(); fresh.close()


def brute_force_closest(cr, meshes, M, mesh_of, w2o, rays):
    """the numpy brute force per instance on the contract's object rays, reduced by (t, instance, id) -> (instance, tri, t)"""
    T = np.full((len(M), rays.shape[0]), np.inf)
    TRI = np.full((len(M), rays.shape[0]), -1)
    for k in range(len(M)):
        tri, t, _, _ = numpy_brute_force(meshes[mesh_of[k]], object_rays(rays, w2o[k], is_identity(M[k])))
        T[k] = np.where(tri >= 0, t.astype(np.float64), np.inf)
        TRI[k] = tri
    best = np.argmin(T, axis=0)
    cols = np.arange(rays.shape[0])
    hit = np.isfinite(T[best, cols])
    return np.where(hit, best, -1), np.where(hit, TRI[best, cols], -1), T[best, cols], hit


@pytest.mark.gpu
def test_animation_of_300_instances(cr, meshes3):
    rng = np.random.default_rng(300)
    M, mesh_of = placed_instances(rng, 300, 3)
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of))
    ref = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of))
    shape = tlas_shape(sc)
    rays = world_rays(cr, rng, 8192, centres=M[:, :, 3])
    for step in range(20):
        if step < 6:                          # jitter
            M = (M + rng.normal(scale=0.02, size=M.shape)).astype(f32)
        elif step < 12:                       # drift: every instance translated, some rotated afresh
            M[:, :, 3] += rng.normal(scale=0.5, size=(300, 3)).astype(f32)
            for k in rng.choice(300, 30, replace=False):
                M[k] = random_matrix(rng, 12.0)
        elif step == 12:                      # a full reshuffle across the scene
            M = M[rng.permutation(300)]
        else:                                 # new placements everywhere
            M, _ = placed_instances(rng, 300, 3, spread=14.0)
        if step % 4 == 1:                     # some instances change mesh
            pick = rng.choice(300, 25, replace=False)
            mesh_of[pick] = (mesh_of[pick] + 1) % 3
        inst = cr.instances_array(M, mesh_of)
        sc.refit(inst)
        ref.set(inst)
        rays = world_rays(cr, rng, 8192, centres=M[:, :, 3])
        got = sc.trace(rays)
        assert (got[0]["tri"] >= 0).sum() > 1000, step
        assert_same_closest(got, ref.trace(rays))
        ga, ia = sc.trace(rays, cr.CRT_TRACE_ANY)
        fa, _ = ref.trace(rays, cr.CRT_TRACE_ANY)
        assert np.array_equal(ga["tri"] >= 0, fa["tri"] >= 0), step
        assert np.array_equal(ia >= 0, fa["tri"] >= 0), step
        assert_same_instance_state(sc, ref)
        if step in (0, 7, 12, 19):
            sub = rays[:24]
            inst_w, tri_w, t_w, hit = brute_force_closest(cr, meshes3, M, mesh_of, sc.world_to_object(), sub)
            assert np.array_equal(got[1][:24], inst_w), step
            assert np.array_equal(got[0]["tri"][:24], tri_w), step
            assert np.array_equal(got[0]["t"][:24][hit].view(np.uint32), t_w[hit].astype(f32).view(np.uint32)), step
        info = sc.info()
        assert info["stack_overflows"] == 0
        assert tlas_shape(sc) == shape, step
    sc.close(); ref.close()


@pytest.mark.gpu
def test_refused_refits_keep_the_state(cr, meshes3):
    from caitlynrenderer_amd import _lib
    import torch
    rng = np.random.default_rng(9)
    M, mesh_of = placed_instances(rng, 60, 3)
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of), capacity=80)
    rays = world_rays(cr, rng, 4096, centres=M[:, :, 3])
    sc.refit(cr.instances_array((M + f32(0.1)).astype(f32), mesh_of))      # the levels are known: the refused calls come after a refit
    before = snapshot(sc, rays)
    good = (M + rng.normal(scale=0.05, size=M.shape)).astype(f32)

    def refused(fn, words):
        with pytest.raises(cr.CrtError) as e:
            fn()
        assert e.value.code == _lib.CRT_ERR_INVALID, str(e.value)
        assert words in str(e.value), str(e.value)
        assert_snapshot_equal(snapshot(sc, rays), before)

    def one_bad(k, fn):
        G, m = good.copy(), mesh_of.copy()
        fn(G, m)
        return cr.instances_array(G, m)

    M61, m61 = placed_instances(rng, 61, 3)
    refused(lambda: sc.refit(cr.instances_array(M61, m61)), "live count")           # above the live count
    refused(lambda: sc.refit(cr.instances_array(good[:59], mesh_of[:59])), "live count")
    refused(lambda: sc.refit(cr.instances_array(good[:0], mesh_of[:0])), "live count")
    M90, m90 = placed_instances(rng, 90, 3)
    refused(lambda: sc.refit(cr.instances_array(M90, m90)), "live count")           # above the capacity
    for bad in (np.nan, np.inf, -np.inf):
        refused(lambda: sc.refit(one_bad(31, lambda G, m: G.__setitem__((31, 1, 2), bad))), "not finite")
        refused(lambda: sc.refit(one_bad(5, lambda G, m: G.__setitem__((5, 2, 3), bad))), "not finite")
    refused(lambda: sc.refit(one_bad(7, lambda G, m: G.__setitem__((7, 2, slice(0, 3)), 0.0))), "singular")
    refused(lambda: sc.refit(one_bad(8, lambda G, m: m.__setitem__(8, 3))), "mesh index")
    refused(lambda: sc.refit(one_bad(9, lambda G, m: G.__setitem__((9, slice(None), slice(0, 3)), np.eye(3) * 1e18))), "1e18")
    L = _lib.lib()
    refused(lambda: _lib.check(L.crt_instances_refit(sc._h, None, 60)), "null")
    refused(lambda: _lib.check(L.crt_instances_refit_device(sc._h, None, 60, 1)), "null")
    bad = torch.from_numpy(one_bad(3, lambda G, m: G.__setitem__((3, 0, 0), np.nan)).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    refused(lambda: sc.refit_device(bad.data_ptr(), 60), "not finite")
    refused(lambda: sc.refit_device(bad.data_ptr(), 61), "live count")
    # the state still takes a refit, which equals a set of the same instances
    inst = cr.instances_array(good, mesh_of)
    sc.refit(inst)
    fresh = cr.InstancedScene(meshes3, inst, capacity=80)
    assert_same_closest(sc.trace(rays), fresh.trace(rays))
    assert_same_instance_state(sc, fresh)
    sc.close(); fresh.close()


def clustered_mesh(K):
    """K clusters of 8 triangles, each cluster 4x smaller than the previous and beside it: a BLAS about K node8 levels deep"""
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
@pytest.mark.parametrize("refit_first", [False, True])
def test_refit_after_a_set_refused_with_limit(cr, refit_first):
    """a set refused with CRT_ERR_LIMIT has rebuilt the TLAS builder's buffers while the live TLAS is the previous one: the refit must
    follow the live TLAS, whether its levels were found before the refused set or after it"""
    from caitlynrenderer_amd import _lib
    V, T = clustered_mesh(30)
    M1 = clustered_instances(1)
    sc = cr.InstancedScene([(V, T)], cr.instances_array(M1, np.zeros(8)), capacity=8 * 48)
    db = sc.info()["max_blas_depth8"]
    rng = np.random.default_rng(4)
    rays = np.zeros(4096, cr.RAY_DT)
    rays["o"] = np.array([-1.0, 0.2, 0.05], f32) + rng.normal(scale=0.02, size=(4096, 3)).astype(f32)
    rays["o"][:, 0] = rng.uniform(0.0, 40.0, 4096).astype(f32)
    rays["o"][:, 2] = f32(5.0)
    rays["d"] = np.array([0.0, 0.0, -1.0], f32)
    rays["tmax"] = f32(1e9)
    if refit_first:
        sc.refit(cr.instances_array(M1, np.zeros(8)))
    deep = cr.instances_array(clustered_instances(48 - db), np.zeros(8 * (48 - db)))
    with pytest.raises(cr.CrtError) as e:
        sc.set(deep)
    assert e.value.code == _lib.CRT_ERR_LIMIT
    for step in range(2):
        M = M1.copy()
        M[:, 0, 3] += f32(1.5 * (step + 1))       # every instance slides along x, some in reverse order
        M[:, 1, 3] += rng.uniform(-0.2, 0.2, 8).astype(f32)
        M = M[::-1].copy() if step else M
        inst = cr.instances_array(M, np.zeros(8))
        sc.refit(inst)
        fresh = cr.InstancedScene([(V, T)], inst, capacity=8 * 48)
        got = sc.trace(rays)
        assert (got[1] >= 0).sum() > 100
        assert_same_closest(got, fresh.trace(rays))
        assert_same_instance_state(sc, fresh)
        assert sc.info()["n_instances"] == 8
        fresh.close()
    sc.close()


@pytest.mark.gpu
def test_refits_sets_and_updates_interleaved(cr, meshes3):
    rng = np.random.default_rng(77)
    M, mesh_of = placed_instances(rng, 300, 3)
    A = cr.instances_array(M[:120], mesh_of[:120])
    sc = cr.InstancedScene(meshes3, A, capacity=300, updatable=True)
    moved = list(meshes3)
    rays = world_rays(cr, rng, 4096, centres=M[:, :, 3])

    def check(inst):
        fresh = cr.InstancedScene(moved, inst, capacity=300)
        got = sc.trace(rays)
        assert (got[0]["tri"] >= 0).sum() > 500
        assert_same_closest(got, fresh.trace(rays))
        assert_same_instance_state(sc, fresh, same_blas=moved == list(meshes3))
        fresh.close()

    def jittered(inst, scale, seed):
        r = np.random.default_rng(seed)
        out = inst.copy()
        out["object_to_world"] = (out["object_to_world"] + r.normal(scale=scale, size=out["object_to_world"].shape)).astype(f32)
        return out

    B = cr.instances_array(M[120:260], mesh_of[120:260])
    sc.set(B)                                                        # set
    check(B)
    B1 = jittered(B, 0.3, 1)
    B1["mesh"][:20] = (B1["mesh"][:20] + 1) % 3
    sc.refit(B1)                                                     # refit
    check(B1)
    v1 = displaced(meshes3[1].vertices, 0.07, 2)
    sc.update_mesh(1, v1)                                            # update: starts from the refitted instances
    moved[1] = with_vertices(cr, meshes3[1], v1)
    check(B1)
    B2 = jittered(B1, 0.5, 3)
    sc.refit(B2)                                                     # refit after an update (new TLAS, new levels)
    check(B2)
    C3 = cr.instances_array(M[:200], mesh_of[:200])
    sc.set(C3)                                                       # a set with a new count
    check(C3)
    C4 = jittered(C3, 0.4, 4)
    sc.refit(C4)                                                     # refit of the new count
    check(C4)
    v0 = displaced(meshes3[0].vertices, 0.05, 5)
    sc.update_mesh(0, v0)
    moved[0] = with_vertices(cr, meshes3[0], v0)
    check(C4)
    sc.set(C4[:0])                                                   # an empty scene refits to nothing
    sc.refit(C4[:0])
    assert (sc.trace(rays)[1] == -1).all()
    sc.close()


@pytest.mark.gpu
def test_device_form_equals_the_host_form(cr, meshes3):
    import torch
    rng = np.random.default_rng(12)
    M, mesh_of = placed_instances(rng, 200, 3)
    inst = cr.instances_array(M, mesh_of)
    a, b, c = (cr.InstancedScene(meshes3, inst) for _ in range(3))
    M2 = (M + rng.normal(scale=0.4, size=M.shape)).astype(f32)
    new = cr.instances_array(M2, (mesh_of + 1) % 3)
    a.refit(new)
    d_new = torch.from_numpy(new.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    b.refit_device(d_new.data_ptr(), 200)
    c.refit_device(d_new.data_ptr(), 200, sync=False)
    rays = world_rays(cr, rng, 4096, centres=M2[:, :, 3])
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_ids.data_ptr(), sync=True)      # on the handle's stream, after the refit
    ha = a.trace(rays, stats=True)
    assert (ha[0]["tri"] >= 0).sum() > 500
    hb = b.trace(rays, stats=True)
    for x, y in zip(ha, hb):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(d_hits.cpu().numpy(), ha[0].view(np.uint8).reshape(-1))
    assert np.array_equal(d_ids.cpu().numpy(), ha[1])
    for sc in (b, c):
        for read in ("tlas_nodes", "instance_records", "world_boxes", "world_to_object"):
            assert np.array_equal(getattr(a, read)().view(np.uint8), getattr(sc, read)().view(np.uint8)), read
    a.close(); b.close(); c.close()


@pytest.mark.gpu
def test_one_mesh_under_4096_instances(cr, meshes3):
    mesh = meshes3[1]
    rng = np.random.default_rng(4096)
    M, _ = placed_instances(rng, 4096, 1, spread=60.0)
    sc = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(4096)))
    shape = tlas_shape(sc)
    for step in range(3):
        M = (M + rng.normal(scale=0.5 * (step + 1), size=M.shape)).astype(f32)
        inst = cr.instances_array(M, np.zeros(4096))
        sc.refit(inst)
        fresh = cr.InstancedScene([mesh], inst)
        rays = world_rays(cr, rng, 8192, spread=64.0, centres=M[:, :, 3])
        got = sc.trace(rays)
        assert (got[0]["tri"] >= 0).sum() > 1000
        assert_same_closest(got, fresh.trace(rays))
        assert_same_instance_state(sc, fresh)
        assert tlas_shape(sc) == shape and sc.info()["stack_overflows"] == 0
        fresh.close()
    sc.close()


@pytest.mark.gpu
def test_the_million_triangle_mesh_under_the_8x8_grid(cr, cornell):
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
    sc = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(64)))
    M2 = M.copy()
    for k in range(64):                       # each copy turned afresh and shifted by up to a third of its size
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        M2[k, :, :3] = q
    M2[:, :, 3] += rng.uniform(-ext / 3, ext / 3, (64, 3)).astype(f32)
    inst = cr.instances_array(M2, np.zeros(64))
    sc.refit(inst)
    fresh = cr.InstancedScene([mesh], inst)
    rays = world_rays(cr, rng, 1 << 20, spread=6 * ext, centres=M2[:, :, 3])
    rays["o"] += f32(5.25 * ext) * np.array([1, 1, 0], f32)
    got = sc.trace(rays)
    assert (got[0]["tri"] >= 0).sum() > 200000
    assert_same_closest(got, fresh.trace(rays))
    assert_same_instance_state(sc, fresh)
    assert sc.info()["stack_overflows"] == 0
    sc.close(); fresh.close()
