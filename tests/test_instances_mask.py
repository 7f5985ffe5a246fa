"""Instance visibility masks (include/crt.h CRT_TRACE_INSTANCE_MASK, crt_instance.mask): the layouts and the refusals
without a GPU; on the GPU masks that hide nothing against the unmasked trace byte for byte, random ray masks against an unmasked trace of
a handle holding only the visible instances, ray mask 0, subtree culling in the TLAS, the TLAS child masks against a host restatement
after a create, a set, a refit and an update, masks carried by refits, refused refits, updates and the device forms, and the mode
checks.  The helpers of tests/test_instances*.py are restated here."""
import ctypes as C

import numpy as np
import pytest

f32 = np.float32
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


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


def with_vertices(cr, mesh, v):
    return cr.Mesh(np.ascontiguousarray(v, f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials, mesh.lights)


def group_masks(rng, n):
    """groups of masks 1, 2, 4 and 8, and a few instances of 0, 3 and 0x80"""
    return rng.choice(np.array([1, 2, 4, 8, 0, 3, 0x80], np.uint32), n, p=[0.21, 0.21, 0.21, 0.21, 0.06, 0.05, 0.05])


def assert_closest_equal(a, b):
    (ga, ia), (gb, ib) = a[:2], b[:2]
    assert np.array_equal(ga["tri"], gb["tri"]), np.nonzero(ga["tri"] != gb["tri"])[0][:10]
    assert np.array_equal(ia, ib), np.nonzero(ia != ib)[0][:10]
    h = ga["tri"] >= 0
    for f in ("t", "u", "v"):
        assert np.array_equal(ga[f][h].view(np.uint32), gb[f][h].view(np.uint32)), f


def subset_reference(cr, ref, inst, rays, ray_masks):
    """per distinct ray mask: an unmasked closest trace on `ref` set to the instances visible to it (in instance order), its instance ids
    mapped back.  -> (hits, ids) in ray order"""
    n = rays.shape[0]
    hits, ids = np.zeros(n, cr.HIT_DT), np.full(n, -1, np.int32)
    hits["tri"] = -1
    for r in np.unique(ray_masks):
        sel = np.nonzero(ray_masks == r)[0]
        vis = np.nonzero((inst["mask"] & 0xff) & r)[0]
        if vis.size == 0:
            continue
        ref.set(inst[vis])
        h, i = ref.trace(rays[sel])
        hits[sel] = h
        ids[sel] = np.where(i >= 0, vis[np.maximum(i, 0)], -1)
    return hits, ids


def expected_child_masks(nodes, rec, masks):
    """the OR of (mask & 0xff) of every instance under each meta slot of each TLAS node8, from the decoded node8s (imask, meta, bases)
    and the records' instance index (row 3 .y)"""
    n8 = nodes.shape[0]
    inst_of = rec[:, 13].view(np.uint32)
    m8 = np.asarray(masks, np.uint32) & 0xff
    out = np.zeros((n8, 8), np.uint8)
    done = np.zeros(n8, bool)

    def visit(i):
        nd = nodes[i]
        imask = int(nd[15])
        child_base, tri_base = (int(x) for x in nd[16:24].view(np.uint32))
        for s in range(8):
            meta = int(nd[24 + s])
            if (imask >> s) & 1:
                c = child_base + bin(imask & ((1 << s) - 1)).count("1")
                if not done[c]:
                    visit(c)
                out[i, s] = np.bitwise_or.reduce(out[c])
            elif meta:
                first = tri_base + (meta & 31)
                out[i, s] = np.bitwise_or.reduce(m8[inst_of[first:first + bin(meta >> 5).count("1")]])
        done[i] = True

    visit(0)
    assert done.all(), "every live TLAS node8 is reachable from the root"
    return out


# ---------------------------------------------------------------- CPU ----

def test_layouts_and_the_mode_bit(cr):
    from caitlynrenderer_amd import _lib
    assert C.sizeof(_lib.crt_instance) == 64 and cr.INSTANCE_DT.itemsize == 64
    assert _lib.crt_instance.mesh.offset == 48 and _lib.crt_instance.mask.offset == 52 and _lib.crt_instance.reserved.offset == 56
    assert cr.INSTANCE_DT.fields["mask"][1] == 52 and cr.INSTANCE_DT.fields["reserved"][1] == 56
    assert _lib.CRT_TRACE_INSTANCE_MASK == 8 and cr.CRT_TRACE_INSTANCE_MASK == 8
    m = np.stack([IDENTITY] * 3)
    plain = cr.instances_array(m, [0, 1, 2])
    assert np.array_equal(plain.view(np.uint8), cr.instances_array(m, [0, 1, 2], None).view(np.uint8))
    assert not plain["mask"].any() and not plain["reserved"].any()
    masked = cr.instances_array(m, [0, 1, 2], [1, 0x80, 0x1ff])
    assert list(masked["mask"]) == [1, 0x80, 0x1ff]
    assert np.array_equal(np.delete(masked.view(np.uint32).reshape(3, 16), 13, 1), np.delete(plain.view(np.uint32).reshape(3, 16), 13, 1))


def test_mask_paths_fail_loudly_without_a_gpu_or_a_handle(cr, cornell):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    assert L.crt_instances_trace(None, None, 0, None, None, _lib.CRT_TRACE_INSTANCE_MASK, None) == _lib.CRT_ERR_INVALID
    assert L.crt_instances_trace_device(None, None, 0, None, None, _lib.CRT_TRACE_INSTANCE_MASK, None, 1) == _lib.CRT_ERR_INVALID
    assert L.crt_instances_debug_read(None, 6, None, 0, None) == _lib.CRT_ERR_INVALID
    sc = object.__new__(cr.InstancedScene)
    sc._h = C.c_void_p()
    rays = np.zeros(4, cr.RAY_DT)
    rays["pad"] = 7
    with pytest.raises(cr.CrtError) as e:
        sc.trace(rays, ray_mask=3)
    assert e.value.code == _lib.CRT_ERR_INVALID and "crt_instances_trace" in str(e.value)
    assert (rays["pad"] == 7).all()                   # the mask went into a copy
    with pytest.raises(cr.CrtError) as e:
        sc.tlas_child_masks()
    assert e.value.code == _lib.CRT_ERR_INVALID
    if L.crt_device_count() > 0:
        return                                        # the GPU tests below cover a live handle
    mesh, _ = cornell
    with pytest.raises(cr.CrtError) as e:
        cr.InstancedScene([mesh], cr.instances_array([IDENTITY], [0], [1]))
    assert e.value.code == _lib.CRT_ERR_NO_DEVICE


# ---------------------------------------------------------------- GPU ----

@pytest.fixture(scope="module")
def meshes3(cr, cornell, tess8, tess40):
    return [with_vertices(cr, m, no_negative_zero(m.vertices)) for m in (cornell[0], tess8[0], tess40[0])]


@pytest.fixture(scope="module")
def placed(cr, meshes3):
    rng = np.random.default_rng(314)
    M, mesh_of = placed_instances(rng, 300, 3)
    rays = world_rays(cr, rng, 6000, centres=M[:, :, 3])
    ray_masks = rng.integers(0, 256, rays.shape[0]).astype(np.uint8)
    return M, mesh_of, rays, ray_masks, rng


@pytest.mark.gpu
def test_masks_that_hide_nothing_change_nothing(cr, meshes3, placed):
    M, mesh_of, rays, _, rng = placed
    n = M.shape[0]
    plain = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of))
    full = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, np.full(n, 0xff)))
    rnd_masks = rng.integers(1, 256, n) | (rng.integers(0, 1 << 20, n) << 8)           # non-zero low bytes, ignored high bits
    rnd = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, rnd_masks))
    for mode in (cr.CRT_TRACE_CLOSEST, cr.CRT_TRACE_ANY):
        want = [x.view(np.uint8) for x in plain.trace(rays, mode, stats=True)]
        assert (want[1].view(np.int32) >= 0).sum() > 1000
        cases = [(full, rng.integers(1, 256, rays.shape[0])), (rnd, 0xff), (rnd, None), (full, None)]
        for sc, rm in cases:
            got = [x.view(np.uint8) for x in sc.trace(rays, mode, stats=True, ray_mask=rm)]
            for k in range(3):
                assert np.array_equal(got[k], want[k]), (mode, rm is None, k)
    for sc in (plain, full, rnd):
        assert sc.info()["stack_overflows"] == 0
        sc.close()


@pytest.mark.gpu
def test_masked_closest_and_any_equal_a_handle_of_the_visible_instances(cr, meshes3, placed):
    M, mesh_of, rays, ray_masks, _ = placed
    n = M.shape[0]
    inst = cr.instances_array(M, mesh_of, group_masks(np.random.default_rng(5), n))
    sc = cr.InstancedScene(meshes3, inst)
    ref = cr.InstancedScene(meshes3, inst, capacity=n)
    want = subset_reference(cr, ref, inst, rays, ray_masks)
    got = sc.trace(rays, ray_mask=ray_masks)
    assert (got[1] >= 0).sum() > 500 and (got[1] >= 0).sum() < (sc.trace(rays)[1] >= 0).sum()
    assert_closest_equal(got, want)
    # any hit: the same rays hit, and the instance reported is visible and has a hit in [0, tmax) on its own
    ga, ia = sc.trace(rays, cr.CRT_TRACE_ANY, ray_mask=ray_masks)
    hit = want[1] >= 0
    assert np.array_equal(ga["tri"] >= 0, hit) and np.array_equal(ia >= 0, hit)
    assert ((inst["mask"][ia[hit]] & ray_masks[hit]) != 0).all()
    for k in np.unique(ia[hit]):
        sel = np.nonzero(ia == k)[0]
        ref.set(inst[k:k + 1])
        h, _ = ref.trace(rays[sel])
        assert (h["tri"] >= 0).all(), k
    assert sc.info()["stack_overflows"] == 0
    sc.close(); ref.close()


@pytest.mark.gpu
def test_ray_mask_zero_hits_nothing_after_the_root_step(cr, meshes3, placed):
    M, mesh_of, rays, _, rng = placed
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, np.full(M.shape[0], 0xff)))
    for mode in (cr.CRT_TRACE_CLOSEST, cr.CRT_TRACE_ANY):
        h, i, st = sc.trace(rays, mode, stats=True, ray_mask=0)
        assert (h["tri"] == -1).all() and (i == -1).all()
        assert (st["nodes"] == 1).all() and (st["tris"] == 0).all()
        _, i2, st2 = sc.trace(rays, mode, stats=True)
        assert (i2 >= 0).sum() > 1000 and st2["nodes"].mean() > 4
    sc.close()


@pytest.mark.gpu
def test_hidden_subtrees_are_not_entered(cr):
    """one visible instance far from a 32 x 32 cluster of hidden ones: a ray into the cluster may enter only the TLAS nodes on the path
    to the visible instance (it misses that instance's box), and tests no triangle"""
    V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5)], f32)
    T = np.zeros((2, 12), np.int32)
    T[:, :3] = [(0, 1, 2), (1, 3, 2)]
    M = []
    for y in range(32):
        for x in range(32):
            M.append(np.concatenate([np.eye(3) * 0.8, [[x], [y], [0.0]]], 1))
    M.append(np.concatenate([np.eye(3), [[500.0], [500.0], [0.0]]], 1))
    M = np.array(M, f32)
    masks = np.full(M.shape[0], 1, np.uint32)
    masks[-1] = 2
    sc = cr.InstancedScene([(V, T)], cr.instances_array(M, np.zeros(M.shape[0]), masks))
    depth = sc.info()["tlas_depth8"]
    rng = np.random.default_rng(11)
    rays = np.zeros(4096, cr.RAY_DT)
    # half from above, down into the cluster; half along x through the gaps between its rows (inside TLAS node boxes, no instance's)
    rays["o"][:2048, :2] = rng.uniform(0.0, 32.0, (2048, 2)).astype(f32)
    rays["o"][:2048, 2] = f32(10.0)
    d = np.concatenate([rng.normal(scale=0.05, size=(2048, 2)), -np.ones((2048, 1))], 1)
    rays["o"][2048:] = np.stack([np.full(2048, -2.0), rng.integers(0, 31, 2048) + 0.9, rng.uniform(0.05, 0.35, 2048)], 1).astype(f32)
    d = np.concatenate([d, np.tile([1.0, 0.0, 0.0], (2048, 1))])
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmax"] = f32(1e9)
    _, i, st = sc.trace(rays, stats=True, ray_mask=2)
    assert (i == -1).all()
    assert (st["tris"] == 0).all() and st["nodes"].max() <= depth, (int(st["nodes"].max()), depth)
    _, i0, st0 = sc.trace(rays, stats=True)
    assert (i0[:2048] >= 0).sum() > 1000 and (i0 < 1024).all()
    assert st0["nodes"].mean() > depth and st0["nodes"].mean() > 2 * st["nodes"].mean() and st0["tris"][:2048].mean() > 1, \
        (float(st0["nodes"].mean()), float(st["nodes"].mean()), depth)
    _, i1, st1 = sc.trace(rays, stats=True, ray_mask=1)          # the cluster's own mask walks as the unmasked trace
    assert np.array_equal(i1, i0) and np.array_equal(st1.view(np.uint8), st0.view(np.uint8))
    sc.close()


@pytest.mark.gpu
def test_tlas_child_masks_after_create_set_refit_and_update(cr, meshes3, placed):
    M, mesh_of, _, _, _ = placed
    n = M.shape[0]
    rng = np.random.default_rng(8)

    def check(sc, masks):
        rec = sc.instance_records()
        got = sc.tlas_child_masks()
        assert got.shape == (sc.info()["tlas_nodes8"], 8)
        assert np.array_equal(got, expected_child_masks(sc.tlas_nodes(), rec, masks))
        # row 3 .w of each record: its instance's mask & 0xff
        assert np.array_equal(rec[:, 15].view(np.uint32), (np.asarray(masks, np.uint32) & 0xff)[rec[:, 13].view(np.uint32)])

    masks = rng.integers(0, 1 << 12, n).astype(np.uint32)             # bits 8..11 are ignored
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, masks), capacity=n, updatable=True)
    check(sc, masks)
    k = 137
    masks = group_masks(rng, k)
    sc.set(cr.instances_array(M[:k], mesh_of[:k], masks))
    check(sc, masks)
    masks = rng.integers(0, 256, k).astype(np.uint32)
    sc.refit(cr.instances_array(M[:k], mesh_of[:k], masks))
    check(sc, masks)
    sc.update_meshes({1: meshes3[1].vertices})
    check(sc, masks)
    one = cr.InstancedScene(meshes3, cr.instances_array(M[:1], mesh_of[:1], [0x40]))
    check(one, [0x40])
    sc.close(); one.close()


@pytest.mark.gpu
def test_refits_updates_and_device_forms_carry_the_masks(cr, meshes3, placed):
    import torch
    from caitlynrenderer_amd import _lib
    M, mesh_of, rays, ray_masks, _ = placed
    n = M.shape[0]
    rng = np.random.default_rng(99)
    first = cr.instances_array(M, mesh_of, group_masks(rng, n))
    second = cr.instances_array(M, mesh_of, group_masks(rng, n))
    ref = cr.InstancedScene(meshes3, first, capacity=n)
    want = subset_reference(cr, ref, second, rays, ray_masks)
    sc = cr.InstancedScene(meshes3, first, updatable=True)
    before = sc.trace(rays, ray_mask=ray_masks)
    # a refit with the same matrices and new masks: shows and hides without a TLAS rebuild
    nodes = sc.tlas_nodes()
    sc.refit(second)
    assert np.array_equal(sc.tlas_nodes(), nodes)
    got = sc.trace(rays, ray_mask=ray_masks)
    assert not np.array_equal(got[1], before[1])
    assert_closest_equal(got, want)
    # a refused refit (one singular matrix) leaves the masked trace as it was
    bad = first.copy()
    bad["object_to_world"][5] = 0.0
    with pytest.raises(cr.CrtError) as e:
        sc.refit(bad)
    assert e.value.code == _lib.CRT_ERR_INVALID
    assert_closest_equal(sc.trace(rays, ray_mask=ray_masks), want)
    # an update keeps the live masks
    sc.update_meshes({0: meshes3[0].vertices, 2: meshes3[2].vertices})
    assert_closest_equal(sc.trace(rays, ray_mask=ray_masks), want)
    # the device forms read the masks from device memory
    dev = cr.InstancedScene(meshes3, first, capacity=n)
    d_second = torch.from_numpy(second.view(np.uint8).copy()).cuda()
    d_first = torch.from_numpy(first.view(np.uint8).copy()).cuda()
    dev.refit_device(d_second.data_ptr(), n)
    assert_closest_equal(dev.trace(rays, ray_mask=ray_masks), want)
    dev.refit_device(d_first.data_ptr(), n)
    assert_closest_equal(dev.trace(rays, ray_mask=ray_masks), before)
    dev.set_device(d_second.data_ptr(), n)
    assert_closest_equal(dev.trace(rays, ray_mask=ray_masks), want)
    # trace_device with the mode bit: the masks in the rays' pad words
    r = rays.copy()
    r["pad"] = ray_masks
    d_rays = torch.from_numpy(r.view(np.uint8).copy()).cuda()
    d_hits = torch.empty(r.shape[0] * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.empty(r.shape[0], dtype=torch.int32, device="cuda")
    dev.trace_device(d_rays.data_ptr(), r.shape[0], d_hits.data_ptr(), d_ids.data_ptr(), cr.CRT_TRACE_CLOSEST | cr.CRT_TRACE_INSTANCE_MASK)
    assert_closest_equal((d_hits.cpu().numpy().view(cr.HIT_DT), d_ids.cpu().numpy()), want)
    for s in (sc, dev, ref):
        assert s.info()["stack_overflows"] == 0
        s.close()


@pytest.mark.gpu
def test_unknown_mode_bits_are_still_refused(cr, cornell, meshes3):
    from caitlynrenderer_amd import _lib
    sc = cr.InstancedScene(meshes3, cr.instances_array([IDENTITY], [0], [1]))
    rays = np.zeros(64, cr.RAY_DT)
    rays["d"][:, 2] = 1.0
    rays["tmax"] = 1.0
    mk = _lib.CRT_TRACE_INSTANCE_MASK
    for mode in (mk | _lib.CRT_TRACE_BVH2, mk | _lib.CRT_TRACE_TIE_LOWEST_ID, mk | 16, 16, 2, -1, -8, mk | 1 | 32):
        with pytest.raises(cr.CrtError) as e:
            sc.trace(rays, mode)
        assert e.value.code == _lib.CRT_ERR_INVALID, mode
    sc.trace(rays, mk | _lib.CRT_TRACE_ANY)
    sc.close()
    mesh, cam = cornell
    flat = cr.Scene(cr.SceneData.for_device_build(mesh, cam), 16, 16, 1)
    with pytest.raises(cr.CrtError) as e:
        flat.trace(rays, mk)
    assert e.value.code == _lib.CRT_ERR_INVALID
    flat.close()
