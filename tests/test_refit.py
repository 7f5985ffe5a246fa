"""Animated geometry: crt_update_vertices refits the CWBVH, the BVH2 and the intersection records of a live scene to new vertex
positions (same topology).  The host refits (crt_bvh2_refit / crt_cwbvh_refit) are checked here against the builders and against
numpy decodes of the quantised boxes; the device refit is checked byte for byte against the host refits, and every walk and frame of
an updated scene against a scene created fresh from the moved vertices and against the CPU oracle."""

import numpy as np
import pytest

from conftest import numpy_brute_force, seeded_rays

RX1, RY1 = 0.6591631174087524, 0.9108020067214966      # frame-1 randomVector


def _tess(cornell, n, amplitude, disney=False):
    from caitlynrenderer_amd.meshgen import tessellated_cornell, with_disney_materials
    base = cornell[0]
    return tessellated_cornell(with_disney_materials(base) if disney else base, n, amplitude)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _records(leaf_tris, ids, slots, V):
    """Intersection records (v0 | id) (e1 | slot) (e2 | material) of the given slots, as crt_scene_create gathers them."""
    t = leaf_tris[slots]
    v0, v1, v2 = V[t[:, 0]], V[t[:, 1]], V[t[:, 2]]
    r = np.zeros((slots.shape[0], 12), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 8:11] = v0, (v1 - v0).astype(np.float32), (v2 - v0).astype(np.float32)
    r[:, 3], r[:, 7], r[:, 11] = ids[slots].view(np.float32), slots.astype(np.int32).view(np.float32), t[:, 3].view(np.float32)
    return r


def _bvh2_refit(cr, flat, leaf_tris, V):
    sb = cr.SBVH.__new__(cr.SBVH)
    sb.flat_nodes, sb.triangles = np.ascontiguousarray(flat, np.float32).copy(), np.ascontiguousarray(leaf_tris, np.int32)
    return sb.refit(V).flat_nodes


def _cwbvh_refit(cr, nodes, tri_slots, leaf_tris, V):
    cw = cr.CWBVH()
    cw.nodes, cw.tri_slots = np.ascontiguousarray(nodes, np.uint8).copy(), np.ascontiguousarray(tri_slots, np.int32)
    return cw.refit(leaf_tris, V).nodes


def _check_cwbvh_boxes(nodes, tri_slots, leaf_tris, V):
    """Every slot decoded as the walk does (p + q * 2^(e-127)) contains the exact union of the vertices below it and lies within one
    quantum of it.  Returns the number of slots checked."""
    n8 = nodes.shape[0]
    p = nodes[:, 0:12].copy().view(np.float32)
    scale = (nodes[:, 12:15].astype(np.uint32) << 23).view(np.float32)
    imask = nodes[:, 15].astype(np.uint32)
    cb = nodes[:, 16:20].copy().view(np.uint32)[:, 0]
    tb = nodes[:, 20:24].copy().view(np.uint32)[:, 0]
    meta = nodes[:, 24:32]
    q = nodes[:, 32:80].reshape(n8, 3, 2, 8).astype(np.float32)
    order, k = [0], 0
    while k < len(order):
        i = order[k]; k += 1
        order += [int(cb[i]) + bin(int(imask[i]) & ((1 << s) - 1)).count("1") for s in range(8) if (imask[i] >> s) & 1]
    exact = np.zeros((n8, 2, 3), np.float32)
    checked = 0
    for i in reversed(order):
        lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for s in range(8):
            m = int(meta[i, s])
            if m == 0:
                continue
            if (imask[i] >> s) & 1:
                c = int(cb[i]) + bin(int(imask[i]) & ((1 << s) - 1)).count("1")
                blo, bhi = exact[c, 0], exact[c, 1]
            else:
                first, cnt = int(tb[i]) + (m & 31), bin(m >> 5).count("1")
                pts = V[leaf_tris[tri_slots[first:first + cnt], :3].ravel()]
                blo, bhi = pts.min(0), pts.max(0)
            dlo = (p[i] + q[i, :, 0, s] * scale[i]).astype(np.float32)
            dhi = (p[i] + q[i, :, 1, s] * scale[i]).astype(np.float32)
            assert (dlo <= blo).all() and (dhi >= bhi).all(), (i, s)
            slack = scale[i].astype(np.float64) + 2.0 * np.spacing(np.abs(np.concatenate([blo, bhi])).max())
            assert ((blo.astype(np.float64) - dlo) <= slack).all() and ((dhi.astype(np.float64) - bhi) <= slack).all(), (i, s)
            lo, hi = np.minimum(lo, blo), np.maximum(hi, bhi)
            checked += 1
        exact[i, 0], exact[i, 1] = lo, hi
    return checked


def _check_bvh2_boxes(flat, leaf_tris, V):
    """Leaf boxes are the exact unions of their triangles' vertex boxes, inner boxes the unions of their children."""
    leaf = flat[:, 7] != 0
    for i in np.nonzero(leaf)[0]:
        a, r = int(flat[i, 3]), int(flat[i, 7])
        pts = V[leaf_tris[a:a + r, :3].ravel()]
        assert np.array_equal(flat[i, 0:3], pts.min(0)) and np.array_equal(flat[i, 4:7], pts.max(0)), i
    inner = np.nonzero(~leaf)[0]
    l = flat[inner, 3].astype(np.int64)
    assert np.array_equal(flat[inner, 0:3], np.minimum(flat[l, 0:3], flat[l + 1, 0:3]))
    assert np.array_equal(flat[inner, 4:7], np.maximum(flat[l, 4:7], flat[l + 1, 4:7]))


# ------------------------------------------------------------------------------------------------------------ host (no GPU) --

@pytest.mark.parametrize("n", [8, 40])
def test_refit_with_unchanged_vertices_gives_the_builders_bytes(cr, cornell, n):
    """The SAH-only SBVH's boxes are exact unions of its triangles' vertex boxes and the converter quantises against the BVH2 node box,
    which is the union of the node8's slot boxes: a refit to the same vertices reproduces both trees byte for byte."""
    m = _tess(cornell, n, 0.02)
    data = cr.SceneData.build(m, cornell[1], sbvh_flags=1)
    flat = _bvh2_refit(cr, data.bvh, data.triangles, m.vertices)
    nodes = _cwbvh_refit(cr, data.bvh8, data.bvh8_tri_slots, data.triangles, m.vertices)
    assert np.array_equal(_bits(flat), _bits(data.bvh))
    assert np.array_equal(_bits(nodes), _bits(data.bvh8))


def test_refit_with_spatial_splits_contains_the_geometry(cr, cornell):
    """With spatial splits the builder clips a duplicate's box to its side of the split plane; the refit gives every reference the
    full box of its triangle, so the boxes contain the builder's (and the geometry) rather than equal them."""
    m = _tess(cornell, 8, 0.02)
    data = cr.SceneData.build(m, cornell[1], sbvh_flags=0)
    flat = _bvh2_refit(cr, data.bvh, data.triangles, m.vertices)
    assert (flat[:, 0:3] <= data.bvh[:, 0:3]).all() and (flat[:, 4:7] >= data.bvh[:, 4:7]).all()
    assert np.array_equal(flat[:, [3, 7]], data.bvh[:, [3, 7]])
    _check_bvh2_boxes(flat, data.triangles, m.vertices)
    nodes = _cwbvh_refit(cr, data.bvh8, data.bvh8_tri_slots, data.triangles, m.vertices)
    assert _check_cwbvh_boxes(nodes, data.bvh8_tri_slots, data.triangles, m.vertices) > 1000


@pytest.mark.parametrize("sbvh_flags", [1, 0])
@pytest.mark.parametrize("motion", ["amp0.1", "amp0.5", "amp3", "translate"])
def test_deformed_refit_contains_every_vertex_within_one_quantum(cr, cornell, sbvh_flags, motion):
    m = _tess(cornell, 8, 0.02)
    data = cr.SceneData.build(m, cornell[1], sbvh_flags=sbvh_flags)
    if motion == "translate":
        V = (m.vertices + np.float32([13.25, -7.5, 101.0])).astype(np.float32)
    else:
        V = _tess(cornell, 8, float(motion[3:])).vertices
    assert V.shape == m.vertices.shape and not np.array_equal(V, m.vertices)
    flat = _bvh2_refit(cr, data.bvh, data.triangles, V)
    _check_bvh2_boxes(flat, data.triangles, V)
    nodes = _cwbvh_refit(cr, data.bvh8, data.bvh8_tri_slots, data.triangles, V)
    assert _check_cwbvh_boxes(nodes, data.bvh8_tri_slots, data.triangles, V) > 1000
    assert np.array_equal(nodes[:, 15:32], data.bvh8[:, 15:32])


@pytest.mark.parametrize("n", [8, 40])
def test_refit_of_a_refit_returns_to_the_original_bytes(cr, cornell, n):
    m = _tess(cornell, n, 0.02)
    data = cr.SceneData.build(m, cornell[1], sbvh_flags=1)
    V = _tess(cornell, n, 0.7).vertices
    flat = _bvh2_refit(cr, data.bvh, data.triangles, V)
    nodes = _cwbvh_refit(cr, data.bvh8, data.bvh8_tri_slots, data.triangles, V)
    assert not np.array_equal(_bits(nodes), _bits(data.bvh8)) and not np.array_equal(_bits(flat), _bits(data.bvh))
    flat = _bvh2_refit(cr, flat, data.triangles, m.vertices)
    nodes = _cwbvh_refit(cr, nodes, data.bvh8_tri_slots, data.triangles, m.vertices)
    assert np.array_equal(_bits(flat), _bits(data.bvh)) and np.array_equal(_bits(nodes), _bits(data.bvh8))


@pytest.mark.parametrize("bad", ["count", "nan", "+inf", "-inf"])
def test_host_refit_refuses_bad_vertices_and_writes_nothing(cr, cornell, bad):
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    m = _tess(cornell, 8, 0.02)
    data = cr.SceneData.build(m, cornell[1], sbvh_flags=1)
    V = _tess(cornell, 8, 0.3).vertices.copy()
    if bad == "count":
        V = V[:-5]
    else:
        V[V.shape[0] // 2, 1] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[bad]
    sb = cr.SBVH.__new__(cr.SBVH)
    sb.flat_nodes, sb.triangles = data.bvh.copy(), data.triangles
    with pytest.raises(CrtError) as e:
        sb.refit(V)
    assert e.value.code == CRT_ERR_INVALID and np.array_equal(_bits(sb.flat_nodes), _bits(data.bvh))
    cw = cr.CWBVH()
    cw.nodes, cw.tri_slots = data.bvh8.copy(), data.bvh8_tri_slots
    with pytest.raises(CrtError) as e:
        cw.refit(data.triangles, V)
    assert e.value.code == CRT_ERR_INVALID and np.array_equal(cw.nodes, data.bvh8)


def test_scene_update_needs_a_device(cr, cornell):
    """The device entry points refuse to run without a GPU like every other scene call; the host refits above do not need one."""
    import caitlynrenderer_amd._lib as L
    for name in ("crt_update_vertices", "crt_update_vertices_device", "crt_last_update_ms", "crt_debug_read_accel"):
        assert name in L.SYMBOLS
    assert hasattr(cr.Scene, "update_vertices") and hasattr(cr.Scene, "update_vertices_device") and hasattr(cr.Scene, "last_update_ms")


# ------------------------------------------------------------------------------------------------------------------ GPU --

def _accel(scene):
    return [scene.debug_read_accel(k) for k in range(4)]


def _host_side(cr, data, mesh, accel0):
    """(leaf-order triangles, slot -> original id, CWBVH tri_slots) of a scene, read back from its own records where the tree was built
    on the device."""
    recs, recs2 = accel0[1], accel0[3]
    tri_slots = recs[:, 7].copy().view(np.int32)
    if data.bvh is not None:
        return data.triangles, data.tri_orig_ids, tri_slots
    ids = recs2[:, 3].copy().view(np.int32)
    return mesh.triangles[ids], ids, tri_slots


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sbvh_sah", "sbvh", "lbvh", "ploc", "sah"])
def test_device_refit_matches_the_host_refit_byte_for_byte(cr, cornell, builder):
    m0, m1 = _tess(cornell, 8, 0.02), _tess(cornell, 8, 0.4)
    if builder.startswith("sbvh"):
        data = cr.SceneData.build(m0, cornell[1], sbvh_flags=1 if builder == "sbvh_sah" else 0)
    else:
        data = cr.SceneData.for_device_build(m0, cornell[1], builder)
    sc = cr.Scene(data, 64, 48, 1)
    a0 = _accel(sc)
    assert all(x.shape[0] > 0 for x in a0)
    leaf_tris, ids, tri_slots = _host_side(cr, data, m0, a0)
    # the records as created are the numpy gather of the original vertices
    assert np.array_equal(_bits(a0[1]), _bits(_records(leaf_tris, ids, tri_slots, m0.vertices)))
    assert np.array_equal(_bits(a0[3]), _bits(_records(leaf_tris, ids, np.arange(leaf_tris.shape[0]), m0.vertices)))
    sc.update_vertices(m1.vertices)
    a1 = _accel(sc)
    assert np.array_equal(_bits(a1[0]), _bits(_cwbvh_refit(cr, a0[0], tri_slots, leaf_tris, m1.vertices)))
    assert np.array_equal(_bits(a1[1]), _bits(_records(leaf_tris, ids, tri_slots, m1.vertices)))
    assert np.array_equal(_bits(a1[2]), _bits(_bvh2_refit(cr, a0[2], leaf_tris, m1.vertices)))
    assert np.array_equal(_bits(a1[3]), _bits(_records(leaf_tris, ids, np.arange(leaf_tris.shape[0]), m1.vertices)))
    dev_ms, wall_ms = sc.last_update_ms()
    assert 0.0 < dev_ms and 0.0 < wall_ms
    sc.close()


@pytest.mark.gpu
def test_walks_of_an_updated_scene(cr, ob, cornell):
    """Closest and any hits (CWBVH, and the BVH2 with lowest-id ties) equal those of a scene created from the moved vertices and a numpy
    brute force; the per-ray visit counters equal the oracle's walk over the host-refitted trees, so the tree itself is checked."""
    from caitlynrenderer_amd._lib import CRT_TRACE_ANY, CRT_TRACE_BVH2, CRT_TRACE_CLOSEST, CRT_TRACE_TIE_LOWEST_ID
    m0, m1 = _tess(cornell, 8, 0.02), _tess(cornell, 8, 0.5)
    data = cr.SceneData.build(m0, cornell[1])
    sc = cr.Scene(data, 64, 48, 1)
    sc.update_vertices(m1.vertices)
    fresh = cr.Scene(cr.SceneData.build(m1, cornell[1]), 64, 48, 1)
    rays = seeded_rays(m1, 20000, 7, cr.RAY_DT)
    for mode in (CRT_TRACE_CLOSEST, CRT_TRACE_BVH2 | CRT_TRACE_TIE_LOWEST_ID):
        got, want = sc.trace(rays, mode), fresh.trace(rays, mode)
        assert np.array_equal(got["tri"], want["tri"]) and (got["tri"] >= 0).mean() > 0.5
        for k in ("t", "u", "v"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (mode, k)
    for mode in (CRT_TRACE_ANY, CRT_TRACE_ANY | CRT_TRACE_BVH2):
        assert np.array_equal(sc.trace(rays, mode)["tri"] >= 0, fresh.trace(rays, mode)["tri"] >= 0), mode
    sub = rays[:48]
    tri, t, u, v = numpy_brute_force(m1, sub)
    got = sc.trace(sub)
    assert np.array_equal(got["tri"], tri) and np.array_equal(got["t"].view(np.uint32), t.view(np.uint32))
    refit = cr.SceneData.build(m0, cornell[1])
    refit.vertices = m1.vertices
    refit.bvh = _bvh2_refit(cr, data.bvh, data.triangles, m1.vertices)
    refit.bvh8 = _cwbvh_refit(cr, data.bvh8, data.bvh8_tri_slots, data.triangles, m1.vertices)
    orc = ob.Oracle(refit, 64, 48, 1, cornell[1])
    got, st = sc.trace(rays, CRT_TRACE_CLOSEST, stats=True)
    want, st_want = orc.trace(rays, ob.BVH8, ob.CLOSEST, ob.TIE_LOWEST_ID, stats=True, threads=8)
    assert np.array_equal(got["tri"], want["tri"])
    assert np.array_equal(st["nodes"], st_want["nodes"]) and np.array_equal(st["tris"], st_want["tris"])
    fresh_st = fresh.trace(rays, CRT_TRACE_CLOSEST, stats=True)[1]
    assert not np.array_equal(st["nodes"], fresh_st["nodes"])        # a different tree than the fresh build's, walked as refitted
    sc.close(); fresh.close()


def _frames(scene, rvs):
    scene.render_frame(*rvs[0])
    scene.render_frames(rvs[1:])
    return scene.read_sum().copy()


@pytest.mark.gpu
@pytest.mark.parametrize("depth,disney", [(1, False), (4, False), (4, True)])
def test_frames_after_an_update_equal_a_fresh_scene_and_the_oracle(cr, ob, cornell, depth, disney):
    W, H = 120, 72
    m0, m1 = _tess(cornell, 8, 0.02, disney), _tess(cornell, 8, 0.35, disney)
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(4)]
    sc = cr.Scene(cr.SceneData.build(m0, cornell[1]), W, H, depth)
    sc.render_frame(RX1, RY1)
    assert sc.read_sum().any()
    sc.update_vertices(m1.vertices)
    assert not sc.read_sum().any()                                  # the update clears the sum
    got = _frames(sc, rvs)
    d1 = cr.SceneData.build(m1, cornell[1])
    fresh = cr.Scene(d1, W, H, depth)
    want = _frames(fresh, rvs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    orc = ob.Oracle(d1, W, H, depth, cornell[1])
    ref = np.zeros((H, W, 3), np.float32)
    for r in rvs:
        orc.render_frame(r[0], r[1], ref, threads=8)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and ref.max() > 0.1
    sc.close(); fresh.close()


@pytest.mark.gpu
def test_moving_the_light_with_its_lights_entry(cr, ob, cornell):
    W, H = 96, 64
    m0 = _tess(cornell, 8, 0.02)
    emissive = m0.materials[m0.triangles[:, 3], 7] != -1.0
    lv = np.unique(m0.triangles[emissive, :3])
    d = np.float32([-40.0, 0.0, 25.0])
    V = m0.vertices.copy()
    V[lv] = (V[lv] + d).astype(np.float32)
    lights = m0.lights.copy()
    lights[:, 0:3] = (lights[:, 0:3] + d).astype(np.float32)
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(3)]
    sc = cr.Scene(cr.SceneData.build(m0, cornell[1]), W, H, 3)
    sc.update_vertices(V, lights=lights)
    got = _frames(sc, rvs)
    m1 = cr.Mesh(V, m0.normals, m0.texcoords, m0.triangles, m0.materials, lights, m0.vertex_min)
    d1 = cr.SceneData.build(m1, cornell[1])
    orc = ob.Oracle(d1, W, H, 3, cornell[1])
    ref = np.zeros((H, W, 3), np.float32)
    for r in rvs:
        orc.render_frame(r[0], r[1], ref, threads=8)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    sc.close()


@pytest.mark.gpu
def test_an_animation_returns_to_the_never_updated_tree(cr, cornell):
    W, H = 96, 64
    m0 = _tess(cornell, 8, 0.02)
    data = cr.SceneData.for_device_build(m0, cornell[1], "sah")
    sc, still = cr.Scene(data, W, H, 2), cr.Scene(data, W, H, 2)
    sc.set_option("count_visits", 1)
    for k, amp in enumerate([0.1, 0.5, 1.5, 3.0, 0.05, 2.0, 0.8, 0.3, 4.0]):
        sc.update_vertices(_tess(cornell, 8, amp).vertices)
        sc.render_frame(RX1, RY1 + 0.01 * k)
        assert sc.frame_stats()["stack_overflows"] == 0
    sc.update_vertices(m0.vertices)
    for k in range(4):
        assert np.array_equal(_bits(sc.debug_read_accel(k)), _bits(still.debug_read_accel(k))), k
    assert np.array_equal(_frames(sc, [(RX1, RY1), (0.25, 0.5)]).view(np.uint32), _frames(still, [(RX1, RY1), (0.25, 0.5)]).view(np.uint32))
    sc.close(); still.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fan", ["devices", "streams"])
def test_fan_out_to_replicas(cr, cornell, fan):
    W, H = 128, 80
    m0, m1 = _tess(cornell, 8, 0.02), _tess(cornell, 8, 0.6)
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(4)]
    data = cr.SceneData.build(m0, cornell[1])
    multi = cr.Scene(data, W, H, 3)
    if fan == "devices":
        multi.set_devices([0, 0, 0])
    else:
        multi.set_option("streams", 2)
    multi.render_frame(RX1, RY1)                                      # the replicas exist and hold the old scene's planes
    multi.update_vertices(m1.vertices)
    got = _frames(multi, rvs)
    single = cr.Scene(data, W, H, 3)
    single.update_vertices(m1.vertices)
    want = _frames(single, rvs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and want.max() > 0.1
    multi.close(); single.close()


@pytest.mark.gpu
def test_device_form_from_a_torch_tensor(cr, cornell):
    import torch
    m0, m1 = _tess(cornell, 8, 0.02), _tess(cornell, 8, 0.45)
    data = cr.SceneData.build(m0, cornell[1])
    a, b = cr.Scene(data, 96, 64, 2), cr.Scene(data, 96, 64, 2)
    t = torch.from_numpy(m1.vertices).to("cuda")
    torch.cuda.synchronize()
    a.update_vertices_device(t.data_ptr(), t.shape[0], sync=False)
    a.sync()
    b.update_vertices(m1.vertices)
    for k in range(4):
        assert np.array_equal(_bits(a.debug_read_accel(k)), _bits(b.debug_read_accel(k))), k
    assert np.array_equal(_frames(a, [(RX1, RY1), (0.3, 0.7)]).view(np.uint32), _frames(b, [(RX1, RY1), (0.3, 0.7)]).view(np.uint32))
    assert a.last_update_ms()[0] > 0.0
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["count_less", "count_more", "nan", "+inf", "-inf", "normals", "lights"])
def test_a_refused_update_leaves_the_scene_as_it_was(cr, cornell, bad):
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    m0 = _tess(cornell, 8, 0.02)
    data = cr.SceneData.build(m0, cornell[1])
    sc, ref = cr.Scene(data, 96, 64, 2), cr.Scene(data, 96, 64, 2)
    sc.render_frame(RX1, RY1); ref.render_frame(RX1, RY1)
    V = _tess(cornell, 8, 0.5).vertices.copy()
    kw = {}
    if bad == "count_less":
        V = V[:-1]
    elif bad == "count_more":
        V = np.concatenate([V, V[:1]])
    elif bad == "normals":
        kw["normals"] = m0.normals[:-1]
    elif bad == "lights":
        kw["lights"] = np.concatenate([m0.lights, m0.lights])
    else:
        V[V.shape[0] - 3, 2] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[bad]
    a0 = _accel(sc)
    with pytest.raises(CrtError) as e:
        sc.update_vertices(V, **kw)
    assert e.value.code == CRT_ERR_INVALID
    for k in range(4):
        assert np.array_equal(_bits(sc.debug_read_accel(k)), _bits(a0[k])), k
    assert np.array_equal(_frames(sc, [(0.3, 0.7), (0.1, 0.2)]).view(np.uint32), _frames(ref, [(0.3, 0.7), (0.1, 0.2)]).view(np.uint32))
    sc.close(); ref.close()


@pytest.mark.gpu
def test_full_size_mesh_update_against_the_oracle(cr, ob, cornell):
    """mesh1m (1,004,672 triangles) built on the device, one update, one four-sample step of four segments, rows against the oracle
    (whose tree is a GPU SAH build of the moved mesh: the sums do not depend on the tree)."""
    W, H = 320, 180
    m0, m1 = _tess(cornell, 183, 0.02), _tess(cornell, 183, 0.1)
    assert m0.triangles.shape[0] == 1004672
    sc = cr.Scene(cr.SceneData.for_device_build(m0, cornell[1], "sah"), W, H, 4)
    sc.update_vertices(m1.vertices)
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(4)]
    sc.render_frames(rvs)
    got = sc.read_sum().reshape(H, W, 3)
    orc = ob.Oracle(cr.SceneData.build(m1, cornell[1], builder="sah", convert="device"), W, H, 4, cornell[1])
    ref = np.zeros((H, W, 3), np.float32)
    rows = (60, 76)
    for r in rvs:
        orc.render_rows(r[0], r[1], rows[0], rows[1], ref)
    assert np.array_equal(got[rows[0]:rows[1]].view(np.uint32), ref[rows[0]:rows[1]].view(np.uint32))
    assert ref[rows[0]:rows[1]].max() > 0.1
    sc.close()
