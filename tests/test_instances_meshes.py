"""Adding and replacing the meshes of a live instanced scene (include/crt.h crt_instances_add_meshes / crt_instances_replace_meshes,
DESIGN.md §15): the entry points and their refusals without a GPU; on the GPU the repacked arrays against a fresh create from the
resulting mesh list byte for byte (every debug read, every info field but the times) where the builders are deterministic, the walk
against the CPU oracle fed the handle's own debug reads (hits, instance ids, per-ray counts), closest hits against the numpy brute force,
refusals with the state kept, the updatable state after either call, an interleaved sequence and the 1 M-triangle mesh.  The helpers of
tests/test_instances*.py are restated here."""
import ctypes as C

import numpy as np
import pytest

from conftest import numpy_brute_force

f32 = np.float32
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
THREADS = 16
TIMES = ("set_device_ms", "set_wall_ms", "create_wall_ms")
BYTE_BUILDERS = ("sah", "lbvh")          # builders whose two builds of one input are equal byte for byte (asserted by the first GPU test)


# ---------------------------------------------------------------- restated helpers ----

def is_identity(m):
    return np.array_equal(np.asarray(m, np.float32).reshape(12).view(np.uint32), IDENTITY.reshape(12).view(np.uint32))


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


def placed_instances(rng, n, n_meshes, spread=12.0, scale=(0.5, 2.0)):
    M = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        s = rng.uniform(*scale, 3) * rng.choice([-1.0, 1.0], 3)
        A = q @ np.diag(s)
        M.append(np.concatenate([A, rng.uniform(-spread, spread, (3, 1))], 1))
    return np.array(M, f32), rng.integers(0, n_meshes, n)


def world_rays(rays_dt, rng, n, spread=16.0, centres=None):
    rays = np.zeros(n, rays_dt)
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


def edge_rays(rays_dt, rng, boxes, n_per=64, far=True):
    """Rays where walks go wrong, aimed at the given world boxes (lo, hi): signed and exact zero direction components, axis-aligned rays,
    origins inside the boxes, non-finite origins, a finite origin whose object origin overflows, tmax 0, the smallest denormal and +inf."""
    boxes = np.asarray(boxes, np.float64)
    centre = (boxes[:, :3] + boxes[:, 3:]) / 2
    pick = lambda k: centre[rng.integers(0, len(centre), k)]
    out = []

    def rays(o, d, tmax=1e9):
        r = np.zeros(len(o), rays_dt)
        r["o"], r["d"], r["tmax"] = np.asarray(o, f32), np.asarray(d, f32), f32(tmax)
        return r
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)
    signed = np.array([(-0.0, 1, 0), (0, -0.0, -1), (0.6, -0.0, 0.8), (-0.0, -0.0, 1), (-0.6, 0.8, -0.0), (0, 0, 0), (-0.0, -0.0, -0.0)], f32)
    for a in axes:
        c = pick(n_per)
        out.append(rays(c - 40.0 * a, np.broadcast_to(a, c.shape)))
    for s in signed:
        c = pick(n_per)
        o = c + rng.normal(scale=8.0, size=c.shape)
        d = (c - o)
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        d = np.where(s == 0, 0.0, d).astype(f32)
        d = np.where(np.signbit(s) & (s == 0), -f32(0.0), d).astype(f32)
        if not s.any():
            d = np.broadcast_to(s, d.shape)
        out.append(rays(o, d))
    lo, hi = boxes[:, :3], boxes[:, 3:]
    k = rng.integers(0, len(boxes), 4 * n_per)
    o = lo[k] + (hi[k] - lo[k]) * rng.random((4 * n_per, 3))
    d = rng.normal(size=o.shape)
    out.append(rays(o, d / np.linalg.norm(d, axis=1, keepdims=True)))
    bad = rays(pick(6), np.tile(np.array([[0.0, 0.0, 1.0]], f32), (6, 1)))
    bad["o"][0, 0] = np.nan; bad["o"][1, 1] = np.inf; bad["o"][2, 2] = -np.inf
    bad["o"][3] = (np.nan, np.nan, np.nan); bad["d"][4] = (np.nan, 0, 1); bad["d"][5] = (np.inf, 0, 0)
    out.append(bad)
    far_rays = rays(np.tile(np.array([[3.3e38, 0.0, 0.0]], f32), (n_per, 1)), np.tile(np.array([[-1.0, 0.0, 0.0]], f32), (n_per, 1)), np.inf)
    far_rays["o"][:, 1:] = pick(n_per)[:, 1:]
    if far:
        out.append(far_rays)
    for tmax in (0.0, np.float32(1e-45), np.inf):
        c = pick(n_per)
        o = c + rng.normal(scale=10.0, size=c.shape)
        d = c - o
        out.append(rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), tmax))
    for tmax in (0.0, np.float32(1e-45)):
        k = rng.integers(0, len(boxes), n_per)
        o = lo[k] + (hi[k] - lo[k]) * rng.random((n_per, 3))
        d = rng.normal(size=o.shape)
        out.append(rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), tmax))
    return np.concatenate(out)


def no_negative_zero(v):
    """x + 0 turns -0 into +0 and keeps every other float: the update's mesh box orders -0 below +0, create keeps the first of equal zeros"""
    return (np.asarray(v, f32) + f32(0.0)).astype(f32)


def displaced(v, amp, seed):
    rng = np.random.default_rng(seed)
    return no_negative_zero(np.asarray(v, f32) + (amp * rng.standard_normal(np.shape(v))).astype(f32))


def with_vertices(cr, mesh, v):
    return cr.Mesh(np.ascontiguousarray(v, f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials, mesh.lights)


def random_masks(rng, n):
    m = (1 << rng.integers(0, 8, n)).astype(np.uint32) | (rng.integers(0, 256, n).astype(np.uint32) & rng.integers(0, 2, n).astype(np.uint32) * 0xff)
    m[::29], m[3::31] = 0, 0xff
    return m


def assert_same_closest(a, b):
    (ga, ia), (gb, ib) = a, b
    assert np.array_equal(ga["tri"], gb["tri"]), np.nonzero(ga["tri"] != gb["tri"])[0][:10]
    assert np.array_equal(ia, ib)
    h = ga["tri"] >= 0
    for f in ("t", "u", "v"):
        assert np.array_equal(ga[f][h].view(np.uint32), gb[f][h].view(np.uint32)), f


def clustered_mesh(K):
    """K clusters of 8 triangles, each cluster 4x smaller than the previous and beside it: a CWBVH about K node8 levels deep"""
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


def blas_layout(sc, meshes):
    """per mesh: (first node8 in the BLAS region, node8 count, BLAS root as a global node index, first record); every mesh instanced"""
    inst = sc.instance_records()[:, 12:16].view(np.uint32)
    info = sc.info()
    tlas_cap = info["tlas_bytes"] // 80
    roots = np.array(sorted(set(int(r) for r in inst[:, 0])), np.int64)
    assert len(roots) == len(meshes), "every mesh needs an instance for the layout"
    ends = list(roots[1:] - tlas_cap) + [int(info["blas_nodes8"])]
    tri_off = np.concatenate([[0], np.cumsum([m.triangles.shape[0] for m in meshes])])
    return {k: (int(roots[k] - tlas_cap), int(ends[k] - (roots[k] - tlas_cap)), int(roots[k]), int(tri_off[k])) for k in range(len(meshes))}


def device_arrays(ob, sc):
    """What the walk reads, through the handle's debug reads 2..6, as tests/test_instances_oracle.py feeds them to the oracle"""
    info = sc.info()
    region = info["tlas_bytes"] // 80
    assert info["tlas_bytes"] == 80 * region and region == max(info["capacity"], 1), info
    a = dict(tlas=sc.tlas_nodes(), inst=sc.instance_records(), blas=sc.blas_nodes(), blas_recs=sc.blas_records(), region=region,
             stack=info["stack_entries"])
    assert a["tlas"].shape[0] == info["tlas_nodes8"] and a["inst"].shape[0] == info["n_instances"]
    assert a["blas"].shape[0] == info["blas_nodes8"] and a["blas_recs"].shape[0] == info["blas_tris"]
    a["cm"] = ob.tlas_child_masks(a["tlas"], a["inst"])
    if info["n_instances"]:
        assert np.array_equal(a["cm"], sc.tlas_child_masks())
    return a


def check_against_oracle(cr, ob, sc, rays, mode, ray_mask=None, a=None):
    """One trace of the kernel and of the oracle: hits, instance ids and stats byte for byte on EVERY ray, the stack within its bound and
    untouched by refusals.  -> instance ids"""
    a = device_arrays(ob, sc) if a is None else a
    n = rays.shape[0]
    before = sc.info()["stack_overflows"]
    gh, gi, gs = sc.trace(rays, mode, stats=True, ray_mask=ray_mask)
    r, m = rays, int(mode)
    if ray_mask is not None:
        r = rays.copy()
        r["pad"] = np.broadcast_to(np.asarray(ray_mask).astype(np.uint32) & 0xff, (n,))
        m |= ob.INSTANCE_MASK
    wh, wi, ws, depth, refused = ob.trace_instances(a["tlas"], a["inst"], a["blas"], a["blas_recs"], r, a["region"], a["stack"], m, a["cm"],
                                                     threads=THREADS)
    bad = np.nonzero((gh.view(np.uint8).reshape(n, 16) != wh.view(np.uint8).reshape(n, 16)).any(1) | (gi != wi) |
                     (gs.view(np.uint32) != ws.view(np.uint32)))[0]
    assert bad.size == 0, (m, bad.size, bad[:4], r[bad[:4]], gh[bad[:4]], wh[bad[:4]], gi[bad[:4]], wi[bad[:4]], gs[bad[:4]], ws[bad[:4]])
    assert depth.max(initial=0) <= a["stack"] and refused.sum() == 0, (depth.max(), a["stack"], refused.sum())
    assert sc.info()["stack_overflows"] == before == 0
    return gi


def check_modes(cr, ob, sc, rays, rng):
    """closest, closest masked, any, any masked (random ray masks, 0 and 0xff among them) against the oracle -> the unmasked closest ids"""
    a = device_arrays(ob, sc)
    rm = rng.integers(0, 256, rays.shape[0]).astype(np.uint32)
    rm[::17], rm[1::13] = 0, 0xff
    out = []
    for mode in (cr.CRT_TRACE_CLOSEST, cr.CRT_TRACE_ANY):
        for mask in (None, rm):
            out.append(check_against_oracle(cr, ob, sc, rays, mode, mask, a))
    return out[0]


def scene_rays(cr, sc, M, rng, n=4096, n_per=16):
    """tests/test_instances_oracle.py's world rays plus its edge rays, aimed at the scene's own world boxes"""
    return np.concatenate([world_rays(cr.RAY_DT, rng, n, centres=M[:, :, 3]), edge_rays(cr.RAY_DT, rng, sc.world_boxes(), n_per=n_per)])


# ---------------------------------------------------------------- this file's own helpers ----

READS = ("world_to_object", "world_boxes", "tlas_nodes", "instance_records", "blas_nodes", "blas_records", "tlas_child_masks")      # 0..6


def reads(sc):
    return [np.ascontiguousarray(getattr(sc, r)()).view(np.uint8) for r in READS]


def info_fields(sc):
    return {k: v for k, v in sc.info().items() if k not in TIMES}


def assert_equals_fresh(sc, fresh, which=range(7), info=True):
    """every debug read and every info field but the times (info=False: where a refitted BLAS stands beside a freshly built one)"""
    a, b = reads(sc), reads(fresh)
    for k in which:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), READS[k]
    if info:
        assert info_fields(sc) == info_fields(fresh)


def state(sc, rays, rm):
    """everything a refused call must leave: the seven reads, the info fields, a traced batch with stats (closest, any, masked)"""
    out = reads(sc) + [info_fields(sc)]
    for mode, mask in ((0, None), (1, None), (0, rm)):
        h, i, s = sc.trace(rays, mode, stats=True, ray_mask=mask)
        out += [h.view(np.uint8), i, s.view(np.uint8)]
    return out


def assert_state_equal(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x == y) if isinstance(x, dict) else np.array_equal(x, y), k


def one_triangle():
    t = np.zeros((1, 12), np.int32)
    t[0, :3] = (0, 1, 2)
    return np.array([(0.25, 0.5, 0.125), (1.5, 0.25, 0.75), (0.5, 1.75, 1.0)], f32), t


def geometry(m):
    return (m.vertices, m.triangles) if hasattr(m, "vertices") else m


def as_mesh(cr, m):
    """a cr.Mesh of a (vertices, triangles) pair, for the numpy brute force"""
    if hasattr(m, "vertices"):
        return m
    v, t = m
    return cr.Mesh(v, np.zeros((1, 3), f32), np.zeros((0, 2), f32), t, np.zeros((1, 16), f32), np.zeros((0, 18), f32))


def assert_closest_equals_brute_force(cr, sc, meshes, M, mesh_of, rays):
    """closest hits against the numpy brute force per instance over the contract's object rays, reduced by (t, instance, id): every ray"""
    w2o = sc.world_to_object()
    got = sc.trace(rays)
    n = rays.shape[0]
    T = np.full((len(M), n), np.inf)
    TRI = np.full((len(M), n), -1)
    for k in range(len(M)):
        tri, t, u, v = numpy_brute_force(as_mesh(cr, meshes[mesh_of[k]]), object_rays(rays, w2o[k], is_identity(M[k])))
        T[k] = np.where(tri >= 0, t.astype(np.float64), np.inf)
        TRI[k] = tri
    best = np.argmin(T, axis=0)
    cols = np.arange(n)
    hit = np.isfinite(T[best, cols])
    assert hit.sum() > n // 8
    assert np.array_equal(got[1], np.where(hit, best, -1))
    assert np.array_equal(got[0]["tri"], np.where(hit, TRI[best, cols], -1))
    assert np.array_equal(got[0]["t"][hit].view(np.uint32), T[best, cols][hit].astype(f32).view(np.uint32))


def raw_descs(_lib, items):
    """crt_blas_desc array from (vertices or None, n_vertices, triangles or None, n_triangles): for the refusals no Python method reaches"""
    d = (_lib.crt_blas_desc * len(items))()
    for k, (v, nv, t, nt) in enumerate(items):
        d[k].vertices = v.ctypes.data if v is not None else None
        d[k].n_vertices = nv
        d[k].triangles = t.ctypes.data if t is not None else None
        d[k].n_triangles = nt
    return d


# ---------------------------------------------------------------- CPU ----

NEW_SYMBOLS = ("crt_instances_add_meshes", "crt_instances_replace_meshes")


def test_entry_points_are_exported_and_bound(cr):
    from caitlynrenderer_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
        assert getattr(_lib.lib(), n).argtypes is not None, n
    for m in ("add_meshes", "replace_meshes"):
        assert callable(getattr(cr.InstancedScene, m)), m
    assert _lib.lib().crt_abi_version() == 6


def test_null_handle_is_invalid_and_the_message_names_the_call(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    v, t = one_triangle()
    d = raw_descs(_lib, [(v, 3, t, 1)])
    ids = np.zeros(1, np.uint32)
    first = C.c_uint32(77)
    assert L.crt_instances_add_meshes(None, d, 1, C.byref(first)) == _lib.CRT_ERR_INVALID
    assert "crt_instances_add_meshes" in L.crt_last_error().decode()
    assert first.value == 77
    assert L.crt_instances_add_meshes(None, d, 0, None) == _lib.CRT_ERR_INVALID
    assert L.crt_instances_replace_meshes(None, ids.ctypes.data, 1, d) == _lib.CRT_ERR_INVALID
    assert "crt_instances_replace_meshes" in L.crt_last_error().decode()


def test_python_methods_refuse_on_a_closed_handle(cr):
    from caitlynrenderer_amd import _lib
    sc = cr.InstancedScene.__new__(cr.InstancedScene)      # a handle as close() leaves it
    sc._h = C.c_void_p()
    with pytest.raises(cr.CrtError) as e:
        sc.add_meshes([one_triangle()])
    assert e.value.code == _lib.CRT_ERR_INVALID and "crt_instances_add_meshes" in str(e.value)
    with pytest.raises(cr.CrtError) as e:
        sc.replace_meshes({0: one_triangle()})
    assert e.value.code == _lib.CRT_ERR_INVALID and "crt_instances_replace_meshes" in str(e.value)


# ---------------------------------------------------------------- GPU ----

@pytest.fixture(scope="module")
def meshes3(cr, cornell, tess8, tess40):
    return [with_vertices(cr, m, no_negative_zero(m.vertices)) for m in (cornell[0], tess8[0], tess40[0])]


@pytest.fixture(scope="module")
def placed300():
    M, mesh_of = placed_instances(np.random.default_rng(21), 300, 3)
    return M, mesh_of, random_masks(np.random.default_rng(22), 300)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", BYTE_BUILDERS)
def test_two_fresh_creates_are_equal_byte_for_byte(cr, meshes3, placed300, builder):
    """the precondition of every byte comparison below, asserted: the builders named in BYTE_BUILDERS are deterministic"""
    M, mesh_of, masks = placed300
    inst = cr.instances_array(M, mesh_of, masks)
    a = cr.InstancedScene(meshes3, inst, builder=builder)
    b = cr.InstancedScene(meshes3, inst, builder=builder, updatable=True)
    assert_equals_fresh(a, b)
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder,updatable", [("sah", False), ("sah", True), ("lbvh", False), ("ploc", False)])
def test_add_keeps_everything_and_the_new_mesh_can_be_named(cr, ob, meshes3, placed300, builder, updatable):
    M, mesh_of, masks = placed300
    rng = np.random.default_rng(41)
    inst2 = cr.instances_array(M, mesh_of % 2, masks)
    sc = cr.InstancedScene(meshes3[:2], inst2, builder=builder, updatable=updatable)
    rays = scene_rays(cr, sc, M, rng)
    rm = rng.integers(0, 256, rays.shape[0]).astype(np.uint32)
    before = state(sc, rays, rm)
    assert sc.add_meshes([meshes3[2]]) == 2
    after = state(sc, rays, rm)
    for k in (0, 1, 2, 3, 6):
        assert np.array_equal(after[k], before[k]), READS[k]
    for k in (4, 5):
        assert after[k].shape[0] > before[k].shape[0] and np.array_equal(after[k][:before[k].shape[0]], before[k]), READS[k]
    for x, y in zip(after[8:], before[8:]):                  # the traces, stats included, bit for bit
        assert np.array_equal(x, y)
    assert sc.info()["n_meshes"] == 3 and sc.info()["set_wall_ms"] > 0
    byte = builder in BYTE_BUILDERS
    if byte:
        fresh = cr.InstancedScene(meshes3, inst2, builder=builder)
        assert_equals_fresh(sc, fresh)
        fresh.close()
    check_modes(cr, ob, sc, rays, rng)
    # a set, then a refit, naming the new mesh
    inst3 = cr.instances_array(M, mesh_of, masks)
    sc.set(inst3)
    fresh = cr.InstancedScene(meshes3, inst3, builder=builder)
    if byte:
        assert_equals_fresh(sc, fresh)
    ids = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 1000 and np.isin(np.nonzero(mesh_of == 2)[0], ids).any()
    assert_same_closest(sc.trace(rays), fresh.trace(rays))
    M4 = M.copy()
    M4[:, :, 3] += rng.normal(scale=0.3, size=(300, 3)).astype(f32)
    inst4 = cr.instances_array(M4, (mesh_of + 1) % 3, masks)
    sc.refit(inst4)
    fresh.refit(inst4)
    if byte:
        assert_equals_fresh(sc, fresh)
    check_modes(cr, ob, sc, rays, rng)
    assert_same_closest(sc.trace(rays), fresh.trace(rays))
    sc.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slot", [0, 1, 2])
@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_replace_growing_and_shrinking_in_every_slot(cr, ob, meshes3, placed300, builder, slot):
    """tess8 -> tess40's geometry -> back -> one triangle, in the first, middle and last slot (meshes behind it shift)"""
    M, mesh_of, masks = placed300
    cornell, t8, t40 = meshes3
    others = [cornell, t40]
    meshes = others[:slot] + [t8] + others[slot:]
    inst = cr.instances_array(M, mesh_of, masks)
    sc = cr.InstancedScene(meshes, inst, builder=builder, updatable=True)
    rng = np.random.default_rng(50 + slot)
    rays = scene_rays(cr, sc, M, rng)
    sub = world_rays(cr.RAY_DT, np.random.default_rng(23), 8192, centres=M[:, :, 3])[:24]
    for step, new in enumerate((t40, t8, one_triangle())):
        sc.replace_meshes({slot: new})
        meshes = meshes[:slot] + [new] + meshes[slot + 1:]
        fresh = cr.InstancedScene(meshes, inst, builder=builder)
        if builder in BYTE_BUILDERS:
            assert_equals_fresh(sc, fresh)
        else:
            assert_equals_fresh(sc, fresh, which=(0, 1))
        assert_same_closest(sc.trace(rays), fresh.trace(rays))
        fresh.close()
        ids = check_modes(cr, ob, sc, rays, rng)
        assert (ids >= 0).sum() > 1000
        # the brute force costs a second of numpy per ten instances: both ends of the SAH cases, the grown state of the middle slot otherwise
        if (builder == "sah" and step != 1) or (slot == 1 and step == 0):
            assert_closest_equals_brute_force(cr, sc, meshes, M, mesh_of, sub)
    sc.close()


@pytest.mark.gpu
def test_replace_rebuilds_a_decayed_blas(cr, ob, meshes3, placed300):
    M, mesh_of, masks = placed300
    inst = cr.instances_array(M, mesh_of, masks)
    sc = cr.InstancedScene(meshes3, inst, updatable=True)
    ext = float((meshes3[2].vertices.max(0) - meshes3[2].vertices.min(0)).max())
    far = displaced(meshes3[2].vertices, 0.25 * ext, 77)
    moved = meshes3[:2] + [with_vertices(cr, meshes3[2], far)]
    sc.update_meshes({2: far})
    fresh = cr.InstancedScene(moved, inst)
    rng = np.random.default_rng(61)
    rays = scene_rays(cr, sc, M, rng)
    decayed, rebuilt = sc.trace(rays, stats=True), fresh.trace(rays, stats=True)
    assert_same_closest(decayed[:2], rebuilt[:2])
    n_decayed, n_fresh = int(decayed[2]["nodes"].astype(np.int64).sum()), int(rebuilt[2]["nodes"].astype(np.int64).sum())
    print(f"node steps over {rays.shape[0]} rays: refitted tree {n_decayed}, fresh build {n_fresh}")
    assert n_decayed > n_fresh, "the refitted tree has not decayed: the test shows nothing"
    sc.replace_meshes({2: moved[2]})
    assert_equals_fresh(sc, fresh)
    again = sc.trace(rays, stats=True)
    for x, y in zip(again, rebuilt):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    check_modes(cr, ob, sc, rays, rng)
    sc.close(); fresh.close()


@pytest.mark.gpu
def test_refusals_keep_the_state(cr, meshes3, placed300):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    M, mesh_of, masks = placed300
    inst = cr.instances_array(M[:60], mesh_of[:60], masks[:60])
    rng = np.random.default_rng(8)
    rays = world_rays(cr.RAY_DT, rng, 4096, centres=M[:60, :, 3])
    rm = rng.integers(0, 256, rays.shape[0]).astype(np.uint32)
    good = meshes3[1]
    gv, gt = good.vertices, good.triangles

    def refused(sc, before, fn, code=_lib.CRT_ERR_INVALID, words=None):
        with pytest.raises(cr.CrtError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        if words:
            assert words in str(e.value), str(e.value)
        assert_state_equal(state(sc, rays, rm), before)

    def bad_geometries():
        for bad in (np.nan, 1e19):
            v = gv.copy()
            v[len(v) // 2, 1] = bad
            yield (v, gt), "not finite"
        t = gt.copy()
        t[len(t) // 3, 1] = gv.shape[0]
        yield (gv, t), "out of range"
        t = gt.copy()
        t[0, 2] = -1
        yield (gv, t), "out of range"
        yield (gv, gt[:0]), "empty"
        yield (gv[:0], gt), "empty"

    for updatable in (True, False):
        sc = cr.InstancedScene(meshes3, inst, updatable=updatable)
        before = state(sc, rays, rm)
        for geo, words in bad_geometries():
            refused(sc, before, lambda: sc.add_meshes([good, geo]), words=words)          # all or nothing: the good one is not taken either
            if updatable:
                refused(sc, before, lambda: sc.replace_meshes({0: good, 2: geo}), words=words)
        d1 = raw_descs(_lib, [(gv, gv.shape[0], gt, gt.shape[0])])
        d2 = raw_descs(_lib, [(gv, gv.shape[0], gt, gt.shape[0])] * 2)
        for nulls in ((None, gv.shape[0], gt, gt.shape[0]), (gv, gv.shape[0], None, gt.shape[0])):
            dn = raw_descs(_lib, [nulls])
            refused(sc, before, lambda: _lib.check(L.crt_instances_add_meshes(sc._h, dn, 1, None)))
        refused(sc, before, lambda: _lib.check(L.crt_instances_add_meshes(sc._h, None, 1, None)), words="null")
        one = np.array([1], np.uint32)
        if updatable:
            refused(sc, before, lambda: sc.replace_meshes({3: good}), words="out of range")
            two = np.array([1, 1], np.uint32)
            refused(sc, before, lambda: _lib.check(L.crt_instances_replace_meshes(sc._h, two.ctypes.data, 2, d2)), words="repeated")
            refused(sc, before, lambda: _lib.check(L.crt_instances_replace_meshes(sc._h, None, 1, d1)), words="null")
            refused(sc, before, lambda: _lib.check(L.crt_instances_replace_meshes(sc._h, one.ctypes.data, 1, None)), words="null")
            # a world box beyond 1e18: coordinates within the bound that an instance's scale carries past it
            ov, ot = one_triangle()
            big = (ov * f32(5e17)).astype(f32)
            assert np.abs(big).max() < 9e17 and np.abs(M[:60, :, :3]).max() > 1.2
            refused(sc, before, lambda: sc.replace_meshes({1: (big, ot)}), words="1e18")
            assert sc.replace_meshes({}) is None                                           # n == 0: CRT_OK, a no-op
        else:
            refused(sc, before, lambda: sc.replace_meshes({1: good}), words="CRT_INSTANCES_UPDATABLE")
            refused(sc, before, lambda: _lib.check(L.crt_instances_replace_meshes(sc._h, one.ctypes.data, 0, None)), words="CRT_INSTANCES_UPDATABLE")
        assert sc.add_meshes([]) == 3                                                      # n == 0: CRT_OK, a no-op, the next index
        assert_state_equal(state(sc, rays, rm), before)
        assert sc.add_meshes([good]) == 3                                                  # the handle still takes a call
        sc.close()


@pytest.mark.gpu
def test_stack_limit_refuses_both_calls_and_keeps_the_state(cr):
    """a deep TLAS over a shallow mesh: adding a deep mesh, or replacing the shallow mesh by it, would carry TLAS depth + deepest BLAS
    beyond the walk's 40 entries"""
    from caitlynrenderer_amd import _lib
    V, T = clustered_mesh(30)
    shallow = clustered_mesh(1)
    probe = cr.InstancedScene([(V, T)], cr.instances_array(clustered_instances(1), np.zeros(8)))
    db = probe.info()["max_blas_depth8"]
    probe.close()
    assert 20 <= db <= 38
    K = 48 - db
    deep = cr.instances_array(clustered_instances(K), np.zeros(8 * K))
    sc = cr.InstancedScene([shallow], deep, updatable=True)
    info = sc.info()
    assert info["stack_entries"] <= 40 and info["tlas_depth8"] + db > 40, (info, db)
    rng = np.random.default_rng(4)
    rays = np.zeros(4096, cr.RAY_DT)
    rays["o"][:, 0] = rng.uniform(0.0, 40.0, 4096).astype(f32)
    rays["o"][:, 1] = rng.uniform(0.0, 0.5, 4096).astype(f32)
    rays["o"][:, 2] = f32(5.0)
    rays["d"] = np.array([0.0, 0.0, -1.0], f32)
    rays["tmax"] = f32(1e9)
    rm = rng.integers(0, 256, 4096).astype(np.uint32)
    before = state(sc, rays, rm)
    assert (before[9] >= 0).sum() > 50
    for fn in (lambda: sc.add_meshes([(V, T)]), lambda: sc.replace_meshes({0: (V, T)})):
        with pytest.raises(cr.CrtError) as e:
            fn()
        assert e.value.code == _lib.CRT_ERR_LIMIT, str(e.value)
        assert_state_equal(state(sc, rays, rm), before)
    # the same calls under a shallow TLAS are taken
    sc.set(deep[:8])
    assert sc.add_meshes([(V, T)]) == 1
    sc.replace_meshes({0: (V, T)})
    assert sc.info()["max_blas_depth8"] == db and sc.info()["stack_entries"] <= 40
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "ploc", "lbvh"])
def test_updatable_state_follows(cr, meshes3, builder):
    """after an add and after a replace, update_meshes on the new / replaced mesh and on a shifted neighbour equals crt_cwbvh_refit of
    that BLAS byte for byte, as test_instances_update.py::test_refit_equals_the_host_refit_byte_for_byte checks it"""
    rng = np.random.default_rng(3)
    M, _ = placed_instances(rng, 6, 3)
    sc = cr.InstancedScene(meshes3[:2], cr.instances_array(M, [0, 1, 0, 1, 0, 1]), builder=builder, updatable=True)
    sc.update_meshes({0: meshes3[0].vertices})
    bytes0 = sc.last_update()["state_bytes"]
    assert sc.add_meshes([meshes3[2]]) == 2
    assert sc.last_update()["state_bytes"] > bytes0
    sc.set(cr.instances_array(M, [0, 1, 2, 0, 1, 2]))
    meshes = list(meshes3)

    def update_and_compare(upd, seed):
        lay = blas_layout(sc, meshes)
        nodes0, recs0, w2o0 = sc.blas_nodes(), sc.blas_records(), sc.world_to_object()
        new = {k: displaced(meshes[k].vertices, a, seed + k) for k, a in upd.items()}
        sc.update_meshes(new)
        nodes1, recs1 = sc.blas_nodes(), sc.blas_records()
        for k, m in enumerate(meshes):
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

    update_and_compare({2: 0.03, 1: 0.05}, 10)             # the added mesh and its neighbour
    # mesh 0 takes tess40's geometry: meshes 1 and 2 shift
    meshes[0] = meshes3[2]
    sc.replace_meshes({0: meshes[0]})
    update_and_compare({0: 0.02, 1: 0.04}, 20)             # the replaced mesh and a shifted neighbour
    update_and_compare({2: 0.02}, 30)                      # the other shifted mesh alone
    # shrinking: mesh 1 becomes the Cornell box, mesh 2 shifts down
    meshes[1] = meshes3[0]
    sc.replace_meshes({1: meshes[1]})
    update_and_compare({1: 0.1, 2: 0.02}, 40)
    t = sc.last_update()
    assert t["device_ms"] > 0 and t["wall_ms"] > 0
    sc.close()


@pytest.mark.gpu
def test_interleaved_calls(cr, ob, meshes3, placed300):
    """add, set, refit, replace, update, masked trace, refused replace, add again: the oracle after every step, a fresh create at the end"""
    from caitlynrenderer_amd import _lib
    M, mesh_of, masks = placed300
    rng = np.random.default_rng(71)
    A = cr.instances_array(M[:120], mesh_of[:120] % 2, masks[:120])
    sc = cr.InstancedScene(meshes3[:2], A, capacity=300, updatable=True)
    rays = scene_rays(cr, sc, M, rng)
    meshes = list(meshes3[:2])
    check_modes(cr, ob, sc, rays, rng)
    assert sc.add_meshes([meshes3[2]]) == 2                                      # add
    meshes.append(meshes3[2])
    check_modes(cr, ob, sc, rays, rng)
    B = cr.instances_array(M[100:300], mesh_of[100:300], masks[100:300])
    sc.set(B)                                                                    # set
    check_modes(cr, ob, sc, rays, rng)
    MB = M[100:300].copy()
    MB[:, :, 3] += rng.normal(scale=0.4, size=(200, 3)).astype(f32)
    B = cr.instances_array(MB, mesh_of[100:300], masks[100:300])
    sc.refit(B)                                                                  # refit
    check_modes(cr, ob, sc, rays, rng)
    meshes[0] = meshes3[2]
    sc.replace_meshes({0: meshes[0]})                                            # replace (the first slot grows: every other mesh shifts)
    check_modes(cr, ob, sc, rays, rng)
    v1 = displaced(meshes[1].vertices, 0.06, 72)
    sc.update_meshes({1: v1})                                                    # update of a shifted mesh
    meshes[1] = with_vertices(cr, meshes[1], v1)
    ids = check_modes(cr, ob, sc, rays, rng)                                     # masked traces among them
    assert (ids >= 0).sum() > 1000
    before = state(sc, rays, masks[0])
    bad = meshes3[1].vertices.copy()
    bad[7, 0] = np.inf
    with pytest.raises(cr.CrtError) as e:
        sc.replace_meshes({2: meshes3[0], 1: (bad, meshes3[1].triangles)})       # refused replace
    assert e.value.code == _lib.CRT_ERR_INVALID
    assert_state_equal(state(sc, rays, masks[0]), before)
    check_modes(cr, ob, sc, rays, rng)
    assert sc.add_meshes([one_triangle(), meshes3[0]]) == 3                      # add again, two at once
    meshes += [one_triangle(), meshes3[0]]
    check_modes(cr, ob, sc, rays, rng)
    C5 = cr.instances_array(MB, (mesh_of[100:300] + np.arange(200)) % 5, masks[100:300])
    sc.set(C5)
    ids = check_modes(cr, ob, sc, rays, rng)
    fresh = cr.InstancedScene(meshes, C5, capacity=300)
    assert_equals_fresh(sc, fresh, which=(0, 1), info=False)      # mesh 1 is a refitted tree here and a built one there
    assert_same_closest(sc.trace(rays), fresh.trace(rays))
    assert sc.info()["n_meshes"] == 5 and fresh.info()["blas_tris"] == sc.info()["blas_tris"]
    sc.close(); fresh.close()


@pytest.mark.gpu
def test_add_and_replace_beside_the_million_triangle_mesh(cr, ob, cornell, meshes3):
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
    sc = cr.InstancedScene([mesh], cr.instances_array(M, np.zeros(64)), capacity=80, updatable=True)
    nodes0, recs0 = sc.blas_nodes(), sc.blas_records()
    assert sc.add_meshes([meshes3[1]]) == 1
    t_add = sc.info()["set_wall_ms"]
    # the small mesh between the big ones
    M2 = np.concatenate([M, M[:16]])
    M2[64:, :, 3] += f32(0.75 * ext) * np.array([1, 1, 0], f32)
    inst = cr.instances_array(M2, np.concatenate([np.zeros(64), np.ones(16)]))
    sc.set(inst)
    rays = world_rays(cr.RAY_DT, rng, 20000, spread=6 * ext, centres=M2[:, :, 3])
    rays["o"] += f32(5.25 * ext) * np.array([1, 1, 0], f32)
    rays = np.concatenate([rays, edge_rays(cr.RAY_DT, rng, sc.world_boxes(), n_per=8)])
    for step in range(2):
        nodes1, recs1 = sc.blas_nodes(), sc.blas_records()
        assert np.array_equal(nodes1[:nodes0.shape[0]], nodes0) and np.array_equal(recs1[:recs0.shape[0]].view(np.uint8), recs0.view(np.uint8))
        assert nodes1.shape[0] > nodes0.shape[0]
        a = device_arrays(ob, sc)
        ids = check_against_oracle(cr, ob, sc, rays, cr.CRT_TRACE_CLOSEST, None, a)
        check_against_oracle(cr, ob, sc, rays, cr.CRT_TRACE_ANY, rng.integers(0, 256, rays.shape[0]), a)
        assert (ids >= 0).sum() > 4000 and (ids >= 64).sum() > 50
        if step == 0:
            sc.replace_meshes({1: meshes3[0]})
            print(f"beside the 1 M-triangle mesh: add {t_add:.2f} ms, replace {sc.info()['set_wall_ms']:.2f} ms wall")
    sc.close()
