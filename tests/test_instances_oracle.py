"""The two-level walk of instanced scenes held to a CPU oracle (oracle/oracle.c orc_trace_instances), counts included.

Without a GPU the oracle itself is checked against references that share no walk code with it, on instanced scenes assembled on the host
exactly as the device lays them out: closest hits against the numpy brute force over object rays, one identity instance against the
flat CWBVH walk (bvh8_walk) step for step, masked walks against unmasked walks of the visible instances, any hits against the brute
force, and the stack bound (TLAS depth + deepest BLAS depth) against a scene built to reach it.

On the GPU, k_trace_instances is compared byte for byte (hits, instance ids, per-ray node and triangle counts) with the oracle fed the
handle's own debug reads, over builders, states (refit, update, sets, refused sets), closest / any, masked or not, edge-case rays and
ray counts around the 64-ray pool.  Every comparison also checks the stack: the oracle's deepest use within info()["stack_entries"],
no push or instance entry refused, no stack overflow counted on the device.  The helpers of tests/test_instances*.py are restated here."""
import numpy as np
import pytest

from conftest import numpy_brute_force

f32 = np.float32
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
THREADS = 16


# ---------------------------------------------------------------- restated helpers ----

def is_identity(m):
    return np.array_equal(np.asarray(m, np.float32).reshape(12).view(np.uint32), IDENTITY.reshape(12).view(np.uint32))


def object_rays(rays, w, identity):
    """the world -> object ray of the contract: fp32, no fma, in the stated order; bitwise-identity instances keep the ray"""
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


def random_matrix(rng, spread, scale=(0.5, 2.0)):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    s = rng.uniform(*scale, 3) * rng.choice([-1.0, 1.0], 3)
    return np.concatenate([q @ np.diag(s), rng.uniform(-spread, spread, (3, 1))], 1)


def placed_instances(rng, n, n_meshes, spread=12.0, scale=(0.5, 2.0)):
    return np.array([random_matrix(rng, spread, scale) for _ in range(n)], f32), rng.integers(0, n_meshes, n)


def special_matrices(rng, n, spread=12.0):
    """signed axis permutations (object directions of axis-aligned world rays are then exact signed zeros), mirrors, shears and identities
    with a translation, in turn"""
    out = []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            A = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3) * rng.choice([0.5, 1.0, 2.0])
        elif kind == 1:
            A = np.diag(rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 2.0, 3))
            A[rng.integers(0, 3)] *= -1.0
        elif kind == 2:
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            S = np.eye(3)
            S[0, 1], S[1, 2], S[0, 2] = rng.uniform(-0.6, 0.6, 3)
            A = q @ S
        else:
            A = np.eye(3)
        out.append(np.concatenate([A, rng.uniform(-spread, spread, (3, 1))], 1))
    return np.array(out, f32)


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
    """Rays where walks go wrong, aimed at the given world boxes (lo, hi): signed and exact zero direction components, axis-aligned rays
    (through signed-permutation and mirrored instances their object directions are exact signed zeros), origins inside the boxes,
    non-finite origins, a finite origin whose object origin overflows (far: beyond the grazing margin's bound, so against the kernel
    only), tmax 0, the smallest denormal and +inf."""
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
    # axis-aligned, from outside along the axis, through a box centre
    for a in axes:
        c = pick(n_per)
        out.append(rays(c - 40.0 * a, np.broadcast_to(a, c.shape)))
    # signed / exact zero components from random origins towards boxes, the component zeroed after aiming
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
    # origins inside the boxes
    lo, hi = boxes[:, :3], boxes[:, 3:]
    k = rng.integers(0, len(boxes), 4 * n_per)
    o = lo[k] + (hi[k] - lo[k]) * rng.random((4 * n_per, 3))
    d = rng.normal(size=o.shape)
    out.append(rays(o, d / np.linalg.norm(d, axis=1, keepdims=True)))
    # non-finite origins; a finite origin far out whose object origin overflows under a scale > 1
    bad = rays(pick(6), np.tile(np.array([[0.0, 0.0, 1.0]], f32), (6, 1)))
    bad["o"][0, 0] = np.nan; bad["o"][1, 1] = np.inf; bad["o"][2, 2] = -np.inf
    bad["o"][3] = (np.nan, np.nan, np.nan); bad["d"][4] = (np.nan, 0, 1); bad["d"][5] = (np.inf, 0, 0)
    out.append(bad)
    far_rays = rays(np.tile(np.array([[3.3e38, 0.0, 0.0]], f32), (n_per, 1)), np.tile(np.array([[-1.0, 0.0, 0.0]], f32), (n_per, 1)), np.inf)
    far_rays["o"][:, 1:] = pick(n_per)[:, 1:]
    if far:
        out.append(far_rays)
    # tmax 0, the smallest denormal and +inf, from outside towards boxes
    for tmax in (0.0, np.float32(1e-45), np.inf):
        c = pick(n_per)
        o = c + rng.normal(scale=10.0, size=c.shape)
        d = c - o
        out.append(rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), tmax))
    # tmax 0 / denormal with origins inside: every t >= 0 is refused or nearly
    for tmax in (0.0, np.float32(1e-45)):
        k = rng.integers(0, len(boxes), n_per)
        o = lo[k] + (hi[k] - lo[k]) * rng.random((n_per, 3))
        d = rng.normal(size=o.shape)
        out.append(rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), tmax))
    return np.concatenate(out)


def records(leaf_tris, ids, slots, V):
    """BLAS intersection records (v0 | id) (e1 | slot) (e2 | material) of the given slots, as the device gathers them"""
    t = leaf_tris[slots]
    v0, v1, v2 = V[t[:, 0]], V[t[:, 1]], V[t[:, 2]]
    r = np.zeros((slots.shape[0], 12), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 8:11] = v0, (v1 - v0).astype(np.float32), (v2 - v0).astype(np.float32)
    r[:, 3], r[:, 7], r[:, 11] = ids[slots].view(np.float32), slots.astype(np.int32).view(np.float32), t[:, 3].view(np.float32)
    return r


def depth8(nodes):
    """node8 levels below and including the root (root = 1), following the inner children"""
    nodes = np.asarray(nodes, np.uint8).reshape(-1, 80)
    if nodes.shape[0] == 0:
        return 0
    best, todo = 0, [(0, 1)]
    while todo:
        i, lv = todo.pop()
        best = max(best, lv)
        imask, base = int(nodes[i, 15]), int(nodes[i, 16:20].view(np.uint32)[0])
        todo += [(base + k, lv + 1) for k in range(bin(imask).count("1"))]
    return best


# ---------------------------------------------------------------- host assembly of an instanced scene ----

def host_blas(cr, mesh):
    """one mesh's BLAS on the host: SBVH, CWBVH, records in CWBVH order; + the SceneData of the same tree (for the flat oracle)"""
    sb = cr.SBVH(mesh.triangles, mesh.vertices)
    cw = cr.CWBVH().convert(sb)
    recs = records(sb.triangles, sb.triangle_indices, cw.tri_slots, mesh.vertices)
    return cw.nodes, recs, cr.SceneData(mesh, sb, cw, None)


def mesh_box(mesh):
    V = mesh.vertices[mesh.triangles[:, :3].reshape(-1)]
    return np.concatenate([V.min(0), V.max(0)]).astype(f32)


def median_split_bvh2(boxes, leaf_size=2):
    """a small BVH2 over boxes (crt_flatnode rows: lo, first / left, hi, count / 0), children adjacent; -> (flat, leaf order)"""
    n = boxes.shape[0]
    order = np.arange(n)
    cen = (boxes[:, :3].astype(np.float64) + boxes[:, 3:]) / 2
    flat = [None]
    todo = [(0, 0, n)]
    while todo:
        i, a, b = todo.pop()
        idx = order[a:b]
        lo, hi = boxes[idx, :3].min(0), boxes[idx, 3:].max(0)
        if b - a <= leaf_size:
            flat[i] = [*lo, a, *hi, b - a]
            continue
        ext = cen[idx].max(0) - cen[idx].min(0)
        ax = int(np.argmax(ext))
        order[a:b] = idx[np.argsort(cen[idx, ax], kind="stable")]
        m = (a + b) // 2
        left = len(flat)
        flat += [None, None]
        flat[i] = [*lo, left, *hi, 0]
        todo += [(left, a, m), (left + 1, m, b)]
    return np.array(flat, np.float32), order


def host_scene(cr, blases, M, mesh_of, masks=None, capacity=None, index=None):
    """The arrays k_trace_instances reads, assembled on the host as the device lays them out: TLAS node8s from a median-split BVH2 over
    the world boxes, instance records in TLAS leaf order, the BLASes packed behind a TLAS region of max(capacity, 1) node8s with their
    child and triangle bases rebased (k_rebase_nodes).  index: the instance index each record carries (default 0..n-1)."""
    n = len(M)
    masks = np.zeros(n, np.uint32) if masks is None else np.asarray(masks, np.uint32)
    index = np.arange(n) if index is None else np.asarray(index)
    region = max(n if capacity is None else capacity, 1)
    roots, packed, recs, node_off, tri_off = [], [], [], region, 0
    for nodes, r, _ in blases:
        nd = nodes.copy()
        nd[:, 16:20] = (nd[:, 16:20].copy().view(np.uint32) + np.uint32(node_off)).view(np.uint8)
        nd[:, 20:24] = (nd[:, 20:24].copy().view(np.uint32) + np.uint32(tri_off)).view(np.uint8)
        roots.append(node_off)
        packed.append(nd); recs.append(r)
        node_off += nodes.shape[0]; tri_off += r.shape[0]
    rec = np.zeros((n, 16), np.float32)
    boxes = np.zeros((n, 6), np.float32)
    for k in range(n):
        rec[k, :12] = cr.instance_inverse(M[k])
        rec[k, 12:].view(np.uint32)[:] = (roots[mesh_of[k]], index[k], 1 if is_identity(M[k]) else 0, masks[k] & 0xff)
        boxes[k] = cr.instance_world_box(M[k], mesh_box(blases[mesh_of[k]][2]))
    if n == 0:
        tlas, inst = np.zeros((0, 80), np.uint8), rec
    else:
        if n == 1:
            flat, order = np.array([[*boxes[0, :3], 0, *boxes[0, 3:], 1]], np.float32), np.arange(1)
        else:
            flat, order = median_split_bvh2(boxes)
        cw = cr.CWBVH().convert_arrays(flat, n)
        tlas, inst = cw.nodes, rec[order[cw.tri_slots]]
    blas_depth = max(depth8(b[0]) for b in blases)
    return dict(tlas=tlas, inst=inst, blas=np.concatenate(packed), blas_recs=np.concatenate(recs), region=region,
                stack=max(2, depth8(tlas) + blas_depth), tlas_depth=depth8(tlas), blas_depth=blas_depth)


def orc(ob, s, rays, mode=0, masked=False):
    return ob.trace_instances(s["tlas"], s["inst"], s["blas"], s["blas_recs"], rays, s["region"], s["stack"],
                              mode | (ob.INSTANCE_MASK if masked else 0), threads=THREADS)


def brute_force(meshes, M, mesh_of, rays, index=None):
    """per instance: the numpy brute force over its object rays; -> T (instances x rays, inf = no hit), TRI, U, V"""
    n = rays.shape[0]
    T = np.full((len(M), n), np.inf)
    TRI, U, V = np.full((len(M), n), -1), np.zeros((len(M), n), f32), np.zeros((len(M), n), f32)
    for k in range(len(M)):
        orays = object_rays(rays, np.asarray(M_inv(M[k])), is_identity(M[k]))
        fin = np.isfinite(orays["o"]).all(1)
        tri, t, u, v = numpy_brute_force(meshes[mesh_of[k]], orays)
        tri = np.where(fin, tri, -1)
        T[k] = np.where(tri >= 0, t.astype(np.float64), np.inf)
        TRI[k], U[k], V[k] = tri, u, v
    return T, TRI, U, V


_INV = {}


def M_inv(m):
    import caitlynrenderer_amd as cr
    key = np.asarray(m, f32).tobytes()
    if key not in _INV:
        _INV[key] = cr.instance_inverse(m)
    return _INV[key]


def brute_closest(T, TRI, U, V):
    """the minimum of (t, instance, id): argmin takes the first (lowest) instance of equal t; the brute force the lowest id within"""
    n = T.shape[1]
    best = np.argmin(T, axis=0)
    hit = np.isfinite(T[best, np.arange(n)])
    cols = np.arange(n)
    return (np.where(hit, best, -1), np.where(hit, TRI[best, cols], -1), T[best, cols].astype(f32), U[best, cols], V[best, cols])


def assert_closest_is(hits, ids, want):
    inst, tri, t, u, v = want
    assert np.array_equal(ids, inst), np.nonzero(ids != inst)[0][:10]
    assert np.array_equal(hits["tri"], tri)
    h = tri >= 0
    for got, w in ((hits["t"], t), (hits["u"], u), (hits["v"], v)):
        assert np.array_equal(got[h].view(np.uint32), w[h].view(np.uint32))


def host_rays(cr, rng, M, n):
    rays = world_rays(cr.RAY_DT, rng, n, centres=M[:, :, 3])
    rays["tmax"][1::11] = np.inf
    return rays


# ---------------------------------------------------------------- CPU: the oracle against independent references ----

@pytest.fixture(scope="module")
def small_meshes(cr, cornell, tess8):
    return [cornell[0], tess8[0]]


@pytest.fixture(scope="module")
def small_blases(cr, small_meshes):
    return [host_blas(cr, m) for m in small_meshes]


@pytest.mark.parametrize("family", ["rotations", "signed_permutations", "mirrors_shears"])
def test_oracle_closest_hits_equal_the_brute_force(cr, ob, small_meshes, small_blases, family):
    rng = np.random.default_rng({"rotations": 1, "signed_permutations": 2, "mirrors_shears": 3}[family])
    n = 24
    if family == "rotations":
        M, mesh_of = placed_instances(rng, n, 2, spread=6.0)
    else:
        M = special_matrices(rng, 4 * n, spread=6.0)
        M = M[[k for k in range(4 * n) if (k % 4 == 0) == (family == "signed_permutations")][:n]]
        mesh_of = rng.integers(0, 2, n)
    s = host_scene(cr, small_blases, M, mesh_of)
    rays = np.concatenate([host_rays(cr, rng, M, 160), edge_rays(cr.RAY_DT, rng, [cr.instance_world_box(M[k], mesh_box(small_meshes[mesh_of[k]]))
                                                                                    for k in range(n)], n_per=4, far=False)])
    hits, ids, st, depth, refused = orc(ob, s, rays)
    want = brute_closest(*brute_force(small_meshes, M, mesh_of, rays))
    assert (want[0] >= 0).sum() > 60
    assert_closest_is(hits, ids, want)
    assert depth.max() <= s["stack"] and refused.sum() == 0
    # node steps >= 1 for every finite ray (the TLAS root), none for a non-finite origin
    fin = np.isfinite(rays["o"]).all(1)
    assert (st["nodes"][fin] >= 1).all() and (st["nodes"][~fin] == 0).all() and (st["tris"][~fin] == 0).all()


def test_oracle_identity_instance_walks_the_flat_tree(cr, ob, cornell, tess8):
    """one identity instance of a mesh walks the mesh's own CWBVH: the flat oracle's hits, nodes + 1 (the TLAS root), equal triangle
    tests; any hits equal too"""
    mesh = tess8[0]
    blas = host_blas(cr, mesh)
    s = host_scene(cr, [blas], IDENTITY[None], [0])
    flat = ob.Oracle(blas[2], 8, 8)
    rng = np.random.default_rng(5)
    lo, hi = mesh.vertices.min(0), mesh.vertices.max(0)
    rays = np.zeros(4000, cr.RAY_DT)
    rays["o"] = (lo + (hi - lo) * rng.random((4000, 3))).astype(f32)
    d = rng.normal(size=(4000, 3))
    rays["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    rays["tmax"] = f32(1e9)
    rays = np.concatenate([rays, edge_rays(cr.RAY_DT, rng, [np.concatenate([lo, hi])], n_per=16)])
    for mode in (ob.CLOSEST, ob.ANY):
        want, wst = flat.trace(rays, ob.BVH8, mode, ob.TIE_LOWEST_ID, stats=True)
        hits, ids, st, _, _ = orc(ob, s, rays, mode)
        assert np.array_equal(hits.view(np.uint8), want.view(np.uint8)), mode
        assert np.array_equal(ids, np.where(want["tri"] >= 0, 0, -1))
        # a ray that enters the instance walks the flat tree behind the TLAS root; one that misses the root's one box (the padded world
        # box) is a ray that the flat walk stops at its root as well
        entered = st["nodes"] > 1
        assert entered.sum() > 3000
        assert np.array_equal(st["nodes"][entered], wst["nodes"][entered].astype(np.int64) + 1)
        assert np.array_equal(st["tris"][entered], wst["tris"][entered])
        fin = np.isfinite(rays["o"]).all(1)
        assert (st["nodes"][~entered & fin] == 1).all() and (st["tris"][~entered] == 0).all()
        assert (wst["nodes"][~entered & fin] == 1).all() and (wst["tris"][~entered] == 0).all()
    assert (want["tri"] >= 0).sum() > 2000


def test_oracle_masked_walk_equals_the_unmasked_walk_of_the_visible_instances(cr, ob, small_meshes, small_blases):
    rng = np.random.default_rng(11)
    n = 40
    M, mesh_of = placed_instances(rng, n, 2, spread=6.0)
    masks = rng.integers(0, 256, n).astype(np.uint32)
    masks[:3] = (0, 0x80, 0xff)
    s = host_scene(cr, small_blases, M, mesh_of, masks)
    rays = host_rays(cr, rng, M, 3000)
    ray_masks = np.array([0, 1, 0x80, 0xff, 0x24, int(masks[5])], np.uint32)
    rays["pad"] = ray_masks[np.arange(rays.shape[0]) % len(ray_masks)]
    n_hidden = 0
    for mode in (ob.CLOSEST, ob.ANY):
        hits, ids, st, depth, refused = orc(ob, s, rays, mode, masked=True)
        assert depth.max() <= s["stack"] and refused.sum() == 0
        for rm in ray_masks:
            sel = rays["pad"] == rm
            vis = np.nonzero(masks & rm)[0]
            if vis.size == 0:
                assert (ids[sel] == -1).all() and (hits["tri"][sel] == -1).all()
                assert (st["nodes"][sel] <= 1).all() and (st["tris"][sel] == 0).all()      # the root only: every child culled
                continue
            sub = host_scene(cr, small_blases, M[vis], mesh_of[vis], masks[vis], index=vis)
            whits, wids, _, _, _ = orc(ob, sub, rays[sel], mode)
            if mode == ob.CLOSEST:
                assert np.array_equal(hits[sel].view(np.uint8), whits.view(np.uint8)), rm
                assert np.array_equal(ids[sel], wids), rm
            else:
                assert np.array_equal(hits["tri"][sel], whits["tri"]), rm
                assert np.isin(ids[sel][ids[sel] >= 0], vis).all()
            n_hidden += n - vis.size
        # a mask that hides nothing gives the unmasked walk's bytes, counts included
        full = rays["pad"] == 0xff
        u = orc(ob, host_scene(cr, small_blases, M, mesh_of, np.full(n, 0xff)), rays[full], mode)
        m = orc(ob, host_scene(cr, small_blases, M, mesh_of, np.full(n, 0xff)), rays[full], mode, masked=True)
        for a, b in zip(u[:3], m[:3]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert n_hidden > 0


def reversed_ids(cr, mesh):
    """the same triangles, ids reversed: a coincident instance of it ties every t of the original with a different triangle id"""
    return cr.Mesh(mesh.vertices, mesh.normals, mesh.texcoords, mesh.triangles[::-1].copy(), mesh.materials, mesh.lights)


def test_oracle_ties_across_instances_go_to_the_lower_index(cr, ob, cornell):
    """coincident instances (the same mesh, or the same triangles with reversed ids, under the same matrix) in both orders: each hit is
    a t tie between two instances, which the lower instance index wins, then the lower id"""
    meshes = [cornell[0], reversed_ids(cr, cornell[0])]
    blases = [host_blas(cr, m) for m in meshes]
    rng = np.random.default_rng(14)
    P, _ = placed_instances(rng, 4, 1, spread=6.0)
    M = np.concatenate([P[[0, 0, 1, 1, 2, 2, 3, 3]]])
    mesh_of = np.array([0, 1, 1, 0, 0, 0, 1, 1])
    s = host_scene(cr, blases, M, mesh_of)
    rays = host_rays(cr, rng, P, 600)
    hits, ids, _, _, _ = orc(ob, s, rays)
    want = brute_closest(*brute_force(meshes, M, mesh_of, rays))
    assert_closest_is(hits, ids, want)
    assert (ids >= 0).sum() > 100 and set(np.unique(ids[ids >= 0])) <= {0, 2, 4, 6}
    for k in (0, 2):                                     # the two orders of a mesh and its reversed-id copy: the lower index wins
        sel = ids == k
        assert sel.sum() > 10 and (want[1][sel] == hits["tri"][sel]).all()


def test_oracle_child_masks_are_the_or_of_the_instances_below(cr, ob, small_blases):
    """tlas_child_masks against a second restatement: every instance's mask ORed up its leaf-to-root path"""
    rng = np.random.default_rng(12)
    M, mesh_of = placed_instances(rng, 57, 2)
    masks = (1 << rng.integers(0, 8, 57)).astype(np.uint32)
    s = host_scene(cr, small_blases, M, mesh_of, masks)
    nodes, inst = s["tlas"], s["inst"]
    want = np.zeros((nodes.shape[0], 8), np.uint8)
    parent = {}
    for i in range(nodes.shape[0]):
        imask, base = int(nodes[i, 15]), int(nodes[i, 16:20].view(np.uint32)[0])
        for slot in range(8):
            if (imask >> slot) & 1:
                parent[base + bin(imask & ((1 << slot) - 1)).count("1")] = (i, slot)
    for i in range(nodes.shape[0]):
        imask, ib = int(nodes[i, 15]), int(nodes[i, 20:24].view(np.uint32)[0])
        for slot in range(8):
            meta = int(nodes[i, 24 + slot])
            if not (imask >> slot) & 1 and meta:
                for p in range(ib + (meta & 31), ib + (meta & 31) + bin(meta >> 5).count("1")):
                    m = int(inst[p, 15:16].view(np.uint32)[0])
                    node, sl = i, slot
                    while True:
                        want[node, sl] |= m
                        if node not in parent:
                            break
                        node, sl = parent[node]
    got = ob.tlas_child_masks(nodes, inst)
    assert np.array_equal(got, want) and got.any()


def test_oracle_any_hit_reports_an_instance_with_a_hit(cr, ob, small_meshes, small_blases):
    rng = np.random.default_rng(13)
    n = 24
    M, mesh_of = placed_instances(rng, n, 2, spread=6.0)
    s = host_scene(cr, small_blases, M, mesh_of)
    rays = host_rays(cr, rng, M, 200)
    hits, ids, st, _, _ = orc(ob, s, rays, ob.ANY)
    T, _, _, _ = brute_force(small_meshes, M, mesh_of, rays)
    occ = np.isfinite(T).any(0)
    assert occ.sum() > 60 and (~occ).sum() > 20
    assert np.array_equal(hits["tri"] >= 0, occ) and np.array_equal(ids >= 0, occ)
    assert np.isfinite(T[ids[occ], np.nonzero(occ)[0]]).all()          # the reported instance has a hit with t < tmax
    assert (hits["t"] == 0).all() and (hits["u"] == 0).all() and (hits["v"] == 0).all()
    _, cids, _, _, _ = orc(ob, s, rays, ob.CLOSEST)
    assert np.array_equal(cids >= 0, occ)


def grid_mesh(G, h=0.25):
    """G x G unit cells in the z = 0 .. h slab, two triangles per cell, each tilted across the whole slab: every node box is h thick
    whichever triangles a builder groups, and a ray in the plane z = h / 2 crosses a line of boxes at every level"""
    V, T = [], []
    for i in range(G):
        for j in range(G):
            b = len(V)
            V += [(i, j, 0.0), (i + 1, j, 0.0), (i, j + 1, h), (i + 1, j + 1, h), (i, j + 1, h), (i + 1, j, 0.0)]
            T += [(b, b + 1, b + 2), (b + 3, b + 4, b + 5)]
    t = np.zeros((len(T), 12), np.int32)
    t[:, :3] = T
    return np.array(V, f32), t


def grid_instances(G, cell):
    """G x G translated copies in the same slab, `cell` apart"""
    M = []
    for i in range(G):
        for j in range(G):
            M.append(np.concatenate([np.eye(3), np.array([[cell * i], [cell * j], [0.0]])], 1))
    return np.array(M, f32)


def grazing_plane_rays(rays_dt, rng, extent, n, z):
    """rays in the plane z = const across the whole grid at random angles and offsets: every TLAS and BLAS level keeps several siblings
    pending, and the TLAS leaves several instances"""
    a = rng.uniform(0, 2 * np.pi, n)
    c = rng.uniform(0.2 * extent, 0.8 * extent, (n, 2))
    d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)
    r = np.zeros(n, rays_dt)
    r["o"][:, :2] = c - 2.0 * extent * d[:, :2]
    r["o"][:, 2] = z
    r["d"] = d.astype(f32)
    r["tmax"] = f32(1e9)
    return r


def test_oracle_reaches_the_stack_bound_on_a_worst_case_scene(cr, ob):
    """The stack bound TLAS depth + deepest BLAS depth is exact: a TLAS node at depth k is visited with k - 1 entries at most, entering
    an instance adds the rest of the node group, the rest of the leaf group and the return marker (at most depth + 1 in all, since the
    deepest level has no node group), and the BLAS walk adds its depth - 1.  In-plane rays over a grid of grid meshes keep a sibling
    pending at every level and reach it."""
    V, T = grid_mesh(16)
    mesh = cr.Mesh(V, np.zeros((1, 3), f32), np.zeros((0, 2), f32), T, np.zeros((1, 16), f32), np.zeros((0, 18), f32))
    blas = host_blas(cr, mesh)
    M = grid_instances(8, 17.0)
    s = host_scene(cr, [blas], M, np.zeros(len(M), int))
    rng = np.random.default_rng(17)
    rays = grazing_plane_rays(cr.RAY_DT, rng, 8 * 17.0, 2000, 0.125)
    _, _, _, depth, refused = orc(ob, s, rays, ob.CLOSEST)
    assert refused.sum() == 0
    assert s["tlas_depth"] >= 2 and s["blas_depth"] >= 3, (s["tlas_depth"], s["blas_depth"])
    assert depth.max() == s["stack"], (depth.max(), s["stack"], s["tlas_depth"], s["blas_depth"])
    # one entry fewer refuses something on the same rays
    s1 = dict(s, stack=s["stack"] - 1)
    _, _, _, d1, r1 = orc(ob, s1, rays, ob.CLOSEST)
    assert d1.max() <= s["stack"] - 1 and r1.sum() > 0


# ---------------------------------------------------------------- GPU: k_trace_instances against the oracle, byte for byte ----

def device_arrays(ob, sc):
    """What the walk reads, through the handle's debug reads; the TLAS region's size from info() (tlas_bytes), checked against the
    capacity; the child masks restated on the host (a plain OR) and compared with the device's"""
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
    """One trace of the kernel and of the oracle: hits, instance ids and stats byte for byte, the stack within its bound and untouched
    by refusals.  -> (the oracle's per-ray stack depth, instance ids)"""
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
    return depth, gi


def check_modes(cr, ob, sc, rays, rng):
    """closest, closest masked, any, any masked (random ray masks, 0 and 0xff among them): their (stack depths, instance ids) in order"""
    a = device_arrays(ob, sc)
    rm = rng.integers(0, 256, rays.shape[0]).astype(np.uint32)
    rm[::17], rm[1::13] = 0, 0xff
    out = []
    for mode in (cr.CRT_TRACE_CLOSEST, cr.CRT_TRACE_ANY):
        for mask in (None, rm):
            out.append(check_against_oracle(cr, ob, sc, rays, mode, mask, a))
    return out


def random_masks(rng, n):
    m = (1 << rng.integers(0, 8, n)).astype(np.uint32) | (rng.integers(0, 256, n).astype(np.uint32) & rng.integers(0, 2, n).astype(np.uint32) * 0xff)
    m[::29], m[3::31] = 0, 0xff
    return m


@pytest.fixture(scope="module")
def meshes3(cr, cornell, tess8, tess40):
    return [cornell[0], tess8[0], tess40[0]]


def fixture_instances():
    """the 300-instance transformed fixture of tests/test_instances.py (seed 21), then 40 signed permutations, mirrors, shears and
    translated identities"""
    M, mesh_of = placed_instances(np.random.default_rng(21), 300, 3)
    rng = np.random.default_rng(22)
    S = special_matrices(rng, 40)
    return np.concatenate([M, S]), np.concatenate([mesh_of, rng.integers(0, 3, 40)]), random_masks(rng, 340)


def scene_rays(cr, sc, M, rng, n=8192, n_per=32):
    return np.concatenate([world_rays(cr.RAY_DT, rng, n, centres=M[:, :, 3]), edge_rays(cr.RAY_DT, rng, sc.world_boxes(), n_per=n_per)])


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "ploc", "lbvh"])
def test_kernel_equals_oracle_on_the_transformed_fixture(cr, ob, meshes3, builder):
    M, mesh_of, masks = fixture_instances()
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, masks), builder=builder)
    rng = np.random.default_rng(31)
    rays = scene_rays(cr, sc, M, rng)
    (_, ids), (_, mids), _, _ = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 2000 and (mids >= 0).sum() > 500
    assert (ids[-2000:] >= 0).sum() > 100                  # edge rays that hit
    sc.close()


@pytest.fixture(scope="module")
def sah_scene(cr, meshes3):
    M, mesh_of, masks = fixture_instances()
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, masks))
    yield sc, M
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 100003])
def test_ray_counts_around_the_64_ray_pool(cr, ob, sah_scene, n):
    sc, M = sah_scene
    rng = np.random.default_rng(n)
    rays = scene_rays(cr, sc, M, rng, n=max(n, 1), n_per=4)
    rays = rays[rng.permutation(rays.shape[0])[:n]]
    if n <= 1000:
        check_modes(cr, ob, sc, rays, rng)
    else:
        a = device_arrays(ob, sc)
        _, ids = check_against_oracle(cr, ob, sc, rays, cr.CRT_TRACE_CLOSEST, None, a)
        check_against_oracle(cr, ob, sc, rays, cr.CRT_TRACE_ANY, rng.integers(0, 256, n), a)
        assert (ids >= 0).sum() > 20000


@pytest.mark.gpu
def test_kernel_equals_oracle_with_4096_instances_of_one_mesh(cr, ob, tess8):
    rng = np.random.default_rng(33)
    M, _ = placed_instances(rng, 4096, 1, spread=60.0)
    sc = cr.InstancedScene([tess8[0]], cr.instances_array(M, np.zeros(4096), random_masks(rng, 4096)))
    rays = scene_rays(cr, sc, M, rng, n=4096, n_per=16)
    rays["o"][:4096] *= f32(4.0)
    (_, ids), _, _, _ = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 1000
    sc.close()


@pytest.mark.gpu
def test_kernel_equals_oracle_after_a_refit_to_jittered_matrices(cr, ob, meshes3):
    """refit keeps the TLAS built for the first placement: instances moved far from it, in a tree that no longer fits them"""
    M, mesh_of, masks = fixture_instances()
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, masks))
    rng = np.random.default_rng(41)
    J = M.copy()
    J[:, :, 3] = M[rng.permutation(len(M)), :, 3] + rng.normal(scale=2.0, size=(len(M), 3)).astype(f32)
    J[:, :, :3] = (M[:, :, :3] @ special_matrices(rng, len(M))[:, :, :3] * f32(0.9)).astype(f32)
    sc.refit(cr.instances_array(J, mesh_of, masks[::-1]))
    rays = scene_rays(cr, sc, J, rng)
    (_, ids), _, _, _ = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 2000
    sc.close()


@pytest.mark.gpu
def test_kernel_equals_oracle_after_update_meshes(cr, ob, cornell, meshes3):
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    M, mesh_of, masks = fixture_instances()
    sc = cr.InstancedScene(meshes3, cr.instances_array(M, mesh_of, masks), updatable=True)
    moved = tessellated_cornell(cornell[0], 8, amplitude=0.6)
    assert moved.vertices.shape == meshes3[1].vertices.shape
    sc.update_meshes({1: moved.vertices, 0: (meshes3[0].vertices * f32(1.1)).astype(f32)})
    rng = np.random.default_rng(43)
    rays = scene_rays(cr, sc, M, rng)
    (_, ids), _, _, _ = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 2000
    sc.close()


@pytest.mark.gpu
def test_kernel_equals_oracle_across_sets_and_a_refused_set(cr, ob, meshes3):
    from caitlynrenderer_amd import _lib
    M, mesh_of, masks = fixture_instances()
    sc = cr.InstancedScene(meshes3, cr.instances_array(M[:200], mesh_of[:200], masks[:200]), capacity=len(M))
    rng = np.random.default_rng(47)
    rays = scene_rays(cr, sc, M, rng, n=4096, n_per=8)
    check_modes(cr, ob, sc, rays, rng)
    for sel in (np.arange(len(M))[::-1], np.arange(1), np.arange(0), np.arange(7, 130)):
        sc.set(cr.instances_array(M[sel], mesh_of[sel], masks[sel]))
        assert sc.info()["n_instances"] == len(sel)
        (_, ids), _, _, _ = check_modes(cr, ob, sc, rays, rng)
        if len(sel) == 0:
            assert (ids == -1).all()
    bad = cr.instances_array(M, mesh_of, masks)
    bad["object_to_world"][17, 5] = np.nan
    with pytest.raises(cr.CrtError) as e:
        sc.set(bad)
    assert e.value.code == _lib.CRT_ERR_INVALID and sc.info()["n_instances"] == 123
    (_, ids), _, _, _ = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 500
    sc.close()


@pytest.mark.gpu
def test_coincident_instances_resolve_ties_to_the_lower_index(cr, ob, meshes3):
    """the same mesh under the same matrix at two indices: every hit on the pair is a t tie, which the lower index wins, whichever of
    the two the TLAS hands out first (the instance list is traced in both orders).  The rays stay within the grazing margin's bound
    (no far origins), where the TLAS culls neither of two equal boxes.
    The exception crt.h states: once the walk holds a hit at t, a BLAS box whose computed entry distance rounds above t is culled, and
    an equal-t hit inside it is never compared.  Each ray that reports the higher index must be such a tie: the lower instance alone
    hits it at the same t.  They are rare: on host-built trees 2 of ~205,000 rays that hit such pairs, and none on the rays of
    test_oracle_ties_across_instances_go_to_the_lower_index."""
    rng = np.random.default_rng(53)
    meshes = meshes3 + [reversed_ids(cr, meshes3[0])]
    M, mesh_of = placed_instances(rng, 24, 3)
    pairs = [(2, 19), (5, 6), (11, 23), (0, 14)]
    for a, b in pairs:
        M[b], mesh_of[b] = M[a], mesh_of[a]
    mesh_of[[5, 14]], mesh_of[[6, 0]] = 0, 3              # two of the pairs: a mesh and its reversed-id copy, in both orders
    for order in (np.arange(24), np.arange(24)[::-1]):
        sc = cr.InstancedScene(meshes, cr.instances_array(M[order], mesh_of[order], np.full(24, 0xff)))
        inv = np.argsort(order)                              # original index -> index in this scene
        rays = world_rays(cr.RAY_DT, rng, 4096, centres=M[[a for a, _ in pairs], :, 3])
        rays = np.concatenate([rays, edge_rays(cr.RAY_DT, rng, sc.world_boxes()[[inv[a] for a, _ in pairs]], n_per=16, far=False)])
        out = check_modes(cr, ob, sc, rays, rng)
        hits = sc.trace(rays)[0]
        for a, b in pairs:
            lo, hi = sorted((inv[a], inv[b]))
            alone = cr.InstancedScene(meshes, cr.instances_array(M[[order[lo]]], mesh_of[[order[lo]]]))
            for _, ids in out[:2]:                       # closest, closest masked
                lost = np.nonzero(ids == hi)[0]
                assert (ids == lo).sum() > 20 and lost.size <= 1 + (ids == lo).sum() // 100, (a, b, (ids == lo).sum(), lost.size)
                if lost.size:
                    h1, i1 = alone.trace(rays[lost])
                    assert (i1 == 0).all() and np.array_equal(h1["t"].view(np.uint32), hits["t"][lost].view(np.uint32))
            alone.close()
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_stack_bound_is_reached_on_a_worst_case_scene(cr, ob, builder):
    """Grid meshes in a grid of instances, all in one slab, and rays in the slab's mid plane: at every TLAS and BLAS level a line of
    siblings stays pending, and the TLAS leaves hold several instances the ray enters in turn.  The oracle reaches exactly
    stack_entries (TLAS depth + deepest BLAS depth), the kernel matches it byte for byte without a refused push.
    The clustered pattern of test_instances.py (test_stack_limit_refuses_and_keeps_the_previous_state) builds deep trees but cannot reach
    the bound: it is a chain, a level's smaller clusters under one inner child, so at most a few node groups stay pending across levels
    (3 on the host-built trees, 6 on the device's SAH trees when this test was written) against 20 and more stack entries.  It is traced
    below too, as the deep case."""
    V, T = grid_mesh(16)
    sc = cr.InstancedScene([(V, T)], cr.instances_array(grid_instances(8, 17.0), np.zeros(64), np.full(64, 0xff)), builder=builder)
    info = sc.info()
    assert info["tlas_depth8"] >= 2 and info["max_blas_depth8"] >= 3, info
    rng = np.random.default_rng(61)
    rays = grazing_plane_rays(cr.RAY_DT, rng, 8 * 17.0, 4000, 0.125)
    depths = check_modes(cr, ob, sc, rays, rng)
    assert depths[0][0].max() == info["stack_entries"], (depths[0][0].max(), info)
    sc.close()
    Vc, Tc = clustered_mesh(20)
    sc = cr.InstancedScene([(Vc, Tc)], cr.instances_array(clustered_instances(12), np.zeros(96), np.full(96, 0xff)), builder=builder)
    info = sc.info()
    assert info["stack_entries"] >= 20, info
    rays = np.zeros(4096, cr.RAY_DT)
    rays["o"][:, 0] = rng.uniform(0.0, 40.0, 4096).astype(f32)
    rays["o"][:, 1] = rng.uniform(-0.01, 0.3, 4096).astype(f32)
    rays["o"][:, 2] = f32(5.0)
    rays["d"] = np.array([0.0, 0.0, -1.0], f32)
    rays["d"][::2] = np.array([1.0, 0.0, 0.0], f32)
    rays["o"][::2, 0] = f32(-1.0)
    rays["o"][::2, 2] = rng.uniform(0.0, 0.2, 2048).astype(f32)
    rays["tmax"] = f32(1e9)
    (cd, ids), _, _, _ = check_modes(cr, ob, sc, rays, rng)
    assert (ids >= 0).sum() > 100 and cd.max() < info["stack_entries"] // 2, (cd.max(), info)
    sc.close()


def clustered_mesh(K):
    """tests/test_instances.py: K clusters of 8 triangles, each 4x smaller than the previous and beside it (about K node8 levels)"""
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
    """tests/test_instances.py: 8 instances per cluster, each cluster 4x smaller (uniform scale) and beside the previous"""
    M = []
    for k in range(first, first + K):
        s = 4.0 ** -k
        for j in range(8):
            M.append(np.concatenate([np.eye(3) * s, np.array([[s * (10.0 + 3.0 * j)], [0.0], [0.0]])], 1))
    return np.array(M, f32)
