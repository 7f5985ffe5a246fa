"""The flat-scene walks against numpy walkers (tests/walk_ref.py) on trees that fill the traversal stack: DESIGN.md "The walks as tested".

CPU part: the walkers equal the C oracle and the brute force; independent depths; a family of worst-case trees whose walks — by the
walkers alone — hold exactly the stack the library would give them; five planted mistakes each change something.
GPU part: every walk form on those trees equals the walkers, hits, per-ray counts and frame counters, and drops no push — as created,
after a refit, after a rebuild to a deeper tree and back, and on replicas."""
import types

import numpy as np
import pytest

import camera_rays_ref as cref
import cwbvh_ref as R
import integrator_ref as ir
import walk_ref as W
from conftest import numpy_brute_force, seeded_rays
from test_instances_oracle import grazing_plane_rays, grid_mesh

f32 = np.float32
H_SLAB = 0.25
CWBVH_DEPTHS = (3, 6, 16)            # the floor's neighbour, one of 5..7, the cap
BUSHES = ((6, 3, 4), (16, 3, 1))     # (depth, stubs per chain node, inner children per stub): the same depths with 64 nodes or more
N_RAYS = 512


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the worst-case family

def slab_triangles(rng, n, repeats=True):
    """n triangles (0, a, 0) (1, 0, b h) (c, 1, h): each touches all six faces of the unit square's slab, so every box over any of them is
    that slab whichever way a tree groups them, and stays it through a refit"""
    a, b, c = rng.random(n), rng.random(n), rng.random(n)
    V = np.zeros((3 * n, 3), f32)
    V[0::3, 1] = a
    V[1::3, 0], V[1::3, 2] = 1.0, b * H_SLAB
    V[2::3, 0], V[2::3, 1], V[2::3, 2] = c, 1.0, H_SLAB
    q = n // 4 if repeats else 0                                       # the last quarter repeats the first: equal t under different ids
    V[3 * (n - q):] = V[:3 * q]
    T = np.zeros((n, 12), np.int32)
    T[:, 0:3] = np.arange(3 * n).reshape(n, 3)
    T[:, 7] = 1                                                        # vertex normals: all normal 0
    T[:, 8:11] = -1
    return V, T


def comb8(D, stubs=1, kids=0, seed=3):
    """A CWBVH of depth D written node by node.  Level k < D holds one chain node whose inner children are the next chain node in slot 7
    (6 on even levels) and `stubs` (<= 3) stub nodes in slots below 4: for a ray with d.x < 0 the chain has the largest slot ^ octant, is
    entered first and leaves the stubs' bits on the stack as ONE entry, at every level — D - 1 entries at the deepest node.  A stub above
    the last level has `kids` inner children of its own, nodes of leaves; walking them holds no more than the chain does.  Every third
    chain node also holds a triangle of its own (tested at once, never pushed).  A node of leaves holds 1 + 2 + 3 triangles, the deepest
    chain node 3 + 1.  stubs = 1, kids = 0 is the plain comb of 2 D - 1 nodes (a "small tree" to the frame path: fewer than 64 nodes);
    more of either makes the same depth a tree of 64 nodes or more.  Returns (nodes, tri_slots, V, T, ids)."""
    assert 1 <= stubs <= 3 and kids <= 5

    def stub(level):
        if level == D or not kids:
            return {2: 1, 4: 2, 5: 3}
        node = {s: {5: 1, 6: 2, 7: 3} for s in range(kids)}
        node[7] = 2
        return node

    def chain(k):
        if k == D:
            return {0: 3, 7: 1}
        node = {s + (k % 2 == 0 and stubs < 3): stub(k + 1) for s in range(stubs)}
        node[7 if k % 2 else 6] = chain(k + 1)
        if k % 3 == 0:
            node[3 if stubs < 3 else 5] = 1
        return node

    order, todo = [], [chain(1)]                                        # breadth-first; a node's inner children follow one another
    while todo:
        node = todo.pop(0)
        order.append(node)
        todo += [node[s] for s in sorted(node) if isinstance(node[s], dict)]
    index = {id(node): i for i, node in enumerate(order)}
    n8 = len(order)
    meta, imask = np.zeros((n8, 8), np.int64), np.zeros(n8, np.int64)
    child_base, tri_base = np.zeros(n8, np.int64), np.zeros(n8, np.int64)
    n_tris = 0
    for i, node in enumerate(order):
        tri_base[i], off = n_tris, 0
        inner = [s for s in sorted(node) if isinstance(node[s], dict)]
        if inner:
            child_base[i] = index[id(node[inner[0]])]
        for s in sorted(node):
            if isinstance(node[s], dict):
                meta[i, s], imask[i] = (24 + s) | 0x20, imask[i] | (1 << s)
            else:
                meta[i, s] = (((1 << node[s]) - 1) << 5) | off
                off += node[s]
        n_tris += off
    rng = np.random.default_rng(seed)
    V, T = slab_triangles(rng, n_tris)
    lo, hi = np.zeros((n8, 3), f32), np.tile(np.array([1, 1, H_SLAB], f32), (n8, 1))
    occupied = meta != 0
    nodes = R.encode(lo, hi, np.broadcast_to(lo[:, None], (n8, 8, 3)), np.broadcast_to(hi[:, None], (n8, 8, 3)), occupied, meta, imask,
                     child_base, tri_base)
    return nodes, np.arange(n_tris, dtype=np.int32), V, T, rng.permutation(n_tris).astype(np.int32)


def comb2(depth, seed=4):
    """A FlatNode comb: every interior node's LEFT child is the rest of the chain and its right child a leaf of one or two triangles, all
    boxes the slab.  Equal entry distances send the walk left, the leaf is pushed: `depth` pushes above the sentinel at the deepest leaf.
    Returns (flat, V, T, ids)."""
    n = 2 * depth + 1
    counts = [1 + (k % 2) for k in range(depth + 1)]
    flat = np.zeros((n, 8), f32)
    flat[:, 4:7] = (1, 1, H_SLAB)
    start = 0
    for k in range(depth):                                             # interior node of level k: 0, then 2k - 1
        i = 0 if k == 0 else 2 * k - 1
        flat[i, 3] = 2 * k + 1
        flat[2 * k + 2, 3], flat[2 * k + 2, 7] = start, counts[k]
        start += counts[k]
    flat[2 * depth - 1, 3], flat[2 * depth - 1, 7] = start, counts[depth]
    rng = np.random.default_rng(seed)
    V, T = slab_triangles(rng, start + counts[depth], repeats=False)   # the BVH2 frame mode keeps the shader's first-visited rule
    return flat, V, T, rng.permutation(T.shape[0]).astype(np.int32)


def slab_rays(cr, n, seed=11):
    """in-plane rays across the unit slab at mid height, every direction of the plane, from outside and (every fourth) from inside it; a
    few carry a finite tmax"""
    rng = np.random.default_rng(seed)
    rays = grazing_plane_rays(cr.RAY_DT, rng, 1.0, n, H_SLAB / 2)
    inside = np.arange(n) % 4 == 3
    rays["o"][inside, :2] = rng.uniform(0.05, 0.95, (int(inside.sum()), 2)).astype(f32)
    rays["tmax"][np.arange(n) % 7 == 5] = f32(2.25)
    return rays


# ---------------------------------------------------------------------------------------------- scenes around the trees

LIGHT_ID = 1                          # the triangle (original id) the lights entry of every scene here describes
EMISSION = (9.0, 7.0, 5.0)


def shading_arrays(V, T_src, lamp_faces_x=True):
    """(triangles, normals, materials, lights): grey Lambert on the even ids; the odd ones glow, all through the one material whose light
    entry is triangle LIGHT_ID inside the slab — so half of the hits carry radiance by themselves (a frame here is to show light in a
    quarter of its pixels, and the slab is too crowded for shadow rays to get far), and every Lambert hit sends a shadow ray along the slab"""
    T = T_src.copy()
    T[:, 3] = np.arange(T.shape[0]) % 2
    T[:, 4:8] = (0, 0, 0, 1)
    T[:, 8:12] = (-1, -1, -1, 0)
    mats = np.full((2, 16), -1.0, f32)
    mats[:, 8:12] = 0.0
    mats[0, 0:4], mats[0, 4:8] = (0.7, 0.6, 0.5, 0.0), (0, 0, 0, -1)
    mats[1, 0:4], mats[1, 4:8] = (0.0, 0.0, 0.0, 0.0), EMISSION + (0.0,)
    p, a, b = (V[T[LIGHT_ID, k]].astype(np.float64) for k in range(3))
    u, v = a - p, b - p
    nrm = np.cross(u, v)
    if lamp_faces_x and nrm[0] < 0:                                    # points beside the unit slab at x > 1 see its lit side
        nrm = -nrm
    area = float(np.linalg.norm(nrm))
    light = np.concatenate([p, u, v, nrm / area, EMISSION, [area, 1.0, 0.0]]).astype(f32).reshape(1, 18)
    return T, np.array([[0, 0, 1]], f32), mats, light


class Tree:
    """One member of the family: the arrays a Scene is created from, the mesh in source order (a triangle's index is its original id) for
    the tree-less references, and the tree as the walkers take it"""

    def __init__(self, cr, name, V, leaf, ids, nodes=None, tri_slots=None, flat=None, extent=1.0):
        self.name, self.V, self.flat = name, V, flat
        src = np.zeros((int(ids.max()) + 1, 12), np.int32)
        src[ids] = leaf
        src, normals, mats, lights = shading_arrays(V, src, lamp_faces_x=extent == 1.0)   # the grid's lamp keeps its winding: it is seen from above
        self.leaf, self.ids = src[ids], np.ascontiguousarray(ids, np.int32)
        self.mesh = cr.Mesh(V, normals, np.zeros((0, 2), f32), src, mats, lights)
        self.cam = cr.Camera((0.5 * extent, 0.5 * extent, 3.0 * extent), (0.5 * extent, 0.5 * extent, 0.0), 15.0)
        if nodes is None and flat is not None:                        # the library converts a BVH2 it is given; this is the host converter
            cw = cr.CWBVH().convert_arrays(flat, leaf.shape[0])
            nodes, tri_slots, given = cw.nodes, cw.tri_slots, None
        else:
            given = types.SimpleNamespace(nodes=nodes, tri_slots=tri_slots)
        self.nodes, self.tri_slots = nodes, tri_slots
        self.data = cr.SceneData(self.mesh, types.SimpleNamespace(triangles=self.leaf, triangle_indices=self.ids, flat_nodes=flat), given, self.cam)
        self.rays = slab_rays(cr, N_RAYS) if extent == 1.0 else None

    @property
    def tris8(self):
        return (self.tri_slots, self.leaf, self.V, self.ids)

    @property
    def tris2(self):
        return (None, self.leaf, self.V, self.ids)


NATURAL_G = 32                        # the smallest grid of those probed (12, 20, 24, 32) whose trees — the host SBVH's and the three GPU
                                      # builders' by their numpy references — are deep enough (4) to leave the floor AND are walked to the bound


def natural_mesh(cr):
    V, T = grid_mesh(NATURAL_G, H_SLAB)
    return Tree(cr, "grid", V, T, np.arange(T.shape[0], dtype=np.int32), nodes=np.zeros((0, 80), np.uint8), tri_slots=np.zeros(0, np.int32),
                extent=float(NATURAL_G)).mesh


def natural_rays(cr, n=300):
    rays = grazing_plane_rays(cr.RAY_DT, np.random.default_rng(17), float(NATURAL_G), n, H_SLAB / 2)
    rays["o"][n - 40:n - 20, 2] = 2 * H_SLAB                            # over the slab: nothing to hit
    rays["tmax"][n - 20:] = f32(2.0 * NATURAL_G + 3.0)                  # cut short a few cells into the grid
    return rays


def natural_tree(cr):
    """the grid through the host builders: SBVH with spatial splits, host converter"""
    mesh = natural_mesh(cr)
    sb = cr.SBVH(mesh.triangles, mesh.vertices, 0)
    cw = cr.CWBVH().convert(sb)
    t = Tree(cr, "grid32", mesh.vertices, sb.triangles, sb.triangle_indices, nodes=cw.nodes, tri_slots=cw.tri_slots, flat=sb.flat_nodes,
             extent=float(NATURAL_G))
    t.rays = natural_rays(cr)
    return t


_family = {}


def family(cr):
    if not _family:
        for D in CWBVH_DEPTHS + (17,):
            nodes, slots, V, T, ids = comb8(D)
            _family[f"comb8-{D}"] = Tree(cr, f"comb8-{D}", V, T, ids, nodes=nodes, tri_slots=slots)
        for D, stubs, kids in BUSHES:
            nodes, slots, V, T, ids = comb8(D, stubs, kids)
            assert nodes.shape[0] >= 64                               # the frame path's walks of many rays side by side start there
            _family[f"bush8-{D}"] = Tree(cr, f"bush8-{D}", V, T, ids, nodes=nodes, tri_slots=slots)
        for d in (94, 95):
            flat, V, T, ids = comb2(d)
            _family[f"comb2-{d}"] = Tree(cr, f"comb2-{d}", V, T, ids, flat=flat)
        _family["grid32"] = natural_tree(cr)
    return _family


WALKED8 = [f"comb8-{D}" for D in CWBVH_DEPTHS] + [f"bush8-{D}" for D, _, _ in BUSHES] + ["grid32"]          # the CWBVHs the premise is about
_walks = {}


def ref_walk(cr, name, accel, any_hit):
    """the walkers' answer for a family member's own rays, computed once"""
    key = (name, accel, any_hit)
    if key not in _walks:
        t = family(cr)[name]
        _walks[key] = W.cwbvh_walk(t.nodes, t.tris8, t.rays, any_hit) if accel == 8 else W.bvh2_walk(t.flat, t.tris2, t.rays, any_hit)
    return _walks[key]


def assert_hits(got, w, any_hit, what=""):
    """crt_hit / orc_hit records against a Walk: occlusion for any-hit walks, (id, t, u, v) bit for bit for closest-hit ones"""
    if any_hit:
        assert np.array_equal(got["tri"] >= 0, w.slot >= 0), what
        return
    assert np.array_equal(got["tri"], w.id), what
    for k in ("t", "u", "v"):
        assert np.array_equal(bits(got[k]), bits(getattr(w, k))), (what, k)


def assert_counts(st, w, what=""):
    assert np.array_equal(st["nodes"], w.n_nodes) and np.array_equal(st["tris"], w.n_tris), what


# ---------------------------------------------------------------------------------------------- CPU: the walkers

def hostile_rays(cr, which):
    """the ray sets of test_gpu_parity's test_edge_cases and test_zero_components_and_non_finite_rays (the second cut to 400 rays)"""
    if which == "edges":
        rays = np.zeros(70, cr.RAY_DT)
        dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
        for i in range(70):
            rays[i]["o"] = (2.78, 2.75, 2.8) if i % 2 == 0 else (0.0, 2.75, 2.8)
            rays[i]["d"] = dirs[i % 6]
            rays[i]["tmax"] = [1e9, 0.0, -1.0, 1e-30, 3.0][i % 5]
        return rays
    n = 400
    rng = np.random.default_rng(2)
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"] = (0.3 + 4.9 * rng.random((n, 3))).astype(f32)
    dirs = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0.6, 0.8), (0.6, 0, -0.8), (-0.0, 1, 0), (0, 0, 0)], f32)
    rays["d"] = dirs[np.arange(n) % len(dirs)]
    rays["tmax"] = f32(1e9)
    rays["o"][5] = (np.nan, 1, 1); rays["o"][6] = (1, -np.inf, 1); rays["d"][7] = (np.nan, 1, 0)
    rays["d"][8] = (1e-30, -1e-30, 1)                                 # below 2^-80 without being zero
    return rays


def fixture_rays(cr, mesh, which):
    if which == "seeded":
        rays = seeded_rays(mesh, 300, 4, cr.RAY_DT)
        rays["tmax"][::3] = (np.random.default_rng(9).random(100) * 6).astype(f32)
        return rays
    return hostile_rays(cr, which)


@pytest.mark.parametrize("which", ["seeded", "edges", "zeros"])
@pytest.mark.parametrize("scene", ["cornell", "tess8"])
def test_walkers_equal_the_oracle_and_the_brute_force(cr, ob, cornell, cornell_data, tess8, scene, which):
    mesh, data = (cornell[0], cornell_data) if scene == "cornell" else tess8
    rays = fixture_rays(cr, mesh, which)
    orc = ob.Oracle(data, 8, 8, 3, cornell[1])
    tri, t, u, v = numpy_brute_force(mesh, rays)
    trees = ((8, ob.BVH8, lambda a: W.cwbvh_walk(data.bvh8, (data.bvh8_tri_slots, data.triangles, data.vertices, data.tri_orig_ids), rays, a)),
             (2, ob.BVH2, lambda a: W.bvh2_walk(data.bvh, (None, data.triangles, data.vertices, data.tri_orig_ids), rays, a)))
    for accel, oa, walk in trees:
        for any_hit in (False, True):
            w = walk(any_hit)
            want, st = orc.trace(rays, oa, ob.ANY if any_hit else ob.CLOSEST, ob.TIE_LOWEST_ID, stats=True)
            assert_hits(want, w, any_hit, (accel, any_hit))
            assert_counts(st, w, (accel, any_hit))
            assert w.refused.sum() == 0
            if any_hit:
                assert np.array_equal(w.slot >= 0, tri >= 0)
            else:
                hit = tri >= 0
                assert np.array_equal(w.id, tri)
                for a, b in ((w.t, t), (w.u, u), (w.v, v)):
                    assert np.array_equal(bits(a[hit]), bits(b[hit]))
    if which == "seeded":
        assert (tri >= 0).sum() > 100 and (tri < 0).sum() > 0


def test_bvh2_walker_keeps_the_shaders_first_visited_rule(cr, ob, tess8):
    """without the lowest-id rule the BVH2 walk is the shipped shader's: strict `<` at the boxes and at the triangles"""
    mesh, data = tess8
    rays = seeded_rays(mesh, 300, 6, cr.RAY_DT)
    w = W.bvh2_walk(data.bvh, (None, data.triangles, data.vertices, data.tri_orig_ids), rays, False, tie_lowest_id=False)
    want, st = ob.Oracle(data, 8, 8, 3, None).trace(rays, ob.BVH2, ob.CLOSEST, ob.TIE_FIRST_VISITED, stats=True)
    assert_hits(want, w, False)
    assert_counts(st, w)


def test_depths_equal_what_the_host_reports(cr, cornell_data, tess8):
    for data in (cornell_data, tess8[1]):
        sb = cr.SBVH(data.triangles[:, :], data.vertices, 1)          # any host-built pair will do: build one more with other flags
        cw = cr.CWBVH().convert(sb)
        assert W.depth8(cw.nodes) == cw.depth and W.depth2(sb.flat_nodes) == sb.depth()
        assert W.depth8(data.bvh8) == cr.CWBVH().convert_arrays(data.bvh, data.triangles.shape[0]).depth
    for name, t in family(cr).items():
        if t.flat is not None:
            assert W.depth2(t.flat) == cr.SBVH.depth(types.SimpleNamespace(flat_nodes=t.flat)), name
            assert W.depth8(t.nodes) == cr.CWBVH().convert_arrays(t.flat, t.leaf.shape[0]).depth, name


def test_the_family_has_the_depths_it_was_made_for(cr):
    fam = family(cr)
    for D in CWBVH_DEPTHS + (17,):
        assert W.depth8(fam[f"comb8-{D}"].nodes) == D
    for d in (94, 95):
        assert W.depth2(fam[f"comb2-{d}"].flat) == d
        assert W.depth8(fam[f"comb2-{d}"].nodes) <= 16                # the library's own conversion of the comb stays walkable
    assert W.depth8(fam["grid32"].nodes) >= 4                         # off the max(2, .) floor


def stack_bound8(D):
    """what csrc/device_build.hpp cwbvh_stack_entries gives a tree of depth D <= 16, restated"""
    return max(2, D - 1)


def test_premise_every_tree_is_walked_to_its_bound_and_not_beyond(cr, capsys):
    """By the walkers alone: the largest stack over the chosen rays IS the bound the library derives from the depth, at least 32 rays hold
    it, and one entry fewer refuses a push on every one of them.  (The undersized walk exists on the CPU only.)
    tree, depth, bound, rays at the bound (closest / any) of 512 (300 on the grid) — DESIGN.md has the table."""
    rows = []
    for name in WALKED8:
        t = family(cr)[name]
        D = W.depth8(t.nodes)
        bound, at = stack_bound8(D), []
        for any_hit in (False, True):
            w = ref_walk(cr, name, 8, any_hit)
            assert w.stack.max() == bound and w.refused.sum() == 0, (name, any_hit, w.stack.max(), bound)
            full = w.stack == bound
            assert full.sum() >= 32, (name, any_hit, int(full.sum()))
            short = W.cwbvh_walk(t.nodes, t.tris8, t.rays[full], any_hit, stack_entries=bound - 1)
            assert (short.refused > 0).all() and short.stack.max() == bound - 1
            at.append(int(full.sum()))
        rows.append((name, D, bound, at[0], at[1]))
    for name in ("comb2-94", "comb2-95"):
        t = family(cr)[name]
        d2, at = W.depth2(t.flat), []
        for any_hit in (False, True):
            w = ref_walk(cr, name, 2, any_hit)
            most = int(w.stack.max())
            assert most == d2 + 1 <= d2 + 2 and w.refused.sum() == 0   # the sentinel and one entry per interior level: one spare row
            full = w.stack == most
            assert full.sum() >= 32
            short = W.bvh2_walk(t.flat, t.tris2, t.rays[full], any_hit, stack_entries=most - 1)
            assert (short.refused > 0).all()
            at.append(int(full.sum()))
        rows.append((name, d2, d2 + 2, at[0], at[1]))
    with capsys.disabled():
        print("\n  tree        depth  bound  rays at the most entries held (closest, any)")
        for r in rows:
            print("  %-10s  %5d  %5d  %d, %d" % r)


def test_the_family_hits_misses_and_ties(cr):
    """the rays of every tree hit and miss, and the walkers agree with the brute force there too; the repeated triangles give equal t"""
    for name in WALKED8 + ["comb2-94"]:
        t = family(cr)[name]
        tri, tt, u, v = numpy_brute_force(t.mesh, t.rays)
        hit = tri >= 0
        assert hit.sum() >= 32 and (~hit).sum() >= 8, (name, int(hit.sum()))
        for accel in (8, 2) if t.flat is not None else (8,):
            w = ref_walk(cr, name, accel, False)
            assert np.array_equal(w.id, tri), (name, accel)
            for a, b in ((w.t, tt), (w.u, u), (w.v, v)):
                assert np.array_equal(bits(a[hit]), bits(b[hit]))
            assert np.array_equal(ref_walk(cr, name, accel, True).slot >= 0, hit)


def test_five_mistakes_each_change_a_hit_a_count_or_a_stack_depth(cr, cornell, cornell_data, tess8):
    """the walker is not vacuous: each wrong reading shows on the fixtures"""
    cases = []
    for mesh, data in ((cornell[0], cornell_data), tess8):
        cases.append((data.bvh8, (data.bvh8_tri_slots, data.triangles, data.vertices, data.tri_orig_ids), seeded_rays(mesh, 300, 4, cr.RAY_DT)))
    for name in ("comb8-6", "grid32"):
        t = family(cr)[name]
        cases.append((t.nodes, t.tris8, t.rays))
    for mistake in W.MISTAKES:
        changed = []
        for nodes, tris, rays in cases:
            for any_hit in (False, True):
                right, wrong = W.cwbvh_walk(nodes, tris, rays, any_hit), W.cwbvh_walk(nodes, tris, rays, any_hit, mistake=mistake)
                for f in ("id", "t", "u", "v", "n_nodes", "n_tris", "stack"):
                    a, b = getattr(right, f), getattr(wrong, f)
                    if not np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b):
                        changed.append(f)
        assert changed, mistake


# ---------------------------------------------------------------------------------------------- GPU: the kernels against the walkers

BVH2_MODE = 2 | 4                     # CRT_TRACE_BVH2 | CRT_TRACE_TIE_LOWEST_ID


def device_tree(sc, with_bvh2):
    """the tree as the device holds it: (node8s, CWBVH-order records, FlatNodes, slot-order records)"""
    return (sc.debug_read_accel(0), sc.debug_read_accel(1)) + ((sc.debug_read_accel(2), sc.debug_read_accel(3)) if with_bvh2 else (None, None))


def check_traces(cr, sc, nodes, recs, flat, recs2, rays, what):
    """crt_trace in its four modes against the walkers on the same arrays: hits, per-ray counts, no dropped push"""
    for any_hit in (False, True):
        mode = cr.CRT_TRACE_ANY if any_hit else cr.CRT_TRACE_CLOSEST
        w = W.cwbvh_walk(nodes, recs, rays, any_hit)
        got, st = sc.trace(rays, mode, stats=True)
        assert_hits(got, w, any_hit, (what, "bvh8", any_hit))
        assert_counts(st, w, (what, "bvh8", any_hit))
        assert_hits(sc.trace(rays, mode), w, any_hit, (what, "bvh8 without stats", any_hit))
        if flat is not None:
            w2 = W.bvh2_walk(flat, recs2, rays, any_hit)
            got, st = sc.trace(rays, mode | BVH2_MODE, stats=True)
            assert_hits(got, w2, any_hit, (what, "bvh2", any_hit))
            assert_counts(st, w2, (what, "bvh2", any_hit))
    assert sc.frame_stats()["stack_overflows"] == 0, what


def premise_holds(nodes, recs, rays, min_rays=32):
    D = W.depth8(nodes)
    for any_hit in (False, True):
        w = W.cwbvh_walk(nodes, recs, rays, any_hit)
        assert w.stack.max() == stack_bound8(D) and (w.stack == stack_bound8(D)).sum() >= min_rays, (D, any_hit, int(w.stack.max()))
    return D


def walk_prefix(w, n):
    return W.Walk(*[f[:n] for f in w])


def rv_product(rv):
    return ir.F(f32(rv[0]) * f32(rv[1]))


def side_camera(cr):
    """a pinhole beside the slab looking along -x through it: every primary ray that meets the slab has d.x < 0"""
    return cr.Camera((2.0, 0.5, H_SLAB / 2), (0.0, 0.5, H_SLAB / 2), 4.0)


def side_scene_data(cr, t):
    return cr.SceneData(t.mesh, types.SimpleNamespace(triangles=t.leaf, triangle_indices=t.ids, flat_nodes=None),
                        types.SimpleNamespace(nodes=t.nodes, tri_slots=t.tri_slots), side_camera(cr))


def assert_refused(e, code, text):
    """a CrtError's code (a name of include/crt.h's crt_status) and a piece of its text"""
    from caitlynrenderer_amd import _lib
    assert e.value.code == getattr(_lib, code) and text in str(e.value), str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WALKED8 + ["comb2-94"])
def test_gpu_host_supplied_trees_depths_and_every_trace_mode(cr, name):
    t = family(cr)[name]
    sc = cr.Scene(t.data, 8, 8, 1)
    try:
        info = sc.bvh_info()
        nodes, recs, flat, recs2 = device_tree(sc, t.flat is not None)
        assert np.array_equal(nodes, t.nodes) and np.array_equal(bits(recs), bits(W.records(t.tris8)))
        assert info["max_depth8"] == W.depth8(nodes)
        if t.flat is not None:
            assert np.array_equal(bits(flat), bits(t.flat)) and info["bvh2_depth"] == W.depth2(flat)
        if name != "comb2-94":
            premise_holds(nodes, recs, t.rays)
        check_traces(cr, sc, nodes, recs, flat, recs2, t.rays, name)
        if t.flat is None:
            with pytest.raises(cr.CrtError):
                sc.trace(t.rays, BVH2_MODE)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["lbvh", "ploc", "sah"])
def test_gpu_device_built_grid_is_walked_to_its_bound(cr, builder):
    mesh, rays = natural_mesh(cr), natural_rays(cr)
    sc = cr.Scene(cr.SceneData.for_device_build(mesh, None, builder), 8, 8, 1)
    try:
        info = sc.bvh_info()
        nodes, recs, flat, recs2 = device_tree(sc, True)
        D = premise_holds(nodes, recs, rays)
        assert info["max_depth8"] == D >= 4 and info["bvh2_depth"] == W.depth2(flat)
        check_traces(cr, sc, nodes, recs, flat, recs2, rays, builder)
        tri = numpy_brute_force(mesh, rays)[0]
        assert np.array_equal(sc.trace(rays)["tri"], tri)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bush8-16", "grid32"])
def test_gpu_pools_refills_and_ragged_counts(cr, name):
    t = family(cr)[name]
    rays = np.tile(t.rays, 9 + 4096 // t.rays.shape[0])[:4096 + 257]
    sc = cr.Scene(t.data, 8, 8, 1)
    try:
        want = {a: W.cwbvh_walk(t.nodes, t.tris8, rays, a) for a in (False, True)}
        for pool, refill in ((64, 8), (128, 1), (128, 32), (256, 8), (256, 64)):
            sc.set_option("trace_pool", pool)
            sc.set_option("refill_min", refill)
            for n in (1, 63, 65, 4096 + 257):
                for any_hit in (False, True):
                    w = walk_prefix(want[any_hit], n)
                    got, st = sc.trace(rays[:n], cr.CRT_TRACE_ANY if any_hit else cr.CRT_TRACE_CLOSEST, stats=True)
                    assert_hits(got, w, any_hit, (pool, refill, n, any_hit))
                    assert_counts(st, w, (pool, refill, n, any_hit))
        assert sc.frame_stats()["stack_overflows"] == 0
    finally:
        sc.close()


# -- frames

_frame_refs = {}
RVS = [(0.6591631, 0.910802), (0.3141592, 0.2718281)]


def frame_shape(t):
    n = t.rays.shape[0]
    return (32, n // 32) if n % 32 == 0 else (20, n // 20)


def camera_frames_ref(cr, name, depth):
    """(sums after the frames RVS, the closest walk of the camera rays) by the numpy references, once per (tree, depth)"""
    key = (name, depth)
    if key not in _frame_refs:
        t = family(cr)[name]
        w, h = frame_shape(t)
        sums = cref.render(ir.RefScene(t.mesh, t.cam, w, h), t.rays["o"], t.rays["d"], RVS, depth)[0][depth - 1]
        lit = (sums.reshape(-1, 3) != 0).any(1).mean()
        assert lit >= 0.25, (name, depth, lit)                        # a frame counts only if the reference shows light in a quarter of it
        _frame_refs[key] = sums
    return _frame_refs[key]


FRAME_OPTIONS = [(), (("inplace_shadow", 0),), (("inplace_shadow", 1),), (("inplace_shadow", 2),), (("inplace_shadow", 3),), (("wave_samples", 0),),
                 (("wave_samples", 1),), (("wave_samples", 3),), (("wide_first", 0),), (("wide_first", 1),), (("streams", 2),), (("lean_build", 0),),
                 (("lean_build", 1),)]


OPTION_DEFAULTS = {"inplace_shadow": 3, "wave_samples": 2, "wide_first": 2, "streams": 1, "lean_build": 1, "accel": 0}   # of a new scene


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["comb8-16", "bush8-16", "bush8-6", "grid32", "comb2-94"])
def test_gpu_frames_along_the_worst_case_rays(cr, name):
    """paths of two segments along the tree's own rays (set_camera_rays): k_segment's walks, the in-place and the deferred shadow walks and
    the bounce walks hold the full stack; every option set gives the reference's words and drops no push"""
    t = family(cr)[name]
    w, h = frame_shape(t)
    want = camera_frames_ref(cr, name, 2)
    o, d = t.rays["o"].reshape(h, w, 3), t.rays["d"].reshape(h, w, 3)
    option_sets = FRAME_OPTIONS + ([(("accel", 1),)] if name == "comb2-94" else [])
    sc = cr.Scene(t.data, w, h, 2)
    try:
        sc.set_camera_rays(o, d)
        for options in option_sets:
            for k, v in options:
                sc.set_option(k, v)
            sc.reset()
            for rx, ry in RVS:
                sc.render_frame(rx, ry)
            got = sc.read_sum()
            assert int((bits(got) != bits(want)).sum()) == 0, (name, options)
            assert sc.frame_stats()["stack_overflows"] == 0, (name, options)
            sc.reset()
            sc.render_frames(RVS)
            assert int((bits(sc.read_sum()) != bits(want)).sum()) == 0, (name, options, "render_frames")
            assert sc.frame_stats()["stack_overflows"] == 0, (name, options)
            for k, v in options:                                        # back to the defaults a new scene has
                sc.set_option(k, OPTION_DEFAULTS[k])
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["comb8-16", "bush8-16", "grid32", "comb2-94"])
def test_gpu_frame_counters_equal_the_walkers_sums(cr, name):
    """count_visits on a one-segment path, under every option set of FRAME_OPTIONS: nodes_closest, tris_closest and closest_hits are the
    walker's sums over the camera rays (whose bound is 1e9f whatever the entry says)"""
    t = family(cr)[name]
    w, h = frame_shape(t)
    rays = t.rays.copy()
    rays["tmax"] = f32(1e9)
    want = camera_frames_ref(cr, name, 1)
    for accel in (0, 1) if name == "comb2-94" else (0,):
        walk = W.bvh2_walk(t.flat, t.tris2, rays, False, tie_lowest_id=False) if accel else W.cwbvh_walk(t.nodes, t.tris8, rays, False)
        sc = cr.Scene(t.data, w, h, 1)
        try:
            sc.set_option("accel", accel)
            sc.set_option("count_visits", 1)
            sc.set_camera_rays(t.rays["o"].reshape(h, w, 3), t.rays["d"].reshape(h, w, 3))
            sums = (int(walk.n_nodes.sum()), int(walk.n_tris.sum()), int((walk.slot >= 0).sum()))
            for options in FRAME_OPTIONS:                               # the counting builds of every frame form
                for k, v in options:
                    sc.set_option(k, v)
                sc.reset()
                sc.render_frame(*RVS[0])
                st = sc.frame_stats()
                assert (st["nodes_closest"], st["tris_closest"], st["closest_hits"]) == sums, (name, accel, options)
                assert st["stack_overflows"] == 0
                sc.render_frame(*RVS[1])
                assert int((bits(sc.read_sum()) != bits(want)).sum()) == 0, (name, accel, options)
                for k, v in options:
                    sc.set_option(k, OPTION_DEFAULTS[k])
        finally:
            sc.close()


@pytest.mark.gpu
def test_gpu_lean_last_segment_build_holds_the_full_stack(cr):
    """The LEAN form pushes without a bound check.  On the host-validated depth-16 tree of 64+ nodes, four samples through one
    render_frames call on a one-segment path (the form that has a LEAN build): the primary rays of a pinhole beside the slab hold all 15
    entries by the walker, the launch says it ran LEAN, and the sum is the numpy integrator's with the option on and off."""
    t = family(cr)["bush8-16"]
    cam, (w, h) = side_camera(cr), (64, 16)
    rnd = cr.Rnd()
    rvs = [(rnd.randf2(), rnd.randf2()) for _ in range(4)]
    ref = ir.RefScene(t.mesh, cam, w, h)
    o, d = ir.primary_rays(ref, *rvs[0])[:2]
    rays = np.zeros(w * h, cr.RAY_DT)
    rays["o"], rays["d"], rays["tmax"] = o, d, f32(1e9)
    stack = W.cwbvh_walk(t.nodes, t.tris8, rays, False).stack
    assert stack.max() == 15 and (stack == 15).sum() >= 32
    want = ir.render(ref, rvs, 1)[0][0]
    assert (want.reshape(-1, 3) != 0).any(1).mean() >= 0.25
    sc = cr.Scene(side_scene_data(cr, t), w, h, 1)
    try:
        sc.set_option("wide_first", 1)
        sc.render_frames(rvs)                                          # the first launch of a view clocks its tiles and is never LEAN
        for lean in (1, 0, 1):
            sc.set_option("lean_build", lean)
            sc.reset()
            sc.render_frames(rvs)
            assert sc.debug_lean_build() == bool(lean), (lean, sc.debug_launch_info())
            assert int((bits(sc.read_sum()) != bits(want)).sum()) == 0, lean
            assert sc.frame_stats()["stack_overflows"] == 0
    finally:
        sc.close()


# -- ambient occlusion and fog from points and segments beside the slab

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bush8-16", "comb8-16"])
def test_gpu_ao_points_and_fog_segments_hold_the_full_stack(cr, name):
    """AO points beside the slab whose normal looks along -x into it, fog segments beside it whose shadow rays run to the lamp inside it:
    the rays the references build for either, put through the walker, hold the full stack (32 of them at least), and the results are
    the references' words"""
    import ao_ref
    import fog_ref
    t = family(cr)[name]
    rng = np.random.default_rng(23)
    n = 96
    ref = ir.RefScene(t.mesh, t.cam, 8, 8)
    pts = np.zeros(n, ao_ref.AO_POINT_DT)
    pts["p"] = np.stack([rng.uniform(1.2, 2.0, n), rng.uniform(0.2, 0.8, n), np.full(n, H_SLAB / 2)], 1)
    pts["n"] = (-1.0, 0.0, 0.0)
    pts["seed_x"], pts["seed_y"] = rng.uniform(0, 64, n), rng.uniform(0, 64, n)
    K = 8
    want, r = ao_ref.ao_points(ref, pts, K, *RVS[0])
    ok, o, sd = ao_ref.rays_of(pts, K, rv_product(RVS[0]))
    rays = np.zeros(n * K, cr.RAY_DT)
    rays["o"], rays["d"], rays["tmax"] = np.repeat(o, K, 0), sd.reshape(-1, 3), f32(1e9)
    stack = W.cwbvh_walk(t.nodes, t.tris8, rays, True).stack
    assert (stack == 15).sum() >= 32
    seg = np.zeros(n, fog_ref.FOG_SEGMENT_DT)
    seg["o"] = np.stack([rng.uniform(1.5, 2.5, n), rng.uniform(0.2, 0.8, n), np.full(n, H_SLAB / 2)], 1)
    seg["e"] = seg["o"] + np.stack([rng.uniform(0.2, 0.6, n), rng.uniform(-0.2, 0.2, n), np.zeros(n)], 1).astype(f32)
    seg["seed_x"], seg["seed_y"] = rng.uniform(0, 64, n), rng.uniform(0, 64, n)
    p = fog_ref.Params(K=K, density=0.3)
    fwant, fr = fog_ref.fog_segments(ref, seg, *RVS[0], p)
    lit = fr["lit"]                                                    # a sample that sees the lamp's lit side sends a shadow ray
    rays = np.zeros(int(lit.sum()), cr.RAY_DT)
    rays["o"], rays["d"], rays["tmax"] = fr["x"][lit], fr["ld"][lit], fr["tmax"][lit]
    stack = W.cwbvh_walk(t.nodes, t.tris8, rays, True).stack
    assert (stack == 15).sum() >= 32, (int(lit.sum()), int((stack == 15).sum()))
    sc = cr.Scene(t.data, 8, 8, 1)
    try:
        got = sc.ao_points(pts, *RVS[0], samples=K)
        assert int((bits(got) != bits(want)).sum()) == 0
        assert sc.frame_stats()["stack_overflows"] == 0
        got = sc.fog_segments(seg, *RVS[0], samples=K, density=0.3)
        assert int((bits(got) != bits(fwant)).sum()) == 0
        assert sc.frame_stats()["stack_overflows"] == 0
    finally:
        sc.close()


# -- mutations

@pytest.mark.gpu
def test_gpu_update_vertices_keeps_the_depth_and_the_walks(cr):
    """a refit changes boxes and records, never the topology: the depth stays, and the moved tree is walked to the same bound"""
    t = family(cr)["bush8-16"]
    sc = cr.Scene(t.data, 8, 8, 1)
    try:
        for scale in (2.0, 1.0):
            sc.update_vertices((t.V * f32(scale)).astype(f32))
            rays = t.rays.copy()
            rays["o"] = (rays["o"] * f32(scale)).astype(f32)
            rays["tmax"] = (rays["tmax"] * f32(scale)).astype(f32)
            nodes, recs, _, _ = device_tree(sc, False)
            assert sc.bvh_info()["max_depth8"] == W.depth8(nodes) == 16
            premise_holds(nodes, recs, rays)
            check_traces(cr, sc, nodes, recs, None, None, rays, scale)
    finally:
        sc.close()


def nested_slabs(clusters, ratio, n=240, seed=7):
    """n slab triangles in `clusters` equal groups, group j shrunk by ratio^-j towards the origin: nested slabs, each a bundle of
    triangles that share its box.  The builders split group from group and a group among its members, and a ray in the mid plane of
    the smallest slab that passes its corner region is offered every box."""
    V, T = slab_triangles(np.random.default_rng(seed), n, repeats=False)
    s = np.repeat(float(ratio) ** -np.arange(clusters), 3 * (n // clusters))
    return (V * s[:, None]).astype(f32), T


def nested_slab_rays(cr, clusters, ratio, n=400, seed=5):
    rng = np.random.default_rng(seed)
    smin = float(ratio) ** -(clusters - 1)
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"][:, :2] = rng.uniform(0.2 * smin, 0.8 * smin, (n, 2)) - 3.0 * d[:, :2]
    rays["o"][:, 2] = H_SLAB * smin / 2
    rays["d"], rays["tmax"] = d.astype(f32), f32(1e9)
    return rays


# (clusters, ratio) of the shallow and the deeper state per builder, all of the same 240 triangles.  Chosen on the CPU with the builders'
# numpy references (tests/bvh_build_ref.py, tests/cwbvh_ref.py) among clusters 2, 3, 5, 10 x ratios 1, 2, 8, 64: the pairs whose trees differ
# in depth (3 -> 6, 3 -> 4, 4 -> 6) and are both walked to their bound by 66 rays or more of nested_slab_rays
REBUILD_STATES = {"lbvh": ((2, 8.0), (10, 8.0)), "ploc": ((5, 1.0), (5, 8.0)), "sah": ((10, 8.0), (10, 64.0))}
REBUILD_FRAME = (24, 16)
_rebuild_states = {}


def rebuild_camera(cr):
    return cr.Camera((0.5, 0.5, 3.0), (0.5, 0.5, 0.0), 15.0)


def rebuild_state(cr, clusters, ratio):
    """(mesh, rays, the numpy integrator's sum of one two-segment frame from above), once per state"""
    key = (clusters, ratio)
    if key not in _rebuild_states:
        V, T = nested_slabs(clusters, ratio)
        src, normals, mats, lights = shading_arrays(V, T)              # triangle LIGHT_ID lies in group 0: the lights entry is every state's
        mesh = cr.Mesh(V, normals, np.zeros((0, 2), f32), src, mats, lights)
        want = ir.render(ir.RefScene(mesh, rebuild_camera(cr), *REBUILD_FRAME), RVS[:1], 2)[0][1]
        assert (want.reshape(-1, 3) != 0).any(1).mean() >= 0.25, key
        _rebuild_states[key] = types.SimpleNamespace(mesh=mesh, rays=nested_slab_rays(cr, clusters, ratio), want=want)
    return _rebuild_states[key]


@pytest.mark.gpu
@pytest.mark.parametrize("fan", ["single", "devices", "streams"])
@pytest.mark.parametrize("builder", ["lbvh", "ploc", "sah"])
def test_gpu_rebuild_to_a_deeper_tree_and_back(cr, builder, fan):
    """crt_rebuild_vertices from the shallow state to the deeper one and back, on one scene, on set_devices([0, 0, 0]) replicas and on
    two streams.  After create and after each rebuild: max_depth8 and bvh2_depth are the read-back tree's by the walkers' own traversal;
    that tree is walked to its bound by at least 32 rays (the stack adopt_tree sized is the one the walk fills); every trace mode equals
    the walkers; one frame of two segments equals the numpy integrator; no push is dropped."""
    states = [rebuild_state(cr, *REBUILD_STATES[builder][k]) for k in (0, 1, 0)]
    w, h = REBUILD_FRAME
    sc = cr.Scene(cr.SceneData.for_device_build(states[0].mesh, rebuild_camera(cr), builder), w, h, 2)
    try:
        if fan == "devices":
            sc.set_devices([0, 0, 0])
        elif fan == "streams":
            sc.set_option("streams", 2)
        sc.render_frame(*RVS[0])                                       # the replicas exist and hold the first tree
        depths = []
        for k, st in enumerate(states):
            if k:
                sc.rebuild_vertices(st.mesh.vertices)
            nodes, recs, flat, recs2 = device_tree(sc, True)
            info = sc.bvh_info()
            depths.append(premise_holds(nodes, recs, st.rays))
            assert info["max_depth8"] == depths[-1] and info["bvh2_depth"] == W.depth2(flat), (builder, fan, k)
            check_traces(cr, sc, nodes, recs, flat, recs2, st.rays, (builder, fan, k))
            sc.reset()
            sc.render_frame(*RVS[0])
            assert int((bits(sc.read_sum()) != bits(st.want)).sum()) == 0, (builder, fan, k)
            assert sc.frame_stats()["stack_overflows"] == 0
        assert depths[1] > depths[0] == depths[2], depths
    finally:
        sc.close()


def nested_vertices(n, step):
    """n triangles (0, 0, 0) (s, 0, 0) (0, s, s), s = 2^(step k - 59): nested boxes of growing size, which the PLOC and SAH builders
    turn into combs — at n = 60, step 2 into CWBVHs of depth 27 and 25 by their numpy references (tests/bvh_build_ref.py, cwbvh_ref.py)"""
    V = np.zeros((3 * n, 3), f32)
    s = np.ldexp(1.0, (step * np.arange(n) - 59).astype(int)).astype(f32)
    V[1::3, 0], V[2::3, 1], V[2::3, 2] = s, s, s
    return V


def nested_mesh(cr, V):
    n = V.shape[0] // 3
    T = np.zeros((n, 12), np.int32)
    T[:, 0:3] = np.arange(3 * n).reshape(n, 3)
    T[:, 4:8], T[:, 8:12] = (0, 0, 0, 1), (-1, -1, -1, 0)
    mats = np.full((1, 16), -1.0, f32)
    mats[0, 0:4], mats[0, 4:8], mats[0, 8:12] = (0.7, 0.6, 0.5, 0.0), (0, 0, 0, -1), 0.0
    return cr.Mesh(V, np.array([[0, 0, 1]], f32), np.zeros((0, 2), f32), T, mats, np.zeros((0, 18), f32))


# -- the cap

@pytest.mark.gpu
def test_gpu_a_device_build_beyond_the_cap_is_refused_at_create_and_at_rebuild(cr):
    """60 triangles nested by a factor 4 each: the SAH builder's tree converts to a CWBVH of depth 25 by the numpy references
    (tests/bvh_build_ref.py, tests/cwbvh_ref.py).  Create refuses it with CRT_ERR_LIMIT and a text that names the stack; so does a rebuild
    of a scene of 60 spread-out triangles, which afterwards gives the bytes and the walks it gave before.  (PLOC's BVH2 of the same input
    is 59 levels deep and meets the builder's own bound of 56 levels first; the linear BVH's Morton codes keep it at depth 7.)"""
    n = 60
    rng = np.random.default_rng(31)
    spread = np.repeat(rng.uniform(0, 8, (n, 3)), 3, 0).astype(f32) + np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1]], f32), (n, 1))
    too_deep = nested_vertices(n, 2)
    rays = seeded_rays(nested_mesh(cr, spread), 256, 5, cr.RAY_DT)
    aim = spread.reshape(n, 3, 3).mean(1)[np.arange(128) % n] - rays["o"][::2]                     # every other ray at a triangle's centroid
    rays["d"][::2] = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(f32)
    assert (numpy_brute_force(nested_mesh(cr, spread), rays)[0] >= 0).sum() >= 128
    with pytest.raises(cr.CrtError) as e:
        cr.Scene(cr.SceneData.for_device_build(nested_mesh(cr, too_deep), None, "sah"), 8, 8, 1)
    assert_refused(e, "CRT_ERR_LIMIT", "deeper than the traversal stack")
    sc = cr.Scene(cr.SceneData.for_device_build(nested_mesh(cr, spread), None, "sah"), 8, 8, 1)
    try:
        before = device_tree(sc, True)
        check_traces(cr, sc, *before, rays, "before")
        hits = sc.trace(rays)
        assert (hits["tri"] >= 0).sum() >= 32
        with pytest.raises(cr.CrtError) as e:
            sc.rebuild_vertices(too_deep)
        assert_refused(e, "CRT_ERR_LIMIT", "deeper than the traversal stack")
        for a, b in zip(before, device_tree(sc, True)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.array_equal(hits.view(np.uint8), sc.trace(rays).view(np.uint8))
        assert sc.bvh_info()["max_depth8"] == W.depth8(before[0])
        assert sc.frame_stats()["stack_overflows"] == 0
    finally:
        sc.close()


@pytest.mark.gpu
def test_gpu_depth_17_and_a_given_bvh2_of_depth_95_are_refused_at_create(cr):
    """Depth 16 is accepted (every test above); depth 17 is refused with a text that names the stack.  A BVH2 of depth 95 handed to
    create is refused too, with CRT_ERR_LIMIT: the walk's 96 rows hold depth + 2, and create does not drop a BVH2 it was given.  The
    scene made from that comb's CWBVH alone walks as the walker does; having no BVH2 at all, it refuses the BVH2 trace mode and the BVH2
    frame mode, each by its own message.  (A BVH2 BUILT on the device and then not kept, DeviceTree::keep_bvh2, has no test: no input
    was found whose BVH2 is 95 levels deep under a CWBVH of 16 or fewer.)"""
    fam = family(cr)
    with pytest.raises(cr.CrtError) as e:
        cr.Scene(fam["comb8-17"].data, 8, 8, 1)
    assert_refused(e, "CRT_ERR_LIMIT", "deeper than the traversal stack")
    t = fam["comb2-95"]
    with pytest.raises(cr.CrtError) as e:
        cr.Scene(t.data, 8, 8, 1)
    assert_refused(e, "CRT_ERR_LIMIT", "BVH2 deeper than 94 levels")
    data = cr.SceneData(t.mesh, types.SimpleNamespace(triangles=t.leaf, triangle_indices=t.ids, flat_nodes=None),
                        types.SimpleNamespace(nodes=t.nodes, tri_slots=t.tri_slots), t.cam)
    sc = cr.Scene(data, 8, 8, 1)
    try:
        with pytest.raises(cr.CrtError) as e:
            sc.trace(t.rays, BVH2_MODE)
        assert_refused(e, "CRT_ERR_INVALID", "crt_trace: the scene was created without a BVH2")
        with pytest.raises(cr.CrtError) as e:
            sc.set_option("accel", 1)
        assert_refused(e, "CRT_ERR_INVALID", "crt_set_option: the scene was created without a BVH2")
        nodes, recs, _, _ = device_tree(sc, False)
        assert np.array_equal(nodes, t.nodes)
        check_traces(cr, sc, nodes, recs, None, None, t.rays, "comb2-95 through its CWBVH")
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fan", ["devices", "streams"])
def test_gpu_replicas_hold_the_full_stack_across_a_refit(cr, fan):
    """the depth-16 tree on replicas of one GPU (set_devices with the same id, option streams), seen by the pinhole beside the slab
    whose rays hold all 15 entries (test_gpu_lean_last_segment_build_holds_the_full_stack shows it): after a refit to twice the size the
    fanned frame is the single scene's, after the refit back it is the numpy integrator's; no replica drops a push"""
    t = family(cr)["bush8-16"]
    w, h = 64, 16
    want = ir.render(ir.RefScene(t.mesh, side_camera(cr), w, h), RVS, 2)[0][1]
    assert (want.reshape(-1, 3) != 0).any(1).mean() >= 0.25

    def frames(sc):
        sc.reset()
        for rx, ry in RVS:
            sc.render_frame(rx, ry)
        assert sc.frame_stats()["stack_overflows"] == 0
        return sc.read_sum()

    data = side_scene_data(cr, t)
    multi, single = cr.Scene(data, w, h, 2), cr.Scene(data, w, h, 2)
    try:
        if fan == "devices":
            multi.set_devices([0, 0, 0])
        else:
            multi.set_option("streams", 2)
        assert int((bits(frames(multi)) != bits(want)).sum()) == 0             # the replicas exist
        for sc in (multi, single):
            sc.update_vertices((t.V * f32(2.0)).astype(f32))
        assert multi.bvh_info()["max_depth8"] == 16
        moved = frames(single)
        assert np.array_equal(bits(frames(multi)), bits(moved)) and (bits(moved) != bits(want)).any()
        multi.update_vertices(t.V)
        assert int((bits(frames(multi)) != bits(want)).sum()) == 0
    finally:
        multi.close(); single.close()


@pytest.mark.gpu
def test_gpu_pinhole_ao_fog_and_first_hit_buffers_on_the_grid(cr, ob):
    """one render_ao, render_fog and render_aov of the grid from above, against tests/ao_ref.py, tests/fog_ref.py and test_aov's reference"""
    import ao_ref
    import fog_ref
    from test_aov import assert_channels, flat_reference, read_all
    t = family(cr)["grid32"]
    w, h, rv = 24, 16, RVS[0]
    ref = ir.RefScene(t.mesh, t.cam, w, h)
    ao_want, _ = ao_ref.render_ao(ref, *rv, 4)
    p = fog_ref.Params(K=4, density=0.02, max_distance=200.0)
    fog_want, _ = fog_ref.render_fog(ref, *rv, p)
    aov_want = flat_reference(cr, ob, "walk_ref grid32", "given", t.mesh, t.data, t.cam, w, h, rv, 1)
    assert (ao_want[..., 3] > 0).mean() >= 0.25 and (fog_want[..., :3] != 0).any(-1).mean() >= 0.25
    sc = cr.Scene(t.data, w, h, 1)
    try:
        sc.render_ao(*rv, samples=4)
        assert int((bits(sc.read_ao()) != bits(ao_want)).sum()) == 0
        assert sc.frame_stats()["stack_overflows"] == 0
        sc.render_fog(*rv, samples=4, density=0.02, max_distance=200.0)
        assert int((bits(sc.read_fog()) != bits(fog_want)).sum()) == 0
        assert sc.frame_stats()["stack_overflows"] == 0
        sc.render_aov(*rv)
        assert_channels(cr, read_all(cr, sc), aov_want, "grid32")
        assert sc.frame_stats()["stack_overflows"] == 0
    finally:
        sc.close()
