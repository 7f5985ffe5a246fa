"""The GPU BVH builders (caitlynrenderer_amd/csrc/lbvh.hip: LBVH, PLOC, binned SAH) held to the plain numpy references of
tests/bvh_build_ref.py, tree for tree and byte for byte.

Without a GPU the references are held to themselves: validity, the Morton order against a bit-by-bit loop, the recursive radix tree
against Karras' per-node rule, the exact sweep against a float64 brute force, and a seeded search for an input that takes PLOC's forced
merge.  On the GPU every case asserts flat_nodes.view(uint32) == reference and triangle_indices == reference; bvh_build_ref.first_difference
says where two trees part."""
import numpy as np
import pytest

import bvh_build_ref as R

f32 = np.float32


# ---------------------------------------------------------------- meshes ----

def _mesh(vertices):
    v = np.ascontiguousarray(vertices, f32).reshape(-1, 3)
    t = np.zeros((v.shape[0] // 3, 12), np.int32)
    t[:, :3] = np.arange(v.shape[0]).reshape(-1, 3)
    return t, v


def _soup_vertices(n, seed):
    """n random triangles: a point uniform in a 4^3 box plus, per vertex, an offset of at most 0.2 per axis"""
    rng = np.random.default_rng(seed)
    return (4.0 * rng.random((n, 1, 3)) + 0.2 * (2.0 * rng.random((n, 3, 3)) - 1.0)).astype(f32)


def soup(n, seed=1):
    return _mesh(_soup_vertices(n, seed))


def flat(n, seed=2):
    v = _soup_vertices(n, seed)
    v[:, :, 2] = f32(1.25)                                          # one centroid extent is 0
    return _mesh(v)


def dups(n):
    return _mesh(np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32), (n, 1)))


def clustered(n, seed=3):
    """a soup whose first half is squeezed into a cube of edge ~0.017 around (2.03, 2.03, 2.03); the last two triangles are far outliers
    that set the scene box to ~100 per axis, so a Morton cell is ~0.098 wide"""
    v = _soup_vertices(n, seed)
    v[: n // 2] = (f32(2.03) + f32(0.004) * (v[: n // 2] - f32(2.0))).astype(f32)
    v[n - 2] = v[n - 2] - f32(40.0)
    v[n - 1] = v[n - 1] + f32(60.0)
    return _mesh(v)


def small_integer_mesh(rng, n, top):
    return _mesh(rng.integers(0, top + 1, (n, 3, 3)).astype(f32))


MESHES = {"flat1000": lambda: flat(1000), "flat3000": lambda: flat(3000), "dups50": lambda: dups(50), "dups300": lambda: dups(300),
          "dups5000": lambda: dups(5000), "clustered3000": lambda: clustered(3000)}
_mesh_cache, _ref_cache = {}, {}


def mesh_of(label, tess8=None):
    if label == "tess8":
        return tess8[0].triangles, tess8[0].vertices
    if label not in _mesh_cache:
        _mesh_cache[label] = MESHES[label]() if label in MESHES else soup(int(label[4:]))
    return _mesh_cache[label]


def reference(builder, param, label, tess8=None):
    """every reference tree is built once per (builder, parameter, mesh) and never modified"""
    key = (builder, param, label)
    if key not in _ref_cache:
        t, v = mesh_of(label, tess8)
        _ref_cache[key] = {"lbvh": lambda: R.ref_lbvh(t, v), "ploc": lambda: R.ref_ploc(t, v, param), "sah": lambda: R.ref_sah(t, v, param)}[builder]()
        for a in _ref_cache[key]:
            a.setflags(write=False)
    return _ref_cache[key]


def assert_same_tree(flat_nodes, order, ref):
    diff = R.first_difference(flat_nodes, order, ref[0], ref[1])
    assert diff is None, diff
    assert np.array_equal(flat_nodes.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(order, ref[1])


# ---------------------------------------------------------------- CPU: the references held to themselves ----

SELF_CHECK = [("lbvh", 0), ("ploc", 4), ("ploc", 0), ("ploc", 64), ("sah", 0), ("sah", 16), ("sah", 32)]


@pytest.mark.parametrize("label", ["soup1", "soup2", "soup3", "soup33", "soup257", "soup1300", "flat1000", "dups300", "clustered3000"])
def test_reference_trees_are_valid(label):
    """Every reference output is a valid BVH2 in the documented layout over the input's boxes and a permutation of its triangles.
    (The references raise on the refused input classes, so a pass also says the meshes stay clear of them.)"""
    t, v = mesh_of(label)
    lo, hi = R.triangle_boxes(t, v)
    for builder, param in SELF_CHECK:
        flat_nodes, order = reference(builder, param, label)
        R.check_tree(flat_nodes, order, lo, hi)
        assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(t.shape[0])), (builder, param)
        assert R.first_difference(flat_nodes, order, flat_nodes.copy(), order.copy()) is None


def test_first_difference_names_the_node():
    t, v = mesh_of("soup33")
    a, oa = reference("sah", 0, "soup33")
    b, ob_ = reference("lbvh", 0, "soup33")
    assert "first node whose link" in R.first_difference(a, oa, b, ob_)
    c = a.copy()
    leaf = int(np.nonzero(c[:, 7] != 0)[0][-1])
    c[leaf, 0] -= 1
    msg = R.first_difference(a, oa, c, oa)
    assert "deepest node whose box differs" in msg and f"node {leaf} " in msg
    o2 = oa.copy()
    o2[[3, 4]] = o2[[4, 3]]
    assert R.first_difference(a, oa, a, o2) is not None


def test_the_references_refuse_what_c_leaves_undefined():
    t, v = soup(20)
    for bad in (np.inf, np.nan, 3e19, -0.0):
        vb = v.copy()
        vb[7, 1] = bad
        for build in (R.ref_lbvh, R.ref_ploc, R.ref_sah):
            with pytest.raises(R.RefusedInput):
                build(t, vb)
    vb = np.zeros_like(v)
    vb[3:, 0] = f32(2.0 ** -110)                                    # a nonzero centroid extent below 2^-100
    for build in (R.ref_lbvh, R.ref_sah):
        with pytest.raises(R.RefusedInput):
            build(t, vb)
    boxes = np.zeros((3, 6), f32)
    boxes[1, 3] = np.inf
    with pytest.raises(R.RefusedInput):
        R.ref_sah_boxes(boxes)


def _code_bit_by_bit(cells):
    code = 0
    for b in range(10):
        for a in range(3):                                          # x lands above y above z in every triple
            if (int(cells[a]) >> b) & 1:
                code += 1 << (3 * b + (2 - a))
    return code


@pytest.mark.parametrize("label", ["soup257", "flat1000", "dups50", "clustered3000"])
def test_morton_order_is_the_lexsort_of_index_and_code(label):
    t, v = mesh_of(label)
    lo, hi = R.triangle_boxes(t, v)
    cen = (f32(0.5) * (lo + hi)).astype(f32)
    cmin, ext = cen.min(0), (cen.max(0) - cen.min(0)).astype(f32)
    code = np.zeros(t.shape[0], np.int64)
    for i in range(t.shape[0]):
        cells = [min(max(int(f32(f32(f32(cen[i, a] - cmin[a]) / ext[a]) * f32(1024))), 0), 1023) if ext[a] > 0 else 0 for a in range(3)]
        code[i] = _code_bit_by_bit(cells)
    assert np.array_equal(code, R.morton_codes(lo, hi).astype(np.int64))
    order = np.lexsort((np.arange(t.shape[0]), code))
    assert np.array_equal(reference("lbvh", 0, label)[1], order)
    if label == "clustered3000":                                    # what the mesh is for: a big run of equal codes
        assert np.unique(code, return_counts=True)[1].max() >= t.shape[0] // 4


def _karras_tree(keys):
    """Karras 2012, section 4, as written there but with linear scans instead of the binary searches: internal node i, leaf j = n-1+j"""
    n = len(keys)

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - (keys[i] ^ keys[j]).bit_length()
    left, right, slot = [-1] * (2 * n - 1), [-1] * (2 * n - 1), [-1] * (n - 1) + list(range(n))
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        l = 0
        while delta(i, i + (l + 1) * d) > dmin:
            l += 1
        j = i + l * d
        dnode = delta(i, j)
        s = 0
        while delta(i, i + (s + 1) * d) > dnode:
            s += 1
        gamma = i + s * d + min(d, 0)
        left[i] = n - 1 + gamma if min(i, j) == gamma else gamma
        right[i] = n - 1 + gamma + 1 if max(i, j) == gamma + 1 else gamma + 1
    return left, right, slot


@pytest.mark.parametrize("label", ["soup257", "soup300", "dups50", "clustered300"])
def test_recursive_radix_tree_equals_karras_per_node_rule(label):
    t, v = clustered(300) if label == "clustered300" else mesh_of(label)
    lo, hi = R.triangle_boxes(t, v)
    keys, order = R.morton_order(lo, hi)
    if label == "clustered300":
        assert np.unique(keys >> np.uint64(32), return_counts=True)[1].max() >= 75          # many duplicate codes
    a = R._emit(0, *R.radix_tree(keys), order, lo, hi)
    b = R._emit(0, *_karras_tree([int(k) for k in keys]), order, lo, hi)
    assert R.first_difference(*a, *b) is None
    assert R.first_difference(*a, *R.ref_lbvh(t, v)) is None


def _area64(lo, hi):
    """the half-area of tests/test_rebuild.py's cost definition: float32 corners, float64 arithmetic"""
    d = hi.astype(np.float64) - lo.astype(np.float64)
    return (d[0] * d[1] + d[1] * d[2]) + d[2] * d[0]


def _triangles_below(flat_nodes, order, p):
    if flat_nodes[p, 7] != 0:
        return [int(order[int(flat_nodes[p, 3])])]
    l = int(flat_nodes[p, 3])
    return _triangles_below(flat_nodes, order, l) + _triangles_below(flat_nodes, order, l + 1)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_exact_sweep_equals_the_float64_brute_force(n):
    """With bins switched off (n <= small) the SAH reference is greedy per node.  On small integer coordinates fp32 and fp64 agree
    exactly, so each node's split must be THE argmin of the float64 cost over all 3 (c - 1) sorted splits: a strictly smaller cost
    wins, in axis order 0, 1, 2 and ascending position."""
    rng = np.random.default_rng(100 + n)
    for case in range(12):
        t, v = small_integer_mesh(rng, n, 7 if case % 2 else 2)      # 0..2: many equal centroids and costs
        lo, hi = R.triangle_boxes(t, v)
        cen = (lo.astype(np.float64) + hi) / 2
        for small in (8, 32):
            flat_nodes, order = R.ref_sah(t, v, small)
            R.check_tree(flat_nodes, order, lo, hi)
            for p in np.nonzero(flat_nodes[:, 7] == 0)[0]:
                l = int(flat_nodes[p, 3])
                got_left, got_right = _triangles_below(flat_nodes, order, l), _triangles_below(flat_nodes, order, l + 1)
                tris = sorted(got_left + got_right)
                best, want = np.inf, None
                for a in range(3):
                    srt = sorted(tris, key=lambda k: (cen[k, a], k))
                    for i in range(1, len(srt)):
                        L, Rr = srt[:i], srt[i:]
                        cost = _area64(lo[L].min(0), hi[L].max(0)) * len(L) + _area64(lo[Rr].min(0), hi[Rr].max(0)) * len(Rr)
                        if cost < best:
                            best, want = cost, (L, Rr)
                chosen = (_area64(lo[got_left].min(0), hi[got_left].max(0)) * len(got_left) +
                          _area64(lo[got_right].min(0), hi[got_right].max(0)) * len(got_right))
                assert chosen == best, (n, case, small, int(p))
                assert sorted(got_left) == sorted(want[0]) and sorted(got_right) == sorted(want[1]), (n, case, small, int(p))


FORCED_SEARCH_CASES = 4000


def _forced_search(cases):
    """-> [(case, radius, n, vertices)] of the inputs on which ref_ploc took the forced merge"""
    rng = np.random.default_rng(2024)
    found = []
    for case in range(cases):
        n = int(rng.integers(3, 17))
        radius = int(rng.choice([1, 2, 3, 4, 16]))
        t, v = small_integer_mesh(rng, n, 3)
        forced = []
        R.ref_ploc(t, v, radius, forced)
        if forced:
            found.append((case, radius, n, v))
    return found


def test_search_for_an_input_that_takes_plocs_forced_merge():
    """At 1,024 clusters or fewer an iteration without a mutual pair merges positions 0 and 1.  The search: 4,000 seeded inputs of 3..16
    triangles with integer coordinates 0..3 (ties everywhere), radius 1, 2, 3, 4 or 16, about 6 s.  NONE takes the branch (nor did a
    one-off run over 120,000 more with coordinates 0..1, 0..2 and 0..3), so there is no GPU case for it and the branch stays untested;
    DESIGN.md §21 says so and gives the argument why no finite input can reach it.  Should the reference ever change so that an input
    is found, this test fails and names it: it then belongs into PLOC_CASES."""
    found = _forced_search(FORCED_SEARCH_CASES)
    assert found == [], [(c, r, n, v.astype(int).tolist()) for c, r, n, v in found]


# ---------------------------------------------------------------- GPU: kernel against reference, byte for byte ----

LBVH_CASES = ["soup1", "soup2", "soup3", "soup255", "soup256", "soup257", "soup2049", "tess8", "flat1000", "dups50", "clustered3000"]
PLOC_CASES = ["soup2", "soup3", "soup1024", "soup1025", "soup1300", "soup5000", "tess8", "dups300", "dups5000"]
SAH_CASES = ["soup2", "soup8", "soup9", "soup33", "soup1023", "soup1024", "soup1025", "soup2048", "soup7168", "tess8", "flat3000", "dups300",
             "clustered3000"]


@pytest.mark.gpu
@pytest.mark.parametrize("label", LBVH_CASES)
def test_gpu_lbvh_equals_reference(cr, tess8, label):
    t, v = mesh_of(label, tess8)
    sb = cr.SBVH(t, v, builder="lbvh")
    assert_same_tree(sb.flat_nodes, sb.triangle_indices, reference("lbvh", 0, label, tess8))


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [4, 16, 64])
@pytest.mark.parametrize("label", PLOC_CASES)
def test_gpu_ploc_equals_reference(cr, tess8, label, radius):
    t, v = mesh_of(label, tess8)
    sb = cr.SBVH(t, v, builder=f"ploc{radius}")
    assert_same_tree(sb.flat_nodes, sb.triangle_indices, reference("ploc", radius, label, tess8))


@pytest.mark.gpu
@pytest.mark.parametrize("small", [8, 16, 32])
@pytest.mark.parametrize("label", SAH_CASES)
def test_gpu_sah_equals_reference(cr, tess8, label, small):
    t, v = mesh_of(label, tess8)
    sb = cr.SBVH(t, v, builder=f"sah{small}")
    assert_same_tree(sb.flat_nodes, sb.triangle_indices, reference("sah", small, label, tess8))


@pytest.mark.gpu
def test_gpu_builder_parameter_defaults_and_clamps(cr):
    """radius 0 -> 16, capped at 64; small 0 -> 8, clamped to [8, 32]"""
    t, v = mesh_of("soup1300")
    for builder, ref in (("ploc", ("ploc", 16)), ("ploc200", ("ploc", 64)), ("sah", ("sah", 8)), ("sah3", ("sah", 8)), ("sah200", ("sah", 32))):
        sb = cr.SBVH(t, v, builder=builder)
        assert_same_tree(sb.flat_nodes, sb.triangle_indices, reference(ref[0], ref[1], "soup1300"))


@pytest.mark.gpu
def test_gpu_morton_order_beyond_one_grid_pass(cr):
    """k_tri_bounds runs at most 1,024 workgroups of 256: from 262,145 triangles on its grid-stride loop takes a second pass.  The
    extreme centroids of every axis lie in the last 257 triangles, which only that pass sees; a scene box without them changes the
    codes, hence the order.  triangle_indices alone is compared (no reference tree at this size)."""
    n = 262_144 + 257
    v = _soup_vertices(n, 9)
    v[-257:] = (f32(2.0) + f32(3.0) * (v[-257:] - f32(2.0))).astype(f32)
    t, v = _mesh(v)
    lo, hi = R.triangle_boxes(t, v)
    cen = f32(0.5) * (lo + hi)
    assert cen.argmin(0).min() >= 262_144 and cen.argmax(0).min() >= 262_144
    sb = cr.SBVH(t, v, builder="lbvh")
    want = R.ref_lbvh_order(t, v)
    assert np.array_equal(sb.triangle_indices, want), int(np.nonzero(sb.triangle_indices != want)[0][0])


def _rigid(rng, n, spread):
    out = np.zeros((n, 3, 4), f32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out[k, :, :3], out[k, :, 3] = q, rng.uniform(-spread, spread, 3)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 9, 300, 1500])
def test_gpu_tlas_equals_reference_over_the_world_boxes(cr, n):
    """sah_build_from_boxes_on_device: no k_tri_bounds, the caller's boxes.  The TLAS node8s are the host conversion of the reference
    tree over world_boxes(), the instance records follow its leaf order (layout: host_scene of tests/test_instances_oracle.py)."""
    rng = np.random.default_rng(40 + n)
    meshes = [(soup(40, 5)[1], soup(40, 5)[0]), (soup(70, 6)[1], soup(70, 6)[0])]
    M, which = _rigid(rng, n, 3.0 * n ** (1 / 3)), rng.integers(0, 2, n)
    sc = cr.InstancedScene(meshes, cr.instances_array(M, which))
    try:
        boxes = sc.world_boxes()
        flat_nodes, order = R.ref_sah_boxes(boxes, 0)
        R.check_tree(flat_nodes, order, boxes[:, :3], boxes[:, 3:])
        cw = cr.CWBVH().convert_arrays(flat_nodes, n)
        tlas = sc.tlas_nodes()
        assert tlas.shape == cw.nodes.shape and np.array_equal(tlas, cw.nodes), int(np.nonzero((tlas != cw.nodes).any(1))[0][0]) if tlas.shape == cw.nodes.shape else (tlas.shape, cw.nodes.shape)
        rec, idx = sc.instance_records(), order[cw.tri_slots]
        assert np.array_equal(rec[:, 12:].copy().view(np.uint32)[:, 1], idx.astype(np.uint32))
        assert np.array_equal(rec[:, :12].copy().view(np.uint32), sc.world_to_object()[idx].copy().view(np.uint32))
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder,ref", [("ploc", ("ploc", 16)), ("sah16", ("sah", 16))])
def test_gpu_blas_equals_reference(cr, builder, ref):
    """lbvh_build_on_device's stride-12 entry, reached through crt_instances_create: the BLAS node8s, rebased to zero, are the host
    conversion of the reference tree."""
    t, v = mesh_of("soup3000")
    sc = cr.InstancedScene([(v, t)], cr.instances_array(np.eye(3, 4, dtype=f32)[None], [0]), builder=builder)
    try:
        region = sc.info()["tlas_bytes"] // 80
        nodes = sc.blas_nodes()
        nodes[:, 16:20] = (nodes[:, 16:20].copy().view(np.uint32) - np.uint32(region)).view(np.uint8)
        cw = cr.CWBVH().convert_arrays(reference(ref[0], ref[1], "soup3000")[0], t.shape[0])
        assert nodes.shape == cw.nodes.shape and np.array_equal(nodes, cw.nodes)
    finally:
        sc.close()
