"""The CWBVH converters (host: crt_cwbvh_convert, device: crt_cwbvh_convert_device) and refits held to tests/cwbvh_ref.py byte for byte
(DESIGN.md §24), and to properties that do not depend on that restatement: tightness of every quantised plane and exponent in exact
arithmetic, optimality of the cost tables against a brute force over every legal collapse, the octant assignment, and exact
power-of-two scale invariance.  One corpus of BVH2 trees serves the CPU cases (host converter) and the GPU cases (device converter)."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import bvh_build_ref as B
import cwbvh_ref as R
import test_builders_ref as TB
from test_host import _validate_cwbvh
from test_refit import _accel, _check_cwbvh_boxes, _cwbvh_refit, _host_side

f32 = np.float32
SCALES = (-60, -20, 20, 28)


# ---------------------------------------------------------------- the corpus ----

SOUPS = ["soup1", "soup2", "soup3", "soup4", "soup8", "soup9", "soup33", "soup257", "soup1300", "soup5000"]
SHAPES = ["flat1000", "dups300", "clustered3000", "tess8"]
BUILDERS = ["lbvh", "ploc", "sah", "sbvh", "sbvh_sah"]
_trees = {}


def base_tree(cr, builder, label, tess8):
    """(flat, n_slots) of one builder over one mesh, built once and never modified.  lbvh / ploc / sah are the numpy references of the GPU
    builders; sbvh / sbvh_sah the host split-BVH with and without spatial splits."""
    key = (builder, label)
    if key not in _trees:
        t, v = TB.mesh_of(label, tess8)
        if builder.startswith("sbvh"):
            s = cr.SBVH(t, v, 1 if builder == "sbvh_sah" else 0)
            flat, n_slots = s.flat_nodes, int(s.triangle_indices.shape[0])
        else:
            flat, order = TB.reference(builder, 0, label, tess8)
            flat, n_slots = flat.copy(), int(order.shape[0])
        flat.setflags(write=False)
        _trees[key] = (flat, n_slots)
    return _trees[key]


def scaled(flat, k):
    out = flat.copy()
    out[:, [0, 1, 2, 4, 5, 6]] = np.ldexp(flat[:, [0, 1, 2, 4, 5, 6]], k)
    return out


def variants(flat):
    """name -> tree: as built, times 2^k, translated (coarse ulps, many equal coordinates; rounding is monotone, so parents still contain
    their children) and mirrored to negative coordinates"""
    out = {"as built": flat}
    for k in SCALES:
        out[f"x 2^{k}"] = scaled(flat, k)
    for off in (1e3, 1e6):
        t = flat.copy()
        t[:, [0, 1, 2, 4, 5, 6]] = (flat[:, [0, 1, 2, 4, 5, 6]] + f32(off)).astype(f32)
        out[f"+ {off:g}"] = t
    m = flat.copy()
    m[:, 0:3], m[:, 4:7] = -flat[:, 4:7], -flat[:, 0:3]
    out["mirrored"] = m
    return out


def _flat_from(left, boxes_lo, boxes_hi, leaf_start, leaf_count, root=0):
    """A breadth-first (n, 8) array from child lists: left[i] = (a, b) or None for a leaf; interior boxes are the unions"""
    ids, queue = [], [root]
    while queue:
        i = queue.pop(0)
        ids.append(i)
        if left[i] is not None:
            queue += list(left[i])
    pos = {i: p for p, i in enumerate(ids)}
    flat = np.zeros((len(ids), 8), f32)
    for p in range(len(ids) - 1, -1, -1):
        i = ids[p]
        if left[i] is None:
            flat[p, 0:3], flat[p, 4:7], flat[p, 3], flat[p, 7] = boxes_lo[i], boxes_hi[i], leaf_start[i], leaf_count[i]
        else:
            a, b = pos[left[i][0]], pos[left[i][1]]
            assert b == a + 1
            flat[p, 0:3], flat[p, 4:7], flat[p, 3] = np.minimum(flat[a, 0:3], flat[b, 0:3]), np.maximum(flat[a, 4:7], flat[b, 4:7]), a
    return flat


def chain(depth, side, seed=5):
    """A one-sided BVH2 of `depth` interior levels: every interior node has one leaf and the rest of the chain"""
    rng = np.random.default_rng(seed)
    n_leaves = depth + 1
    lo = (np.arange(n_leaves)[:, None] * f32(0.75) + rng.random((n_leaves, 3))).astype(f32)
    hi = (lo + f32(0.25) + rng.random((n_leaves, 3)).astype(f32)).astype(f32)
    left, blo, bhi, start, count = {}, {}, {}, {}, {}
    for d in range(depth):                                                      # node 2d = interior, 2d + 1 = its leaf
        leaf, rest = 2 * d + 1, 2 * d + 2
        left[2 * d] = (leaf, rest) if side == "right" else (rest, leaf)
        left[leaf] = None
        blo[leaf], bhi[leaf], start[leaf], count[leaf] = lo[d], hi[d], d, 1
    last = 2 * depth
    left[last] = None
    blo[last], bhi[last], start[last], count[last] = lo[depth], hi[depth], depth, 1
    return _flat_from(left, blo, bhi, start, count), n_leaves


def wide_tree(level_sizes, seed=9):
    """A BVH2 made to collapse into a node8 tree whose levels hold level_sizes nodes: an octree of cells, every node8 a balanced binary
    tree over its children.  A node8 with fewer than 7 children would pull grandchildren into its free slots, so every node8 that has
    node8 children has 7 or 8 of them (the first nodes of a level in depth-first order; as few as the next level's size allows), and
    every other one holds 8 single-triangle leaves that fill the octants of its cell.  Whether the converter sees it that way is its
    cost tables' business: the test reads the level sizes back."""
    rng = np.random.default_rng(seed)
    left, blo, bhi, start, count = {}, {}, {}, {}, {}
    counter = itertools.count()
    n_tris = itertools.count()
    kids_of = []                                                                # per level: the child counts of its parents, in order
    for d in range(len(level_sizes) - 1):
        size, kids = level_sizes[d], level_sizes[d + 1]
        parents = (kids + 7) // 8
        assert parents <= size and (7 * parents <= kids or parents == 1), (d, parents)
        kids_of.append([kids // parents + (1 if i < kids % parents else 0) for i in range(parents)])

    def balanced(items):
        if len(items) == 1:
            return items[0]
        node = next(counter)
        half = (len(items) + 1) // 2
        left[node] = (balanced(items[:half]), balanced(items[half:]))
        return node

    def cell(origin, size, depth):
        corners = [origin + size * 0.5 * np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1], np.float64) for c in range(8)]
        if depth == len(level_sizes) - 1 or not kids_of[depth]:
            kids = []
            for c in corners:
                leaf = next(counter)
                left[leaf] = None
                a = c + size * 0.02 * (1.0 + rng.random(3))                     # leaves that fill their octants: halving a cell costs more
                blo[leaf], bhi[leaf], start[leaf], count[leaf] = a.astype(f32), (a + size * 0.4).astype(f32), next(n_tris), 1
                kids.append(leaf)
            return balanced(kids)
        n_kids = kids_of[depth].pop(0)
        return balanced([cell(corners[c] + size * 0.02, size * 0.45, depth + 1) for c in range(n_kids)])

    root = cell(np.zeros(3), 64.0, 0)
    return _flat_from(left, blo, bhi, start, count, root), next(n_tris)


def with_leaf_size(flat, size):
    out = flat.copy()
    leaf = out[:, 7] != 0
    out[leaf, 3] = out[leaf, 3] * size
    out[leaf, 7] = size
    return out, int(leaf.sum()) * size


WIDE = {"wide63": [1, 8, 63], "wide64": [1, 8, 64], "wide65": [1, 8, 15, 65], "wide255": [1, 8, 35, 255], "wide256": [1, 8, 35, 256],
        "wide257": [1, 8, 36, 257]}
HAND = (["chain-left5", "chain-right5", "chain-left64", "chain-right64", "chain-left300", "chain-right300"] + sorted(WIDE)
        + ["threes33", "threes257", "ones257"])
_hand = {}


def hand_tree(label):
    if label not in _hand:
        if label.startswith("chain"):
            side, depth = ("left", label[10:]) if label.startswith("chain-left") else ("right", label[11:])
            _hand[label] = chain(int(depth), side)
        elif label in WIDE:
            _hand[label] = wide_tree(WIDE[label])
        else:
            flat, _ = TB.reference("sah", 0, "soup" + "".join(ch for ch in label if ch.isdigit()))
            _hand[label] = with_leaf_size(flat, 3 if label.startswith("threes") else 1)
        _hand[label][0].setflags(write=False)
    return _hand[label]


def corpus_member(cr, name, tess8):
    """name = 'builder/mesh' or a hand-made label -> (flat, n_slots)"""
    if "/" in name:
        builder, label = name.split("/")
        return base_tree(cr, builder, label, tess8)
    return hand_tree(name)


BUILT = [f"{b}/{m}" for m in SOUPS + SHAPES for b in BUILDERS]
CORPUS = BUILT + HAND


# ---------------------------------------------------------------- properties in exact arithmetic ----

def bvh2_of_nodes(cw):
    """the BVH2 node every node8 stands for, from the converter's child map"""
    f = R.fields(cw.nodes)
    out = np.full(cw.nodes.shape[0], -1, np.int64)
    out[0] = 0
    for i in range(cw.nodes.shape[0]):                                          # children have larger indices than their parent
        for s in range(8):
            if (f["imask"][i] >> s) & 1:
                out[R.inner_child(f, i, s)] = cw.child_bvh2[i, s]
    assert (out >= 0).all()
    return out


def check_tightness(cw, flat):
    """p is the node's lo.  e is the smallest exponent whose 255 steps reach the node's hi (never below the floor of a zero extent).
    Inside the frame [p, p + 255 * 2^(e-127)] q_lo is the LARGEST step at or below the child's lo and q_hi the SMALLEST at or above the
    child's hi: the next step on either side is wrong.  All comparisons exact (cwbvh_ref.sign_of_sum_minus, itself checked against
    fractions below).  Returns (axes checked, planes checked)."""
    f = R.fields(cw.nodes)
    node2 = bvh2_of_nodes(cw)
    lo, hi = flat[node2, 0:3], flat[node2, 4:7]
    assert np.array_equal(f["p"].view(np.uint32), lo.view(np.uint32)), "the origin is not the node's lower corner"
    e = f["e"].astype(np.int64)
    assert ((e >= 1) & (e <= 254)).all()
    p, lo64, hi64 = f["p"].astype(np.float64), lo.astype(np.float64), hi.astype(np.float64)
    reach = R.sign_of_sum_minus(p, 255.0 * R.scale_of(e), hi64) >= 0
    assert (reach | (e == 254)).all(), "255 steps do not reach the node's upper corner"
    reach_below = R.sign_of_sum_minus(p, 255.0 * R.scale_of(np.maximum(e - 1, 1)), hi64) >= 0
    minimal = (e == 1) | ~reach_below
    assert (minimal | (e == R.E_FLOOR)).all(), f"{int((~minimal & (e != R.E_FLOOR)).sum())} exponents are larger than needed"
    occupied = cw.child_bvh2 >= 0
    assert np.array_equal(occupied, f["meta"] != 0)
    kid = np.where(occupied, cw.child_bvh2, 0)
    scale = R.scale_of(e)[:, None, :]
    pp = p[:, None, :]
    for col, which, sense in ((slice(0, 3), 0, -1), (slice(4, 7), 1, 1)):
        c = flat[kid][:, :, col].astype(np.float64)                              # (n8, slot, axis)
        q = f["q"][:, :, which, :].transpose(0, 2, 1).astype(np.float64)         # (n8, slot, axis)
        here = R.sign_of_sum_minus(pp, q * scale, c)
        step = R.sign_of_sum_minus(pp, (q - sense) * scale, c)                   # one step towards the box
        contains = (here * sense >= 0) | (q == (255 if sense > 0 else 0))        # outside the frame the plane is clamped
        tight = (step * sense < 0) | (q == (0 if sense > 0 else 255))
        assert (contains | ~occupied[:, :, None]).all(), "a plane cuts into its child"
        assert (tight | ~occupied[:, :, None]).all(), "a plane is at least one step looser than it has to be"
    assert (f["q"].transpose(0, 3, 1, 2)[~occupied] == 0).all()
    return 3 * cw.nodes.shape[0], 6 * int(occupied.sum())


def check_scaled_output(base, got, flat, k):
    """the conversion of the tree times 2^k: origins times 2^k, exponents plus k except on an axis without extent, all else equal"""
    assert got.nodes.shape == base.nodes.shape and got.depth == base.depth
    assert np.array_equal(got.tri_slots, base.tri_slots) and np.array_equal(got.child_bvh2, base.child_bvh2)
    assert np.array_equal(got.nodes[:, 15:], base.nodes[:, 15:])
    pb, pg = R.fields(base.nodes)["p"], R.fields(got.nodes)["p"]
    assert np.array_equal(np.ldexp(pb, k).view(np.uint32), pg.view(np.uint32))
    node2 = bvh2_of_nodes(base)
    has_extent = flat[node2, 4:7] != flat[node2, 0:3]
    eb, eg = base.nodes[:, 12:15].astype(np.int64), got.nodes[:, 12:15].astype(np.int64)
    assert np.array_equal((eb + k)[has_extent], eg[has_extent])
    assert (eg[~has_extent] == R.E_FLOOR).all() and (eb[~has_extent] == R.E_FLOOR).all()


def assert_same(got, want, what):
    assert got.nodes.shape == want.nodes.shape, (what, got.nodes.shape, want.nodes.shape)
    diff = np.argwhere(got.nodes != want.nodes)
    assert diff.shape[0] == 0, f"{what}: {diff.shape[0]} bytes differ, first at node {diff[0][0]} byte {diff[0][1]}"
    assert np.array_equal(got.tri_slots, want.tri_slots), what
    assert np.array_equal(got.child_bvh2, want.child_bvh2), what
    assert got.depth == want.depth, what


_ref_out = {}


def ref_convert(name, variant, flat, n_slots):
    """the reference's output, computed once per corpus member and variant and shared by the CPU and the GPU case"""
    key = (name, variant)
    if key not in _ref_out:
        _ref_out[key] = R.convert(flat, n_slots)
        for a in _ref_out[key][:3]:
            a.setflags(write=False)
    return _ref_out[key]


# ---------------------------------------------------------------- CPU ----

def test_exact_sign_agrees_with_fractions():
    rng = np.random.default_rng(11)
    n = 4000
    mant = rng.integers(-2 ** 24, 2 ** 24, (3, n)).astype(np.float64)
    expo = rng.choice([-90, -60, -30, -24, -1, 0, 1, 23, 30, 60, 90], (3, n))
    p, t, c = np.ldexp(mant, expo)
    c[::3] = p[::3] + t[::3]                                                    # near ties: the rounded sum, compared with the exact one
    got = R.sign_of_sum_minus(p, t, c)
    for i in range(n):
        d = Fraction(float(p[i])) + Fraction(float(t[i])) - Fraction(float(c[i]))
        assert got[i] == (d > 0) - (d < 0), (p[i], t[i], c[i])
    assert (got != 0).any() and (got == 0).any() and (got[::3] != 0).any()


@pytest.mark.parametrize("name", CORPUS)
def test_host_converter_equals_the_reference_and_is_tight(cr, tess8, name):
    """Byte for byte on every variant of the member; every plane and exponent tight in exact arithmetic; the structural validity check
    of test_host.py; exact scale invariance of the host output."""
    flat, n_slots = corpus_member(cr, name, tess8)
    base = None
    for variant, tree in variants(flat).items():
        got = cr.CWBVH().convert_arrays(tree, n_slots)
        assert_same(got, ref_convert(name, variant, tree, n_slots), f"{name} {variant}")
        axes, planes = check_tightness(got, tree)
        assert axes >= 3 and planes >= 6
        if variant == "as built":
            base = got
            _validate_cwbvh(got, tree)
        elif variant.startswith("x 2^"):
            check_scaled_output(base, got, flat, int(variant[4:]))


def test_the_hand_made_trees_reach_the_level_sizes_they_were_made_for():
    sizes = set()
    for label, want in WIDE.items():
        flat, n_slots = hand_tree(label)
        out = R.convert(flat, n_slots)
        f = R.fields(out.nodes)
        level = np.ones(out.nodes.shape[0], np.int64)
        for i in range(out.nodes.shape[0]):
            for s in range(8):
                if (f["imask"][i] >> s) & 1:
                    level[R.inner_child(f, i, s)] = level[i] + 1
        got = np.bincount(level)[1:].tolist()
        assert got == want, (label, got)
        sizes |= set(got)
    assert {63, 64, 65, 255, 256, 257} <= sizes                                 # one below, at and above a wave and a block of k_discover
    for label, depth in (("chain-left5", 5), ("chain-right300", 300)):
        flat, n_slots = hand_tree(label)
        assert n_slots == depth + 1 and B._depths_and_counts(flat)[0].max() == depth
    for label, size in (("threes33", 3), ("ones257", 1)):
        flat, _ = hand_tree(label)
        assert (flat[flat[:, 7] != 0, 7] == size).all()


def _random_small_tree(rng, n_leaves):
    """a random BVH2 over n_leaves leaves of 1..3 triangles with integer boxes in [0, 12]^3: every area and every sum is exact in fp32"""
    left, blo, bhi, start, count = {}, {}, {}, {}, {}
    counter, slot = itertools.count(), 0

    def grow(n):
        nonlocal slot
        node = next(counter)
        if n == 1:
            left[node] = None
            a = rng.integers(0, 9, 3)
            blo[node], bhi[node] = a.astype(f32), (a + rng.integers(0, 4, 3)).astype(f32)
            count[node] = int(rng.integers(1, 4))
            start[node] = slot
            slot += count[node]
            return node
        k = int(rng.integers(1, n))
        a = grow(k)
        left[node] = (a, grow(n - k))
        return node
    # children must be adjacent in breadth-first order: _flat_from numbers them by a queue, which puts siblings side by side
    grow(n_leaves)
    return _flat_from(left, blo, bhi, start, count), slot


def _brute_force_cost(flat):
    """The least cost over every legal collapse: a node8 costs the half-area of the BVH2 node it stands for; its slots are a frontier of
    at most 8 BVH2 descendants, each either a leaf slot (at most 3 triangles below it, cost area * triangles) or a node8 of its own
    (interior nodes only).  The root is a node8; it may hold itself as its only slot when it has at most 3 triangles."""
    def area(i):
        d = [Fraction(float(flat[i, 4 + k])) - Fraction(float(flat[i, k])) for k in range(3)]
        return d[0] * (d[1] + d[2]) + d[1] * d[2]

    def tris(i):
        return int(flat[i, 7]) if flat[i, 7] != 0 else tris(int(flat[i, 3])) + tris(int(flat[i, 3]) + 1)

    def frontiers(i):
        """every antichain below or at i that covers i's leaves, as tuples of nodes"""
        out = [(i,)]
        if flat[i, 7] == 0:
            l = int(flat[i, 3])
            out += [a + b for a in frontiers(l) for b in frontiers(l + 1)]
        return out

    def slot_cost(i):
        best = None
        if tris(i) <= 3:
            best = area(i) * tris(i)
        if flat[i, 7] == 0:
            c = node8_cost(i)
            best = c if best is None or c < best else best
        return best

    def node8_cost(i):
        l = int(flat[i, 3])
        sets = [a + b for a in frontiers(l) for b in frontiers(l + 1)]
        return area(i) + min(sum(slot_cost(x) for x in fr) for fr in sets if len(fr) <= 8)

    best = node8_cost(0) if flat[0, 7] == 0 else None
    if tris(0) <= 3:
        own = area(0) + area(0) * tris(0)
        best = own if best is None or own < best else best
    return best


def _realised_cost(cw, flat):
    node2 = bvh2_of_nodes(cw)
    f = R.fields(cw.nodes)

    def area(i):
        d = [Fraction(float(flat[i, 4 + k])) - Fraction(float(flat[i, k])) for k in range(3)]
        return d[0] * (d[1] + d[2]) + d[1] * d[2]
    total = sum(area(int(i)) for i in node2)
    for i in range(cw.nodes.shape[0]):
        for s in range(8):
            m = int(f["meta"][i, s])
            if m and not (f["imask"][i] >> s) & 1:
                total += area(int(cw.child_bvh2[i, s])) * bin(m >> 5).count("1")
    return total


def test_cost_tables_find_the_cheapest_collapse(cr):
    """260 random trees: 200 of 2..7 leaves, 60 of 8..11 (where the limit of 8 slots binds)"""
    rng = np.random.default_rng(2024)
    sizes = [int(rng.integers(2, 8)) for _ in range(200)] + [int(rng.integers(8, 12)) for _ in range(60)]
    multi = 0
    for n_leaves in sizes:
        flat, n_slots = _random_small_tree(rng, n_leaves)
        got = cr.CWBVH().convert_arrays(flat, n_slots)
        assert_same(got, R.convert(flat, n_slots), "random small tree")
        assert _realised_cost(got, flat) == _brute_force_cost(flat), flat.tolist()
        multi += got.nodes.shape[0] > 1
    assert multi > 20                                                           # collapses of more than one node8 are among them


def _corner_tree(perm, tie=False):
    """8 unit leaves in the corners of [0, 10]^3 under a complete BVH2; leaf j (left to right) sits in corner perm[j] = 4 x + 2 y + z.
    tie: all eight coincide, 3 triangles each (so that no two of them can share a leaf slot)"""
    left, blo, bhi, start, count = {}, {}, {}, {}, {}
    for j, c in enumerate(perm):
        a = np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1], f32) * f32(9)
        if tie:
            a = np.full(3, 4.5, f32)
        left[7 + j], blo[7 + j], bhi[7 + j], start[7 + j], count[7 + j] = None, a, (a + f32(1)).astype(f32), j * (3 if tie else 1), (3 if tie else 1)
    for i in range(7):
        left[i] = (2 * i + 1, 2 * i + 2)
    return _flat_from(left, blo, bhi, start, count)


def test_octant_assignment(cr):
    """Slot s must hold the child on the high side of x iff s & 4, of y iff s & 2, of z iff s & 1: the walk visits slot ^ octant of the ray
    direction in descending order, which is front to back only then.  Eight coincident children tie everywhere: the
    documented scan order puts them in slots 0..7 in left-first order."""
    rng = np.random.default_rng(3)
    for perm in [list(range(8)), list(range(7, -1, -1))] + [rng.permutation(8).tolist() for _ in range(6)]:
        flat = _corner_tree(perm)
        for cw in (cr.CWBVH().convert_arrays(flat, 8), R.convert(flat, 8)):
            assert cw.nodes.shape[0] == 1
            for s in range(8):
                leaf = int(cw.child_bvh2[0, s])
                centre = (flat[leaf, 0:3] + flat[leaf, 4:7]) * 0.5
                assert [bool(x) for x in centre > 5.0] == [bool(s & 4), bool(s & 2), bool(s & 1)], (perm, s)
    flat = _corner_tree(list(range(8)), tie=True)
    for cw in (cr.CWBVH().convert_arrays(flat, 24), R.convert(flat, 24)):
        assert cw.child_bvh2[0].tolist() == list(range(7, 15))
    # two children only, in opposite corners along x: they take the two slots that differ in the x bit
    left = {0: (1, 2), 1: None, 2: None}
    flat = _flat_from(left, {1: f32([8, 0, 0]), 2: f32([0, 0, 0])}, {1: f32([9, 1, 1]), 2: f32([1, 1, 1])}, {1: 0, 2: 1}, {1: 1, 2: 1})
    cw = cr.CWBVH().convert_arrays(flat, 2)
    slots = {int(cw.child_bvh2[0, s]): s for s in range(8) if cw.child_bvh2[0, s] >= 0}
    assert slots[1] & 4 and not slots[2] & 4


# ---------------------------------------------------------------- CPU: what the scales exposed ----

@pytest.mark.parametrize("k", [30, 40, 90, -70])
def test_scales_beyond_the_old_sentinel_convert_exactly(cr, tess8, k):
    """Unscaled areas summed to 1e20 from 2^30 on (a valid tree was refused as 'leaves do not cover the triangle array') and underflowed
    from 2^-70 down; the tables are formed from extents scaled by a power of two taken from the root box, so both ends are the
    unscaled conversion shifted."""
    flat, n_slots = base_tree(cr, "sbvh", "tess8", tess8)
    base = cr.CWBVH().convert_arrays(flat, n_slots)
    tree = scaled(flat, k)
    got = cr.CWBVH().convert_arrays(tree, n_slots)
    assert_same(got, R.convert(tree, n_slots), f"x 2^{k}")
    check_scaled_output(base, got, flat, k)
    check_tightness(got, tree)
    _validate_cwbvh(got, tree)


def _one_huge_leaf(factor):
    flat, n_slots = hand_tree("ones257")
    flat = flat.copy()
    leaf = int(np.nonzero(flat[:, 7] != 0)[0][5])
    flat[leaf, 4:7] = flat[leaf, 0:3] + f32(factor)
    return flat, n_slots


def test_cost_domain_has_a_named_refusal(cr):
    """§24: inside the root box every cost is below 12 * 3 * 2^24; a box 2^17 root extents wide still converts (257 * 3 * 2^34 < 1e20), one
    2^40 wide is refused by name, by the host and by the reference"""
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    flat, n_slots = _one_huge_leaf(2.0 ** 19)                                   # the root is 4 wide: 2^17 root extents
    assert_same(cr.CWBVH().convert_arrays(flat, n_slots), R.convert(flat, n_slots), "wide leaf")
    flat, n_slots = _one_huge_leaf(2.0 ** 42)
    with pytest.raises(CrtError) as e:
        cr.CWBVH().convert_arrays(flat, n_slots)
    assert e.value.code == CRT_ERR_INVALID and "cost range" in str(e.value)
    with pytest.raises(R.RefusedInput, match="cost range"):
        R.convert(flat, n_slots)


@pytest.mark.parametrize("flags", [0, 1])
def test_sbvh_build_ends_at_2_to_the_40(cr, tess8, flags):
    """Every SAH price of tess8 times 2^40 is at or above the builder's 1e20 'no split yet' value: no split was ever chosen, the node went
    whole to its right child and the build never ended.  Such a node is now split at the median of its widest axis."""
    mesh = tess8[0]
    v = np.ldexp(mesh.vertices, 40).astype(f32)
    s = cr.SBVH(mesh.triangles, v, flags)
    n = mesh.triangles.shape[0]
    assert s.flat_nodes.shape[0] == 2 * n - 1 and sorted(s.triangle_indices.tolist()) == list(range(n))
    lo, hi = B.triangle_boxes(mesh.triangles, v)
    B.check_tree(s.flat_nodes, s.triangle_indices, lo, hi)
    cw = cr.CWBVH().convert_arrays(s.flat_nodes, n)
    assert_same(cw, R.convert(s.flat_nodes, n), "tess8 x 2^40")
    check_tightness(cw, s.flat_nodes)


def test_sbvh_spatial_splits_end_on_coincident_triangles(cr, tess8):
    """No plane tells coincident references apart: a spatial split clipped every one of them into both children, again and again (3
    copies of one triangle: 220,989 references; 300: no end within a minute).  A node whose reference boxes are all equal now takes the
    object split.  Smallest first: were the doubling back, the 3-copy case fails in a second, before anything long starts."""
    for n in (3, 10, 300):
        t, v = TB.dups(n)
        s = cr.SBVH(t, v, 0)
        assert s.flat_nodes.shape[0] == 2 * n - 1 and sorted(s.triangle_indices.tolist()) == list(range(n)), n
        lo, hi = B.triangle_boxes(t, v)
        B.check_tree(s.flat_nodes, s.triangle_indices, lo, hi)
    # meshes whose references differ keep their spatial splits: tess8's tree still holds duplicates
    assert tess8[1].tri_orig_ids.shape[0] > tess8[0].triangles.shape[0]


# ---------------------------------------------------------------- refusals ----

def _not_breadth_first():
    """children after their parents, yet nodes 5 and 6 (depth 3) come before 7 and 8 (depth 2)"""
    flat = np.zeros((9, 8), f32)
    for i, l in ((0, 1), (1, 3), (2, 7), (3, 5)):
        flat[i, 3] = l
    for slot, i in enumerate((4, 5, 6, 7, 8)):
        flat[i, 0:3], flat[i, 4:7], flat[i, 3], flat[i, 7] = slot, slot + 1, slot, 1
    for i in (3, 2, 1, 0):
        l = int(flat[i, 3])
        flat[i, 0:3], flat[i, 4:7] = np.minimum(flat[l, 0:3], flat[l + 1, 0:3]), np.maximum(flat[l, 4:7], flat[l + 1, 4:7])
    return flat, 5


def _refusals():
    """name -> (flat, n_slots, words of the message)"""
    flat, n_slots = hand_tree("ones257")
    leaves = np.nonzero(flat[:, 7] != 0)[0]
    inner = np.nonzero(flat[:, 7] == 0)[0]
    out = {}

    def case(name, words, n=n_slots):
        f = flat.copy()
        out[name] = (f, n, words)
        return f
    case("leaf of 4 triangles", "more than 3 triangles")[leaves[3], 7] = 4
    case("leaf range past the slots", "outside the triangle array")[leaves[3], 3] = n_slots - 0
    case("negative leaf start", "outside the triangle array")[leaves[3], 3] = -1
    case("link backwards", "link out of order")[inner[9], 3] = 3
    case("link to itself", "link out of order")[inner[9], 3] = inner[9]
    case("link past the end", "link out of order")[inner[9], 3] = flat.shape[0] - 1
    case("NaN link", "link out of order")[inner[9], 3] = np.nan
    case("negative link", "link out of order")[inner[9], 3] = -5
    case("slot covered twice", "exactly once")[leaves[4], 3] = flat[leaves[5], 3]
    case("slot never covered", "exactly once", n_slots + 1)
    out["not breadth-first"] = _not_breadth_first() + ("link out of order",)
    return out


REFUSALS = ["leaf of 4 triangles", "leaf range past the slots", "negative leaf start", "link backwards", "link to itself", "link past the end",
            "NaN link", "negative link", "slot covered twice", "slot never covered"]


@pytest.mark.parametrize("name", REFUSALS)
def test_host_refuses_what_the_reference_refuses(cr, name):
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    flat, n_slots, words = _refusals()[name]
    with pytest.raises(R.RefusedInput, match=words):
        R.check_bvh2(flat, n_slots)
    with pytest.raises(CrtError) as e:
        cr.CWBVH().convert_arrays(flat, n_slots)
    assert e.value.code == CRT_ERR_INVALID and words in str(e.value), str(e.value)


def test_host_accepts_children_after_parents_in_any_order(cr):
    """The device converter works level by level and refuses (as the reference does) an array that is not breadth-first; the host
    converter sweeps the array backwards and needs only that children follow their parents (test helpers number TLAS trees that way):
    its output for such an array is that of the same tree renumbered breadth-first, node for node."""
    flat, n_slots = _not_breadth_first()
    with pytest.raises(R.RefusedInput, match="link out of order"):
        R.check_bvh2(flat, n_slots)
    order = [0, 1, 2, 3, 4, 7, 8, 5, 6]                                         # breadth-first positions -> positions in `flat`
    bfs = flat[order].copy()
    for p in np.nonzero(bfs[:, 7] == 0)[0]:
        bfs[p, 3] = order.index(int(bfs[p, 3]))
    got, want = cr.CWBVH().convert_arrays(flat, n_slots), R.convert(bfs, n_slots)
    assert np.array_equal(got.nodes, want.nodes) and np.array_equal(got.tri_slots, want.tri_slots)
    assert np.array_equal(np.where(got.child_bvh2 >= 0, np.asarray(order)[np.maximum(want.child_bvh2, 0)], -1), got.child_bvh2)


def test_host_accepts_a_chain_deeper_than_the_device_limits(cr):
    """The host converter has no depth limit of its own (the walk refuses at its stack limit when a scene is created): a one-sided BVH2 of
    depth 455 becomes 65 node8 levels, one more than crt_cwbvh_convert_device accepts (CRT_ERR_LIMIT, tested on the GPU)."""
    flat, n_slots = chain(455, "right")
    cw = cr.CWBVH().convert_arrays(flat, n_slots)
    assert cw.depth == 65 == R.convert(flat, n_slots).depth


# ---------------------------------------------------------------- refit on the host ----

def _soup_mesh(cr, cornell, t, vertices):
    """the soup as a scene's mesh: material 0 and geometric normals on every triangle, the Cornell box's materials and lights"""
    base = cornell[0]
    return cr.Mesh(vertices.reshape(-1, 3), np.zeros((1, 3), f32), np.zeros((0, 2), f32), t, base.materials, base.lights)


def _poses(n=1300):
    """vertex sets of one soup: as generated, squeezed (half of it into a small cube) and stretched along x"""
    t, v = TB.soup(n)
    v = v.reshape(-1, 3)
    squeezed = v.copy()
    squeezed[: v.shape[0] // 2] = (f32(2.0) + f32(0.01) * (v[: v.shape[0] // 2] - f32(2.0))).astype(f32)
    stretched = (v * f32([7.0, 1.0, 0.25])).astype(f32)
    return t, v, squeezed, stretched


def _placed(v, where):
    return np.ldexp(v, 20).astype(f32) if where == "x 2^20" else (v + f32(1e3)).astype(f32) if where == "+ 1e3" else v


@pytest.mark.parametrize("where", ["as built", "x 2^20", "+ 1e3"])
def test_host_refit_equals_the_refit_reference(cr, where):
    t, v, squeezed, stretched = _poses()
    s = cr.SBVH(t, _placed(v, where), 1)
    cw = cr.CWBVH().convert(s)
    for pose in (squeezed, stretched):
        V = _placed(pose, where)
        got = _cwbvh_refit(cr, cw.nodes, cw.tri_slots, s.triangles, V)
        want = R.refit(cw.nodes, cw.tri_slots, s.triangles, V)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        assert _check_cwbvh_boxes(got, cw.tri_slots, s.triangles, V) > 1300
    same = R.refit(cw.nodes, cw.tri_slots, s.triangles, _placed(v, where))     # the SAH-only tree's boxes are exact unions: a fixed point
    assert np.array_equal(same, cw.nodes)


# ---------------------------------------------------------------- GPU ----

def _n8_of(builder, t, V):
    flat, order = {"lbvh": B.ref_lbvh, "ploc": B.ref_ploc, "sah": B.ref_sah}[builder](t, V)
    return R.convert(flat, order.shape[0]).nodes.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CORPUS)
def test_device_converter_equals_the_reference(cr, tess8, name):
    """nodes, tri_slots, child_bvh2 and depth, byte for byte, on every variant; a second call gives the same bytes"""
    flat, n_slots = corpus_member(cr, name, tess8)
    for variant, tree in variants(flat).items():
        got = cr.CWBVH().convert_arrays(tree, n_slots, device=True)
        assert_same(got, ref_convert(name, variant, tree, n_slots), f"{name} {variant}")
        assert_same(cr.CWBVH().convert_arrays(tree, n_slots, device=True), got, f"{name} {variant}, second call")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [30, 40, -70])
def test_device_converter_beyond_the_old_sentinel(cr, tess8, k):
    flat, n_slots = base_tree(cr, "sbvh", "tess8", tess8)
    tree = scaled(flat, k)
    assert_same(cr.CWBVH().convert_arrays(tree, n_slots, device=True), R.convert(tree, n_slots), f"x 2^{k}")


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["as built", "x 2^20", "+ 1e3"])
@pytest.mark.parametrize("builder", ["lbvh", "ploc", "sah"])
def test_device_built_and_rebuilt_scenes_hold_the_references_nodes(cr, cornell, builder, where):
    """A scene created on the device, rebuilt once to fewer and once to more node8s than the tree before it: each time the node8 array
    the scene holds is the reference's conversion of the BVH2 the scene holds.  (A flat scene's rebuild allocates its node array anew;
    the reuse of a caller's buffer, into_cap, is the instanced scene's TLAS path.)"""
    t, v, squeezed, stretched = _poses()
    poses = sorted((v, squeezed, stretched), key=lambda p: _n8_of(builder, t, _placed(p, where)))
    counts = [_n8_of(builder, t, _placed(p, where)) for p in poses]
    assert counts[0] < counts[1] < counts[2], counts
    mesh = _soup_mesh(cr, cornell, t, _placed(poses[1], where))
    sc = cr.Scene(cr.SceneData.for_device_build(mesh, cornell[1], builder), 32, 24, 1)
    for step, pose in enumerate((poses[1], poses[0], poses[2])):
        if step:
            sc.rebuild_vertices(_placed(pose, where))
        nodes, flat = sc.debug_read_accel(0), sc.debug_read_accel(2)
        want = R.convert(flat, t.shape[0])
        assert nodes.shape[0] == counts[(1, 0, 2)[step]], (step, nodes.shape, counts)
        assert np.array_equal(nodes, want.nodes), (step, np.argwhere(nodes != want.nodes)[:4])
        tri_slots = sc.debug_read_accel(1)[:, 7].copy().view(np.int32)
        assert np.array_equal(tri_slots, want.tri_slots)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["x 2^20", "+ 1e3"])
def test_device_refit_equals_the_refit_reference(cr, cornell, where):
    t, v, squeezed, stretched = _poses()
    mesh = _soup_mesh(cr, cornell, t, _placed(v, where))
    data = cr.SceneData.for_device_build(mesh, cornell[1], "sah")
    sc = cr.Scene(data, 32, 24, 1)
    a0 = _accel(sc)
    leaf_tris, ids, tri_slots = _host_side(cr, data, mesh, a0)
    V = _placed(stretched, where)
    sc.update_vertices(V)
    nodes = sc.debug_read_accel(0)
    want = R.refit(a0[0], tri_slots, leaf_tris, V)
    assert np.array_equal(nodes, want), np.argwhere(nodes != want)[:4]
    assert _check_cwbvh_boxes(nodes, tri_slots, leaf_tris, V) > 1300
    sc.close()


@pytest.mark.gpu
def test_tlas_converted_into_its_staging_buffer_equals_the_reference(cr):
    """The converter's other output path: an instanced scene's TLAS is converted INTO a buffer the handle owns (d_nodes_into), sized at
    create for `capacity` instances, which bounds the node8 count (a CWBVH over c leaves has at most max(1, c - 1) node8s): the branch
    that allocates instead cannot be reached from there.  Create, a set of fewer and a set of more instances each give the reference's
    conversion of the reference SAH tree over the world boxes the scene reports, and records in its leaf order."""
    rng = np.random.default_rng(77)
    meshes = [(TB.soup(40, 5)[1], TB.soup(40, 5)[0]), (TB.soup(70, 6)[1], TB.soup(70, 6)[0])]
    sc = cr.InstancedScene(meshes, cr.instances_array(TB._rigid(rng, 300, 20.0), rng.integers(0, 2, 300)), capacity=700)
    try:
        sizes = []
        for n in (300, 65, 1, 700):
            if sizes:
                sc.set(cr.instances_array(TB._rigid(rng, n, 3.0 * n ** (1 / 3)), rng.integers(0, 2, n)))
            boxes = sc.world_boxes()
            flat, order = B.ref_sah_boxes(boxes, 0)
            want = R.convert(flat, n)
            tlas = sc.tlas_nodes()
            assert tlas.shape == want.nodes.shape and np.array_equal(tlas, want.nodes), (n, tlas.shape, want.nodes.shape)
            rec = sc.instance_records()
            assert np.array_equal(rec[:, 12:].copy().view(np.uint32)[:, 1], order[want.tri_slots].astype(np.uint32)), n
            sizes.append(tlas.shape[0])
        assert sizes[1] < sizes[0] < sizes[3] and sizes[2] == 1, sizes
    finally:
        sc.close()


_walk = {}


def _walk_inputs(cr, ob, cornell, tess8):
    """tess8, 20 000 seeded rays and the oracle's BVH8 walk of them, unscaled: shared by the CPU confirmation and the GPU case"""
    if not _walk:
        from conftest import seeded_rays
        mesh, data = tess8
        rays = seeded_rays(mesh, 20000, 7, cr.RAY_DT)
        orc = ob.Oracle(data, 32, 24, 1, cornell[1])
        _walk["rays"] = rays
        _walk["closest"] = orc.trace(rays, ob.BVH8, ob.CLOSEST, ob.TIE_LOWEST_ID, stats=True, threads=8)
    return _walk["rays"], _walk["closest"]


def _scaled_scene_data(cr, cornell, tess8, k):
    mesh, data = tess8
    v = np.ldexp(mesh.vertices, k).astype(f32)
    m = cr.Mesh(v, mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials, mesh.lights, mesh.vertex_min)
    s = cr.SBVH.__new__(cr.SBVH)
    s.flat_nodes, s.triangle_indices, s.triangles = scaled(data.bvh, k), data.tri_orig_ids, data.triangles
    return cr.SceneData(m, s, cr.CWBVH().convert(s), cornell[1])


def _scaled_rays(rays, k):
    out = rays.copy()
    out["o"] = np.ldexp(rays["o"], k)
    out["tmax"] = np.ldexp(rays["tmax"], k)
    return out


def _same_walk(got, st, want, st_want, k):
    assert np.array_equal(got["tri"], want["tri"]) and (want["tri"] >= 0).mean() > 0.5
    for key in ("u", "v"):
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
    hit = want["tri"] >= 0
    assert np.array_equal(got["t"][hit].view(np.uint32), np.ldexp(want["t"][hit], k).astype(f32).view(np.uint32))
    assert np.array_equal(st["nodes"], st_want["nodes"]) and np.array_equal(st["tris"], st_want["tris"])


@pytest.mark.parametrize("k", [20, -20])
def test_oracle_walk_is_scale_invariant_on_the_chosen_rays(cr, ob, cornell, tess8, k):
    """The expectation the GPU case below relies on, confirmed without a GPU: the CPU oracle's BVH8 walk of tess8 times 2^k, rays scaled
    alike, gives the unscaled tri, u, v and counters, and t times 2^k bit for bit"""
    rays, (want, st_want) = _walk_inputs(cr, ob, cornell, tess8)
    orc = ob.Oracle(_scaled_scene_data(cr, cornell, tess8, k), 32, 24, 1, cornell[1])
    got, st = orc.trace(_scaled_rays(rays, k), ob.BVH8, ob.CLOSEST, ob.TIE_LOWEST_ID, stats=True, threads=8)
    _same_walk(got, st, want, st_want, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [20, -20])
def test_device_walk_is_scale_invariant(cr, ob, cornell, tess8, k):
    from caitlynrenderer_amd._lib import CRT_TRACE_ANY, CRT_TRACE_CLOSEST
    rays, _ = _walk_inputs(cr, ob, cornell, tess8)
    base = cr.Scene(tess8[1], 32, 24, 1)
    sc = cr.Scene(_scaled_scene_data(cr, cornell, tess8, k), 32, 24, 1)
    want, st_want = base.trace(rays, CRT_TRACE_CLOSEST, stats=True)
    got, st = sc.trace(_scaled_rays(rays, k), CRT_TRACE_CLOSEST, stats=True)
    _same_walk(got, st, want, st_want, k)
    want, st_want = base.trace(rays, CRT_TRACE_ANY, stats=True)
    got, st = sc.trace(_scaled_rays(rays, k), CRT_TRACE_ANY, stats=True)
    assert np.array_equal(got["tri"], want["tri"])
    assert np.array_equal(st["nodes"], st_want["nodes"]) and np.array_equal(st["tris"], st_want["tris"])
    base.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", REFUSALS + ["not breadth-first", "cost range"])
def test_device_refuses_what_the_reference_refuses(cr, name):
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    if name == "cost range":
        flat, n_slots = _one_huge_leaf(2.0 ** 42)
        words = "cost range"
    else:
        flat, n_slots, words = _refusals()[name]
    with pytest.raises(CrtError) as e:
        cr.CWBVH().convert_arrays(flat, n_slots, device=True)
    assert e.value.code == CRT_ERR_INVALID and words in str(e.value), str(e.value)


@pytest.mark.gpu
def test_device_refuses_the_65_level_chain_with_a_limit_error(cr):
    from caitlynrenderer_amd._lib import CRT_ERR_LIMIT, CrtError
    flat, n_slots = chain(455, "right")
    with pytest.raises(CrtError) as e:
        cr.CWBVH().convert_arrays(flat, n_slots, device=True)
    assert e.value.code == CRT_ERR_LIMIT and "64 levels" in str(e.value)
    flat, n_slots = chain(448, "right")                                         # 64 levels: accepted, and the reference's bytes
    assert_same(cr.CWBVH().convert_arrays(flat, n_slots, device=True), R.convert(flat, n_slots), "64-level chain")
