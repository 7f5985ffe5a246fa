"""Plain numpy definition of the BVH2 -> CWBVH conversion (crt_cwbvh_convert / crt_cwbvh_convert_device) and of the CWBVH refit
(crt_cwbvh_refit / crt_update_vertices), written from DESIGN.md §24 and SURVEY.md appendix C, not from host/cwbvh_core.hpp.

convert(flat, n_slots) takes a breadth-first (n, 8) float32 BVH2 (cr.SBVH(...).flat_nodes: lo xyz, link, hi xyz, leaf count) and returns
Converted(nodes (n8, 80) uint8, tri_slots (n_slots,) int32, child_bvh2 (n8, 8) int32, depth).  check_bvh2 raises RefusedInput for what the
converters refuse.  refit(nodes, tri_slots, leaf_triangles, vertices) returns the re-quantised nodes.

What decides a byte and rounds is computed in np.float32, one rounding per operation, in the order §24 fixes: the half-areas, the cost
sums, the box centres and the octant dot products.  What §24 defines WITHOUT rounding — the exponent and the quantised planes — is found
here by exact comparison over every candidate value (float64 with an error-free sum), not by the converters' float formula."""
from collections import namedtuple

import numpy as np

f32 = np.float32
LEAF, INTERNAL, DISTRIBUTE = 0, 1, 2
E_FLOOR = 20                       # 2^(20-127) is the smallest scale: what an extent of 1e-30 / 255 or less asks for (§24)
COST_LIMIT = f32(1.0e20)           # a (scaled) cost at or above this is refused (§24 "cost domain")
Converted = namedtuple("Converted", "nodes tri_slots child_bvh2 depth")


class RefusedInput(ValueError):
    pass


# ---------------------------------------------------------------- exact comparisons ----

def sign_of_sum_minus(p, t, c):
    """sign(p + t - c) for float64 arrays, exactly: s + err == p + t without rounding (Knuth's two-sum), s - c is exact when the two are
    within a factor of two of each other and dominates err otherwise, and a rounded sum keeps the sign of the exact one."""
    p, t, c = np.broadcast_arrays(np.asarray(p, np.float64), np.asarray(t, np.float64), np.asarray(c, np.float64))
    s = p + t
    bb = s - p
    err = (p - (s - bb)) + (t - bb)
    return np.sign((s - c) + err)


def scale_of(e):
    """2^(e - 127) as float64 for exponent bytes 1..254"""
    return np.ldexp(1.0, np.asarray(e, np.int64) - 127)


def pick_exponents(lo, hi):
    """The smallest e in 1..254 with lo + 255 * 2^(e-127) >= hi (254 if none), and never below E_FLOOR.  lo, hi: (...,) float32."""
    lo64, hi64 = np.asarray(lo, np.float64)[..., None], np.asarray(hi, np.float64)[..., None]
    cand = np.arange(1, 255)
    reaches = sign_of_sum_minus(lo64, 255.0 * scale_of(cand), hi64) >= 0          # monotone in e
    e = np.where(reaches.any(-1), 1 + np.argmax(reaches, -1), 254)
    return np.maximum(e, E_FLOOR).astype(np.uint8)


def quantise(p, e, c_lo, c_hi):
    """q_lo = the largest q in 0..255 with p + q * 2^(e-127) <= c_lo (0 if none); q_hi = the smallest with >= c_hi (255 if none)"""
    q = np.arange(256, dtype=np.float64)
    grid = q * scale_of(e)[..., None]
    p64 = np.asarray(p, np.float64)[..., None]
    below = sign_of_sum_minus(p64, grid, np.asarray(c_lo, np.float64)[..., None]) <= 0      # true for q = 0..q_lo
    above = sign_of_sum_minus(p64, grid, np.asarray(c_hi, np.float64)[..., None]) >= 0      # true for q = q_hi..255
    q_lo = np.maximum(below.sum(-1) - 1, 0)
    q_hi = np.where(above.any(-1), np.argmax(above, -1), 255)
    return q_lo.astype(np.uint8), q_hi.astype(np.uint8)


# ---------------------------------------------------------------- the BVH2 ----

def links(flat):
    """column 3 as integers (a link below 2^24 is stored as the float of its value)"""
    w = np.asarray(flat, f32)[:, 3]
    ok = np.isfinite(w) & (w >= 0) & (w < 2.0 ** 24) & (w == np.floor(w))
    return np.where(ok, w, -1).astype(np.int64)


def check_bvh2(flat, n_slots):
    """Raises RefusedInput for what both converters refuse (CRT_ERR_INVALID), with the message they give.  Returns (is_leaf, link, count)."""
    flat = np.asarray(flat, f32).reshape(-1, 8)
    n = flat.shape[0]
    if n == 0:
        raise RefusedInput("empty BVH2")
    leaf = flat[:, 7] != 0
    link = links(flat)
    count = np.where(leaf, np.nan_to_num(flat[:, 7], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), 0)
    inner = np.nonzero(~leaf)[0]
    if ((link[inner] <= inner) | (link[inner] + 1 >= n)).any():                # a NaN, negative or fractional link reads as -1
        raise RefusedInput("BVH2 child link out of order")
    parent = np.full(n, -1, np.int64)
    parent[link[inner]] = inner
    parent[link[inner] + 1] = inner
    depth = np.zeros(n, np.int64)
    for i in range(1, n):                                                       # parents come first
        depth[i] = depth[parent[i]] + 1 if parent[i] >= 0 else 0
    claimed = np.concatenate([link[inner], link[inner] + 1])
    if (np.diff(depth) < 0).any() or np.unique(claimed).shape[0] != claimed.shape[0]:
        raise RefusedInput("BVH2 child link out of order")                     # not breadth-first, or a node with two parents
    if ((count[leaf] < 1) | (count[leaf] > 3)).any():
        raise RefusedInput("BVH2 leaf with more than 3 triangles cannot be encoded")
    if ((link[leaf] < 0) | (link[leaf] + count[leaf] > n_slots)).any():
        raise RefusedInput("BVH2 leaf range outside the triangle array")
    reached = np.zeros(n, bool)
    reached[0] = True
    for i in inner:
        if reached[i]:
            reached[link[i]] = reached[link[i] + 1] = True
    seen = np.zeros(n_slots, np.int64)
    for i in np.nonzero(leaf & reached)[0]:
        seen[link[i]:link[i] + count[i]] += 1
    if (seen != 1).any():
        raise RefusedInput("BVH2 leaves do not cover the triangle array exactly once")
    return leaf, link, count


def area_scale(flat):
    """The power of two every extent is multiplied by before the areas are formed: 2^-floor(log2(largest extent of the root box)),
    exponent clamped to the normal range, so that the root's half-area lies in [1, 12) at any scale of the scene (§24)"""
    ext = (flat[0, 4:7] - flat[0, 0:3]).astype(f32)
    biased = int(np.clip((np.float32(ext.max()).view(np.uint32) >> 23) & 0xff, 1, 253))
    return f32(np.ldexp(1.0, 127 - biased))


def half_areas(flat, a):
    """dx * (dy + dz) + dy * dz of the extents times a, every operation rounded to float32"""
    d = ((flat[:, 4:7] - flat[:, 0:3]).astype(f32) * a).astype(f32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return ((dx * (dy + dz).astype(f32)).astype(f32) + (dy * dz).astype(f32)).astype(f32)


def _levels(leaf, link):
    """breadth-first node ranges of equal depth: [(begin, end), ...]"""
    n = leaf.shape[0]
    out, begin, end = [], 0, 1
    while begin < n:
        out.append((begin, end))
        inner = np.nonzero(~leaf[begin:end])[0] + begin
        begin, end = end, (int(link[inner].max()) + 2 if inner.size else end)
    return out


def cost_tables(flat, leaf, link, count):
    """T[node, i] for i = 0..6: the cheapest way to stand for the node's subtree with at most i + 1 slots of one node8 (§24).
    -> cost (n, 7) float32, kind (n, 7), dl, dr (n, 7) (the rows of the left / right child a decision refers to), nprims (n,)"""
    n = flat.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        area = half_areas(flat, area_scale(flat))
        cost = np.zeros((n, 7), f32)
        kind = np.zeros((n, 7), np.int8)
        dl, dr = np.full((n, 7), -1, np.int8), np.full((n, 7), -1, np.int8)
        nprims = count.copy()
        rows = np.arange(7)
        for begin, end in reversed(_levels(leaf, link)):
            idx = np.arange(begin, end)
            lf = idx[leaf[idx]]
            cost[lf] = (area[lf] * count[lf].astype(f32)).astype(f32)[:, None]
            kind[lf] = LEAF
            nd = idx[~leaf[idx]]
            if not nd.size:
                continue
            L, R = link[nd], link[nd] + 1
            nprims[nd] = nprims[L] + nprims[R]
            # i = 0: a node8 of its own (INTERNAL) over the best split of 8 slots between the two children, or a leaf slot
            sums = (cost[L][:, rows] + cost[R][:, 6 - rows]).astype(f32)
            k = np.argmin(sums, 1)                                              # the first minimum
            internal = (sums[np.arange(nd.size), k] + area[nd]).astype(f32)
            as_leaf = (nprims[nd].astype(f32) * area[nd]).astype(f32)
            take_leaf = (nprims[nd] <= 3) & (as_leaf < internal)
            cost[nd, 0] = np.where(take_leaf, as_leaf, internal)
            kind[nd, 0] = np.where(take_leaf, LEAF, INTERNAL)
            dl[nd, 0], dr[nd, 0] = k, 6 - k
            # i >= 1: hand i + 1 slots to the children (DISTRIBUTE) where that is strictly cheaper than what i slots achieve
            for i in range(1, 7):
                ks = np.arange(i)
                sums = (cost[L][:, ks] + cost[R][:, i - 1 - ks]).astype(f32)
                k = np.argmin(sums, 1)
                best = sums[np.arange(nd.size), k]
                better = best < cost[nd, i - 1]
                cost[nd, i] = np.where(better, best, cost[nd, i - 1])
                kind[nd, i] = np.where(better, DISTRIBUTE, kind[nd, i - 1])
                dl[nd, i] = np.where(better, k, dl[nd, i - 1])
                dr[nd, i] = np.where(better, i - 1 - k, dr[nd, i - 1])
    if not (cost[:, 0] < COST_LIMIT).all():
        raise RefusedInput("BVH2 boxes out of the cost range: a summed cost is not below 1e20 times the root's scale")
    return cost, kind, dl, dr, nprims


def child_set(node, leaf, link, kind, dl, dr):
    """The BVH2 nodes that become the slots of the node8 standing for `node`, left subtree first"""
    if leaf[node]:
        return [node]
    out, todo = [], [(node, 0, True)]
    while todo:
        n, i, expand = todo.pop()
        if not expand:
            out.append(n)
            continue
        l, r = link[n], link[n] + 1
        jl, jr = dl[n, i], dr[n, i]
        todo.append((r, jr, kind[r, jr] == DISTRIBUTE))
        todo.append((l, jl, kind[l, jl] == DISTRIBUTE))
    return out


def octant_slots(centre, child_centres):
    """Greedy assignment of children to the 8 slots.  Slot s looks along d(s) = (-1 if s & 4 else +1, -1 if s & 2 else +1, -1 if s & 1
    else +1); the cost of child c in slot s is dot(centre_c - centre, d(s)) = (x + y) + z in float32.  Repeatedly the (child, slot) pair
    of least cost among unplaced children and free slots is fixed; of equal costs the first in the scan child-major, slot-minor."""
    r = (np.asarray(child_centres, f32) - np.asarray(centre, f32)).astype(f32)
    s = np.arange(8)
    d = np.stack([np.where(s & 4, -1, 1), np.where(s & 2, -1, 1), np.where(s & 1, -1, 1)], 1).astype(f32)
    cost = (((r[:, None, 0] * d[None, :, 0]) + (r[:, None, 1] * d[None, :, 1])).astype(f32) + (r[:, None, 2] * d[None, :, 2])).astype(f32)
    cost = cost.astype(np.float64)
    slot_of = [-1] * r.shape[0]
    for _ in range(r.shape[0]):
        c, sl = divmod(int(np.argmin(cost)), 8)
        slot_of[c] = sl
        cost[c, :] = np.inf
        cost[:, sl] = np.inf
    return slot_of


def subtree_slots(node, leaf, link, count):
    if leaf[node]:
        return list(range(link[node], link[node] + count[node]))
    return subtree_slots(link[node], leaf, link, count) + subtree_slots(link[node] + 1, leaf, link, count)


def convert(flat, n_slots):
    flat = np.ascontiguousarray(flat, f32).reshape(-1, 8)
    leaf, link, count = check_bvh2(flat, n_slots)
    cost, kind, dl, dr, nprims = cost_tables(flat, leaf, link, count)
    centres = ((flat[:, 0:3] + flat[:, 4:7]).astype(f32) * f32(0.5)).astype(f32)

    # topology: depth-first, a node's inner children numbered consecutively when the node is visited, its triangles appended then too
    bvh2_of, child_bvh2, child_base, tri_base, level = [0], [None], [0], [0], [1]
    tri_slots = []
    todo = [0]
    while todo:
        i = todo.pop()
        node = bvh2_of[i]
        if i == 0 and kind[0, 0] == LEAF:
            kids = [0]                                                          # a root of at most 3 triangles: one leaf slot
        else:
            kids = child_set(node, leaf, link, kind, dl, dr)
        slots = [-1] * 8
        for c, s in zip(kids, octant_slots(centres[node], centres[kids])):
            slots[s] = c
        child_bvh2[i] = slots
        tri_base[i], child_base[i] = len(tri_slots), len(bvh2_of)
        inner = []
        for s in range(8):
            c = slots[s]
            if c < 0:
                continue
            if kind[c, 0] == LEAF:
                tri_slots += subtree_slots(c, leaf, link, count)
            else:
                inner.append(c)
        for c in inner:
            bvh2_of.append(c); child_bvh2.append(None); child_base.append(0); tri_base.append(0); level.append(level[i] + 1)
        todo += list(range(len(bvh2_of) - 1, len(bvh2_of) - 1 - len(inner), -1))    # the first inner child is visited next

    n8 = len(bvh2_of)
    bvh2_of, child_bvh2 = np.asarray(bvh2_of), np.asarray(child_bvh2, np.int64).reshape(n8, 8)
    occupied = child_bvh2 >= 0
    kid = np.where(occupied, child_bvh2, 0)
    is_leaf_slot = occupied & (kind[kid, 0] == LEAF)
    cnt = np.where(is_leaf_slot, nprims[kid], 0)
    offset = np.cumsum(cnt, 1) - cnt
    meta = np.where(is_leaf_slot, (((1 << cnt) - 1) << 5) | offset, np.where(occupied, (np.arange(8) + 24) | 0x20, 0))
    imask = ((occupied & ~is_leaf_slot) << np.arange(8)).sum(1)
    nodes = encode(flat[bvh2_of, 0:3], flat[bvh2_of, 4:7], flat[kid, 0:3], flat[kid, 4:7], occupied, meta, imask,
                   np.asarray(child_base), np.asarray(tri_base))
    return Converted(nodes, np.asarray(tri_slots, np.int32), child_bvh2.astype(np.int32), max(level))


def encode(lo, hi, c_lo, c_hi, occupied, meta, imask, child_base, tri_base):
    """80-byte nodes from the node boxes lo / hi (n8, 3), the slot boxes c_lo / c_hi (n8, 8, 3) and the topology bytes: the origin is lo,
    the exponents reach hi, the planes of an occupied slot are the tightest that contain the slot box inside the node's frame"""
    n8 = lo.shape[0]
    nodes = np.zeros((n8, 80), np.uint8)
    nodes[:, 0:12] = np.ascontiguousarray(lo, f32).view(np.uint8).reshape(n8, 12)
    e = pick_exponents(lo, hi)
    nodes[:, 12:15] = e
    nodes[:, 15] = imask
    nodes[:, 16:20] = np.ascontiguousarray(child_base, np.uint32).view(np.uint8).reshape(n8, 4)
    nodes[:, 20:24] = np.ascontiguousarray(tri_base, np.uint32).view(np.uint8).reshape(n8, 4)
    nodes[:, 24:32] = meta
    q_lo, q_hi = quantise(np.asarray(lo, f32)[:, None, :], e[:, None, :], c_lo, c_hi)                  # (n8, 8 slots, 3 axes)
    q = np.stack([q_lo, q_hi], 1) * occupied[:, None, :, None]                                       # (n8, lo/hi, slot, axis)
    nodes[:, 32:80] = q.transpose(0, 3, 1, 2).reshape(n8, 48)                                         # axis, lo/hi, slot
    return nodes


# ---------------------------------------------------------------- refit ----

def fields(nodes):
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 80)
    return {"p": nodes[:, 0:12].copy().view(f32), "e": nodes[:, 12:15], "imask": nodes[:, 15].astype(np.int64),
            "child_base": nodes[:, 16:20].copy().view(np.uint32)[:, 0].astype(np.int64),
            "tri_base": nodes[:, 20:24].copy().view(np.uint32)[:, 0].astype(np.int64), "meta": nodes[:, 24:32].astype(np.int64),
            "q": nodes[:, 32:80].reshape(-1, 3, 2, 8)}


def inner_child(f, i, s):
    return int(f["child_base"][i]) + bin(int(f["imask"][i]) & ((1 << s) - 1)).count("1")


def refit(nodes, tri_slots, leaf_triangles, vertices):
    """Topology, meta, imask and both bases stay; a leaf slot's box is the box of its triangles' new vertices, an inner slot's the union
    of its child node8's slots; origin, exponents and planes follow from those boxes as in convert.  Negative zeros are refused (the
    converters order -0 below +0, numpy's minimum does not)."""
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 80)
    V = np.asarray(vertices, f32).reshape(-1, 3)
    if not np.isfinite(V).all() or (np.signbit(V) & (V == 0)).any():
        raise RefusedInput("a vertex is not finite or a negative zero")
    tri = np.asarray(leaf_triangles)[:, :3].astype(np.int64)
    f = fields(nodes)
    n8 = nodes.shape[0]
    order, k = [0], 0
    while k < len(order):
        i = order[k]; k += 1
        order += [inner_child(f, i, s) for s in range(8) if (f["imask"][i] >> s) & 1]
    assert len(order) == n8
    c_lo, c_hi = np.full((n8, 8, 3), np.inf, f32), np.full((n8, 8, 3), -np.inf, f32)
    for i in reversed(order):
        for s in range(8):
            m = int(f["meta"][i, s])
            if m == 0:
                continue
            if (f["imask"][i] >> s) & 1:
                c = inner_child(f, i, s)
                c_lo[i, s], c_hi[i, s] = c_lo[c].min(0), c_hi[c].max(0)
            else:
                first = int(f["tri_base"][i]) + (m & 31)
                pts = V[tri[np.asarray(tri_slots)[first:first + bin(m >> 5).count("1")]].ravel()]
                c_lo[i, s], c_hi[i, s] = pts.min(0), pts.max(0)
    occupied = f["meta"] != 0
    lo, hi = c_lo.min(1), c_hi.max(1)
    return encode(lo, hi, np.where(occupied[:, :, None], c_lo, 0), np.where(occupied[:, :, None], c_hi, 0), occupied, f["meta"], f["imask"],
                  f["child_base"], f["tri_base"])
