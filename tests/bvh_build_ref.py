"""Plain numpy references of the three GPU BVH builders (caitlynrenderer_amd/csrc/lbvh.hip), written from the algorithms' definitions
(DESIGN.md §21), not from the kernels: ref_lbvh (Morton codes + the recursive radix-tree split), ref_ploc (locally-ordered clustering
with a search radius), ref_sah / ref_sah_boxes (binned SAH above a small-node threshold, the exact sweep below it).

Every function returns (flat_nodes (2n-1, 8) float32, triangle_indices (n,) int32) in the layout of cr.SBVH(...).flat_nodes /
.triangle_indices: breadth-first numbering as a queue gives it (root 0, left child before right, children adjacent), the link in
column 3, column 7 = 0 for an interior node and 1 for a leaf, a leaf's link = its slot, triangle_indices[slot] = its triangle, interior
boxes = the union of their children.  Everything that decides anything is computed in np.float32, one rounding per operation.

The references REFUSE (RefusedInput) what C++ leaves undefined or where two correct implementations may differ: a non-finite or
over-range coordinate, a negative zero (fminf / fmaxf may return either zero), a nonzero centroid extent below 2^-100, a quotient that is
not finite before the float -> int conversion, a split cost at or above the builders' "no split" sentinel."""
import bisect
from collections import deque

import numpy as np

f32 = np.float32
MAX_COORD = f32(1.0e18)
MIN_EXTENT = f32(2.0 ** -100)
NO_SPLIT = f32(3.0e38)
PLOC_SINGLE_WORKGROUP = 1024          # at this many clusters or fewer an iteration without a mutual pair merges positions 0 and 1


class RefusedInput(ValueError):
    pass


class PlocNoProgress(RuntimeError):
    """an iteration over more than 1,024 clusters merged nothing (the device returns CRT_ERR_INVALID)"""


# ---------------------------------------------------------------- shared ----

def _check_boxes(lo, hi):
    for a in (lo, hi):
        if not np.isfinite(a).all() or (np.abs(a) > MAX_COORD).any():
            raise RefusedInput("a coordinate is not finite or exceeds 1e18")
        if (np.signbit(a) & (a == 0)).any():
            raise RefusedInput("a coordinate is a negative zero")


def triangle_boxes(triangles, vertices):
    """(lo, hi), each (n, 3) float32: the min / max of every triangle's three vertices"""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    t = np.asarray(triangles)[:, :3].astype(np.int64)
    p = v[t]                                                        # (n, 3 vertices, 3 axes)
    lo, hi = p.min(1), p.max(1)
    _check_boxes(lo, hi)
    return lo, hi


def _centroids(lo, hi):
    return (f32(0.5) * (lo + hi).astype(f32)).astype(f32)


def _half_area(lo, hi):
    """dx*dy + dy*dz + dz*dx in fp32, left to right; lo, hi: (..., 3)"""
    d = (hi - lo).astype(f32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (((dx * dy).astype(f32) + (dy * dz).astype(f32)).astype(f32) + (dz * dx).astype(f32)).astype(f32)


def _extent(cmin, cmax):
    ext = (cmax - cmin).astype(f32)
    if ((ext > 0) & (ext < MIN_EXTENT)).any():
        raise RefusedInput("a nonzero centroid extent below 2^-100")
    return ext


def _emit(root, left, right, slot, order, lo, hi):
    """Breadth-first numbering by a queue, then the boxes bottom-up.  left / right: child ids (-1: leaf), slot: a leaf's slot;
    order[slot] = the triangle in it; lo / hi: the triangles' boxes."""
    n = len(order)
    flat = np.zeros((2 * n - 1, 8), f32)
    ids = []
    queue = deque([root])
    while queue:
        k = queue.popleft()
        ids.append(k)
        if left[k] >= 0:
            queue.append(left[k]); queue.append(right[k])
    assert len(ids) == 2 * n - 1
    nxt = 1
    for p, k in enumerate(ids):
        if left[k] >= 0:
            flat[p, 3] = nxt                                        # the queue hands out positions in the order it was filled
            nxt += 2
        else:
            t = order[slot[k]]
            flat[p, 0:3], flat[p, 4:7], flat[p, 3], flat[p, 7] = lo[t], hi[t], slot[k], 1
    for p in range(2 * n - 2, -1, -1):
        if flat[p, 7] == 0:
            l = int(flat[p, 3])
            flat[p, 0:3] = np.minimum(flat[l, 0:3], flat[l + 1, 0:3])
            flat[p, 4:7] = np.maximum(flat[l, 4:7], flat[l + 1, 4:7])
    return flat, np.asarray(order, np.int32)


# ---------------------------------------------------------------- Morton order, LBVH ----

def morton_codes(lo, hi):
    """30-bit codes of the centroids inside the centroid bounds, x in the highest position of every bit triple"""
    cen = _centroids(lo, hi)
    cmin, cmax = cen.min(0), cen.max(0)
    ext = _extent(cmin, cmax)
    code = np.zeros(cen.shape[0], np.uint64)
    for a in range(3):
        if ext[a] > 0:
            q = (((cen[:, a] - cmin[a]).astype(f32) / ext[a]).astype(f32) * f32(1024)).astype(f32)
            if not np.isfinite(q).all():
                raise RefusedInput("a Morton quotient is not finite")
        else:
            q = np.zeros(cen.shape[0], f32)
        cell = np.clip(q, f32(0), f32(1023)).astype(np.uint64)      # truncation of a value in [0, 1023]
        for b in range(10):
            code |= ((cell >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return code


def morton_order(lo, hi):
    """(keys sorted ascending, the triangle of every position): key = code << 32 | index"""
    n = lo.shape[0]
    keys = (morton_codes(lo, hi) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    return keys[order], order.astype(np.int64)


def radix_tree(keys):
    """The recursive definition: a range of sorted, distinct keys splits after the last key that has a 0 in the highest bit in which
    the range's first and last key differ.  -> (left, right, slot) with node 0 the root."""
    keys = [int(k) for k in keys]
    left, right, slot = [-1], [-1], [-1]
    todo = [(0, 0, len(keys) - 1)]
    while todo:
        node, first, last = todo.pop()
        if first == last:
            slot[node] = first
            continue
        bit = (keys[first] ^ keys[last]).bit_length() - 1
        # the keys of the range agree above `bit`, so the first one with the bit set is the first >= (common prefix, 1, zeros)
        bound = ((keys[first] >> bit) | 1) << bit
        split = bisect.bisect_left(keys, bound, first, last + 1) - 1
        l = len(left)
        left += [-1, -1]; right += [-1, -1]; slot += [-1, -1]
        left[node], right[node] = l, l + 1
        todo += [(l, first, split), (l + 1, split + 1, last)]
    return left, right, slot


def ref_lbvh(triangles, vertices):
    lo, hi = triangle_boxes(triangles, vertices)
    keys, order = morton_order(lo, hi)
    left, right, slot = radix_tree(keys)
    return _emit(0, left, right, slot, order, lo, hi)


def ref_lbvh_order(triangles, vertices):
    """triangle_indices alone (no tree): for sizes at which only the order is compared"""
    lo, hi = triangle_boxes(triangles, vertices)
    return morton_order(lo, hi)[1].astype(np.int32)


# ---------------------------------------------------------------- PLOC ----

def ploc_radius(radius):
    return 16 if radius == 0 else min(int(radius), 64)


def ploc_neighbours(lo, hi, radius):
    """The position every cluster chooses: positions i +- d, d = 1..radius, nearest first, at each distance the side of the buddy i ^ 1
    first; a candidate replaces the current one only if its union's half-area is strictly smaller (or none was taken yet)."""
    m = lo.shape[0]
    i = np.arange(m)
    towards_buddy = np.where(i & 1, -1, 1)
    best = np.zeros(m, f32)
    nn = np.full(m, -1, np.int64)
    for d in range(1, radius + 1):
        if d >= m:
            break
        for sign in (1, -1):
            j = i + sign * d * towards_buddy
            ok = (j >= 0) & (j < m)
            jj = np.where(ok, j, 0)
            area = _half_area(np.minimum(lo, lo[jj]), np.maximum(hi, hi[jj]))
            if (area[ok] >= NO_SPLIT).any():
                raise RefusedInput("a union's half-area reaches 3e38")
            take = ok & ((nn < 0) | (area < best))
            best = np.where(take, area, best)
            nn = np.where(take, j, nn)
    return nn


def ref_ploc(triangles, vertices, radius=0, forced=None):
    """forced: an optional list that receives the cluster count of every iteration that took the forced merge of positions 0 and 1"""
    radius = ploc_radius(radius)
    lo, hi = triangle_boxes(triangles, vertices)
    n = lo.shape[0]
    _, order = morton_order(lo, hi)
    left, right, slot = [-1] * n, [-1] * n, list(range(n))          # node j < n: the leaf of Morton position j
    ids = np.arange(n)
    clo, chi = lo[order].copy(), hi[order].copy()
    while ids.shape[0] > 1:
        m = ids.shape[0]
        nn = ploc_neighbours(clo, chi, radius)
        i = np.arange(m)
        mutual = nn[nn] == i
        if not mutual.any():
            if m > PLOC_SINGLE_WORKGROUP:
                raise PlocNoProgress(f"no mutual pair among {m} clusters")
            if forced is not None:
                forced.append(m)
            nn = np.full(m, -1, np.int64)
            nn[0], nn[1] = 1, 0
            mutual = i < 2
        merge = mutual & (i < nn)
        keep = ~(mutual & (i > nn))
        partner = np.where(merge, nn, 0)
        new_ids = ids.copy()
        for p in np.nonzero(merge)[0]:                              # lower position first = left child
            new_ids[p] = len(left)
            left.append(int(ids[p])); right.append(int(ids[partner[p]])); slot.append(-1)
        nlo = np.where(merge[:, None], np.minimum(clo, clo[partner]), clo)
        nhi = np.where(merge[:, None], np.maximum(chi, chi[partner]), chi)
        ids, clo, chi = new_ids[keep], nlo[keep], nhi[keep]
    return _emit(int(ids[0]), left, right, slot, order, lo, hi)


# ---------------------------------------------------------------- SAH ----

SAH_BINS = 16


def sah_small(small):
    return 8 if small == 0 else min(max(int(small), 8), 32)


def _sah_cost(lo_l, hi_l, n_l, lo_r, hi_r, n_r):
    return ((_half_area(lo_l, hi_l) * n_l.astype(f32)).astype(f32) + (_half_area(lo_r, hi_r) * n_r.astype(f32)).astype(f32)).astype(f32)


def sah_bins_of(cen, cmin, ext):
    """(cnt, 3) bin numbers: clamp((int)((c - cmin) * (16 / ext)), 0, 15), 0 on an axis without extent"""
    out = np.zeros(cen.shape, np.int64)
    for a in range(3):
        if ext[a] > 0:
            scale = (f32(SAH_BINS) / ext[a]).astype(f32)
            q = ((cen[:, a] - cmin[a]).astype(f32) * scale).astype(f32)
            if not np.isfinite(q).all():
                raise RefusedInput("a bin quotient is not finite")
            out[:, a] = np.clip(q, f32(0), f32(SAH_BINS - 1)).astype(np.int64)
    return out


def _binned_split(tri, lo, hi, cen):
    """-> boolean mask of the triangles that go left, or None when no plane has triangles on both sides"""
    c = cen[tri]
    cmin, cmax = c.min(0), c.max(0)
    bins = sah_bins_of(c, cmin, _extent(cmin, cmax))
    cost = np.full((3, SAH_BINS - 1), np.inf, f32)
    for a in range(3):
        cnt = np.bincount(bins[:, a], minlength=SAH_BINS)
        blo = np.full((SAH_BINS, 3), np.inf, f32)
        bhi = np.full((SAH_BINS, 3), -np.inf, f32)
        np.minimum.at(blo, bins[:, a], lo[tri])
        np.maximum.at(bhi, bins[:, a], hi[tri])
        n_l = np.cumsum(cnt)[:-1]                                   # plane p = 1..15: bins [0, p) | [p, 16)
        n_r = cnt.sum() - n_l
        lo_l, hi_l = np.minimum.accumulate(blo, 0)[:-1], np.maximum.accumulate(bhi, 0)[:-1]
        lo_r, hi_r = np.minimum.accumulate(blo[::-1], 0)[::-1][1:], np.maximum.accumulate(bhi[::-1], 0)[::-1][1:]
        ok = (n_l > 0) & (n_r > 0)
        if ok.any():
            cst = _sah_cost(lo_l[ok], hi_l[ok], n_l[ok], lo_r[ok], hi_r[ok], n_r[ok])
            if (cst >= NO_SPLIT).any():
                raise RefusedInput("a split cost reaches 3e38")
            cost[a, ok] = cst
    best = int(np.argmin(cost))                                     # the first minimum: lower axis, then lower plane
    if not np.isfinite(cost.flat[best]):
        return None
    axis, plane = best // (SAH_BINS - 1), best % (SAH_BINS - 1) + 1
    return bins[:, axis] < plane


def _sweep_split(tri, lo, hi, cen):
    """The exact sweep over 2 or more triangles: -> (the winning axis's order of tri, number that go left)"""
    c = tri.shape[0]
    best, best_order, best_i = NO_SPLIT, None, c // 2
    k = np.arange(1, c)
    for a in range(3):
        o = tri[np.lexsort((tri, cen[tri, a]))]                     # by (centroid, triangle index)
        lo_l, hi_l = np.minimum.accumulate(lo[o], 0)[:-1], np.maximum.accumulate(hi[o], 0)[:-1]
        lo_r, hi_r = np.minimum.accumulate(lo[o][::-1], 0)[::-1][1:], np.maximum.accumulate(hi[o][::-1], 0)[::-1][1:]
        cost = _sah_cost(lo_l, hi_l, k, lo_r, hi_r, c - k)
        if (cost >= NO_SPLIT).any():
            raise RefusedInput("a split cost reaches 3e38")
        i = int(np.argmin(cost))                                    # ascending position, strictly smaller wins
        if cost[i] < best or best_order is None:
            if cost[i] < best:
                best, best_i = cost[i], i + 1
            best_order = o
    return best_order, best_i


def _sah_tree(lo, hi, small):
    n = lo.shape[0]
    cen = _centroids(lo, hi)
    idx = np.arange(n)
    left, right, slot = [-1], [-1], [-1]
    todo = [(0, 0, n)]
    while todo:
        node, beg, end = todo.pop()
        cnt = end - beg
        if cnt == 1:
            slot[node] = beg
            continue
        tri = idx[beg:end]
        if cnt > small:
            goes_left = _binned_split(tri, lo, hi, cen)
            if goes_left is None:
                n_left = cnt // 2                                   # by position
            else:
                n_left = int(goes_left.sum())
                idx[beg:end] = np.concatenate([tri[goes_left], tri[~goes_left]])      # stable
        else:
            idx[beg:end], n_left = _sweep_split(tri, lo, hi, cen)
        l = len(left)
        left += [-1, -1]; right += [-1, -1]; slot += [-1, -1]
        left[node], right[node] = l, l + 1
        todo += [(l, beg, beg + n_left), (l + 1, beg + n_left, end)]
    return _emit(0, left, right, slot, idx, lo, hi)


def ref_sah(triangles, vertices, small=0):
    lo, hi = triangle_boxes(triangles, vertices)
    return _sah_tree(lo, hi, sah_small(small))


def ref_sah_boxes(boxes, small=0):
    """the same build over given leaf boxes (n, 6) = lo, hi: the TLAS's path"""
    b = np.asarray(boxes, f32).reshape(-1, 6)
    lo, hi = b[:, :3].copy(), b[:, 3:].copy()
    _check_boxes(lo, hi)
    return _sah_tree(lo, hi, sah_small(small))


# ---------------------------------------------------------------- checks and diagnostics ----

def check_tree(flat, order, lo, hi):
    """A valid BVH2 in the documented layout over the boxes lo / hi (what tests/test_gpu_parity.py asserts of a device-built tree)"""
    n = lo.shape[0]
    order = np.asarray(order)
    assert flat.shape == (2 * n - 1, 8) and flat.dtype == np.float32
    assert sorted(order.tolist()) == list(range(n)), "triangle_indices is not a permutation"
    leaf = flat[:, 7] != 0
    assert (flat[leaf, 7] == 1).all() and int(leaf.sum()) == n
    inner = np.nonzero(~leaf)[0]
    l = flat[inner, 3].astype(np.int64)
    assert np.array_equal(l, 2 * np.arange(inner.shape[0]) + 1), "not breadth-first with adjacent children"
    slots = flat[leaf, 3].astype(np.int64)
    assert sorted(slots.tolist()) == list(range(n)), "leaf slots are not a permutation"
    assert np.array_equal(flat[leaf, 0:3], lo[order[slots]]) and np.array_equal(flat[leaf, 4:7], hi[order[slots]]), "leaf boxes"
    assert np.array_equal(flat[inner, 0:3], np.minimum(flat[l, 0:3], flat[l + 1, 0:3])), "interior lo is not the union"
    assert np.array_equal(flat[inner, 4:7], np.maximum(flat[l, 4:7], flat[l + 1, 4:7])), "interior hi is not the union"


def _depths_and_counts(flat):
    n = flat.shape[0]
    depth, count = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for p in range(n):
        if flat[p, 7] == 0:
            l = int(flat[p, 3])
            if 0 < l < n - 1:
                depth[l] = depth[l + 1] = depth[p] + 1
    for p in range(n - 1, -1, -1):
        if flat[p, 7] != 0:
            count[p] = 1
        else:
            l = int(flat[p, 3])
            if 0 < l < n - 1:
                count[p] = count[l] + count[l + 1]
    return depth, count


def first_difference(flat_a, order_a, flat_b, order_b):
    """None if the two trees are the same bytes; else a sentence that names the first breadth-first node at which they part (link, leaf
    flag or leaf triangle), or, with equal topology, the deepest node whose box differs: its depth, the triangles under it, both rows."""
    flat_a, flat_b = np.asarray(flat_a, f32), np.asarray(flat_b, f32)
    order_a, order_b = np.asarray(order_a), np.asarray(order_b)
    if flat_a.shape != flat_b.shape or order_a.shape != order_b.shape:
        return f"shapes differ: {flat_a.shape} {order_a.shape} against {flat_b.shape} {order_b.shape}"
    same_rows = (flat_a.view(np.uint32) == flat_b.view(np.uint32)).all(1)
    if same_rows.all() and np.array_equal(order_a, order_b):
        return None

    def leaf_triangle(flat, order):
        leaf = flat[:, 7] != 0
        s = np.clip(flat[:, 3].astype(np.int64), 0, order.shape[0] - 1)
        return np.where(leaf, order[s], -1)
    topo = (flat_a[:, 3] != flat_b[:, 3]) | (flat_a[:, 7] != flat_b[:, 7]) | (leaf_triangle(flat_a, order_a) != leaf_triangle(flat_b, order_b))
    if topo.any():
        p, what = int(np.nonzero(topo)[0][0]), "first node whose link, leaf flag or triangle differs"
    elif not same_rows.all():
        p, what = int(np.nonzero(~same_rows)[0][-1]), "same topology; deepest node whose box differs"
    else:
        s = int(np.nonzero(order_a != order_b)[0][0])
        return f"same nodes; triangle_indices differ first at slot {s}: {order_a[s]} against {order_b[s]}"
    da, ca = _depths_and_counts(flat_a)
    _, cb = _depths_and_counts(flat_b)
    ta, tb = leaf_triangle(flat_a, order_a)[p], leaf_triangle(flat_b, order_b)[p]
    return (f"{what}: node {p} of {flat_a.shape[0]}, depth {da[p]}, triangles below {ca[p]} against {cb[p]}, leaf triangle {ta} against {tb}\n"
            f"  a: {flat_a[p].tolist()}\n  b: {flat_b[p].tolist()}")
