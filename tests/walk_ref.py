"""Numpy walkers for the two trees a flat scene is walked through, written from include/crt.h (the crt_node8 and crt_flatnode layouts and
the meta bytes), DESIGN.md §3 and §5 and the shader the kernels restate (Shader/cwbvh.fs for the CWBVH walk, the octant and the inner test;
Shader/path_trace.fs trace_bvh / hit_shadow and hit_bbox for the BVH2) — not from oracle/ or csrc/, and importing nothing from either — so that
the HIP walks and the C oracle are both held to a third reading, visit counts and stack use included (DESIGN.md "The walks as tested").

The walkers step all rays of a call side by side (one numpy operation per step of the slowest ray), but every ray's own sequence of node
visits and triangle tests is the one a scalar walk makes: no ray's step reads another ray's state.  Every arithmetic step is ONE float32
IEEE operation; the only fused one is the plane of the CWBVH child test.

    cwbvh_walk(nodes, tris, rays, any_hit)  ->  Walk (slot, id, t, u, v, n_nodes, n_tris, stack, refused)
    bvh2_walk(flat, tris, rays, any_hit)    ->  Walk
    depth8(nodes), depth2(flat)             ->  depths by their own traversal

`tris` is either the (n, 12) float32 intersection records (v0 | id) (e1 | slot) (e2 | material) in the order the tree names them, or the
tuple (tri_slots, leaf_tris, V, ids) they are gathered from (tri_slots None for the BVH2: its leaves name the slots themselves).

The CWBVH walk, per ray (cwbvh.fs:448-616 with the corrections of SURVEY appendix C):
  * a ray whose origin is not finite visits nothing;
  * dc = d with every component of magnitude <= 2^-80 (zeros, -0, denormals; a NaN too) replaced by 2^-80 with the component's sign bit;
    octant, near / far plane choice and inv = 1 / dc come from dc, Moeller-Trumbore keeps d;
  * node test: adj_inv = 2^(e-127) * inv, adj_o = (p - o) * inv, plane = fma(q, adj_inv, adj_o);
    tmin = max(max(tx, ty), max(tz, 0)), tmax = min(min(tx, ty), min(tz, max_t)) with NaN operands ignored; a child passes when tmin <= tmax;
    a passing child sets (meta >> 5) << ((meta ^ (octant & inner)) & 31): inner children land in bits 24..31 at (slot ^ octant), a leaf's
    unary count at its offset into the node's triangle group;
  * the node group (child base, inner hits | imask): the highest hit bit is taken first, what is left of the group is pushed if any inner
    hit is left, the child is tested, and ITS triangle group is tested at once, highest bit first — a triangle group is never pushed;
  * with no inner hit left the walk pops; with nothing to pop it ends;
  * closest hit: nearer wins, equal t goes to the lower original id, max_t follows the best t; any hit: the first t < max_t ends the walk.
The stack use of a ray is the largest number of entries it held; with `stack_entries` given, a push that does not fit is dropped and counted
in `refused` (what the kernels' checked pushes do and count in stack_overflows).

The BVH2 walk (path_trace.fs:511-652 closest, :669-819 any; hit_bbox :84-109): raw 1 / d, the sentinel -1 pushed first, near child first
(tl1 > tl2 picks the right one), the far one pushed; closest: th > 0 and th >= tl and tl < t (`<=` under the lowest-id tie rule, so that a
box holding an equal-t triangle is still entered); any: th >= 0 and th >= tl and tl <= max_t.  The stack use counts the sentinel.

`mistake` plants one wrong reading (tests/test_walk_ref.py shows that each changes a hit, a count or a stack depth on the fixtures).
"""
from collections import namedtuple

import numpy as np

from integrator_ref import _add_round_to_odd

f32 = np.float32
f64 = np.float64
u32 = np.uint32

Walk = namedtuple("Walk", "slot id t u v n_nodes n_tris stack refused")

MISTAKES = ("reversed child order", "< for <= in the child test", "leaf group pushed", "tie rule dropped", "octant bit flipped")
_CAP = 128          # the walker's own stack rows: above every bound the library knows (16 CWBVH, 96 BVH2)
_EPS = f32(2.0 ** -80)


def fma32(a, b, c):
    """a * b + c of float32 arrays with one rounding: the product of two float32 is exact in float64, the sum is rounded to odd there
    (integrator_ref's helper, tested against fractions.Fraction) and once more, now correctly, to float32.  Where the float64 sum is not
    finite (an infinite or NaN operand: float32 products cannot overflow float64) it is the result as it stands."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
        c64 = np.broadcast_to(np.asarray(c, f32).astype(f64), p.shape)
        plain = p + c64
        ok = np.isfinite(plain)
        odd = _add_round_to_odd(np.where(ok, p, 0.0), np.where(ok, c64, 0.0))
        return np.where(ok, odd, plain).astype(f32)


def records(tris):
    """(n, 12) float32 records from either form of `tris`"""
    if isinstance(tris, tuple):
        tri_slots, leaf_tris, V, ids = tris
        leaf_tris = np.asarray(leaf_tris, np.int32).reshape(-1, 12)
        V = np.asarray(V, f32).reshape(-1, 3)
        slots = np.arange(leaf_tris.shape[0], dtype=np.int32) if tri_slots is None else np.asarray(tri_slots, np.int32)
        ids = slots if ids is None else np.asarray(ids, np.int32)[slots]
        t = leaf_tris[slots]
        v0 = V[t[:, 0]]
        r = np.zeros((slots.shape[0], 12), f32)
        r[:, 0:3], r[:, 4:7], r[:, 8:11] = v0, V[t[:, 1]] - v0, V[t[:, 2]] - v0
        r[:, 3], r[:, 7], r[:, 11] = ids.astype(np.int32).view(f32), slots.view(f32), t[:, 3].copy().view(f32)
        return r
    return np.ascontiguousarray(tris, f32).reshape(-1, 12)


def _dot(a, b):
    return ((a[:, 0] * b[:, 0]).astype(f32) + (a[:, 1] * b[:, 1]).astype(f32)).astype(f32) + (a[:, 2] * b[:, 2]).astype(f32)


def _cross(a, b):
    return np.stack([(a[:, 1] * b[:, 2]).astype(f32) - (a[:, 2] * b[:, 1]).astype(f32),
                     (a[:, 2] * b[:, 0]).astype(f32) - (a[:, 0] * b[:, 2]).astype(f32),
                     (a[:, 0] * b[:, 1]).astype(f32) - (a[:, 1] * b[:, 0]).astype(f32)], 1).astype(f32)


def _moller_trumbore(o, d, rec):
    """path_trace.fs:322-374 in the order of conftest.numpy_brute_force, one record per ray: (u, v, t, inside)"""
    v0, e1, e2 = rec[:, 0:3], rec[:, 4:7], rec[:, 8:11]
    with np.errstate(all="ignore"):
        return _moller_trumbore_ops(o, d, v0, e1, e2)


def _moller_trumbore_ops(o, d, v0, e1, e2):
    pv = _cross(d, e2)
    tv = (o - v0).astype(f32)
    qv = _cross(tv, e1)
    u, v, t = _dot(tv, pv), _dot(d, qv), _dot(e2, qv)
    inv = (f32(1.0) / _dot(e1, pv)).astype(f32)
    u, v, t = (u * inv).astype(f32), (v * inv).astype(f32), (t * inv).astype(f32)
    w = ((f32(1.0) - u).astype(f32) - v).astype(f32)
    return u, v, t, (u >= 0) & (v >= 0) & (t >= 0) & (w >= 0)


class _Hits:
    """the best hit of every ray, and the counters"""

    def __init__(self, rays, recs):
        n = rays.shape[0]
        self.recs = recs
        self.o, self.d = np.ascontiguousarray(rays["o"], f32), np.ascontiguousarray(rays["d"], f32)
        self.max_t = np.ascontiguousarray(rays["tmax"], f32).copy()
        self.slot, self.id = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        self.t, self.u, self.v = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
        self.n_nodes, self.n_tris = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.stack, self.refused = np.zeros(n, np.int64), np.zeros(n, np.int64)

    def test(self, r, k, any_hit, tie=True):
        """rays r against records k; returns which of them end their walk (any hit)"""
        rec = self.recs[k]
        self.n_tris[r] += 1
        u, v, t, inside = _moller_trumbore(self.o[r], self.d[r], rec)
        rid = rec[:, 3].copy().view(np.int32)
        if any_hit:
            take = inside & (t < self.max_t[r])
        else:
            take = inside & (t < self.max_t[r])
            if tie:
                take |= inside & (t == self.max_t[r]) & (self.slot[r] >= 0) & (rid < self.id[r])
        w = r[take]
        self.slot[w], self.id[w] = rec[take, 7].copy().view(np.int32), rid[take]
        self.t[w], self.u[w], self.v[w] = t[take], u[take], v[take]
        if not any_hit:
            self.max_t[w] = t[take]
        return take if any_hit else np.zeros(r.shape[0], bool)

    def result(self):
        return Walk(self.slot, self.id, self.t, self.u, self.v, self.n_nodes, self.n_tris, self.stack, self.refused)


def _push(h, r, sp, rows, values, bound):
    """push values[i] (tuple of columns) for rays r where it fits under `bound`; the others are refused"""
    fits = sp[r] < bound
    w = r[fits]
    for row, val in zip(rows, values):
        row[w, sp[w]] = val[fits]
    sp[w] += 1
    h.stack[w] = np.maximum(h.stack[w], sp[w])
    h.refused[r[~fits]] += 1


def _msb(x):
    """findMSB of non-zero uint32 values"""
    return np.frexp(x.astype(f64))[1].astype(np.int64) - 1


def _popcount(x):
    x = x.astype(np.uint64)
    c = np.zeros(x.shape, np.int64)
    for k in range(32):
        c += ((x >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
    return c


def _node_test(nd, o, neg, inv, oct4, max_t, strict=False):
    """cwbvh.fs:376-446 as corrected: the hit mask of the rays' nodes nd (m, 80) uint8"""
    with np.errstate(all="ignore"):
        p = nd[:, 0:12].copy().view(f32)
        e = nd[:, 12:15].astype(u32)
        scale = (e << u32(23)).view(f32)
        adj_inv = (scale * inv).astype(f32)
        adj_o = ((p - o).astype(f32) * inv).astype(f32)
        meta = nd[:, 24:32].astype(u32)
        inner = ((meta & (meta << u32(1))) & u32(0x10)) != 0
        bit_index = (meta ^ np.where(inner, oct4[:, None], u32(0))) & u32(0x1f)
        child_bits = (meta >> u32(5)) & u32(7)
        q = nd[:, 32:80].reshape(-1, 3, 2, 8).astype(f32)                       # axis, lo / hi, slot
        tn, tf = [], []
        for k in range(3):
            near = np.where(neg[:, k, None], q[:, k, 1], q[:, k, 0])
            far = np.where(neg[:, k, None], q[:, k, 0], q[:, k, 1])
            tn.append(fma32(near, adj_inv[:, k, None], adj_o[:, k, None]))
            tf.append(fma32(far, adj_inv[:, k, None], adj_o[:, k, None]))
        tmin = np.fmax(np.fmax(tn[0], tn[1]), np.fmax(tn[2], f32(0.0)))
        tmax = np.fmin(np.fmin(tf[0], tf[1]), np.fmin(tf[2], max_t[:, None]))
        passes = (tmin < tmax) if strict else (tmin <= tmax)
        bits = np.where(passes, child_bits << bit_index, u32(0)).astype(u32)
        return np.bitwise_or.reduce(bits, axis=1).astype(u32)


def cwbvh_walk(nodes, tris, rays, any_hit, stack_entries=None, mistake=None):
    assert mistake is None or mistake in MISTAKES
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 80)
    recs = records(tris)
    n = rays.shape[0]
    h = _Hits(rays, recs)
    bound = _CAP if stack_entries is None else int(stack_entries)
    assert bound <= _CAP
    with np.errstate(all="ignore"):
        d = h.d
        dc = np.where(np.abs(d) > _EPS, d, np.copysign(_EPS, d)).astype(f32)
        neg = dc < 0
        inv = (f32(1.0) / dc).astype(f32)
    octant = (np.where(neg[:, 0], 0, 4) | np.where(neg[:, 1], 0, 2) | np.where(neg[:, 2], 0, 1)).astype(u32)
    if mistake == "octant bit flipped":
        octant = octant ^ u32(1)
    oct4 = octant                                                       # one byte of oct_inv4: every use is per slot
    cur_x, cur_y = np.zeros(n, u32), np.full(n, 0x80000000, u32)
    tri_x, tri_y = np.zeros(n, u32), np.zeros(n, u32)
    sp = np.zeros(n, np.int64)
    stk_x, stk_y = np.zeros((n, _CAP), u32), np.zeros((n, _CAP), u32)
    alive = np.isfinite(h.o).all(1)
    INNER = u32(0xff000000)
    while alive.any():
        # one step per live ray: a triangle of its pending group, else a node of its node group, else a pop
        r = np.nonzero(alive & (tri_y != 0))[0]
        if r.size:
            b = _msb(tri_y[r])
            tri_y[r] &= ~(u32(1) << b.astype(u32))
            done = h.test(r, tri_x[r].astype(np.int64) + b, any_hit, tie=mistake != "tie rule dropped")
            alive[r[done]] = False
        r = np.nonzero(alive & (tri_y == 0) & ((cur_y & INNER) != 0))[0]
        stepped = np.zeros(n, bool)
        if r.size:
            stepped[r] = True
            hits_imask = cur_y[r]
            if mistake == "reversed child order":
                low = hits_imask & INNER
                off = _msb(low & (~low + u32(1)))                       # the lowest inner bit
            else:
                off = _msb(hits_imask)
            cur_y[r] = hits_imask & ~(u32(1) << off.astype(u32))
            more = (cur_y[r] & INNER) != 0
            _push(h, r[more], sp, (stk_x, stk_y), (cur_x[r][more], cur_y[r][more]), bound)
            slot = (off - 24).astype(u32) ^ oct4[r]
            rel = _popcount(hits_imask & ~(u32(0xffffffff) << slot) & u32(0xff))
            idx = cur_x[r].astype(np.int64) + rel
            nd = nodes[idx]
            h.n_nodes[r] += 1
            mask = _node_test(nd, h.o[r], neg[r], inv[r], oct4[r], h.max_t[r], strict=mistake == "< for <= in the child test")
            cur_x[r] = nd[:, 16:20].copy().view(u32)[:, 0]
            cur_y[r] = (mask & INNER) | nd[:, 15].astype(u32)
            tx, ty = nd[:, 20:24].copy().view(u32)[:, 0], mask & u32(0x00ffffff)
            if mistake == "leaf group pushed":
                # the wrong reading: with inner hits pending the triangle group waits on the stack
                wait = ((cur_y[r] & INNER) != 0) & (ty != 0)
                _push(h, r[wait], sp, (stk_x, stk_y), (tx[wait], ty[wait]), bound)
                ty = np.where(wait, u32(0), ty)
            tri_x[r], tri_y[r] = tx, ty
        # a ray with neither a triangle nor an inner hit left pops, or ends
        r = np.nonzero(alive & ~stepped & (tri_y == 0) & ((cur_y & INNER) == 0))[0]
        if r.size:
            empty = sp[r] == 0
            alive[r[empty]] = False
            w = r[~empty]
            sp[w] -= 1
            px, py = stk_x[w, sp[w]], stk_y[w, sp[w]]
            is_group = (py & INNER) != 0
            cur_x[w], cur_y[w] = np.where(is_group, px, u32(0)), np.where(is_group, py, u32(0))
            tri_x[w], tri_y[w] = np.where(is_group, tri_x[w], px), np.where(is_group, u32(0), py)
    return h.result()


def _hit_bbox(o, lo, hi, inv):
    """path_trace.fs:84-109: (th, tl), min / max ignoring a NaN operand"""
    with np.errstate(all="ignore"):
        a = ((lo - o).astype(f32) * inv).astype(f32)
        b = ((hi - o).astype(f32) * inv).astype(f32)
        far, near = np.fmax(b, a), np.fmin(b, a)
        th = np.fmin(far[:, 0], np.fmin(far[:, 1], far[:, 2]))
        tl = np.fmax(near[:, 0], np.fmax(near[:, 1], near[:, 2]))
    return th, tl


def _link(x):
    """a FlatNode link: an index stored as a float (include/crt.h crt_flatnode)"""
    return x.astype(np.int64)


def bvh2_walk(flat, tris, rays, any_hit, stack_entries=None, tie_lowest_id=True):
    flat = np.ascontiguousarray(flat, f32).reshape(-1, 8)
    recs = records(tris)
    n = rays.shape[0]
    h = _Hits(rays, recs)
    bound = _CAP if stack_entries is None else int(stack_entries)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / h.d).astype(f32)
    stk = np.zeros((n, _CAP), np.int64)
    sp = np.zeros(n, np.int64)
    allr = np.arange(n)
    _push(h, allr, sp, (stk,), (np.full(n, -1, np.int64),), bound)
    ind = np.zeros(n, np.int64)
    lo_i, hi_i = np.zeros(n, np.int64), np.zeros(n, np.int64)           # the leaf range a ray is testing
    alive = np.ones(n, bool)
    while alive.any():
        # a ray inside a leaf tests its next triangle
        r = np.nonzero(alive & (lo_i < hi_i))[0]
        in_leaf = np.zeros(n, bool)
        in_leaf[r] = True
        if r.size:
            done = h.test(r, lo_i[r], any_hit, tie=tie_lowest_id)
            lo_i[r] += 1
            alive[r[done]] = False
            fin = r[~done & (lo_i[r] >= hi_i[r])]                       # the leaf is finished: pop
            sp[fin] -= 1
            ind[fin] = stk[fin, sp[fin]]
            alive[fin[ind[fin] < 0]] = False
        r = np.nonzero(alive & ~in_leaf)[0]
        if not r.size:
            continue
        nd = flat[ind[r]]
        h.n_nodes[r] += 1
        left = _link(nd[:, 3])
        leaf = nd[:, 7] != 0
        w = r[leaf]
        lo_i[w], hi_i[w] = left[leaf], left[leaf] + nd[leaf, 7].astype(np.int64)
        w, left = r[~leaf], left[~leaf]
        if w.size:
            a, b = flat[left], flat[left + 1]
            th1, tl1 = _hit_bbox(h.o[w], a[:, 0:3], a[:, 4:7], inv[w])
            th2, tl2 = _hit_bbox(h.o[w], b[:, 0:3], b[:, 4:7], inv[w])
            t = h.max_t[w]
            with np.errstate(all="ignore"):
                if any_hit:
                    l = (th1 >= 0) & (th1 >= tl1) & (tl1 <= t)
                    rr = (th2 >= 0) & (th2 >= tl2) & (tl2 <= t)
                elif tie_lowest_id:
                    l = (th1 > 0) & (th1 >= tl1) & (tl1 <= t)
                    rr = (th2 > 0) & (th2 >= tl2) & (tl2 <= t)
                else:
                    l = (th1 > 0) & (th1 >= tl1) & (tl1 < t)
                    rr = (th2 > 0) & (th2 >= tl2) & (tl2 < t)
                off = np.where(tl1 > tl2, 1, 0)
            both = l & rr
            _push(h, w[both], sp, (stk,), ((left + 1 - off)[both],), bound)
            nxt = np.where(both, left + off, np.where(l, left, left + 1))
            go = l | rr
            ind[w[go]] = nxt[go]
            pop = w[~go]
            sp[pop] -= 1
            ind[pop] = stk[pop, sp[pop]]
            alive[pop[ind[pop] < 0]] = False
    return h.result()


def depth8(nodes):
    """node8 levels, the root's = 1: every node's level from its parent's, through imask and child_base_index"""
    nodes = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 80)
    if nodes.shape[0] == 0:
        return 0
    deepest, level = 0, [0]
    while level:
        deepest += 1
        nxt = []
        for i in level:
            base = int(nodes[i, 16:20].copy().view(u32)[0])
            nxt += [base + k for k in range(bin(int(nodes[i, 15])).count("1"))]
        level = nxt
    return deepest


def depth2(flat):
    """deepest leaf level of a FlatNode tree, the root's = 0 (what crt_bvh_info.bvh2_depth and the BVH2 stack bound count)"""
    flat = np.ascontiguousarray(flat, f32).reshape(-1, 8)
    if flat.shape[0] == 0:
        return 0
    deepest, level = -1, [0]
    while level:
        deepest += 1
        nxt = []
        for i in level:
            if flat[i, 7] == 0:
                left = int(flat[i, 3])
                nxt += [left, left + 1]
        level = nxt
    return deepest
