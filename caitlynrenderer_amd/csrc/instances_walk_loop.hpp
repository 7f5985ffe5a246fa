// The loop of the two-level walk, as TEXT: included inside a kernel's body, once per pool of rays a wave walks.
// k_trace_instances must keep the machine code it had before the frame path existed ("assembly"); as a function template
// the loop did not (the compiler simplifies a callee on its own before it inlines it, and the kernel came out with other branches), as
// text it does, and the three kernels still share one source.
//
// In scope at the point of inclusion:
//   ANY, STATS, MASK   compile-time bools
//   a                  the kernel's arguments: nodes, tris, inst, n_instances, refill_min, tri_min, overflow (+ child_masks, n_tlas8 with MASK)
//   stk, lane          the lane's stack column in LDS and its lane index;  stack_entries  (int)
//   next, end          the pool [next, end); next is advanced
//   CRT_WALK_LOAD(idx, r0, r1)                  declares float4 r0, r1 = the two rows of ray idx
//   CRT_WALK_DONE(idx, h, hit, inst, nn, nt)    ray idx is done: h = crt_hit's row, hit, inst = its instance when hit, visit counts (STATS)
//   CRT_WALK_MASK(lane_mask)                    MASK: the ray mask the two tests take, given the lane's own (the low byte of its ray's pad word).
//                                               k_trace_instances: lane_mask itself, a mask per ray.  The frame kernels: their launch's mask, a
//                                               kernel argument, so that no register carries a mask per lane
//
// One lane per ray with lane refill, one loop and one LDS stack over both levels.  Stack entries: a node group (top byte set), the rest of a
// TLAS leaf (low 24 bits only) or the return marker (y == 0).
// MASK: the ray's mask is CRT_WALK_MASK of the low 8 bits of its pad word; a TLAS step culls the children whose child mask does not meet it, and the
// instance step skips an instance whose mask does not, before it transforms the ray.  Without MASK every such test folds away.
    uint32_t idx = 0, nn = 0, nt = 0, inst_cur = 0, rmask = 0;
    vec3 wo = V3(0.f, 0.f, 0.f), wd = V3(0.f, 0.f, 1.f), o = wo, d = wd, inv = V3(0.f, 0.f, 0.f);
    bool negx = false, negy = false, negz = false, in_blas = false;
    uint32_t oct4 = 0;
    float best_t = 0.f, best_u = 0.f, best_v = 0.f;
    int best_id = -1, best_inst = -1;
    int sp = 0;
    uint2 cur = make_uint2(0u, 0u), tg = make_uint2(0u, 0u);
    for (;;) {
        bool busy = tg.y != 0u || (cur.y & 0xff000000u) != 0u;
        if (next < end) {
            const unsigned long long idle = __ballot(!busy);
            const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle);
            if (n_idle >= a.refill_min || n_idle == 64u) {
                const uint32_t got = end - next < n_idle ? end - next : n_idle;
                const uint32_t rank = (uint32_t)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
                if (!busy && rank < got) {
                    idx = next + rank;
                    CRT_WALK_LOAD(idx, r0, r1)
                    wo = V3(r0.x, r0.y, r0.z); wd = V3(r1.x, r1.y, r1.z);
                    if (MASK) rmask = __float_as_uint(r1.w) & 0xffu;
                    o = wo; d = wd;
                    best_t = r0.w; best_u = 0.f; best_v = 0.f; best_id = -1; best_inst = -1;
                    nn = 0; nt = 0; sp = 0; in_blas = false;
                    busy = true;
                    // a non-finite origin hits nothing (traverse()); no instance: every ray misses
                    const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z);
                    ray_setup(d, inv, negx, negy, negz, oct4);
                    cur = (finite && a.n_instances != 0u) ? make_uint2(0u, 0x80000000u) : make_uint2(0u, 0u);
                    tg = make_uint2(0u, 0u);
                }
                next += got;
            }
        }
        if (__ballot(busy) == 0ull) break;        // pool drained and every lane finished

        // one step per iteration: a node step (TLAS or BLAS: the same code) or a leaf step (a triangle test, or entering an instance),
        // with walk_pool's vote between the two
        const bool has_tri = busy && tg.y != 0u;
        const bool can_node = busy && !has_tri && (cur.y & 0xff000000u);
        const uint32_t n_tri = (uint32_t)__builtin_popcountll(__ballot(has_tri));
        const uint32_t n_node = (uint32_t)__builtin_popcountll(__ballot(can_node));
        const bool node_phase = n_node != 0u && n_node >= a.tri_min * n_tri;
        bool finished = false;
        if (node_phase) {
            if (can_node) {
                const uint32_t hits_imask = cur.y;
                const int off = 31 - __builtin_clz(hits_imask);
                const uint32_t nbase = cur.x;
                cur.y &= ~(1u << off);
                if (cur.y & 0xff000000u) { if (sp < stack_entries) { stk[sp * 64] = cur; ++sp; } else atomicAdd(a.overflow, 1u); }
                const uint32_t slot = (uint32_t)(off - 24) ^ (oct4 & 0xffu);
                const uint32_t nidx = nbase + (uint32_t)__builtin_popcount(hits_imask & ~(0xffffffffu << slot));
                const uint4* np = node_rows(a.nodes, nidx);
                const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3], n4 = np[4];
                if (STATS) ++nn;
                uint32_t keep = 0xffu;
                if constexpr (MASK) { if (nidx < a.n_tlas8) keep = child_keep(a.child_masks[nidx], CRT_WALK_MASK(rmask)); }
                const uint32_t hitmask = node8_intersect(n0, n1, n2, n3, n4, o, inv, negx, negy, negz, oct4, best_t, keep);
                cur.x = n1.x;
                tg.x = n1.y;
                cur.y = (hitmask & 0xff000000u) | (n0.w >> 24);
                tg.y = hitmask & 0x00ffffffu;
            }
        } else if (has_tri) {
            const int b = 31 - __builtin_clz(tg.y);
            tg.y &= ~(1u << b);
            const uint32_t ti = tg.x + (uint32_t)b;
            if (in_blas) {
                const float4* tp = tri_rows(a.tris, ti);
                const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                if (STATS) ++nt;
                float u, vv, t;
                if (mt_test(ta, tb, tc, o, d, u, vv, t)) {
                    if (ANY) {
                        if (t < best_t) { best_inst = (int)inst_cur; finished = true; tg.y = 0u; }
                    } else {
                        // nearest t, then lowest instance, then lowest triangle id: independent of the order the TLAS hands out instances
                        const int id = __float_as_int(ta.w);
                        bool take = t < best_t;
                        if (t == best_t && best_inst >= 0) take = (int)inst_cur < best_inst || ((int)inst_cur == best_inst && id < best_id);
                        if (take) { best_t = t; best_u = u; best_v = vv; best_id = id; best_inst = (int)inst_cur; }
                    }
                }
            } else {
                // an instance: into its object space (fp32, no fma, direction not renormalised: t is the same parameter in both spaces)
                const float4* ip = a.inst + 4 * (size_t)ti;
                const float4 w0 = ip[0], w1 = ip[1], w2 = ip[2], w3 = ip[3];
                const bool visible = !MASK || (__float_as_uint(w3.w) & CRT_WALK_MASK(rmask)) != 0u;      // a hidden instance: skipped untransformed
                vec3 oo = wo, od = wd;
                if (visible && __float_as_uint(w3.z) == 0u) {
                    oo = V3(((w0.x * wo.x + w0.y * wo.y) + w0.z * wo.z) + w0.w, ((w1.x * wo.x + w1.y * wo.y) + w1.z * wo.z) + w1.w,
                            ((w2.x * wo.x + w2.y * wo.y) + w2.z * wo.z) + w2.w);
                    od = V3((w0.x * wd.x + w0.y * wd.y) + w0.z * wd.z, (w1.x * wd.x + w1.y * wd.y) + w1.z * wd.z, (w2.x * wd.x + w2.y * wd.y) + w2.z * wd.z);
                }
                // an object origin that is not finite hits nothing in this instance (traverse()): the instance is skipped
                if (visible && __builtin_isfinite(oo.x) && __builtin_isfinite(oo.y) && __builtin_isfinite(oo.z)) {
                    const int need = ((cur.y & 0xff000000u) ? 1 : 0) + (tg.y ? 1 : 0) + 1;
                    if (sp + need <= stack_entries) {
                        if (cur.y & 0xff000000u) { stk[sp * 64] = cur; ++sp; }
                        if (tg.y) { stk[sp * 64] = tg; ++sp; }
                        stk[sp * 64] = make_uint2(0u, 0u);      // return marker
                        ++sp;
                        o = oo; d = od;
                        ray_setup(d, inv, negx, negy, negz, oct4);
                        in_blas = true;
                        inst_cur = __float_as_uint(w3.y);
                        cur = make_uint2(__float_as_uint(w3.x), 0x80000000u);
                        tg = make_uint2(0u, 0u);
                    } else {
                        atomicAdd(a.overflow, 1u);
                    }
                }
            }
        }
        // a lane with neither a leaf group nor inner hits left pops its stack (through a return marker: back to the world ray), or is done
        if (busy && !finished && tg.y == 0u && !(cur.y & 0xff000000u)) {
            for (;;) {
                if (sp == 0) { finished = true; break; }
                --sp;
                const uint2 e = stk[sp * 64];
                if (e.y == 0u) {
                    o = wo; d = wd;
                    ray_setup(d, inv, negx, negy, negz, oct4);
                    in_blas = false;
                    continue;
                }
                if (e.y & 0xff000000u) cur = e;
                else { tg = e; cur = make_uint2(0u, 0u); }
                break;
            }
        }
        if (finished) {
            const bool hit = best_inst >= 0;
            float4 h;
            h.x = ANY ? 0.f : (hit ? best_t : 0.f);
            h.y = ANY ? 0.f : best_u;
            h.z = ANY ? 0.f : best_v;
            h.w = __int_as_float(ANY ? (hit ? 0 : -1) : (hit ? best_id : -1));
            CRT_WALK_DONE(idx, h, hit, best_inst, nn, nt)
            cur = make_uint2(0u, 0u); tg = make_uint2(0u, 0u); sp = 0; in_blas = false;
        }
    }
