// HIP kernels of instanced scenes (include/crt.h crt_instances_*): per-instance preparation (validation, inverse, world
// box, record), the packing of the BLASes into one node array, and the two-level walk k_trace_instances.
//
// The walk is ONE loop with ONE stack per lane.  TLAS and BLAS nodes are the same node8 format in the same array, so a wave whose lanes
// are at different levels still runs a single node step together.  A TLAS leaf's "triangles" are instances: the instance step pushes
// what the lane still has pending at the TLAS level (inner hits, the rest of the leaf), then a return marker, moves the ray into object
// space and continues at the BLAS root.  Popping the marker restores the world ray, which the lane keeps in registers.
// The masked walk (MASK) culls TLAS children whose instances are all hidden from the ray and skips hidden instances.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "instances.hpp"
#include "rt_kernels.hpp"
#include "rt_math.hpp"
#include "rt_traverse.hpp"
#include "host/instance_math.hpp"

namespace crt {

__global__ void __launch_bounds__(256) k_instance_prep(InstPrepArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t* src = a.in + 16 * (size_t)i;
    float m[12];
    for (int k = 0; k < 12; ++k) m[k] = __uint_as_float(src[k]);
    const uint32_t mesh = src[12];
    uint32_t bad = 0;
    float w[12];
    if (!instance_inverse(m, w)) bad |= 1u;
    if (mesh >= a.n_meshes) bad |= 2u;
    float box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!bad) {
        instance_world_box(m, a.mesh_box + 6 * (size_t)mesh, box);
        for (int k = 0; k < 6; ++k) if (!(fabsf(box[k]) <= 1e18f)) bad |= 4u;      // the builder's coordinate bound (lbvh.hip CRT_MAX_COORD)
    }
    if (bad) { atomicOr(a.flag, bad); return; }
    float4* r = a.rec + 4 * (size_t)i;
    r[0] = make_float4(w[0], w[1], w[2], w[3]);
    r[1] = make_float4(w[4], w[5], w[6], w[7]);
    r[2] = make_float4(w[8], w[9], w[10], w[11]);
    r[3] = make_float4(__uint_as_float(a.mesh_root[mesh]), __uint_as_float(i), __uint_as_float(instance_is_identity(m) ? 1u : 0u),
                       __uint_as_float(src[13] & 0xffu));       // crt_instance.mask: bits 8..31 are ignored
    for (int k = 0; k < 6; ++k) a.box[6 * (size_t)i + k] = box[k];
    for (int k = 0; k < 12; ++k) a.w2o[12 * (size_t)i + k] = w[k];
}

__global__ void __launch_bounds__(256) k_rebase_nodes(uint4* __restrict__ nodes, uint32_t n8, uint32_t node_off, uint32_t tri_off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    uint4 r = nodes[5 * (size_t)i + 1];
    r.x += node_off;
    r.y += tri_off;
    nodes[5 * (size_t)i + 1] = r;
}

// Repack of a live handle (crt_instances_add_meshes / crt_instances_replace_meshes): node8 i of a BLAS region copied from
// src to dst, a SEPARATE array (the repack never moves a region inside the array it reads), with its child and triangle bases moved by
// the signed difference new offset - old offset, passed as its two's complement: unsigned wrap-around gives the right sum, since both the
// old and the new base are below 2^32.  A freshly built BLAS is the case old offset = 0.  One thread per 16-byte row: consecutive lanes
// read and write consecutive rows.
__global__ void __launch_bounds__(256) k_move_nodes(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t n8, uint32_t node_delta,
                                                    uint32_t tri_delta) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 5u * n8) return;                     // 5 n8 < 2^32: the packed array is below 4 GiB
    uint4 r = src[j];
    if (j % 5u == 1u) { r.x += node_delta; r.y += tri_delta; }
    dst[j] = r;
}

// the level order of a moved BLAS (global node indices): dst[i] = src[i] + delta, delta again a wrapped difference
__global__ void __launch_bounds__(256) k_move_order(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n, uint32_t delta) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dst[i] = src[i] + delta;
}

__global__ void k_single_leaf(const float* __restrict__ box, crt_flatnode* __restrict__ flat, uint32_t* __restrict__ tri_order) {
    if (threadIdx.x != 0) return;
    crt_flatnode f;
    for (int k = 0; k < 3; ++k) { f.bmin[k] = box[k]; f.bmax[k] = box[3 + k]; }
    f.bmin[3] = 0.f;        // first slot
    f.bmax[3] = 1.f;        // one primitive: a leaf
    flat[0] = f;
    tri_order[0] = 0u;
}

__global__ void __launch_bounds__(256) k_gather_instances(const float4* __restrict__ rec, const uint32_t* __restrict__ order, const int32_t* __restrict__ slots,
                                                          uint32_t n, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = order[slots[i]];
    for (int k = 0; k < 4; ++k) out[4 * (size_t)i + k] = rec[4 * (size_t)src + k];
}

// crt_instances_refit: each leaf slot of the live TLAS takes the new record of the instance it already holds (row 3 .y), in place
__global__ void __launch_bounds__(256) k_regather_instances(const float4* __restrict__ rec, uint32_t n, float4* __restrict__ inst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = __float_as_uint(inst[4 * (size_t)i + 3].y);
    if (src >= n) return;
    for (int k = 0; k < 4; ++k) inst[4 * (size_t)i + k] = rec[4 * (size_t)src + k];
}

// TLAS child masks, pass 1, one thread per live TLAS node8: its 8 bytes zeroed, and the link (node << 3 | meta slot) of each child
// written: to parent[] for an inner child, to leaf_of[] for every instance position a leaf slot holds.  The root's parent is ~0.
__global__ void __launch_bounds__(256) k_tlas_links(const uint4* __restrict__ nodes, uint32_t n8, uint32_t n, uint32_t* __restrict__ parent,
                                                    uint32_t* __restrict__ leaf_of, uint2* __restrict__ child_masks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const uint4 n0 = nodes[5 * (size_t)i], n1 = nodes[5 * (size_t)i + 1];
    child_masks[i] = make_uint2(0u, 0u);
    if (i == 0) parent[0] = 0xffffffffu;
    const uint32_t imask = n0.w >> 24;
    for (uint32_t slot = 0; slot < 8u; ++slot) {
        const uint32_t meta = ((slot < 4u ? n1.z : n1.w) >> (8u * (slot & 3u))) & 0xffu;
        const uint32_t link = (i << 3) | slot;
        if ((imask >> slot) & 1u) {
            // the walk's child index: child base + the inner slots below this one
            const uint32_t c = n1.x + (uint32_t)__builtin_popcount(imask & ((1u << slot) - 1u));
            if (c < n8) parent[c] = link;
        } else if (meta) {
            // a leaf slot: (meta >> 5) unary count of instance positions from triangle base + (meta & 31)
            const uint32_t first = n1.y + (meta & 0x1fu), cnt = (uint32_t)__builtin_popcount(meta >> 5);
            for (uint32_t k = 0; k < cnt; ++k)
                if (first + k < n) leaf_of[first + k] = link;
        }
    }
}

// TLAS child masks, pass 2, one thread per instance position: its mask ORed into the slot that holds it and up through its ancestors.
// Only the bits the OR newly set travel on: a bit already present was set by a thread that carries it up itself.
__global__ void __launch_bounds__(256) k_tlas_mask_up(const float4* __restrict__ inst, uint32_t n, uint32_t n8, const uint32_t* __restrict__ parent,
                                                      const uint32_t* __restrict__ leaf_of, uint32_t* __restrict__ words) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t m = __float_as_uint(inst[4 * (size_t)p + 3].w) & 0xffu;
    uint32_t link = leaf_of[p];
    for (uint32_t up = 0; m != 0u && link != 0xffffffffu && up < 64u; ++up) {      // 64: beyond any TLAS depth the stack admits
        const uint32_t node = link >> 3, sh = 8u * (link & 3u);
        if (node >= n8) break;
        const uint32_t old = atomicOr(words + 2u * node + ((link >> 2) & 1u), m << sh);
        m &= ~(old >> sh);
        link = parent[node];
    }
}

// the ray's mask against one TLAS node8's child masks: bit i set iff byte i of cm meets rmask (rmask <= 0xff)
__device__ __forceinline__ uint32_t child_keep(uint2 cm, uint32_t rmask) {
    const uint32_t r4 = rmask * 0x01010101u;
    uint32_t lo = cm.x & r4, hi = cm.y & r4;
    lo = (((lo & 0x7f7f7f7fu) + 0x7f7f7f7fu) | lo) & 0x80808080u;      // 0x80 in each non-zero byte, no carry between bytes
    hi = (((hi & 0x7f7f7f7fu) + 0x7f7f7f7fu) | hi) & 0x80808080u;
    // bits 0, 8, 16, 24 times 2^21 + 2^14 + 2^7 + 1 land on bits 21..24 without carries
    return ((((lo >> 7) * 0x00204081u) >> 21) & 0xfu) | (((((hi >> 7) * 0x00204081u) >> 21) & 0xfu) << 4);
}

// direction-dependent part of a walk's ray: octant and clamped reciprocal (traverse() / walk_pool's prologue)
__device__ __forceinline__ void ray_setup(vec3 d, vec3& inv, bool& negx, bool& negy, bool& negz, uint32_t& oct4) {
    const vec3 dc = V3(clamp_dir(d.x), clamp_dir(d.y), clamp_dir(d.z));
    negx = dc.x < 0.0f; negy = dc.y < 0.0f; negz = dc.z < 0.0f;
    oct4 = (negx ? 0u : 0x04040404u) | (negy ? 0u : 0x02020202u) | (negz ? 0u : 0x01010101u);
    inv = V3(rcp_ieee(dc.x), rcp_ieee(dc.y), rcp_ieee(dc.z));
}

// One lane per ray, pools of 64 rays per wave with lane refill (k_trace's mapping with crt_trace's default pool of 64: each 256-ray slot
// of the index space is walked by four single-wave workgroups), one loop and one LDS stack over both levels.  Stack entries: a node group (top byte set), the rest of a TLAS leaf (low 24 bits only) or the return marker (y == 0).
// MASK: the low 8 bits of the ray's pad word are its mask; a TLAS step culls the children whose child mask does not meet it, and the
// instance step skips an instance whose mask does not, before it transforms the ray.  Without MASK every such test folds away.
template <bool ANY, bool STATS, bool MASK>
__global__ void __launch_bounds__(64) k_trace_instances(std::conditional_t<MASK, InstMaskTraceArgs, InstTraceArgs> a) {
    extern __shared__ uint2 s_lds[];          // [level][lane] of the workgroup's one wave
    const WaveId wid = wave_id(false, false, 2u);
    const uint32_t lane = wid.lane;
    uint2* const stk = s_lds + lane;
    const int stack_entries = (int)a.stack_entries;
    CRT_CHUNK_LOOP(it) {
        const uint32_t v = static_pool_chunk<true>(wid, nullptr, a.n, it);
        if (v == CRT_NO_WORK) break;
        uint32_t next = dense_pool_first(v, wid.wave) + wid.sub * 64u;
        if (next >= a.n) continue;
        const uint32_t end = next + 64u < a.n ? next + 64u : a.n;
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
                        const float4 r0 = a.rays[2 * (size_t)idx], r1 = a.rays[2 * (size_t)idx + 1];
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
                    if constexpr (MASK) { if (nidx < a.n_tlas8) keep = child_keep(a.child_masks[nidx], rmask); }
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
                    const bool visible = !MASK || (__float_as_uint(w3.w) & rmask) != 0u;      // a hidden instance: skipped untransformed
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
                a.hits[idx] = h;
                if (a.inst_out) a.inst_out[idx] = hit ? best_inst : -1;
                if (STATS) a.stats[idx] = ((nt > 65535u ? 65535u : nt) << 16) | (nn > 65535u ? 65535u : nn);
                cur = make_uint2(0u, 0u); tg = make_uint2(0u, 0u); sp = 0; in_blas = false;
            }
        }
    }
}

static inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u)); }

void launch_instance_prep(const InstPrepArgs& a, hipStream_t stream) {
    if (a.n) hipLaunchKernelGGL(k_instance_prep, grid_for(a.n), dim3(256), 0, stream, a);
}
void launch_rebase_nodes(void* d_nodes, uint32_t n8, uint32_t node_off, uint32_t tri_off, hipStream_t stream) {
    if (n8) hipLaunchKernelGGL(k_rebase_nodes, grid_for(n8), dim3(256), 0, stream, static_cast<uint4*>(d_nodes), n8, node_off, tri_off);
}
void launch_move_nodes(const void* d_src, void* d_dst, uint32_t n8, uint32_t node_delta, uint32_t tri_delta, hipStream_t stream) {
    if (n8) hipLaunchKernelGGL(k_move_nodes, grid_for(5ull * n8), dim3(256), 0, stream, static_cast<const uint4*>(d_src), static_cast<uint4*>(d_dst), n8,
                               node_delta, tri_delta);
}
void launch_move_order(const uint32_t* d_src, uint32_t* d_dst, uint32_t n, uint32_t delta, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_move_order, grid_for(n), dim3(256), 0, stream, d_src, d_dst, n, delta);
}
void launch_single_leaf(const float* d_box, crt_flatnode* d_flat, uint32_t* d_tri_order, hipStream_t stream) {
    hipLaunchKernelGGL(k_single_leaf, dim3(1), dim3(64), 0, stream, d_box, d_flat, d_tri_order);
}
void launch_gather_instances(const float4* d_rec, const uint32_t* d_tri_order, const int32_t* d_tri_slots, uint32_t n, float4* d_out, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_gather_instances, grid_for(n), dim3(256), 0, stream, d_rec, d_tri_order, d_tri_slots, n, d_out);
}
void launch_regather_instances(const float4* d_rec, uint32_t n, float4* d_inst, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_regather_instances, grid_for(n), dim3(256), 0, stream, d_rec, n, d_inst);
}
void launch_tlas_child_masks(const void* d_nodes, uint32_t n8, const float4* d_inst, uint32_t n, uint32_t* d_parent, uint32_t* d_leaf_of,
                             uint2* d_child_masks, hipStream_t stream) {
    if (!n8 || !n) return;
    hipLaunchKernelGGL(k_tlas_links, grid_for(n8), dim3(256), 0, stream, static_cast<const uint4*>(d_nodes), n8, n, d_parent, d_leaf_of, d_child_masks);
    hipLaunchKernelGGL(k_tlas_mask_up, grid_for(n), dim3(256), 0, stream, d_inst, n, n8, d_parent, d_leaf_of, reinterpret_cast<uint32_t*>(d_child_masks));
}
template <bool MASK>
static void launch_trace_instances_t(const std::conditional_t<MASK, InstMaskTraceArgs, InstTraceArgs>& a, int any, bool stats, dim3 g, dim3 b, size_t lds,
                                     hipStream_t stream) {
    if (any) {
        if (stats) hipLaunchKernelGGL((k_trace_instances<true, true, MASK>), g, b, lds, stream, a);
        else       hipLaunchKernelGGL((k_trace_instances<true, false, MASK>), g, b, lds, stream, a);
    } else {
        if (stats) hipLaunchKernelGGL((k_trace_instances<false, true, MASK>), g, b, lds, stream, a);
        else       hipLaunchKernelGGL((k_trace_instances<false, false, MASK>), g, b, lds, stream, a);
    }
}
void launch_trace_instances(const InstMaskTraceArgs& a, int any, bool stats, bool mask, uint32_t chunks, hipStream_t stream) {
    const dim3 g(chunks * 16u), b(64);                      // sixteen single-wave workgroups per 1024-ray chunk: 64-ray pools (wave_id)
    const size_t lds = (size_t)a.stack_entries * 64 * sizeof(uint2);
    if (mask) launch_trace_instances_t<true>(a, any, stats, g, b, lds, stream);
    else      launch_trace_instances_t<false>(static_cast<const InstTraceArgs&>(a), any, stats, g, b, lds, stream);
}

// crt_warmup: load this translation unit's code object on the current device (device_build.hpp)
int warm_instance_kernels() {
    hipFuncAttributes at;
    hipError_t e;
    if ((e = hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_trace_instances<false, false, false>))) != hipSuccess) return (int)e;
    if ((e = hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_trace_instances<false, false, true>))) != hipSuccess) return (int)e;
    if ((e = hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_tlas_mask_up))) != hipSuccess) return (int)e;
    if ((e = hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_instance_prep))) != hipSuccess) return (int)e;
    return 0;
}

}  // namespace crt
