// HIP kernels of instanced scenes (include/crt.h crt_instances_*): per-instance preparation (validation, inverse, world
// box, record), the packing of the BLASes into one node array, and the kernels of the two-level walk (instances_walk.hpp,
// instances_walk_loop.hpp): k_trace_instances for explicit rays, k_closest_instances_queue and k_shadow_instances_deferred for the frames
// of an instanced scene, each also in a masked form that culls by one ray mask per launch (§17), and the check of
// per-instance material offsets against a bound scene's material table (§17).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#define CRT_AO_DEVICE_MATH 1      // ao.hpp: the generator of the occlusion rays, in device code
#include "ao.hpp"
#define CRT_FOG_DEVICE_MATH 1     // fog.hpp: the generator of the fog's shadow rays, in device code
#include "fog.hpp"
#include "instances.hpp"
#include "instances_walk.hpp"
#include "rt_kernels.hpp"
#include "rt_math.hpp"
#include "rt_traverse.hpp"
#include "host/instance_math.hpp"
#define CRT_LIGHT_DEVICE_MATH 1      // light_math.hpp: sqrt_ieee / rcp_ieee of rt_math.hpp in device code
#include "host/light_math.hpp"

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
    a.mesh_of[i] = make_uint2(mesh | (instance_is_identity(m) ? 0x80000000u : 0u), src[14]);
    for (int k = 0; k < 12; ++k) a.o2w[12 * (size_t)i + k] = m[k];
}

// A bound scene's rule for material offsets (include/crt.h crt_scene_create_instanced) against (mesh, offset) words: those a
// set or refit has staged, or the live ones at a scene's create.  Offset 0 is exempt.  A mesh index out of range is k_instance_prep's to
// refuse (it has then written no word for that instance: what lies there is stale).
__global__ void __launch_bounds__(256) k_instance_offsets(InstOffsetCheckArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint2 w = a.mesh_of[i];
    const uint32_t mesh = w.x & 0x7fffffffu, off = w.y;
    if (off == 0u || mesh >= a.n_meshes) return;
    const uint4 mm = a.rule.mesh_mtl[mesh];          // lo, hi (< n_materials), vt_ok
    uint32_t bad = 0u;
    if (off >= 0x80000000u || mm.y + off >= a.rule.n_materials) bad = 8u;      // hi + off < 2^32: no wrap
    else if (mm.z == 0u && a.rule.tex_before[mm.y + off + 1u] != a.rule.tex_before[mm.x + off]) bad = 16u;
    if (bad) { atomicOr(a.flag, bad); atomicMin(a.flag + 1, i); }
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

// ---- the world light table of a scene with mesh lights (crt_scene_create_instanced_lit) ----

// Scan, pass 1: 1024 instances per block, four consecutive ones per thread.  first[i] = the lights of the block's instances before i,
// block_sums[block] = the block's lights.
__global__ void __launch_bounds__(256) k_light_counts(LightTableArgs a) {
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, i0 = blockIdx.x * 1024u + 4u * t;
    uint32_t c[4], mine = 0u;
    for (uint32_t k = 0; k < 4u; ++k) {
        c[k] = 0u;
        if (i0 + k < a.n_instances) {
            const uint32_t mesh = a.mesh_of[i0 + k].x & 0x7fffffffu;
            if (mesh < a.n_meshes) c[k] = a.mesh_lights[mesh].y;
        }
        mine += c[k];
    }
    uint32_t incl = mine;                                     // inclusive scan over the wave, then over the block's four waves
    const uint32_t lane = t & 63u, wave = t >> 6;
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) before += s_wave[w]; all += s_wave[w]; }
    uint32_t run = before + incl - mine;
    for (uint32_t k = 0; k < 4u; ++k) {
        if (i0 + k < a.n_instances) a.first[i0 + k] = run;
        run += c[k];
    }
    if (t == 0u) a.block_sums[blockIdx.x] = all;
}

// Scan, pass 2, ONE block: block_sums[] -> their exclusive prefix sums in place, total[0] = the sum of all
__global__ void __launch_bounds__(256) k_light_block_scan(uint32_t* __restrict__ block_sums, uint32_t n_blocks, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < n_blocks; base += 256u) {
        const uint32_t mine = base + t < n_blocks ? block_sums[base + t] : 0u;
        uint32_t incl = mine;
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        __syncthreads();                                      // the previous round's s_wave has been read
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (uint32_t w = 0; w < 4u; ++w) { if (w < wave) before += s_wave[w]; all += s_wave[w]; }
        if (base + t < n_blocks) block_sums[base + t] = carry + before + incl - mine;
        carry += all;
    }
    if (t == 0u) total[0] = carry;
}

// Scan, pass 3: first[i] += its block's prefix + n_static
__global__ void __launch_bounds__(256) k_light_first(LightTableArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_instances) return;
    a.first[i] += a.block_sums[i >> 10] + a.n_static;
}

// One lane per light of the table.  A static light is copied; any other finds its instance by binary search in first[] (the LAST
// instance whose first light is at or before it: instances without lights repeat their successor's value and are never the last) and
// is its mesh's object-space light through that instance's live matrices (light_math.hpp).  Lane-per-light, not wave-per-instance: the
// work per lane is the same whatever the meshes' light counts, and the 18 steps of a search at 256 k instances read a 1 MB array that
// stays in L2 — less than the 72 B it then writes.
__global__ void __launch_bounds__(256) k_light_transform(LightTableArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n_total) return;
    float* out = a.table + 18 * (size_t)k;
    if (k < a.n_static) {
        for (int j = 0; j < 18; ++j) out[j] = a.static_lights[18 * (size_t)k + j];
        return;
    }
    uint32_t lo = 0u, hi = a.n_instances;                     // first[lo] <= k < first[hi] (first[n] = n_total)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.first[mid] <= k) lo = mid; else hi = mid;
    }
    const uint32_t word = a.mesh_of[lo].x, mesh = word & 0x7fffffffu;
    const uint32_t j = k - a.first[lo];
    float in[18], res[18];
    bool ok = mesh < a.n_meshes;
    uint2 ml = make_uint2(0u, 0u);
    if (ok) { ml = a.mesh_lights[mesh]; ok = j < ml.y; }
    if (!ok) {                                                // cannot happen while first[] and the live words agree: leave a dark light
        for (int q = 0; q < 18; ++q) out[q] = 0.0f;
        return;
    }
    const float* src = a.obj_lights + 18 * ((size_t)ml.x + j);
    for (int q = 0; q < 18; ++q) in[q] = src[q];
    float A[12], W[12];
    for (int q = 0; q < 12; ++q) { A[q] = a.o2w[12 * (size_t)lo + q]; W[q] = a.w2o[12 * (size_t)lo + q]; }
    light_to_world(A, W, (word & 0x80000000u) != 0u, in, res);
    for (int q = 0; q < 18; ++q) out[q] = res[q];
}

// The pairwise tree sum (include/crt.h): each block leaves the tree sum of an aligned chunk of 256 values (missing ones +0) — lane
// offsets 1, 2, 4 .. 32 inside a wave, then the four waves pairwise — so that a further pass over the partials continues the same tree.
// AREAS: the values are the area terms of the table's lights; else plain floats.
template <bool AREAS>
__global__ void __launch_bounds__(256) k_light_tree_sum(const float* __restrict__ src, uint32_t n, float* __restrict__ dst) {
    __shared__ float s_wave[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float v = 0.0f;
    if (i < n) v = AREAS ? light_area_term(src[18 * (size_t)i + 15]) : src[i];
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0u) dst[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ void __launch_bounds__(256) k_light_pdf(float* __restrict__ table, uint32_t n, const float* __restrict__ sum) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    table[18 * (size_t)i + 16] = light_pdf(light_area_term(table[18 * (size_t)i + 15]), sum[0]);
}

// One lane per ray, pools of 64 rays per wave with lane refill (k_trace's mapping with crt_trace's default pool of 64: each 256-ray slot
// of the index space is walked by four single-wave workgroups); the walk itself is instances_walk_loop.hpp.
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
#define CRT_WALK_LOAD(idx, r0, r1) const float4 r0 = a.rays[2 * (size_t)idx], r1 = a.rays[2 * (size_t)idx + 1];
#define CRT_WALK_DONE(idx, h, hit, inst, nn, nt)                \
            a.hits[idx] = h;                                    \
            if (a.inst_out) a.inst_out[idx] = hit ? inst : -1;  \
            if (STATS) a.stats[idx] = ((nt > 65535u ? 65535u : nt) << 16) | (nn > 65535u ? 65535u : nn);
#define CRT_WALK_MASK(lane_mask) (lane_mask)
#include "instances_walk_loop.hpp"
#undef CRT_WALK_LOAD
#undef CRT_WALK_DONE
#undef CRT_WALK_MASK
    }
}

// ---- the frame path of an instanced scene (crt_scene_create_instanced) ----

// a wave's visit counts into the frame's totals: [0] += node steps, [1] += triangle tests
__device__ __forceinline__ void flush_inst_totals(unsigned long long* totals, uint32_t nn, uint32_t nt) {
    for (int off = 32; off > 0; off >>= 1) { nn += __shfl_down(nn, off); nt += __shfl_down(nt, off); }
    if ((threadIdx.x & 63u) == 0u) {
        if (nn) atomicAdd(totals, (unsigned long long)nn);
        if (nt) atomicAdd(totals + 1, (unsigned long long)nt);
    }
}

// the ray mask of a masked frame launch: a kernel argument, the same in every lane (the unmasked argument blocks have none: never called)
__device__ __forceinline__ uint32_t launch_mask(const InstMaskQueueArgs& a) { return a.ray_mask; }
__device__ __forceinline__ uint32_t launch_mask(const InstMaskShadowArgs& a) { return a.ray_mask; }
__device__ __forceinline__ uint32_t launch_mask(const InstQueueArgs&) { return 0u; }
__device__ __forceinline__ uint32_t launch_mask(const InstShadowArgs&) { return 0u; }
__device__ __forceinline__ uint32_t launch_mask(const InstMaskAoArgs& a) { return a.ray_mask; }
__device__ __forceinline__ uint32_t launch_mask(const InstAoArgs&) { return 0u; }
__device__ __forceinline__ uint32_t launch_mask(const InstMaskFogArgs& a) { return a.ray_mask; }
__device__ __forceinline__ uint32_t launch_mask(const InstFogArgs&) { return 0u; }

// Closest hits of a segment's path-ray queue: workgroup (g, c) = one wave walks entries [64 c, 64 c + 64) of sub-queue g, as far as its
// device-side count goes; hits and hit instances go to buffers parallel to the queue, and k_segment<PRETRACED, INST> shades them.
// MASK: the walk culls by a.ray_mask, one mask for the launch.
template <bool STATS, bool MASK>
__global__ void __launch_bounds__(64) k_closest_instances_queue(std::conditional_t<MASK, InstMaskQueueArgs, InstQueueArgs> a) {
    extern __shared__ uint2 s_lds[];          // [level][lane] of the workgroup's one wave
    constexpr bool ANY = false;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x & 7u, c = blockIdx.x >> 3;
    const uint32_t cnt = a.count[g * CRT_COUNTER_STRIDE], n = cnt < a.sub_capacity ? cnt : a.sub_capacity;
    if (c * 64u >= n) return;
    uint32_t next = g * a.sub_capacity + c * 64u;
    const uint32_t end = g * a.sub_capacity + (c * 64u + 64u < n ? c * 64u + 64u : n);
    uint2* const stk = s_lds + lane;
    const int stack_entries = (int)a.stack_entries;
    uint32_t tn = 0, tt = 0;
#define CRT_WALK_LOAD(idx, r0, r1) const float4 r0 = a.rays[2 * (size_t)idx], r1 = a.rays[2 * (size_t)idx + 1];
#define CRT_WALK_DONE(idx, h, hit, inst, nn, nt) \
            a.hits[idx] = h;                     \
            a.hit_inst[idx] = hit ? inst : -1;   \
            if (STATS) { tn += nn; tt += nt; }
#define CRT_WALK_MASK(lane_mask) ((void)(lane_mask), launch_mask(a))
#include "instances_walk_loop.hpp"
#undef CRT_WALK_LOAD
#undef CRT_WALK_DONE
#undef CRT_WALK_MASK
    if (STATS) flush_inst_totals(a.visit_totals, tn, tt);
}

// The frame's deferred NEE shadow rays (k_shadow_deferred's queue layout: region r = segment, 8 sub-queues each, entry = (o, tmax)
// (d, contribution slot)): workgroup (g, r, c) walks 64 entries; an OCCLUDED ray clears the visibility word of its contribution slot.
template <bool STATS, bool MASK>
__global__ void __launch_bounds__(64) k_shadow_instances_deferred(std::conditional_t<MASK, InstMaskShadowArgs, InstShadowArgs> a) {
    extern __shared__ uint2 s_lds[];
    constexpr bool ANY = true;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x & 7u, q = blockIdx.x >> 3;
    const uint32_t r = q / a.pools_per_region, c = q - r * a.pools_per_region;
    if (r >= a.n_regions) return;
    const uint32_t cnt = a.count[(size_t)r * a.count_stride + g * CRT_COUNTER_STRIDE], n = cnt < a.sub_capacity ? cnt : a.sub_capacity;
    if (c * 64u >= n) return;
    const uint32_t qb = (r * 8u + g) * a.sub_capacity;
    uint32_t next = qb + c * 64u;
    const uint32_t end = qb + (c * 64u + 64u < n ? c * 64u + 64u : n);
    uint2* const stk = s_lds + lane;
    const int stack_entries = (int)a.stack_entries;
    uint32_t tn = 0, tt = 0;
#define CRT_WALK_LOAD(idx, r0, r1) const float4 r0 = a.shadow[2 * (size_t)idx], r1 = a.shadow[2 * (size_t)idx + 1];
#define CRT_WALK_DONE(idx, h, hit, inst, nn, nt)                                              \
            if (hit) {                                                                        \
                const uint32_t slot = __float_as_uint(a.shadow[2 * (size_t)idx + 1].w);       \
                if (slot < a.n_slots) reinterpret_cast<float*>(a.contrib + slot)[3] = 0.0f;   \
            }                                                                                 \
            if (STATS) { tn += nn; tt += nt; }
#define CRT_WALK_MASK(lane_mask) ((void)(lane_mask), launch_mask(a))
#include "instances_walk_loop.hpp"
#undef CRT_WALK_LOAD
#undef CRT_WALK_DONE
#undef CRT_WALK_MASK
    if (STATS) flush_inst_totals(a.visit_totals, tn, tt);
}

// The occlusion rays of an instanced scene's AO points (ao.hpp): workgroup c = one wave walks entries [64 c, 64 c + 64) of
// the index space [0, n K); the ray of an entry is built where it is loaded and never stored, an UNoccluded ray sets its bit of its point's
// visibility words.  A point without rays loads a ray whose origin is not finite, which the walk finishes as a miss at once.
// MASK: the walk culls by a.ray_mask (the scene's "mask_shadow").
template <bool MASK>
__global__ void __launch_bounds__(64) k_ao_walk_instances(std::conditional_t<MASK, InstMaskAoArgs, InstAoArgs> a) {
    extern __shared__ uint2 s_lds[];
    constexpr bool ANY = true, STATS = false;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t total = a.g.n * a.g.K;
    const uint64_t first64 = (uint64_t)blockIdx.x * 64u;
    if (first64 >= total) return;
    uint32_t next = (uint32_t)first64;
    const uint32_t end = total - next < 64u ? total : next + 64u;
    uint2* const stk = s_lds + lane;
    const int stack_entries = (int)a.stack_entries;
#define CRT_WALK_LOAD(idx, r0, r1)                                                         \
            float4 r0 = make_float4(__builtin_nanf(""), 0.f, 0.f, a.g.radius), r1 = make_float4(0.f, 0.f, 1.f, 0.f); \
            {                                                                              \
                vec3 ao_o, ao_d;                                                           \
                if (ao_ray(a.g, idx, ao_o, ao_d)) {                                        \
                    r0 = make_float4(ao_o.x, ao_o.y, ao_o.z, a.g.radius);                  \
                    r1 = make_float4(ao_d.x, ao_d.y, ao_d.z, 0.f);                         \
                }                                                                          \
            }
#define CRT_WALK_DONE(idx, h, hit, inst, nn, nt) (void)(nn); (void)(nt); if (!hit) ao_mark_visible(a.g, a.vis, idx);
#define CRT_WALK_MASK(lane_mask) ((void)(lane_mask), launch_mask(a))
#include "instances_walk_loop.hpp"
#undef CRT_WALK_LOAD
#undef CRT_WALK_DONE
#undef CRT_WALK_MASK
}

// The shadow rays of an instanced scene's fog (fog.hpp): k_ao_walk_instances' form over the index space [0, n K); the ray
// of an entry is built where it is loaded and never stored, an UNoccluded ray sets its bit of its segment's visibility words.  An entry
// without a ray (a dark sample, a segment without rays) loads a ray whose origin is not finite, which the walk finishes as a miss at once:
// the fold never counts its bit.  MASK: the walk culls by a.ray_mask (the scene's "mask_shadow").
template <bool MASK>
__global__ void __launch_bounds__(64) k_fog_walk_instances(std::conditional_t<MASK, InstMaskFogArgs, InstFogArgs> a) {
    extern __shared__ uint2 s_lds[];
    constexpr bool ANY = true, STATS = false;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t total = a.g.n * a.g.K;
    const uint64_t first64 = (uint64_t)blockIdx.x * 64u;
    if (first64 >= total) return;
    uint32_t next = (uint32_t)first64;
    const uint32_t end = total - next < 64u ? total : next + 64u;
    uint2* const stk = s_lds + lane;
    const int stack_entries = (int)a.stack_entries;
#define CRT_WALK_LOAD(idx, r0, r1)                                                         \
            float4 r0 = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, 1.f, 0.f); \
            {                                                                              \
                vec3 fog_o, fog_d;                                                         \
                float fog_tmax;                                                            \
                if (fog_ray(a.g, idx, fog_o, fog_d, fog_tmax)) {                           \
                    r0 = make_float4(fog_o.x, fog_o.y, fog_o.z, fog_tmax);                 \
                    r1 = make_float4(fog_d.x, fog_d.y, fog_d.z, 0.f);                      \
                }                                                                          \
            }
#define CRT_WALK_DONE(idx, h, hit, inst, nn, nt) (void)(nn); (void)(nt); if (!hit) fog_mark_visible(a.g, a.vis, idx);
#define CRT_WALK_MASK(lane_mask) ((void)(lane_mask), launch_mask(a))
#include "instances_walk_loop.hpp"
#undef CRT_WALK_LOAD
#undef CRT_WALK_DONE
#undef CRT_WALK_MASK
}

static inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u)); }

void launch_instance_prep(const InstPrepArgs& a, hipStream_t stream) {
    if (a.n) hipLaunchKernelGGL(k_instance_prep, grid_for(a.n), dim3(256), 0, stream, a);
}
void launch_light_scan(const LightTableArgs& a, hipStream_t stream) {
    const uint32_t blocks = (a.n_instances + 1023u) / 1024u;
    if (a.n_instances) hipLaunchKernelGGL(k_light_counts, dim3(blocks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_light_block_scan, dim3(1), dim3(256), 0, stream, a.block_sums, blocks, a.total);
    if (a.n_instances) hipLaunchKernelGGL(k_light_first, grid_for(a.n_instances), dim3(256), 0, stream, a);
}
void launch_light_table(const LightTableArgs& a, hipStream_t stream) {
    if (!a.n_total) return;
    hipLaunchKernelGGL(k_light_transform, grid_for(a.n_total), dim3(256), 0, stream, a);
    // the tree sum: passes of 256 until one value is left, alternating between the two regions of a.partial
    uint32_t n = a.n_total;
    const uint32_t region = (a.n_total + 255u) / 256u;
    float* dst = a.partial;
    hipLaunchKernelGGL((k_light_tree_sum<true>), grid_for(n), dim3(256), 0, stream, a.table, n, dst);
    n = (n + 255u) / 256u;
    while (n > 1u) {
        float* next = dst == a.partial ? a.partial + region : a.partial;
        hipLaunchKernelGGL((k_light_tree_sum<false>), grid_for(n), dim3(256), 0, stream, dst, n, next);
        dst = next;
        n = (n + 255u) / 256u;
    }
    hipLaunchKernelGGL(k_light_pdf, grid_for(a.n_total), dim3(256), 0, stream, a.table, a.n_total, dst);
}
void launch_instance_offsets(const InstOffsetCheckArgs& a, hipStream_t stream) {
    if (a.n) hipLaunchKernelGGL(k_instance_offsets, grid_for(a.n), dim3(256), 0, stream, a);
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

void launch_closest_instances_queue(const InstMaskQueueArgs& a, bool stats, bool mask, hipStream_t stream) {
    const dim3 g(8u * ((a.sub_capacity + 63u) / 64u)), b(64);
    const size_t lds = (size_t)a.stack_entries * 64 * sizeof(uint2);
    const InstQueueArgs& u = a;
    if (mask) {
        if (stats) hipLaunchKernelGGL((k_closest_instances_queue<true, true>), g, b, lds, stream, a);
        else       hipLaunchKernelGGL((k_closest_instances_queue<false, true>), g, b, lds, stream, a);
    } else {
        if (stats) hipLaunchKernelGGL((k_closest_instances_queue<true, false>), g, b, lds, stream, u);
        else       hipLaunchKernelGGL((k_closest_instances_queue<false, false>), g, b, lds, stream, u);
    }
}
void launch_shadow_instances_deferred(const InstMaskShadowArgs& a, bool stats, bool mask, hipStream_t stream) {
    const dim3 g(8u * a.n_regions * a.pools_per_region), b(64);
    const size_t lds = (size_t)a.stack_entries * 64 * sizeof(uint2);
    const InstShadowArgs& u = a;
    if (mask) {
        if (stats) hipLaunchKernelGGL((k_shadow_instances_deferred<true, true>), g, b, lds, stream, a);
        else       hipLaunchKernelGGL((k_shadow_instances_deferred<false, true>), g, b, lds, stream, a);
    } else {
        if (stats) hipLaunchKernelGGL((k_shadow_instances_deferred<true, false>), g, b, lds, stream, u);
        else       hipLaunchKernelGGL((k_shadow_instances_deferred<false, false>), g, b, lds, stream, u);
    }
}

void launch_fog_walk_instances(const InstMaskFogArgs& a, bool mask, hipStream_t stream) {
    const uint64_t total = (uint64_t)a.g.n * a.g.K;
    if (!total) return;
    const dim3 g((uint32_t)((total + 63u) / 64u)), b(64);
    const size_t lds = (size_t)a.stack_entries * 64 * sizeof(uint2);
    const InstFogArgs& u = a;
    if (mask) hipLaunchKernelGGL((k_fog_walk_instances<true>), g, b, lds, stream, a);
    else      hipLaunchKernelGGL((k_fog_walk_instances<false>), g, b, lds, stream, u);
}

void launch_ao_walk_instances(const InstMaskAoArgs& a, bool mask, hipStream_t stream) {
    const uint64_t total = (uint64_t)a.g.n * a.g.K;
    if (!total) return;
    const dim3 g((uint32_t)((total + 63u) / 64u)), b(64);
    const size_t lds = (size_t)a.stack_entries * 64 * sizeof(uint2);
    const InstAoArgs& u = a;
    if (mask) hipLaunchKernelGGL((k_ao_walk_instances<true>), g, b, lds, stream, a);
    else      hipLaunchKernelGGL((k_ao_walk_instances<false>), g, b, lds, stream, u);
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
