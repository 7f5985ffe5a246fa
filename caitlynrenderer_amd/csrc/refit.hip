// Refit kernels of crt_update_vertices: new vertex positions, same topology.  The BVH2, the CWBVH and both record arrays are
// rewritten in place from the new vertices, one launch per tree level, deepest first (the kernel boundary orders the levels,
// as in lbvh.hip k_refit_level).  Every box and quantised plane comes from host/refit_core.hpp, which the host refits
// (crt_bvh2_refit / crt_cwbvh_refit) use too: the device output is byte-identical to theirs.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_build.hpp"
#include "host/flatnode_link.hpp"
#include "host/refit_core.hpp"

namespace crt {
namespace {

using rf::Box;

// ordered key of a finite float: unsigned compare of keys == float compare (-0 below +0, as rf::tmin / tmax)
__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// out[0] |= 1 when a coordinate is not finite or exceeds 1e18 (crt_scene_create's rule); out[1..3] = max keys of x, y, z;
// out[4..6] = complemented min keys (so that one zeroing memset and atomicMax serve both)
__global__ void k_check_vertices(const float* __restrict__ v, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t bad = 0, hi[3] = {0u, 0u, 0u}, lo_c[3] = {0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        for (int k = 0; k < 3; ++k) {
            const float c = v[3 * (size_t)i + k];
            if (!(c <= 1.0e18f && c >= -1.0e18f)) { bad = 1u; continue; }
            const uint32_t key = order_key(c);
            hi[k] = max(hi[k], key);
            lo_c[k] = max(lo_c[k], ~key);
        }
    for (int m = 32; m >= 1; m >>= 1) {
        bad |= __shfl_xor(bad, m);
        for (int k = 0; k < 3; ++k) { hi[k] = max(hi[k], (uint32_t)__shfl_xor((int)hi[k], m)); lo_c[k] = max(lo_c[k], (uint32_t)__shfl_xor((int)lo_c[k], m)); }
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (bad) atomicOr(out, 1u);
        for (int k = 0; k < 3; ++k) { atomicMax(out + 1 + k, hi[k]); atomicMax(out + 4 + k, lo_c[k]); }
    }
}

// ---- level discovery (once per scene, at its first update) ----
__global__ void k_node8_parents(const uint4* __restrict__ nodes, uint32_t node_rows, uint32_t n8, int32_t* __restrict__ parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const uint4 r0 = nodes[(size_t)i * node_rows], r1 = nodes[(size_t)i * node_rows + 1];
    const uint32_t imask = r0.w >> 24;
    for (uint32_t s = 0, rank = 0; s < 8; ++s)
        if ((imask >> s) & 1u) {
            const uint32_t c = r1.x + rank++;
            if (c < n8) parent[c] = (int32_t)i;
        }
}
__global__ void k_bvh2_parents(const crt_flatnode* __restrict__ flat, uint32_t n2, int32_t* __restrict__ parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    const crt_flatnode f = flat[i];
    if (f.bmax[3] != 0.0f) return;
    const uint32_t l = (uint32_t)link_of(f.bmin[3]);
    if (l > i && l + 1u < n2) { parent[l] = (int32_t)i; parent[l + 1u] = (int32_t)i; }
}
// depth of every node by climbing its parent links (root = 0; at most 255 levels, both trees are far shallower)
__global__ void k_depths(const int32_t* __restrict__ parent, uint32_t n, uint8_t* __restrict__ depth) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d = 0;
    for (int32_t p = parent[i]; p >= 0 && d < 255u; p = parent[p]) ++d;
    depth[i] = (uint8_t)d;
}

// ---- per update ----
// records: rows (v0 | id) (e1 | slot) (e2 | material) regathered from the slot in e1.w and the leaf-order triangle array, with the two
// fp32 subtractions of scene_build.hip make_record; the w words stay.  slot_order: record i is slot i (the BVH2 walk's array).
__global__ void k_refit_records(float4* __restrict__ recs, uint32_t rows, uint32_t n, const int4* __restrict__ tris, uint32_t n_slots,
                                const float* __restrict__ verts, int slot_order) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4* r = recs + (size_t)i * rows;
    float4 a = r[0], b = r[1], c = r[2];
    const uint32_t slot = slot_order ? i : (uint32_t)__float_as_int(b.w);
    if (slot >= n_slots) return;
    const int4 t = tris[3 * (size_t)slot];
    const float* v0 = verts + 3 * (size_t)(uint32_t)t.x;
    const float* v1 = verts + 3 * (size_t)(uint32_t)t.y;
    const float* v2 = verts + 3 * (size_t)(uint32_t)t.z;
    a.x = v0[0]; a.y = v0[1]; a.z = v0[2];
    b.x = v1[0] - v0[0]; b.y = v1[1] - v0[1]; b.z = v1[2] - v0[2];
    c.x = v2[0] - v0[0]; c.y = v2[1] - v0[1]; c.z = v2[2] - v0[2];
    r[0] = a; r[1] = b; r[2] = c;
}

// one BVH2 level: leaves from their slot ranges, inner nodes from their two children (the deeper level, final by now)
__global__ void k_refit_bvh2_level(crt_flatnode* __restrict__ flat, uint32_t n2, const uint32_t* __restrict__ order, uint32_t count,
                                   const int4* __restrict__ tris, uint32_t n_slots, const float* __restrict__ verts) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint32_t i = order[j];
    crt_flatnode f = flat[i];
    const uint32_t a = (uint32_t)link_of(f.bmin[3]);
    Box b = rf::empty_box();
    if (f.bmax[3] != 0.0f) {
        const uint32_t end = min(a + (uint32_t)f.bmax[3], n_slots);
        for (uint32_t s = a; s < end; ++s) {
            const int4 t = tris[3 * (size_t)s];
            const int32_t v[3] = {t.x, t.y, t.z};
            rf::grow_triangle(b, v, verts);
        }
    } else if (a + 1u < n2) {
        const crt_flatnode l = flat[a], r = flat[a + 1u];
        for (int k = 0; k < 3; ++k) { b.lo[k] = rf::tmin(l.bmin[k], r.bmin[k]); b.hi[k] = rf::tmax(l.bmax[k], r.bmax[k]); }
    }
    for (int k = 0; k < 3; ++k) { f.bmin[k] = b.lo[k]; f.bmax[k] = b.hi[k]; }
    flat[i] = f;
}

// lane ^ 1, ^ 2, ^ 4 inside groups of 8 lanes (ds_swizzle bit-mask mode: and 0x1f, or 0, xor m)
template <int XOR>
__device__ __forceinline__ float swz(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1f | (XOR << 10))); }

constexpr uint32_t kNodesPerBlock = 32;      // 8 lanes per node8, 256 threads

// one node8 level: eight adjacent lanes per node, one per slot.  A lane builds its slot's box (leaf: the vertex boxes of its triangles;
// inner: the child node8's float box, written by the previous launch), the node box is reduced across the eight lanes, and every lane
// quantises its own slot against it.  meta, imask, child and triangle bases stay; so do the planes of empty slots.
__global__ __launch_bounds__(256) void k_refit_node8_level(uint4* __restrict__ nodes, uint32_t node_rows, uint32_t n8, const uint32_t* __restrict__ order,
                                                           uint32_t count, const float4* __restrict__ recs, uint32_t tri_rows, uint32_t n_tris8,
                                                           const int4* __restrict__ tris, uint32_t n_slots, const float* __restrict__ verts,
                                                           float2* __restrict__ box8) {
    __shared__ uint4 q_rows[kNodesPerBlock][3];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 3, s = t & 7u, local = threadIdx.x >> 3;
    const bool valid = j < count;
    const uint32_t node = valid ? order[j] : 0u;
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    if (valid) { r0 = nodes[(size_t)node * node_rows]; r1 = nodes[(size_t)node * node_rows + 1]; }
    if (valid && s < 3u) q_rows[local][s] = nodes[(size_t)node * node_rows + 2u + s];
    const uint32_t imask = r0.w >> 24;
    const uint8_t meta = (uint8_t)(((s < 4u ? r1.z : r1.w) >> (8u * (s & 3u))) & 0xffu);
    Box b = rf::empty_box();
    if (valid && meta) {
        if ((imask >> s) & 1u) {
            const uint32_t c = r1.x + (uint32_t)__builtin_popcount(imask & ((1u << s) - 1u));
            if (c < n8) {
                const float2 x0 = box8[3 * (size_t)c], x1 = box8[3 * (size_t)c + 1], x2 = box8[3 * (size_t)c + 2];
                b = Box{{x0.x, x0.y, x1.x}, {x1.y, x2.x, x2.y}};
            }
        } else {
            const uint32_t first = r1.y + (uint32_t)rf::leaf_offset(meta), cnt = (uint32_t)rf::leaf_count(meta);
            for (uint32_t k = 0; k < cnt; ++k) {
                if (first + k >= n_tris8) break;
                const uint32_t slot = (uint32_t)__float_as_int(recs[(size_t)(first + k) * tri_rows + 1].w);
                if (slot >= n_slots) continue;
                const int4 tr = tris[3 * (size_t)slot];
                const int32_t v[3] = {tr.x, tr.y, tr.z};
                rf::grow_triangle(b, v, verts);
            }
        }
    }
    Box u = b;
    for (int k = 0; k < 3; ++k) { u.lo[k] = rf::tmin(u.lo[k], swz<1>(u.lo[k])); u.hi[k] = rf::tmax(u.hi[k], swz<1>(u.hi[k])); }
    for (int k = 0; k < 3; ++k) { u.lo[k] = rf::tmin(u.lo[k], swz<2>(u.lo[k])); u.hi[k] = rf::tmax(u.hi[k], swz<2>(u.hi[k])); }
    for (int k = 0; k < 3; ++k) { u.lo[k] = rf::tmin(u.lo[k], swz<4>(u.lo[k])); u.hi[k] = rf::tmax(u.hi[k], swz<4>(u.hi[k])); }
    float p[3], scale[3];
    uint8_t e[3];
    rf::node_frame(u, p, e, scale);
    __syncthreads();                                  // the original plane rows are in LDS
    if (valid && meta) {
        uint8_t q[6];
        rf::quantise_slot(b, p, scale, q);
        uint8_t* row = reinterpret_cast<uint8_t*>(&q_rows[local][0]);
        for (int k = 0; k < 3; ++k) { row[16 * k + s] = q[2 * k]; row[16 * k + 8 + s] = q[2 * k + 1]; }
    }
    __syncthreads();
    if (!valid) return;
    uint4* dst = nodes + (size_t)node * node_rows;
    if (s < 3u) dst[2u + s] = q_rows[local][s];
    if (s == 0u) {
        dst[0] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]),
                            (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | (imask << 24));
        box8[3 * (size_t)node] = make_float2(u.lo[0], u.lo[1]);
        box8[3 * (size_t)node + 1] = make_float2(u.lo[2], u.hi[0]);
        box8[3 * (size_t)node + 2] = make_float2(u.hi[1], u.hi[2]);
    }
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u ? (n + 255u) / 256u : 1u)); }

}  // namespace

void launch_check_vertices(const float* d_verts, uint32_t n_vertices, uint32_t* d_out, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024u, (n_vertices + 255u) / 256u + 1u);
    hipLaunchKernelGGL(k_check_vertices, dim3(blocks), dim3(256), 0, stream, d_verts, n_vertices, d_out);
}
void launch_node8_parents(const void* d_nodes, uint32_t node_rows, uint32_t n8, int32_t* d_parent, hipStream_t stream) {
    hipLaunchKernelGGL(k_node8_parents, grid_for(n8), dim3(256), 0, stream, static_cast<const uint4*>(d_nodes), node_rows, n8, d_parent);
}
void launch_bvh2_parents(const void* d_flat, uint32_t n2, int32_t* d_parent, hipStream_t stream) {
    hipLaunchKernelGGL(k_bvh2_parents, grid_for(n2), dim3(256), 0, stream, static_cast<const crt_flatnode*>(d_flat), n2, d_parent);
}
void launch_depths(const int32_t* d_parent, uint32_t n, uint8_t* d_depth, hipStream_t stream) {
    hipLaunchKernelGGL(k_depths, grid_for(n), dim3(256), 0, stream, d_parent, n, d_depth);
}
void launch_refit_records(void* d_recs, uint32_t rows, uint32_t n, const void* d_tris, uint32_t n_slots, const float* d_verts, int slot_order,
                          hipStream_t stream) {
    hipLaunchKernelGGL(k_refit_records, grid_for(n), dim3(256), 0, stream, static_cast<float4*>(d_recs), rows, n, static_cast<const int4*>(d_tris), n_slots,
                       d_verts, slot_order);
}
void launch_refit_bvh2_level(void* d_flat, uint32_t n2, const uint32_t* d_order, uint32_t count, const void* d_tris, uint32_t n_slots,
                             const float* d_verts, hipStream_t stream) {
    hipLaunchKernelGGL(k_refit_bvh2_level, grid_for(count), dim3(256), 0, stream, static_cast<crt_flatnode*>(d_flat), n2, d_order, count,
                       static_cast<const int4*>(d_tris), n_slots, d_verts);
}
void launch_refit_node8_level(void* d_nodes, uint32_t node_rows, uint32_t n8, const uint32_t* d_order, uint32_t count, const void* d_recs,
                              uint32_t tri_rows, uint32_t n_tris8, const void* d_tris, uint32_t n_slots, const float* d_verts, float* d_box8,
                              hipStream_t stream) {
    hipLaunchKernelGGL(k_refit_node8_level, grid_for((uint64_t)count * 8u), dim3(256), 0, stream, static_cast<uint4*>(d_nodes), node_rows, n8, d_order,
                       count, static_cast<const float4*>(d_recs), tri_rows, n_tris8, static_cast<const int4*>(d_tris), n_slots, d_verts,
                       reinterpret_cast<float2*>(d_box8));
}

}  // namespace crt
