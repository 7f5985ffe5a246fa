// Refit kernels of crt_instances_update_meshes (include/crt.h): new vertex positions for some meshes of an updatable
// instanced scene, same topology.  Every kernel covers ALL meshes of the call in one launch: a small per-call table maps a block (check)
// or an entry (records, node8 levels) to its mesh by a binary search over cumulative starts.  The per-node arithmetic is
// host/refit_core.hpp's, as in refit.hip, so a refitted BLAS is byte-identical to the host crt_cwbvh_refit of it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "host/refit_core.hpp"
#include "instances_refit.hpp"

namespace crt {
namespace {

using rf::Box;

// ordered key of a finite float: unsigned compare of keys == float compare (-0 below +0, as rf::tmin / tmax)
__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the last k in [0, n) with start[k] <= x (start[0] == 0 <= x)
__device__ __forceinline__ uint32_t find_segment(const uint32_t* __restrict__ start, uint32_t stride, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start[(size_t)mid * stride] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

constexpr uint32_t kCheckItems = 16;        // vertices / triangles per thread and chunk: a block covers kCheckChunk of each

// One block = one chunk of one mesh of the call.  Thread items: vertex i (every coordinate finite, |x| <= 1e18) and triangle i (the
// ordered keys of the three vertices it references).  out[8 k]: |= 1 on a bad coordinate; [8k+1..3] max keys; [8k+4..6] complemented min
// keys (one zeroing memset, atomicMax for both).
__global__ __launch_bounds__(256) void k_inst_check(const InstRefitMesh* __restrict__ meshes, const uint32_t* __restrict__ chunk_start, uint32_t n,
                                                     const int32_t* __restrict__ src_idx, uint32_t* __restrict__ out) {
    const uint32_t k = find_segment(chunk_start, 1u, n, blockIdx.x);
    const InstRefitMesh m = meshes[k];
    const uint32_t base = (blockIdx.x - chunk_start[k]) * kCheckChunk;
    uint32_t bad = 0, hi[3] = {0u, 0u, 0u}, lo_c[3] = {0u, 0u, 0u};
    for (uint32_t r = 0; r < kCheckItems; ++r) {
        const uint32_t i = base + r * 256u + threadIdx.x;
        if (i < m.n_vertices)
            for (int a = 0; a < 3; ++a) {
                const float c = m.verts[3 * (size_t)i + a];
                if (!(c <= 1.0e18f && c >= -1.0e18f)) bad = 1u;
            }
        if (i < m.n_tris) {
            const int32_t* t = src_idx + 3 * ((size_t)m.tri_off + i);
            for (int j = 0; j < 3; ++j) {
                const uint32_t v = (uint32_t)t[j];
                if (v >= m.n_vertices) { bad = 1u; continue; }
                for (int a = 0; a < 3; ++a) {
                    const uint32_t key = order_key(m.verts[3 * (size_t)v + a]);
                    hi[a] = max(hi[a], key);
                    lo_c[a] = max(lo_c[a], ~key);
                }
            }
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        bad |= __shfl_xor(bad, s);
        for (int a = 0; a < 3; ++a) { hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], s)); lo_c[a] = max(lo_c[a], (uint32_t)__shfl_xor((int)lo_c[a], s)); }
    }
    if ((threadIdx.x & 63u) == 0u) {
        uint32_t* o = out + 8 * (size_t)k;
        if (bad) atomicOr(o, 1u);
        for (int a = 0; a < 3; ++a) { atomicMax(o + 1 + a, hi[a]); atomicMax(o + 4 + a, lo_c[a]); }
    }
}

// Records (v0 | id) (e1 | slot) (e2 | w) of every updated mesh, one lane each: the vertex indices come from the source-order index array
// by the record's id (v0.w); the two fp32 subtractions of scene_build.hip make_record; the w words stay.
__global__ __launch_bounds__(256) void k_inst_refit_records(float4* __restrict__ recs, uint32_t n_recs, const InstRefitSeg* __restrict__ segs,
                                                             uint32_t n_segs, uint32_t count, const InstRefitMesh* __restrict__ meshes,
                                                             const int32_t* __restrict__ src_idx) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const InstRefitSeg sg = segs[find_segment(&segs[0].start, 4u, n_segs, j)];
    const uint32_t i = sg.first + (j - sg.start);
    if (i >= n_recs) return;
    const InstRefitMesh m = meshes[sg.slot];
    float4* r = recs + 3 * (size_t)i;
    float4 a = r[0], b = r[1], c = r[2];
    const uint32_t id = (uint32_t)__float_as_int(a.w);
    if (id >= m.n_tris) return;
    const int32_t* t = src_idx + 3 * ((size_t)m.tri_off + id);
    const float* v0 = m.verts + 3 * (size_t)(uint32_t)t[0];
    const float* v1 = m.verts + 3 * (size_t)(uint32_t)t[1];
    const float* v2 = m.verts + 3 * (size_t)(uint32_t)t[2];
    a.x = v0[0]; a.y = v0[1]; a.z = v0[2];
    b.x = v1[0] - v0[0]; b.y = v1[1] - v0[1]; b.z = v1[2] - v0[2];
    c.x = v2[0] - v0[0]; c.y = v2[1] - v0[1]; c.z = v2[2] - v0[2];
    r[0] = a; r[1] = b; r[2] = c;
}

// lane ^ 1, ^ 2, ^ 4 inside groups of 8 lanes (ds_swizzle bit-mask mode: and 0x1f, or 0, xor m)
template <int XOR>
__device__ __forceinline__ float swz(float v) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1f | (XOR << 10))); }

constexpr uint32_t kNodesPerBlock = 32;      // 8 lanes per node8, 256 threads

// One depth level of every updated BLAS: refit.hip k_refit_node8_level's mapping (eight adjacent lanes per node8, one per slot; the node
// box reduced with ds_swizzle; each lane quantises its own slot).  Nodes are global indices into the packed array, whose child and
// triangle bases are rebased already; box8 holds 6 floats per BLAS node8 (index node - node_base).  A leaf slot's box grows from its
// records' ids through the source-order index array.  meta, imask, both bases and the planes of empty slots stay.
__global__ __launch_bounds__(256) void k_inst_refit_node8_level(uint4* __restrict__ nodes, uint32_t node_base, uint32_t n_nodes,
                                                                 const uint32_t* __restrict__ order, const InstRefitSeg* __restrict__ segs,
                                                                 uint32_t n_segs, uint32_t count, const float4* __restrict__ recs, uint32_t n_recs,
                                                                 const InstRefitMesh* __restrict__ meshes, const int32_t* __restrict__ src_idx,
                                                                 float2* __restrict__ box8) {
    __shared__ uint4 q_rows[kNodesPerBlock][3];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 3, s = t & 7u, local = threadIdx.x >> 3;
    bool valid = j < count;
    InstRefitSeg sg{0u, 0u, 0u, 0u};
    if (valid) sg = segs[find_segment(&segs[0].start, 4u, n_segs, j)];
    const uint32_t node = valid ? order[sg.first + (j - sg.start)] : 0u;
    valid = valid && node >= node_base && node < n_nodes;
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    if (valid) { r0 = nodes[5 * (size_t)node]; r1 = nodes[5 * (size_t)node + 1]; }
    if (valid && s < 3u) q_rows[local][s] = nodes[5 * (size_t)node + 2u + s];
    const uint32_t imask = r0.w >> 24;
    const uint8_t meta = (uint8_t)(((s < 4u ? r1.z : r1.w) >> (8u * (s & 3u))) & 0xffu);
    Box b = rf::empty_box();
    if (valid && meta) {
        if ((imask >> s) & 1u) {
            const uint32_t c = r1.x + (uint32_t)__builtin_popcount(imask & ((1u << s) - 1u));
            if (c >= node_base && c < n_nodes) {
                const size_t cb = 3 * (size_t)(c - node_base);
                const float2 x0 = box8[cb], x1 = box8[cb + 1], x2 = box8[cb + 2];
                b = Box{{x0.x, x0.y, x1.x}, {x1.y, x2.x, x2.y}};
            }
        } else {
            const InstRefitMesh m = meshes[sg.slot];
            const uint32_t first = r1.y + (uint32_t)rf::leaf_offset(meta), cnt = (uint32_t)rf::leaf_count(meta);
            for (uint32_t k = 0; k < cnt; ++k) {
                if (first + k >= n_recs) break;
                const uint32_t id = (uint32_t)__float_as_int(recs[3 * (size_t)(first + k)].w);
                if (id >= m.n_tris) continue;
                const int32_t* tr = src_idx + 3 * ((size_t)m.tri_off + id);
                const int32_t v[3] = {tr[0], tr[1], tr[2]};
                rf::grow_triangle(b, v, m.verts);
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
    uint4* dst = nodes + 5 * (size_t)node;
    if (s < 3u) dst[2u + s] = q_rows[local][s];
    if (s == 0u) {
        dst[0] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]),
                            (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | (imask << 24));
        const size_t nb = 3 * (size_t)(node - node_base);
        box8[nb] = make_float2(u.lo[0], u.lo[1]);
        box8[nb + 1] = make_float2(u.lo[2], u.hi[0]);
        box8[nb + 2] = make_float2(u.hi[1], u.hi[2]);
    }
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1u, (n + 255u) / 256u)); }

}  // namespace

void launch_inst_check(const InstRefitMesh* d_meshes, const uint32_t* d_chunk_start, uint32_t n, uint32_t n_chunks, const int32_t* d_src_idx,
                       uint32_t* d_out, hipStream_t stream) {
    if (n && n_chunks) hipLaunchKernelGGL(k_inst_check, dim3(n_chunks), dim3(256), 0, stream, d_meshes, d_chunk_start, n, d_src_idx, d_out);
}
void launch_inst_refit_records(float4* d_recs, uint32_t n_recs, const InstRefitSeg* d_segs, uint32_t n_segs, uint32_t count,
                               const InstRefitMesh* d_meshes, const int32_t* d_src_idx, hipStream_t stream) {
    if (n_segs && count)
        hipLaunchKernelGGL(k_inst_refit_records, grid_for(count), dim3(256), 0, stream, d_recs, n_recs, d_segs, n_segs, count, d_meshes, d_src_idx);
}
void launch_inst_refit_node8_level(void* d_nodes, uint32_t node_base, uint32_t n_nodes, const uint32_t* d_order, const InstRefitSeg* d_segs,
                                   uint32_t n_segs, uint32_t count, const float4* d_recs, uint32_t n_recs, const InstRefitMesh* d_meshes,
                                   const int32_t* d_src_idx, float* d_box8, hipStream_t stream) {
    if (n_segs && count)
        hipLaunchKernelGGL(k_inst_refit_node8_level, grid_for((uint64_t)count * 8u), dim3(256), 0, stream, static_cast<uint4*>(d_nodes), node_base,
                           n_nodes, d_order, d_segs, n_segs, count, d_recs, n_recs, d_meshes, d_src_idx, reinterpret_cast<float2*>(d_box8));
}

}  // namespace crt
