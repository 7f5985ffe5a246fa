// Refit kernels of crt_update_vertices, crt_instances_update_meshes (§12) and crt_instances_refit (§13): new vertex
// positions or instance boxes, same topology; and what tells a caller when to stop refitting (§19): the SAH cost of a tree.  The
// trees and record arrays are rewritten in place, one launch per tree level, deepest first (the kernel boundary orders the levels, as in
// lbvh.hip k_refit_level).  The records and node8 kernels serve both callers: each refitted tree is a RefitMesh (device_build.hpp), and a
// per-launch segment table maps an entry to its mesh and item, so one launch covers every mesh of an instanced call and a scene is the
// one-mesh, one-segment case.  Every box and quantised plane comes from host/refit_core.hpp, which the host refits (crt_bvh2_refit /
// crt_cwbvh_refit) use too: the device output is byte-identical to theirs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "crt_error.hpp"
#include "device_build.hpp"
#include "host/cost_core.hpp"
#include "host/flatnode_link.hpp"
#include "host/refit_core.hpp"

namespace crt {
namespace {

using rf::Box;

// the last k in [0, n) with start[k] <= x (start[0] == 0 <= x)
__device__ __forceinline__ uint32_t find_segment(const uint32_t* __restrict__ start, uint32_t stride, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start[(size_t)mid * stride] <= x) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ RefitSeg segment_of(const RefitSeg* __restrict__ segs, uint32_t n_segs, uint32_t j) {
    return segs[find_segment(&segs[0].start, 4u, n_segs, j)];
}

// ---- checks ----
// crt_scene_create's rule for a coordinate: finite and |x| <= 1e18
__device__ __forceinline__ bool coord_ok(float c) { return c <= 1.0e18f && c >= -1.0e18f; }
__device__ __forceinline__ void grow_keys(uint32_t hi[3], uint32_t lo_c[3], int a, float c) {
    const uint32_t key = rf::order_key(c);
    hi[a] = max(hi[a], key);
    lo_c[a] = max(lo_c[a], ~key);
}
// a wave's verdict and bounds, published by its first lane: out[0] |= 1 on a bad item; out[1..3] max keys; out[4..6] complemented min keys
// (so that one zeroing memset and atomicMax serve both)
__device__ __forceinline__ void publish_check(uint32_t bad, uint32_t hi[3], uint32_t lo_c[3], uint32_t* out) {
    for (int m = 32; m >= 1; m >>= 1) {
        bad |= __shfl_xor(bad, m);
        for (int a = 0; a < 3; ++a) { hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], m)); lo_c[a] = max(lo_c[a], (uint32_t)__shfl_xor((int)lo_c[a], m)); }
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (bad) atomicOr(out, 1u);
        for (int a = 0; a < 3; ++a) { atomicMax(out + 1 + a, hi[a]); atomicMax(out + 4 + a, lo_c[a]); }
    }
}

// scene: the bounds of ALL vertices (they feed the ray_bins / sort_shadow cell grid)
__global__ void k_check_vertices(const float* __restrict__ v, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t bad = 0, hi[3] = {0u, 0u, 0u}, lo_c[3] = {0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        for (int a = 0; a < 3; ++a) {
            const float c = v[3 * (size_t)i + a];
            if (!coord_ok(c)) { bad = 1u; continue; }
            grow_keys(hi, lo_c, a, c);
        }
    publish_check(bad, hi, lo_c, out);
}

constexpr uint32_t kCheckItems = kCheckChunk / 256;      // vertices / triangles per thread and chunk

// instanced meshes: one block = one chunk of one mesh of the call.  Thread items: vertex i (its coordinates) and index entry i (its three
// indices below n_vertices, and the keys of the vertices they reference: the mesh box covers the referenced vertices only).  out: 8 words
// per mesh.
__global__ __launch_bounds__(256) void k_check_meshes(const RefitMesh* __restrict__ meshes, const uint32_t* __restrict__ chunk_start, uint32_t n,
                                                      uint32_t* __restrict__ out) {
    const uint32_t k = find_segment(chunk_start, 1u, n, blockIdx.x);
    const RefitMesh m = meshes[k];
    const uint32_t base = (blockIdx.x - chunk_start[k]) * kCheckChunk;
    uint32_t bad = 0, hi[3] = {0u, 0u, 0u}, lo_c[3] = {0u, 0u, 0u};
    for (uint32_t r = 0; r < kCheckItems; ++r) {
        const uint32_t i = base + r * 256u + threadIdx.x;
        if (i < m.n_vertices)
            for (int a = 0; a < 3; ++a)
                if (!coord_ok(m.verts[3 * (size_t)i + a])) bad = 1u;
        if (i < m.n_idx) {
            const int32_t* t = m.idx + (size_t)m.stride * i;
            for (int j = 0; j < 3; ++j) {
                const uint32_t v = (uint32_t)t[j];
                if (v >= m.n_vertices) { bad = 1u; continue; }
                for (int a = 0; a < 3; ++a) grow_keys(hi, lo_c, a, m.verts[3 * (size_t)v + a]);
            }
        }
    }
    publish_check(bad, hi, lo_c, out + 8 * (size_t)k);
}

// ---- level discovery ----
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
// depth of every node by climbing its parent links (root = 0; at most 255 levels, the trees are far shallower)
__global__ void k_depths(const int32_t* __restrict__ parent, uint32_t n, uint8_t* __restrict__ depth) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t d = 0;
    for (int32_t p = parent[i]; p >= 0 && d < 255u; p = parent[p]) ++d;
    depth[i] = (uint8_t)d;
}

// ---- per update ----
// records: rows (v0 | w) (e1 | w) (e2 | w) regathered from the index entry the key word names, with the two fp32 subtractions of
// scene_build.hip make_record; the w words stay
__global__ __launch_bounds__(256) void k_refit_records(float4* __restrict__ recs, uint32_t rows, uint32_t n_recs, const RefitSeg* __restrict__ segs,
                                                       uint32_t n_segs, uint32_t count, const RefitMesh* __restrict__ meshes) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const RefitSeg sg = segment_of(segs, n_segs, j);
    const uint32_t i = sg.first + (j - sg.start);
    if (i >= n_recs) return;
    const RefitMesh m = meshes[sg.mesh];
    float4* r = recs + (size_t)i * rows;
    float4 a = r[0], b = r[1], c = r[2];
    const uint32_t e = (uint32_t)__float_as_int(m.key_word < 4u ? a.w : b.w);      // scenes and BLASes: v0.w or e1.w
    if (e >= m.n_idx) return;
    const int32_t* t = m.idx + (size_t)m.stride * e;
    const float* v0 = m.verts + 3 * (size_t)(uint32_t)t[0];
    const float* v1 = m.verts + 3 * (size_t)(uint32_t)t[1];
    const float* v2 = m.verts + 3 * (size_t)(uint32_t)t[2];
    a.x = v0[0]; a.y = v0[1]; a.z = v0[2];
    b.x = v1[0] - v0[0]; b.y = v1[1] - v0[1]; b.z = v1[2] - v0[2];
    c.x = v2[0] - v0[0]; c.y = v2[1] - v0[1]; c.z = v2[2] - v0[2];
    r[0] = a; r[1] = b; r[2] = c;
}

// one BVH2 level (scenes only): leaves from their slot ranges, inner nodes from their two children (the deeper level, final by now)
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

// one node8 level: eight adjacent lanes per node, one per slot.  A lane builds its slot's box (leaf: the vertex boxes of its records' index
// entries; inner: the child node8's float box, written by the previous launch), the node box is reduced across the eight lanes, and every
// lane quantises its own slot against it.  Nodes are indices into the whole node array (an instanced scene's BLAS bases are rebased
// already); box8 is indexed from node_base.  meta, imask, child and triangle bases stay; so do the planes of empty slots.
__global__ __launch_bounds__(256) void k_refit_node8_level(uint4* __restrict__ nodes, uint32_t node_rows, uint32_t node_base, uint32_t n_nodes,
                                                           const uint32_t* __restrict__ order, const RefitSeg* __restrict__ segs, uint32_t n_segs,
                                                           uint32_t count, const float4* __restrict__ recs, uint32_t tri_rows, uint32_t n_recs,
                                                           const RefitMesh* __restrict__ meshes, float2* __restrict__ box8) {
    __shared__ uint4 q_rows[kNodesPerBlock][3];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 3, s = t & 7u, local = threadIdx.x >> 3;
    bool valid = j < count;
    RefitSeg sg{0u, 0u, 0u, 0u};
    if (valid) sg = segment_of(segs, n_segs, j);
    const uint32_t node = valid ? order[sg.first + (j - sg.start)] : 0u;
    valid = valid && node >= node_base && node < n_nodes;
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    if (valid) { r0 = nodes[(size_t)node * node_rows]; r1 = nodes[(size_t)node * node_rows + 1]; }
    if (valid && s < 3u) q_rows[local][s] = nodes[(size_t)node * node_rows + 2u + s];
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
            const RefitMesh m = meshes[sg.mesh];
            const uint32_t first = r1.y + (uint32_t)rf::leaf_offset(meta), cnt = (uint32_t)rf::leaf_count(meta);
            for (uint32_t k = 0; k < cnt; ++k) {
                if (first + k >= n_recs) break;
                const uint32_t e = reinterpret_cast<const uint32_t*>(recs)[4 * (size_t)(first + k) * tri_rows + m.key_word];
                if (e >= m.n_idx) continue;
                const int32_t* tr = m.idx + (size_t)m.stride * e;
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
    if (valid && s == 0u) {                           // the box the parent level reads (the next launch)
        const size_t nb = 3 * (size_t)(node - node_base);
        box8[nb] = make_float2(u.lo[0], u.lo[1]);
        box8[nb + 1] = make_float2(u.lo[2], u.hi[0]);
        box8[nb + 2] = make_float2(u.hi[1], u.hi[2]);
    }
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
    }
}

// the TLAS as a refit mesh: instance i's world box (lo, hi) is vertices 2i and 2i + 1 of the box array, its triangle (2i, 2i + 1, 2i)
__global__ void k_box_triples(int32_t* __restrict__ idx, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    idx[3 * (size_t)i] = (int32_t)(2u * i);
    idx[3 * (size_t)i + 1] = (int32_t)(2u * i + 1u);
    idx[3 * (size_t)i + 2] = (int32_t)(2u * i);
}

// ---- SAH cost of a node8 range (crt_get_tree_cost, crt_instances_tree_cost) ----
// Eight adjacent lanes per node8, one per slot, as k_refit_node8_level maps them.  A lane decodes its slot's box (host/cost_core.hpp: the
// host function's arithmetic) and adds its half-area to its own partial; a block walks its share of the range with a fixed stride, so
// which slots a lane adds, and in which order, depends on the launch shape alone.  The partials are reduced across the wave by lane
// shuffles and across the block's four waves through LDS in wave order; k_tree_cost_sum adds the blocks' partials in index order.  No
// floating-point atomics anywhere: two calls on one tree return the same bits.
struct CostPartial { double inner, leaf; unsigned long long n_inner, n_leaf, n_items, pad; };
static_assert(sizeof(CostPartial) == 48, "CostPartial is 48 bytes");
struct CostResult { double root, inner, leaf; unsigned long long n_inner, n_leaf, n_items; };

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(b & 0xffffffffll), m), hi = __shfl_xor((int)(b >> 32), m);
    return __longlong_as_double(((long long)hi << 32) | (long long)(uint32_t)lo);
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const int lo = __shfl_xor((int)(v & 0xffffffffull), m), hi = __shfl_xor((int)(v >> 32), m);
    return ((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo;
}

constexpr uint32_t kCostBlocks = 256;      // at most: 65,536 lanes = 8,192 node8s per pass over the range

__global__ __launch_bounds__(256) void k_tree_cost(const uint4* __restrict__ nodes, uint32_t node_rows, uint64_t first, uint64_t count, uint64_t root,
                                                   CostPartial* __restrict__ partial, double* __restrict__ root_area) {
    __shared__ CostPartial wave_part[4];
    const uint32_t s = threadIdx.x & 7u;
    CostPartial acc{0.0, 0.0, 0ull, 0ull, 0ull, 0ull};
    const uint64_t per_pass = (uint64_t)gridDim.x * kNodesPerBlock;
    // every lane of a wave runs the same number of passes (the shuffles below need them all)
    for (uint64_t base = (uint64_t)blockIdx.x * kNodesPerBlock; base < count; base += per_pass) {
        const uint64_t j = base + (threadIdx.x >> 3);
        const bool valid = j < count;
        const uint64_t node = first + (valid ? j : 0ull);
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(nodes + node * node_rows);
        const uint8_t meta = valid ? bytes[24 + s] : (uint8_t)0;
        const uint32_t imask = valid ? (uint32_t)bytes[15] : 0u;
        Box b = rf::empty_box();
        uint32_t used = 0u;
        if (meta) {
            b = tc::slot_box(bytes, (int)s);
            used = 1u;
            const double a = tc::half_area(b);
            if ((imask >> s) & 1u) {
                acc.inner += a;
                ++acc.n_inner;
            } else {
                const int items = rf::leaf_count(meta);
                acc.leaf += a * (double)items;
                ++acc.n_leaf;
                acc.n_items += (unsigned long long)items;
            }
        }
        // the root's box: the union of its used slots across its eight lanes
        Box u = b;
        for (int m = 1; m <= 4; m <<= 1) {
            for (int k = 0; k < 3; ++k) { u.lo[k] = rf::tmin(u.lo[k], __shfl_xor(u.lo[k], m)); u.hi[k] = rf::tmax(u.hi[k], __shfl_xor(u.hi[k], m)); }
            used |= (uint32_t)__shfl_xor((int)used, m);
        }
        if (valid && s == 0u && first + j == root) *root_area = used ? tc::half_area(u) : 0.0;
    }
    for (int m = 1; m <= 32; m <<= 1) {
        acc.inner += shfl_xor_f64(acc.inner, m);
        acc.leaf += shfl_xor_f64(acc.leaf, m);
        acc.n_inner += shfl_xor_u64(acc.n_inner, m);
        acc.n_leaf += shfl_xor_u64(acc.n_leaf, m);
        acc.n_items += shfl_xor_u64(acc.n_items, m);
    }
    if ((threadIdx.x & 63u) == 0u) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0u) {
        CostPartial t = wave_part[0];
        for (int w = 1; w < 4; ++w) {
            t.inner += wave_part[w].inner; t.leaf += wave_part[w].leaf;
            t.n_inner += wave_part[w].n_inner; t.n_leaf += wave_part[w].n_leaf; t.n_items += wave_part[w].n_items;
        }
        partial[blockIdx.x] = t;
    }
}
// the last pass: one lane adds the blocks' partials in index order
__global__ void k_tree_cost_sum(const CostPartial* __restrict__ partial, uint32_t n, const double* __restrict__ root_area, CostResult* __restrict__ out) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    CostResult r{*root_area, 0.0, 0.0, 0ull, 0ull, 0ull};
    for (uint32_t i = 0; i < n; ++i) {
        r.inner += partial[i].inner; r.leaf += partial[i].leaf;
        r.n_inner += partial[i].n_inner; r.n_leaf += partial[i].n_leaf; r.n_items += partial[i].n_items;
    }
    *out = r;
}

// ---- crt_rebuild_vertices: the source-order triangle array back from the leaf-order one ----
// Record i of a device-built scene names its triangle's original id in v0.w and its leaf slot in e1.w; one triangle per slot and no
// duplicates, so id <- slot is a permutation.
__global__ void k_scatter_source(const float4* __restrict__ recs, uint32_t tri_rows, uint32_t n, const crt_triangle* __restrict__ slot_tris,
                                 crt_triangle* __restrict__ src) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = (uint32_t)__float_as_int(recs[(size_t)i * tri_rows].w), slot = (uint32_t)__float_as_int(recs[(size_t)i * tri_rows + 1].w);
    if (id < n && slot < n) src[id] = slot_tris[slot];
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>(1u, (n + 255u) / 256u)); }

}  // namespace

int discover_levels(const RefitTree* trees, size_t n_trees, hipStream_t stream, uint32_t** d_order, std::vector<std::vector<uint32_t>>& level) {
    *d_order = nullptr;
    uint64_t n_all = 0;
    for (size_t t = 0; t < n_trees; ++t) n_all += trees[t].n;
    DeviceArena tmp;
    hipError_t he = tmp.reserve(DeviceArena::padded(4 * n_all) + DeviceArena::padded(n_all));
    if (he != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("refit level discovery: hipMalloc: ") + hipGetErrorString(he));
    int32_t* d_parent = tmp.take<int32_t>(n_all);
    uint8_t* d_depth = tmp.take<uint8_t>(n_all);
    std::vector<uint8_t> depth(n_all);
    if ((he = hipMemsetAsync(d_parent, 0xff, 4 * n_all, stream)) != hipSuccess)
        return fail(CRT_ERR_HIP, std::string("refit level discovery: ") + hipGetErrorString(he));
    uint64_t off = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        const RefitTree& x = trees[t];
        if (x.bvh2) hipLaunchKernelGGL(k_bvh2_parents, grid_for(x.n), dim3(256), 0, stream, static_cast<const crt_flatnode*>(x.d_nodes), x.n, d_parent + off);
        else hipLaunchKernelGGL(k_node8_parents, grid_for(x.n), dim3(256), 0, stream, static_cast<const uint4*>(x.d_nodes), x.node_rows, x.n, d_parent + off);
        hipLaunchKernelGGL(k_depths, grid_for(x.n), dim3(256), 0, stream, d_parent + off, x.n, d_depth + off);
        off += x.n;
    }
    if ((he = hipMemcpyAsync(depth.data(), d_depth, n_all, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
        (he = hipStreamSynchronize(stream)) != hipSuccess || (he = hipGetLastError()) != hipSuccess)
        return fail(CRT_ERR_HIP, std::string("refit level discovery: ") + hipGetErrorString(he));
    std::vector<uint32_t> order(n_all);
    level.assign(n_trees, {});
    off = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        const RefitTree& x = trees[t];
        std::vector<uint32_t> count(257, 0);
        for (uint32_t i = 0; i < x.n; ++i) ++count[depth[off + i] + 1u];
        uint32_t levels = 0;
        for (uint32_t d = 0; d < 256; ++d) if (count[d + 1]) levels = d + 1;
        std::vector<uint32_t>& start = level[t];
        start.assign(levels + 1, (uint32_t)off);
        for (uint32_t d = 0; d < levels; ++d) start[d + 1] = start[d] + count[d + 1];
        std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
        for (uint32_t i = 0; i < x.n; ++i) order[cursor[depth[off + i]]++] = x.base + i;
        off += x.n;
    }
    if ((he = hipMalloc(reinterpret_cast<void**>(d_order), std::max<uint64_t>(n_all, 1) * 4)) != hipSuccess)
        return fail(CRT_ERR_NOMEM, std::string("refit level discovery: hipMalloc: ") + hipGetErrorString(he));
    if ((he = hipMemcpyAsync(*d_order, order.data(), n_all * 4, hipMemcpyHostToDevice, stream)) != hipSuccess ||
        (he = hipStreamSynchronize(stream)) != hipSuccess)               // before the host order goes
        return fail(CRT_ERR_HIP, std::string("refit level discovery: ") + hipGetErrorString(he));
    return CRT_OK;
}

int tree_cost_on_device(const void* d_nodes, uint32_t node_rows, uint64_t first, uint64_t count, uint64_t root, hipStream_t stream,
                        crt_tree_cost* out) {
    *out = crt_tree_cost{};
    if (count == 0) return CRT_OK;
    if (!d_nodes || root < first || root - first >= count) return fail(CRT_ERR_INVALID, "tree cost: the root lies outside the node range");
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kCostBlocks, (count + kNodesPerBlock - 1u) / kNodesPerBlock);
    DeviceArena tmp;
    hipError_t he = tmp.reserve(DeviceArena::padded(blocks * sizeof(CostPartial)) + DeviceArena::padded(sizeof(double)) + DeviceArena::padded(sizeof(CostResult)));
    if (he != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("tree cost: hipMalloc: ") + hipGetErrorString(he));
    CostPartial* d_partial = tmp.take<CostPartial>(blocks);
    double* d_root = tmp.take<double>(1);
    CostResult* d_res = tmp.take<CostResult>(1);
    CostResult res{};
    if ((he = hipMemsetAsync(d_root, 0, sizeof(double), stream)) != hipSuccess) return fail(CRT_ERR_HIP, std::string("tree cost: ") + hipGetErrorString(he));
    hipLaunchKernelGGL(k_tree_cost, dim3(blocks), dim3(256), 0, stream, static_cast<const uint4*>(d_nodes), node_rows, first, count, root, d_partial, d_root);
    hipLaunchKernelGGL(k_tree_cost_sum, dim3(1), dim3(64), 0, stream, d_partial, blocks, d_root, d_res);
    if ((he = hipGetLastError()) != hipSuccess || (he = hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream)) != hipSuccess ||
        (he = hipStreamSynchronize(stream)) != hipSuccess)
        return fail(CRT_ERR_HIP, std::string("tree cost: ") + hipGetErrorString(he));
    out->root_area = res.root; out->inner_area = res.inner; out->leaf_area = res.leaf;
    out->n_nodes8 = count; out->n_inner_slots = res.n_inner; out->n_leaf_slots = res.n_leaf; out->n_leaf_items = res.n_items;
    out->cost = tc::finish(res.root, res.inner, res.leaf);
    return CRT_OK;
}

void launch_scatter_source(const void* d_recs, uint32_t tri_rows, uint32_t n, const crt_triangle* d_slot_tris, crt_triangle* d_src, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_scatter_source, grid_for(n), dim3(256), 0, stream, static_cast<const float4*>(d_recs), tri_rows, n, d_slot_tris, d_src);
}

void launch_check_vertices(const float* d_verts, uint32_t n_vertices, uint32_t* d_out, hipStream_t stream) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024u, (n_vertices + 255u) / 256u + 1u);
    hipLaunchKernelGGL(k_check_vertices, dim3(blocks), dim3(256), 0, stream, d_verts, n_vertices, d_out);
}
void launch_check_meshes(const RefitMesh* d_meshes, const uint32_t* d_chunk_start, uint32_t n, uint32_t n_chunks, uint32_t* d_out,
                         hipStream_t stream) {
    if (n && n_chunks) hipLaunchKernelGGL(k_check_meshes, dim3(n_chunks), dim3(256), 0, stream, d_meshes, d_chunk_start, n, d_out);
}
void launch_box_triples(int32_t* d_idx, uint32_t n, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_box_triples, grid_for(n), dim3(256), 0, stream, d_idx, n);
}
void launch_refit_records(void* d_recs, uint32_t rows, uint32_t n_recs, const RefitSeg* d_segs, uint32_t n_segs, uint32_t count,
                          const RefitMesh* d_meshes, hipStream_t stream) {
    if (n_segs && count)
        hipLaunchKernelGGL(k_refit_records, grid_for(count), dim3(256), 0, stream, static_cast<float4*>(d_recs), rows, n_recs, d_segs, n_segs, count,
                           d_meshes);
}
void launch_refit_bvh2_level(void* d_flat, uint32_t n2, const uint32_t* d_order, uint32_t count, const void* d_tris, uint32_t n_slots,
                             const float* d_verts, hipStream_t stream) {
    hipLaunchKernelGGL(k_refit_bvh2_level, grid_for(count), dim3(256), 0, stream, static_cast<crt_flatnode*>(d_flat), n2, d_order, count,
                       static_cast<const int4*>(d_tris), n_slots, d_verts);
}
void launch_refit_node8_level(void* d_nodes, uint32_t node_rows, uint32_t node_base, uint32_t n_nodes, const uint32_t* d_order,
                              const RefitSeg* d_segs, uint32_t n_segs, uint32_t count, const void* d_recs, uint32_t tri_rows, uint32_t n_recs,
                              const RefitMesh* d_meshes, float* d_box8, hipStream_t stream) {
    if (n_segs && count)
        hipLaunchKernelGGL(k_refit_node8_level, grid_for((uint64_t)count * 8u), dim3(256), 0, stream, static_cast<uint4*>(d_nodes), node_rows,
                           node_base, n_nodes, d_order, d_segs, n_segs, count, static_cast<const float4*>(d_recs), tri_rows, n_recs, d_meshes,
                           reinterpret_cast<float2*>(d_box8));
}

}  // namespace crt
