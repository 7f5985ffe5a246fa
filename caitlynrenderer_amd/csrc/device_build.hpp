// Device-resident halves of the GPU builders, shared by the host-array entry points
// (crt_lbvh_build, crt_cwbvh_convert_device) and by crt_scene_create's build-on-device path, where the BVH2, the CWBVH
// and the intersection records are produced in HBM and never cross PCIe (the reference's own flow is
// build on the host, Scene.h:929-958, then one upload, :1000-1062).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/crt.h"
#include "crt_error.hpp"
#include "rt_kernels.hpp"

namespace crt {

// ---- what the host files share ----
inline int require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(CRT_ERR_NO_DEVICE, "no HIP device visible: the traversal path has no CPU fallback");
    return CRT_OK;
}

template <typename T>
int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return fail(CRT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return CRT_OK;
}

// the builder a create's CRT_BUILD_* flags ask of the device (CRT_GPU_BUILD_*; bits 8-15: the PLOC radius)
inline uint32_t gpu_flags_of(uint32_t build_flags) {
    return (build_flags & CRT_BUILD_SAH) ? (CRT_GPU_BUILD_SAH | (build_flags & 0xff00u))
           : (build_flags & CRT_BUILD_PLOC) ? (CRT_GPU_BUILD_PLOC | (build_flags & 0xff00u)) : 0u;
}

// A walk pushes at most one entry per level it has descended FROM — what is left of that node's hit list — and the deepest level (depth8,
// root = 1) has no inner children to descend to: depth8 - 1 entries hold any walk.  One row of the wave's LDS region is 512 bytes and LDS is
// handed out in 1,280-byte units: at depth 11 (8 M triangles) the row saved is the difference between 21 and 24 waves per CU.
inline uint32_t cwbvh_stack_entries(uint32_t depth8) { return std::min<uint32_t>(CRT_STACK_ENTRIES, std::max<uint32_t>(2u, depth8 - 1u)); }
// The BVH2 walk's LDS stack: depth + 2 entries, 96 at the most.  0 = deeper than that: such a BVH2 is not walked (nor kept)
inline uint32_t bvh2_stack_entries(uint32_t depth2) { return depth2 + 2u <= 96u ? depth2 + 2u : 0u; }

// One hipMalloc carved into 256-byte aligned pieces and freed as a whole: the builders need ~25 temporaries, and a
// hipMalloc / hipFree pair per temporary was most of the wall time of a call.
struct DeviceArena {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() { release(); }
    hipError_t reserve(size_t bytes) {
        release();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), bytes ? bytes : 256);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() { if (base) (void)hipFree(base); base = nullptr; cap = used = 0; }
    void reset() { used = 0; }
    template <typename T> T* take(size_t count) {          // nullptr when the arena is exhausted
        const size_t bytes = (count * sizeof(T) + 255) & ~size_t(255);
        if (used + bytes > cap) return nullptr;
        T* p = reinterpret_cast<T*>(base + used);
        used += bytes;
        return p;
    }
    static size_t padded(size_t bytes) { return (bytes + 255) & ~size_t(255); }
};

// ---- linear BVH (lbvh.hip) ----
// d_vidx: vertex indices of triangle i at d_vidx[stride * i + 0..2] (stride 3 = packed, 12 = the crt_triangle array itself).
// d_flat (2n - 1 nodes, BFS order, one triangle per leaf) and d_tri_order (leaf slot -> input triangle) are caller-owned
// device buffers; temporaries come from `tmp` (lbvh_tmp_bytes).  Synchronises the stream twice (level table).
// flags: CRT_GPU_BUILD_* of include/crt.h (0 = linear BVH; CRT_GPU_BUILD_PLOC | radius << 8 = PLOC, whose boxes need no refit).
size_t lbvh_tmp_bytes(size_t n_tris, uint32_t flags);
int lbvh_build_on_device(const int32_t* d_vidx, uint32_t stride, const float* d_verts, uint32_t n_tris, uint32_t flags, DeviceArena& tmp,
                         crt_flatnode* d_flat, uint32_t* d_tri_order, uint32_t* depth_out, float* device_ms, hipStream_t stream);
// the binned-SAH build (CRT_GPU_BUILD_SAH) over n >= 2 caller-given leaf boxes (6 floats each: lo, hi; finite, |x| <= 1e18) instead of
// triangles; temporaries: lbvh_tmp_bytes(n, CRT_GPU_BUILD_SAH).  d_tri_order: leaf slot -> box index.
int sah_build_from_boxes_on_device(const float* d_boxes, uint32_t n, uint32_t flags, DeviceArena& tmp, crt_flatnode* d_flat, uint32_t* d_tri_order,
                                   uint32_t* depth_out, float* device_ms, hipStream_t stream);

// ---- BVH2 -> CWBVH (cwbvh_device.hip) ----
// d_tri_slots (n_slots) is caller-owned; *d_nodes_out is hipMalloc'ed here once the node count is known (caller frees) — unless the
// caller passes d_nodes_into with room for into_cap node8s and the tree fits: then *d_nodes_out == d_nodes_into and nothing is allocated.
// d_child_bvh2_out may be null (the debug child map is then not produced).  Same bytes as the host converter.
size_t cwbvh_tmp_bytes(size_t n_bvh2_nodes, size_t n_slots);
int cwbvh_convert_on_device(const crt_flatnode* d_bvh2, uint32_t n_nodes, uint32_t n_slots, DeviceArena& tmp, int32_t* d_tri_slots,
                            crt_node8** d_nodes_out, int32_t** d_child_bvh2_out, uint32_t* n8_out, uint32_t* depth_out, float* device_ms,
                            hipStream_t stream, crt_node8* d_nodes_into = nullptr, uint32_t into_cap = 0);

// ---- scene assembly on the device (scene_build.hip) ----
// Index validation of the uploaded crt_triangle array (what crt_scene_create checks on the host for host-built scenes):
// *d_flag |= 1 vertex index, 2 material index, 4 normal index, 8 texcoord index of a textured material out of range.
void launch_validate_triangles(const crt_triangle* d_tris, uint32_t n, uint32_t n_vertices, uint32_t n_materials, uint32_t n_normals,
                               uint32_t n_texcoords, const float* d_materials /* 16 floats each */, int have_tex, uint32_t* d_flag, hipStream_t stream);
// items of rows_in 16-byte rows -> items of rows_out rows (padding zeroed): the line-aligned device copies of nodes and records
void launch_restride(const void* d_src, uint32_t rows_in, void* d_dst, uint32_t rows_out, uint64_t n_items, hipStream_t stream);
// 12 float4 rows per node: the child planes as floats (uniform node steps; layout in scene_build.hip k_expand_planes)
void launch_expand_planes(const void* d_nodes, uint32_t node_rows, void* d_planes, uint64_t n_nodes, hipStream_t stream);
// d_slot_tris[slot] = d_in[tri_order[slot]] (the triangle array in BVH2 leaf order, as sbvh.h:130-139 leaves it) and the
// slot-ordered intersection records (v0 | original id) (e1 | slot) (e2 | material) of the BVH2 walk (may be null).
void launch_gather_slots(const crt_triangle* d_in, const uint32_t* d_tri_order, const float* d_verts, uint32_t n_slots, crt_triangle* d_slot_tris,
                         float4* d_recs2, hipStream_t stream);
// CWBVH-ordered intersection records: record i describes slot d_tri_slots[i].
void launch_gather_records(const crt_triangle* d_in, const uint32_t* d_tri_order, const int32_t* d_tri_slots, const float* d_verts, uint32_t n_tris8,
                           float4* d_recs, hipStream_t stream);

// ---- source-order triangles -> a walkable tree (scene_build.hip): crt_scene_create's build-on-device path, crt_rebuild_vertices, every BLAS ----
// What differs between a scene's tree and a mesh's.
struct TreeKind {
    const char* build;         // the two builder stages, as the messages name them
    const char* convert;
    uint32_t max_depth8;       // a deeper CWBVH is refused; 0 = no bound here
    bool slot_arrays;          // also the leaf-order triangle array and, while the BVH2 is walkable, its records
};
constexpr TreeKind kSceneTree{"LBVH build", "BVH2 -> CWBVH", CRT_STACK_ENTRIES, true};
constexpr TreeKind kBlasTree{"BLAS build", "BLAS BVH2 -> CWBVH", 0u /* bounded with the TLAS's depth, at every set */, false};

// A built tree.  Owns what it holds until the caller takes it (and nulls the pointer): the destructor waits for the stream and frees the rest.
struct DeviceTree {
    hipStream_t st = nullptr;
    float4* bvh2 = nullptr;    // the caller's own allocation, when it wants the tree to own it (a scene's; a BLAS's BVH2 is a piece of its arena)
    uint4* nodes = nullptr;    // packed: 5 rows per node8 ...
    float4* tris = nullptr;    // ... and 3 per record, CWBVH order
    int4* triangles = nullptr; // slot arrays: the triangles in BVH2 leaf order (what sbvh.h:130-139 leaves behind)
    float4* tris2 = nullptr;   // slot arrays: the records in that order
    float4* planes = nullptr;  // the caller's, when it expands them (crt_rebuild_vertices)
    uint32_t n = 0, n8 = 0, depth8 = 0, depth2 = 0;
    float lbvh_ms = 0.f, conv_ms = 0.f;
    bool keep_bvh2() const { return bvh2_stack_entries(depth2) != 0u; }
    uint32_t stack_entries() const { return cwbvh_stack_entries(depth8); }
    DeviceTree() = default;
    DeviceTree(const DeviceTree&) = delete;
    DeviceTree& operator=(const DeviceTree&) = delete;
    ~DeviceTree() {
        void* ptrs[] = {bvh2, nodes, tris, triangles, tris2, planes};
        if (std::all_of(std::begin(ptrs), std::end(ptrs), [](void* p) { return !p; })) return;
        (void)hipStreamSynchronize(st);
        for (void* p : ptrs) if (p) (void)hipFree(p);
    }
};
// what build_device_tree takes from the arena: leaf order, CWBVH slots, and the larger of the two builders' temporaries
size_t device_tree_tmp_bytes(uint32_t n, uint32_t gpu_flags);
// LBVH / PLOC / SAH BVH2 of the n triangles d_src (source order) into d_flat (2n - 1 nodes, the caller's), then the CWBVH, the records and the
// slot arrays, each in a hipMalloc of its own that *out owns.  The builders wait for the stream; the gather kernels are only enqueued, and read
// the arena: the caller waits for the stream before the arena goes.  `who` prefixes the messages.
int build_device_tree(const crt_triangle* d_src, const float* d_verts, uint32_t n, uint32_t gpu_flags, DeviceArena& arena, crt_flatnode* d_flat,
                      const TreeKind& kind, hipStream_t st, const std::string& who, DeviceTree* out);

// ---- refit to new positions, same topology (refit.hip): crt_update_vertices, crt_instances_update_meshes, crt_instances_refit ----
// One refitted tree's geometry.  Index entry e holds a triangle's three vertex indices at idx[stride * e + 0..2]; a record names its entry
// in its 32-bit word key_word.  Scene: d_triangles (crt_triangle, stride 12), the slot in e1.w.  BLAS: its slice of the source-order
// index array (stride 3), the source id in v0.w.  TLAS: the world boxes as 2 vertices each, the triples of launch_box_triples, the
// instance index in row 3 .y of the instance record (4 rows: node8 level kernel only).
struct RefitMesh {
    const float* verts;        // xyz per vertex
    const int32_t* idx;
    uint32_t stride;           // ints per entry
    uint32_t n_idx;            // valid entries
    uint32_t key_word;         // 3: v0.w, 7: e1.w, 13: row 3 .y
    uint32_t n_vertices;
};
static_assert(sizeof(RefitMesh) == 32, "RefitMesh is 32 bytes");

// a run of entries of one mesh: entries [start, next start) of a launch are items first .. of the array it covers (records, or positions
// in the level order); a launch finds its entry's segment by a binary search over the starts
struct RefitSeg { uint32_t start, first, mesh, pad; };

// one tree for discover_levels: a node8 array of node_rows 16-byte rows per node, or a BVH2 (crt_flatnode array)
struct RefitTree {
    const void* d_nodes;
    bool bvh2;
    uint32_t node_rows, n;
    uint32_t base;             // added to the tree's local node indices in the order
};
// The node indices of every tree level by level, root level first: parent links and depths on the device (at most 255 levels), a counting
// sort by depth on the host.  *d_order (hipMalloc'ed here, caller frees) holds the trees one after another; level[t][l] is the position in
// it of tree t's level l (+ end).  Synchronises the stream.
int discover_levels(const RefitTree* trees, size_t n_trees, hipStream_t stream, uint32_t** d_order, std::vector<std::vector<uint32_t>>& level);

// d_out[0] |= 1 when a coordinate is not finite or exceeds 1e18; d_out[1..3] = ordered keys (rf::order_key) of the max x, y, z; d_out[4..6] =
// the complements of the min keys.  d_out (7 words) must be zeroed before the launch.  Scene: the bounds of all vertices.
void launch_check_vertices(const float* d_verts, uint32_t n_vertices, uint32_t* d_out, hipStream_t stream);
constexpr uint32_t kCheckChunk = 4096;      // vertices and triangles per block of the mesh check
// The n meshes of a call: every coordinate checked as above, every index below n_vertices, and the box of the referenced vertices.
// One block per chunk: d_chunk_start[k] = first block of mesh k (d_chunk_start[0] = 0); d_out: 8 words per mesh, zeroed before the launch.
void launch_check_meshes(const RefitMesh* d_meshes, const uint32_t* d_chunk_start, uint32_t n, uint32_t n_chunks, uint32_t* d_out,
                         hipStream_t stream);
// records at `rows` float4 per item: entries [0, count) of the segments, regathered in place from their mesh's index entry (key_word 3 or 7)
void launch_refit_records(void* d_recs, uint32_t rows, uint32_t n_recs, const RefitSeg* d_segs, uint32_t n_segs, uint32_t count,
                          const RefitMesh* d_meshes, hipStream_t stream);
// d_idx[3i .. 3i + 2] = (2i, 2i + 1, 2i), i < n: a box array (lo, hi per item) as a refit mesh of 2n vertices
void launch_box_triples(int32_t* d_idx, uint32_t n, hipStream_t stream);
// one level of each tree (d_order: its node indices); call deepest level first
void launch_refit_bvh2_level(void* d_flat, uint32_t n2, const uint32_t* d_order, uint32_t count, const void* d_tris, uint32_t n_slots,
                             const float* d_verts, hipStream_t stream);
// one node8 level: entries [0, count) of the segments are positions in d_order, whose nodes lie in [node_base, n_nodes); d_box8: 6 floats
// per node8 (index node - node_base), the float box the parent's slot reads
void launch_refit_node8_level(void* d_nodes, uint32_t node_rows, uint32_t node_base, uint32_t n_nodes, const uint32_t* d_order,
                              const RefitSeg* d_segs, uint32_t n_segs, uint32_t count, const void* d_recs, uint32_t tri_rows, uint32_t n_recs,
                              const RefitMesh* d_meshes, float* d_box8, hipStream_t stream);

// ---- SAH cost of a tree, rebuild support (refit.hip) ----
// crt_tree_cost of the node8s [first, first + count) of a device array at node_rows 16-byte rows per node, `root` among them (count == 0:
// all zeros).  Allocates its partial sums, runs on `stream` and waits for it.
int tree_cost_on_device(const void* d_nodes, uint32_t node_rows, uint64_t first, uint64_t count, uint64_t root, hipStream_t stream,
                        crt_tree_cost* out);
// d_src[id] = d_slot_tris[slot] for the (id, slot) every CWBVH-order record of a device-built scene names (v0.w, e1.w): the source-order
// triangle array crt_scene_create's build-on-device path read and threw away
void launch_scatter_source(const void* d_recs, uint32_t tri_rows, uint32_t n, const crt_triangle* d_slot_tris, crt_triangle* d_src, hipStream_t stream);

// ---- code-object warm-up (crt_warmup) ----
// HIP loads a code object the first time one of its kernels is looked up; each of these asks for the attributes of its
// translation unit's kernels, which loads that unit's code object on the current device (~ms each) without launching anything.
int warm_lbvh_kernels();
int warm_cwbvh_kernels();
int warm_scene_build_kernels();
int warm_instance_kernels();

}  // namespace crt
