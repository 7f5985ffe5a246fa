// Per-call tables and launchers of the BLAS refit of crt_instances_update_meshes (instances_refit.hip), shared with crt_instances.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crt {

// one updated mesh of a call: its new positions (device) and its slice of the source-order index array
struct InstRefitMesh {
    const float* verts;        // xyz per vertex, the create's order
    uint32_t n_vertices, n_tris;
    uint32_t tri_off;          // first triangle of the mesh in the index array and in the record array
    uint32_t pad;
};
static_assert(sizeof(InstRefitMesh) == 24, "InstRefitMesh is 24 bytes");

// a run of `count` entries of one mesh: entries [start, next start) of the launch are items first .. of the array it covers (records,
// or positions in the node8 level order)
struct InstRefitSeg { uint32_t start, first, slot, pad; };

constexpr uint32_t kCheckChunk = 4096;      // vertices and triangles per block of the check kernel

// one block per chunk: d_chunk_start[k] = first block of call mesh k (n entries, d_chunk_start[0] = 0); d_out: 8 words per call mesh,
// zeroed before the launch ([0] |= 1 bad coordinate, [1..3] max keys, [4..6] complemented min keys of the referenced vertices)
void launch_inst_check(const InstRefitMesh* d_meshes, const uint32_t* d_chunk_start, uint32_t n, uint32_t n_chunks, const int32_t* d_src_idx,
                       uint32_t* d_out, hipStream_t stream);
void launch_inst_refit_records(float4* d_recs, uint32_t n_recs, const InstRefitSeg* d_segs, uint32_t n_segs, uint32_t count,
                               const InstRefitMesh* d_meshes, const int32_t* d_src_idx, hipStream_t stream);
// one depth level of every updated BLAS (call deepest first); d_box8: 6 floats per BLAS node8, index node - node_base
void launch_inst_refit_node8_level(void* d_nodes, uint32_t node_base, uint32_t n_nodes, const uint32_t* d_order, const InstRefitSeg* d_segs,
                                   uint32_t n_segs, uint32_t count, const float4* d_recs, uint32_t n_recs, const InstRefitMesh* d_meshes,
                                   const int32_t* d_src_idx, float* d_box8, hipStream_t stream);

}  // namespace crt
