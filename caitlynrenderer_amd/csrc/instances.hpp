// Kernel argument blocks and launchers of instanced scenes (instances.hip), shared with crt_instances.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crt.h"

namespace crt {

// Traversal-stack entries of the two-level walk: TLAS depth + deepest BLAS depth; create and set refuse more.
#define CRT_INST_STACK_ENTRIES 40

struct InstTraceArgs {
    const uint4* nodes;        // ONE node8 array (5 x 16 B each): the TLAS from node 0, then every BLAS (child / triangle bases rebased)
    const float4* tris;        // ONE record array (3 x 16 B each): every BLAS's records, (v0 | id in its mesh) (e1 | slot) (e2 | material)
    const float4* inst;        // 4 x 16 B per TLAS leaf slot: world_to_object rows 0..2, (BLAS root node, instance index, identity, 0)
    const float4* rays;        // crt_ray
    float4* hits;              // crt_hit
    int32_t* inst_out;         // instance of the hit, -1 = miss (may be null)
    uint32_t* stats;           // optional: nodes | tris << 16
    uint32_t n, n_instances, stack_entries, refill_min, tri_min;
    uint32_t* overflow;        // += 1 per dropped stack push (never happens for a depth create / set accepted)
};
// The masked walk's arguments (CRT_TRACE_INSTANCE_MASK).  A type of its own, so that the unmasked kernels keep their
// argument block, and with it their code, exactly as before.
struct InstMaskTraceArgs : InstTraceArgs {
    const uint2* child_masks;  // 8 B per TLAS node8: byte i = OR of the masks of every instance under meta slot i
    uint32_t n_tlas8;          // live TLAS node8s: node steps below this index are TLAS steps
};

struct InstPrepArgs {
    const uint32_t* in;        // crt_instance array, 16 words each
    uint32_t n, n_meshes;
    const float* mesh_box;     // 6 floats per mesh: the exact float box of its vertices
    const uint32_t* mesh_root; // BLAS root node of each mesh in the shared node array
    float4* rec;               // 4 rows per instance, instance order (row 3: BLAS root, instance index, identity flag, mask & 0xff)
    float* box;                // 6 floats per instance: world box
    float* w2o;                // 12 floats per instance: world_to_object
    uint32_t* flag;            // |= 1 matrix not finite / singular / inverse not finite, 2 mesh index out of range, 4 world box beyond 1e18
    uint2* mesh_of;            // x: the instance's mesh index, bit 31 = the identity flag (what a frame's shading looks the hit triangle up by;
                               // DESIGN.md §16), y: crt_instance.material_offset (what it adds to the triangle's material; §17)
    float* o2w;                // 12 floats per instance: object_to_world as given (what the light tables of §18 transform by)
};
// What a scene bound to the handle admits as material offsets (crt_scene_create_instanced's validation rule)
struct InstOffsetRule {
    const uint4* mesh_mtl;     // per mesh: least and greatest v[3] of its triangles, 1 = every vt indexes the mesh's texcoords, 0
    const uint32_t* tex_before;// n_materials + 1 words: the textured materials below each index
    uint32_t n_materials;
};
struct InstOffsetCheckArgs {   // k_instance_offsets: the rule against n instances' (mesh, offset) words
    const uint2* mesh_of;
    uint32_t n, n_meshes;
    InstOffsetRule rule;
    uint32_t* flag;            // [0] |= 8 offset out of range, 16 offset onto a textured material without texcoords; [1] min= the instance
};

// The frame path of an instanced scene (crt_scene_create_instanced): the two-level walk fed by a frame's device-written
// ray queues.  The member names the walk reads (instances_walk.hpp) are InstTraceArgs'.
struct InstQueueArgs {         // k_closest_instances_queue: closest hits of a segment's path-ray queue
    const uint4* nodes;
    const float4* tris;
    const float4* inst;
    const uint2* child_masks;  // the unmasked kernels read neither: null / 0.  The masked ones (InstMaskQueueArgs): as InstMaskTraceArgs
    uint32_t n_tlas8;
    const float4* rays;        // 8 sub-queues of crt_ray, sub_capacity entries each
    const uint32_t* count;     // 8 device-side counts, CRT_COUNTER_STRIDE apart
    float4* hits;              // parallel to the queue: (t, u, v, triangle id within the hit instance's mesh)
    int32_t* hit_inst;         // parallel to the queue: the hit's instance, -1 = miss
    uint32_t sub_capacity, n_instances, stack_entries, refill_min, tri_min;
    unsigned long long* visit_totals;   // counting frames: [0] += node steps, [1] += triangle tests
    uint32_t* overflow;
};
// The masked walks of a frame (option "instance_masks").  Types of their own, as InstMaskTraceArgs, so that the unmasked
// kernels keep their argument blocks and code.  ray_mask: the launch's ONE ray mask (0..255) — in the queues the rays' w words are the
// path index and the contribution slot — wave-uniform, a scalar operand of both mask tests.
struct InstMaskQueueArgs : InstQueueArgs { uint32_t ray_mask; };
struct InstShadowArgs {        // k_shadow_instances_deferred: the frame's deferred NEE shadow rays, every segment's in one launch
    const uint4* nodes;
    const float4* tris;
    const float4* inst;
    const uint2* child_masks;  // as InstQueueArgs: null / 0
    uint32_t n_tlas8;
    const float4* shadow;      // [region][8 sub-queues][sub_capacity] x 2 float4: (o, tmax) (d, contribution slot)
    const uint32_t* count;     // region r, group g: count[r * count_stride + g * CRT_COUNTER_STRIDE]
    float4* contrib;           // n_slots contribution slots; an occluded ray clears its slot's visibility word
    uint32_t n_slots, count_stride, pools_per_region, n_regions;
    uint32_t sub_capacity, n_instances, stack_entries, refill_min, tri_min;
    unsigned long long* visit_totals;
    uint32_t* overflow;
};

struct InstMaskShadowArgs : InstShadowArgs { uint32_t ray_mask; };

// The world light table of a scene with mesh lights (crt_scene_create_instanced_lit), rebuilt from the handle's live arrays.
struct LightTableArgs {
    const uint2* mesh_of;      // live, per instance: (mesh | identity bit 31, material offset)
    const float* o2w;          // live object_to_world, 12 floats per instance
    const float* w2o;          // live world_to_object
    const uint2* mesh_lights;  // per mesh: (first light in obj_lights, count)
    const float* obj_lights;   // every mesh's object-space lights, 18 floats each
    const float* static_lights;// n_static world lights as given at create
    uint32_t n_instances, n_meshes, n_static;
    uint32_t* first;           // per instance: table index of its first light (n_static + exclusive prefix sum of the counts)
    uint32_t* block_sums;      // one word per 1024 instances
    uint32_t* total;           // [0] = lights of all instances (without n_static)
    float* table;              // n_total x 18 floats
    uint32_t n_total;
    float* partial;            // the tree sum's partials: two regions of ceil(n_total / 256) floats
};
// per-instance counts and their exclusive scan into first[] (+ n_static), the total into total[0].  Enqueued only
void launch_light_scan(const LightTableArgs& a, hipStream_t stream);
// with a.n_total known (n_static + total[0]): every table entry, then the tree sum of the areas and the pdf column.  Enqueued only
void launch_light_table(const LightTableArgs& a, hipStream_t stream);

void launch_instance_prep(const InstPrepArgs& a, hipStream_t stream);
void launch_instance_offsets(const InstOffsetCheckArgs& a, hipStream_t stream);
// node8 i: child_base_index += node_off, triangle_base_index += tri_off
void launch_rebase_nodes(void* d_nodes, uint32_t n8, uint32_t node_off, uint32_t tri_off, hipStream_t stream);
// d_dst node8 i = d_src node8 i with child_base_index += node_delta, triangle_base_index += tri_delta (wrapped differences new - old
// offset).  d_src and d_dst must not overlap
void launch_move_nodes(const void* d_src, void* d_dst, uint32_t n8, uint32_t node_delta, uint32_t tri_delta, hipStream_t stream);
// d_dst[i] = d_src[i] + delta, i < n: a BLAS's level order (global node indices) after its move.  No overlap either
void launch_move_order(const uint32_t* d_src, uint32_t* d_dst, uint32_t n, uint32_t delta, hipStream_t stream);
// the BVH2 of ONE box: a leaf root holding slot 0
void launch_single_leaf(const float* d_box, crt_flatnode* d_flat, uint32_t* d_tri_order, hipStream_t stream);
// out[i] = rec[tri_order[tri_slots[i]]] (4 rows): the instance records in CWBVH leaf order
void launch_gather_instances(const float4* d_rec, const uint32_t* d_tri_order, const int32_t* d_tri_slots, uint32_t n, float4* d_out, hipStream_t stream);
// in place, i < n: inst[i] = rec[inst[i] row 3 .y] (4 rows): the live TLAS leaf order kept, each record renewed (crt_instances_refit)
void launch_regather_instances(const float4* d_rec, uint32_t n, float4* d_inst, hipStream_t stream);
// TLAS child masks of the live TLAS (n8 node8s from node 0 of d_nodes, n >= 1 instance records in leaf order): per node8 its 8 bytes
// zeroed and the links (node << 3 | meta slot) of its children written, then each instance's mask ORed into every ancestor slot.
// parent: n8 words, leaf_of: n words.  Enqueued only.
void launch_tlas_child_masks(const void* d_nodes, uint32_t n8, const float4* d_inst, uint32_t n, uint32_t* d_parent, uint32_t* d_leaf_of,
                             uint2* d_child_masks, hipStream_t stream);
// `chunks`: 1024-ray chunks of the dense index space (k_trace's mapping), a multiple of 8; mask: CRT_TRACE_INSTANCE_MASK walk
void launch_trace_instances(const InstMaskTraceArgs& a, int any, bool stats, bool mask, uint32_t chunks, hipStream_t stream);
// one single-wave workgroup per 64 entries a sub-queue can hold; LDS = stack_entries x 512 B
// mask: the masked walk with a.ray_mask (child_masks, n_tlas8 set); else those three are not read
void launch_closest_instances_queue(const InstMaskQueueArgs& a, bool stats, bool mask, hipStream_t stream);
void launch_shadow_instances_deferred(const InstMaskShadowArgs& a, bool stats, bool mask, hipStream_t stream);

}  // namespace crt
