// What a crt_scene whose geometry is a crt_instances handle (crt_scene_create_instanced) needs of that handle: its live
// device arrays, read when a frame is enqueued, and the binding that makes the handle's mutators wait for the scene's stream and refuse
// what would leave the scene's per-mesh shading tables stale.  crt_instances.cpp defines these; crt_device.cpp (creation), crt_frames.cpp (frames)
// and crt_outputs.cpp (AOVs) call them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crt.h"
#include "instances.hpp"

namespace crt {

struct InstancesView {
    int device;
    const uint4* nodes;        // the TLAS from node 0, then every BLAS
    const float4* tris;        // every BLAS's records
    const float4* inst;        // instance records in TLAS leaf order
    const float* w2o;          // world_to_object, 12 floats per instance, instance order
    const uint2* mesh_of;      // per instance: (mesh index, bit 31 = the matrix is bitwise the identity; material offset)
    const uint2* child_masks;  // per TLAS node8, for masked walks: fresh once instances_child_masks_for has been called
    uint32_t n_instances, stack_entries, n_meshes;
    uint32_t tlas_nodes8, tlas_depth8, max_blas_depth8;
    uint64_t blas_nodes8, blas_tris;
    const float* o2w;          // object_to_world, 12 floats per instance, instance order: what the light tables of DESIGN.md §18 move by
    uint32_t capacity;
    uint64_t mutations;        // successful sets, refits and mesh updates so far
};
void instances_view(const crt_instances* h, InstancesView* out);
uint32_t instances_mesh_triangles(const crt_instances* h, uint32_t mesh);     // mesh < n_meshes
// from now on sets, refits and updates of the handle first wait for `stream`; destroy, add_meshes and replace_meshes are refused
// and of every set / refit the material offsets are held to `rule` (device tables the scene keeps while bound); refused, with nothing
// bound, when the handle's live instances break it
int instances_bind(crt_instances* h, hipStream_t stream, const InstOffsetRule& rule);
// before a masked frame is enqueued on `stream`: the handle's TLAS child masks renewed if stale, and `stream` ordered behind that pass.
// *seen: the scene's note of the last pass it waited for (0 at first).  No host wait
int instances_child_masks_for(crt_instances* h, hipStream_t stream, uint64_t* seen);
void instances_unbind(crt_instances* h, hipStream_t stream);

}  // namespace crt
