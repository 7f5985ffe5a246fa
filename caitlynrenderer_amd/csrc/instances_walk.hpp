// The two-level walk of instanced scenes: what its loop (instances_walk_loop.hpp) calls.  k_trace_instances
// (explicit rays) and the frame path's queue-fed kernels (k_closest_instances_queue, k_shadow_instances_deferred) are that one loop with
// different sources and sinks.
//
// The walk is ONE loop with ONE stack per lane.  TLAS and BLAS nodes are the same node8 format in the same array, so a wave whose lanes
// are at different levels still runs a single node step together.  A TLAS leaf's "triangles" are instances: the instance step pushes
// what the lane still has pending at the TLAS level (inner hits, the rest of the leaf), then a return marker, moves the ray into object
// space and continues at the BLAS root.  Popping the marker restores the world ray, which the lane keeps in registers.
// The masked walk (MASK) culls TLAS children whose instances are all hidden from the ray and skips hidden instances.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_math.hpp"
#include "rt_traverse.hpp"

namespace crt {

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

}  // namespace crt
