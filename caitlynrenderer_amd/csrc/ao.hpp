// Ambient occlusion (include/crt.h at crt_render_ao): the argument blocks and launchers of its kernels, and — for the two
// units that hold them, rt_kernels.hip and instances.hip — the generator of a point's occlusion rays.  A ray exists only in the registers of
// the lane that walks it: the any-hit walk builds ray e = (point e / K, sample e % K) where it loads it, an unoccluded ray sets bit k of its
// point's visibility words, and the fold (one lane per point) re-derives the directions of the set bits in k order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.hpp"

namespace crt {

struct AoGen {                 // what every AO kernel knows of the call
    const float4* points;      // 2 rows per point: (p, seed_x) (n, seed_y)
    uint32_t n;                // points
    uint32_t K;                // samples per point, 1..256; n * K < 2^32
    uint32_t words;            // visibility words per point: ceil(K / 32)
    float rv, radius, offset;
};

struct AoWalkArgs {            // k_ao_walk: a flat scene
    const uint4* nodes;
    const float4* tris;
    AoGen g;
    uint32_t* vis;             // n x words, zero at launch
    uint32_t stack_entries, refill_min, tri_min, pool, lanes_log2;
    uint32_t* overflow;
};

// k_ao_walk_instances: the member names the two-level walk reads (instances_walk_loop.hpp) are InstTraceArgs'
struct InstAoArgs {
    const uint4* nodes;
    const float4* tris;
    const float4* inst;
    const uint2* child_masks;  // the unmasked kernel reads neither: null / 0
    uint32_t n_tlas8;
    AoGen g;
    uint32_t* vis;
    uint32_t n_instances, stack_entries, refill_min, tri_min;
    uint32_t* overflow;
};
struct InstMaskAoArgs : InstAoArgs { uint32_t ray_mask; };

struct AoViewArgs {            // k_ao_view_points: the points of a view from its first hits
    FrameArgs f;
    const float4* hit;         // crt_render_aov's HIT and NORMAL values of the view, in buffers of the AO state's own
    const float4* normal;
    float4* points;            // 2 rows per pixel, linear pixel order
    uint32_t n_pixels;
};

void launch_ao_view_points(const AoViewArgs& a, hipStream_t stream);
void launch_ao_walk(const AoWalkArgs& a, hipStream_t stream);
void launch_ao_walk_instances(const InstMaskAoArgs& a, bool mask, hipStream_t stream);
void launch_ao_fold(const AoGen& g, const uint32_t* vis, float4* out, hipStream_t stream);

}  // namespace crt

#if defined(__HIPCC__) && defined(CRT_AO_DEVICE_MATH)
#include "rt_math.hpp"

namespace crt {

// steps 1 - 3 of the definition: what a point's rays share
struct AoFrame { vec3 o, nn, bu, bv; float seed_x, seed_y; };

__device__ __forceinline__ bool ao_frame(const AoGen& g, uint32_t point, AoFrame& fr) {
    const float4 r0 = g.points[2 * (size_t)point], r1 = g.points[2 * (size_t)point + 1];
    const vec3 p = V3(r0.x, r0.y, r0.z), n = V3(r1.x, r1.y, r1.z);
    fr.seed_x = r0.w; fr.seed_y = r1.w;
    const float l2 = dot(n, n);
    if (!(l2 > 0.0f) || !__builtin_isfinite(l2) || !__builtin_isfinite(p.x) || !__builtin_isfinite(p.y) || !__builtin_isfinite(p.z)) return false;
    const vec3 nn = n * rcp_ieee(sqrt_ieee(l2));
    fr.nn = nn;
    fr.o = p + nn * g.offset;
    if (nn.z < -0.9999999f) { fr.bu = V3(0.f, -1.f, 0.f); fr.bv = V3(-1.f, 0.f, 0.f); }
    else {
        const float a = rcp_ieee(1.0f + nn.z);
        const float b = (-nn.x * nn.y) * a;
        fr.bu = V3(1.0f - (nn.x * nn.x) * a, b, -nn.x);
        fr.bv = V3(b, 1.0f - (nn.y * nn.y) * a, -nn.y);
    }
    return true;
}

// step 5: the direction of sample k
__device__ __forceinline__ vec3 ao_direction(const AoFrame& fr, uint32_t k, float rv) {
    const float u1 = rand_at(fr.seed_x, fr.seed_y, 2u * k + 1u, rv), u2 = rand_at(fr.seed_x, fr.seed_y, 2u * k + 2u, rv);      // step 4
    const float r = sqrt_ieee(u1);
    const float phi = 6.2831853f * u2;
    const float sx = r * pinned_cos(phi), sy = r * pinned_sin(phi), sz = sqrt_ieee(1.0f - u1);
    return (fr.bu * sx + fr.bv * sy) + fr.nn * sz;
}

// ray e of the call; false = its point has no rays (step 1)
__device__ __forceinline__ bool ao_ray(const AoGen& g, uint32_t e, vec3& o, vec3& d) {
    const uint32_t point = e / g.K, k = e - point * g.K;
    AoFrame fr;
    if (!ao_frame(g, point, fr)) return false;
    o = fr.o;
    d = ao_direction(fr, k, g.rv);
    return true;
}

// ray e was found unoccluded
__device__ __forceinline__ void ao_mark_visible(const AoGen& g, uint32_t* vis, uint32_t e) {
    const uint32_t point = e / g.K, k = e - point * g.K;
    atomicOr(vis + (size_t)point * g.words + (k >> 5), 1u << (k & 31u));
}

}  // namespace crt
#endif
