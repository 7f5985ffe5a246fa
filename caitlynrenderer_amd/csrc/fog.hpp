// Fog with light shafts (include/crt.h at crt_render_fog): the argument blocks and launchers of its kernels, and — for the two
// units that hold them, rt_kernels.hip and instances.hip — the generator of a segment's shadow rays.  A ray exists only in the registers of
// the lane that walks it: the any-hit walk builds ray e = (segment e / K, sample e % K) where it loads it, an unoccluded ray sets bit j of
// its segment's visibility words, and the fold (one lane per segment) re-derives the samples of the set bits in j order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.hpp"

namespace crt {

struct FogGen {                // what every fog kernel knows of the call
    const float4* segments;    // 2 rows per segment: (o, seed_x) (e, seed_y)
    const float* lights;       // the table a frame reads: 18 floats per light
    int32_t n_lights;
    uint32_t n;                // segments
    uint32_t K;                // samples per segment, 1..256; n * K < 2^32
    uint32_t words;            // visibility words per segment: ceil(K / 32)
    float rv, sigma, g;
    float albedo[3], ambient[3];
};

struct FogWalkArgs {           // k_fog_walk: a flat scene
    const uint4* nodes;
    const float4* tris;
    FogGen g;
    uint32_t* vis;             // n x words, zero at launch
    uint32_t stack_entries, refill_min, tri_min, pool, lanes_log2;
    uint32_t* overflow;
};

// k_fog_walk_instances: the member names the two-level walk reads (instances_walk_loop.hpp) are InstTraceArgs'
struct InstFogArgs {
    const uint4* nodes;
    const float4* tris;
    const float4* inst;
    const uint2* child_masks;  // the unmasked kernel reads neither: null / 0
    uint32_t n_tlas8;
    FogGen g;
    uint32_t* vis;
    uint32_t n_instances, stack_entries, refill_min, tri_min;
    uint32_t* overflow;
};
struct InstMaskFogArgs : InstFogArgs { uint32_t ray_mask; };

struct FogViewArgs {           // k_fog_view_segments: the segments of a view from its first hits
    FrameArgs f;
    const float4* hit;         // crt_render_aov's HIT values of the view, in a buffer of the fog state's own
    float4* segments;          // 2 rows per pixel, linear pixel order
    uint32_t n_pixels;
    float max_distance;
};

struct FogCompositeArgs {      // k_fog_composite: out = c * TD + S
    const float* image;        // width * height * 3, linear pixel order
    const float4* fog;         // crt_render_fog's image
    float* out;
    uint32_t n_pixels;
    uint32_t scale;            // 1 = the running sum: c = image * inv_count
    float inv_count;
};

void launch_fog_view_segments(const FogViewArgs& a, hipStream_t stream);
void launch_fog_walk(const FogWalkArgs& a, hipStream_t stream);
void launch_fog_walk_instances(const InstMaskFogArgs& a, bool mask, hipStream_t stream);
void launch_fog_fold(const FogGen& g, const uint32_t* vis, float4* out, hipStream_t stream);
void launch_fog_composite(const FogCompositeArgs& a, hipStream_t stream);

}  // namespace crt

#if defined(__HIPCC__) && defined(CRT_FOG_DEVICE_MATH)
#include "rt_math.hpp"

namespace crt {

// step 1 of the definition: what a segment's samples share
struct FogFrame { vec3 o, dir; float D, h, seed_x, seed_y; };

__device__ __forceinline__ bool fog_frame(const FogGen& g, uint32_t segment, FogFrame& fr) {
    const float4 r0 = g.segments[2 * (size_t)segment], r1 = g.segments[2 * (size_t)segment + 1];
    const vec3 o = V3(r0.x, r0.y, r0.z), e = V3(r1.x, r1.y, r1.z);
    fr.seed_x = r0.w; fr.seed_y = r1.w;
    const float D2 = dot(e, e);
    if (!(D2 > 0.0f) || !__builtin_isfinite(D2) || !__builtin_isfinite(o.x) || !__builtin_isfinite(o.y) || !__builtin_isfinite(o.z)) return false;
    fr.o = o;
    fr.D = sqrt_ieee(D2);
    fr.dir = e * rcp_ieee(fr.D);
    fr.h = __fdiv_rn(fr.D, (float)g.K);
    return true;
}

// steps 3 and 4: sample j's point on the segment and its light sample; false = the sample is dark
struct FogSample { vec3 x, ld; float s, ln, cos_light; const float* Lt; };

__device__ __forceinline__ bool fog_sample(const FogGen& g, const FogFrame& fr, uint32_t j, FogSample& sm) {
    if (g.n_lights <= 0) return false;
    const float u0 = rand_at(fr.seed_x, fr.seed_y, 4u * j + 1u, g.rv), r0 = rand_at(fr.seed_x, fr.seed_y, 4u * j + 2u, g.rv);
    const float r1 = rand_at(fr.seed_x, fr.seed_y, 4u * j + 3u, g.rv), r2 = rand_at(fr.seed_x, fr.seed_y, 4u * j + 4u, g.rv);
    sm.s = ((float)j + u0) * fr.h;
    sm.x = fr.o + fr.dir * sm.s;
    int li = (int)(r0 * (float)g.n_lights);
    if (li > g.n_lights - 1) li = g.n_lights - 1;
    const float* Lt = g.lights + 18 * (size_t)li;
    sm.Lt = Lt;
    const float sq = sqrt_ieee(r1);
    const float b0 = 1.0f - sq;
    const float b1 = r2 * sq;
    const vec3 pos = (V3(Lt[0], Lt[1], Lt[2]) + V3(Lt[3], Lt[4], Lt[5]) * b0) + V3(Lt[6], Lt[7], Lt[8]) * b1;
    vec3 ld = pos - sm.x;
    sm.ln = length(ld);
    ld = ld * rcp_ieee(sm.ln);
    sm.ld = ld;
    sm.cos_light = dot(ld, V3(Lt[9], Lt[10], Lt[11]));
    return sm.cos_light < 0.0f;
}

// ray e of the call (step 5); false = no ray: its segment has none, or its sample is dark
__device__ __forceinline__ bool fog_ray(const FogGen& g, uint32_t e, vec3& o, vec3& d, float& tmax) {
    const uint32_t segment = e / g.K, j = e - segment * g.K;
    FogFrame fr;
    FogSample sm;
    if (!fog_frame(g, segment, fr) || !fog_sample(g, fr, j, sm)) return false;
    o = sm.x; d = sm.ld; tmax = sm.ln - 1e-4f;
    return true;
}

// ray e was found unoccluded.  (An entry without a ray ends as a miss and sets its bit too: the fold asks fog_sample again.)
__device__ __forceinline__ void fog_mark_visible(const FogGen& g, uint32_t* vis, uint32_t e) {
    const uint32_t segment = e / g.K, j = e - segment * g.K;
    atomicOr(vis + (size_t)segment * g.words + (j >> 5), 1u << (j & 31u));
}

// step 6: what an unoccluded sample adds
__device__ __forceinline__ vec3 fog_contribution(const FogGen& g, const FogFrame& fr, const FogSample& sm) {
    const float* Lt = sm.Lt;
    const float pdf = __fdiv_rn(sm.ln * sm.ln, Lt[15] * -sm.cos_light) * Lt[16];
    const float ct = dot(fr.dir, sm.ld);
    const float den = (1.0f + g.g * g.g) - (2.0f * g.g) * ct;
    const float ph = __fdiv_rn((1.0f - g.g * g.g) * 0.07957747f, den * sqrt_ieee(den));
    const float att = exp_neg(g.sigma * (sm.s + sm.ln));
    const float w = __fdiv_rn((att * ph) * (g.sigma * fr.h), pdf);
    return V3((Lt[12] * g.albedo[0]) * w, (Lt[13] * g.albedo[1]) * w, (Lt[14] * g.albedo[2]) * w);
}

}  // namespace crt
#endif
