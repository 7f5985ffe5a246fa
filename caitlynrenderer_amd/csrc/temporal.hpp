// crt_temporal's kernel (temporal.hip): temporal accumulation by reprojection.  Each pixel's first-hit point is carried into
// the previous call's view (through the instance's previous transform where it moved), the previous result is gathered there from four
// taps that show the same surface, and the source is blended into it.  Every arithmetic step is one IEEE float32 operation in a fixed
// order, so a float32 numpy restatement (tests/temporal_ref.py) gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crt {

// a view as crt_render_aov rendered it: the camera and what FrameArgs carries of the frame
struct TemporalView {
    float pos[3], right[3], up[3], fwd[3];
    float aspect_tan, tan_fov;   // formed where FrameArgs' are formed
    float rv;                    // rx * ry of the call: the seed of the jitter draws
    uint32_t jitter;
};

struct TemporalArgs {
    const float* src;            // the source image, 3 floats per pixel, linear pixel order
    const float4* hit;           // CRT_AOV_HIT    (t, u, v, tri as bits)
    const int4* ids;             // CRT_AOV_IDS    (instance, mesh, material, flags)
    const float4* normal;        // CRT_AOV_NORMAL (n, 0), not normalised
    const float4* albedo;        // CRT_AOV_ALBEDO (rgb, 0)
    const float4* hist_in;       // the previous call's (y, N)
    const float4* guide_in;      // the previous call's (unit normal, t)
    const uint32_t* key_in;      // the previous call's key
    float4* hist_out;
    float4* guide_out;
    uint32_t* key_out;
    float* out;                  // y times the divisor, 3 floats per pixel
    const float* o2w;            // an instanced scene's live object_to_world, 12 floats per instance; null = a flat scene
    const float* w2o;            // its live world_to_object
    const float* o2w_prev;       // object_to_world as of the previous call
    uint32_t n_instances, n_prev_instances;
    uint32_t width, height;
    float inv_count;
    uint32_t scale_source;       // 1: c = src * inv_count (source SUM); 0: c = src (source DENOISED)
    uint32_t demodulate, clamp;
    uint32_t has_history;        // 0: every pixel takes y = x, N = 1 and no previous buffer is read
    float max_history, sigma_depth, normal_min;
    TemporalView cur, prev;
};

// form: 0 = the build's choice, 1 = the CLAMP neighbourhood staged in LDS, 2 = read from global memory; the same bytes.  Without CLAMP
// (or without history) there is no neighbourhood and the forms are one kernel
void launch_temporal(const TemporalArgs& a, uint32_t form, hipStream_t stream);
int warm_temporal_kernels();     // crt_warmup: loads this unit's code object on the current device

}  // namespace crt
