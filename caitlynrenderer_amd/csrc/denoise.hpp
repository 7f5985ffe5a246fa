// crt_denoise's kernels (denoise.hip): an edge-avoiding a-trous wavelet filter over the un-tiled running sum, guided by the
// first-hit feature buffers of crt_render_aov.  Every arithmetic step is one IEEE float32 operation in a fixed order, so a float32 numpy
// restatement (tests/denoise_ref.py) gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crt {

struct DenoisePrepareArgs {
    const float* sum;            // the un-tiled sum: 3 floats per pixel, linear pixel order
    const float4* hit;           // CRT_AOV_HIT    (t, u, v, tri as bits)
    const int4* ids;             // CRT_AOV_IDS    (instance, mesh, material, flags)
    const float4* normal;        // CRT_AOV_NORMAL (n, 0), not normalised
    const float4* albedo;        // CRT_AOV_ALBEDO (rgb, 0)
    float4* g;                   // out: (unit normal, t); zeros for a pixel that is not filterable
    float4* x;                   // out: (x, key as bits); (c, 0) for a pixel that is not filterable
    uint32_t n_pixels;
    float inv_count;
    uint32_t demodulate;
};

struct DenoisePassArgs {
    const float4* g;
    const float4* x_in;
    float4* x_out;               // passes before the last
    float* out;                  // the last pass: 3 floats per pixel, x times the divisor
    const float4* albedo;        // the last pass with demodulate: the divisor is recomputed from it
    uint32_t width, height;
    uint32_t step_log2;          // tap spacing s = 1 << step_log2
    float inv_c;                 // 1 / (sigma_i * sigma_i); unused when use_color is 0
    float sigma_depth;
    uint32_t use_color;
    uint32_t normal_squarings;
    uint32_t demodulate;
};

void launch_denoise_prepare(const DenoisePrepareArgs& a, hipStream_t stream);
// form: 0 = the build's choice (per tap spacing as measured), 1 = taps staged in LDS, 2 = taps from global memory; the same bytes
void launch_denoise_pass(const DenoisePassArgs& a, bool last, uint32_t form, hipStream_t stream);
int warm_denoise_kernels();      // crt_warmup: loads this unit's code object on the current device

}  // namespace crt
