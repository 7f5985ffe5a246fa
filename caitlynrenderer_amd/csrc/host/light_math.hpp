// Arithmetic of the lights that follow emissive instances (include/crt.h crt_scene_create_instanced_lit), shared by the
// host entry points (crt_instance_lights, crt_lights_finish) and the table kernels of instances.hip, so that both give the same bits.
// fp32 throughout, nothing fused (-ffp-contract=off on both sides), products rounded before sums, IEEE square root and division.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define CRT_LIGHT_HD __host__ __device__ inline
#else
#define CRT_LIGHT_HD inline
#endif

namespace crt {

#if defined(__HIP_DEVICE_COMPILE__) && defined(CRT_LIGHT_DEVICE_MATH)
// rt_math.hpp's correctly rounded forms: the kernels' translation unit includes it first and defines CRT_LIGHT_DEVICE_MATH
#define CRT_LIGHT_SQRT(x) ::crt::sqrt_ieee(x)
#define CRT_LIGHT_RCP(x) ::crt::rcp_ieee(x)
#else
#define CRT_LIGHT_SQRT(x) sqrtf(x)
#define CRT_LIGHT_RCP(x) (1.0f / (x))
#endif

// One object-space light (18 floats: p, u, v, n, e, (area, pdf, 0)) of an instance into world space.  A | t = the rows of
// object_to_world, W = world_to_object (its inverse transpose carries the normal: the light's side agrees with the shading normal of
// include/crt.h contract item 4, mirrors included).  identity: the instance's matrix is bitwise the identity: all 18 floats are copied.
CRT_LIGHT_HD void light_to_world(const float A[12], const float W[12], bool identity, const float* in, float* out) {
    if (identity) {
        for (int k = 0; k < 18; ++k) out[k] = in[k];
        return;
    }
    float u[3], v[3], m[3];
    for (int r = 0; r < 3; ++r) {
        out[r] = ((A[4 * r] * in[0] + A[4 * r + 1] * in[1]) + A[4 * r + 2] * in[2]) + A[4 * r + 3];
        u[r] = (A[4 * r] * in[3] + A[4 * r + 1] * in[4]) + A[4 * r + 2] * in[5];
        v[r] = (A[4 * r] * in[6] + A[4 * r + 1] * in[7]) + A[4 * r + 2] * in[8];
        m[r] = (W[r] * in[9] + W[4 + r] * in[10]) + W[8 + r] * in[11];
    }
    const float inv = CRT_LIGHT_RCP(CRT_LIGHT_SQRT((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]));
    const float c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    for (int r = 0; r < 3; ++r) {
        out[3 + r] = u[r];
        out[6 + r] = v[r];
        out[9 + r] = m[r] * inv;
        out[12 + r] = in[12 + r];
    }
    out[15] = CRT_LIGHT_SQRT((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    out[16] = 0.0f;
    out[17] = 0.0f;
}

// what a light's area counts for in the sum of the pdf column: itself when it is a finite positive float, else +0
CRT_LIGHT_HD float light_area_term(float a) { return (a > 0.0f && a <= 3.402823466e38f) ? a : 0.0f; }

// pdf of choosing a light of area term a when the terms sum to S (the loader's area / sum with the reciprocal taken once)
CRT_LIGHT_HD float light_pdf(float a, float S) { return S > 0.0f ? a * CRT_LIGHT_RCP(S) : 0.0f; }

}  // namespace crt
