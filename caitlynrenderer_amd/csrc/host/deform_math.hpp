// Arithmetic of the deformer (include/crt.h crt_deformer_create), shared by the host entry (crt_deform_host) and the
// kernel of deform.hip, so that both give the same bits.  fp32 throughout, nothing fused (-ffp-contract=off on both sides), products
// rounded before sums, IEEE square root and division.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define CRT_DEFORM_HD __host__ __device__ inline
#else
#define CRT_DEFORM_HD inline
#endif

namespace crt {
namespace dm {

#if defined(__HIP_DEVICE_COMPILE__)
// llvm.sqrt.f32 and the division are expanded to their correctly rounded forms (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt)
#define CRT_DEFORM_SQRT(x) __builtin_sqrtf(x)
#define CRT_DEFORM_DIV(a, b) __fdiv_rn((a), (b))
#else
#define CRT_DEFORM_SQRT(x) sqrtf(x)
#define CRT_DEFORM_DIV(a, b) ((a) / (b))
#endif

// Morph, one listed delta: p.c = p.c + w * d.c
CRT_DEFORM_HD void morph_add(float p[3], float w, const float d[3]) {
    for (int c = 0; c < 3; ++c) p[c] = p[c] + w * d[c];
}

// Blend, the first influence: M_j = w_0 * B[b_0][j]
CRT_DEFORM_HD void blend_first(float M[12], float w, const float B[12]) {
    for (int j = 0; j < 12; ++j) M[j] = w * B[j];
}
// Blend, influences 1..3; the caller has tested w != 0
CRT_DEFORM_HD void blend_add(float M[12], float w, const float B[12]) {
    for (int j = 0; j < 12; ++j) M[j] = M[j] + w * B[j];
}

CRT_DEFORM_HD void skin_position(const float M[12], const float p[3], float out[3]) {
    for (int r = 0; r < 3; ++r) out[r] = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
}

// the linear part of M on n, brought to unit length where its squared length is a normal, finite float
CRT_DEFORM_HD void skin_normal(const float M[12], const float n[3], float out[3]) {
    float q[3];
    for (int r = 0; r < 3; ++r) q[r] = (M[4 * r] * n[0] + M[4 * r + 1] * n[1]) + M[4 * r + 2] * n[2];
    const float l2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    if (l2 >= 0x1p-126f && l2 <= 3.402823466e38f) {          // NaN fails both
        const float l = CRT_DEFORM_SQRT(l2);
        for (int r = 0; r < 3; ++r) out[r] = CRT_DEFORM_DIV(q[r], l);
    } else {
        for (int r = 0; r < 3; ++r) out[r] = q[r];
    }
}

}  // namespace dm
}  // namespace crt
