// Per-instance arithmetic of instanced scenes (include/crt.h, crt_instances_*), shared by the host entry points
// (crt_instance_inverse, crt_instance_world_box) and the device prep kernel of instances.hip, so that both give the same bits.
// Both sides are compiled with -ffp-contract=off: nothing below is fused.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define CRT_INST_HD __host__ __device__ inline
#else
#define CRT_INST_HD inline
#endif

namespace crt {

CRT_INST_HD bool inst_finite(double x) { return x == x && x - x == 0.0; }      // false for NaN and +-inf

// world_to_object of a row-major 3x4 object_to_world (world = A * p + t): the adjugate of A divided by det(A) (a division, not a
// multiply by 1 / det), det expanded along the first row in the order written, translation 0 - (W_A . t); all in double from the
// unrounded entries, each result rounded once to float.  Returns false (and leaves w untouched) when an input entry is not finite,
// det is 0 or not finite, or a rounded entry is not finite.
CRT_INST_HD bool instance_inverse(const float m[12], float w[12]) {
    for (int k = 0; k < 12; ++k) if (!inst_finite((double)m[k])) return false;
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double t0 = m[3], t1 = m[7], t2 = m[11];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double det = (a * c00 + b * c01) + c * c02;
    if (det == 0.0 || !inst_finite(det)) return false;
    const double adj[9] = {c00, c * h - b * i, b * f - c * e,
                           c01, a * i - c * g, c * d - a * f,
                           c02, b * g - a * h, a * e - b * d};
    double r[12];
    for (int row = 0; row < 3; ++row) {
        const double x = adj[3 * row] / det, y = adj[3 * row + 1] / det, z = adj[3 * row + 2] / det;
        r[4 * row] = x; r[4 * row + 1] = y; r[4 * row + 2] = z;
        r[4 * row + 3] = 0.0 - ((x * t0 + y * t1) + z * t2);       // 0 - (not a negation): the identity maps to +0, not -0
    }
    float out[12];
    for (int k = 0; k < 12; ++k) {
        out[k] = (float)r[k];
        if (!inst_finite((double)out[k])) return false;
    }
    for (int k = 0; k < 12; ++k) w[k] = out[k];
    return true;
}

// object_to_world bitwise the identity: the walk then uses the world ray as it is (no arithmetic: signs of zeros and non-finite
// components stay exactly those of a flat trace)
CRT_INST_HD bool instance_is_identity(const float m[12]) {
    for (int k = 0; k < 12; ++k) {
        uint32_t u;
        memcpy(&u, &m[k], 4);
        if (u != ((k == 0 || k == 5 || k == 10) ? 0x3f800000u : 0u)) return false;
    }
    return true;
}

// Relative margin of a world box: 2^-16 of the largest absolute coordinate of the transformed box (DESIGN.md §11 sizes it).  A build switch
// only so that a variant library can show what the grazing-ray test sees without it (make EXTRA="-DCRT_INSTANCE_BOX_MARGIN=0.0").
#ifndef CRT_INSTANCE_BOX_MARGIN
#define CRT_INSTANCE_BOX_MARGIN 0x1p-16
#endif

// float nearest to x rounded toward -inf (down) or +inf (up)
CRT_INST_HD float inst_round_out(double x, bool up) {
    float f = (float)x;
    if (up ? (double)f < x : (double)f > x) {
        uint32_t u;
        memcpy(&u, &f, 4);
        if (f == 0.0f) u = up ? 0x00000001u : 0x80000001u;
        else if ((f > 0.0f) == up) ++u;
        else --u;
        memcpy(&f, &u, 4);
    }
    return f;
}

// World box of an instance: the 8 corners of the object box (lo[3], hi[3] in box[6]) through object_to_world in double, their bounds
// widened by CRT_INSTANCE_BOX_MARGIN x the largest absolute coordinate and rounded outward to float.  out = (lo[3], hi[3]).
CRT_INST_HD void instance_world_box(const float m[12], const float box[6], float out[6]) {
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 8; ++k) {
        const double p[3] = {(double)box[(k & 1) ? 3 : 0], (double)box[(k & 2) ? 4 : 1], (double)box[(k & 4) ? 5 : 2]};
        for (int r = 0; r < 3; ++r) {
            const double q = (((double)m[4 * r] * p[0] + (double)m[4 * r + 1] * p[1]) + (double)m[4 * r + 2] * p[2]) + (double)m[4 * r + 3];
            if (k == 0 || q < lo[r]) lo[r] = q;
            if (k == 0 || q > hi[r]) hi[r] = q;
        }
    }
    double big = 0.0;
    for (int r = 0; r < 3; ++r) {
        const double a = lo[r] < 0.0 ? -lo[r] : lo[r], b = hi[r] < 0.0 ? -hi[r] : hi[r];
        if (a > big) big = a;
        if (b > big) big = b;
    }
    const double pad = big * CRT_INSTANCE_BOX_MARGIN;
    for (int r = 0; r < 3; ++r) {
        out[r] = inst_round_out(lo[r] - pad, false);
        out[3 + r] = inst_round_out(hi[r] + pad, true);
    }
}

}  // namespace crt
