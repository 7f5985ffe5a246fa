// The per-slot pieces of the SAH cost of a CWBVH (include/crt.h crt_tree_cost).  Compiled for the host function
// (host/cost.cpp, g++) and for the device kernel (refit.hip, gfx950): a slot's corners are decoded in fp32 as the walk sees them, each
// rounded once, and everything after that is double arithmetic without contraction, so both sides compute every slot's area to the
// same bits and differ only in the order they add the areas up.
#pragma once
#include <stdint.h>

#include "../../../include/crt.h"
#include "refit_core.hpp"

namespace crt {
namespace tc {

constexpr double kNodeStep = 233.0, kTriangleTest = 71.0;    // profiles/isa_counts.json: a general node step, a triangle test

// 2^(e-127) as a float: the walk's scale for every exponent the converter writes (1..254); e = 0 is the subnormal 2^-127
CRT_HD float scale_of(uint8_t e) { return cw::u2f(e ? (uint32_t)e << 23 : 0x00400000u); }

// corner = p + q * 2^(e-127): the product is exact (8 bits times a power of two), the sum rounds once
CRT_HD float corner(float p, uint8_t q, float scale) { return p + (float)q * scale; }

// the six planes of slot s of a node8 given as its 80 bytes
CRT_HD rf::Box slot_box(const uint8_t* node, int s) {
    float p[3];
    __builtin_memcpy(p, node, sizeof p);
    rf::Box b;
    for (int k = 0; k < 3; ++k) {
        const float scale = scale_of(node[12 + k]);
        b.lo[k] = corner(p[k], node[32 + 16 * k + s], scale);
        b.hi[k] = corner(p[k], node[32 + 16 * k + 8 + s], scale);
    }
    return b;
}

// half the surface area of a box, in double from the fp32 corners
CRT_HD double half_area(const rf::Box& b) {
    const double dx = (double)b.hi[0] - (double)b.lo[0], dy = (double)b.hi[1] - (double)b.lo[1], dz = (double)b.hi[2] - (double)b.lo[2];
    return (dx * dy + dy * dz) + dz * dx;
}

CRT_HD double finish(double root_area, double inner_area, double leaf_area) {
    if (root_area == 0.0) return 0.0;
    return (kNodeStep * (root_area + inner_area) + kTriangleTest * leaf_area) / root_area;
}

}  // namespace tc
}  // namespace crt
