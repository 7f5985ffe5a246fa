// The per-node pieces of a refit (crt_update_vertices): new boxes for an unchanged topology.  Compiled for the host refits
// (host/refit.cpp, g++) and for the device refit (refit.hip, gfx950), so that both produce the same bytes.  Every box is a
// min / max of input coordinates, and the node8 re-encoding is cwbvh_core.hpp's pick_exponent / quant_lo / quant_hi: nothing
// rounds except what those already do, identically on both sides.
#pragma once
#include <stdint.h>

#include "../../../include/crt.h"
#include "cwbvh_core.hpp"

namespace crt {
namespace rf {

// min / max in a total order of the finite floats (-0 below +0): the result does not depend on the order of the operands,
// so a lane-parallel reduction gives the bits a sequential loop gives
CRT_HD float tmin(float a, float b) { return a < b ? a : b < a ? b : (cw::f2u(a) >> 31) ? a : b; }
CRT_HD float tmax(float a, float b) { return a > b ? a : b > a ? b : (cw::f2u(a) >> 31) ? b : a; }

// ordered key of a finite float: unsigned compare of keys == float compare (-0 below +0, as tmin / tmax); the device checks reduce
// their bounds as keys, and key_to_float gives the float back
CRT_HD uint32_t order_key(float f) {
    const uint32_t b = cw::f2u(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
CRT_HD float key_to_float(uint32_t key) { return cw::u2f((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

constexpr float kEmpty = 3.4028235e38f;   // lo of an empty box (hi = -kEmpty): neutral under tmin / tmax of finite values

struct Box { float lo[3], hi[3]; };
CRT_HD Box empty_box() { return Box{{kEmpty, kEmpty, kEmpty}, {-kEmpty, -kEmpty, -kEmpty}}; }
CRT_HD void grow(Box& b, const Box& o) {
    for (int k = 0; k < 3; ++k) { b.lo[k] = tmin(b.lo[k], o.lo[k]); b.hi[k] = tmax(b.hi[k], o.hi[k]); }
}
// the full vertex box of a triangle (v[0..2] index `verts`, xyz each): spatial-split duplicates get it too, not a clipped one
CRT_HD void grow_triangle(Box& b, const int32_t v[3], const float* verts) {
    for (int j = 0; j < 3; ++j) {
        const float* p = verts + 3 * (size_t)(uint32_t)v[j];
        for (int k = 0; k < 3; ++k) { b.lo[k] = tmin(b.lo[k], p[k]); b.hi[k] = tmax(b.hi[k], p[k]); }
    }
}

// inner slot `slot` of a node8 -> its child node8 (the walk's child_base_index + rank among the inner slots)
CRT_HD uint32_t inner_child(const crt_node8& n, int slot) {
    return n.child_base_index + (uint32_t)__builtin_popcount((uint32_t)n.imask & ((1u << slot) - 1u));
}
// leaf slot: number of triangles (unary bits 7..5) and their offset from triangle_base_index (bits 4..0)
CRT_HD int leaf_count(uint8_t meta) { return __builtin_popcount((uint32_t)(meta >> 5)); }
CRT_HD int leaf_offset(uint8_t meta) { return meta & 31; }

// origin and exponents of a node8 from the union of its slot boxes (what encode_node takes from the BVH2 node's box)
CRT_HD void node_frame(const Box& u, float p[3], uint8_t e[3], float scale[3]) {
    for (int k = 0; k < 3; ++k) {
        p[k] = u.lo[k];
        e[k] = cw::pick_exponent(u.lo[k], u.hi[k]);
        scale[k] = cw::u2f((uint32_t)e[k] << 23);
    }
}
// the six quantised planes of one occupied slot: (lo x, hi x, lo y, hi y, lo z, hi z)
CRT_HD void quantise_slot(const Box& b, const float p[3], const float scale[3], uint8_t q[6]) {
    for (int k = 0; k < 3; ++k) {
        q[2 * k] = cw::quant_lo(b.lo[k], p[k], scale[k]);
        q[2 * k + 1] = cw::quant_hi(b.hi[k], p[k], scale[k]);
    }
}

}  // namespace rf
}  // namespace crt
